"""forward_features(x, cls=False) without a GPU: the fixtures tests/golden/tokens*.pt (the UNMODIFIED reference's all-token output,
tests/golden/make_golden_tokens.py) and the all-token forward composed from oracle/rounded_oracle.py's pieces (tests/tokens_checks.py)
that tests/test_tokens_gpu.py prices the HIP path's patch rows with."""
import pytest
import torch

import e2e_checks as ec
import tokens_checks as tc

SHAPES = dict(tok_div=(2, 33, 768), tok_div_train=(4, 33, 768), tok_stream=(2, 883, 768), tok_joint=(2, 33, 768), tok_space=(2, 5, 768),
              tok_large=(2, 33, 1024))


@pytest.fixture(scope="module")
def gold():
    return tc.load()


def test_the_cases_and_their_shapes(gold):
    assert sorted(gold) == sorted(tc.CASES)
    for name, f in gold.items():
        B, S, C = SHAPES[name]
        assert (f["B"], tc.n_tokens(f), f["width"]) == (B, S, C)
        stored = S if f["rows"] is None else len(f["rows"])
        assert tuple(f["tok"].shape) == (B, stored, C) and f["tok"].dtype == torch.float32
        x, dtok = tc.inputs(f)
        assert tuple(dtok.shape) == (B, S, C) and tuple(x.shape) == (B, 3, f["T"], f["crop"], f["crop"])
        assert f["depth"] == 2 and len(f["draws"]) == (3 if f["drop_path"] else 0)
    assert gold["tok_stream"]["rows"] == list(range(0, 883, 8))       # S = 442 per frame: the streamed attention
    assert tuple(gold["tok_stream"]["grads"]["model.pos_embed"].shape) == (1, len(range(0, 442, 8)), 768)
    assert gold["tok_div_train"]["train"] and gold["tok_div_train"]["drop_path"] == 0.5


@pytest.mark.parametrize("name", tc.CASES)
def test_row_0_is_the_cls_feature_and_only_the_head_is_without_a_gradient(gold, name):
    f = gold[name]
    assert tuple(f["feat"].shape) == (f["B"], f["width"])
    assert torch.equal(f["tok"][:, 0], f["feat"]), "row 0 is not forward_features(x) of the same seeded model"
    assert f["no_grad"] == ["model.head.bias", "model.head.weight"]
    assert all(k in f["grad_sums"] for k in f["grads"]) and all(torch.isfinite(g).all() for g in f["grads"].values())


@pytest.mark.parametrize("name", tc.CASES)
def test_the_composed_oracle_reproduces_the_fixture_within_its_own_rounding(gold, name):
    """without rounding the composed forward IS the reference's arithmetic (fp32 re-association at the most); with the HIP datapath's
    rounding points its patch-row error is the constant tokens_checks.ORACLE_PATCH_ERR holds for the case (CPU thread counts move a
    rounding-chaotic error by a few per cent: held to 20 %), which is what the GPU test's absolute bar is 1.5 x of."""
    f = gold[name]
    model, sd = tc.make_model(f)
    x, _ = tc.inputs(f)
    o32 = tc.oracle_tokens(f, sd, x)
    assert tuple(o32.shape) == SHAPES[name]
    e32 = ec.rel(tc.rows_of(f, o32), f["tok"])
    print(f"[{name}] composed oracle, fp32, all stored rows: err={e32:.3e}")
    assert e32 <= 1e-5
    for dtype, key in ((torch.float16, "f16"), (torch.bfloat16, "bf16")):
        o = tc.oracle_tokens(f, sd, x, dtype)
        e, want = tc.patch_err(f, o), tc.ORACLE_PATCH_ERR[key][name]
        e0 = ec.rel(tc.rows_of(f, o)[:, 0], f["tok"][:, 0])
        print(f"[{name}] composed oracle, {key}: patch rows err={e:.3e} (constant {want:.3e}), row 0 err={e0:.3e}")
        assert 0.8 * want <= e <= 1.2 * want
        assert e0 <= (1e-2 if key == "bf16" else 1e-3)          # e2e_checks.TOL_ACT of that flavour


def test_the_flag_is_part_of_the_graph_key_and_of_the_signatures(gold):
    import inspect
    from procedurevrl_amd.engine import EncoderEngine
    from procedurevrl_amd.functional import EncoderFn
    for fn in (EncoderEngine.forward, EncoderEngine._forward, EncoderEngine.backward, EncoderFn.forward):
        p = inspect.signature(fn).parameters["tokens"]
        assert p.default is False, fn
    model, _ = tc.make_model(gold["tok_div"])
    eng = model.model.engine
    x = torch.zeros(2, 3, 8, 32, 32)
    off = eng._graph_key(x, True, True)
    eng._tok = True
    on = eng._graph_key(x, True, True)
    eng._tok = False
    assert on != off and eng._graph_key(x, True, True) == off


def test_cpu_input_still_raises_the_hip_only_error(gold):
    model, _ = tc.make_model(gold["tok_div"])
    with pytest.raises(RuntimeError, match="HIP path only"):
        model.model.forward_features(torch.zeros(2, 3, 8, 32, 32), cls=False)
