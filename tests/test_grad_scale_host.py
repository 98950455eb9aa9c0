"""The CPU half of tests/grad_scale_checks.py (no GPU):
  * the rules that tests/test_grad_scale_gpu.py holds the engines to are themselves exact -- the S-scaled fp16 rounding model and the
    unscaled bf16 model (oracle/rounded_oracle.py fed S * g, gradients / S; and the toy engine) are bit-covariant under 2^k;
  * each planted defect of grad_scale_checks.DEFECTS fails its named case, and the healthy toy passes every case;
  * the fp32 reference has no zero-norm gradient in any regime beyond the ones the case table names (STRUCTURAL_ZEROS)."""
import pytest
import torch

import grad_scale_checks as gc
import tokens_checks as tc

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
KS = {"f16": (-24, -7, 7, 24), "bf16": (-7, 7)}


@pytest.fixture(scope="module")
def cls_inputs():
    return gc.cls_oracle_inputs()


@pytest.fixture(scope="module")
def gold():
    return tc.load()


@pytest.mark.parametrize("flavour", sorted(DTYPES))
def test_the_rounded_oracle_run_as_the_engine_runs_it_is_bit_covariant(cls_inputs, flavour):
    _, sd, x = cls_inputs
    g = gc.cls_gradient("randn", gc.CLS_GEOM["B"], 768) * 3e-5
    g0 = gc.cls_oracle_grads(sd, x, g, DTYPES[flavour])
    assert g0 and all(bool(torch.isfinite(v).all()) for v in g0.values())
    for k in KS[flavour]:
        bad = gc.mismatches(g0, gc.cls_oracle_grads(sd, x, g * 2.0 ** k, DTYPES[flavour]), k)
        assert not bad, (k, bad[:8])


def test_the_scale_formula_is_covariant_and_matches_the_torch_branch():
    g = gc.cls_gradient("randn", 4, 768) * 3e-5
    for k in (-24, -9, -7, 0, 7, 9, 24):
        assert gc.scale_of(g * 2.0 ** k) == gc.scale_of(g) * 2.0 ** -k == float(gc.model_scale(g * 2.0 ** k))
    assert gc.scale_of(g, scaled=False) == 1.0
    assert gc.scale_of(torch.zeros(3)) == 2.0 ** 100


@pytest.mark.parametrize("flavour", sorted(DTYPES))
@pytest.mark.parametrize("case", gc.TOY_CASES)
def test_the_healthy_toy_engine_passes_every_case(case, flavour):
    bad = gc.toy_case(case, DTYPES[flavour])
    assert not bad, bad


@pytest.mark.parametrize("defect", sorted(gc.DEFECTS))
def test_each_planted_defect_fails_its_named_case(defect):
    case, seen_before = gc.DEFECTS[defect]
    assert case in gc.TOY_CASES and seen_before
    bad = gc.toy_case(case, torch.float16, defect)
    assert bad, f"{defect} passed the case '{case}'"
    print(f"{defect}: fails '{case}' ({str(bad[0])[:120]}); seen by the suite before: {seen_before}")


def test_a_saturating_row_sum_copy_passes_a_finite_only_check():
    """why the headroom case bounds the value ENTERING the cast: the saturated copy gives finite, wrong gradients"""
    bad, grads, eng = gc.toy_headroom(torch.float16, "row_sum_copy_saturates")
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert bad and any("exceeds" in b for b in bad)
    # without its own power of two the healthy copy overflows loudly (the engine before this test existed) ...
    bad, grads, eng = gc.toy_headroom(torch.float16, None, rescale=False)
    assert eng.max_row_sum > gc.FP16_MAX and not bool(torch.isfinite(grads["W1_chain"]).all()) and bad
    # ... with it, it is exact (a power of two) and a no-op while the sum is small: bit-equal gradients at 64 rows
    bad, grads, eng = gc.toy_headroom(torch.float16, None)
    assert not bad and eng.max_row_sum > gc.FP16_MAX and eng.max_into_cast <= gc.ToyEngine.DWE_LIMIT
    a, b = gc.toy_headroom(torch.float16, None, rows=64), gc.toy_headroom(torch.float16, None, rows=64, rescale=False)
    assert not a[0] and not b[0] and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


def test_at_least_eight_defects_are_planted():
    assert len(gc.DEFECTS) >= 8 and {c for c, _ in gc.DEFECTS.values()} <= set(gc.TOY_CASES)


def _zero_norm(grads):
    return sorted(k for k, g in grads.items() if float(g.norm()) == 0.0)


@pytest.mark.parametrize("regime", gc.CLS_REGIMES)
def test_cls_regimes_have_no_unnamed_zero_gradient_in_the_reference(cls_inputs, regime):
    _, sd, x = cls_inputs
    g = gc.cls_gradient(regime, gc.CLS_GEOM["B"], 768)
    assert float(g.abs().max()) > 0
    assert _zero_norm(gc.cls_oracle_grads(sd, x, g)) == sorted(gc.STRUCTURAL_ZEROS.get(("cls", regime), ()))


@pytest.mark.parametrize("regime", gc.TOK_REGIMES)
@pytest.mark.parametrize("name", ["tok_div", "tok_space"])
def test_token_regimes_have_no_unnamed_zero_gradient_in_the_reference(gold, name, regime):
    f = gold[name]
    _, sd = tc.make_model(f, drop_path=0.0)
    g = gc.tok_gradient(regime, f["B"], tc.n_tokens(f), f["width"])
    assert float(g.abs().max()) > 0
    assert _zero_norm(gc.tok_oracle_grads(f, sd, tc.inputs(f)[0], g)) == sorted(gc.STRUCTURAL_ZEROS.get((name, regime), ()))


def test_the_regimes_are_what_their_names_say():
    B, S, C = 3, 17, 8
    g = {r: gc.tok_gradient(r, B, S, C) for r in gc.TOK_REGIMES}
    assert torch.equal(g["mean_pool"], g["mean_pool"][:, :1].expand(B, S, C)) and float(g["mean_pool"].abs().max()) > 0
    assert float(g["cls_only"][:, 1:].abs().max()) == 0 and float(g["cls_only"][:, 0].abs().min()) > 0
    assert float(g["patch_only"][:, 0].abs().max()) == 0 and float(g["patch_only"][:, 1:].abs().min()) > 0
    assert int((g["one_token"].abs().sum(-1) > 0).sum()) == 1
    frac = float((g["masked"].abs().sum(-1) > 0).float().mean())
    assert 0.05 < frac < 0.5
    ratio = float(g["outlier"][-1].abs().max() / g["outlier"][:-1].abs().max())
    assert 2.0 ** 8 < ratio < 2.0 ** 12
    assert float(gc.small_part("outlier", g["outlier"])[-1].abs().max()) == 0
    c = {r: gc.cls_gradient(r, 4, C) for r in gc.CLS_REGIMES}
    assert float(c["one_clip"][1:].abs().max()) == 0 and int((c["one_hot"] != 0).sum()) == 1
