"""VisionTransformer.forward_features(x, cls=False) -- the encoder's normalised output of EVERY token -- through the HIP engine against the
UNMODIFIED reference (tests/golden/tokens*.pt, tests/golden/make_golden_tokens.py), with the bars of e2e_checks (they switch with
PVRL_OPERAND).  (pytest -m gpu)

Row 0 (cls) is held to ec.TOL_ACT and, in eval mode, is bit-equal to forward_features(x) of a model built with PVRL_PRUNE_LAST=0 on the
same weights: the same launches feed that row.

The PATCH rows come out of the 16-bit residual stream, so their error is not the cls rows': it is priced by the all-token forward
composed from oracle/rounded_oracle.py's pieces (tokens_checks.oracle_tokens) -- (a) the project's ratio test, HIP error <= ec.TOL_RATIO x
that oracle's error against the same fixture, and (b) an absolute bar of 1.5 x that oracle's error, computed on the CPU per case and
kept as constants (tokens_checks.ORACLE_PATCH_ERR, re-derived by tests/test_tokens_host.py):
                    tok_div   tok_div_train  tok_stream  tok_joint  tok_space  tok_large
    oracle, fp16    7.02e-4   6.60e-4        7.06e-4     6.31e-4    5.37e-4    7.48e-4       bar = 1.5 x
    oracle, bf16    5.62e-3   5.29e-3        5.64e-3     5.01e-3    4.27e-3    5.99e-3
    MI355X, fp16    7.06e-4   6.57e-4        7.05e-4     6.33e-4    5.40e-4    7.45e-4       observed (ratio 0.995 .. 1.013)
    MI355X, bf16    5.64e-3   5.28e-3        5.63e-3     5.03e-3    4.25e-3    5.99e-3       observed (ratio 0.997 .. 1.002)
Gradients of the loss sum(tokens * dtok): the fixture's KEEP tensors to ec.TOL_GRAD, the worst sum |grad| over all parameters to
ec.TOL_GSUM, and the same parameters without a gradient (the head)."""
import os

import pytest
import torch

import e2e_checks as ec
import tokens_checks as tc

DEV = ec.DEV


@pytest.fixture(scope="module")
def gold():
    return tc.load()


@pytest.fixture(scope="module")
def oracle_err(gold):
    """the composed rounded oracle's patch-row error per case, computed once on the CPU for the library's operand type"""
    out = {}
    for name in tc.CASES:
        f = gold[name]
        _, sd = tc.make_model(f)
        out[name] = tc.patch_err(f, tc.oracle_tokens(f, sd, tc.inputs(f)[0], ec.OPERAND_DTYPE))
    return out


def _model(f, **kw):
    return tc.make_model(f, **kw)[0].to(DEV)


def _droppath(f):
    """the reference's captured torch.rand draws of block 1's three DropPath calls (block 0's rate is 0) -> forward_features(droppath=...)"""
    if not f["draws"]:
        return None
    from procedurevrl_amd.engine import EncoderEngine
    keep = 1.0 - f["drop_path"]
    s1, s2, s3 = (torch.floor(keep + u.float()) / keep for u in f["draws"])
    return [None, EncoderEngine.expand_droppath(s1.to(DEV), s2.to(DEV), s3.to(DEV), f["B"], (f["crop"] // 16) ** 2, f["T"])]


def _step(model, x, dtok, droppath=None):
    model.zero_grad(set_to_none=True)
    tok = model.model.forward_features(x, cls=False, droppath=droppath)
    (tok * dtok).sum().backward()
    return tok.detach().clone(), model.model.adopt_grads().flat.clone()


@pytest.mark.gpu
@pytest.mark.parametrize("name", tc.CASES)
def test_tokens_and_gradients_match_the_reference(gold, oracle_err, name):
    f = gold[name]
    model = _model(f).train(f["train"])
    model.model.grad_store()
    x, dtok = tc.inputs(f)
    tok = model.model.forward_features(x.to(DEV), cls=False, droppath=_droppath(f))
    assert tok.dtype == torch.float32 and tuple(tok.shape) == (f["B"], tc.n_tokens(f), f["width"])
    (tok * dtok.to(DEV)).sum().backward()
    named = dict(model.named_parameters())
    e_patch, e_model = tc.patch_err(f, tok), oracle_err[name]
    res = [("row 0 (cls) vs reference", ec.rel(tok[:, 0], f["tok"][:, 0]), ec.TOL_ACT),
           (f"patch rows: error / rounded oracle's ({e_patch:.3e} / {e_model:.3e})", e_patch / e_model, ec.TOL_RATIO),
           ("patch rows vs reference, absolute", e_patch, tc.patch_bar(name))]
    for k, g in f["grads"].items():
        got = named[k].grad
        if name == "tok_stream" and k == "model.pos_embed":
            got = got[:, list(range(0, got.shape[1], 8))]
        res.append((f"grad {k[6:]}", ec.rel(got, g), ec.TOL_GRAD))
    worst, wk = 0.0, ""
    for k, s in f["grad_sums"].items():
        assert named[k].grad is not None, k
        e = abs(float(named[k].grad.double().abs().sum()) - s) / max(s, 1e-30)
        if e > worst:
            worst, wk = e, k
    res.append((f"worst sum |grad| over all {len(f['grad_sums'])} parameters ({wk})", worst, ec.TOL_GSUM))
    for label, e, tol in res:
        print(f"[{name}] {label}: err={e:.3e} tol={tol:g}")
    assert sorted(k for k, p in named.items() if p.grad is None) == f["no_grad"]
    bad = [r for r in res if not r[1] <= r[2]]
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tok_div", "tok_stream", "tok_joint", "tok_space", "tok_large"])
def test_row_0_is_bit_equal_to_the_unpruned_cls_features(gold, name, monkeypatch):
    f = gold[name]
    x = tc.inputs(f)[0].to(DEV)
    model = _model(f).eval()
    with torch.no_grad():
        tok = model.model.forward_features(x, cls=False)
    monkeypatch.setenv("PVRL_PRUNE_LAST", "0")
    unpruned = _model(f).eval()
    assert not unpruned.model.engine.prune_last
    with torch.no_grad():
        feat = unpruned.model.forward_features(x)
    assert torch.equal(tok[:, 0], feat)
    assert ec.rel(feat, f["feat"]) <= ec.TOL_ACT


@pytest.mark.gpu
def test_graph_replay_is_bit_equal_and_keeps_the_two_outputs_apart(gold):
    f = gold["tok_div"]
    x, dtok = (t.to(DEV) for t in tc.inputs(f))
    dfeat = dtok[:, 0].contiguous()

    def cls_step(model):
        model.zero_grad(set_to_none=True)
        feat = model.model.forward_features(x)
        (feat * dfeat).sum().backward()
        return feat.detach().clone(), model.model.adopt_grads().flat.clone()

    model = _model(f, drop_path=0.0).train()
    eng = model.model.engine
    assert eng.use_graphs
    toks, clss = [], []
    for i in range(eng.GRAPH_WARMUP + 3):           # cls before tokens and after: each output warms up, is captured and replayed
        clss.append(cls_step(model))
        toks.append(_step(model, x, dtok))
    assert len(eng._graphs) == 2 and all("bwd" in g for g in eng._graphs.values()), "the two steps were not both captured"
    for out in (toks, clss):
        assert all(torch.isfinite(t).all() for t in out[-1])
        assert torch.equal(out[-1][0], out[-2][0]) and torch.equal(out[-1][1], out[-2][1])          # two replays
        assert torch.equal(out[0][0], out[-1][0]) and torch.equal(out[0][1], out[-1][1]), "replay differs from the eager launches"
    assert tuple(toks[-1][0].shape) == (2, 33, 768) and tuple(clss[-1][0].shape) == (2, 768)
    # against eager launches of models that never captured anything
    old = os.environ.get("PVRL_HIP_GRAPHS")
    os.environ["PVRL_HIP_GRAPHS"] = "0"
    try:
        fresh_tok, fresh_cls = _model(f, drop_path=0.0).train(), _model(f, drop_path=0.0).train()
    finally:
        if old is None:
            del os.environ["PVRL_HIP_GRAPHS"]
        else:
            os.environ["PVRL_HIP_GRAPHS"] = old
    assert not fresh_tok.model.engine.use_graphs
    t, g = _step(fresh_tok, x, dtok)
    assert torch.equal(t, toks[-1][0]) and torch.equal(g, toks[-1][1])
    c, g = cls_step(fresh_cls)
    assert torch.equal(c, clss[-1][0]) and torch.equal(g, clss[-1][1])
    assert ec.rel(toks[-1][0][:, 0], f["tok"][:, 0]) <= ec.TOL_ACT


@pytest.mark.gpu
def test_activation_checkpointing_is_bit_equal_to_the_plain_path(gold):
    f = gold["tok_div_train"]
    x, dtok = (t.to(DEV) for t in tc.inputs(f))
    out = []
    for ckpt in (False, True):
        model = _model(f, act_checkpoint=ckpt).train()
        assert model.model.engine.act_checkpoint == ckpt
        out.append(_step(model, x, dtok, droppath=_droppath(f)))
    assert torch.isfinite(out[1][0]).all() and torch.isfinite(out[1][1]).all()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tok_div", "tok_space"])
def test_a_forward_that_keeps_nothing_gives_the_same_tokens(gold, name):
    f = gold[name]
    x = tc.inputs(f)[0].to(DEV)
    model = _model(f).eval()
    eng = model.model.engine
    model.model.grad_store()
    kept = eng.forward(x, training=False, save=True, tokens=True).clone()
    assert eng.saved is not None and eng.saved.get("tokens")
    eng.saved = None
    free = eng.forward(x, training=False, save=False, tokens=True)
    assert eng.saved is None
    assert torch.equal(kept, free)
    assert ec.rel(free[:, 0], f["tok"][:, 0]) <= ec.TOL_ACT


@pytest.mark.gpu
def test_decoded_clips_give_the_tokens_of_the_same_clips_in_fp32(gold):
    import numpy as np
    from procedurevrl_amd import ops
    from procedurevrl_amd.transform import DecodedClips, spatial_sampling_params
    f = gold["tok_div"]
    model = _model(f).eval()
    cfg = model.model.cfg
    g = torch.Generator().manual_seed(23)
    B, T, H0, W0, crop = f["B"], f["T"], 40, 56, f["crop"]
    fr = torch.randint(0, 256, (B, T, H0, W0, 3), generator=g, dtype=torch.uint8)
    np.random.seed(5)
    prms = [spatial_sampling_params(H0, W0, -1, 36, 48, crop) for _ in range(B)]
    clips = lambda: DecodedClips(fr.to(DEV), prms, cfg.DATA.MEAN, cfg.DATA.STD, crop)
    with torch.no_grad():
        tok_u8 = model.model.forward_features(clips(), cls=False)
        tok_f32 = model.model.forward_features(ops.frames_u8_to_f32(clips()), cls=False)
    assert tuple(tok_u8.shape) == (B, tc.n_tokens(f), f["width"]) and torch.isfinite(tok_u8).all()
    assert torch.equal(tok_u8, tok_f32)
