"""MODEL.ACT_CHECKPOINT on the TimeSformer encoder engine (pytest -m gpu).

No training kernel uses atomics, so a block recomputed from its saved input reproduces its activations bit for bit: every comparison
with the unchanged path below is `torch.equal` -- features and the flat gradient buffer -- on each path of the engine (divided with the
three pruning settings, the T = 8 temporal kernel, streamed spatial attention, the undivided schemes, ViT-L, the fp32 residual stream,
decoded uint8 input), under accumulation into existing gradients, with a gradient hook installed, from HIP graphs, and once against the
unmodified reference (tests/golden/divided_large.pt).  What the forward keeps is counted exactly (`EncoderEngine.saved_nbytes`), and the
allocator's peak is held to a bound derived from that count.  "Step": forward_features(x), then (feat * dfeat).sum().backward().

On the commit before this one the engine has no `act_checkpoint` and no `saved_nbytes`: the accounting test fails there."""
import numpy as np
import pytest
import torch

import e2e_checks as ec
from oracle import timesformer_oracle as orc
from test_divided_large_gpu import _droppath, _inputs, _model as _golden_model

DEV = ec.DEV
BASE, LARGE = "vit_base_patch16_224_develop", "vit_large_patch16_224_develop"


def _model(depth, crop, T, scheme="divided_space_time", name=BASE, drop_path=0.1, seed=11):
    """as tests/test_divided_large_gpu.py::_model builds it: ec.make_cfg, seeded state (temporal_fc is not zero)"""
    from procedurevrl_amd.build import build_model
    cfg = ec.make_cfg(depth, crop, 16, drop_path=drop_path, frames=T)
    cfg.MODEL.MODEL_NAME = name
    cfg.TIMESFORMER.ATTENTION_TYPE = scheme
    cfg.DEV.TEST_LANG_EMB = torch.randn(16, 512)
    cfg.TRAIN.LABEL_EMB = ""
    model = build_model(cfg, gpu_id=torch.device(DEV).index or 0)
    sd = orc.seeded_state({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed)
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).train()
    eng = model.model.engine
    assert eng.act_checkpoint is False and eng.undivided == (scheme != "divided_space_time")
    return model


def _data(B, T, crop, C=768, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, T, crop, crop, generator=g).to(DEV), torch.randn(B, C, generator=g).to(DEV)


def _step(model, x, dfeat, flag, seed=1234, zero=True, droppath=None):
    """one step with MODEL.ACT_CHECKPOINT = flag and the DropPath draws of `seed` -> (features, a copy of the flat gradient buffer)"""
    model.model.engine.act_checkpoint = flag
    if zero:
        model.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    feat = model.model.forward_features(x, droppath=droppath)
    (feat * dfeat).sum().backward()
    return feat.detach().clone(), model.model.adopt_grads().flat.clone()


def _same(a, b, what=""):
    (fa, ga), (fb, gb) = a, b
    assert torch.isfinite(fa).all() and torch.isfinite(ga).all(), what
    assert float(ga.abs().sum()) > 0.0
    nf, ng = int((fa != fb).sum()), int((ga != gb).sum())
    print(f"[{what}] differing features {nf} of {fa.numel()}, differing gradient elements {ng} of {ga.numel()}")
    assert torch.equal(fa, fb) and torch.equal(ga, gb), what


# (depth, B, T, crop, scheme, model, (prune_last, prune_attn) or None, resid16)
PATHS = {
    "divided-pruned": (3, 2, 2, 64, "divided_space_time", BASE, (True, True), True),
    "divided-attn_all_queries": (3, 2, 2, 64, "divided_space_time", BASE, (True, False), True),
    "divided-unpruned": (3, 2, 2, 64, "divided_space_time", BASE, (False, False), True),
    "divided-t8": (3, 2, 8, 32, "divided_space_time", BASE, None, True),                 # attn_t8: no lse_t
    "divided-streamed-s442": (3, 1, 2, 336, "divided_space_time", BASE, None, True),     # 442 tokens per frame
    "space_only": (3, 2, 2, 64, "space_only", BASE, None, True),
    "joint_space_time": (3, 2, 2, 64, "joint_space_time", BASE, None, True),
    "vit_large": (2, 2, 2, 64, "divided_space_time", LARGE, None, True),
    "divided-resid_f32": (3, 2, 2, 64, "divided_space_time", BASE, None, False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_step_is_bit_equal_to_the_unchanged_path(path):
    depth, B, T, crop, scheme, name, prune, resid16 = PATHS[path]
    model = _model(depth, crop, T, scheme, name)
    eng = model.model.engine
    eng.use_graphs = False
    if prune is not None:
        eng.prune_last, eng.prune_attn = prune
    eng.resid16 = resid16
    x, dfeat = _data(B, T, crop, eng.C)
    off = _step(model, x, dfeat, False)
    assert eng.saved is None
    on = _step(model, x, dfeat, True)
    assert eng.saved is None
    _same(off, on, path)
    if path == "divided-t8":
        eng.act_checkpoint = False
        model.model.forward_features(x)
        assert eng.saved["blocks"][0]["lse_t"] is None
        eng.saved = None


@pytest.mark.gpu
def test_decoded_uint8_clips_train_bit_equal():
    from procedurevrl_amd.transform import DecodedClips, spatial_sampling_params
    B, T, crop, H0, W0 = 2, 2, 64, 90, 120
    model = _model(3, crop, T)
    model.model.engine.use_graphs = False
    fr = torch.randint(0, 256, (B, T, H0, W0, 3), generator=torch.Generator().manual_seed(33), dtype=torch.uint8).to(DEV)
    np.random.seed(5)
    prms = [spatial_sampling_params(H0, W0, -1, 70, 85, crop) for _ in range(B)]
    cfg = model.model.cfg
    clips = lambda: DecodedClips(fr, prms, cfg.DATA.MEAN, cfg.DATA.STD, crop)
    _, dfeat = _data(B, T, crop)
    _same(_step(model, clips(), dfeat, False), _step(model, clips(), dfeat, True), "DecodedClips")


@pytest.mark.gpu
def test_accumulation_into_existing_gradients_is_bit_equal():
    """two steps without zero_grad: the second runs the beta = 1 launches"""
    model = _model(3, 64, 2)
    model.model.engine.use_graphs = False
    x, dfeat = _data(2, 2, 64)
    x2, dfeat2 = _data(2, 2, 64, seed=6)
    res = []
    for flag in (False, True):
        _step(model, x, dfeat, flag, seed=1)
        res.append(_step(model, x2, dfeat2, flag, seed=2, zero=False))
    _same(res[0], res[1], "two accumulated steps")
    one = _step(model, x2, dfeat2, False, seed=2)
    assert not torch.equal(one[1], res[0][1])             # (the second step did accumulate)


@pytest.mark.gpu
@pytest.mark.parametrize("tail_split", [True, False], ids=["tail_per_block", "tail_grouped"])
def test_gradient_hook_order_and_finality(tail_split):
    """the recompute runs inside _bwd_block: the hook is called for the same blocks in the same order, and a block's gradients are final
    when its hook runs.  Depth 4, hook_group 3: block 3 alone, then blocks 2, 1, 0 -- as ONE group without the tail split."""
    model = _model(4, 64, 2)
    eng = model.model.engine
    eng.use_graphs = False
    eng.hook_group, eng.hook_tail_split = 3, tail_split
    assert eng._group_of(1, 4) == ((1, 1) if tail_split else (0, 2))
    x, dfeat = _data(2, 2, 64)
    gs = model.model.grad_store()
    spans = {}
    for k, n in enumerate(gs.names):
        if n.startswith("blocks."):
            i = int(n.split(".")[1])
            a, b = gs.span(k)
            spans[i] = (min(a, spans[i][0]), max(b, spans[i][1])) if i in spans else (a, b)
    assert sorted(spans) == [0, 1, 2, 3]
    runs = {}
    for flag in (False, True):
        calls = []
        eng.grad_hook = lambda i: calls.append((i, gs.flat[spans[i][0]:spans[i][1]].clone()))
        try:
            feat, flat = _step(model, x, dfeat, flag)
        finally:
            eng.grad_hook = None
        for i, g in calls:
            assert torch.equal(g, flat[spans[i][0]:spans[i][1]]), f"block {i}: the gradients changed after its hook (flag {flag})"
            assert float(g.abs().sum()) > 0.0
        runs[flag] = ([i for i, _ in calls], feat, flat)
    assert runs[True][0] == runs[False][0] == [3, 2, 1, 0]
    _same(runs[False][1:], runs[True][1:], "hooked backward")


@pytest.mark.gpu
def test_the_reference_case_with_pinned_draws_under_checkpointing():
    """tests/test_divided_large_gpu.py's assertion on div_s442_t3_droppath (depth 2: block 0 checkpointed, pinned DropPath draws)"""
    f = ec.load("divided_large")["div_s442_t3_droppath"]
    model = _golden_model(f).train()
    eng = model.model.engine
    eng.act_checkpoint = True
    x, dfeat = _inputs(f)
    N = (f["crop"] // 16) ** 2
    feat = model.model.forward_features(x.to(DEV), droppath=_droppath(f, N))
    assert eng.saved["blocks"][0].get("ckpt") and not eng.saved["blocks"][1].get("ckpt")
    (feat * dfeat.to(DEV)).sum().backward()
    named = dict(model.named_parameters())
    res = [("features vs reference", ec.rel(feat, f["feat"]), ec.TOL_ACT)]
    res += [(f"grad {k[6:]}", ec.rel(named[k].grad, g), ec.TOL_GRAD) for k, g in f["grads"].items()]
    if "pos_embed_grad_rows" in f:
        res.append((f"grad pos_embed, every {f['pos_row_step']}th token row",
                    ec.rel(named["model.pos_embed"].grad[:, ::f["pos_row_step"]], f["pos_embed_grad_rows"]), ec.TOL_GRAD))
    worst, wk = 0.0, ""
    for k, s in f["grad_sums"].items():
        assert named[k].grad is not None, k
        e = abs(float(named[k].grad.double().abs().sum()) - s) / max(s, 1e-30)
        if e > worst:
            worst, wk = e, k
    res.append((f"worst sum |grad| over all {len(f['grad_sums'])} parameters ({wk})", worst, ec.TOL_GSUM))
    for label, e, tol in res:
        print(f"[div_s442_t3_droppath, checkpointed] {label}: err={e:.3e} tol={tol:g}")
    assert sorted(k for k, p in named.items() if p.grad is None) == f["no_grad"]
    bad = [(label, e, tol) for label, e, tol in res if not e <= tol]
    assert not bad, bad


@pytest.mark.gpu
def test_hip_graph_replay_with_and_without_the_flag():
    model = _model(3, 64, 2)
    eng = model.model.engine
    assert eng.use_graphs
    x, dfeat = _data(2, 2, 64)
    out = [_step(model, x, dfeat, True) for _ in range(eng.GRAPH_WARMUP + 3)]
    assert eng.use_graphs and len(eng._graphs) == 1, "the checkpointed step was not captured"
    assert all(g.get("bwd") is not None for g in eng._graphs.values())
    _same(out[-2], out[-1], "two replays")
    _same(out[0], out[-1], "eager step against a replay")
    out_off = [_step(model, x, dfeat, False) for _ in range(eng.GRAPH_WARMUP + 2)]
    assert eng.use_graphs and len(eng._graphs) == 2, "the flag is not part of the graph key"
    assert all(g.get("bwd") is not None for g in eng._graphs.values())
    _same(out[-1], out_off[-1], "replay without the flag against the replay with it")
    _same(out_off[0], out_off[-1], "eager step against a replay, flag off")
    eng.release_graphs()
    assert len(eng._graphs) == 0


# ---------------------------------------------------------------------------------------------------------------------
# what is kept
# ---------------------------------------------------------------------------------------------------------------------
ACC = dict(depth=4, B=2, T=2, crop=224)


@pytest.fixture(scope="module")
def acc_model():
    model = _model(ACC["depth"], ACC["crop"], ACC["T"])
    model.model.engine.use_graphs = False
    return model, _data(ACC["B"], ACC["T"], ACC["crop"])


def _tensors(obj, out=None):
    from procedurevrl_amd.engine import _X
    out = [] if out is None else out
    if isinstance(obj, torch.Tensor):
        out.append(obj)
    elif isinstance(obj, _X):
        _tensors((obj.p, obj.c, obj.full), out)
    elif isinstance(obj, dict):
        _tensors(list(obj.values()), out)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _tensors(v, out)
    return out


def _accounting(model, x, flag):
    """a training forward -> (saved_nbytes() - rest, the saved dict); rest = the last block's entry + a_pe + x_final + the norm statistics"""
    from procedurevrl_amd.engine import storage_nbytes
    eng = model.model.engine
    eng.act_checkpoint = flag
    torch.manual_seed(3)
    model.model.forward_features(x)
    sv = eng.saved
    rest = storage_nbytes([sv["blocks"][-1], sv["a_pe"], sv["x_final"], sv["norm_stats"]])
    kept = eng.saved_nbytes() - rest
    eng.saved = None
    return kept, sv


@pytest.mark.gpu
def test_what_a_checkpointed_forward_keeps(acc_model):
    model, (x, _) = acc_model
    eng = model.model.engine
    B, T, C = ACC["B"], ACC["T"], eng.C
    R = B * (ACC["crop"] // 16) ** 2 * T
    assert R == 784 and eng.resid16
    kept_on, sv = _accounting(model, x, True)
    assert len(sv["blocks"]) == 4 and not sv["blocks"][-1].get("ckpt")
    for s in sv["blocks"][:-1]:
        own = {t.untyped_storage().data_ptr() for t in _tensors([s["x0"], s["dp"]])}
        assert all(t.untyped_storage().data_ptr() in own for t in _tensors(s)), sorted(s)
        assert s["x0"].p.shape == (R, C) and s["x0"].c.shape == (B, C)
    stage = R * C * 2 + B * C * 4
    # (one block's DropPath vectors by their own sizes: the blocks' vectors are rows of shared [depth, .] tensors)
    dpb = max(sum(t.numel() * t.element_size() for t in _tensors(s["dp"])) for s in sv["blocks"])
    print(f"checkpointed: kept beyond the last block {kept_on} B; stage {stage} B, DropPath vectors {dpb} B")
    assert 0 < kept_on <= 3 * (stage + dpb)
    del sv
    kept_off, sv = _accounting(model, x, False)
    del sv
    print(f"plain: kept beyond the last block {kept_off} B = {kept_off / (3 * R * C * 2):.2f} token-matrix widths per block")
    assert kept_off >= 3 * 20 * R * C * 2


@pytest.mark.gpu
def test_peak_allocated_memory_falls_by_two_blocks_of_three(acc_model):
    """The accounting difference d covers three blocks; while a checkpointed block is back-propagated ONE recomputed entry is alive next
    to the saved inputs, and the allocator rounds the small statistics tensors to 512 B: the bound asks for two thirds of d.
    Measured: plain 119.9 MB, checkpointed 61.4 MB above the resident bytes, a drop of 0.767 d (d = 76.3 MB).  The plain peak is in the
    last block's backward, the checkpointed one in the first recomputed block's (three stages, one entry, its backward buffers).  While
    the deferred LayerNorm partial sums and dW_e buffers were kept to the end of the backward in this mode too, they moved its peak to
    block 0 (82.2 MB, 0.494 d: these buffers do not shrink with the rows); the engine now finishes them per block (_bwd_block)."""
    model, (x, dfeat) = acc_model
    d = _accounting(model, x, False)[0] - _accounting(model, x, True)[0]
    assert d > 0
    eng = model.model.engine

    def step():         # (no copies of the results: the flat gradient buffer is larger than a block's activations at this size)
        model.zero_grad(set_to_none=True)
        torch.manual_seed(3)
        feat = model.model.forward_features(x)
        (feat * dfeat).sum().backward()

    peak = {}
    for flag in (False, True):
        eng.act_checkpoint = flag
        step()                                              # workspaces, weight copies
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        peak[flag] = torch.cuda.max_memory_allocated() - base
    drop = peak[False] - peak[True]
    print(f"peak above the resident bytes: plain {peak[False]} B, checkpointed {peak[True]} B; drop {drop} B = {drop / d:.3f} of the "
          f"accounting difference {d} B")
    assert drop >= (2.0 / 3.0) * d


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["divided_space_time", "joint_space_time"])
def test_a_forward_that_keeps_nothing_has_the_same_features(scheme):
    """engine.forward(save=False) -- what a frozen encoder (TRAIN.LINEAR) runs -- takes fc1 with PVRL_EPI_GELU_ONLY, save=True with
    PVRL_EPI_GELU: train mode, drop_path 0, the same features bit for bit"""
    model = _model(3, 64, 2, scheme, drop_path=0.0)
    eng = model.model.engine
    eng.use_graphs = False
    x, _ = _data(2, 2, 64)
    with torch.no_grad():
        kept_nothing = eng.forward(x, training=True, save=False)
        assert eng.saved is None
        saving = eng.forward(x, training=True, save=True)
    assert eng.saved is not None and eng.saved["blocks"][0]["u"] is not None
    eng.saved = None
    assert torch.isfinite(saving).all() and float(saving.abs().sum()) > 0.0 and torch.equal(kept_nothing, saving)
