"""Shared by tests/test_grad_scale_gpu.py and tests/test_grad_scale_host.py: the mechanism that makes the fp16-operand flavour's
backward work -- every engine runs its backward in S-scaled units, S a power of two picked on the device from max|incoming gradient|
(grads.GradStore.begin_scaled, SCALE_TARGET = 256), and un-scales every parameter gradient where it is written.  TEST INFRASTRUCTURE.

  1. covariance: a training step whose loss is multiplied by 2^k gives 2^k times the k = 0 gradients BIT FOR BIT (S is a power of two,
     the backward is linear in the gradient), eager, replayed from graphs captured at another k, accumulated across two k;
  2. the two branches of begin_scaled (one launch up to 2^20 elements, torch ops above) against optim_checks.gsb_allowed and each other;
  3. regimes of the incoming gradient (one clip, an outlier clip, one token, ...) against the fp32 oracle, priced by the rounded oracle
     whose backward is fed S * g with S from the same formula;
  4. the headroom below fp16's 65,504 of the S-scaled sums over rows that are rounded to 16 bits (ROW_SUM_SITES).

The CPU half (`ToyEngine`, `toy_case`, `DEFECTS`) restates the scaling rules on plain tensors: the host test shows the rules themselves are
bit-covariant and that each planted defect fails a named case."""
import math

import torch

import e2e_checks as ec

F32 = torch.float32
DEV = ec.DEV
SCALED = ec.OPERAND != "bf16"                  # the fp16-operand flavour scales; bf16 moves through fp32's exponent range directly
KS = (-24, -7, 7, 24) if SCALED else (-7, 7)
KS_REPLAY = (-9, 9)
SCALE_TARGET = 256.0
FP16_MAX = 65504.0
SEAM = 1 << 20                                 # begin_scaled: one launch up to here, torch ops above

# Every site where an S-scaled SUM OVER ROWS is rounded to the operand type (found by reading engine.py, mvit.py, head_engine.py,
# tfm_engine.py; every other 16-bit gradient operand is one row's value, bounded by the row it came from):
ROW_SUM_SITES = {
    "dW_e": "engine._temporal_chain_all: dW_e = dz^T o_t, a sum over all R patch rows, cast by cast_weights_multi for the two chain GEMMs "
            "(`dW_e_sum`: the sum itself; `dW_e`: what enters the cast, after the all-token backward's own power of two)",
    "dqkv_cls": "engine._block_bwd / _block_bwd_undivided: the cls rows of dqkv, group_reduce's sum over a clip's T frames, written 16-bit",
}
# (mvit.py, head_engine.py and tfm_engine.py round per-row values only: cast_scale of the gradient stream; their sums over rows --
#  weight gradients, bias sums, batch_sum -- stay fp32 until `gscale` / unscale() has taken S out.)


# ====================================================================================================== covariance (GPU)
def grads_of(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def mismatches(g0, gk, k):
    """-> [(name, elements that are not bit-equal to 2^k x the k = 0 gradient)]"""
    out = []
    if set(g0) != set(gk):
        out.append(("parameters with a gradient differ", sorted(set(g0) ^ set(gk))))
    f = 2.0 ** k
    for n in g0:
        if n in gk and not torch.equal(gk[n], g0[n] * f):
            out.append((n, int((gk[n] != g0[n] * f).sum())))
    return out


def assert_finite(grads):
    bad = [n for n, g in grads.items() if not bool(torch.isfinite(g).all())]
    assert not bad, f"non-finite gradients: {bad}"


def assert_covariant(case, ks=KS):
    """case = (model, step): step(k) runs one training step with the loss (or the fed gradient) multiplied by 2^k, .grad reset first"""
    model, step = case
    step(0)
    g0 = grads_of(model)
    assert g0 and any(float(g.abs().max()) > 0 for g in g0.values()), "no gradient at all"
    assert_finite(g0)
    for k in ks:
        step(k)
        bad = mismatches(g0, grads_of(model), k)
        assert not bad, f"k = {k}: not bit-equal to 2^k x the k = 0 gradient: {bad[:8]}"
    return g0


def _reinit_temporal_fc(vt):
    with torch.no_grad():
        for blk in vt.blocks:
            if hasattr(blk, "temporal_fc"):
                torch.nn.init.normal_(blk.temporal_fc.weight, std=0.02)


def encoder_case(crop=48, K=200, B=5, depth=2, frames=8, att="divided_space_time", prune=None, resid16=None, ckpt=False, large=False,
                 graphs=False, seed=4):
    """the step of e2e_checks.check_hip_graph_replay (model(x), top-5 KL loss: head parameters included)"""
    from procedurevrl_amd.datasets import synthetic_label_emb
    from procedurevrl_amd.functional import kl_topk_loss
    cfg = ec.make_cfg(depth, crop, K, drop_path=0.0, frames=frames)
    cfg.TIMESFORMER.ATTENTION_TYPE = att
    cfg.MODEL.ACT_CHECKPOINT = bool(ckpt)
    if large:
        cfg.MODEL.MODEL_NAME = "vit_large_patch16_224_develop"
    model = ec.build(cfg, synthetic_label_emb(K, 512, seed=1)).to(DEV).train()
    vt = model.model
    eng = vt.engine
    assert eng.act_checkpoint == bool(ckpt) and eng.C == (1024 if large else 768)
    _reinit_temporal_fc(vt)
    if prune is not None:
        eng.prune_last, eng.prune_attn = prune
    if resid16 is not None:
        eng.resid16 = resid16
    eng.use_graphs = graphs
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, frames, crop, crop, generator=g).to(DEV)
    teacher = (torch.randn(B, K, generator=g) * 3).to(DEV)

    def step(k, zero=True):
        if zero:
            model.zero_grad(set_to_none=True)
        (kl_topk_loss(model(x), teacher, 5) * 2.0 ** k).backward()

    return model, step


def token_case(f, graphs=False, dtok=None):
    """forward_features(cls=False) on a tokens_checks fixture's model, fed `dtok * 2^k` directly"""
    import tokens_checks as tc
    model = tc.make_model(f, drop_path=0.0)[0].to(DEV).train()
    _reinit_temporal_fc(model.model)
    model.model.engine.use_graphs = graphs
    x, d = tc.inputs(f)
    x, d = x.to(DEV), (d if dtok is None else dtok).to(DEV)

    def step(k, zero=True, d=d):
        if zero:
            model.zero_grad(set_to_none=True)
        model.model.forward_features(x, cls=False).backward(d * 2.0 ** k)

    return model, step


def mvit_case():
    """the small geometry of mvit_checks.check_mvit_hip_graph_replay"""
    import mvit_checks as mc
    from procedurevrl_amd.build import build_model
    from procedurevrl_amd.datasets import synthetic_label_emb
    from procedurevrl_amd.functional import kl_topk_loss
    g = mc._load("mvit_small")
    cfg = mc._mvit_cfg(g["mvit"], 4, 64, K=128)
    cfg.TRAIN.LABEL_EMB = synthetic_label_emb(128, 512, seed=1)
    torch.manual_seed(0)
    model = build_model(cfg, gpu_id=0).train()
    model.model.engine.use_graphs = False
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(3, 3, 4, 64, 64, generator=gen).to(DEV)
    teacher = (torch.randn(3, 128, generator=gen) * 3).to(DEV)

    def step(k, zero=True):
        if zero:
            model.zero_grad(set_to_none=True)
        (kl_topk_loss(model(x), teacher, 5) * 2.0 ** k).backward()

    return model, step


def pretrain_case():
    """the full pre-training step of tests/golden/e2e.pt, every draw pinned (encoder, text tower, PretrainHeadEngine -- or, with
    PVRL_HEAD_ENGINE=0 in the environment, the same head through autograd and functional.StackFn, whose dx feeds the encoder)"""
    from procedurevrl_amd.vit import pretrain_loss
    f = ec.load("e2e")
    cfg, model, _ = ec._e2e_model(f)
    model.train()
    model.model.engine.use_graphs = False
    meta = {"clip_text_ids": f["clip_text_ids"].to(DEV), "clip_vis_feat": f["clip_vis_feat"].to(DEV)}
    rng = dict(order=dict(mask_inds=f["rng"]["mask_inds"].to(DEV), pad_start=f["rng"]["pad_start"].to(DEV),
                          noises=[n.to(DEV) for n in f["rng"]["noises"]]), rand_inds=f["rng"]["rand_inds"].to(DEV))
    x = f["inputs"].to(DEV)

    def step(k, zero=True):
        if zero:
            for p in model.parameters():
                p.grad = None
        pred, teacher, mse = model([x, meta], rng=rng)
        he = getattr(model.model, "head_engine", None)
        if he is not None:
            he.use_graphs = False
        (pretrain_loss(pred, teacher, mse, cfg)[0] * 2.0 ** k).backward()

    return model, step


def assert_replay_covariant(case, ks=KS_REPLAY):
    """eager k = 0 gradients; graphs captured at k = 0; replays at other k, plain and staged under a gradient hook, must be 2^k x them"""
    model, step = case
    eng = model.model.engine
    eng.use_graphs = False
    step(0)
    g0 = grads_of(model)
    assert_finite(g0)
    eng.use_graphs = True
    for _ in range(eng.GRAPH_WARMUP + 1):
        step(0)
    assert len(eng._graphs) == 1 and all("bwd" in g for g in eng._graphs.values()), "the step was not captured"
    assert not mismatches(g0, grads_of(model), 0), "capture at k = 0 differs from the eager launches"
    for k in ks + (0,):
        step(k)
        bad = mismatches(g0, grads_of(model), k)
        assert not bad, f"replay at k = {k} of a graph captured at k = 0: {bad[:8]}"
    calls = []
    eng.grad_hook = calls.append
    try:
        for k in (0,) + ks:
            del calls[:]
            step(k)
            bad = mismatches(g0, grads_of(model), k)
            assert not bad, f"staged replay at k = {k}: {bad[:8]}"
            assert calls, "the gradient hook never ran"
    finally:
        eng.grad_hook = None


ACC_K = 9


def accumulation_errors(g, acc, k=ACC_K):
    """-> [(name, worst |acc - (1 + 2^k) g| / bound)] with bound = 4 * 2^-24 * (|g| + |2^k g|) per element: at most two fp32 roundings of
    quantities no larger than that sum, factor 2 margin"""
    out = []
    for n in g:
        a, b = acc[n].double(), g[n].double()
        bound = 4 * 2.0 ** -24 * (b.abs() + (2.0 ** k * b).abs())
        err = (a - (1 + 2.0 ** k) * b).abs()
        over = err > bound
        if bool(over.any()):
            out.append((n, int(over.sum()), float((err / bound.clamp_min(1e-300))[over].max())))
    return out


def assert_accumulates(case, hook_unscale=False):
    """backward at k = 0 then at k = +9 without zeroing, and in the other order"""
    model, step = case
    eng = model.model.engine
    eng.use_graphs = False
    step(0)
    g = grads_of(model)
    if hook_unscale:
        eng.grad_hook = lambda i: model.model.grad_store().unscale()
    try:
        for first, second in ((0, ACC_K), (ACC_K, 0)):
            step(first)
            step(second, zero=False)
            acc = grads_of(model)
            assert_finite(acc)
            bad = accumulation_errors(g, acc)
            assert not bad, f"k = {first} then k = {second} without zeroing (hook_unscale={hook_unscale}): {bad[:8]}"
    finally:
        eng.grad_hook = None


def skip_flag(model):
    return float(model.model.grad_store().bad.item())


# ====================================================================================================== begin_scaled's branches (GPU)
def new_store():
    from procedurevrl_amd.grads import GradStore
    return GradStore([("w", torch.nn.Parameter(torch.zeros(64, device=DEV)))], DEV)


def begin_scaled_kernel(g):
    """the one-launch branch's kernel on any size (the product takes it up to SEAM elements)"""
    from procedurevrl_amd import ops
    from procedurevrl_amd._lib import lib
    out, scale, inv = torch.empty_like(g), torch.empty(1, device=g.device, dtype=F32), torch.full((4096,), float("nan"), device=g.device)
    lib().call("pvrl_grad_scale_begin", ops._ptr(g), g.numel(), SCALE_TARGET, ops._ptr(out), ops._ptr(scale), ops._ptr(inv), 4096, ops._stream())
    return out, scale, inv


def begin_scaled_torch(g):
    """the torch branch on any size: the same values behind a stride of 2 (a non-contiguous gradient takes that branch)"""
    gs = new_store()
    buf = torch.empty((g.numel(), 2), device=g.device, dtype=F32)
    buf[:, 0] = g.reshape(-1)
    nc = buf[:, 0]
    assert not nc.is_contiguous() or g.numel() == 1
    out = gs.begin_scaled(nc)
    return out.reshape(g.shape), gs.scale, gs.inv_row


def seam_gradient(n, j=None, nb=0, seed=0):
    """n values of rms 2^j / 8 whose largest magnitude is 2^j (nb = 0) or its fp32 neighbour below / above (nb = -1 / +1)"""
    gen = torch.Generator().manual_seed(seed + n % 1000)
    g = torch.randn(n, generator=gen)
    if j is not None:
        g = (g / g.abs().max() * 0.75 * 2.0 ** j).float()
        top = torch.tensor(2.0 ** j, dtype=F32)
        if nb:
            top = torch.nextafter(top, torch.tensor(float("inf") if nb > 0 else 0.0))
        g[n // 3] = -top
    return g


def check_branches(g):
    """-> findings: both branches on g (contiguous fp32 on the device)"""
    import optim_checks as oc
    amax = float(g.abs().max())
    allowed = oc.gsb_allowed(amax, True, SCALE_TARGET)
    res = {"kernel": begin_scaled_kernel(g), "torch": begin_scaled_torch(g)}
    gs = new_store()
    res["product"] = (gs.begin_scaled(g), gs.scale, gs.inv_row)
    bad = []
    for name, (out, S, inv) in res.items():
        s = float(S)
        if s not in allowed:
            bad.append(f"{name}: S = {s} not in {sorted(allowed)} (amax = {amax!r})")
        if inv.numel() != 4096 or not bool((inv == 1.0 / s).all()):
            bad.append(f"{name}: inv_row not 1 / S in every slot")
        if not torch.equal(out.reshape(-1), g.reshape(-1) * s):
            bad.append(f"{name}: g * S is not the exact product")
    names = sorted(res)
    for a in names:
        for b in names:
            if a < b and float(res[a][1]) == float(res[b][1]) and not torch.equal(res[a][0].reshape(-1), res[b][0].reshape(-1)):
                bad.append(f"{a} / {b}: same S, different g * S")
    return bad, {n: float(r[1]) for n, r in res.items()}


# ====================================================================================================== regimes
CLS_REGIMES = ("randn", "one_clip", "outlier", "one_hot")
TOK_REGIMES = ("randn", "mean_pool", "cls_only", "patch_only", "one_token", "masked", "outlier")
OUTLIER = 2.0 ** 10
# parameters whose REFERENCE gradient is exactly zero in a regime, and must be exactly zero through the engine (every other parameter is
# judged by the ratio rule; tests/test_grad_scale_host.py checks on the CPU that the reference has no other zero-norm gradient)
STRUCTURAL_ZEROS = {}


def cls_gradient(regime, B, C, seed=11):
    g = torch.randn(B, C, generator=torch.Generator().manual_seed(seed))
    if regime == "one_clip":
        g[1:] = 0
    elif regime == "outlier":
        g[B - 1] *= OUTLIER
    elif regime == "one_hot":
        g = torch.zeros(B, C)
        g[B // 2, C // 3] = 1.0
    else:
        assert regime == "randn"
    return g


def tok_gradient(regime, B, S, C, seed=13):
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(B, S, C, generator=gen)
    if regime == "mean_pool":
        g = (torch.randn(B, 1, C, generator=gen) / S).expand(B, S, C).contiguous()
    elif regime == "cls_only":
        g[:, 1:] = 0
    elif regime == "patch_only":
        g[:, 0] = 0
    elif regime == "one_token":
        keep = g[B - 1, S // 2].clone()
        g = torch.zeros(B, S, C)
        g[B - 1, S // 2] = keep
    elif regime == "masked":
        m = torch.rand(B, S, generator=gen) < 0.25
        g = g * m.unsqueeze(-1)
    elif regime == "outlier":
        g[B - 1] *= OUTLIER
    else:
        assert regime == "randn"
    return g


def small_part(regime, g):
    """`outlier`: the gradient of the small clips alone"""
    assert regime == "outlier"
    s = g.clone()
    s[-1] = 0
    return s


def scale_of(g, scaled=True):
    """S of GradStore.begin_scaled, in exact arithmetic (1 for the bf16 flavour: no scaling)"""
    if not scaled:
        return 1.0
    a = min(max(float(g.abs().max()), 1e-30), 3e38)
    return 2.0 ** min(max(math.floor(math.log2(SCALE_TARGET / a)), -100), 100)


CLS_GEOM = dict(depth=2, crop=32, K=64, B=4, frames=8, seed=3)          # e2e_checks._hip_vs_oracle's small step


def cls_oracle_inputs():
    from oracle import timesformer_oracle as orc
    c = CLS_GEOM
    g = torch.Generator().manual_seed(c["seed"])
    label = torch.randn(c["K"], 512, generator=g) * 0.38
    label = label / label.norm(dim=1, keepdim=True)
    sd = orc.seeded_state(orc.encoder_shapes(c["depth"], c["frames"], (c["crop"] // 16) ** 2), c["seed"])
    x = torch.randn(c["B"], 3, c["frames"], c["crop"], c["crop"], generator=g)
    return label, sd, x


def cls_oracle_grads(sd, x, dfeat, rounded=None):
    """gradients of the encoder parameters for features.backward(dfeat) on the CPU: the fp32 oracle, or the rounded oracle run as the engine
    runs it -- its backward fed S * dfeat, its gradients divided by S"""
    from oracle import rounded_oracle as rorc
    from oracle import timesformer_oracle as orc
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    if rounded is None:
        orc.forward_features(params, x, CLS_GEOM["depth"]).backward(dfeat)
        return {k: p.grad for k, p in params.items() if p.grad is not None}
    S = scale_of(dfeat, rounded == torch.float16)
    rorc.RESID = "both"
    try:
        with rorc.operand(rounded):
            rorc.forward_features(params, x, CLS_GEOM["depth"]).backward(dfeat * S)
    finally:
        rorc.RESID = None
    return {k: p.grad / S for k, p in params.items() if p.grad is not None}


def tok_oracle_grads(f, sd, x, dtok, rounded=None):
    import tokens_checks as tc
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    S = scale_of(dtok, rounded == torch.float16)
    tc.oracle_tokens(f, params, x, rounded, grad=True).backward(dtok * S)
    return {k: p.grad / S for k, p in params.items() if p.grad is not None}


def judge(regime, hip, ref, model, zeros=()):
    """the project's rule: worst parameter's error / the model's worst <= TOL_RATIO_GRAD; the flat TOL_GRAD in `randn` only.
    -> (findings, per-parameter table [(name, hip error, model error)])"""
    bad, table = [], []
    for k, r in ref.items():
        if float(r.norm()) == 0.0:
            if k not in zeros:
                bad.append(f"{k}: the reference gradient is exactly zero but the case table does not name it")
            if k in hip and float(hip[k].abs().max()) != 0.0:
                bad.append(f"{k}: structurally zero in the reference, {float(hip[k].abs().max()):.3e} through the engine")
            continue
        if k in zeros:
            bad.append(f"{k}: named structurally zero, reference norm {float(r.norm()):.3e}")
        if k not in hip:
            bad.append(f"{k}: no gradient through the engine")
            continue
        table.append((k, ec.rel(hip[k], r), ec.rel(model[k], r)))
    for k in hip:               # a gradient the reference does not have at all (space_only: time_embed, the temporal layers)
        if k not in ref and float(hip[k].abs().max()) != 0.0:
            bad.append(f"{k}: no gradient in the reference, {float(hip[k].abs().max()):.3e} through the engine")
    wh, wm = max(t[1] for t in table), max(t[2] for t in table)
    if not wh / wm <= ec.TOL_RATIO_GRAD:
        bad.append(f"worst gradient error / rounding model's = {wh:.3e} / {wm:.3e} = {wh / wm:.3f} > {ec.TOL_RATIO_GRAD}")
    if regime == "randn" and not wh <= ec.TOL_GRAD:
        bad.append(f"worst gradient error {wh:.3e} > {ec.TOL_GRAD}")
    return bad, table, (wh, wm)


def print_table(tag, table, worst):
    wh, wm = worst
    print(f"[{tag}] worst error {wh:.3e} / model's {wm:.3e} = ratio {wh / wm:.3f}")
    for k, eh, em in sorted(table, key=lambda t: -t[1] / max(t[2], 1e-30))[:6]:
        print(f"[{tag}]   {k}: {eh:.3e} / {em:.3e} = {eh / max(em, 1e-30):.3f}")


# ====================================================================================================== headroom hook (GPU, test only)
class RowSumProbe:
    """records max|value| going into each 16-bit rounding of an S-scaled sum over rows (ROW_SUM_SITES) while an engine's backward runs:
    wraps ops.cast_weights_multi inside EncoderEngine._temporal_chain_all and the 16-bit ops.group_reduce of the cls rows' dqkv, the way
    tools/probe/grad_range.py wraps the GEMM entry points.  No switch in product code."""

    def __init__(self, eng):
        self.eng, self.maxima, self._in_chain = eng, {"dW_e": [], "dW_e_sum": [], "dqkv_cls": []}, False

    def __enter__(self):
        from procedurevrl_amd import ops
        self.ops, self._cast, self._gr, self._chain = ops, ops.cast_weights_multi, ops.group_reduce, self.eng._temporal_chain_all

        def cast(items):
            if self._in_chain:
                self.maxima["dW_e"] += [w.abs().max() for w, _, _ in items]
            return self._cast(items)

        def group_reduce(x, *a, **kw):
            out = self._gr(x, *a, **kw)
            o = kw.get("out")
            if o is not None and o.dtype != F32 and self.eng.saved is not None and x.dtype != F32 and x.shape[-1] == 3 * self.eng.C:
                self.maxima["dqkv_cls"].append(o.float().abs().max())
            return out

        def chain(gs):
            self.maxima["dW_e_sum"] += [dwe.abs().max() for _, dwe, _ in self.eng._chain]      # the sum itself, before its own power of two
            self._in_chain = True
            try:
                return self._chain(gs)
            finally:
                self._in_chain = False

        ops.cast_weights_multi, ops.group_reduce, self.eng._temporal_chain_all = cast, group_reduce, chain
        return self

    def __exit__(self, *a):
        self.ops.cast_weights_multi, self.ops.group_reduce = self._cast, self._gr
        del self.eng._temporal_chain_all

    def report(self):
        return {k: (max(float(t) for t in v) if v else None) for k, v in self.maxima.items()}


def headroom_model(B, crop, frames=8, depth=1):
    """ViT-B divided space-time, `depth` blocks, seeded weights with a non-trivial temporal_fc"""
    from procedurevrl_amd.datasets import synthetic_label_emb
    cfg = ec.make_cfg(depth, crop, 64, drop_path=0.0, frames=frames)
    torch.manual_seed(0)
    model = ec.build(cfg, synthetic_label_emb(64, 512, seed=1)).to(DEV).train()
    _reinit_temporal_fc(model.model)
    model.model.engine.use_graphs = False
    return model


def headroom_dtok(regime, B, S, C, seed=17):
    """`randn` / `mean_pool` generated on the device (mean_pool: d mean(tokens) . v / d tokens = v / S on every token of the clip)"""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    if regime == "randn":
        return torch.randn(B, S, C, device=DEV, generator=gen)
    assert regime == "mean_pool"
    return (torch.randn(B, 1, C, device=DEV, generator=gen) / S).expand(B, S, C).contiguous()


def headroom_run(model, x, dtok, ks=()):
    """one all-token step under the probe -> (maxima, gradients); then covariance at `ks`"""
    vt = model.model

    def step(k, zero=True):
        if zero:
            model.zero_grad(set_to_none=True)
        vt.forward_features(x, cls=False).backward(dtok * 2.0 ** k)

    vt.grad_store().bad.zero_()
    with RowSumProbe(vt.engine) as probe:
        step(0)
    g0 = grads_of(model)
    maxima = probe.report()
    bad = headroom_findings(maxima, g0)
    assert not bad, (bad, maxima)
    assert skip_flag(model) == 0.0, "the optimiser's skip flag was raised"
    for k in ks:
        step(k)
        bad = mismatches(g0, grads_of(model), k)
        assert not bad, f"k = {k}: {bad[:8]}"
    assert skip_flag(model) == 0.0
    return maxima, g0




def headroom_findings(maxima, grads, scaled=SCALED):
    """the headroom case: every value entering a 16-bit cast of a row sum is representable (fp16 flavour), every gradient finite.  (A
    finite-only check would pass a copy that SATURATES at 65,504.)"""
    bad = [f"non-finite gradient: {k}" for k, g in grads.items() if not bool(torch.isfinite(g).all())]
    for site, v in maxima.items():
        if scaled and site != "dW_e_sum" and v is not None and not v <= FP16_MAX:
            bad.append(f"{site}: max|value| {v:.4g} entering the 16-bit cast exceeds fp16's {FP16_MAX:g}")
    return bad


# ====================================================================================================== the rules on the CPU (host test)
def r16(t, dtype, flush=False, saturate=False):
    """round to the operand type and back; `flush`: 16-bit subnormals to zero; `saturate`: clamp at the type's largest finite value"""
    if saturate:
        t = t.clamp(-torch.finfo(dtype).max, torch.finfo(dtype).max)
    o = t.to(dtype).float()
    if flush:
        o = torch.where(o.abs() < torch.finfo(dtype).tiny, torch.zeros_like(o), o)
    return o


def model_scale(g, off=0):
    """GradStore.begin_scaled's torch branch"""
    a = torch.nan_to_num(g.abs().max(), nan=1.0, posinf=3e38).clamp(1e-30, 3e38)
    return torch.exp2((torch.floor(torch.log2(SCALE_TARGET / a)) + off).clamp(-100.0, 100.0))


class ToyEngine:
    """A two-layer linear chain h = x W1^T, y = h W2^T + b with the engines' scaling rules on plain fp32 tensors: the backward is fed
    S * dy (fp16) or dy (bf16), every gradient operand is rounded to the operand type, a sum over rows is rounded for a chain GEMM the way
    dW_e is, each parameter gradient is un-scaled where it is written (`gscale`) and accumulates into what is there in true units.
    W2 attenuates by `atten`, so the inner gradient dh sits low in the 16-bit range, as the engines' inner gradients do.
    `defect`: one of DEFECTS."""

    DWE_LIMIT = 32768.0         # EncoderEngine.DWE_LIMIT

    def __init__(self, dtype, seed=0, rows=48, width=24, atten=2.0 ** -8, x_mean=0.0, defect=None, rescale=True):
        g = torch.Generator().manual_seed(seed)
        self.dtype, self.scaled, self.defect = dtype, dtype == torch.float16, defect
        self.x = torch.randn(rows, width, generator=g) + x_mean
        self.W1 = torch.randn(width, width, generator=g) * width ** -0.5
        self.W2 = torch.randn(width, width, generator=g) * width ** -0.5 * atten
        self.grads, self.S_first, self.S_prev, self.S, self.max_into_cast, self.max_row_sum = {}, None, None, None, 0.0, 0.0
        self.rescale = rescale and defect != "row_sum_copy_saturates"      # (the engine's own power of two for the row sum's copy)

    def R(self, t, **kw):
        return r16(t, self.dtype, **kw)

    def zero(self):
        self.grads = {}

    def exact(self, dy):
        """the fp32 chain without rounding or scaling (the reference)"""
        dh = dy @ self.W2
        dW1 = dh.t() @ self.x
        return {"W2": dy.t() @ (self.x @ self.W1.t()), "W1": dW1, "W1_chain": dW1 @ self.W2, "b": dy.sum(0)}

    def backward(self, dy):
        d = self.defect
        S = model_scale(dy, off=1 if d == "torch_branch_S_one_power_off" else 0) if self.scaled else torch.tensor(1.0)
        if d == "S_frozen_at_first_value":
            self.S_first = S if self.S_first is None else self.S_first
            S = self.S_first
        inv = 1.0 / S
        prev, self.S_prev, self.S = (S if self.S_prev is None else self.S_prev), S, S
        acc = bool(self.grads)
        flush = d == "subnormals_flushed"
        h = self.R(self.x) @ self.R(self.W1).t()
        dys = self.R(dy * S, flush=flush)                                   # 16-bit gradient operand, S-scaled units
        dh = self.R(dys @ self.R(self.W2), flush=flush)
        dW2 = dys.t() @ self.R(h)                                           # fp32 sums over rows, S-scaled
        dW1 = dh.t() @ self.R(self.x)
        e = torch.tensor(0.0)
        if self.scaled and self.rescale:                                    # EncoderEngine._temporal_chain_all: 2^-e into the copy, 2^e into its scale
            e = torch.ceil(torch.log2(dW1.abs().max().clamp_min(1e-30) / self.DWE_LIMIT)).clamp(0.0, 100.0)
        self.max_row_sum, self.max_into_cast = float(dW1.abs().max()), float((dW1 * torch.exp2(-e)).abs().max())
        dW1c = self.R(dW1 * torch.exp2(-e), saturate=d == "row_sum_copy_saturates")     # the 16-bit copy of a row sum (dW_e's)
        db = dys.sum(0)
        out = {"W2": dW2 * inv, "W1": dW1 * inv, "W1_chain": (dW1c @ self.R(self.W2)) * (inv * torch.exp2(e)), "b": db * inv}
        if d == "one_parameter_left_in_S_units":
            out["W1"] = dW1
        if d == "bias_sum_in_true_units":
            out["b"] = (db + dy[0]) * inv                                   # a true-unit term added to the S-unit accumulator
        if acc and d == "inv_twice_on_accumulating_step":
            out = {k: v * inv for k, v in out.items()}
        for k, v in out.items():
            if k in self.grads:
                old = self.grads[k]
                if d == "target_converts_with_previous_S":                 # what is there joins the S units with the wrong S
                    old = old * prev * inv
                self.grads[k] = old + v
            else:
                self.grads[k] = v

    def run(self, dy, k=0, zero=True):
        if zero:
            self.zero()
        self.backward(dy * 2.0 ** k)
        return {n: g.clone() for n, g in self.grads.items()}


def toy_dy(rows=48, width=24, regime="randn", seed=1, mag=3e-5):
    g = torch.randn(rows, width, generator=torch.Generator().manual_seed(seed)) * mag
    if regime == "outlier":
        g[-1] *= OUTLIER
    elif regime == "mean_pool":
        g = g[:1].expand(rows, width).contiguous()
    return g


def toy_covariance(eng, ks):
    dy = toy_dy()
    g0 = eng.run(dy)
    return [(k, m) for k in ks for m in mismatches(g0, eng.run(dy, k), k)]


def toy_accumulation(eng):
    dy = toy_dy()
    g = eng.run(dy)
    bad = []
    for first, second in ((0, ACC_K), (ACC_K, 0)):
        eng.run(dy, first)
        bad += accumulation_errors(g, eng.run(dy, second, zero=False))
    return bad


def toy_branches(eng):
    import optim_checks as oc
    bad = []
    if not eng.scaled:          # (the bf16 flavour picks no S)
        return bad
    for j in (-20, 0, 8):
        dy = toy_dy() / toy_dy().abs().max() * 2.0 ** j
        eng.run(dy)
        if float(eng.S) not in oc.gsb_allowed(float(dy.abs().max()), True, SCALE_TARGET):
            bad.append((j, float(eng.S)))
    return bad


def toy_headroom(dtype, defect=None, rows=8192, rescale=True):
    """coherent rows (`mean_pool`) on an input with a mean: the row sum grows with the row count, here past 65,504.  Also held to the
    fp32 chain: the copy's own power of two must cost no accuracy"""
    eng = ToyEngine(dtype, rows=rows, atten=1.0, x_mean=1.0, defect=defect, rescale=rescale)
    dy = toy_dy(rows, regime="mean_pool")
    g = eng.run(dy)
    bad = headroom_findings({"dW_e": eng.max_into_cast}, g, scaled=eng.scaled)
    err = ec.rel(g["W1_chain"], eng.exact(dy)["W1_chain"])
    if not err <= 4 * float(torch.finfo(dtype).eps):
        bad.append(f"W1_chain: {err:.3e} from the fp32 chain")
    return bad, g, eng


def toy_outlier(eng, healthy):
    dy = toy_dy(regime="outlier")
    ref = healthy.exact(dy)
    bad, table, worst = judge("outlier", eng.run(dy), ref, healthy.run(dy))
    return bad, worst


TOY_CASES = ("covariance", "replay", "accumulation", "branches", "headroom", "outlier")


def toy_case(case, dtype, defect=None):
    """-> findings of one named case on the toy engine (empty: passes)"""
    eng = ToyEngine(dtype, defect=defect)
    if case == "covariance":
        return toy_covariance(eng, (-24, -7, 7, 24) if dtype == torch.float16 else (-7, 7))
    if case == "replay":
        return toy_covariance(eng, KS_REPLAY)
    if case == "accumulation":
        return toy_accumulation(eng)
    if case == "branches":
        return toy_branches(eng)
    if case == "headroom":
        return toy_headroom(dtype, defect)[0]
    assert case == "outlier"      # (a deeper attenuation: the small clips' inner gradient sits AT fp16's subnormal threshold, 6.1e-5)
    return toy_outlier(ToyEngine(dtype, atten=2.0 ** -10, defect=defect), ToyEngine(dtype, atten=2.0 ** -10))[0]


DEFECTS = {
    # name: (the case that fails, would the suite before these tests have seen it?)
    "S_frozen_at_first_value": ("replay", "no: check_hip_graph_replay replays on a second input of the same magnitude"),
    "one_parameter_left_in_S_units": ("covariance", "only where S != 1 happens to hold and the parameter is compared; invisible at S = 1"),
    "inv_twice_on_accumulating_step": ("accumulation", "yes where S != 1: the accumulating step of check_hip_graph_replay (1e-5 of the sum)"),
    "bias_sum_in_true_units": ("covariance", "no: at the suite's one magnitude it is a term 1 / S too small or large, inside TOL_GRAD"),
    "target_converts_with_previous_S": ("accumulation", "no: every accumulating step of the suite repeats the magnitude, so both S agree"),
    "torch_branch_S_one_power_off": ("branches", "no: no GPU test compares the branches or checks the S the torch branch picks"),
    "row_sum_copy_saturates": ("headroom", "no: no test has more than 300 rows under an all-token gradient, and none looks at the cast's input"),
    "subnormals_flushed": ("outlier", "no: every engine test feeds a dense gradient of one magnitude"),
}
