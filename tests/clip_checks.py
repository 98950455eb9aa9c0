"""Global-norm gradient clipping (csrc/optim.hip: pvrl_sumsq_f32, pvrl_clip_coef, pvrl_adam_step_clip, pvrl_sgd_step_clip; optimizer.FusedOptimizer
with `clip_grad_l2norm`) against torch's clip_grad_norm_ formula with the sum of squares taken in float64.

Used by tests/test_clip_kernels_gpu.py and tests/test_clip_optimizer_gpu.py (pytest -m gpu) and by tests/test_clip_host.py (no GPU: a Python
model of the two kernels stands in through the `run=` hook, and planted defects show that the checks bite).

The reference is NOT torch's fp32 norm (2.9e-4 away from the fp64 norm on 20 M `randn * 0.05` elements, and `inf` from |g| = 2^70 on):
    total = gscale_f32 * sqrt(sum_f64 g^2)                 the norm of what the update applies
    coef  = min(1, max_norm / (total + 1e-6))
both evaluated in float64 here, unrounded, from the same fp32 inputs.

Bars, from the rounding count (u = 2^-24, half an ulp of fp32; nothing here comes from what the kernels give):
  norm  The kernels square exactly (a float times a float fits a double) and add in fp64: n <= 2^27 terms, each add within 2^-53, so the sum
        is within n * 2^-53 <= 2^-26 of the exact one even if every error had one sign, and the square root halves that.  The issue counts
        two fp32 roundings on top (the product with gscale, the result): NORM_BAR = 2 u = 2^-23, relative.  (The kernel takes the product in
        fp64 and rounds once: u + 2^-27.)  A norm below 2^-126 -- one denormal element on its own -- is held to 2^-149 absolute instead.
  coef  max_norm / (norm + 1e-6f) evaluated in fp32, max_norm an fp32 number (the tests pass one): the norm's error, the rounding of the sum
        (u), the rounding of the quotient (u), and 1e-6f against 1e-6 (2^-28.6 relative, scaled by 1e-6 / (norm + 1e-6) <= 1).  The issue
        fixes COEF_BAR = 2^-22 = 4 u: the two-rounding norm of its count fills it (2 u + u + u), the kernel's one-rounding norm leaves
        room (3 u + 2^-27 + 2^-28.6).  Where the unclamped value is above 1 by more than the bar the coefficient must be EXACTLY 1; within
        the bar of 1 either side of the clamp is right; it is never above 1.
Both bars are asserted as derived; a miss on the GPU would be a finding to explain.

Paths (the ids of the GPU tests name them).  sumsq_kernel is nonfinite_kernel's grid: ceil(floor(n / 4) / 256) workgroups of 256 threads,
at most 2048, one f32x4 per thread and pass; the n % 4 tail belongs to thread floor(n / 4), which at n = 1027 and 262,147 is thread 0 on its
SECOND pass; past 2,097,152 elements every thread loops.  One fp64 slot per workgroup: pvrl_sumsq_slots(n), restated in `slots_model`.

Planted defects (tests/test_clip_host.py), each caught by the checks the GPU runs: the norm taken without gscale; the coefficient not
clamped at 1; the 1e-6 dropped; the tail elements not summed (and not scanned); a second run writing its slots over the first run's.
"""
import math

import numpy as np
import torch

import optim_checks as oc
from attn_checks import Finding, report, Guarded  # noqa: F401

F32, F64 = torch.float32, torch.float64
NORM_BAR, COEF_BAR = 2.0 ** -23, 2.0 ** -22
MAX_GRID = 2048                                 # workgroups of sumsq_kernel's largest grid
PASS = MAX_GRID * 256 * 4                       # elements one pass of it covers
assert PASS == oc.SCAN_GRID
NS = (1, 3, 4, 5, 1023, 1024, 1027, 262147, PASS + 5)
MULTI = (1027, 3, 262147)                       # three runs laid into one workspace
CASES = [(n,) for n in NS] + [MULTI]
REGIMES = ("random", "small", "large", "zero", "non_finite", "clean_extremes")
GSCALE = 0.25
DEFECTS = ("norm_without_gscale", "coef_not_clamped", "eps_dropped", "tail_not_summed", "second_run_overwrites_first")
WS_FILL = -7.25                                 # a sum of squares is never negative: a slot that still holds this was not written


def slots_model(n):
    """pvrl_sumsq_slots restated"""
    return 0 if n <= 0 else min(max((n // 4 + 255) // 256, 1), MAX_GRID)


def case_id(ns):
    def one(n):
        path = ("tail_only" if n < 4 else "no_tail" if n % 4 == 0 else "loop_and_tail" if n > PASS else
                "tail_on_second_pass" if (n // 4) % 256 == 0 else "tail")
        return f"n{n}-{slots_model(n)}wg-{path}"
    return "sumsq-" + "+".join(one(n) for n in ns)


def ref_norm(xs, gscale):
    """xs: fp32 CPU tensors -> gscale_f32 * sqrt(sum_f64 g^2), a Python float (float64, unrounded)"""
    s = sum(float((x.double() ** 2).sum()) for x in xs)
    return oc.f32(gscale) * math.sqrt(s)


def ref_coef(total, max_norm):
    return min(1.0, max_norm / (total + 1e-6))


def make_inputs(ns, regime):
    gen = oc._gen("clip", ns, regime)
    if regime in ("random", "non_finite", "clean_extremes"):
        return [torch.randn(n, generator=gen) * 0.05 for n in ns]
    val = {"small": 2.0 ** -70, "large": 2.0 ** 70, "zero": 0.0}[regime]
    return [torch.full((n,), val) for n in ns]


def positions(ns):
    """(run, index): the first element, the last (in the tail where n % 4 != 0), the first element of the tail, and in every later run again"""
    out = []
    for r, n in enumerate(ns):
        out += sorted({(r, i) for i in (0, n - 1, n - n % 4 if n % 4 else n - 1) if 0 <= i < n})
    return out


def plant(xs, where, bits):
    ys = [x.clone() for x in xs]
    for r, i in where:
        ys[r].view(torch.int32)[i] = oc._i32(bits)
    return ys


# ---------------------------------------------------------------------------------------------------------------------
# a Python model of sumsq_kernel + clip_coef_kernel (and of what can go wrong in them)
# ---------------------------------------------------------------------------------------------------------------------
def model_run(defect=None):
    def run(xs, gscale, max_norms):
        total = sum(slots_model(x.numel()) for x in xs)
        ws = torch.full((total,), WS_FILL, dtype=F64)
        flag, slot = 0.0, 0
        for x in xs:
            n = x.numel()
            if defect == "tail_not_summed":
                x = x[:n - n % 4]
            blocks = slots_model(n)
            wg = (torch.arange(x.numel()) // 4 // 256) % blocks              # the workgroup that reads element i
            part = torch.zeros(blocks, dtype=F64).index_add_(0, wg, x.double() ** 2)
            at = 0 if defect == "second_run_overwrites_first" else slot
            ws[at:at + blocks] = part
            if bool(((x.view(torch.int32) & 0x7f800000) == 0x7f800000).any()):
                flag = 1.0
            slot += blocks
        s = float(ws.sum())
        g32 = np.float32(1.0 if defect == "norm_without_gscale" else gscale)
        with np.errstate(all="ignore"):
            norm = np.float32(np.float64(g32) * np.sqrt(np.float64(s)))
            coefs = []
            for m in max_norms:
                c = np.float32(m) / (norm if defect == "eps_dropped" else norm + np.float32(1e-6))
                coefs.append(float(c if defect == "coef_not_clamped" or not c > 1 else np.float32(1.0)))
        if not np.isfinite(norm):
            flag = 1.0
        return dict(norm=float(norm), coefs=coefs, flag=flag, findings=[])
    return run


# ---------------------------------------------------------------------------------------------------------------------
# the kernels (GPU)
# ---------------------------------------------------------------------------------------------------------------------
def gpu_run():
    """-> run(xs, gscale, max_norms): every x 16-byte aligned between bands of +inf (a read outside shows as a raised flag and an infinite
    norm), the workspace between bands of WS_FILL and exactly as large as the slot counts say (a write behind it is refused by the entry
    and would show in the band), norm / coef and the flag inside guard bands.  Everything is launched twice: bit-identical."""
    L, P, S = oc._abi()
    dev = torch.device("cuda:0")

    def run(xs, gscale, max_norms):
        f = []
        bufs = []
        for x in xs:
            b = torch.full((x.numel() + 8,), float("inf"), device=dev)
            b[4:4 + x.numel()].copy_(x)
            bufs.append(b)
        before = [b.clone() for b in bufs]
        total = sum(L.call("pvrl_sumsq_slots", x.numel()) for x in xs)
        f.append(Finding("pvrl_sumsq_slots against its restatement", total == sum(slots_model(x.numel()) for x in xs), float(total), 0.0, ""))
        twice = []
        for _ in range(2):
            ws = torch.full((total + 16,), WS_FILL, device=dev, dtype=F64)
            fb = Guarded("flag", [1], 1, F32, device=dev)
            fb.seg(0).fill_(0.0)
            slot = 0
            for x, b in zip(xs, bufs):
                L.call("pvrl_sumsq_f32", P(b[4:]), x.numel(), P(ws[8:]), slot, total, P(fb.seg(0)), S())
                slot += L.call("pvrl_sumsq_slots", x.numel())
            norms, coefs = [], []
            for m in max_norms:
                ob = Guarded("norm, coef", [2], 1, F32, device=dev)
                L.call("pvrl_clip_coef", P(ws[8:]), total, gscale, m, P(ob.seg(0)), P(fb.seg(0)), S())
                torch.cuda.synchronize()
                f += ob.check()[:1]
                o = ob.seg(0).cpu().reshape(-1)
                norms.append(o[0:1].clone())
                coefs.append(o[1:2].clone())
            f += fb.check()[:1]
            w = ws.cpu()
            nb = int((w[:8] != WS_FILL).sum() + (w[8 + total:] != WS_FILL).sum())
            f.append(Finding("workspace: elements in front of / behind the slots that changed", nb == 0, float(nb), 0.0, ""))
            nw = int((w[8:8 + total] == WS_FILL).sum())
            f.append(Finding("workspace: slots left unwritten", nw == 0, float(nw), 0.0, f"of {total}"))
            twice.append((w[8:8 + total].view(torch.int64), torch.cat(norms + coefs), float(fb.seg(0).cpu())))
        for b, b0 in zip(bufs, before):
            f += oc.bits_equal("an input and its bands", b, b0)
        nd = int((twice[0][0] != twice[1][0]).sum())
        f.append(Finding("slots of a second identical call whose bits differ", nd == 0, float(nd), 0.0, ""))
        f += oc.bits_equal("norm and coef of a second identical call", twice[0][1], twice[1][1])
        f.append(Finding("the flag of a second identical call", twice[0][2] == twice[1][2], twice[1][2], twice[0][2], ""))
        f += oc.bits_equal("the norm does not depend on max_norm", torch.cat(norms), norms[0].repeat(len(norms)))
        return dict(norm=float(norms[0]), coefs=[float(c) for c in coefs], flag=twice[0][2], findings=f)
    return run


def _rel(got, want):
    if want == 0.0:
        return 0.0 if got == 0.0 else float("inf")
    return abs(got - want) / abs(want) if math.isfinite(got) else float("inf")


def judge(label, got, xs, gscale, max_norms, expect_flag):
    """norm and every coef against the float64 formula, the flag against `expect_flag` -> [Finding]"""
    total = ref_norm(xs, gscale)
    under = total < 2.0 ** -126              # a denormal norm (one denormal element on its own): two roundings are 2 * 2^-150 absolute there
    ok = abs(got["norm"] - total) <= 2.0 ** -149 if under else _rel(got["norm"], total) <= NORM_BAR
    f = [Finding(f"{label}: norm, relative to the fp64 value", ok, _rel(got["norm"], total), NORM_BAR, f"got {got['norm']!r}, fp64 {total!r}")]
    for m, c in zip(max_norms, got["coefs"]):
        raw = m / (total + 1e-6)
        want = min(1.0, raw)
        ok = _rel(c, want) <= COEF_BAR and (c == 1.0 or raw < 1.0 + COEF_BAR) and c <= 1.0
        f.append(Finding(f"{label}: coef at max_norm {m!r}, relative to the fp64 value", ok, _rel(c, want), COEF_BAR,
                         f"got {c!r}, fp64 {want!r} (unclamped {raw!r})"))
    f.append(Finding(f"{label}: flag", got["flag"] == expect_flag, got["flag"], expect_flag, ""))
    return f


def max_norms_for(total):
    """fp32 thresholds: half the norm (clips), four times the norm (coef exactly 1), and for a norm below 1 also 2^-21 (below the 1e-6 of
    the formula: what a zero gradient is divided by)"""
    t = total if 2.0 ** -100 < total < float("inf") else 1.0       # (a zero or denormal norm: thresholds around 1)
    out = [oc.f32(0.5 * t), oc.f32(min(4.0 * t, 3e38))]                       # (3e38: next to FLT_MAX four times the norm is no fp32 number)
    return out + [2.0 ** -21] if total < 1.0 else out                         # (above a norm of 2^105 that coefficient would be a denormal)


def check_case(ns, regime, run=None):
    """one size (or the three-run case) in one regime -> [Finding]"""
    run = run or gpu_run()
    xs = make_inputs(ns, regime)
    f = []
    if regime in ("random", "small", "large", "zero"):
        mn = max_norms_for(ref_norm(xs, GSCALE))
        got = run(xs, GSCALE, mn)
        f += got["findings"] + judge(regime, got, xs, GSCALE, mn, 0.0)
        if regime == "zero":
            f.append(Finding("zero: norm is 0 and coef at max_norm 1.0 is exactly 1", got["norm"] == 0.0 and run(xs, GSCALE, [1.0])["coefs"] == [1.0],
                             got["norm"], 0.0, ""))
        if regime == "large":
            f.append(Finding("large: the norm is finite", math.isfinite(got["norm"]), got["norm"], 0.0, ""))
    elif regime == "clean_extremes":
        for b in oc.CLEAN_BITS:
            ys = plant(xs, positions(ns), b)
            mn = max_norms_for(ref_norm(ys, GSCALE))
            got = run(ys, GSCALE, mn)
            f += [h for h in got["findings"] if not h.ok] + judge(f"0x{b:08x} at {positions(ns)}", got, ys, GSCALE, mn, 0.0)
    else:
        for where in positions(ns):
            for b in oc.BAD_BITS:
                got = run(plant(xs, [where], b), GSCALE, [1.0])
                f += [h for h in got["findings"] if not h.ok]
                f.append(Finding(f"0x{b:08x} at (run, index) {where} of {ns}: flag", got["flag"] == 1.0, got["flag"], 1.0, ""))
                f.append(Finding(f"0x{b:08x} at (run, index) {where} of {ns}: the norm is not finite", not math.isfinite(got["norm"]),
                                 got["norm"], float("inf"), ""))
    return f


# ---------------------------------------------------------------------------------------------------------------------
# refusals: PVRL_EINVAL, nothing launched, outputs untouched
# ---------------------------------------------------------------------------------------------------------------------
def check_refusals():
    from procedurevrl_amd._lib import PvrlError
    L, P, S = oc._abi()
    dev = torch.device("cuda:0")
    g = Guarded("g", [64], 1, F32, device=dev)
    g.seg(0).fill_(0.5)
    out, flag = Guarded("out", [2], 1, F32, device=dev), Guarded("flag", [1], 1, F32, device=dev)
    out.seg(0).fill_(3.0)
    flag.seg(0).fill_(0.0)
    ws = torch.full((24,), WS_FILL, device=dev, dtype=F64)
    gp = lambda off=0: P(g.seg(0)[off:])
    w8 = P(ws[8:])
    half = P(ws[8:].view(F32)[1:])                                           # 4 bytes into a double
    sumsq = lambda g_=None, n=32, ws_=w8, slot=0, cap=8, fl=None: L.call("pvrl_sumsq_f32", g_ or gp(), n, ws_, slot, cap, fl or P(flag.seg(0)), S())
    coef = lambda ws_=w8, ns=8, mx=1.0, o=None, fl=None: L.call("pvrl_clip_coef", ws_, ns, 0.25, mx, o or P(out.seg(0)), fl or P(flag.seg(0)), S())
    null = lambda name, args: L.call(name, *args)
    refused = [("sumsq_f32: g one element off 16-byte alignment", lambda: sumsq(g_=gp(1))),
               ("sumsq_f32: g two elements off 16-byte alignment", lambda: sumsq(g_=gp(2))),
               ("sumsq_f32: null g", lambda: null("pvrl_sumsq_f32", (None, 32, w8, 0, 8, P(flag.seg(0)), S()))),
               ("sumsq_f32: null workspace", lambda: null("pvrl_sumsq_f32", (gp(), 32, None, 0, 8, P(flag.seg(0)), S()))),
               ("sumsq_f32: null flag", lambda: null("pvrl_sumsq_f32", (gp(), 32, w8, 0, 8, None, S()))),
               ("sumsq_f32: workspace 4 bytes off", lambda: sumsq(ws_=half)),
               ("sumsq_f32: slot -1", lambda: sumsq(slot=-1)),
               ("sumsq_f32: the last slot would lie behind the workspace", lambda: sumsq(slot=8)),
               ("sumsq_f32: a workspace of 0 slots", lambda: sumsq(cap=0)),
               ("clip_coef: max_norm 0", lambda: coef(mx=0.0)), ("clip_coef: max_norm -1", lambda: coef(mx=-1.0)),
               ("clip_coef: max_norm nan", lambda: coef(mx=float("nan"))), ("clip_coef: nslots -1", lambda: coef(ns=-1)),
               ("clip_coef: null workspace", lambda: null("pvrl_clip_coef", (None, 8, 0.25, 1.0, P(out.seg(0)), P(flag.seg(0)), S()))),
               ("clip_coef: null out", lambda: null("pvrl_clip_coef", (w8, 8, 0.25, 1.0, None, P(flag.seg(0)), S()))),
               ("clip_coef: null flag", lambda: null("pvrl_clip_coef", (w8, 8, 0.25, 1.0, P(out.seg(0)), None, S()))),
               ("clip_coef: workspace 4 bytes off", lambda: coef(ws_=half))]
    accepted = [("sumsq_f32: n 0", lambda: sumsq(n=0)), ("sumsq_f32: n -5 with null pointers", lambda: null("pvrl_sumsq_f32", (None, -5, None, 0, 0, None, S())))]
    before = {k: b.buf.clone() for k, b in (("g", g), ("out", out), ("flag", flag))}
    f = []
    for want, calls in ((-1, refused), (0, accepted)):
        for label, call in calls:
            try:
                call()
                rc = 0
            except PvrlError as e:
                rc = -1 if str(e).endswith("status -1") else str(e)
            f.append(Finding(label + ": status", rc == want, float(rc) if isinstance(rc, int) else float("nan"), float(want), str(rc)))
    torch.cuda.synchronize()
    for k, b in (("g", g), ("out", out), ("flag", flag)):
        f += oc.bits_equal(f"{k} and its guard bands after the refused and the empty calls", b.buf, before[k])
    nb = int((ws.cpu() != WS_FILL).sum())
    f.append(Finding("workspace elements changed by the refused and the empty calls", nb == 0, float(nb), 0.0, ""))
    return f


# ---------------------------------------------------------------------------------------------------------------------
# the update kernels with the coefficient's address
# ---------------------------------------------------------------------------------------------------------------------
CLIP = 0.37


def _launch_adam(L, S, name, c, b, gscale, skip, clip):
    tail = (skip, S()) if name == "pvrl_adam_step" else (skip, clip, S())
    L.call(name, b["p"], b["g"], b["m"], b["v"], c.n, oc.ADAM_LR, c.beta1, oc.ADAM_B2, oc.ADAM_EPS, c.wd, c.step, gscale, c.decoupled, *tail)


def _launch_sgd(L, S, name, c, b, gscale, skip, clip):
    tail = (skip, S()) if name == "pvrl_sgd_step" else (skip, clip, S())
    L.call(name, b["p"], b["g"], b.get("buf"), c.n, oc.SGD_LR, c.momentum, c.dampening, c.wd, c.nesterov, c.first, gscale, *tail)


def check_null_and_one_equal_plain(kind, c):
    """pvrl_*_step_clip with clip == NULL and with *clip = 1.0f against pvrl_*_step on the same inputs: every output bit-equal"""
    L, P, S = oc._abi()
    dev = torch.device("cuda:0")
    adam = kind == "adam"
    q = oc.make_adam_problem(c) if adam else oc.make_sgd_problem(c)
    names = ("p", "g", "m", "v") if adam else (("p", "g", "buf") if c.momentum != 0.0 else ("p", "g"))
    launch, plain = (_launch_adam, "pvrl_adam_step") if adam else (_launch_sgd, "pvrl_sgd_step")
    one = torch.ones(1, device=dev)
    outs = []
    for name, clip in ((plain, None), (plain + "_clip", None), (plain + "_clip", P(one))):
        d = {k: q[k].to(dev) for k in names}                  # (torch allocations are 256-byte aligned)
        launch(L, S, name, c, {k: P(d[k]) for k in names}, c.gscale, None, clip)
        torch.cuda.synchronize()
        outs.append({k: d[k].cpu() for k in names})
    f = []
    for label, o in (("clip == NULL", outs[1]), ("*clip = 1.0f", outs[2])):
        for k in names:
            f += oc.bits_equal(f"{plain}_clip, {label}, against {plain}: {k}", o[k], outs[0][k])
    f += oc.bits_equal("g", outs[0]["g"], q["g"])
    f += oc.bits_equal("the coefficient", one, torch.ones(1))
    return f


def clipped_case(c):
    """the case whose gradient scale is gscale * 0.37: what the existing reference and models see.  The kernel runs with the ORIGINAL gscale
    and *clip = 0.37f; gscale is a power of two in every case of the tables, so fl(fl(g * gscale) * 0.37f) == fl(g * f32(gscale * 0.37))
    and the existing rule (one rounding for the scaled gradient) covers the kernel's two operations as it stands."""
    assert math.frexp(c.gscale)[0] == 0.5
    return c._replace(gscale=c.gscale * oc.f32(CLIP))


def gpu_adam_clipped(orig):
    def run(c2, q):
        L, P, S = oc._abi()
        dev = torch.device("cuda:0")
        clip = torch.full((1,), CLIP, device=dev)
        out, f = oc._run_update(("p", "g", "m", "v"), q, lambda b, skip: _launch_adam(L, S, "pvrl_adam_step_clip", orig, b, orig.gscale, skip, P(clip)), dev)
        return out, f + oc.bits_equal("the coefficient", clip, torch.full((1,), CLIP))
    return run


def gpu_sgd_clipped(orig):
    def run(c2, q):
        L, P, S = oc._abi()
        dev = torch.device("cuda:0")
        clip = torch.full((1,), CLIP, device=dev)
        names = ("p", "g", "buf") if orig.momentum != 0.0 else ("p", "g")
        out, f = oc._run_update(names, q, lambda b, skip: _launch_sgd(L, S, "pvrl_sgd_step_clip", orig, b, orig.gscale, skip, P(clip)), dev)
        return out, f + oc.bits_equal("the coefficient", clip, torch.full((1,), CLIP))
    return run


# ---------------------------------------------------------------------------------------------------------------------
# through FusedOptimizer: the setup of tests/test_optimizer_gpu.py
# ---------------------------------------------------------------------------------------------------------------------
NUM_ITERS, STEPS, SKIP_NAME, SKIP_STEP = 4, 5, "model.time_embed", 2


def small_model(method, sgd, seed=0):
    import e2e_checks as ec
    from procedurevrl_amd.datasets import synthetic_label_emb
    from procedurevrl_amd.optimizer import construct_optimizer
    torch.manual_seed(seed)
    cfg = ec.make_cfg(2, 32, 64)
    cfg.SOLVER.OPTIMIZING_METHOD = method
    cfg.SOLVER.WEIGHT_DECAY, cfg.BN.WEIGHT_DECAY, cfg.TRAIN.MULT = 1e-2, 3e-3, 0.1      # two groups: encoder (lr_mult 0.1) / the rest
    cfg.SOLVER.MOMENTUM, cfg.SOLVER.DAMPENING, cfg.SOLVER.NESTEROV = sgd
    model = ec.build(cfg, synthetic_label_emb(64, 512, seed=1))
    with torch.no_grad():
        for p in model.parameters():
            p.add_(torch.randn_like(p) * 0.02)
    opt = construct_optimizer(model, cfg)
    assert len([g for g in opt.param_groups if g["params"]]) == 2
    opt.grad_scale = 1.0 / NUM_ITERS
    return cfg, model, opt


def make_grads(named, steps=STEPS, seed=5):
    """-> [{name: accumulated gradient of NUM_ITERS micro-batches}] per step; SKIP_NAME has none at SKIP_STEP.  Drawn once per (shapes,
    steps, seed) and shared: the tensors are not to be modified (the dicts are fresh)"""
    key = (tuple((n, tuple(p.shape)) for n, p in named), steps, seed)
    if key not in _GRADS:
        _GRADS[key] = _draw_grads(named, steps, seed)
    return [dict(d) for d in _GRADS[key]]


_GRADS = {}


def _draw_grads(named, steps, seed):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for step in range(steps):
        d = {}
        for n, p in named:
            if n == SKIP_NAME and step == SKIP_STEP:
                continue
            acc = torch.randn(p.shape, generator=gen) * 0.05
            for _ in range(NUM_ITERS - 1):
                acc += torch.randn(p.shape, generator=gen) * 0.05
            d[n] = acc
        out.append(d)
    return out


def torch_reference(cfg, opt, named, method):
    cpu = {n: p.detach().cpu().clone().requires_grad_(True) for n, p in named}
    by_id = {id(p): n for n, p in named}
    groups = [{"params": [cpu[by_id[id(p)]] for p in g["params"] if id(p) in by_id], "weight_decay": g["weight_decay"], "lr_mult": g["lr_mult"]}
              for g in opt.param_groups]
    s = cfg.SOLVER
    if method == "sgd":
        ref = torch.optim.SGD(groups, lr=s.BASE_LR, momentum=s.MOMENTUM, weight_decay=s.WEIGHT_DECAY, dampening=s.DAMPENING, nesterov=s.NESTEROV)
    else:
        ref = (torch.optim.Adam if method == "adam" else torch.optim.AdamW)(groups, lr=s.BASE_LR, betas=(0.9, 0.999), eps=1e-8,
                                                                           weight_decay=s.WEIGHT_DECAY)
    return cpu, ref


def reference_clip_(grads, gscale, max_norm):
    """the issue's reference on CPU gradients that already hold g * gscale (fp32): total from the RAW gradients in float64, rounded to fp32;
    coef in float64 from that, rounded to fp32; g.mul_(coef) in fp32 -> (total unrounded, coef unrounded)"""
    total = ref_norm([g / oc.f32(gscale) for g in grads], gscale)            # gscale is a power of two: the division restores the raw bits
    coef = ref_coef(oc.f32(total), max_norm)
    for g in grads:
        g.mul_(oc.f32(coef))
    return total, ref_coef(total, max_norm)


def set_grads(named, cpu, d):
    for n, p in named:
        p.grad = d[n].to(p.device) if n in d else None
        cpu[n].grad = None
        if n in d:
            cpu[n].grad = d[n].clone()
            cpu[n].grad /= NUM_ITERS                                          # tools/train_net.py:187-189


def state_worst(opt, ref, cpu, named, method):
    """-> {"exp_avg" | "exp_avg_sq" | "momentum_buffer": worst |a - b| / max|b|}; asserts the step counts"""
    sd = opt.state_dict()
    by_id = {id(p): n for n, p in named}
    idx, k = {}, 0
    for g in opt.param_groups:
        for j, p in enumerate(g["params"]):
            if id(p) in by_id:
                idx[by_id[id(p)]] = k + j
        k += len(g["params"])
    worst = {}
    for n, _ in named:
        st, st_ref = sd["state"][idx[n]], ref.state[cpu[n]]
        for key in (["momentum_buffer"] if method == "sgd" else ["exp_avg", "exp_avg_sq"]):
            a, b = st[key].cpu(), st_ref[key]
            worst[key] = max(worst.get(key, 0.0), float((a - b).abs().max() / b.abs().max()))
        if method != "sgd":
            assert float(st["step"]) == float(st_ref["step"]), (n, st["step"], st_ref["step"])
    return worst


def count_calls(L):
    """-> (list that receives the name of every L.call, undo)"""
    names, real = [], L.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)
    L.call = spy
    return names, lambda: L.__dict__.pop("call", None)
