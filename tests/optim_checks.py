"""Optimiser kernels (csrc/optim.hip) through the C ABI -- pvrl_adam_step, pvrl_sgd_step, pvrl_nonfinite_flag_f32, pvrl_grad_scale_begin --
against an fp64 reference, PER ELEMENT, at the sizes where each kernel takes another path, inside guard bands.

Used by tests/test_optim_kernels_gpu.py (pytest -m gpu: the HIP kernels through lib().call) and by tests/test_optim_harness_host.py (no
GPU: CPU models and torch.optim stand in for the kernels through the `run=` hooks, and planted defects show that the rule bites).

Rule for the two update kernels -- a derived running-error bound, no free constant.  The "kernel error <= ROW_FACTOR x model error" rule
of tests/attn_checks.py does not work element by element for an element-wise kernel: the model's error on one element is often zero.
Instead the update is evaluated in fp64 on the same fp32 inputs, with the fp32 constants the C entry forms in double and rounds once
(`adam_consts` / `sgd_consts`), and an absolute error bound is carried through every operation as a (value, err) pair:
  * the result of every fp32 operation adds 2^-24 |result| + 2^-150 (half an ulp; the second term is gradual underflow);
  * operand bounds pass through +, - and * by the absolute partial derivatives;
  * / and sqrt take the worst case at operand +- bound, not the derivative (not an upper bound once an operand's bound is a visible
    fraction of its value, as with a denormal v).
The operation sequence is the kernel's (adam_one / the comment in sgd_kernel):
    gg = g * gscale;  p *= decay (AdamW) | gg += wd * p (Adam);  d = gg - m;  m + w1 * d  (w1 < 0.5) | gg - d * (1 - w1)  (Tensor.lerp_'s
    other formula; 1 - w1 is an fp32 subtraction of constants, taken exactly);  (b2 * v) + ((w2 * gg) * gg);  sqrt(v) / bc2_sqrt + eps;
    p - step_size * (m / denom)
An fma contraction only removes a rounding, so one bound covers whatever the compiler contracts.  Every element of p, m, v (SGD: p, buf)
must satisfy |kernel - ref| <= (1 + 2^-10) * bound; the factor covers the second-order terms the propagation drops and is not a
tolerance to tune.  A Finding names the worst element, its index and its ratio.  No term of the bound has been widened.

Paths (the ids of the GPU tests name them).  adam_kernel: one f32x4 per thread, ceil(floor(n / 4) / 256) workgroups; the n % 4 tail belongs
to thread floor(n / 4), which exists in the grid unless floor(n / 4) is a multiple of 256 -- then (n = 1027, 262,147) thread 0 reaches it
on the SECOND pass of the grid-stride loop.  sgd_kernel: 8192 x 256 threads, loops above 2,097,152 elements.  nonfinite_kernel:
2048 x 256 threads x 4 elements, the same 2,097,152.  grad_scale_begin_kernel: one workgroup of 1024.

Side conditions on every update case: p / state / g sit inside guard bands (bands and g bit-unchanged); a launch whose `skip` flag
holds 0.0 equals the `skip == NULL` launch bit for bit; a launch whose flag is non-zero leaves p and the state bit-unchanged.  In the
`zero_grad_slots` regime (the 64-element padding of the flat buffers: p = g = m = v = 0) the outputs stay bit-zero.

pvrl_grad_scale_begin: the contract for S is in exact arithmetic (`gsb_allowed`): a = clamp(max|g|, 1e-30f, 3e38f) (3e38f when any
value is not finite), S = 2^clamp(floor(log2(target / a)), -100, 100); where target / a lies within 2^-20 (relative) of a power of two
either neighbour is accepted.  out == g * S and inv[0, ninv) == 1 / S bit for bit.

Measured on the CPU (pytest tests/test_optim_harness_host.py -s prints these), worst |x - ref| / bound over every GPU case:
  adam_step   0.977 (rounded model) / 0.977 (contracted model) / 0.977 (torch.optim);   adamw_step  0.982 / 0.983 / 0.983
  sgd_step    0.994 / 0.994 / 0.994 (the two production-loop sizes included)
  over 2^18 elements (`randn`, `eps_bound`, `underflow`, `cancel`; steps 1, 2, 1000, 100000; beta1 0.9 and 0.3): adam 0.994, adamw 0.992
Measured on an MI355X (pytest -m gpu tests/test_optim_kernels_gpu.py -s; identical in both operand flavours, the kernels are fp32):
  adam_step 0.977, adamw_step 0.943, sgd_step 0.994; every regime, `underflow` (denormal v) included, passes the bound as derived: nothing
  widened, no flush-to-zero floor.  Every scan, grad_scale_begin, refusal and padding-slot case passes.
Planted defects, the finding that caught each, value / bound:
  Adam, on the n = 1027 cases unless named (worst finding / its ratio to the bound):
    bias correction from step - 1: p 7.7e5 (step 2), p 598 (step 1000)        w2 replaced by b2: v 3.4e9
    eps inside the square root: p 8.8e3 (`eps_bound`), p 1.1e6 (`randn`)       coupled decay in AdamW mode: m 7.3e6
    gscale applied after the weight-decay term (Adam, wd 1e-2, gscale 0.25): v 3.8e6
    tail not updated: m 4.2e6 (`randn`), m 6.7e6 (`underflow`), m 1.3e7 (n = 3); tail updated twice: m 3.8e6, m 2.1e6 (n = 262,147);
    each of the tail findings names an element of the tail
  SGD: a stride of half the grid (n = 2,097,152 + 259): p 4.4e6 with momentum, p 5.6e6 without, naming an element >= 1,048,576
    first_step ignoring a loaded buffer (n = 257): buf 8.4e6        Nesterov using buf alone: p 1.8e6 (first step), p 2.1e6
  scan: tail not scanned: the flag stays 0 for every bad pattern at n - 1 (n = 3, 1027, 2,097,157); a signalling NaN with a zero quiet
    bit missed: 0x7f800001 leaves the flag 0 at every position
  grad_scale_begin: S from ceil: max|g| = nextafter(32, 0), target / max|g| just above 8, gives 16 where {4, 8} are accepted; inv written
    for the first 1024 slots only: 1 slot of ninv = 1025 is not 1 / S; a NaN dropped by fmaxf: S = 512 where 2^-100 is due
"""
import collections
import functools
import math
import zlib

import numpy as np
import torch

from attn_checks import Finding, report, Guarded, guarded_input  # noqa: F401

F32, F64 = torch.float32, torch.float64
U, TINY = 2.0 ** -24, 2.0 ** -150
SLACK = 1.0 + 2.0 ** -10
SGD_GRID = 8192 * 256               # threads of sgd_kernel's largest grid
SCAN_GRID = 2048 * 256 * 4          # elements one pass of nonfinite_kernel's largest grid covers
assert SGD_GRID == SCAN_GRID == 2097152
WORST = {}                          # entry -> worst ratio seen by `judge_bound` (printed by the test modules)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) % (1 << 31))


def f32(x):
    """a double rounded once to fp32, as a Python float"""
    return float(np.float32(x))


def _bits(t):
    return t.contiguous().cpu().view(torch.int32)


def bits_equal(name, a, b):
    a, b = _bits(a).reshape(-1), _bits(b).reshape(-1)
    nd = int((a != b).sum()) if a.shape == b.shape else a.numel() + 1
    first = int((a != b).nonzero()[0]) if 0 < nd <= a.numel() else None
    return [Finding(name + ": elements whose bits differ", nd == 0, float(nd), 0.0, f"first at {first}")]


# ---------------------------------------------------------------------------------------------------------------------
# (value, err) arithmetic: fp64 value, absolute bound on the fp32 kernel's distance from it
# ---------------------------------------------------------------------------------------------------------------------
def _x(t):
    return t.double(), torch.zeros(t.shape, dtype=F64)


def _rnd(v, e):
    return v, e + U * v.abs() + TINY


def _mul(a, b):
    """a pair times a pair or an exact constant"""
    if isinstance(b, float):
        return _rnd(a[0] * b, a[1] * abs(b))
    return _rnd(a[0] * b[0], a[0].abs() * b[1] + b[0].abs() * a[1])


def _add(a, b, sign=1.0):
    return _rnd(a[0] + sign * b[0], a[1] + b[1])


def _addc(a, c):
    return _rnd(a[0] + c, a[1])


def _div(a, b):
    """worst case over operand +- bound; a divisor whose interval reaches zero gives an infinite bound"""
    if isinstance(b, float):
        v = a[0] / b
        return _rnd(v, a[1] / abs(b))
    v = a[0] / b[0]
    e = torch.zeros_like(v)
    for sa in (-1.0, 1.0):
        for sb in (-1.0, 1.0):
            e = torch.maximum(e, ((a[0] + sa * a[1]) / (b[0] + sb * b[1]) - v).abs())
    e = torch.where(b[0].abs() > b[1], e, torch.full_like(e, float("inf")))
    return _rnd(v, e)


def _sqrt(a):
    v = a[0].sqrt()
    e = torch.maximum((a[0] + a[1]).sqrt() - v, v - (a[0] - a[1]).clamp_min(0.0).sqrt())
    return _rnd(v, e)


def judge_bound(entry, name, x, pair):
    """-> [Finding]: every element within SLACK * bound of the fp64 value; names the worst element"""
    v, e = pair
    d = (x.double() - v).abs()
    ratio = torch.where(torch.isfinite(d) & torch.isfinite(e), d / e, torch.full_like(d, float("inf")))
    i = int(ratio.argmax())
    r = float(ratio[i])
    WORST[entry] = max(WORST.get(entry, 0.0), r)
    return [Finding(f"{name} |x - ref| / bound", r <= SLACK, r, SLACK,
                    f"worst element {i} of {x.numel()}: got {float(x[i])!r}, fp64 {float(v[i])!r}, bound {float(e[i]):.3e}")]


# =====================================================================================================================
# pvrl_adam_step
# =====================================================================================================================
AdamConst = collections.namedtuple("AdamConst", "decay wd w1 omw1 b2 w2 step_size bc2_sqrt eps gscale")
ADAM_LR, ADAM_EPS, ADAM_B2 = 1e-3, 1e-8, 0.999


def adam_consts(lr, beta1, beta2, eps, wd, step, gscale):
    """the fp32 constants of pvrl_adam_step, formed in double and rounded once; omw1 = the kernel's fp32 `1.f - w1`"""
    bc1, bc2 = 1.0 - beta1 ** float(step), 1.0 - beta2 ** float(step)
    w1 = np.float32(1.0 - beta1)
    return AdamConst(f32(1.0 - lr * wd), f32(wd), float(w1), float(np.float32(1.0) - w1), f32(beta2), f32(1.0 - beta2), f32(lr / bc1),
                     f32(math.sqrt(bc2)), f32(eps), f32(gscale))


AdamCase = collections.namedtuple("AdamCase", "n regime step beta1 wd gscale decoupled")
ADAM_REGIMES = ("randn", "eps_bound", "underflow", "scaled", "cancel", "zero_grad_slots")
ADAM_NS = (1, 3, 4, 5, 1023, 1024, 1027, 262147)
ADAM_STEPS = (1, 2, 1000, 1000000)


def adam_path(n):
    nv = n // 4
    blocks = max(1, (nv + 255) // 256)
    if n < 4:
        return "tail_only"
    wg = "one_wg" if blocks == 1 else f"{blocks}_wgs"
    if n % 4 == 0:
        return wg + "_no_tail"
    return wg + ("_tail_on_second_pass" if nv % 256 == 0 else "_tail")


def adam_case_id(c):
    return (f"{'adamw' if c.decoupled else 'adam'}_step-n{c.n}-{adam_path(c.n)}-{c.regime}-step{c.step}-b{c.beta1}-wd{c.wd:g}"
            f"-gscale{c.gscale:g}")


def _build_adam_cases():
    cases = []
    k = 0
    for n in ADAM_NS:                                   # every n in `randn`
        for dec in (1, 0):
            cases.append(AdamCase(n, "randn", ADAM_STEPS[k % 4], (0.9, 0.3)[(k // 2) % 2], (0.0, 1e-2)[(k // 4 + k) % 2],
                                  (1.0, 0.25)[(k // 3) % 2], dec))
            k += 1
    for r, regime in enumerate(ADAM_REGIMES):           # every regime at n = 1027
        for dec in (1, 0):
            for j in range(2):
                step = ADAM_STEPS[(2 * r + j + dec) % 4]
                if regime == "cancel" and step == 1:    # gg next to m needs an m
                    step = 1000
                gs = 2.0 ** -8 if regime == "scaled" else (1.0, 0.25)[(r + j) % 2]
                wd = 0.0 if regime == "cancel" and not dec else (1e-2, 0.0)[(r + j + dec) % 2]
                cases.append(AdamCase(1027, regime, step, (0.9, 0.3)[(r + j + dec) % 2], wd, gs, dec))
                k += 1
    # gscale != 1 with (coupled) decay, and both formulas of the lerp, at every step count
    for step in ADAM_STEPS:
        for dec in (0, 1):
            cases.append(AdamCase(1027, "randn", step, 0.3, 1e-2, 0.25, dec))
            cases.append(AdamCase(5, "randn", step, 0.9, 1e-2, 0.25, dec))
    return list(dict.fromkeys(cases))


ADAM_CASES = _build_adam_cases()
ZERO_SLOTS = ((64, 128), (963, 1027))          # `zero_grad_slots` at n = 1027: one stretch of whole vectors, one that holds the tail


def make_adam_problem(c):
    """-> dict of fp32 CPU tensors p, g, m, v [n] (m = v = 0 at step 1)"""
    gen = _gen("adam", c.n, c.regime, c.step, c.beta1, c.wd, c.gscale, c.decoupled)
    rn = lambda s=1.0: torch.randn(c.n, generator=gen) * s
    ru = lambda s=1.0: torch.rand(c.n, generator=gen) * s
    p = rn(0.02)
    if c.regime in ("randn", "zero_grad_slots", "cancel"):
        g, m, v = rn(0.05) / c.gscale, rn(0.03), ru(2.5e-3) + 1e-8
    elif c.regime == "eps_bound":
        g, m, v = rn(1e-12) / c.gscale, rn(1e-12), ru(1e-24)
    elif c.regime == "underflow":
        g, m, v = rn(1e-21) / c.gscale, rn(1e-21), ru(1e-40)
    elif c.regime == "scaled":
        g, m, v = rn(1e4), rn(25.0), ru(1.6e3) + 1e-3
    if c.step == 1:
        m, v = torch.zeros(c.n), torch.zeros(c.n)
    if c.regime == "cancel":                           # gg = g * gscale within 3 ulp of m (gscale is a power of two)
        k = torch.randint(-3, 4, (c.n,), generator=gen).float()
        g = (m * (1.0 + k * 2.0 ** -23)) / c.gscale
    if c.regime == "zero_grad_slots":
        for a, b in ZERO_SLOTS:
            for t in (p, g, m, v):
                t[a:b] = 0.0
    return dict(p=p, g=g, m=m, v=v)


def _adam_k(c, step=None):
    return adam_consts(ADAM_LR, c.beta1, ADAM_B2, ADAM_EPS, c.wd, c.step if step is None else step, c.gscale)


@functools.lru_cache(maxsize=None)
def adam_reference(c):
    """-> {"p" | "m" | "v": (fp64 value, bound)}; computed once per case and left unchanged"""
    q, k = make_adam_problem(c), _adam_k(c)
    P, G, M, V = (_x(q[key]) for key in "pgmv")
    gg = _mul(G, k.gscale)
    if c.decoupled:
        P = _mul(P, k.decay)
    else:
        gg = _add(gg, _mul(P, k.wd))
    d = _add(gg, M, -1.0)
    M = _add(M, _mul(d, k.w1)) if k.w1 < 0.5 else _add(gg, _mul(d, k.omw1), -1.0)
    V = _add(_mul(V, k.b2), _mul(_mul(gg, k.w2), gg))
    den = _addc(_div(_sqrt(V), k.bc2_sqrt), k.eps)
    P = _add(P, _mul(_div(M, den), k.step_size), -1.0)
    return dict(p=P, m=M, v=V)


def _fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in fp64"""
    a = a.double() if torch.is_tensor(a) else a
    b = b.double() if torch.is_tensor(b) else b
    return (a * b + c.double()).float()


def _mad(form):
    return _fma if form == "fma" else (lambda a, b, c: a * b + c)


ADAM_DEFECTS = ("bias_correction_from_step_minus_1", "w2_replaced_by_b2", "eps_inside_the_sqrt", "coupled_decay_in_adamw_mode",
                "gscale_after_the_weight_decay_term", "tail_not_updated", "tail_updated_twice")


def _adam_once(p, g, m, v, k, decoupled, form, defect):
    mad = _mad(form)
    if defect == "gscale_after_the_weight_decay_term" and not decoupled:
        gg = mad(p, k.wd, g) * k.gscale
    else:
        gg = g * k.gscale
        if decoupled:
            p = p * k.decay
        if not decoupled or defect == "coupled_decay_in_adamw_mode":
            gg = mad(p, k.wd, gg)
    d = gg - m
    m = mad(d, k.w1, m) if k.w1 < 0.5 else mad(-d, k.omw1, gg)
    w2 = k.b2 if defect == "w2_replaced_by_b2" else k.w2
    v = mad(w2 * gg, gg, k.b2 * v)
    den = torch.sqrt(v + k.eps) / k.bc2_sqrt if defect == "eps_inside_the_sqrt" else torch.sqrt(v) / k.bc2_sqrt + k.eps
    return mad(m / den, -k.step_size, p), m, v


def adam_model(c, q, form="plain", defect=None):
    """fp32 torch restatement of adam_kernel on the CPU; form "plain": every operation rounded, "fma": every a * b + c contracted"""
    k = _adam_k(c, c.step - 1 if defect == "bias_correction_from_step_minus_1" else None)
    p, m, v = _adam_once(q["p"], q["g"], q["m"], q["v"], k, c.decoupled, form, defect)
    t = c.n - c.n % 4
    if defect == "tail_not_updated":
        p[t:], m[t:], v[t:] = q["p"][t:], q["m"][t:], q["v"][t:]
    if defect == "tail_updated_twice":
        p[t:], m[t:], v[t:] = _adam_once(p[t:], q["g"][t:], m[t:], v[t:], k, c.decoupled, form, defect)
    return dict(p=p, m=m, v=v)


def adam_torch_optim(c, q):
    """one step of torch.optim.Adam / AdamW (foreach=False: Tensor.lerp_, addcmul_, addcdiv_) on the CPU in fp32; the accumulation
    division of the gradient (tools/train_net.py:187-189) is the fp32 product g * gscale"""
    p = q["p"].clone().requires_grad_(True)
    p.grad = q["g"] * f32(c.gscale)
    cls = torch.optim.AdamW if c.decoupled else torch.optim.Adam
    opt = cls([p], lr=ADAM_LR, betas=(c.beta1, ADAM_B2), eps=ADAM_EPS, weight_decay=c.wd, foreach=False)
    if c.step > 1:
        opt.state[p] = dict(step=torch.tensor(float(c.step - 1)), exp_avg=q["m"].clone(), exp_avg_sq=q["v"].clone())
    opt.step()
    st = opt.state[p]
    assert float(st["step"]) == c.step
    return dict(p=p.detach(), m=st["exp_avg"], v=st["exp_avg_sq"])


def _vec(name, x, dev):
    """x [n] inside a guard band on the device (element 0 is 16-byte aligned) -> (Guarded, [n] view)"""
    gb = Guarded(name, [x.numel()], 1, F32, device=dev)
    gb.seg(0).copy_(x.reshape(-1, 1))
    return gb, gb.seg(0)[:, 0]


def _abi():
    from procedurevrl_amd import ops
    from procedurevrl_amd._lib import lib
    return lib(), ops._ptr, ops._stream


def _run_update(names, q, launch, dev):
    """the side conditions of an update entry: launch(buffers by name, skip pointer) three times -- skip NULL on one copy of the inputs;
    skip -> 0.0 on a second copy (bit-equal to the first); skip -> 1.0 on that result (bit-unchanged) -> (outputs of the first, findings)"""
    L, P, S = _abi()
    f = []
    flag0, flag1 = torch.zeros(1, device=dev), torch.ones(1, device=dev)
    runs = []
    for skip in (None, flag0):
        gb = {k: _vec(k, q[k], dev) for k in names}
        g_before = _bits(gb["g"][0].buf)
        launch({k: P(gb[k][1]) for k in names}, None if skip is None else P(skip))
        torch.cuda.synchronize()
        for k in names:
            f += gb[k][0].check()
        f += bits_equal("g and its guard bands", gb["g"][0].buf, g_before.view(F32))
        runs.append(gb)
    out = {k: runs[0][k][1].cpu() for k in names if k != "g"}
    for k in out:
        f += bits_equal(f"{k}: skip -> 0.0 against skip == NULL", runs[1][k][1], out[k])
    launch({k: P(runs[1][k][1]) for k in names}, P(flag1))
    torch.cuda.synchronize()
    for k in names:
        f += bits_equal(f"{k} and its guard bands after a launch with skip -> 1.0", runs[1][k][0].buf, runs[0][k][0].buf)
    f += bits_equal("the skip flags", torch.cat([flag0, flag1]), torch.tensor([0.0, 1.0]))
    return out, f


def gpu_adam(c, q):
    L, P, S = _abi()
    dev = torch.device("cuda:0")

    def launch(b, skip):
        L.call("pvrl_adam_step", b["p"], b["g"], b["m"], b["v"], c.n, ADAM_LR, c.beta1, ADAM_B2, ADAM_EPS, c.wd, c.step, c.gscale,
               c.decoupled, skip, S())
    return _run_update(("p", "g", "m", "v"), q, launch, dev)


def check_adam_case(c, run=None):
    """one case on the GPU (or through `run(c, problem) -> (dict p m v, findings)`) -> list of Finding"""
    q = make_adam_problem(c)
    ref = adam_reference(c)
    got, f = (run or gpu_adam)(c, {k: t.clone() for k, t in q.items()})
    entry = "adamw_step" if c.decoupled else "adam_step"
    for k in ("p", "m", "v"):
        f += judge_bound(entry, k, got[k], ref[k])
    if c.regime == "zero_grad_slots":
        for a, b in ZERO_SLOTS:
            for k in ("p", "m", "v"):
                f += bits_equal(f"{k}[{a}:{b}] (zero gradient, zero state) against zero", got[k][a:b], torch.zeros(b - a))
    return f


# =====================================================================================================================
# pvrl_sgd_step
# =====================================================================================================================
SgdCase = collections.namedtuple("SgdCase", "n momentum dampening nesterov first wd gscale")
SGD_LR = 0.05
SGD_CONFIGS = ((0.9, 0.0, 1), (0.9, 0.1, 0), (0.0, 0.0, 0))
SGD_PATHS = {1: "one_thread", 255: "one_wg_ragged", 256: "one_wg", 257: "two_wgs", SGD_GRID + 259: "second_pass_for_259_threads",
             2 * SGD_GRID + 1: "third_pass_for_one_thread"}


def sgd_case_id(c):
    cfg = "momentum0_null_buf" if c.momentum == 0 else f"m{c.momentum}-damp{c.dampening}-{'nesterov' if c.nesterov else 'plain'}"
    return f"sgd_step-n{c.n}-{SGD_PATHS[c.n]}-{cfg}-first{c.first}-wd{c.wd:g}-gscale{c.gscale:g}"


def _build_sgd_cases():
    cases = []
    for i, n in enumerate((1, 255, 256)):
        for j, (mo, da, ne) in enumerate(SGD_CONFIGS):
            cases.append(SgdCase(n, mo, da, ne, (i + j) % 2, (1e-4, 0.0)[(i + j) % 2], (1.0, 0.25)[(i + j + 1) % 2]))
    for (mo, da, ne) in SGD_CONFIGS:                    # every configuration x first_step x gscale at n = 257
        for first in ((1, 0) if mo else (0,)):
            for gs in (1.0, 0.25):
                cases.append(SgdCase(257, mo, da, ne, first, 1e-4, gs))
    # the production loop: `randn` only
    cases += [SgdCase(SGD_GRID + 259, 0.9, 0.0, 1, 0, 1e-4, 0.25), SgdCase(SGD_GRID + 259, 0.0, 0.0, 0, 0, 1e-4, 1.0),
              SgdCase(2 * SGD_GRID + 1, 0.9, 0.1, 0, 0, 1e-4, 1.0), SgdCase(2 * SGD_GRID + 1, 0.9, 0.0, 1, 1, 0.0, 0.25)]
    return cases


SGD_CASES = _build_sgd_cases()
SgdConst = collections.namedtuple("SgdConst", "lr momentum omd wd gscale")


def sgd_consts(c):
    return SgdConst(f32(SGD_LR), f32(c.momentum), f32(1.0 - c.dampening), f32(c.wd), f32(c.gscale))


@functools.lru_cache(maxsize=4)
def make_sgd_problem(c):
    """-> dict of fp32 CPU tensors p, g, buf [n] (cached: do not modify)"""
    gen = _gen("sgd", *c)
    rn = lambda s: torch.randn(c.n, generator=gen) * s
    return dict(p=rn(0.02), g=rn(0.05) / c.gscale, buf=rn(0.08))


@functools.lru_cache(maxsize=4)
def sgd_reference(c):
    q, k = make_sgd_problem(c), sgd_consts(c)
    P, G, B = _x(q["p"]), _x(q["g"]), _x(q["buf"])
    gg = _add(_mul(G, k.gscale), _mul(P, k.wd))
    out = {}
    if k.momentum != 0.0:
        B = gg if c.first else _add(_mul(B, k.momentum), _mul(gg, k.omd))
        out["buf"] = B
        gg = _add(gg, _mul(B, k.momentum)) if c.nesterov else B
    out["p"] = _add(P, _mul(gg, k.lr), -1.0)
    return out


SGD_DEFECTS = ("stride_of_half_the_grid", "first_step_ignores_a_loaded_buffer", "nesterov_uses_buf_alone")


def _sgd_once(p, g, buf, k, c, form, defect):
    mad = _mad(form)
    gg = mad(p, k.wd, g * k.gscale)
    if k.momentum != 0.0:
        first = c.first or defect == "first_step_ignores_a_loaded_buffer"
        buf = gg if first else mad(gg, k.omd, k.momentum * buf)
        gg = mad(buf, k.momentum, gg) if c.nesterov and defect != "nesterov_uses_buf_alone" else buf
    return mad(gg, -k.lr, p), buf


def sgd_model(c, q, form="plain", defect=None):
    k = sgd_consts(c)
    p, buf = _sgd_once(q["p"], q["g"], q["buf"], k, c, form, defect)
    if defect == "stride_of_half_the_grid":             # elements from SGD_GRID / 2 on are visited by two threads
        h = SGD_GRID // 2
        p, buf = p.clone(), buf.clone()
        p[h:], b2 = _sgd_once(p[h:], q["g"][h:], buf[h:], k, c._replace(first=0), form, None)
        buf[h:] = b2
    return dict(p=p, buf=buf) if k.momentum != 0.0 else dict(p=p)


def sgd_torch_optim(c, q):
    p = q["p"].clone().requires_grad_(True)
    p.grad = q["g"] * f32(c.gscale)
    opt = torch.optim.SGD([p], lr=SGD_LR, momentum=c.momentum, dampening=c.dampening, nesterov=bool(c.nesterov), weight_decay=c.wd,
                          foreach=False)
    if c.momentum != 0.0 and not c.first:
        opt.state[p] = dict(momentum_buffer=q["buf"].clone())
    opt.step()
    out = dict(p=p.detach())
    if c.momentum != 0.0:
        out["buf"] = opt.state[p]["momentum_buffer"]
    return out


def gpu_sgd(c, q):
    L, P, S = _abi()
    dev = torch.device("cuda:0")
    names = ("p", "g", "buf") if c.momentum != 0.0 else ("p", "g")

    def launch(b, skip):
        L.call("pvrl_sgd_step", b["p"], b["g"], b.get("buf"), c.n, SGD_LR, c.momentum, c.dampening, c.wd, c.nesterov, c.first, c.gscale,
               skip, S())
    return _run_update(names, q, launch, dev)


def check_sgd_case(c, run=None):
    q = make_sgd_problem(c)
    ref = sgd_reference(c)
    got, f = (run or gpu_sgd)(c, q)
    for k in ref:
        f += judge_bound("sgd_step", k, got[k], ref[k])
    return f


# =====================================================================================================================
# pvrl_nonfinite_flag_f32
# =====================================================================================================================
SCAN_NS = (1, 3, 4, 5, 1024, 1027, SCAN_GRID + 5)
BAD_BITS = (0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001)         # +inf, -inf, quiet NaNs, a signalling NaN
CLEAN_BITS = (0x7f7fffff, 0xff7fffff, 0x00000001, 0x807fffff, 0x80000000)       # +-FLT_MAX, denormals, -0.0
SCAN_DEFECTS = ("tail_not_scanned", "snan_with_a_zero_quiet_bit_missed")


def scan_case_id(n):
    path = ("tail_only" if n < 4 else "no_tail" if n % 4 == 0 else "second_pass_and_tail" if n > SCAN_GRID else "vectors_and_tail")
    return f"nonfinite_flag_f32-n{n}-{path}"


def scan_positions(n):
    """index 0, n - 1 (the tail branch), n - 4, the first element of the second pass, one drawn index"""
    drawn = int(torch.randint(0, n, (1,), generator=_gen("scan", n)))
    return sorted({i for i in (0, n - 1, n - 4, SCAN_GRID, drawn) if 0 <= i < n})


def _i32(b):
    return b - (1 << 32) if b >= (1 << 31) else b


def scan_model(x, flag, defect=None):
    """x: int32 bits [n], flag: float -> flag afterwards"""
    n = x.numel()
    e = (x & 0x7f800000) == 0x7f800000
    if defect == "snan_with_a_zero_quiet_bit_missed":
        e &= ((x & 0x007fffff) == 0) | ((x & 0x00400000) != 0)
    if defect == "tail_not_scanned":
        e = e[:n - n % 4]
    return (1.0 if bool(e.any()) else flag), []


def gpu_scan():
    """-> run(x int32 bits [n] on the CPU, flag) -> (flag afterwards, findings): x 16-byte aligned between bands of +inf, the flag
    inside a guard band"""
    L, P, S = _abi()
    dev = torch.device("cuda:0")
    state = {}

    def run(x, flag):
        n = x.numel()
        if state.get("n") != n:
            state["n"], state["buf"] = n, torch.full((n + 8,), float("inf"), device=dev)
        buf = state["buf"]
        buf[4:4 + n].view(torch.int32).copy_(x)
        fb = Guarded("flag", [1], 1, F32, device=dev)
        fb.seg(0).fill_(flag)
        L.call("pvrl_nonfinite_flag_f32", P(buf[4:]), n, P(fb.seg(0)), S())
        torch.cuda.synchronize()
        return float(fb.seg(0).cpu()), fb.check()[:1] + bits_equal("x", buf[4:4 + n].cpu(), x.view(F32))
    return run


def check_scan_case(n, run=None):
    run = run or gpu_scan()
    gen = _gen("scan-data", n)
    x = _bits(torch.randn(n, generator=gen)).clone()
    pos = scan_positions(n)
    f = []
    for j, b in enumerate(CLEAN_BITS + CLEAN_BITS[:1]):           # values that must NOT raise the flag, where the bad ones will sit
        for i in pos:
            x[i] = _i32(b)
        flag = 1.0 if j == len(CLEAN_BITS) else 0.0
        got, g = run(x, flag)
        f += g + [Finding(f"clean data holding 0x{b:08x} at {pos}, flag prefilled {flag}: flag afterwards",
                          math.copysign(1.0, got) == 1.0 and got == flag, got, flag, "")]
    for i in pos:
        for b in BAD_BITS:
            y = x.clone()
            y[i] = _i32(b)
            got, g = run(y, 0.0)
            f += [h for h in g if not h.ok]
            f.append(Finding(f"0x{b:08x} at index {i} of {n}: flag", got == 1.0, got, 1.0, ""))
    return f


# =====================================================================================================================
# pvrl_grad_scale_begin
# =====================================================================================================================
GSB_NS = (1, 63, 64, 65, 1023, 1024, 1025, 40000)
GSB_NINV = (1, 64, 1025)
GSB_TARGET = 256.0
GSB_FULL_SWEEP = (65, 1025)          # n at which max|g| runs over 2^j, j = -40 .. 40, and its two neighbours
GSB_DEFECTS = ("S_from_ceil", "inv_written_for_the_first_1024_slots_only", "nan_dropped_by_fmaxf")


def gsb_case_id(n):
    return f"grad_scale_begin-n{n}-{'one_pass' if n <= 1024 else 'loop'}-{'full_sweep' if n in GSB_FULL_SWEEP else 'five_exponents'}"


def gsb_allowed(amax, finite, target):
    """the contract in exact arithmetic -> the set of S accepted"""
    a = 3e38 if not finite else min(max(amax, f32(1e-30)), f32(3e38))
    a = f32(a)
    mt, et = math.frexp(target)
    ma, ea = math.frexp(a)
    r = mt / ma                                   # target / a = r * 2^(et - ea), r in (0.5, 2), exact enough: only its distance from 1 matters
    e = et - ea + (0 if r >= 1.0 else -1)
    frac = r if r >= 1.0 else 2.0 * r            # target / a = frac * 2^e, frac in [1, 2)
    es = {e}
    if frac < 1.0 + 2.0 ** -20:
        es.add(e - 1)
    if frac > 2.0 * (1.0 - 2.0 ** -20):
        es.add(e + 1)
    return {2.0 ** min(max(x, -100), 100) for x in es}


def gsb_model(g, target, ninv, defect=None):
    """fp32 restatement of grad_scale_begin_kernel -> (out, S, inv [ninv], findings)"""
    bad = bool((~torch.isfinite(g)).any())
    if defect == "nan_dropped_by_fmaxf":
        bad = bool(torch.isinf(g).any())
    a = torch.nan_to_num(g, nan=0.0).abs().max() if g.numel() else torch.tensor(0.0)
    a = torch.tensor(3e38) if bad else a.clamp(1e-30, 3e38)
    e = torch.log2(torch.tensor(target, dtype=F32) / a)
    e = (torch.ceil(e) if defect == "S_from_ceil" else torch.floor(e)).clamp(-100.0, 100.0)
    S = torch.exp2(e)
    inv = torch.full((ninv,), float("nan"))
    inv[:1024 if defect == "inv_written_for_the_first_1024_slots_only" else ninv] = 1.0 / S
    return g * S, float(S), inv, []


def gpu_gsb(g, target, ninv):
    L, P, S = _abi()
    dev = torch.device("cuda:0")
    n = g.numel()
    gd = guarded_input(g.reshape(-1, 1), F32, dev, 0)[:, 0]
    ob, sb, ib = (Guarded("out", [n], 1, F32, device=dev), Guarded("scale", [1], 1, F32, device=dev), Guarded("inv", [ninv], 1, F32, device=dev))
    L.call("pvrl_grad_scale_begin", P(gd), n, target, P(ob.seg(0)), P(sb.seg(0)), P(ib.seg(0)), ninv, S())
    torch.cuda.synchronize()
    f = [ob.check()[0], sb.check()[0], ib.check()[0]]
    return ob.seg(0)[:, 0].cpu(), float(sb.seg(0).cpu()), ib.seg(0)[:, 0].cpu(), f


def gsb_magnitudes(n):
    js = range(-40, 41) if n in GSB_FULL_SWEEP else (-40, -7, 0, 13, 40)
    out = []
    for j in js:
        m = 2.0 ** j
        out += [m, float(np.nextafter(np.float32(m), np.float32(np.inf))), float(np.nextafter(np.float32(m), np.float32(0)))]
    return out


def gsb_launches(n):
    """-> [(label, g, ninv)]: one placement per launch"""
    gen = _gen("gsb", n)
    base = (torch.rand(n, generator=gen) - 0.5) * 0.9           # |base| < 0.45: scaled by max|g| it stays below the planted maximum
    out = []
    t1023 = 1023 + 1024 * ((n - 1024) // 1024) if n >= 1024 else None       # the last element only thread 1023 reads
    for k, m in enumerate(gsb_magnitudes(n)):
        for place, i, val in (("max_negative_in_the_last_element", n - 1, -m), ("max_only_thread_1023_reads", t1023, m)):
            if i is None:
                continue
            g = base * m
            g[i] = val
            out.append((f"{place}, max|g| = {m!r}", g, GSB_NINV[k % 3]))
    for k, val in enumerate((float("inf"), float("-inf"), float("nan"))):
        g = base.clone()
        g[n - 1] = val
        out.append((f"only_non_finite_value_in_the_last_element ({val})", g, GSB_NINV[k % 3]))
    out.append(("all zero", torch.zeros(n), 64))
    out.append(("max|g| = 1e-35 (floor of 1e-30)", base * 1e-35, 1))
    out.append(("max|g| = 3.3e38 (exponent clamp)", base.sign() * 3.3e38, 1025))
    return out


def check_gsb_case(n, run=None):
    run = run or gpu_gsb
    f = []
    for label, g, ninv in gsb_launches(n):
        out, S, inv, guards = run(g.clone(), GSB_TARGET, ninv)
        finite = bool(torch.isfinite(g).all())
        amax = float(torch.nan_to_num(g, nan=0.0, posinf=0.0, neginf=0.0).abs().max())
        ok_set = gsb_allowed(amax, finite, GSB_TARGET)
        bad = [h for h in guards if not h.ok]
        bad.append(Finding(f"S ({label}, ninv {ninv})", S in ok_set, S, max(ok_set), f"accepted: {sorted(ok_set)}"))
        if math.isfinite(S) and S > 0 and math.frexp(S)[0] == 0.5:
            nb = int((_bits(inv) != _bits(torch.full((ninv,), f32(1.0 / S)))).sum())
            bad.append(Finding(f"inv slots that are not 1 / S ({label}, ninv {ninv})", nb == 0, float(nb), 0.0, ""))
            ref = g * f32(S)
            nd = int((_bits(torch.nan_to_num(out, nan=7.0)) != _bits(torch.nan_to_num(ref, nan=7.0))).sum())
            bad.append(Finding(f"out elements that are not g * S ({label})", nd == 0, float(nd), 0.0, ""))
        f += [h for h in bad if not h.ok]
    return f + [Finding(f"grad_scale_begin n = {n}: launches judged", True, float(len(gsb_launches(n))), 0.0, "failures are listed above")]


# =====================================================================================================================
# refusals (nothing is launched) and n <= 0
# =====================================================================================================================
def check_refusals():
    from procedurevrl_amd._lib import PvrlError
    L, P, S = _abi()
    dev = torch.device("cuda:0")
    bufs = {k: Guarded(k, [64], 1, F32, device=dev) for k in ("p", "g", "m", "v", "flag")}
    for b in bufs.values():
        b.seg(0).fill_(0.5)
    before = {k: b.buf.clone() for k, b in bufs.items()}
    ptr = lambda k, off=0: P(bufs[k].seg(0)[off:])
    a = dict(p=ptr("p"), g=ptr("g"), m=ptr("m"), v=ptr("v"))
    adam = lambda n=32, step=1, **kw: L.call("pvrl_adam_step", *[{**a, **kw}[k] for k in "pgmv"], n, 1e-3, 0.9, 0.999, 1e-8, 0.0, step,
                                             1.0, 1, None, S())
    sgd = lambda n=32, mom=0.9, **kw: L.call("pvrl_sgd_step", *[{**a, "buf": a["m"], **kw}[k] for k in ("p", "g", "buf")], n, 0.1, mom, 0.0,
                                             0.0, 1, 0, 1.0, None, S())

    def gsb(target=256.0, ninv=4, **kw):                # g, out, scale, inv = the g, p, m, v buffers
        b = {**a, **kw}
        return L.call("pvrl_grad_scale_begin", b["g"], 32, target, b["p"], b["m"], b["v"], ninv, S())
    refused = [(f"adam_step: {k} one element off 16-byte alignment", lambda k=k: adam(**{k: ptr(k, 1)})) for k in "pgmv"]
    refused += [(f"adam_step: {k} two elements off 16-byte alignment", lambda k=k: adam(**{k: ptr(k, 2)})) for k in "pgmv"]
    refused += [(f"adam_step: null {k}", lambda k=k: adam(**{k: None})) for k in "pgmv"]
    refused += [("adam_step: step 0", lambda: adam(step=0)), ("adam_step: step -3", lambda: adam(step=-3))]
    refused += [(f"sgd_step: null {k}", lambda k=k: sgd(**{k: None})) for k in ("p", "g")]
    refused += [("sgd_step: momentum 0.9 with a null buf", lambda: sgd(buf=None))]
    refused += [("nonfinite_flag_f32: null x", lambda: L.call("pvrl_nonfinite_flag_f32", None, 32, ptr("flag"), S())),
                ("nonfinite_flag_f32: null flag", lambda: L.call("pvrl_nonfinite_flag_f32", ptr("g"), 32, None, S())),
                ("nonfinite_flag_f32: x one element off 16-byte alignment", lambda: L.call("pvrl_nonfinite_flag_f32", ptr("g", 1), 32, ptr("flag"), S()))]
    refused += [("grad_scale_begin: target 0", lambda: gsb(target=0.0)), ("grad_scale_begin: target -1", lambda: gsb(target=-1.0)),
                ("grad_scale_begin: target nan", lambda: gsb(target=float("nan"))), ("grad_scale_begin: ninv 0", lambda: gsb(ninv=0)),
                ("grad_scale_begin: ninv -1", lambda: gsb(ninv=-1))]
    refused += [(f"grad_scale_begin: null {name}", lambda k=k: gsb(**{k: None})) for k, name in zip("gpmv", ("g", "out", "scale", "inv"))]
    accepted = [("adam_step: n 0", lambda: adam(n=0)), ("adam_step: n -5 with null pointers", lambda: adam(n=-5, p=None, g=None)),
                ("sgd_step: n 0", lambda: sgd(n=0)), ("sgd_step: n -1", lambda: sgd(n=-1)),
                ("sgd_step: momentum 0 with a null buf, n 0", lambda: sgd(n=0, mom=0.0, buf=None)),
                ("nonfinite_flag_f32: n 0", lambda: L.call("pvrl_nonfinite_flag_f32", ptr("g"), 0, ptr("flag"), S()))]
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
    for k, b in bufs.items():
        f += bits_equal(f"{k} and its guard bands after the refused and the empty calls", b.buf, before[k])
    return f


# =====================================================================================================================
# through FusedOptimizer: the padding slots of the flat buffers stay bit-zero
# =====================================================================================================================
class OddSizes(torch.nn.Module):
    """what FusedOptimizer needs of a model (grad_store, adopt_grads), over parameters whose sizes leave padding behind them in the flat
    buffers: the small model of tests/test_optimizer_gpu.py has none (all of its 104 parameter sizes are multiples of 64)"""
    SHAPES = ((1,), (63,), (65,), (3, 7), (1000,), (64,), (129, 5))

    def __init__(self, dev):
        super().__init__()
        g = _gen("odd sizes")
        self.ps = torch.nn.ParameterList([torch.nn.Parameter((torch.randn(s, generator=g) * 0.02).to(dev)) for s in self.SHAPES])
        self._gs = None

    def grad_store(self):
        from procedurevrl_amd.grads import GradStore
        if self._gs is None:
            self._gs = GradStore(list(self.named_parameters()), self.ps[0].device)
        return self._gs

    def adopt_grads(self, keep_none=False, zero_unused=True):
        from procedurevrl_amd.vit import VisionTransformer
        return VisionTransformer.adopt_grads(self, keep_none, zero_unused)


def check_padding_slots(method, which):
    """five steps of FusedOptimizer on `which` = "small_model" (tests/test_optimizer_gpu.py's; it happens to have no padding slot) or
    "odd_sizes" (OddSizes) -> every padding slot of flat_p, buf1 and buf2 is bit-zero"""
    from procedurevrl_amd.optimizer import FusedOptimizer, construct_optimizer, set_lr
    torch.manual_seed(0)
    if which == "small_model":
        import e2e_checks as ec
        from procedurevrl_amd.datasets import synthetic_label_emb
        cfg = ec.make_cfg(2, 32, 64)
        cfg.SOLVER.OPTIMIZING_METHOD = method
        cfg.SOLVER.WEIGHT_DECAY, cfg.BN.WEIGHT_DECAY, cfg.TRAIN.MULT = 1e-2, 3e-3, 0.1
        model = ec.build(cfg, synthetic_label_emb(64, 512, seed=1))
        opt = construct_optimizer(model, cfg)
        gs = model.model.grad_store()
    else:
        model = OddSizes(torch.device("cuda:0"))
        ps = list(model.parameters())
        opt = FusedOptimizer([{"params": ps[:3], "weight_decay": 3e-3, "lr_mult": 0.1}, {"params": ps[3:], "weight_decay": 1e-2, "lr_mult": 1.0}],
                             model, method, lr=1e-3, momentum=0.9, dampening=0.0, nesterov=True, weight_decay=1e-2)
        gs = model.grad_store()
    opt.grad_scale = 0.25
    gen = torch.Generator(device=gs.flat.device).manual_seed(3)
    for step in range(5):
        set_lr(opt, 1e-3 * (1.0 + 0.37 * step))
        opt.zero_grad(set_to_none=True)
        for p, v in zip(gs.params, gs.views):
            v.copy_(torch.randn(v.shape, device=v.device, generator=gen) * 5e-2)
            p.grad = v
        opt.step()
    torch.cuda.synchronize()
    pad = torch.zeros(gs.end, dtype=torch.bool)
    for i, p in enumerate(gs.params):
        a, b = gs.span(i)
        pad[a + p.numel():b] = True
    npad = int(pad.sum())
    f = [Finding("padding slots of the flat buffers", npad > 0 or which == "small_model", float(npad), 1.0,
                 f"{len(gs.params)} parameters, {gs.end} slots")]
    moved = (opt.flat_p[:gs.end].cpu() != 0)[~pad].float().mean().item()
    f.append(Finding("share of the parameter slots that are non-zero after five steps", moved > 0.9, moved, 0.9, ""))
    for name, t in (("flat_p", opt.flat_p), ("buf1", opt.buf1), ("buf2", opt.buf2)):
        if t is not None:
            f += bits_equal(f"{method}: padding slots of {name} against zero", t[:gs.end].cpu()[pad], torch.zeros(npad))
    return f
