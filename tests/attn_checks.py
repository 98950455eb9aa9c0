"""Attention kernels (head_dim 64) vs an fp64 reference, PER ROW: reference, rounding model, metric, input regimes, cases, guard bands.

Used by tests/test_attention_gpu.py (pytest -m gpu: the HIP kernels through procedurevrl_amd.ops) and by
tests/test_attn_harness_host.py (no GPU: the rounding model stands in for the kernel, and planted defects show that the rule bites).

Why not the aggregate norm of tests/kernel_checks.py: the kernels under test are persistent, walk (sequence, head) items and have
ragged last tiles, so their typical bug is LOCAL -- one row, one item, the tail of the last workgroup.  One zeroed row in 208,032
moves the relative L2 norm of the whole tensor by 2e-3, which the 1.5e-2 backward bound cannot see.

Metric.  For every output tensor laid out [item = sequence * H + head][token][64]:
    rowerr = max over rows of ||x_row - ref_row||_2 / N,   N = root mean square of ||ref_row||_2 over the tensor.
(Not divided by the row's own norm: rows whose true gradient vanishes -- peaked softmax -- make that quotient ill-conditioned.)
The aggregate relative L2 error is kept as a second number.  lse: absolute error against fp64 logsumexp.

Tolerance rule -- no free constants.  A tensor passes when rowerr(kernel) <= ROW_FACTOR * rowerr(model) on the same inputs, the model
being oracle/rounded_oracle.AttnMFMA with the library flavour's operand type and outputs rounded to it (attn_t8: fp32 math, outputs
rounded), evaluated on the CPU inside the check.  ROW_FACTOR = 4: two legitimate implementations of the same contract differ by up to
~2.2x in this statistic (AttnMFMA against `model_variant` below, which rounds the normalised P, takes P from lse and D from the
unrounded o: tests/test_attn_harness_host.py keeps that comparison running); 4 leaves that a factor of two and still flags a 1 % error
of one (sequence, head) item in the fp16 flavour.  Where the reference tensor is identically zero (dq when all keys of an item are
equal) max|x| is compared with ROW_FACTOR * max|model| plus the fp32 cancellation floor of `fp32_zero_floor`.  Where a case's tensors have
fewer than MIN_ROWS rows the kernel runs on several draws of the case and the statistics are taken over all of them (`n_draws` says why).
Aggregate L2: the `randn` regime is what tests/kernel_checks.py measures, and keeps its bounds (AGG_FWD / AGG_BWD; attn_t8 backward
TOL_BF16).  Those constants were chosen for N(0, 1) logits and mean nothing for the other regimes (the model's own aggregate dq error
in the `offset` regime is several per cent with bf16 operands), so there the aggregate follows the model like the row statistic does:
agg(kernel) <= ROW_FACTOR * agg(model).
lse: the yardstick is plain fp32 torch.logsumexp of fp32 logits on the CPU against the fp64 value, Y = its largest error over the
tensor; an entry passes when |lse - lse64| <= 8 Y + 4 fp32 ulp of max(1, |lse|) (the kernel uses a fast log and sums in tile order).
"""
import collections
import math

import torch

from oracle import rounded_oracle as rorc
from procedurevrl_amd._lib import OPERAND

BF = torch.bfloat16 if OPERAND == "bf16" else torch.float16
AGG_FWD = 1e-2 if OPERAND == "bf16" else 1.5e-3          # kernel_checks.TOL_BF16
AGG_BWD = 1.5e-2                                          # kernel_checks: the flat backward bound of the attention checks
ROW_FACTOR = 4.0
LSE_FACTOR, LSE_ULPS = 8.0, 4.0
GUARD_ROWS = 4
INPUT_GUARD = 1000.0
# guard pattern: a fixed non-NaN bit pattern per element width (fp16 0.0583 / bf16 2.5e-13 / fp32 0.1674)
PATTERN = {2: 0x2B77, 4: 0x3E2B6701}
FULL_REF_BUDGET = 1.2e7          # items * S * S above which the fp64 reference runs on a subset of the (sequence, head) items
REGIMES = ("randn", "hot", "peaked", "offset", "equal", "one_live")


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "entry mode nseq S H T scale causal pad ldd_extra zero_dq kernel")
# entry: "attn" (pvrl_attn_fwd / _bwd), "cls" (pvrl_attn_cls_fwd / _bwd), "t8" (pvrl_attn_t8_fwd / _bwd).  mode 1: nseq = B * T, S = N + 1.
# ldd_extra: columns of dqkv behind the 3 * H * 64 owned ones (8 keeps ldd % 8 == 0; 4 is the ABI's minimum and takes the two-pass backward).
# kernel: the instantiation(s) the case is meant to reach, "<forward>+<backward>"; names as in the launch_* lines of csrc/attn_mfma.hip:
#   fwd_NKT_NW[_gen][_sS]   attn_fwd_kernel<NKT, GEN, NW, SFIX>             (launch_fwd<NKT, NW>)
#   bwd2p_NKT_NW[_gen][_sS] attn_bwd_q_kernel + attn_bwd_kv_kernel          (launch_bwd<NKT, NW>, the two-pass backward)
#   fused_0 / fused_7       attn_bwd_fused_kernel<0> (96 < S <= 192) / <7>  (pvrl_attn_bwd_fused_launch)
#   s32                     attn_bwd_s32_kernel                             (pvrl_attn_bwd_s32_launch)
#   cls_fwd / cls_bwd, t8_fwd / t8_bwd

POW2 = 0.125
ODD_SCALE = 64 ** -0.5 * 1.1


def _bucket(S):
    for lim, nkt, nw in ((16, 1, 4), (32, 2, 4), (48, 3, 4), (80, 5, 4), (208, 13, 8), (272, 17, 8), (416, 26, 8)):
        if S <= lim:
            return nkt, nw
    raise ValueError(S)


def _is_pow2(x):
    return math.frexp(x)[0] == 0.5


def kernel_names(mode, S, scale, masked, ldd_extra):
    """the dispatch of pvrl_attn_fwd / pvrl_attn_bwd restated (csrc/attn_mfma.hip:531-565, attn_bwd_fused.hip:454, attn_bwd_s32.hip:188);
    test_attn_harness_host.py pins the set of names this table reaches against a hand-written list"""
    nkt, nw = _bucket(S)
    sfix = {13: 197, 2: 32}.get(nkt)
    tail = "_gen" if masked else (f"_s{S}" if sfix == S else "")
    fwd = f"fwd_{nkt}_{nw}{tail}"
    fast = (not masked) and _is_pow2(scale) and ldd_extra % 8 == 0
    if fast and 96 < S <= 224:
        bwd = "fused_7" if S > 192 else "fused_0"
    elif fast and mode == 0 and 16 < S <= 32:
        bwd = "s32"
    else:
        bwd = f"bwd2p_{nkt}_{nw}{tail}"
    return fwd + "+" + bwd


def _attn(mode, nseq, S, H, T=1, scale=POW2, causal=False, pad=False, ldd_extra=8):
    return Case("attn", mode, nseq, S, H, T, scale, causal, pad, ldd_extra, True,
                kernel_names(mode, S, scale, causal or pad, ldd_extra))


def _build_cases():
    cases = []
    # mode 0, unmasked: every bucket edge of the dispatch; nseq not a multiple of 8 with many heads (the grids are 8 * ceil(nseq / 8) * H:
    # the padding items must do nothing)
    s_list = [1, 8, 16, 17, 31, 32, 33, 48, 49, 80, 81, 96, 97, 192, 193, 197, 208, 209, 224, 225, 272, 273, 401, 416]
    for i, S in enumerate(s_list):
        cases.append(_attn(0, (1, 5, 8, 9)[i % 4], S, (1, 3, 12)[i % 3]))
    # a scale that is not a power of two / a dqkv leading dimension of 3 * H * 64 + 4: the two-pass fallbacks, the S-constant ones included
    for i, S in enumerate([24, 32, 100, 197, 224]):
        cases.append(_attn(0, (5, 9, 1, 8, 5)[i], S, (3, 12, 3, 3, 1)[i], scale=ODD_SCALE))
    for S, nseq, H in [(32, 9, 3), (197, 5, 3)]:
        cases.append(_attn(0, nseq, S, H, ldd_extra=4))
    # masked (GEN = true) forms: <1,4> <2,4> <3,4> <5,4> and the 8-wave <13,8>
    kinds = [(True, False), (False, True), (True, True)]
    for i, S in enumerate([2, 16, 17, 32, 33, 48, 77, 81, 130, 197, 208]):
        c, p = kinds[i % 3]
        cases.append(_attn(0, (5, 3, 9, 8, 1, 5, 5, 3, 9, 5, 2)[i], S, (3, 2, 12, 3, 1, 3, 8, 2, 3, 12, 2)[i], causal=c, pad=p))
    cases.append(_attn(0, 3, 197, 2, causal=True, pad=True))
    cases.append(_attn(0, 4, 130, 2, causal=True, pad=False))
    # mode 1 (TimeSformer spatial): T = 1, odd T, T = 16, B = 1; H = 12 where the item count exceeds the persistent backward's grid (256)
    for (B, T, N) in [(1, 1, 196), (2, 3, 196), (1, 16, 49), (3, 8, 196), (11, 8, 196), (1, 2, 256), (2, 4, 100), (5, 4, 207)]:
        H = 12 if 8 * ((B * T + 7) // 8) * 12 > 256 else 2
        cases.append(_attn(1, B * T, N + 1, H, T=T))
    for (B, T, N) in [(1, 1, 1), (2, 4, 16), (3, 8, 196), (1, 2, 255), (2, 3, 400)]:
        H = {196: 12, 255: 3}.get(N, 2)
        for z in (True, False):
            cases.append(Case("cls", 1, B * T, N + 1, H, T, POW2, False, False, 8, z, "cls_fwd+cls_bwd" + ("" if z else "_nodq")))
    for nseq in (1, 37, 6272):
        for H in (1, 12):
            cases.append(Case("t8", 0, nseq, 8, H, 1, POW2, False, False, 8, True, "t8_fwd+t8_bwd"))
    return cases


CASES = _build_cases()


def case_id(c):
    shape = f"n{c.nseq}xS{c.S}xH{c.H}" if c.mode == 0 else f"B{c.nseq // c.T}xT{c.T}xN{c.S - 1}xH{c.H}"
    extra = ("-causal" if c.causal else "") + ("-pad" if c.pad else "") + ("-oddscale" if not _is_pow2(c.scale) else "") + \
            ("-ldd4" if c.ldd_extra == 4 else "")
    return f"{c.entry}-m{c.mode}-{shape}{extra}-{c.kernel}"


def _build_tests():
    """every case runs `randn` and `peaked`; the first case that reaches a forward or a backward kernel not seen before also runs `hot`,
    `offset` and `equal` (and `one_live` when it is a masked form)"""
    tests, seen = [], set()
    for c in CASES:
        regs = ["randn", "peaked"]
        new = [k for k in c.kernel.split("+") if k not in seen]
        if new:
            seen.update(new)
            regs += ["hot", "offset", "equal"]
            if c.causal or c.pad:
                regs.append("one_live")
        tests += [(c, r) for r in regs]
    return tests


TESTS = _build_tests()


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _rnd(x, dt):
    return x.to(dt).float()


def make_problem(c, regime, operand=None, seed=None):
    """-> dict: qkv [rows, 3 H 64] and do ([rows_o, H 64]) fp32 CPU tensors already rounded to the operand type, kpm (bool [nseq, S] or
    None), in the packed layouts of include/pvrl.h (mode 1: patch rows (b, n, t), then the B cls rows; do: patch rows, then nseq cls rows)."""
    operand = BF if operand is None else operand
    if seed is None:        # one fixed stream per (shape, regime)
        seed = 100000 + ((((c.mode * 9973 + c.nseq) * 431 + c.S) * 13 + c.H) * 17 + c.T) * 7 + REGIMES.index(regime)
    g = torch.Generator().manual_seed(seed)
    HD = c.H * 64
    if c.mode == 0:
        rows, groups, R, B = c.nseq * c.S, c.nseq, c.nseq * c.S, 0
    else:
        B = c.nseq // c.T
        R = B * (c.S - 1) * c.T
        rows, groups = R + B, B
    qkv = torch.randn(rows, 3, c.H, 64, generator=g)
    if regime == "hot":
        qkv[:, :2] *= 2.0
    elif regime == "peaked":
        qkv[:, :2] *= 3.5
    elif regime in ("offset", "equal"):
        # one vector per (group, head): group = sequence (mode 0) or clip (mode 1: its T sequences share the cls key row)
        vec = torch.randn(groups, c.H, 64, generator=g)
        if regime == "offset":
            vec = torch.where(vec > 0, 8.0, -8.0)
        if c.mode == 0:
            grp = torch.arange(rows) // c.S
        else:
            grp = torch.cat([torch.arange(R) // ((c.S - 1) * c.T), torch.arange(B)])
        qkv[:, 1] = vec[grp] + (qkv[:, 1] if regime == "offset" else 0.0)
    qkv = _rnd(qkv.reshape(rows, 3 * HD), operand)
    rows_o = R + (c.nseq if c.mode == 1 else 0)
    if c.entry == "cls":
        rows_o = c.nseq
    do = _rnd(torch.randn(rows_o, HD, generator=g), operand)
    kpm = None
    if regime == "one_live":
        kpm = torch.ones(c.nseq, c.S, dtype=torch.bool)
        kpm[:, 0] = False
    elif c.pad:
        kpm = torch.zeros(c.nseq, c.S, dtype=torch.bool)
        for i in range(1, c.nseq):          # sequence 0 keeps every key; no row is ever fully masked (key 0 always stays)
            kpm[i, 1 + int(torch.randint(0, c.S - 1, (1,), generator=g)):] = True
    return dict(qkv=qkv, do=do, kpm=kpm, R=R, B=B)


def gather(c, tok, cls, parts, shared_cls):
    """packed rows -> [parts, nseq * H, S, 64].  mode 1 exactly like vit.py:139-143 / kernel_checks.check_attn_mfma_spatial; `cls`: the B
    shared cls rows (inputs: expanded over T) or nseq per-sequence rows (the *_cls side buffers)."""
    HD = c.H * 64
    if c.mode == 0:
        x = tok.reshape(c.nseq, c.S, parts, c.H, 64)
    else:
        B, N, T = c.nseq // c.T, c.S - 1, c.T
        t = tok.reshape(B, N, T, parts * HD).permute(0, 2, 1, 3)                 # b t n c
        k = cls.reshape(B, 1, 1, parts * HD).expand(B, T, 1, parts * HD) if shared_cls else cls.reshape(B, T, 1, parts * HD)
        x = torch.cat([k, t], 2).reshape(c.nseq, c.S, parts, c.H, 64)
    return x.permute(2, 0, 3, 1, 4).reshape(parts, c.nseq * c.H, c.S, 64)


def choose_items(c, seed=7):
    """all (sequence, head) items when the fp64 reference fits the time budget, else the first, the last and 8 seeded-random ones"""
    n = c.nseq * c.H
    if n * c.S * c.S <= FULL_REF_BUDGET or n <= 10:
        return torch.arange(n)
    g = torch.Generator().manual_seed(seed)
    mid = 1 + torch.randperm(n - 2, generator=g)[:8]
    return torch.cat([torch.tensor([0]), mid.sort().values, torch.tensor([n - 1])])


def gathered_inputs(c, prob, items):
    """q, k, v, do [n_items, S, 64] fp32 and the bool mask [n_items, S, S] (True = not seen) or None"""
    R = prob["R"]
    qkv = gather(c, prob["qkv"][:R] if c.mode == 1 else prob["qkv"], prob["qkv"][R:] if c.mode == 1 else None, 3, True)[:, items]
    if c.entry == "cls":            # dO is zero for every patch query
        do = torch.zeros(len(items), c.S, 64)
        do[:, 0] = prob["do"].reshape(c.nseq * c.H, 64)[items]
    else:
        do = gather(c, prob["do"][:R] if c.mode == 1 else prob["do"], prob["do"][R:] if c.mode == 1 else None, 1, False)[0, items]
    mask = None
    if c.causal or prob["kpm"] is not None:
        mask = torch.zeros(len(items), c.S, c.S, dtype=torch.bool)
        if c.causal:
            mask |= torch.triu(torch.ones(c.S, c.S, dtype=torch.bool), 1)
        if prob["kpm"] is not None:
            mask |= prob["kpm"][items // c.H][:, None, :]
    return qkv[0], qkv[1], qkv[2], do, mask


# ---------------------------------------------------------------------------------------------------------------------
# reference, rounding models
# ---------------------------------------------------------------------------------------------------------------------
def _chunks(n, S):
    step = max(1, int(2e6 // (S * S)))
    return [slice(i, min(n, i + step)) for i in range(0, n, step)]


def _cat(parts):
    return {k: torch.cat([p[k] for p in parts]) for k in parts[0]}


def reference(q, k, v, do, scale, mask):
    """fp64 autograd of softmax(q k^T * scale [+ mask]) v -> o, lse, dq, dk, dv (fp64), and lse32 = the fp32 yardstick's logsumexp"""
    out = []
    for sl in _chunks(q.shape[0], q.shape[1]):
        qd, kd, vd = (t[sl].double().requires_grad_(True) for t in (q, k, v))
        s = (qd @ kd.transpose(-1, -2)) * scale
        if mask is not None:
            s = s.masked_fill(mask[sl], float("-inf"))
        o = torch.softmax(s, -1) @ vd
        o.backward(do[sl].double())
        s32 = (q[sl] @ k[sl].transpose(-1, -2)) * scale
        if mask is not None:
            s32 = s32.masked_fill(mask[sl], float("-inf"))
        out.append(dict(o=o.detach(), lse=torch.logsumexp(s.detach(), -1), dq=qd.grad, dk=kd.grad, dv=vd.grad,
                        lse32=torch.logsumexp(s32, -1)))
    return _cat(out)


def model(q, k, v, do, scale, mask, operand, kind="mfma"):
    """the kernels' rounding model: oracle/rounded_oracle.AttnMFMA with OPERAND = the operand type, outputs rounded to it; kind "t8":
    fp32 math, only the outputs rounded (rounded_oracle.attention_core(mfma=False))"""
    out = []
    with rorc.operand(operand):
        for sl in _chunks(q.shape[0], q.shape[1]):
            ql, kl, vl = (t[sl].clone().requires_grad_(True) for t in (q, k, v))
            m = None if mask is None else mask[sl]
            if kind == "mfma":
                o = rorc.AttnMFMA.apply(ql, kl, vl, scale, m)
            else:
                s = (ql @ kl.transpose(-1, -2)) * scale
                if m is not None:
                    s = s.masked_fill(m, float("-inf"))
                o = torch.softmax(s, -1) @ vl
            o.backward(do[sl])
            out.append(dict(o=_rnd(o.detach(), operand), dq=_rnd(ql.grad, operand), dk=_rnd(kl.grad, operand), dv=_rnd(vl.grad, operand)))
    return _cat(out)


def model_variant(q, k, v, do, scale, mask, operand):
    """another legitimate implementation of the same contract: the NORMALISED P is rounded for the second product, the backward takes P
    from lse and D from the unrounded o.  What the tolerance rule must let pass (test_attn_harness_host.py)."""
    out = []
    for sl in _chunks(q.shape[0], q.shape[1]):
        ql, kl, vl, dl = q[sl], k[sl], v[sl], do[sl]
        s = (ql @ kl.transpose(-1, -2)) * scale
        if mask is not None:
            s = s.masked_fill(mask[sl], float("-inf"))
        lse = torch.logsumexp(s, -1, keepdim=True)
        p = torch.exp(s - lse)
        o = _rnd(p, operand) @ vl
        dp = dl @ vl.transpose(-1, -2)
        d = (dl * o).sum(-1, keepdim=True)
        ds = _rnd(p * (dp - d) * scale, operand)
        out.append(dict(o=_rnd(o, operand), dq=_rnd(ds @ kl, operand), dk=_rnd(ds.transpose(-1, -2) @ ql, operand),
                        dv=_rnd(_rnd(p, operand).transpose(-1, -2) @ dl, operand)))
    return _cat(out)


# ---------------------------------------------------------------------------------------------------------------------
# metric and verdicts
# ---------------------------------------------------------------------------------------------------------------------
def rowerr(x, ref):
    """-> (max over rows of ||x_row - ref_row|| / rms of ||ref_row||, flat index of the worst row); x, ref [..., W], a row = the last dimension;
    inf when x is not finite"""
    x, ref = x.double().reshape(-1, x.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    e = (x - ref).pow(2).sum(-1).sqrt()
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
    i = int(e.argmax())
    return e[i].item() / row_rms(ref), i


def row_rms(ref):
    return max(ref.double().reshape(-1, ref.shape[-1]).pow(2).sum(-1).mean().sqrt().item(), 1e-300)


def agg(x, ref):
    d = (x.double() - ref.double()).norm().item()
    return d / max(ref.double().norm().item(), 1e-300) if math.isfinite(d) else float("inf")


Finding = collections.namedtuple("Finding", "tensor ok value bound detail")


def _where(c, items, flat, S):
    """items: flat (sequence, head) indices; a further draw d of a small case (`n_draws`) counts on from d * nseq * H"""
    draw, item = divmod(int(items[flat // S]), c.nseq * c.H)
    return f"(sequence {item // c.H}, head {item % c.H}, token {flat % S}" + (f"; draw {draw})" if draw else ")")


def judge_tensor(c, name, x, ref, mod, items, agg_bound, zero_floor=0.0, where=None):
    """the tolerance rule of the module docstring for one output tensor [n_items, S', W] (a row = one vector of W: 64 here, 96 / J in
    tests/pool_attn_checks.py) -> [Finding, Finding] (row statistic, aggregate).
    agg_bound: a number (the `randn` regime: today's flat bound) or None (follow the model).  zero_floor: see `fp32_zero_floor`.
    where: (flat row index, rows per item) -> text naming the row, for cases that are not a `Case` (default: `_where` of c, items)."""
    S = x.shape[1]
    loc = where if where is not None else (lambda flat, S: _where(c, items, flat, S))
    if ref.abs().max().item() < 1e-10:          # identically zero reference (dq with equal keys): absolute comparison with the model
        xm, mm = x.abs().max().item(), mod.abs().max().item()
        xm = xm if math.isfinite(xm) else float("inf")
        i = int(torch.nan_to_num(x.abs().reshape(-1, x.shape[-1]).amax(-1), nan=float("inf")).argmax())
        bound = ROW_FACTOR * mm + zero_floor
        return [Finding(name + " max|x| (zero reference)", xm <= bound, xm, bound,
                        f"model max {mm:.3e}, fp32 floor {zero_floor:.1e}, ratio {xm / max(mm, 1e-300):.2f}, worst row {loc(i, S)}")]
    rk, i = rowerr(x, ref)
    rm, _ = rowerr(mod, ref)
    ak, am = agg(x, ref), agg(mod, ref)
    ab = ROW_FACTOR * am if agg_bound is None else agg_bound
    return [Finding(name + " rowerr", rk <= ROW_FACTOR * rm, rk, ROW_FACTOR * rm,
                    f"model rowerr {rm:.3e}, ratio {rk / max(rm, 1e-300):.2f}, worst row {loc(i, S)}"),
            Finding(name + " aggregate L2", ak <= ab, ak, ab, f"model aggregate {am:.3e}, ratio {ak / max(am, 1e-300):.2f}")]


def judge_lse(c, lse, ref, items, where=None):
    """lse [n_items, S'] against ref["lse"] (fp64), yardstick ref["lse32"]; where: as in `judge_tensor`"""
    S = lse.shape[1]
    loc = where if where is not None else (lambda flat, S: _where(c, items, flat, S))
    r64, r32 = ref["lse"][:, :S], ref["lse32"][:, :S]
    y = (r32.double() - r64).abs().max().item()
    ulp = torch.exp2(torch.floor(torch.log2(r64.abs().clamp_min(1.0))) - 23)
    err = (lse.double() - r64).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    slack = err - (LSE_FACTOR * y + LSE_ULPS * ulp)
    i = int(slack.argmax())
    e, b = err.reshape(-1)[i].item(), (LSE_FACTOR * y + LSE_ULPS * ulp).reshape(-1)[i].item()
    return [Finding("lse abs error", e <= b, e, b, f"fp32 yardstick {y:.3e}, max error {err.max().item():.3e}, worst entry {loc(i, S)}")]


def agg_bounds(c, regime, operand=None):
    """today's flat aggregate bounds in the regime they were made for, else None = follow the model"""
    if regime != "randn":
        return None, None
    fwd = AGG_FWD if operand is None else (1e-2 if operand == torch.bfloat16 else 1.5e-3)
    return fwd, (fwd if c.entry == "t8" else AGG_BWD)


def fp32_zero_floor(q, k, v, do, scale):
    """Where the true dq / dk is identically zero (equal keys, one live key, S = 1) the kernel's and the model's values are pure
    cancellation noise of dS = P * (dP - D) * scale, and either may happen to be exactly zero.  dP and D are 64-term fp32 dot products of
    magnitude <= A = max_ij sum_d |dO_id| |V_jd| summed in different orders, so |dP - D| carries up to 64 * 2^-24 * A = 2^-18 A of fp32
    noise whatever the implementation; dq_i = sum_j dS_ij k_j with sum_j P_ij = 1, dk_j = sum_i dS_ij q_i with sum_i P_ij <= S.
    -> additive floors for the zero-reference comparison of dq and dk."""
    a = (do.abs() @ v.abs().transpose(-1, -2)).max().item()
    base = scale * 2.0 ** -18 * a
    return {"dq": base * k.abs().max().item(), "dk": base * q.abs().max().item() * q.shape[1]}


MIN_ROWS = 4 * 3 * 32


def n_draws(c):
    """Small cases.  rowerr is a maximum over rows and the rule compares two such maxima; the aggregate is a quotient of two norms.  Over a
    handful of rows neither has a stable value: the cls-query backward at S = 2, H = 2 has TWO dq rows, whose error is one draw of
    (D - rowsum(dO * O_stored)) * scale * sum_j P_j k_j -- the contract's own rounding of the stored o.  On the GPU that sat at 21x the
    model's two draws in the `offset` regime while equal to the model's typical value there, and at 1.7e-2 aggregate with bf16 operands on
    N(0, 1) logits where the model itself reaches 9e-2 on some draws and 4e-3 over 192 of them.  So a case whose smallest compared tensor has
    fewer than MIN_ROWS rows (the smallest tensor over which the factor 4 is validated in test_attn_harness_host.py: 4 sequences x 3
    heads x 32 tokens) is run through the kernel on as many seeded draws as it takes to reach MIN_ROWS (at most 256), and every
    statistic -- kernel's, model's, reference norms -- is taken over all draws together: same inputs for both, same bounds."""
    rows = c.nseq * c.H * (1 if c.entry == "cls" else c.S)
    return 1 if rows >= MIN_ROWS else min(256, -(-MIN_ROWS // rows))


def judge(c, regime, got, ref, mod, items, inputs=None, operand=None):
    """got: o [n, S or 1, 64], lse [n, S or 1] or None, dq, dk, dv -> list of Finding.  inputs: (q, k, v, do) for fp32_zero_floor;
    operand: the 16-bit type whose aggregate bounds apply (default: the library flavour's)."""
    fwd_b, bwd_b = agg_bounds(c, regime, operand)
    floor = fp32_zero_floor(*inputs, c.scale) if inputs is not None else {}
    out = []
    for name in ("o", "dq", "dk", "dv"):
        s = got[name].shape[1]
        out += judge_tensor(c, name, got[name], ref[name][:, :s], mod[name][:, :s], items, fwd_b if name == "o" else bwd_b,
                            floor.get(name, 0.0))
    if got.get("lse") is not None:
        out += judge_lse(c, got["lse"], ref, items)
    return out


def report(findings):
    return "\n".join(f"{'ok  ' if f.ok else 'FAIL'} {f.tensor}: {f.value:.3e} (bound {f.bound:.3e}); {f.detail}" for f in findings)


# ---------------------------------------------------------------------------------------------------------------------
# guard bands
# ---------------------------------------------------------------------------------------------------------------------
class Guarded:
    """Output segments (row ranges) inside one larger buffer: GUARD_ROWS rows in front of, between and behind the segments and `extra_cols`
    columns to the right hold PATTERN; owned elements start as NaN.  `unowned` = [(segment, row0, row1, col0, col1)] ranges inside a
    segment that the header declares untouched: they hold the pattern and must keep it.  check() -> [Finding]."""

    def __init__(self, name, segs, cols, dtype, extra_cols=0, unowned=(), device="cpu"):
        self.name, self.cols, self.dtype = name, cols, dtype
        self.idt = {2: torch.int16, 4: torch.int32}[torch.empty(0, dtype=dtype).element_size()]
        pat = PATTERN[torch.empty(0, dtype=dtype).element_size()]
        total = GUARD_ROWS + sum(n + GUARD_ROWS for n in segs)
        ibuf = torch.full((total, cols + extra_cols), pat, dtype=self.idt)
        self.owned = torch.zeros(total, cols + extra_cols, dtype=torch.bool)
        self.rows = []
        r = GUARD_ROWS
        for n in segs:
            self.owned[r:r + n, :cols] = True
            self.rows.append((r, n))
            r += n + GUARD_ROWS
        for (sg, r0, r1, c0, c1) in unowned:
            self.owned[self.rows[sg][0] + r0:self.rows[sg][0] + r1, c0:c1] = False
        ibuf.view(dtype)[self.owned] = float("nan")
        self.before = ibuf
        self.buf = ibuf.clone().to(device).view(dtype)

    def seg(self, i):
        r, n = self.rows[i]
        return self.buf[r:r + n, :self.cols]

    def check(self):
        after = self.buf.view(self.idt).cpu()
        touched = (after != self.before) & ~self.owned
        nt = int(touched.sum())
        where = tuple(int(v) for v in touched.nonzero()[0]) if nt else None
        bad = ~torch.isfinite(after.view(self.dtype).float()) & self.owned
        nb = int(bad.sum())
        wb = tuple(int(v) for v in bad.nonzero()[0]) if nb else None
        return [Finding(f"{self.name}: elements outside the owned rows / columns that changed", nt == 0, float(nt), 0.0,
                        f"first at buffer (row, column) {where}; segments start at rows {[r for r, _ in self.rows]}"),
                Finding(f"{self.name}: owned elements left NaN / not finite", nb == 0, float(nb), 0.0, f"first at buffer (row, column) {wb}")]


def guarded_input(x, dtype, device, extra_cols=8):
    """x [rows, cols] followed by GUARD_ROWS rows and `extra_cols` columns holding INPUT_GUARD: a read past the end shows in the numbers"""
    buf = torch.full((x.shape[0] + GUARD_ROWS, x.shape[1] + extra_cols), INPUT_GUARD)
    buf[:x.shape[0], :x.shape[1]] = x
    return buf.to(device, dtype)[:x.shape[0], :x.shape[1]]


# ---------------------------------------------------------------------------------------------------------------------
# the kernels (GPU)
# ---------------------------------------------------------------------------------------------------------------------
def run_kernels(c, prob, items):
    """the case through procedurevrl_amd.ops on cuda:0 -> (got, guard findings); got in the gathered layout, restricted to `items`"""
    from procedurevrl_amd import ops
    dev = torch.device("cuda:0")
    HD, R, B, S, nseq, H = c.H * 64, prob["R"], prob["B"], c.S, c.nseq, c.H
    qd = guarded_input(prob["qkv"], BF, dev)
    dod = guarded_input(prob["do"], BF, dev)
    kd = prob["kpm"].to(torch.uint8).to(dev) if prob["kpm"] is not None else None
    f = []
    cpu = lambda t: t.float().cpu()
    if c.entry == "t8":
        ob = Guarded("o", [nseq * 8], HD, BF, 8, device=dev)
        ops.attn_t8_fwd(qd, nseq, H, c.scale, out=ob.seg(0))
        db = Guarded("dqkv", [nseq * 8], 3 * HD, BF, 8, device=dev)
        ops.attn_t8_bwd(qd, dod, nseq, H, c.scale, dqkv=db.seg(0))
        torch.cuda.synchronize()
        f += ob.check() + db.check()
        dg = gather(c, cpu(db.seg(0)), None, 3, False)[:, items]
        return dict(o=gather(c, cpu(ob.seg(0)), None, 1, False)[0, items], lse=None, dq=dg[0], dk=dg[1], dv=dg[2]), f
    if c.entry == "cls":
        ob = Guarded("o_cls", [nseq], HD, BF, 8, device=dev)
        lb = Guarded("lse", [nseq * H], S, torch.float32, 0, unowned=[(0, 0, nseq * H, 1, S)], device=dev)
        ops.attn_cls_fwd(qd, nseq, S, H, c.scale, c.T, R, o_cls=ob.seg(0), lse=lb.seg(0).view(nseq, H, S))
        un = [(0, R, R + B, 0, 3 * HD)] + ([] if c.zero_dq else [(0, 0, R, 0, HD)])
        db = Guarded("dqkv / dqkv_cls", [R + B, nseq], 3 * HD, BF, 8, unowned=un, device=dev)
        ops.attn_cls_bwd(qd, ob.seg(0), dod, lb.seg(0).view(nseq, H, S), nseq, S, H, c.scale, c.T, R, db.seg(0), db.seg(1),
                         zero_patch_dq=c.zero_dq)
        torch.cuda.synchronize()
        f += ob.check() + lb.check() + db.check()
        dg = gather(c, cpu(db.seg(0))[:R], cpu(db.seg(1)), 3, False)[:, items]
        return dict(o=cpu(ob.seg(0)).reshape(nseq * H, 1, 64)[items], lse=cpu(lb.seg(0))[items, :1],
                    dq=dg[0] if c.zero_dq else dg[0][:, :1], dk=dg[1], dv=dg[2]), f
    m1 = c.mode == 1
    ntok = R if m1 else nseq * S
    ob = Guarded("o / o_cls", [ntok] + ([nseq] if m1 else []), HD, BF, 8, device=dev)
    lb = Guarded("lse", [nseq * H], S, torch.float32, 0, device=dev)
    lse = lb.seg(0).view(nseq, H, S)
    ops.attn_fwd(qd, nseq, S, H, c.scale, mode=c.mode, T=c.T, cls_base=R, causal=c.causal, kpm=kd, o=ob.seg(0),
                 o_cls=ob.seg(1) if m1 else None, lse=lse)
    db = Guarded("dqkv / dqkv_cls", [ntok + B] + ([nseq] if m1 else []), 3 * HD, BF, c.ldd_extra,
                 unowned=[(0, R, R + B, 0, 3 * HD)] if m1 else (), device=dev)
    ops.attn_bwd(qd, ob.seg(0), ob.seg(1) if m1 else None, dod[:ntok], dod[ntok:] if m1 else None, lse, nseq, S, H, c.scale, mode=c.mode,
                 T=c.T, cls_base=R, causal=c.causal, kpm=kd, dqkv=db.seg(0), dqkv_cls=db.seg(1) if m1 else None)
    torch.cuda.synchronize()
    f += ob.check() + lb.check() + db.check()
    og = gather(c, cpu(ob.seg(0)), cpu(ob.seg(1)) if m1 else None, 1, False)[0, items]
    dg = gather(c, cpu(db.seg(0))[:ntok], cpu(db.seg(1)) if m1 else None, 3, False)[:, items]
    return dict(o=og, lse=cpu(lb.seg(0))[items], dq=dg[0], dk=dg[1], dv=dg[2]), f


def check_case(c, regime):
    """one case x regime on the GPU -> list of Finding (guard bands, then the tolerance rule per tensor); small cases: `n_draws` draws"""
    items = choose_items(c)
    kind = "t8" if c.entry == "t8" else "mfma"
    findings, parts = [], []
    for d in range(n_draws(c)):
        prob = make_problem(c, regime, seed=None if d == 0 else d)
        got, guards = run_kernels(c, prob, items)
        findings += [f for f in guards if d == 0 or not f.ok]
        q, k, v, do, mask = gathered_inputs(c, prob, items)
        ref = reference(q, k, v, do, c.scale, mask)
        mod = model(q, k, v, do, c.scale, mask, BF, kind)
        parts.append((got, ref, mod, dict(q=q, k=k, v=v, do=do), items + d * c.nseq * c.H))
    got, ref, mod, inp = ({key: (torch.cat([p[j][key] for p in parts]) if parts[0][j][key] is not None else None) for key in parts[0][j]}
                          for j in range(4))
    return findings + judge(c, regime, got, ref, mod, torch.cat([p[4] for p in parts]), (inp["q"], inp["k"], inp["v"], inp["do"]))


def check_masked_too_long():
    """S = 209 with a mask: PVRL_EINVAL from both entry points, nothing is launched -> list of Finding"""
    from procedurevrl_amd import ops
    from procedurevrl_amd._lib import PvrlError
    dev = torch.device("cuda:0")
    nseq, S, H = 2, 209, 2
    qd = torch.zeros(nseq * S, 3 * H * 64, device=dev, dtype=BF)
    od = torch.zeros(nseq * S, H * 64, device=dev, dtype=BF)
    lse = torch.zeros(nseq, H, S, device=dev)
    kpm = torch.zeros(nseq, S, dtype=torch.uint8, device=dev)
    out = []
    for name, kw in (("causal", dict(causal=True)), ("key padding", dict(kpm=kpm))):
        for what, call in (("fwd", lambda: ops.attn_fwd(qd, nseq, S, H, POW2, **kw)),
                           ("bwd", lambda: ops.attn_bwd(qd, od, None, od, None, lse, nseq, S, H, POW2, **kw))):
            try:
                call()
                msg = "returned 0"
            except PvrlError as e:
                msg = str(e)
            out.append(Finding(f"pvrl_attn_{what} S=209 {name}: status", msg.endswith("status -1"), 0.0, 0.0, msg))
    return out
