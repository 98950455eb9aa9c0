"""MViTv2 pooling attention (csrc/attn_pool.hip: pvrl_mvit_attn_fwd / _bwd) and the decomposed relative-position kernels
(csrc/mvit_rel.hip: pvrl_mvit_rel_fwd / _bwd) vs an fp64 reference, PER ROW, through every dispatch path, inside guard bands.

Used by tests/test_pool_attention_gpu.py (pytest -m gpu: the HIP kernels through the C ABI) and tests/test_pool_attn_harness_host.py (no
GPU: the rounding model stands in for the kernel, planted defects show that the rule bites).  Metric, tolerance rule, guard bands and
the small-case rule are those of tests/attn_checks.py (read its docstring first); only what differs is said here.

Reference.  fp64 autograd of softmax(scale q k^T + bias) v (+ q for patch queries), head_dim 96, the cls token LAST on both sides.  The
bias is rel [BH, Lq, J] times the 0/1 key map E [Lk, J] (j = h(key), kh + w(key), kh + kw + t(key)) -- what mvit_checks._attn_ref
builds by indexing -- for patch queries x patch keys only.  In the attention cases rel is DEFINED as the value of the 16-bit pair the
kernel is handed, (hi + lo) * scale, so reference, model and kernel see the same numbers; in the chain cases rel = Q . R_j(q) from the
three tables and the reference differentiates through rel and attention together.
Rounding model (`pool_model`).  logits = scale * (q.k + (hi + lo).E) in fp32; the UNNORMALISED exp is rounded to the operand type for
the second product, o = R(acc / l + q); D from the stored o minus q; dS = R(P (dP - D)) (not pre-multiplied by scale);
dq = R(scale dS K + dO), dk = R(scale dS^T Q), dv = R(R(P)^T dO), drel = dS E in fp32.  `model_variant`: the NORMALISED P is rounded
and D comes from the unrounded o -- another legitimate implementation that the rule must let pass (host test).
Rows.  o, dq, dk, dv: one (item, token) vector of 96.  drel: one (item, query) vector of J.  delta: one entry.  Rule: rowerr(kernel)
<= 4 rowerr(model), aggregate <= the flat bounds of mvit_checks.check_mvit_attention in `randn` (6e-3 forward, 1.5e-2 backward) and
<= 4 agg(model) elsewhere (delta, which those checks never bounded: 4 agg(model) everywhere).  lse: the kernel stores a BASE-2 logarithm; lse * ln 2 against fp64 with attn_checks.judge_lse.
Rel kernels.  Model = fp32 math in which every table entry (forward) and every drel entry (table gradient) is replaced by its hi + lo
16-bit pair, the forward's output passed through the pair it is stored as; the chained dQ is R(dq_attn) + drel . R rounded once.  A
tensor passes when rowerr <= max(4 model, 8 Y), Y = the row error of plain fp32 einsum against fp64 (in the fp16 flavour the pair is
nearly exact and only the summation order is left).  The dR tables are ACCUMULATED into: they start from a non-zero value and are
compared with start + gradient.
Regimes.  randn, hot, peaked, offset as in attn_checks (rel scales along with q and k); `equal`: all keys of an item equal and rel = 0
(dq = dO on patch rows and 0 on the cls row: the attention term is pure cancellation; v still differs per key, so dk and drel are NOT
zero and take the normal rule -- should a reference tensor be identically zero, judge_tensor's zero-reference floor applies);
`bias_only`: all keys equal and rel ~ 6 N(0, 1), the softmax is decided by the key map alone.
"""
import collections
import math
import zlib

import torch
import torch.nn.functional as F

import attn_checks as ac
from attn_checks import Finding, Guarded, guarded_input, rowerr, agg, ROW_FACTOR, MIN_ROWS, report  # noqa: F401 (re-exported)
from oracle import mvit_oracle as mo
from oracle import mvit_rounded_oracle as mro

BF = ac.BF
D = 96
SCALE = 96 ** -0.5
AGG_FWD, AGG_BWD = 6e-3, 1.5e-2          # mvit_checks.check_mvit_attention
REL_Y_FACTOR = 8.0
LN2 = math.log(2.0)
REGIMES = ("randn", "hot", "peaked", "offset", "equal", "bias_only")
WS_TAIL, WS_FILL = 4096, 0x5A            # bytes behind the advertised workspace size that must keep their fill


def _rnd(x, dt):
    return x.to(dt).float()


# ---------------------------------------------------------------------------------------------------------------------
# cases and the dispatch restated
# ---------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "kind B H Lq q_thw k_thw ldo_extra misaligned kernel")
# kind "attn": pvrl_mvit_attn_fwd / _bwd on a packed random bias (Lq is free there, q_thw None).  kind "rel": pvrl_mvit_rel_fwd / _bwd on
# their own, then the chain rel_fwd(out_scale = 1 / scale) -> attn_fwd -> attn_bwd -> rel_bwd adding into the 16-bit dQ, as the engine runs
# it.  ldo_extra: columns of o / d_o behind the H * 96 owned ones.  misaligned: the three tables are views 4 bytes off a 16-byte boundary.
# kernel: "+"-joined instantiations the case is meant to reach:
#   fwd<1|2>  bwd_q<1|2>          pattn_fwd_kernel<NJS> / pattn_bwd_q_kernel<NJS>, NJS = 1 for kh + kw + kt <= 32 (JP = 32), else 2
#   bwd_kv<1|2>.z<nsplit>         pattn_bwd_kv_kernel<NJS> on nsplit query slices + pattn_kv_reduce_kernel summing them
#   rel_fwd                       rel_fwd_kernel
#   rel_bwd_q_lds / _gather       rel_bwd_q_kernel<12, true> (tables in LDS) / <12, false>
#   rel_table.c<chunks>           rel_bwd_table_kernel + rel_table_reduce_kernel, chunks = the largest chunks[a] of the three axes


def attn_names(Lq, k_thw):
    """pvrl_mvit_attn_fwd / _bwd: JP = pvrl_mvit_rel_width (attn_pool.hip: fill, kv_splits)"""
    njs = 1 if sum(k_thw) <= 32 else 2
    z = min(16, max(1, (Lq + 1 + 2047) // 2048))
    return [f"fwd{njs}", f"bwd_q{njs}", f"bwd_kv{njs}.z{z}"]


def rel_chunks(BH, q_thw):
    """mvit_rel.hip: rel_axes -> (per, chunks of the height, width, time axis)"""
    NQ = BH * q_thw[0] * q_thw[1] * q_thw[2]
    per = min(8192, max(512, (3 * NQ // 1536 + 127) // 128 * 128))
    return per, [-(-(NQ // qn) // per) for qn in (q_thw[1], q_thw[2], q_thw[0])]


def table_rows(q_thw, k_thw):
    """rows of rel_pos_h, rel_pos_w, rel_pos_t"""
    return [2 * max(q_thw[a], k_thw[a]) - 1 for a in (1, 2, 0)]


def rel_names(BH, q_thw, k_thw, misaligned):
    """pvrl_mvit_rel_fwd / _bwd (mvit_rel.hip: the RELQ_MAXROWS / RELQ_MAXIDX / alignment test of pvrl_mvit_rel_bwd)"""
    lds = sum(table_rows(q_thw, k_thw)) <= 240 and all(q * k <= 1024 for q, k in zip(q_thw, k_thw)) and not misaligned
    return ["rel_fwd", "rel_bwd_q_lds" if lds else "rel_bwd_q_gather", f"rel_table.c{max(rel_chunks(BH, q_thw)[1])}"]


def pad128(n):
    return (n + 127) // 128 * 128


def _attn(B, H, Lq, k_thw, ldo_extra=None):
    ldo_extra = pad128(H * D) - H * D if ldo_extra is None else ldo_extra          # default: the engine's leading dimension
    return Case("attn", B, H, Lq, None, k_thw, ldo_extra, False, "+".join(attn_names(Lq, k_thw)))


def _rel(B, H, q_thw, k_thw, misaligned=False):
    Lq = q_thw[0] * q_thw[1] * q_thw[2]
    return Case("rel", B, H, Lq, q_thw, k_thw, pad128(H * D) - H * D, misaligned,
                "+".join(rel_names(B * H, q_thw, k_thw, misaligned) + attn_names(Lq, k_thw)))


def _build_cases():
    c = []
    # tile edges: Lq = 1 / Lk = 1; Lq + 1 = 64; Lq = 64 (the cls query alone in a second tile) with Lk + 1 = 64; Lk + 1 = 33; Lk + 1 = 65
    c += [_attn(1, 1, 1, (1, 1, 1)), _attn(3, 3, 63, (1, 3, 5)), _attn(1, 2, 64, (1, 7, 9)), _attn(2, 1, 65, (2, 4, 4)),
          _attn(1, 1, 100, (4, 4, 4))]
    # the XCD launch order: BH = 17 (grid padded to 24), 9 (above) and 8 (below)
    c += [_attn(17, 1, 40, (1, 3, 5))]
    # J = 32 (last JP = 32 form), 33 (first NJS = 2 form), 38 (the largest the ABI can reach), 1,569 keys, the production geometry
    c += [_attn(2, 4, 130, (2, 15, 15)), _attn(1, 3, 130, (3, 15, 15)), _attn(1, 2, 70, (6, 16, 16)), _attn(1, 1, 200, (7, 16, 14)),
          _attn(1, 2, 392, (8, 14, 14))]
    # dK / dV query slices: 1, 2, 3 (uneven), 17 clamped to 16; 2 slices with NJS = 2
    c += [_attn(1, 2, 2047, (1, 3, 5)), _attn(1, 2, 2048, (1, 3, 5)), _attn(1, 1, 4100, (1, 3, 5)), _attn(1, 1, 32800, (1, 3, 5)),
          _attn(1, 2, 2500, (7, 16, 14))]
    # ldo: H * 96 exactly, padded to 128, H * 96 + 8
    c += [_attn(1, 4, 40, (1, 3, 5), 0), _attn(2, 1, 40, (1, 3, 5), 32), _attn(2, 2, 40, (1, 3, 5), 8)]
    # rel + chain: the three geometries of mvit_checks.check_mvit_maxpool_rel with BH = 9; 3 chunks of 512, 512, 128 on the time axis;
    # 2 chunks, the last of 63 queries; 255 table rows (gather form); misaligned tables (gather form); q_n < k_n; production block geometry
    c += [_rel(3, 3, (2, 8, 8), (2, 2, 2)), _rel(3, 3, (2, 4, 4), (2, 4, 4)), _rel(3, 3, (3, 4, 8), (3, 4, 2)),
          _rel(1, 2, (2, 24, 24), (2, 12, 12)), _rel(1, 1, (1, 23, 25), (1, 12, 13)), _rel(1, 1, (1, 64, 64), (1, 4, 4)),
          _rel(1, 2, (2, 6, 6), (2, 3, 3), misaligned=True), _rel(3, 1, (2, 4, 4), (2, 8, 8)), _rel(1, 2, (8, 14, 14), (8, 14, 14))]
    return c


CASES = _build_cases()


def case_id(c):
    k = "x".join(map(str, c.k_thw))
    if c.kind == "attn":
        return f"attn-B{c.B}xH{c.H}-Lq{c.Lq}-k{k}-ldo{c.H * D + c.ldo_extra}-{c.kernel}"
    return f"rel-B{c.B}xH{c.H}-q{'x'.join(map(str, c.q_thw))}-k{k}{'-misaligned' if c.misaligned else ''}-{c.kernel}"


def _build_tests():
    """every case runs `randn` and `peaked`; the first case to reach an instantiation not seen before also runs the other regimes"""
    tests, seen = [], set()
    for c in CASES:
        regs = ["randn", "peaked"]
        if any(k not in seen for k in c.kernel.split("+")):
            seen.update(c.kernel.split("+"))
            regs += ["hot", "offset", "equal", "bias_only"]
        tests += [(c, r) for r in regs]
    return tests


TESTS = _build_tests()


def n_draws(c):
    """attn_checks.n_draws: the smallest per-token tensor (q side: BH (Lq + 1) rows, key side: BH (Lk + 1)) reaches MIN_ROWS rows"""
    Lk = c.k_thw[0] * c.k_thw[1] * c.k_thw[2]
    rows = c.B * c.H * (min(c.Lq, Lk) + 1)
    return 1 if rows >= MIN_ROWS else min(256, -(-MIN_ROWS // rows))


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
key_map = mro.key_map          # E [Lk, J] (fp32 0/1): the columns mvit_checks._attn_ref indexes


def pack(x, dt):
    """fp32 -> the hi, lo pair of the operand type (as fp32 tensors)"""
    return mro.pack(x, lambda t: _rnd(t, dt))


def make_problem(c, regime, operand=None, draw=0):
    """-> dict of CPU fp32 tensors already rounded to the operand type where the kernels take 16 bits: q, do [BH, Lq + 1, 96], k, v
    [BH, Lk + 1, 96] (cls LAST); kind attn: hi, lo [BH, Lq, J] (the pair of rel / scale); kind rel: the tables Rh, Rw, Rt (fp32), the int
    index maps ih, iw, it, and for the rel kernels on their own drel_in [BH, Lq, J] (fp32), dq0 [BH, Lq + 1, 96] and the tables' start"""
    operand = BF if operand is None else operand
    g = torch.Generator().manual_seed(zlib.crc32(repr((tuple(c[:8]), regime)).encode()) % (1 << 31) + draw)
    BH, Lq1 = c.B * c.H, c.Lq + 1
    Lk1, J = c.k_thw[0] * c.k_thw[1] * c.k_thw[2] + 1, sum(c.k_thw)
    q, k, v = (torch.randn(BH, n, D, generator=g) for n in (Lq1, Lk1, Lk1))
    f = {"hot": 2.0, "peaked": 3.5}.get(regime, 1.0)
    q *= f
    k *= f
    if regime in ("offset", "equal", "bias_only"):
        vec = torch.randn(BH, 1, D, generator=g)
        k = torch.where(vec > 0, 8.0, -8.0) + k if regime == "offset" else vec.expand(BH, Lk1, D).clone()
    rel_gain = {"equal": 0.0, "bias_only": 6.0}.get(regime, 1.0)
    p = dict(q=_rnd(q, operand), k=_rnd(k, operand), v=_rnd(v, operand), do=_rnd(torch.randn(BH, Lq1, D, generator=g), operand))
    if c.kind == "attn":
        p["hi"], p["lo"] = pack(torch.randn(BH, c.Lq, J, generator=g) * (f * rel_gain / SCALE), operand)
        return p
    for name, n in zip(("Rh", "Rw", "Rt"), table_rows(c.q_thw, c.k_thw)):           # rel = Q . R ~ f * rel_gain * N(0, 1)
        p[name] = torch.randn(n, D, generator=g) * (0.1 * rel_gain)
        p["start_" + name] = torch.randn(n, D, generator=g)
    p["ih"], p["iw"], p["it"] = (mo.rel_index(c.q_thw[a], c.k_thw[a]) for a in (1, 2, 0))
    p["drel_in"] = torch.randn(BH, c.Lq, J, generator=g)
    p["dq0"] = _rnd(torch.randn(BH, Lq1, D, generator=g), operand)
    return p


def to_tok(x, B, H):
    """[BH, Lq + 1, 96] -> token-major [B Lq + B, H 96] (patch rows (b, query), then the B cls rows; column h 96 + d)"""
    Lq = x.shape[1] - 1
    t = x.reshape(B, H, Lq + 1, D).permute(0, 2, 1, 3)
    return torch.cat((t[:, :Lq].reshape(B * Lq, H * D), t[:, Lq].reshape(B, H * D)))


def from_tok(t, B, H):
    Lq = t.shape[0] // B - 1
    x = torch.cat((t[:B * Lq].reshape(B, Lq, H, D), t[B * Lq:].reshape(B, 1, H, D)), 1)
    return x.permute(0, 2, 1, 3).reshape(B * H, Lq + 1, D)


# ---------------------------------------------------------------------------------------------------------------------
# the rel terms (any dtype; autograd gives their gradients)
# ---------------------------------------------------------------------------------------------------------------------
def rel_terms(Qp, Rh, Rw, Rt, p, q_thw, flip=False):
    """Qp [n, Lq, 96] -> rel [n, Lq, J]; flip: the channels are summed in reverse order (a second implementation for the host test)"""
    return mro.rel_terms(Qp, Rh, Rw, Rt, (p["ih"], p["iw"], p["it"]), q_thw, flip)


def _paired(x, dt):
    hi, lo = pack(x, dt)
    return hi + lo


def rel_fwd_model(p, c, operand, out_scale, paired=True, flip=False):
    """-> (hi, lo) of out_scale * rel as the forward stores it; paired = False: plain fp32 einsum (the yardstick), no output pair"""
    Lq = c.Lq
    T = [(_paired(p[n], operand) if paired else p[n]) for n in ("Rh", "Rw", "Rt")]
    rel = rel_terms(p["q"][:, :Lq], *T, p, c.q_thw, flip)
    return pack(rel * out_scale, operand) if paired else (rel * out_scale, torch.zeros_like(rel))


def rel_bwd_model(p, c, operand, drel, dq_in, start, paired=True, flip=False):
    """dQ = R(dq_in + drel . R) on patch rows (fp32 tables and drel: the dQ kernel is plain fp32), dR = start + pair(drel)^T Q in fp32.
    paired = False: the yardstick (plain fp32, dQ still rounded once: that rounding is the contract's)"""
    Lq = c.Lq
    Qp = p["q"][:, :Lq].clone().requires_grad_(True)
    T = [p[n].clone().requires_grad_(True) for n in ("Rh", "Rw", "Rt")]
    rel = rel_terms(Qp, *T, p, c.q_thw, flip)
    dqr, = torch.autograd.grad(rel, Qp, drel, retain_graph=True)
    dT = torch.autograd.grad(rel, T, _paired(drel, operand) if paired else drel)
    dq = dq_in.clone()
    dq[:, :Lq] = _rnd(dq_in[:, :Lq] + dqr, operand)
    return dict(dQ=dq, dRh=start[0] + dT[0], dRw=start[1] + dT[1], dRt=start[2] + dT[2])


def rel_reference(p, c, out_scale, drel, dq_in, start):
    """fp64: rel * out_scale, dq_in + drel . R, start + drel^T Q"""
    Lq = c.Lq
    Qp = p["q"][:, :Lq].double().requires_grad_(True)
    T = [p[n].double().requires_grad_(True) for n in ("Rh", "Rw", "Rt")]
    rel = rel_terms(Qp, *T, p, c.q_thw)
    g = torch.autograd.grad(rel, [Qp] + T, drel.double())
    dq = dq_in.double().clone()
    dq[:, :Lq] += g[0]
    return dict(rel=rel.detach() * out_scale, dQ=dq, dRh=start[0].double() + g[1], dRw=start[1].double() + g[2], dRt=start[2].double() + g[3])


# ---------------------------------------------------------------------------------------------------------------------
# reference and rounding models of the attention
# ---------------------------------------------------------------------------------------------------------------------
def _slices(n, Lq1, Lk1, budget=4e6):
    step = max(1, int(budget // (Lq1 * Lk1)))
    return [slice(i, min(n, i + step)) for i in range(0, n, step)]


def _cat(parts):
    return {k: torch.cat([p[k] for p in parts]) for k in parts[0]}


def reference(p, c, chain=False):
    """fp64 autograd -> o, lse (natural logarithm), dq, dk, dv, drel, lse32 (the fp32 yardstick's logsumexp); chain: rel comes from the
    tables, dq is the TOTAL gradient of q and dRh, dRw, dRt are returned too (without a start value)"""
    Lq, Lk1 = c.Lq, p["k"].shape[1]
    E = key_map(c.k_thw)
    E64 = E.double()
    T = [p[n].double().requires_grad_(True) for n in ("Rh", "Rw", "Rt")] if chain else None
    out = []
    for sl in _slices(p["q"].shape[0], Lq + 1, Lk1):
        qd, kd, vd = (p[n][sl].double().requires_grad_(True) for n in ("q", "k", "v"))
        if chain:
            rd = rel_terms(qd[:, :Lq], *T, p, c.q_thw)
            rd.retain_grad()
        else:
            rd = ((p["hi"][sl].double() + p["lo"][sl].double()) * SCALE).requires_grad_(True)
        s = (qd @ kd.transpose(1, 2)) * SCALE + F.pad(rd @ E64.t(), (0, 1, 0, 1))
        o = torch.softmax(s, -1) @ vd + F.pad(qd[:, :Lq], (0, 0, 0, 1))
        o.backward(p["do"][sl].double())
        s32 = (p["q"][sl] @ p["k"][sl].transpose(1, 2)) * SCALE + F.pad(rd.detach().float() @ E.t(), (0, 1, 0, 1))
        out.append(dict(o=o.detach(), lse=torch.logsumexp(s.detach(), -1), dq=qd.grad, dk=kd.grad, dv=vd.grad, drel=rd.grad,
                        lse32=torch.logsumexp(s32, -1)))
    out = _cat(out)
    if chain:
        out.update(dRh=T[0].grad, dRw=T[1].grad, dRt=T[2].grad)
    return out


def pool_model(p, c, operand, hi=None, lo=None, variant=False, E_kernel=None, cls_bias=False, cls_resid=False, keep_ds=False):
    """the kernels' rounding model (module docstring) -> o, lse (natural), delta, dq, dk, dv (rounded to the operand type), drel (fp32).
    variant: `model_variant`.  E_kernel / cls_bias / cls_resid: defects the host test plants (a wrong key map; the cls query takes the
    bias row of the last patch query; the residual q is added to the cls row too).  keep_ds: also return the rounded dS."""
    Lq, Lk = c.Lq, p["k"].shape[1] - 1
    E = key_map(c.k_thw) if E_kernel is None else E_kernel
    hi = p["hi"] if hi is None else hi
    lo = p["lo"] if lo is None else lo
    out = []
    rnd = lambda t: _rnd(t, operand)
    for sl in _slices(p["q"].shape[0], Lq + 1, Lk + 1):
        ql, kl, vl, dl = (p[n][sl] for n in ("q", "k", "v", "do"))
        # the arithmetic itself: oracle/mvit_rounded_oracle.py (one restatement of the kernel for the per-row and the end-to-end rule)
        f = mro.pattn_fwd(ql, kl, vl, hi[sl], lo[sl], E, SCALE, rnd, variant, cls_bias, cls_resid)
        b = mro.pattn_bwd(ql, kl, vl, dl, f, E, SCALE, rnd, variant, cls_resid)
        r = dict(o=f["o"], lse=f["lse"][..., 0], delta=b["delta"], dq=b["dq"], dk=b["dk"], dv=b["dv"], drel=b["drel"])
        if keep_ds:
            r["ds"] = b["ds"]
        out.append(r)
    return _cat(out)


def model_variant(p, c, operand):
    return pool_model(p, c, operand, variant=True)


def chain_model(p, c, operand, variant=False):
    """rel_fwd_model(out_scale = 1 / scale) -> pool_model -> rel_bwd_model adding into the rounded dq; tables without a start value"""
    hi, lo = rel_fwd_model(p, c, operand, 1.0 / SCALE)
    m = pool_model(p, c, operand, hi, lo, variant=variant)
    zero = [torch.zeros_like(p[n]) for n in ("Rh", "Rw", "Rt")]
    m.update(rel_bwd_model(p, c, operand, m["drel"], m["dq"], zero))
    return m


# ---------------------------------------------------------------------------------------------------------------------
# verdicts
# ---------------------------------------------------------------------------------------------------------------------
def _loc(c, unit="token"):
    BH = c.B * c.H

    def where(flat, S):
        draw, item = divmod(flat // S, BH)
        return f"(clip {item // c.H}, head {item % c.H}, {unit} {flat % S}" + (f"; draw {draw})" if draw else ")")
    return where


def zero_floors(p):
    """attn_checks.fp32_zero_floor for dq and dk; drel = sum over keys of dS: the dk floor without the q factor, times Lk"""
    a = (p["do"].abs() @ p["v"].abs().transpose(1, 2)).max().item() * 2.0 ** -18
    return {"dq": SCALE * a * p["k"].abs().max().item(), "dk": SCALE * a * p["q"].abs().max().item() * p["q"].shape[1],
            "drel": a * p["k"].shape[1]}


def judge_attention(c, regime, got, ref, mod, p, names=("o", "dq", "dk", "dv", "drel", "delta"), lse=True):
    """got / mod: o, dq [n, Lq + 1, 96], dk, dv [n, Lk + 1, 96], drel [n, Lq, J], delta [n, Lq + 1, 1], lse [n, Lq + 1] (natural)"""
    fwd_b, bwd_b = (AGG_FWD, AGG_BWD) if regime == "randn" else (None, None)
    floor = zero_floors(p)
    out = []
    for name in names:
        r = ref[name] if name != "delta" else (p["do"].double() * (ref["o"] - F.pad(p["q"][:, :c.Lq], (0, 0, 0, 1)).double())).sum(-1, keepdim=True)
        # delta is no tensor of check_mvit_attention: no flat bound is "today's" for it (rowsum(dO (o - q)) cancels; the bf16 MODEL's aggregate
        # error is 1.5e-2 to 1.6e-2 in `randn` at 1,569 keys), so its aggregate follows the model in every regime
        flat = None if name == "delta" else (fwd_b if name == "o" else bwd_b)
        out += ac.judge_tensor(None, name, got[name], r, mod[name], None, flat, floor.get(name, 0.0),
                               where=_loc(c, "query" if name in ("drel", "delta") else "token"))
    if lse:
        out += ac.judge_lse(None, got["lse"], ref, None, where=_loc(c, "query"))
    return out


def judge_rel_tensor(c, name, x, ref, mod, yard, per_item=True):
    """the rel rule: rowerr <= max(ROW_FACTOR * model, REL_Y_FACTOR * fp32 yardstick); x [.., rows, W]"""
    rk, i = rowerr(x, ref)
    rm, ry = rowerr(mod, ref)[0], rowerr(yard, ref)[0]
    bound = max(ROW_FACTOR * rm, REL_Y_FACTOR * ry)
    S = x.shape[-2]
    where = _loc(c, "query")(i, S) if per_item else f"(row {i})"
    return [Finding(name + " rowerr", rk <= bound, rk, bound, f"model rowerr {rm:.3e}, fp32 yardstick {ry:.3e}, ratio to the bound's "
                    f"larger term {rk / max(bound / (ROW_FACTOR if ROW_FACTOR * rm >= REL_Y_FACTOR * ry else REL_Y_FACTOR), 1e-300):.2f}, "
                    f"worst row {where}")]


def rel_unpack(hi, lo, J, out_scale):
    return (hi + lo)[..., :J] / out_scale


def judge_rel(c, p, operand, got, start):
    """the rel kernels on their own.  got: hi, lo [BH, Lq, JP] (fp32 values of the stored pair), dQ [BH, Lq + 1, 96], dRh, dRw, dRt"""
    J, osc = sum(c.k_thw), 1.0 / SCALE
    ref = rel_reference(p, c, 1.0, p["drel_in"], p["dq0"], start)
    mh, ml = rel_fwd_model(p, c, operand, osc)
    yh, _ = rel_fwd_model(p, c, operand, osc, paired=False)
    out = judge_rel_tensor(c, "rel (decoded relp)", rel_unpack(got["hi"], got["lo"], J, osc), ref["rel"], (mh + ml) / osc, yh / osc)
    padz = torch.cat((got["hi"][..., J:], got["lo"][..., J:]), -1).abs().max().item() if got["hi"].shape[-1] > J else 0.0
    out.append(Finding("relp: padding columns J .. JP of hi and lo are zero", padz == 0.0, padz, 0.0, ""))
    mod = rel_bwd_model(p, c, operand, p["drel_in"], p["dq0"], start)
    yard = rel_bwd_model(p, c, operand, p["drel_in"], p["dq0"], start, paired=False)
    out += judge_rel_tensor(c, "rel_bwd dQ", got["dQ"], ref["dQ"], mod["dQ"], yard["dQ"])
    same = torch.equal(got["dQ"][:, c.Lq], p["dq0"][:, c.Lq])
    out.append(Finding("rel_bwd dQ: cls rows unchanged", same, 0.0 if same else 1.0, 0.0, ""))
    for n in ("dRh", "dRw", "dRt"):
        out += judge_rel_tensor(c, "rel_bwd " + n + " (start + gradient)", got[n], ref[n], mod[n], yard[n], per_item=False)
    return out


def judge_chain_tables(c, p, operand, got, ref, mod, start):
    """the chain's tables by the rel rule (yardstick: the plain fp32 table gradient of the fp64 drel); o, the total dQ, dk and dv take
    the attention rule in `check_case`"""
    yard = rel_bwd_model(p, c, operand, ref["drel"].float(), torch.zeros_like(p["q"]), start, paired=False)
    out = []
    for i, n in enumerate(("dRh", "dRw", "dRt")):
        out += judge_rel_tensor(c, "chain " + n + " (start + gradient)", got[n], start[i].double() + ref[n], start[i] + mod[n], yard[n],
                                per_item=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the kernels (GPU), through the C ABI: every output inside a guard band
# ---------------------------------------------------------------------------------------------------------------------
def _abi():
    from procedurevrl_amd._lib import lib
    from procedurevrl_amd.ops import _ptr, _stream
    return lib(), _ptr, _stream


def _workspace(nbytes, dev):
    return torch.full((int(nbytes) + WS_TAIL,), WS_FILL, dtype=torch.uint8, device=dev)


def _ws_check(name, ws, nbytes):
    n = int((ws[int(nbytes):] != WS_FILL).sum())
    return [Finding(f"{name}: bytes behind the advertised workspace size that changed", n == 0, float(n), 0.0, "")]


def gpu_attention(c, p, relp, dev):
    """pvrl_mvit_attn_fwd + _bwd.  relp: device [BH Lq, 2 JP] (operand type).  -> (Guarded buffers by name, guard findings)"""
    from procedurevrl_amd import ops_mvit as om
    L, ptr, stream = _abi()
    B, H, Lq, BH = c.B, c.H, c.Lq, c.B * c.H
    Lq1, Lk1, J, HD = Lq + 1, p["k"].shape[1], sum(c.k_thw), c.H * D
    ldo = HD + c.ldo_extra
    f32 = torch.float32
    qd, kd, vd = (guarded_input(p[n].reshape(-1, D), BF, dev, 0) for n in ("q", "k", "v"))
    dod = guarded_input(to_tok(p["do"], B, H), BF, dev, c.ldo_extra)
    km = om.keymap(c.k_thw, dev)
    b = dict(o=Guarded("o", [B * Lq + B], HD, BF, c.ldo_extra, device=dev), lse=Guarded("lse", [BH], Lq1, f32, device=dev),
             delta=Guarded("delta", [BH], Lq1, f32, device=dev), dq=Guarded("dq", [BH * Lq1], D, BF, device=dev),
             dk=Guarded("dk", [BH * Lk1], D, BF, device=dev), dv=Guarded("dv", [BH * Lk1], D, BF, device=dev),
             drel=Guarded("drel", [BH * Lq], J, f32, device=dev))
    L.call("pvrl_mvit_attn_fwd", ptr(qd), ptr(kd), ptr(vd), ptr(relp), ptr(km), B, H, Lq, *c.k_thw, float(SCALE), ptr(b["o"].seg(0)), ldo,
           ptr(b["lse"].seg(0)), stream())
    nbytes = L.call("pvrl_mvit_attn_bwd_workspace_bytes", B, H, Lq, *c.k_thw)
    ws = _workspace(nbytes, dev)
    L.call("pvrl_mvit_attn_bwd", ptr(qd), ptr(kd), ptr(vd), ptr(relp), ptr(km), B, H, Lq, *c.k_thw, float(SCALE), ptr(b["o"].seg(0)),
           ptr(dod), ldo, ptr(b["lse"].seg(0)), ptr(b["delta"].seg(0)), ptr(b["dq"].seg(0)), ptr(b["dk"].seg(0)), ptr(b["dv"].seg(0)),
           ptr(b["drel"].seg(0)), ptr(ws), int(nbytes), stream())
    torch.cuda.synchronize()
    f = _ws_check("attn_bwd", ws, nbytes)
    for g in b.values():
        f += g.check()
    b["q_dev"] = qd
    return b, f


def attention_outputs(c, b, Lk1, dq=None):
    cpu = lambda t: t.float().cpu()
    BH, Lq1 = c.B * c.H, c.Lq + 1
    return dict(o=from_tok(cpu(b["o"].seg(0)), c.B, c.H), lse=cpu(b["lse"].seg(0)) * LN2, delta=cpu(b["delta"].seg(0)).reshape(BH, Lq1, 1),
                dq=cpu(b["dq"].seg(0)).reshape(BH, Lq1, D), dk=cpu(b["dk"].seg(0)).reshape(BH, Lk1, D),
                dv=cpu(b["dv"].seg(0)).reshape(BH, Lk1, D), drel=cpu(b["drel"].seg(0)).reshape(BH, c.Lq, -1))


def _misaligned(x, dev):
    """x [n, 96] fp32 as a device view whose first byte sits 4 bytes behind a 16-byte boundary (input guard values around it)"""
    buf = torch.full((x.numel() + 8,), ac.INPUT_GUARD, device=dev)
    v = buf[1:1 + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4
    return v


class RelDevice:
    """the tables, index maps and q of a rel case on the device, and the two entry points"""

    def __init__(self, c, p, dev, q_dev=None):
        self.c, self.dev = c, dev
        up = (lambda x: _misaligned(x, dev)) if c.misaligned else (lambda x: guarded_input(x, torch.float32, dev, 0))
        self.R = [up(p[n]) for n in ("Rh", "Rw", "Rt")]
        self.idx = [p[n].to(dev, torch.int32).contiguous() for n in ("ih", "iw", "it")]
        self.q = guarded_input(p["q"].reshape(-1, D), BF, dev, 0) if q_dev is None else q_dev
        self.JP = 32 if sum(c.k_thw) <= 32 else 64

    def fwd(self, out_scale):
        L, ptr, stream = _abi()
        c = self.c
        rb = Guarded("relp", [c.B * c.H * c.Lq], 2 * self.JP, BF, device=self.dev)
        L.call("pvrl_mvit_rel_fwd", ptr(self.q), c.B * c.H, *c.q_thw, *c.k_thw, *(ptr(t) for t in self.R), *(ptr(t) for t in self.idx),
               float(out_scale), ptr(rb.seg(0)), stream())
        return rb

    def bwd(self, drel, dQ, start):
        """drel fp32 [BH Lq, J], dQ [BH (Lq + 1), 96] in place -> (the three Guarded tables, findings)"""
        L, ptr, stream = _abi()
        c = self.c
        tabs = []
        for s, n in zip(start, ("dRh", "dRw", "dRt")):
            g = Guarded(n, [s.shape[0]], D, torch.float32, device=self.dev)
            g.seg(0).copy_(s)
            tabs.append(g)
        nbytes = L.call("pvrl_mvit_rel_bwd_workspace_bytes", c.B * c.H, *c.q_thw, *c.k_thw)
        ws = _workspace(nbytes, self.dev)
        L.call("pvrl_mvit_rel_bwd", ptr(drel), ptr(self.q), ptr(dQ), c.B * c.H, *c.q_thw, *c.k_thw, *(ptr(t) for t in self.R),
               *(ptr(t) for t in self.idx), *(int(s.shape[0]) for s in start), *(ptr(g.seg(0)) for g in tabs), ptr(ws), int(nbytes), stream())
        torch.cuda.synchronize()
        f = _ws_check("rel_bwd", ws, nbytes)
        for g in tabs:
            f += g.check()
        return tabs, f


def _run_attn_case(c, p, dev):
    JP = 32 if sum(c.k_thw) <= 32 else 64
    relp = torch.zeros(c.B * c.H * c.Lq, 2 * JP)
    J = sum(c.k_thw)
    relp[:, :J] = p["hi"].reshape(-1, J)
    relp[:, JP:JP + J] = p["lo"].reshape(-1, J)
    b, f = gpu_attention(c, p, guarded_input(relp, BF, dev, 0), dev)
    return attention_outputs(c, b, p["k"].shape[1]), f


def _run_rel_case(c, p, dev):
    """-> (outputs of the rel kernels on their own, outputs of the chain, guard findings)"""
    cpu = lambda t: t.float().cpu()
    BH, Lq, Lq1, JP = c.B * c.H, c.Lq, c.Lq + 1, 32 if sum(c.k_thw) <= 32 else 64
    start = [p["start_" + n] for n in ("Rh", "Rw", "Rt")]
    rd = RelDevice(c, p, dev)
    rb = rd.fwd(1.0 / SCALE)
    torch.cuda.synchronize()
    f = rb.check()
    relp = cpu(rb.seg(0)).reshape(BH, Lq, 2 * JP)
    dqb = Guarded("rel_bwd dQ", [BH * Lq1], D, BF, device=dev)
    dqb.seg(0).copy_(p["dq0"].reshape(-1, D))
    tabs, f2 = rd.bwd(guarded_input(p["drel_in"].reshape(BH * Lq, -1), torch.float32, dev, 0), dqb.seg(0), start)
    f += f2 + dqb.check()
    alone = dict(hi=relp[..., :JP], lo=relp[..., JP:], dQ=cpu(dqb.seg(0)).reshape(BH, Lq1, D),
                 **{n: cpu(g.seg(0)) for n, g in zip(("dRh", "dRw", "dRt"), tabs)})
    b, f3 = gpu_attention(c, p, rb.seg(0), dev)
    tabs, f4 = RelDevice(c, p, dev, b["q_dev"]).bwd(b["drel"].seg(0), b["dq"].seg(0), start)
    f += f3 + f4 + b["dq"].check()
    chain = attention_outputs(c, b, p["k"].shape[1])
    chain["dQ"] = chain.pop("dq")
    chain.update({n: cpu(g.seg(0)) for n, g in zip(("dRh", "dRw", "dRt"), tabs)})
    return alone, chain, f


def _stack(parts):
    return {k: torch.cat([p[k] for p in parts]) for k in parts[0] if torch.is_tensor(parts[0][k]) and parts[0][k].is_floating_point()}


def check_case(c, regime, run=None, operand=None):
    """one case x regime -> list of Finding (guard bands, then the rules per tensor); small cases: `n_draws` draws, all statistics over all
    of them.  run(c, p) -> what _run_attn_case / _run_rel_case return: the host test passes a stand-in for the GPU."""
    operand = BF if operand is None else operand
    if run is None:
        dev = torch.device("cuda:0")
        run = (lambda c, p: _run_attn_case(c, p, dev)) if c.kind == "attn" else (lambda c, p: _run_rel_case(c, p, dev))
    findings, P, G, R, M, A, C2, R2, M2 = [], [], [], [], [], [], [], [], []
    for d in range(n_draws(c)):
        p = make_problem(c, regime, operand, d)
        res = run(c, p)
        findings += [f for f in res[-1] if d == 0 or not f.ok]
        P.append(p)
        if c.kind == "attn":
            G.append(res[0])
            R.append(reference(p, c))
            M.append(pool_model(p, c, operand))
        else:
            A.append(res[0])
            C2.append(res[1])
            R2.append(reference(p, c, chain=True))
            M2.append(chain_model(p, c, operand))
    p = _stack(P)
    for n in ("ih", "iw", "it"):
        if n in P[0]:
            p[n] = P[0][n]
    if c.kind == "attn":
        return findings + judge_attention(c, regime, _stack(G), _stack(R), _stack(M), p)
    # the rel kernels on their own and the chain's tables (one set of tables per draw) are judged draw by draw; the chain's per-token
    # tensors over all draws together
    out = findings
    for d, q in enumerate(P):
        st = [q["start_" + n] for n in ("Rh", "Rw", "Rt")]
        fs = judge_rel(c, q, operand, A[d], st) + judge_chain_tables(c, q, operand, C2[d], R2[d], M2[d], st)
        out += [f for f in fs if d == 0 or not f.ok]
    g, m = _stack(C2), _stack(M2)
    fs = judge_attention(c, regime, dict(g, dq=g["dQ"]), _stack(R2), dict(m, dq=m["dQ"]), p, names=("o", "dq", "dk", "dv"), lse=False)
    return out + [f._replace(tensor="chain " + f.tensor) for f in fs]


# ---------------------------------------------------------------------------------------------------------------------
# refusals: PVRL_EINVAL and nothing launched
# ---------------------------------------------------------------------------------------------------------------------
def check_refusals():
    from procedurevrl_amd._lib import PvrlError
    L, ptr, stream = _abi()
    dev = torch.device("cuda:0")
    out = []

    def attempt(what, fn, outputs):
        for t in outputs:
            t.fill_(7.0)
        try:
            fn()
            msg = "returned 0"
        except PvrlError as e:
            msg = str(e)
        torch.cuda.synchronize()
        clean = all(bool((t == 7.0).all()) for t in outputs)
        out.append(Finding(f"{what}: status", msg.endswith("status -1"), 0.0, 0.0, msg))
        out.append(Finding(f"{what}: outputs untouched", clean, 0.0 if clean else 1.0, 0.0, ""))

    def attn(what, B, H, Lq, k_thw, ldo, short=0, fwd=True, keymap_of=None):
        BH, Lk1, J = B * H, k_thw[0] * k_thw[1] * k_thw[2] + 1, sum(k_thw)
        JP = 32 if J <= 32 else 64
        z = lambda *s, dt=BF: torch.zeros(*s, device=dev, dtype=dt)
        q, k, v, relp = z(BH * (Lq + 1), D), z(BH * Lk1, D), z(BH * Lk1, D), z(BH * Lq, 2 * JP)
        km = torch.zeros(((Lk1 + 31) // 32) * 4096, device=dev, dtype=torch.uint8)
        if keymap_of is not None:
            L.call("pvrl_mvit_attn_keymap", *keymap_of, ptr(km), stream())
        o, do = z(B * Lq + B, ldo + 8), z(B * Lq + B, ldo + 8)
        f32 = torch.float32
        lse, delta, drel = z(BH, Lq + 1, dt=f32), z(BH, Lq + 1, dt=f32), z(BH * Lq, J, dt=f32)
        dq, dk, dv = z(BH * (Lq + 1), D), z(BH * Lk1, D), z(BH * Lk1, D)
        nbytes = max(int(L.call("pvrl_mvit_attn_bwd_workspace_bytes", B, H, Lq, *k_thw)), 16)
        ws = torch.zeros(nbytes, device=dev, dtype=torch.uint8)
        if fwd:
            attempt(f"pvrl_mvit_attn_fwd {what}", lambda: L.call("pvrl_mvit_attn_fwd", ptr(q), ptr(k), ptr(v), ptr(relp), ptr(km), B, H, Lq,
                                                                 *k_thw, float(SCALE), ptr(o), ldo, ptr(lse), stream()), [o, lse])
        attempt(f"pvrl_mvit_attn_bwd {what}", lambda: L.call(
            "pvrl_mvit_attn_bwd", ptr(q), ptr(k), ptr(v), ptr(relp), ptr(km), B, H, Lq, *k_thw, float(SCALE), ptr(o), ptr(do), ldo, ptr(lse),
            ptr(delta), ptr(dq), ptr(dk), ptr(dv), ptr(drel), ptr(ws), nbytes - short, stream()), [delta, dq, dk, dv, drel])

    def rel(what, BH, q_thw, k_thw, short=0, fwd=True):
        Lq, J = q_thw[0] * q_thw[1] * q_thw[2], sum(k_thw)
        JP = 32 if J <= 32 else 64
        f32 = torch.float32
        z = lambda *s, dt=f32: torch.zeros(*s, device=dev, dtype=dt)
        Q, dQ, relp = z(BH * (Lq + 1), D, dt=BF), z(BH * (Lq + 1), D, dt=BF), z(BH * Lq, 2 * JP, dt=BF)
        nr = table_rows(q_thw, k_thw)
        R, dR = [z(n, D) for n in nr], [z(n, D) for n in nr]
        idx = [mo.rel_index(q_thw[a], k_thw[a]).to(dev, torch.int32).contiguous() for a in (1, 2, 0)]
        drel = z(BH * Lq, J)
        nbytes = int(L.call("pvrl_mvit_rel_bwd_workspace_bytes", BH, *q_thw, *k_thw))
        ws = torch.zeros(max(nbytes, 16), device=dev, dtype=torch.uint8)
        if fwd:
            attempt(f"pvrl_mvit_rel_fwd {what}", lambda: L.call("pvrl_mvit_rel_fwd", ptr(Q), BH, *q_thw, *k_thw, *(ptr(t) for t in R),
                                                                *(ptr(t) for t in idx), 1.0, ptr(relp), stream()), [relp])
        attempt(f"pvrl_mvit_rel_bwd {what}", lambda: L.call(
            "pvrl_mvit_rel_bwd", ptr(drel), ptr(Q), ptr(dQ), BH, *q_thw, *k_thw, *(ptr(t) for t in R), *(ptr(t) for t in idx), *nr,
            *(ptr(t) for t in dR), ptr(ws), max(nbytes, 16) - short if nbytes > 0 else 16, stream()), [dQ] + dR)

    attn("Lk + 1 = 1665", 1, 1, 8, (8, 16, 13), 128)
    attn("ldo = H 96 + 4", 1, 2, 8, (1, 3, 5), 2 * D + 4, keymap_of=(1, 3, 5))
    attn("workspace one byte short", 1, 2, 8, (1, 3, 5), 2 * D + 8, short=1, fwd=False, keymap_of=(1, 3, 5))
    rel("kh = 17", 2, (1, 2, 2), (1, 17, 2))
    rel("workspace one byte short", 2, (1, 4, 4), (1, 2, 2), short=1, fwd=False)
    return out
