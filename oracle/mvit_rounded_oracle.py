"""CPU ORACLE OF THE MViTv2 ENCODER WITH THE HIP DATAPATH'S ROUNDING POINTS -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

`oracle/mvit_oracle.py` restates the reference's MViT_encoder in fp32 and is pinned to it by tests/golden/mvit_small.pt.  This module is the
same restatement with a rounding to the operand type at every point where `procedurevrl_amd/mvit.py: MViTEngine` and its kernels round, and
nowhere else -- what `oracle/rounded_oracle.py` is to the TimeSformer path (read its docstring first; `OPERAND`, `operand(dtype)`, `R`, `RW`,
`RB` and `GeluStore` are ITS objects, imported, so one switch serves both).  With `OPERAND is None` it is the fp32 oracle bit for bit
(tests/test_mvit_rounding_host.py), which pins it to the reference; tests/mvit_rounding_checks.py then holds the HIP path's distance from the
fp32 oracle to this model's, per block and per parameter.

Rounding points (kernel that rounds -> where it appears below):
  forward   im2col3d (pixels -> operand)                                     `R(x)` in front of the stem convolution
            weight operand copies (WeightCache.padded)                       `RW(w)` on every GEMM weight; biases, LN parameters, pool weights fp32
            stem, residual stream x / xs / xres / x1 / x2 (PVRL_EPI_F32, PVRL_EPI_RESID_F32, max-pool in fp32)      no rounding
            ln_fwd outputs xn, xn2 (16-bit)                                  `R(ln(..))` (`RW` for xn where dim != dim_out, see backward)
            qkv (gemm_nt PVRL_EPI_BF16)                                      `R(linear(xn))`
            pool_fwd: conv output c = R(conv), q / k / v = R(LN(unrounded conv))          `PoolLN` (core: `pool_ln_fwd`)
            rel_fwd: tables read as their hi + lo pair, rel / scale stored as a hi + lo pair   `RelPair` (core: `rel_terms`, `pack`)
            attn_fwd: logits = scale (q.k + (hi + lo).E) in fp32, the UNNORMALISED exp rounded for the second MFMA, o = R(acc / l + q),
            lse fp32                                                         `PoolAttn` (core: `pattn_fwd`)
            skip projection: from the 16-bit xn, fp32 result                 `RB(linear(xn, RW(w)))`
            fc1: u and g 16-bit (PVRL_EPI_GELU)                              `RB(..)`, `GeluStore`, `RW(g)`
            final norm: fp32 on the cls rows                                 no rounding
            prune_last: the last block's projection and MLP on the cls rows only, through the same 16-bit GEMMs.  Only those rows reach
            the features, so the all-row model below computes the same values and, in the backward, exact zeros where the engine skips.
  backward  cast_scale(dx2, rowscale = rs_m): R(DropPath factor x fp32 gradient)        `RB(linear(g, ..)) * dp`: the factor multiplies first
            du (PVRL_EPI_DGELU, from the stored 16-bit u), dxn2 16-bit       `GeluStore`, backward half of `R`
            ln_bwd: fp32 dx1, and its 16-bit copy R(rs_a dx1) for the projection's backward    `RB(linear(o, ..)) * dp`
            d_o 16-bit                                                       backward half of `R(o)`
            attn_bwd: dS = R(P (dP - D)), D from the stored o minus q, dq = R(scale dS K + dO), dk = R(scale dS^T Q),
            dv = R(R(P)^T dO), drel = dS E fp32                              `PoolAttn` (core: `pattn_bwd`)
            rel_bwd: dQ = R(dq + drel . R) -- a second rounding, tables and drel in fp32 there; table gradients = pair(drel)^T Q in fp32
                                                                             `DQAdd`, `RelPair`
            pool_bwd: LN statistics from the ROUNDED c, dc = R(dLN), dqkv = R(transposed conv of dc) (cls: dc itself); dw, dgamma,
            dbeta fp32 sums over the 16-bit dc / dy / x                      `PoolLN` (core: `pool_ln_bwd`)
            dxn = dqkv W_qkv: 16-bit where dim == dim_out, fp32 where the skip projection's dxs W_skip is added to it    `R` / `RW` on xn
            cast_scale(dxs) in front of the skip projection's backward       `RB`
            block 0's ln_bwd writes R(dx): the stem's gradient operand       `RB` behind the stem convolution
            every weight, bias, LN, pool-weight and rel-table gradient: fp32 sums of products of those 16-bit operands
            fp16 flavour (grads.SCALED_GRADS): the whole backward runs in S-scaled units, S a power of two (GradStore.begin_scaled).  The
            caller feeds this model S * g and divides the gradients by S (tests/mvit_rounding_checks.py: `scale_of`).

`VARIANT = True`: another legitimate implementation of the same datapath -- the NORMALISED P rounded for the second product, as in
tests/pool_attn_checks.model_variant; dq_attn + drel . R rounded ONCE; the table gradients in one torch sum instead of item by item.  The rule
of tests/mvit_rounding_checks.py must let it pass: it shows the rule does not hang on one choice of order.  (D stays the kernel's, from the
stored o minus q, unlike model_variant's: the gradient of norm_k.bias, zero in exact arithmetic, is NOTHING BUT the rounding error of D
summed over keys, so a D from the unrounded o is not the same datapath in another order but a 2 to 3.4 times more exact one for that tensor.)
`DEFECT`: one of `DEFECTS`, planted by tests/test_mvit_rounding_host.py to show that the rule bites.  Switch -> site:
  x2_16bit             `block`: its return value rounded (forward only)
  resid_16bit          `block`: x1 and x2 rounded, `forward_features`: the stem output rounded (the whole residual stream, forward only)
  rel_single           `RelPair.forward`: the lo half dropped
  table_grad_16bit     `RelPair.backward`: the table gradients accumulated in the operand type, one add per (item, t, h) line of queries
  dxn_16bit            `block`, dim != dim_out: the attention branch's input gradient dqkv W_qkv rounded before dxs W_skip is added
  droppath_after_cast  `_dp`: the DropPath factor multiplies behind the backward's cast
  stem_partial_16bit   `forward_features`: one rounded partial weight gradient per clip
  (no_grad_scale lives in tests/mvit_rounding_checks.oracle_step: S = 1 in the fp16 flavour)
`TAPS`: a dict that collects the per-site facts tests/mvit_rounding_checks.py also reads off the engine (`rel_lo`: share of rel entries with a
live lo half, per block; `dxn`: 16-bit-valued share of dqkv W_qkv where dim != dim_out, per block; `dxn_sum`: ... of norm1's incoming
gradient, per block; `dp_cast`: per DropPath factor, the share of the 16-bit gradient operand's entries that are not R(factor x fp32 gradient)).
`SITES`: with `OPERAND is None` the custom sites are by-passed (`mvit_oracle.msa` runs, so the result is the fp32 oracle bit for bit);
`SITES = True` forces them on without rounding, which shows that they compute the same function (sums in another order).

The cores (`pattn_fwd` / `pattn_bwd`, `pool_ln_fwd` / `pool_ln_bwd`, `rel_terms`, `pack`, `key_map`) are what tests/pool_attn_checks.py and
tests/mvit_pool_checks.py build their per-row models from: one restatement of each kernel.
"""
import torch
import torch.nn.functional as F

from . import mvit_oracle as mo
from . import rounded_oracle as ro
from .rounded_oracle import R, RW, RB, GeluStore, operand  # noqa: F401 (`operand` re-exported: the same switch)

VARIANT = False
DEFECT = None
DEFECTS = ("x2_16bit", "rel_single", "table_grad_16bit", "dxn_16bit", "droppath_after_cast", "stem_partial_16bit", "resid_16bit")
SITES = False
TAPS = None             # a dict: the per-site facts tests/mvit_rounding_checks.py also reads off the engine (keys `rel_lo`, `dxn`, `dxn_sum`, `dp_cast`)
EPS = 1e-6


def _rnd(t):
    return ro._rnd(t)


def _on():
    return ro.OPERAND is not None or SITES


def valued16(t, dtype):
    """share of the non-zero entries of t that are exact values of the 16-bit type: ~1 for a tensor stored in it, 2^-13 / 2^-16 for fp32 data"""
    t = t.detach().float()
    nz = t != 0
    return float((t.to(dtype).float() == t)[nz].float().mean()) if bool(nz.any()) else 0.0


# ------------------------------------------------------------------------------------------------ cores, shared with the per-row harnesses
def key_map(k_thw):
    """E [Lk, J] (fp32 0/1): key -> its three rel columns j = h(key), kh + w(key), kh + kw + t(key)"""
    kt, kh, kw = k_thw
    Lk = kt * kh * kw
    j = torch.arange(Lk)
    E = torch.zeros(Lk, kt + kh + kw)
    E[j, (j // kw) % kh] = 1
    E[j, kh + j % kw] = 1
    E[j, kh + kw + j // (kw * kh)] = 1
    return E


def pack(x, rnd):
    """fp32 -> the hi, lo pair of the operand type (as fp32 tensors)"""
    hi = rnd(x)
    return hi, rnd(x - hi)


def paired(x, rnd):
    hi, lo = pack(x, rnd)
    return hi + lo


def rel_terms(Qp, Rh, Rw, Rt, idx, q_thw, flip=False):
    """Qp [n, Lq, d] -> rel [n, Lq, J], idx = (ih, iw, it) of mvit_oracle.rel_index; flip: the channels are summed in reverse order"""
    if flip:
        Qp, Rh, Rw, Rt = (t.flip(-1) for t in (Qp, Rh, Rw, Rt))
    rq = Qp.reshape(Qp.shape[0], *q_thw, Qp.shape[-1])
    return torch.cat((torch.einsum("bthwc,hkc->bthwk", rq, Rh[idx[0]]), torch.einsum("bthwc,wkc->bthwk", rq, Rw[idx[1]]),
                      torch.einsum("bthwc,tkc->bthwk", rq, Rt[idx[2]])), -1).reshape(Qp.shape[0], Qp.shape[1], -1)


def pattn_fwd(q, k, v, hi, lo, E, scale, rnd, variant=False, cls_bias=False, cls_resid=False):
    """csrc/attn_pool.hip forward on 16-bit-valued q [n, Lq + 1, d], k, v [n, Lk + 1, d] (cls LAST) and the pair hi, lo [n, Lq, J] of
    rel / scale -> dict(o, lse, oa, res, s).  cls_bias / cls_resid: defects the per-row host test plants."""
    Lq, Lk = q.shape[1] - 1, k.shape[1] - 1
    t = q @ k.transpose(1, 2)
    bias = hi @ E.t() + lo @ E.t()
    t[:, :Lq, :Lk] += bias
    if cls_bias:
        t[:, Lq, :Lk] += bias[:, Lq - 1]
    s = t * scale
    m = s.amax(-1, keepdim=True)
    pt = torch.exp(s - m)
    l = pt.sum(-1, keepdim=True)
    lse = m + torch.log(l)
    res = q.clone()
    if not cls_resid:
        res[:, Lq] = 0
    oa = rnd(pt / l) @ v if variant else (rnd(pt) @ v) / l
    return dict(o=rnd(oa + res), lse=lse, oa=oa, res=res, s=s)


def pattn_bwd(q, k, v, do, f, E, scale, rnd, variant=False, cls_resid=False, round_dq=True, delta_unrounded=None):
    """... backward; f = what pattn_fwd returned -> dict(delta, ds, dq, dk, dv, drel).  delta_unrounded: D from the unrounded o instead of
    the stored o minus q (default: with `variant`, as pool_attn_checks.model_variant has it)"""
    Lq, Lk = q.shape[1] - 1, k.shape[1] - 1
    dres = do.clone()
    if not cls_resid:
        dres[:, Lq] = 0
    P = torch.exp(f["s"] - f["lse"])
    delta = (do * (f["oa"] if (variant if delta_unrounded is None else delta_unrounded) else f["o"] - f["res"])).sum(-1, keepdim=True)
    ds = rnd(P * (do @ v.transpose(1, 2) - delta))
    dq = scale * (ds @ k) + dres
    return dict(delta=delta, ds=ds, dq=rnd(dq) if round_dq else dq, dk=rnd(scale * (ds.transpose(1, 2) @ q)),
                dv=rnd(rnd(P).transpose(1, 2) @ do), drel=ds[:, :Lq, :Lk] @ E)


def _ln_stats(v, eps=EPS):
    mu = v.mean(-1, keepdim=True)
    return mu, torch.rsqrt((v - mu).pow(2).mean(-1, keepdim=True) + eps)


def pool_ln_fwd(conv32, gm, bt, rnd, variant=False):
    """csrc/mvit.hip pool_fwd behind the fp32 conv -> (c = R(conv), y = R(LN(conv))); variant: the statistics come from the rounded c"""
    cr = rnd(conv32)
    mu, rs = _ln_stats(cr if variant else conv32)
    return cr, rnd((conv32 - mu) * rs * gm + bt)


def pool_ln_bwd(cr, gm, dy, rnd):
    """pool_ln_bwd_kernel: statistics from the ROUNDED c -> (dc = R(dLN(dy | c)), xhat)"""
    mu, rs = _ln_stats(cr)
    xh = (cr - mu) * rs
    gg = dy * gm
    return rnd(rs * (gg - gg.mean(-1, keepdim=True) - xh * (gg * xh).mean(-1, keepdim=True))), xh


# ------------------------------------------------------------------------------------------------ the custom sites
def _conv(x, w, stride):
    """x [n, 1 + L.., d] is passed as the patch grid [n, d, T, H, W]"""
    return F.conv3d(x, w, None, stride=tuple(stride), padding=tuple(kk // 2 for kk in w.shape[2:]), groups=w.shape[0])


class PoolLN(torch.autograd.Function):
    """mvit_oracle.attention_pool as pool_fwd / pool_bwd compute it: t [B, heads, 1 + L, d] (cls FIRST) -> [B, heads, 1 + Lo, d]"""
    @staticmethod
    def forward(ctx, t, w, gm, bt, stride, thw):
        B, N, L1, C = t.shape
        grid = t[:, :, 1:].reshape(B * N, *thw, C).permute(0, 4, 1, 2, 3).contiguous()
        c = _conv(grid, w, stride)
        conv32 = torch.cat((t[:, :, :1], c.reshape(B, N, C, -1).transpose(2, 3)), 2)
        cr, y = pool_ln_fwd(conv32, gm, bt, _rnd, VARIANT)
        ctx.save_for_backward(grid, w, gm, cr)
        ctx.stride, ctx.oshape = stride, c.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        grid, w, gm, cr = ctx.saved_tensors
        dc, xh = pool_ln_bwd(cr, gm, dy, _rnd)
        B, N = dy.shape[:2]
        dcg = dc[:, :, 1:].transpose(2, 3).reshape(ctx.oshape)
        with torch.enable_grad():
            g_, w_ = grid.detach().requires_grad_(True), w.detach().requires_grad_(True)
            gx, gw = torch.autograd.grad(_conv(g_, w_, ctx.stride), [g_, w_], dcg)
        C = dy.shape[-1]
        gx = gx.permute(0, 2, 3, 4, 1).reshape(B, N, -1, C)
        dt = torch.cat((dc[:, :, :1], _rnd(gx)), 2)
        return dt, gw, (dy * xh).sum((0, 1, 2)), dy.sum((0, 1, 2)), None, None


class RelPair(torch.autograd.Function):
    """rel_fwd / the table half of rel_bwd: Qp [n, Lq, d] (16-bit), the three fp32 tables -> [2, n, Lq, J], the hi, lo pair of out_scale * rel.
    Its gradient slot [0] carries drel as attn_bwd hands it over (fp32, the gradient of the unscaled rel); [1] is not read."""
    @staticmethod
    def forward(ctx, Qp, Rh, Rw, Rt, idx, q_thw, out_scale):
        T = [paired(t, _rnd) for t in (Rh, Rw, Rt)]
        hi, lo = pack(rel_terms(Qp, *T, idx, q_thw) * out_scale, _rnd)
        if DEFECT == "rel_single":
            lo = torch.zeros_like(lo)
        if TAPS is not None:          # share of the entries whose lo half is live: a pair, not a single 16-bit value
            TAPS.setdefault("rel_lo", []).append(float((lo != 0)[hi != 0].float().mean()))
        ctx.save_for_backward(Qp, Rh, Rw, Rt)
        ctx.idx, ctx.q_thw = idx, q_thw
        return torch.stack((hi, lo))

    @staticmethod
    def backward(ctx, g):
        Qp, Rh, Rw, Rt = ctx.saved_tensors
        drel = g[0]
        dp = paired(drel, _rnd)
        with torch.enable_grad():
            Q_ = Qp.detach().requires_grad_(True)
            T_ = [t.detach().requires_grad_(True) for t in (Rh, Rw, Rt)]
            rel = rel_terms(Q_, *T_, ctx.idx, ctx.q_thw)
            dQ, = torch.autograd.grad(rel, Q_, drel, retain_graph=True)          # the dQ kernel: plain fp32 tables and drel
            if DEFECT == "table_grad_16bit":          # a 16-bit accumulator: one add per (item, t, h) line of queries
                dT = [torch.zeros_like(t) for t in T_]
                lines = dp.reshape(Qp.shape[0] * ctx.q_thw[0] * ctx.q_thw[1], -1)
                for i in range(lines.shape[0]):
                    sel = torch.zeros_like(lines)
                    sel[i] = lines[i]
                    part = torch.autograd.grad(rel, T_, sel.reshape(dp.shape), retain_graph=True)
                    dT = [_rnd(a + _rnd(b)) for a, b in zip(dT, part)]
            elif VARIANT:
                dT = torch.autograd.grad(rel, T_, dp)
            else:                                       # item by item, in index order
                dT = [torch.zeros_like(t) for t in T_]
                for i in range(Qp.shape[0]):
                    sel = torch.zeros_like(dp)
                    sel[i] = dp[i]
                    part = torch.autograd.grad(rel, T_, sel, retain_graph=True)
                    dT = [a + b for a, b in zip(dT, part)]
        return dQ, dT[0], dT[1], dT[2], None, None, None


class PoolAttn(torch.autograd.Function):
    """attn_fwd / attn_bwd on [n, L + 1, d] tensors with the cls token LAST; pair = RelPair's output"""
    @staticmethod
    def forward(ctx, q, k, v, pair, k_thw, scale):
        E = key_map(k_thw).to(q.dtype)
        f = pattn_fwd(q, k, v, pair[0], pair[1], E, scale, _rnd, VARIANT)
        ctx.save_for_backward(q, k, v, E, f["o"], f["lse"], f["oa"], f["res"], f["s"])
        ctx.scale = scale
        return f["o"]

    @staticmethod
    def backward(ctx, do):
        q, k, v, E, o, lse, oa, res, s = ctx.saved_tensors
        b = pattn_bwd(q, k, v, do, dict(o=o, lse=lse, oa=oa, res=res, s=s), E, ctx.scale, _rnd, VARIANT, round_dq=not VARIANT, delta_unrounded=False)
        return b["dq"], b["dk"], b["dv"], torch.stack((b["drel"], torch.zeros_like(b["drel"]))), None, None


class DQAdd(torch.autograd.Function):
    """q as the attention reads it and q as the rel kernels read it; rel_bwd adds drel . R into the 16-bit dQ: R(dq_attn + dq_rel)"""
    @staticmethod
    def forward(ctx, q):
        return q.view_as(q), q.view_as(q)

    @staticmethod
    def backward(ctx, ga, gr):
        return _rnd(ga + gr)


class _RoundPartial(torch.autograd.Function):
    """DEFECT stem_partial_16bit: the weight as one slice of the rows reads it; that slice's partial gradient sum is rounded"""
    @staticmethod
    def forward(ctx, w):
        return w.view_as(w)

    @staticmethod
    def backward(ctx, g):
        return _rnd(g)


# ------------------------------------------------------------------------------------------------ forward
def _cls_last(t):
    """[B, h, 1 + L, d] cls first -> [B h, L + 1, d] cls last"""
    return torch.cat((t[:, :, 1:], t[:, :, :1]), 2).reshape(-1, t.shape[2], t.shape[3])


def msa(sd, pre, x, blk):
    """mvit_oracle.msa with the kernels' rounding points; x = the 16-bit xn"""
    if not _on():
        return mo.msa(sd, pre, x, blk)
    B, N, _ = x.shape
    h, dout = blk["heads"], blk["dim_out"]
    d = dout // h
    scale = d ** -0.5
    qkv = R(F.linear(x, RW(sd[pre + "qkv.weight"]), sd[pre + "qkv.bias"])).reshape(B, N, 3, h, d).permute(2, 0, 3, 1, 4)
    thw = blk["in_thw"]
    out_thw = lambda st: [(n + 2 - 3) // s + 1 for n, s in zip(thw, st)]
    q_thw, k_thw = out_thw(blk["stride_q"]), out_thw(blk["stride_kv"])
    pool = lambda t, n, st: PoolLN.apply(t, sd[pre + f"pool_{n}.weight"], sd[pre + f"norm_{n}.weight"], sd[pre + f"norm_{n}.bias"],
                                         tuple(st), tuple(thw))
    q, k, v = pool(qkv[0], "q", blk["stride_q"]), pool(qkv[1], "k", blk["stride_kv"]), pool(qkv[2], "v", blk["stride_kv"])
    Lq = q.shape[2] - 1
    qa, qr = DQAdd.apply(_cls_last(q))
    idx = (mo.rel_index(q_thw[1], k_thw[1]), mo.rel_index(q_thw[2], k_thw[2]), mo.rel_index(q_thw[0], k_thw[0]))
    pair = RelPair.apply(qr[:, :Lq], sd[pre + "rel_pos_h"], sd[pre + "rel_pos_w"], sd[pre + "rel_pos_t"], idx, tuple(q_thw), 1.0 / scale)
    o = PoolAttn.apply(qa, _cls_last(k), _cls_last(v), pair, tuple(k_thw), scale).reshape(B, h, Lq + 1, d)
    o = torch.cat((o[:, :, Lq:], o[:, :, :Lq]), 2).transpose(1, 2).reshape(B, -1, dout)
    return F.linear(R(o), RW(sd[pre + "proj.weight"]), sd[pre + "proj.bias"]), q_thw


def _dp(t, s):
    """DropPath factor s [B] (None = identity) on the branch t whose incoming gradient is cast to 16 bits: the factor goes in FIRST"""
    if DEFECT == "droppath_after_cast":
        z = RB(t if s is None else t * s[:, None, None])
    else:
        z = RB(t) if s is None else RB(t) * s[:, None, None]
    if TAPS is not None and ro.OPERAND is not None and s is not None and t.requires_grad:
        # the 16-bit gradient operand the branch's backward GEMMs read must be R(factor x fp32 gradient): share of entries where it is not
        box = {}
        z.register_hook(lambda g: box.__setitem__("g", g.detach()))
        t.register_hook(lambda g, dt=ro.OPERAND: TAPS.setdefault("dp_cast", []).append(
            float((g != (box["g"] * s[:, None, None]).to(dt).float()).float().mean())))
    return z


def block(sd, pre, x, blk, dp=None):
    """mvit_oracle.block with the engine's rounding points (MViTEngine._block_fwd / _block_bwd)"""
    same = blk["dim"] == blk["dim_out"]
    xn = mo.ln(x, sd[pre + "norm1.weight"], sd[pre + "norm1.bias"])
    tap = TAPS is not None and ro.OPERAND is not None and xn.requires_grad
    if tap:           # the gradient norm1's backward reads: dqkv W_qkv, plus dxs W_skip where dim != dim_out
        xn.register_hook(lambda g, pre=pre, dt=ro.OPERAND: TAPS.setdefault("dxn_sum", {}).__setitem__(pre, valued16(g, dt)))
    if same:          # one consumer: the 16-bit output of the W_qkv^T GEMM is what norm1's backward reads
        xn = xa = R(xn)
    else:             # dxn = dqkv W_qkv is written fp32 (PVRL_EPI_F32) and the skip projection's GEMM adds dxs W_skip to it (its `aux`)
        xn = RW(xn)
        xa = xn.view_as(xn)           # the copy the attention branch reads: its gradient is dxn alone
        if tap:
            xa.register_hook(lambda g, pre=pre, dt=ro.OPERAND: TAPS.setdefault("dxn", {}).__setitem__(pre, valued16(g, dt)))
        if DEFECT == "dxn_16bit":     # the W_qkv^T GEMM with the 16-bit epilogue here too
            xa = RB(xa)
    xb, _ = msa(sd, pre + "attn.", xa, blk)
    if not same:
        x = RB(F.linear(xn, RW(sd[pre + "proj.weight"]), sd[pre + "proj.bias"]))
    x = mo.pool_skip(x, blk["stride_q"], blk["in_thw"]) + _dp(xb, None if dp is None else dp[0])
    if DEFECT == "resid_16bit":
        x = RW(x)
    xn = R(mo.ln(x, sd[pre + "norm2.weight"], sd[pre + "norm2.bias"]))
    u = RB(F.linear(xn, RW(sd[pre + "mlp.fc1.weight"]), sd[pre + "mlp.fc1.bias"]))
    g = RW(GeluStore.apply(u)) if ro.OPERAND is not None else F.gelu(u)
    y = F.linear(g, RW(sd[pre + "mlp.fc2.weight"]), sd[pre + "mlp.fc2.bias"])
    x = x + _dp(y, None if dp is None else dp[1])
    return RW(x) if DEFECT in ("x2_16bit", "resid_16bit") else x


def forward_features(sd, x, mv, block_outputs=None, droppath=None):
    """mvit_oracle.forward_features with the HIP datapath's rounding points (module docstring)"""
    _, blocks = mo.plan(mv, x.shape[2], x.shape[3])
    conv = lambda xx, w: F.conv3d(R(xx), RW(w), sd["patch_embed.proj.bias"], stride=tuple(mv["PATCH_STRIDE"]), padding=tuple(mv["PATCH_PADDING"]))
    if DEFECT == "stem_partial_16bit":      # one 16-bit partial per clip instead of one fp32 sum over all rows
        t = torch.cat([conv(x[b:b + 1], _RoundPartial.apply(sd["patch_embed.proj.weight"])) for b in range(x.shape[0])])
    else:
        t = conv(x, sd["patch_embed.proj.weight"])
    t = (RW(RB(t)) if DEFECT == "resid_16bit" else RB(t)).flatten(2).transpose(1, 2)
    t = torch.cat((sd["cls_token"].expand(t.shape[0], -1, -1), t), dim=1)
    for i, blk in enumerate(blocks):
        t = block(sd, f"blocks.{i}.", t, blk, dp=None if droppath is None else droppath[i])
        if block_outputs is not None:
            block_outputs.append(t)
    t = mo.ln(t, sd["norm.weight"], sd["norm.bias"])
    return t[:, 0]
