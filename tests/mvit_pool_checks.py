"""The MViTv2 pooling-operator kernels of csrc/mvit.hip -- attention_pool (pvrl_mvit_pool_fwd / _bwd), the max-pool skip
(pvrl_mvit_maxpool_fwd / _bwd), im2col (pvrl_im2col3d_bf16) and the any-width LayerNorm (pvrl_layernorm_g_fwd / _bwd) -- against an fp64
reference PER TOKEN, through every dispatch path, inside guard bands.

Used by tests/test_mvit_pool_gpu.py (pytest -m gpu: the HIP kernels through the C ABI) and tests/test_mvit_pool_harness_host.py (no GPU:
the rounding model stands in for the kernel, planted defects show that the rules bite).  Metric (`rowerr`, `agg`), tolerance rule
(`judge_tensor`, ROW_FACTOR), guard bands (`Guarded`, `guarded_input`) and the small-case rule (MIN_ROWS) are those of
tests/attn_checks.py, imported through tests/pool_attn_checks.py; read those docstrings first.  Only what differs is said here.

attention_pool
  Reference.  fp64 autograd of oracle.mvit_oracle.attention_pool (depthwise Conv3d 3x3x3, padding 1, + LayerNorm(96), the cls token
  skipping the conv) on the 16-bit-valued inputs.
  Rounding model (`pool_model`), RESTATED FROM THE KERNELS (pool_fwd*_kernel, pool_ln_bwd_kernel, pool_dgrad*_kernel, pool_wgrad*_kernel):
  c = R16(fp32 conv) is what conv_out holds; y = R16(LN(unrounded fp32 conv)); the backward takes mu and rstd from the ROUNDED c,
  dc = R16(dLN(dy | c)); the cls token's dc is copied to its dqkv row; dX = R16(fp32 transposed conv of dc); dw, dgamma, dbeta are fp32
  sums over the rounded dc / dy and the 16-bit x, ACCUMULATED into their buffers: those start non-zero and are compared with start +
  gradient.  `variant=True`: the forward's LN statistics come from the rounded c -- another legitimate implementation the rule lets pass.
  Rule.  Rows of 96 per (item, token): y [BH, Lo + 1, 96] and dX [BH, L + 1, 96] (cls LAST in both, so the cls rows are rows of the same
  tensors); rowerr(kernel) <= ROW_FACTOR rowerr(model); aggregate <= the flat bounds of mvit_checks.check_mvit_pool (6e-3 forward, 1.5e-2
  backward) in `randn`, <= ROW_FACTOR agg(model) elsewhere.  dw in rows of 27 per channel, dgamma and dbeta as one row of 96 per draw:
  the same rule with judge_tensor's zero-reference floor (`sum_floor`: the worst case of an n-term fp32 sum).
  conv_out, ELEMENTWISE, derived: |c - c64| <= ulp16(c64) / 2 + 27 * 2^-24 * sum_i |x_i w_i| (one rounding to 16 bits plus the worst case
  of a 27-term fp32 FMA chain in any order).
  Exact tap map (`check_tap_map`).  For each of the 27 taps w[c][tap] = 1 and every other weight 0, x = distinct 16-bit values: conv_out
  must be BIT-EQUAL to the shifted input (zero where the tap leaves the grid).  The ABI does not take dc, but it hands it back
  (dc_scratch): dX must be bit-equal to the transposed shift of the dc the kernel itself wrote, and the cls dqkv row to dc's cls row.
  dw[c][tap'] is then sum dc * x shifted by tap' -- judged by the row rule like everywhere.
  Regimes.  randn; offset (every token = a common vector of size ~30 + 0.1 N(0, 1): LN cancels the vector, rounding c costs most of
  the signal, forward and backward statistics part ways); constant (one-hot centre-tap weights and a quarter of the tokens constant over
  the 96 channels: c constant, y = beta, rstd = eps^-0.5); impulse (one non-zero patch token per clip); hot (|x| ~ 200).
  Dispatch (`pool_names`).  fwd_t<dense> (st = 1, a spatial stride > 1), fwd_t<sparse> (1, 1, 1), fwd (st > 1); dgrad_t<true,1>,
  dgrad_t<false,2|4|8> (st = 1, sh = sw = 2 | 4 | 8), dgrad_t<false,0> (st = 1, anything else), dgrad (st > 1); wgrad_t (st = 1), wgrad;
  ln_bwd, ln_bwd.loop when B H (Lo + 1) > 32,768 (the grid-stride loop of pool_ln_bwd_kernel).  pool_dgrad_kernel has run-time strides
  only: a compile-time spatial stride S > 0 exists only for st = 1, and st = 1 always takes a dgrad_t form, so pool_dgrad_kernel<S > 0>
  could never be reached from pvrl_mvit_pool_bwd and is gone from mvit.hip.  NOT reachable at test size and left to the end-to-end checks
  (mvit_checks.check_mvit_timed_config_train_step): the `grid_blocks` cap (1,048,560 workgroups) and PW_MAX_WG (2,048 workgroups of the
  weight gradient = 262,144 output tokens).
max-pool skip
  Reference mvit_oracle.pool_skip in fp64; both outputs BIT-EXACT (the forward selects; dy is drawn from multiples of 2^-6 with
  |dy| <= 4, so a sum of up to four is exact in any order).  The saved argmax bytes are decoded and compared with the indices of torch's
  max_pool3d (first maximum in scan order); the re-scanning and the saved-argmax backward must agree with each other and the reference.
  Regimes: randn, ties (x from {-1, 0, 1}), plateau (x constant).
im2col
  Bit-exact against `unfold` of the once-rounded input, padding columns exactly zero.  `im2col_kernel` restates `rows_form`.  (W = 244
  still satisfies every clause of rows_form -- 244 + 4 + 7 = 255 <= 256 -- so it is kept as the largest rows-form width and W = 248 is the
  first width the pitch clause sends to the generic kernel.)
LayerNorm (ln_g, and the split-row LayerNorm of csrc/norm.hip: pvrl_layernorm_fwd / _bwd / _split, C = 512 / 768)
  One row judge against fp64 layer_norm, rows of C.  fp32 outputs: rowerr <= max(ROW_FACTOR model, REL_Y_FACTOR Y), Y = the row error of
  plain fp32 torch layer_norm (forward) / its autograd (backward) against fp64, the model (`ln_model`) the kernels' own two-pass arithmetic
  and summation order restated in fp32 (see there for why the two differ on constant rows and on rows with a large mean); 16-bit outputs (y16, the fused dx16 = R16(rowscale dx)):
  ROW_FACTOR model.  mean AND rstd: per entry (rows of 1) under the Y rule.  dgamma / dbeta start
  non-zero.  The backward is handed the mean / rstd the forward kernel wrote, as the engine does.  Regimes: randn, offset (mean 100, spread
  0.01), constant rows, hot, one_live (one non-zero channel).
  norm.hip: rows [0, rows16) of x, dx_in and dx_out live in a 16-bit matrix, the others in an fp32 one; the 16-bit rows of dx_out are
  R16(dx_in + dLN) (ROW_FACTOR model), the fp32 rows take the Y rule; dxs = R16(dxs_scale dx_out) on its first dxs_rows rows, dxsum = start
  + the column sums of those rows of the UNROUNDED dx_out; every backward runs twice, with the immediate and with the deferred (batched)
  reduce, whose dgamma / dbeta / dxsum / dx_out must be bit-equal.
"""
import collections
import zlib

import torch
import torch.nn.functional as F

import pool_attn_checks as pc
from pool_attn_checks import Finding, Guarded, guarded_input, rowerr, agg, ROW_FACTOR, MIN_ROWS, report, BF  # noqa: F401 (re-exported)
from attn_checks import judge_tensor
from oracle import mvit_oracle as mo
from oracle import mvit_rounded_oracle as mro

D = 96
EPS = mro.EPS
AGG_FWD, AGG_BWD = 6e-3, 1.5e-2          # mvit_checks.check_mvit_pool
REL_Y_FACTOR = pc.REL_Y_FACTOR
WS_TAIL, WS_FILL = pc.WS_TAIL, pc.WS_FILL
POOL_REGIMES = ("randn", "offset", "constant", "impulse", "hot")
MAXPOOL_REGIMES = ("randn", "ties", "plateau")
LN_REGIMES = ("randn", "offset", "constant", "hot", "one_live")


def _rnd(x, dt):
    return x.to(dt).float()


def pad128(n):
    return (n + 127) // 128 * 128


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) % (1 << 31))


def ulp16(v, dt):
    """spacing of the 16-bit type at |v| (fp64 tensor); the subnormal spacing below the smallest normal"""
    mant, emin = (10, -14) if dt == torch.float16 else (7, -126)
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** emin)))
    return torch.exp2(e - mant)


# =====================================================================================================================
# attention_pool
# =====================================================================================================================
PoolCase = collections.namedtuple("PoolCase", "B H thw stride slot pad kernel")
# slot: the tensor's place in the packed activation (col0 = slot * H * 96); pad: ld = pad128(3 H 96) instead of 3 H 96 exactly


def out_thw(thw, stride):
    return tuple((n + 2 - 3) // s + 1 for n, s in zip(thw, stride))


def pool_names(B, H, thw, stride):
    """the dispatch of pvrl_mvit_pool_fwd / _bwd restated (module docstring)"""
    st, sh, sw = stride
    o = out_thw(thw, stride)
    if st == 1:
        fwd = "fwd_t<dense>" if (sh > 1 or sw > 1) else "fwd_t<sparse>"
        if sh == 1 and sw == 1:
            dg = "dgrad_t<true,1>"
        elif sh == sw and sh in (2, 4, 8):
            dg = f"dgrad_t<false,{sh}>"
        else:
            dg = "dgrad_t<false,0>"
        wg = "wgrad_t"
    else:
        fwd, dg, wg = "fwd", "dgrad", "wgrad"
    ntok = B * H * (o[0] * o[1] * o[2] + 1)
    return [fwd, dg, wg, "ln_bwd.loop" if ntok > 2048 * 16 else "ln_bwd"]


def fwd_grid(c):
    """workgroups of the forward launch (grid_blocks(16 lanes per column / token, 256 threads)): the XCD launch-order remap sees it"""
    o = out_thw(c.thw, c.stride)
    n = c.B * c.H * ((o[1] * o[2] if c.stride[0] == 1 else o[0] * o[1] * o[2]) + 1)
    return max(1, -(-n * 16 // 256))


def _pool(B, H, thw, stride, slot=1, pad=True):
    return PoolCase(B, H, tuple(thw), tuple(stride), slot, pad, "+".join(pool_names(B, H, thw, stride)))


def _build_pool_cases():
    c = []
    bh = [(2, 2), (1, 3), (3, 1), (2, 1), (1, 2)]
    geoms = [((1, 1, 1), (1, 2, 2)), ((2, 2, 2), (1, 2, 2)), ((3, 7, 5), (1, 2, 2)), ((5, 3, 9), (1, 2, 2)), ((8, 14, 14), (1, 2, 2)),
             ((2, 6, 10), (1, 4, 4)), ((3, 8, 8), (1, 4, 4)),
             ((2, 8, 8), (1, 8, 8)), ((3, 9, 17), (1, 8, 8)), ((1, 3, 3), (1, 8, 8)),          # the last: stride larger than the plane
             ((3, 7, 7), (1, 3, 3)), ((2, 6, 8), (1, 2, 4)),
             ((1, 6, 6), (1, 1, 1)), ((3, 6, 10), (1, 1, 1)), ((2, 1, 9), (1, 1, 1)), ((4, 2, 1), (1, 1, 1)),
             ((4, 6, 6), (2, 2, 2)), ((5, 5, 7), (2, 2, 2)), ((1, 4, 4), (2, 1, 1)), ((7, 3, 3), (3, 1, 1))]
    for i, (thw, stride) in enumerate(geoms):
        B, H = bh[i % len(bh)]
        c.append(_pool(B, H, thw, stride, slot=i % 3, pad=i % 2 == 0))
    # launch order: (2, 6, 6) / (1, 2, 2) has 3 x 3 + 1 = 10 columns per (clip, head); 14, 26 and 12 of them -> 9, 17 and 8 workgroups
    c += [_pool(7, 2, (2, 6, 6), (1, 2, 2)), _pool(13, 2, (2, 6, 6), (1, 2, 2)), _pool(4, 3, (2, 6, 6), (1, 2, 2))]
    # heads
    c += [_pool(1, 3, (2, 5, 6), (1, 2, 2), slot=2), _pool(1, 8, (2, 5, 6), (1, 2, 2), slot=0), _pool(1, 8, (3, 4, 4), (1, 1, 1), slot=2, pad=False)]
    # column slice x leading dimension
    for slot in (0, 1, 2):
        for pad in (False, True):
            c.append(_pool(2, 1, (2, 4, 6), (1, 2, 2), slot=slot, pad=pad))
    # the grid-stride loop of pool_ln_bwd_kernel: 34,849 pooled tokens
    c.append(_pool(1, 1, (8, 66, 66), (1, 1, 1)))
    return c


POOL_CASES = _build_pool_cases()


def pool_case_id(c):
    return (f"pool-B{c.B}xH{c.H}-{'x'.join(map(str, c.thw))}-s{'x'.join(map(str, c.stride))}-slot{c.slot}-"
            f"{'pad128' if c.pad else 'ld3d'}-g{fwd_grid(c)}-{c.kernel}")


def _build_pool_tests():
    """every case runs `randn`; the first case to reach an instantiation not seen before runs every regime (the 34,849-token case: `randn` only)"""
    tests, seen = [], set()
    for c in POOL_CASES:
        regs = ["randn"]
        new = [k for k in c.kernel.split("+") if k not in seen and k != "ln_bwd.loop"]
        if new:
            seen.update(new)
            regs += [r for r in POOL_REGIMES if r != "randn"]
        tests += [(c, r) for r in regs]
    return tests


POOL_TESTS = _build_pool_tests()


def pool_draws(c):
    o = out_thw(c.thw, c.stride)
    rows = c.B * c.H * (o[0] * o[1] * o[2] + 1)
    return 1 if rows >= MIN_ROWS else min(256, -(-MIN_ROWS // rows))


def make_pool_problem(c, regime, operand=None, draw=0, tap=None):
    """-> dict of CPU fp32 tensors (16-bit-valued where the kernels take 16 bits): x [BH, L + 1, 96] and dy [BH, Lo + 1, 96] (cls LAST),
    w [96, 27], gamma, beta, and the start values of dw, dgamma, dbeta.  tap: the exact tap-map inputs (w one-hot at `tap`, x distinct)."""
    operand = BF if operand is None else operand
    g = _gen("pool", c.B, c.H, c.thw, c.stride, regime, draw, tap)
    BH, L = c.B * c.H, c.thw[0] * c.thw[1] * c.thw[2]
    o = out_thw(c.thw, c.stride)
    Lo = o[0] * o[1] * o[2]
    x = torch.randn(BH, L + 1, D, generator=g)
    w = torch.randn(D, 27, generator=g) * 0.2
    if tap is not None:
        # 2,048 distinct values exact in fp16 and bf16 (8 significant bits): +- an odd integer below 256 times 2^0 .. 2^-7, dealt at random
        n = BH * (L + 1) * D
        idx = torch.randperm(n, generator=g)
        vals = ((2 * (idx % 128) + 1).float() * torch.exp2(-(idx // 128 % 8).float())) * torch.where(idx // 1024 % 2 == 0, 1.0, -1.0)
        x = vals.reshape(BH, L + 1, D)
        w = torch.zeros(D, 27)
        w[:, tap] = 1.0
    elif regime == "offset":
        vec = 30.0 * torch.randn(BH, 1, D, generator=g)
        x = vec + 0.1 * x
    elif regime == "constant":
        const = torch.rand(BH, L + 1, generator=g) < 0.25
        x = torch.where(const[..., None], x[..., :1].expand_as(x), x)
        w = torch.zeros(D, 27)
        w[:, 13] = 1.0
    elif regime == "impulse":
        keep = torch.zeros(c.B, L + 1, dtype=torch.bool)
        keep[torch.arange(c.B), torch.randint(0, L, (c.B,), generator=g)] = True
        keep[:, L] = True                                                  # the cls token stays as drawn
        x = x * keep[:, None, :, None].expand(c.B, c.H, L + 1, 1).reshape(BH, L + 1, 1)
    elif regime == "hot":
        x = x * 200.0
    gm = 1 + 0.1 * torch.randn(D, generator=g)
    bt = 0.1 * torch.randn(D, generator=g)
    return dict(x=_rnd(x, operand), w=w, gamma=gm, beta=bt, dy=_rnd(torch.randn(BH, Lo + 1, D, generator=g), operand),
                dw0=torch.randn(D, 27, generator=g), dgamma0=torch.randn(D, generator=g), dbeta0=torch.randn(D, generator=g))


def _grid(x, c):
    """patch tokens [BH, L, 96] -> [BH, 96, T, Hh, Ww]"""
    return x.reshape(x.shape[0], *c.thw, D).permute(0, 4, 1, 2, 3)


def _tokens(t):
    """[BH, 96, To, Ho, Wo] -> [BH, Lo, 96]"""
    return t.reshape(t.shape[0], D, -1).transpose(1, 2)


def conv(x, w, c):
    """depthwise conv of the patch tokens, cls row appended unchanged: x [BH, L + 1, 96] -> [BH, Lo + 1, 96] (any dtype)"""
    L = x.shape[1] - 1
    t = F.conv3d(_grid(x[:, :L], c), w.reshape(D, 1, 3, 3, 3), None, stride=c.stride, padding=1, groups=D)
    return torch.cat((_tokens(t), x[:, L:]), 1)


def pool_reference(p, c):
    """fp64: y, c (the conv output), dX, dw, dgamma, dbeta (start + gradient), absxw = sum_i |x_i w_i| per conv output"""
    L = p["x"].shape[1] - 1
    x = p["x"].double().requires_grad_(True)
    w, gm, bt = (p[n].double().requires_grad_(True) for n in ("w", "gamma", "beta"))
    t = torch.cat((x[:, L:], x[:, :L]), 1).reshape(c.B, c.H, L + 1, D)                      # the oracle wants the cls token FIRST
    y, _ = mo.attention_pool(t, w.reshape(D, 1, 3, 3, 3), c.stride, c.thw, gm, bt)
    y = y.reshape(c.B * c.H, -1, D)
    y = torch.cat((y[:, 1:], y[:, :1]), 1)
    gx, gw, gg, gb = torch.autograd.grad(y, [x, w, gm, bt], p["dy"].double())
    with torch.no_grad():
        c64 = conv(p["x"].double(), p["w"].double(), c)
        absxw = conv(p["x"].double().abs(), p["w"].double().abs(), c)
    return dict(y=y.detach(), c=c64, absxw=absxw, dX=gx, dw=p["dw0"].double() + gw, dgamma=p["dgamma0"].double() + gg,
                dbeta=p["dbeta0"].double() + gb)


def pool_model(p, c, operand, variant=False, defect=None):
    """the kernels' rounding model (module docstring) -> y, c, dc, dX (16-bit-valued), dw, dgamma, dbeta (fp32, start + gradient).
    defect: one of the structural defects tests/test_mvit_pool_harness_host.py plants (`POOL_DEFECTS`)."""
    L = p["x"].shape[1] - 1
    x, w, gm, bt, dy = p["x"], p["w"], p["gamma"], p["beta"], p["dy"]
    o = out_thw(c.thw, c.stride)
    HoWo = o[1] * o[2]
    xg = x.clone().requires_grad_(True)
    wg = w.clone().requires_grad_(True)
    conv32 = conv(xg, wg, c)
    if defect == "border_taps_transposed":          # outputs on the plane's border use the (yy, xx)-transposed tap
        wt = wg.reshape(D, 3, 3, 3).transpose(2, 3).reshape(D, 27)
        alt = conv(xg, wt, c)
        pos = torch.arange(o[0] * HoWo) % HoWo
        yo, xo = pos // o[2], pos % o[2]
        border = (yo == 0) | (yo == o[1] - 1) | (xo == 0) | (xo == o[2] - 1)
        border = torch.cat((border, torch.tensor([False])))
        conv32 = torch.where(border[None, :, None], alt, conv32)
    elif defect == "last_frame_from_t_sum":         # fwd_t: the last frame's output stored from the running sum of output t = T, which
        w3 = wg.reshape(D, 3, 9)                     # holds only the last input frame through the a = 0 taps
        wz = torch.cat((torch.zeros(D, 1, 9), w3[:, :1], torch.zeros(D, 1, 9)), 1).reshape(D, 27)
        alt = conv(xg, wz, c)
        last = torch.arange(o[0] * HoWo + 1) // HoWo == o[0] - 1
        conv32 = torch.where(last[None, :, None], alt, conv32)
    elif defect == "cls_through_conv":              # the cls token is multiplied by the centre tap
        conv32 = torch.cat((conv32[:, :-1], conv32[:, -1:] * wg[:, 13]), 1)
    # the rounding points themselves: oracle/mvit_rounded_oracle.py (one restatement of the kernels for the per-token and the end-to-end rule)
    rnd = lambda t: _rnd(t, operand)
    cr, y = mro.pool_ln_fwd(conv32.detach(), gm, bt, rnd, variant)
    dc, xh = mro.pool_ln_bwd(cr, gm, dy, rnd)
    dcg = dc.clone()
    dc_w = dc.clone()
    if defect == "dgrad_drops_last_output_row" and c.thw[1] % 2 == 1:
        rowsel = (torch.arange(o[0] * HoWo) % HoWo) // o[2] == o[1] - 1
        dcg[:, :-1][:, rowsel] = 0.0
    if defect == "wgrad_skips_last_frame" and c.thw[0] % 2 == 1:
        dc_w[:, (o[0] - 1) * HoWo:o[0] * HoWo] = 0.0
    gx, = torch.autograd.grad(conv32, xg, dcg, retain_graph=True)
    gw, = torch.autograd.grad(conv32, wg, dc_w)
    dX = _rnd(gx, operand)
    return dict(y=y, c=cr, dc=dc, dX=dX, dw=p["dw0"] + gw, dgamma=p["dgamma0"] + (dy * xh).sum((0, 1)), dbeta=p["dbeta0"] + dy.sum((0, 1)))


POOL_DEFECTS = ("border_taps_transposed", "last_frame_from_t_sum", "cls_through_conv", "dgrad_drops_last_output_row", "wgrad_skips_last_frame")


def _ploc(c, S_unit="token"):
    BH = c.B * c.H

    def where(flat, S):
        draw, item = divmod(flat // S, BH)
        return f"(clip {item // c.H}, head {item % c.H}, {S_unit} {flat % S}" + (f"; draw {draw})" if draw else ")")
    return where


def judge_conv_out(c, got, ref, operand):
    """the derived elementwise bound on conv_out; cls rows must equal the input exactly (absxw = |x| there, c64 = x: bound = 0 + fp32 term,
    so they are compared for equality separately)"""
    bound = ulp16(ref["c"], operand) / 2 + 27 * 2.0 ** -24 * ref["absxw"]
    err = (got.double() - ref["c"]).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    slack = err - bound
    i = int(slack.argmax())
    S = got.shape[1]
    e, b = err.reshape(-1)[i].item(), bound.reshape(-1)[i].item()
    cls_same = torch.equal(got[:, -1].double(), ref["c"][:, -1])
    return [Finding("conv_out elementwise (derived bound)", e <= b, e, b,
                    f"worst entry {_ploc(c)(i // D, S)} channel {i % D}; {int((slack > 0).sum())} entries over their bound"),
            Finding("conv_out cls rows equal the input", cls_same, 0.0 if cls_same else 1.0, 0.0, "")]


def sum_floor(terms_abs_sum, n):
    """worst-case error of an n-term fp32 sum in any order: n 2^-24 sum |terms| (the zero-reference floor of the accumulated tensors)"""
    return n * 2.0 ** -24 * terms_abs_sum


def judge_pool(c, regime, got, ref, mod, p, operand):
    """got / mod: y, c [n, Lo + 1, 96], dX [n, L + 1, 96], dw [draws 96, 27], dgamma, dbeta [draws, 96] -> list of Finding"""
    fwd_b, bwd_b = (AGG_FWD, AGG_BWD) if regime == "randn" else (None, None)
    out = judge_conv_out(c, got["c"], ref, operand)
    out += judge_tensor(None, "y", got["y"], ref["y"], mod["y"], None, fwd_b, where=_ploc(c))
    out += judge_tensor(None, "dX", got["dX"], ref["dX"], mod["dX"], None, bwd_b, where=_ploc(c))
    ntok = p["dy"].shape[0] * p["dy"].shape[1]
    fl_w = sum_floor(float(mod["dc"].abs().sum() * p["x"].abs().max()), ntok)
    fl_g = sum_floor(float(p["dy"].abs().sum()) * 10.0, ntok)          # |xhat| <= sqrt(95) < 10
    ch = lambda flat, S: f"(channel {flat % D}" + (f"; draw {flat // D})" if flat >= D else ")")
    dr = lambda flat, S: f"(draw {flat})"
    out += judge_tensor(None, "dw (start + gradient)", got["dw"][None], ref["dw"][None], mod["dw"][None], None, bwd_b, fl_w, where=ch)
    for n in ("dgamma", "dbeta"):
        out += judge_tensor(None, n + " (start + gradient)", got[n][None], ref[n][None], mod[n][None], None, bwd_b, fl_g, where=dr)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the kernels (GPU), through the C ABI: every output inside a guard band
# ---------------------------------------------------------------------------------------------------------------------
def _abi():
    return pc._abi()


def to_packed(x, c):
    """[BH, L + 1, 96] (cls LAST) -> token-major [B L + B, H 96]"""
    return pc.to_tok(x, c.B, c.H)


def from_packed(t, c):
    return pc.from_tok(t, c.B, c.H)


def gpu_pool(c, p, dev, call_bwd=True):
    """pvrl_mvit_pool_fwd + _bwd -> (outputs as CPU fp32 in the layouts of `pool_model`, guard findings)"""
    L_, ptr, stream = _abi()
    B, H, BH = c.B, c.H, c.B * c.H
    T, Hh, Ww = c.thw
    L = T * Hh * Ww
    o = out_thw(c.thw, c.stride)
    Lo = o[0] * o[1] * o[2]
    dout = H * D
    ld = pad128(3 * dout) if c.pad else 3 * dout
    col0 = c.slot * dout
    rows = B * L + B
    f32 = torch.float32
    packed = torch.full((rows, 3 * dout), 3.0)                           # the other two tensors of the activation: a constant that would show
    packed[:, col0:col0 + dout] = to_packed(p["x"], c)
    qkv = guarded_input(packed, BF, dev, ld - 3 * dout)
    un = [(0, 0, rows, 0, col0), (0, 0, rows, col0 + dout, 3 * dout)]
    b = dict(y=Guarded("y", [BH * (Lo + 1)], D, BF, device=dev), c=Guarded("conv_out", [BH * (Lo + 1)], D, BF, device=dev),
             dc=Guarded("dc_scratch", [BH * (Lo + 1)], D, BF, device=dev),
             dqkv=Guarded("dqkv", [rows], 3 * dout, BF, ld - 3 * dout, unowned=un, device=dev),
             dw=Guarded("dw", [D], 27, f32, device=dev), dgamma=Guarded("dgamma", [1], D, f32, device=dev),
             dbeta=Guarded("dbeta", [1], D, f32, device=dev))
    w, gm, bt = (guarded_input(p[n].reshape(-1, p[n].shape[-1]), f32, dev, 0) for n in ("w", "gamma", "beta"))
    L_.call("pvrl_mvit_pool_fwd", ptr(qkv), ld, col0, B, H, T, Hh, Ww, *c.stride, ptr(w), ptr(gm), ptr(bt), EPS, ptr(b["y"].seg(0)),
            ptr(b["c"].seg(0)), stream())
    dy = guarded_input(p["dy"].reshape(-1, D), BF, dev, 0)
    b["dw"].seg(0).copy_(p["dw0"])
    b["dgamma"].seg(0).copy_(p["dgamma0"][None])
    b["dbeta"].seg(0).copy_(p["dbeta0"][None])
    nbytes = int(L_.call("pvrl_mvit_pool_bwd_workspace_bytes"))
    ws = pc._workspace(nbytes, dev)
    L_.call("pvrl_mvit_pool_bwd", ptr(dy), ptr(b["c"].seg(0)), ptr(qkv), ptr(b["dqkv"].seg(0)), ld, col0, B, H, T, Hh, Ww, *c.stride,
            ptr(w), ptr(gm), EPS, ptr(b["dc"].seg(0)), ptr(b["dw"].seg(0)), ptr(b["dgamma"].seg(0)), ptr(b["dbeta"].seg(0)), ptr(ws),
            nbytes, stream())
    torch.cuda.synchronize()
    f = pc._ws_check("pool_bwd", ws, nbytes)
    for g in b.values():
        f += g.check()
    cpu = lambda t: t.float().cpu()
    got = dict(y=cpu(b["y"].seg(0)).reshape(BH, Lo + 1, D), c=cpu(b["c"].seg(0)).reshape(BH, Lo + 1, D),
               dc=cpu(b["dc"].seg(0)).reshape(BH, Lo + 1, D), dX=from_packed(cpu(b["dqkv"].seg(0))[:, col0:col0 + dout], c),
               dw=cpu(b["dw"].seg(0)), dgamma=cpu(b["dgamma"].seg(0))[0], dbeta=cpu(b["dbeta"].seg(0))[0])
    return got, f


def _stack_pool(parts):
    out = {}
    for k in parts[0]:
        if k in ("dgamma", "dbeta", "dgamma0", "dbeta0", "gamma", "beta"):
            out[k] = torch.stack([q[k] for q in parts])
        else:
            out[k] = torch.cat([q[k] for q in parts])
    return out


def check_pool_case(c, regime, run=None, operand=None):
    """one case x regime -> list of Finding; small cases: `pool_draws` draws, every statistic over all of them.
    run(c, p) -> (outputs, findings): the host test passes a stand-in for the GPU."""
    operand = BF if operand is None else operand
    if run is None:
        dev = torch.device("cuda:0")
        run = lambda c, p: gpu_pool(c, p, dev)
    findings, P, G, R, M = [], [], [], [], []
    for d in range(pool_draws(c)):
        p = make_pool_problem(c, regime, operand, d)
        got, f = run(c, p)
        findings += [x for x in f if d == 0 or not x.ok]
        P.append(p)
        G.append(got)
        R.append(pool_reference(p, c))
        M.append(pool_model(p, c, operand))
    return findings + judge_pool(c, regime, _stack_pool(G), _stack_pool(R), _stack_pool(M), _stack_pool(P), operand)


# one small geometry per forward / dgrad / wgrad instantiation
TAP_CASES = [_pool(1, 2, (3, 5, 4), (1, 2, 2), slot=1), _pool(2, 1, (2, 6, 5), (1, 4, 4), slot=0), _pool(1, 1, (2, 9, 10), (1, 8, 8), slot=2),
             _pool(1, 1, (3, 5, 7), (1, 3, 3), slot=1, pad=False), _pool(1, 1, (2, 4, 6), (1, 2, 4), slot=1), _pool(1, 2, (3, 4, 5), (1, 1, 1), slot=2),
             _pool(1, 1, (5, 5, 4), (2, 2, 2), slot=0, pad=False), _pool(1, 1, (7, 3, 3), (3, 1, 1), slot=1)]


def check_tap_map(c, run=None, operand=None):
    """the exact tap-map check of the module docstring, all 27 taps on one geometry"""
    operand = BF if operand is None else operand
    if run is None:
        dev = torch.device("cuda:0")
        run = lambda c, p: gpu_pool(c, p, dev)
    out = []
    L = c.thw[0] * c.thw[1] * c.thw[2]
    for tap in range(27):
        p = make_pool_problem(c, "randn", operand, 0, tap=tap)
        got, f = run(c, p)
        out += [x for x in f if not x.ok]
        want = conv(p["x"].double(), p["w"].double(), c)
        bad = got["c"].double() != want
        nb = int(bad.sum())
        wb = tuple(int(v) for v in bad.nonzero()[0]) if nb else None
        out.append(Finding(f"tap {tap} (a, yy, xx) = {(tap // 9, tap // 3 % 3, tap % 3)}: conv_out bit-equal to the shifted input", nb == 0,
                           float(nb), 0.0, f"first difference at (item, token, channel) {wb}"))
        dc = got["dc"].double().requires_grad_(False)
        xg = p["x"].double().requires_grad_(True)
        gx, = torch.autograd.grad(conv(xg, p["w"].double(), c), xg, dc)
        gx[:, L] = dc[:, -1]
        bad = got["dX"].double() != gx
        nb = int(bad.sum())
        wb = tuple(int(v) for v in bad.nonzero()[0]) if nb else None
        out.append(Finding(f"tap {tap}: dX bit-equal to the transposed shift of the dc the backward wrote", nb == 0, float(nb), 0.0,
                           f"first difference at (item, token, channel) {wb}"))
        ref, mod = pool_reference(p, c), pool_model(p, c, operand)
        fl = sum_floor(float(mod["dc"].abs().sum() * p["x"].abs().max()), mod["dc"].shape[0] * mod["dc"].shape[1])
        out += [x for x in judge_tensor(None, f"tap {tap}: dw (start + gradient)", got["dw"][None], ref["dw"][None], mod["dw"][None], None, None, fl,
                                        where=lambda flat, S: f"(channel {flat})") if "rowerr" in x.tensor or "zero" in x.tensor]
    return out


# =====================================================================================================================
# max-pool skip
# =====================================================================================================================
MaxCase = collections.namedtuple("MaxCase", "B T H W s C ldi ldo")
MAXPOOL_CASES = [MaxCase(2, 3, 8, 6, 2, 192, 256, 192), MaxCase(3, 1, 7, 5, 2, 96, 96, 128), MaxCase(2, 3, 1, 1, 2, 4, 8, 4),
                 MaxCase(1, 1, 2, 3, 2, 4, 4, 12), MaxCase(2, 1, 8, 8, 4, 192, 196, 256), MaxCase(1, 3, 6, 10, 4, 96, 128, 100),
                 MaxCase(2, 3, 7, 7, 3, 96, 100, 96)]
MAXPOOL_TESTS = [(c, r) for c in MAXPOOL_CASES for r in MAXPOOL_REGIMES]


def maxpool_case_id(c):
    return f"maxpool-B{c.B}-{c.T}x{c.H}x{c.W}-s{c.s}-C{c.C}-ldi{c.ldi}-ldo{c.ldo}"


def maxpool_out(c):
    k = c.s + 1
    pad = k // 2
    return (c.H + 2 * pad - k) // c.s + 1, (c.W + 2 * pad - k) // c.s + 1


def make_maxpool_problem(c, regime):
    """x [B L + B, C] fp32 (patch rows (b, t, h, w), then the cls rows), dy [B Lo + B, C]: multiples of 2^-6, |dy| <= 4"""
    g = _gen("maxpool", tuple(c), regime)
    L = c.T * c.H * c.W
    Ho, Wo = maxpool_out(c)
    x = torch.randn(c.B * L + c.B, c.C, generator=g)
    if regime == "ties":
        x = torch.randint(-1, 2, x.shape, generator=g).float()
    elif regime == "plateau":
        x = torch.full_like(x, 0.75)
    dy = torch.randint(-256, 257, (c.B * c.T * Ho * Wo + c.B, c.C), generator=g).float() / 64.0
    return dict(x=x, dy=dy)


def maxpool_reference(p, c):
    """fp64 mvit_oracle.pool_skip and its autograd -> y, dx in the packed row order, idx = torch max_pool3d's indices [B, C, T, Ho, Wo]"""
    L = c.T * c.H * c.W
    Ho, Wo = maxpool_out(c)
    Lo = c.T * Ho * Wo
    x = p["x"].double()
    xr = torch.cat((x[c.B * L:].reshape(c.B, 1, c.C), x[:c.B * L].reshape(c.B, L, c.C)), 1).requires_grad_(True)
    y = mo.pool_skip(xr, (1, c.s, c.s), (c.T, c.H, c.W))
    dy = p["dy"].double()
    gx, = torch.autograd.grad(y, xr, torch.cat((dy[c.B * Lo:].reshape(c.B, 1, c.C), dy[:c.B * Lo].reshape(c.B, Lo, c.C)), 1))
    k = c.s + 1
    grid = x[:c.B * L].reshape(c.B, c.T, c.H, c.W, c.C).permute(0, 4, 1, 2, 3)
    _, idx = F.max_pool3d(grid, (1, k, k), (1, c.s, c.s), (0, k // 2, k // 2), return_indices=True)
    pk = lambda t: torch.cat((t[:, 1:].reshape(-1, c.C), t[:, 0]), 0)
    return dict(y=pk(y.detach()), dx=pk(gx), idx=idx)


def maxpool_model(p, c, last=False):
    """plain fp32 selection -> y, dx, amax (window-local byte yy * k + xx of the winner).  last = True: the defect `ties go to the LAST
    maximum` that the host test plants."""
    L = c.T * c.H * c.W
    Ho, Wo = maxpool_out(c)
    k, pad = c.s + 1, (c.s + 1) // 2
    x = p["x"][:c.B * L].reshape(c.B * c.T, c.H, c.W, c.C)
    dyp = p["dy"][:c.B * c.T * Ho * Wo].reshape(c.B * c.T, Ho, Wo, c.C)
    y = torch.full((c.B * c.T, Ho, Wo, c.C), float("-inf"))
    am = torch.full((c.B * c.T, Ho, Wo, c.C), -1, dtype=torch.long)
    dx = torch.zeros_like(x)
    for ho in range(Ho):
        for wo in range(Wo):
            for yy in range(k):
                for xx in range(k):
                    yi, xi = ho * c.s - pad + yy, wo * c.s - pad + xx
                    if 0 <= yi < c.H and 0 <= xi < c.W:
                        v = x[:, yi, xi]
                        take = ((v >= y[:, ho, wo]) if last else (v > y[:, ho, wo])) | (am[:, ho, wo] < 0)
                        y[:, ho, wo] = torch.where(take, v, y[:, ho, wo])
                        am[:, ho, wo] = torch.where(take, torch.tensor(yy * k + xx), am[:, ho, wo])
    for ho in range(Ho):
        for wo in range(Wo):
            a = am[:, ho, wo]
            yi, xi = ho * c.s - pad + a // k, wo * c.s - pad + a % k
            n, ch = torch.meshgrid(torch.arange(c.B * c.T), torch.arange(c.C), indexing="ij")
            dx.index_put_((n, yi, xi, ch), dyp[:, ho, wo], accumulate=True)
    return dict(y=torch.cat((y.reshape(-1, c.C), p["x"][c.B * L:])), dx=torch.cat((dx.reshape(-1, c.C), p["dy"][c.B * c.T * Ho * Wo:])),
                amax=am.reshape(-1, c.C))


def gpu_maxpool(c, p, dev):
    """-> dict y, y_am (forward with argmax), amax, dx_scan, dx_am (CPU), guard findings"""
    L_, ptr, stream = _abi()
    L = c.T * c.H * c.W
    Ho, Wo = maxpool_out(c)
    Lo = c.T * Ho * Wo
    f32 = torch.float32
    x = guarded_input(p["x"], f32, dev, c.ldi - c.C)
    dy = guarded_input(p["dy"], f32, dev, c.ldo - c.C)
    b = {n: Guarded(n, [c.B * Lo + c.B], c.C, f32, c.ldo - c.C, device=dev) for n in ("y", "y_am")}
    b.update({n: Guarded(n, [c.B * L + c.B], c.C, f32, c.ldi - c.C, device=dev) for n in ("dx_scan", "dx_am")})
    am = torch.full((c.B * Lo * c.C + 64,), 0xEE, dtype=torch.uint8, device=dev)
    geo = (c.B, c.T, c.H, c.W, c.s, c.C)
    L_.call("pvrl_mvit_maxpool_fwd", ptr(x), c.ldi, *geo, ptr(b["y"].seg(0)), c.ldo, None, stream())
    L_.call("pvrl_mvit_maxpool_fwd", ptr(x), c.ldi, *geo, ptr(b["y_am"].seg(0)), c.ldo, ptr(am), stream())
    L_.call("pvrl_mvit_maxpool_bwd", ptr(x), c.ldi, ptr(dy), c.ldo, *geo, ptr(b["dx_scan"].seg(0)), None, stream())
    L_.call("pvrl_mvit_maxpool_bwd", ptr(x), c.ldi, ptr(dy), c.ldo, *geo, ptr(b["dx_am"].seg(0)), ptr(am), stream())
    torch.cuda.synchronize()
    f = []
    for g in b.values():
        f += g.check()
    tail = bool((am[c.B * Lo * c.C:] == 0xEE).all())
    f.append(Finding("argmax: bytes behind [B T Ho Wo][C] keep their fill", tail, 0.0 if tail else 1.0, 0.0, ""))
    got = {n: g.seg(0).cpu() for n, g in b.items()}
    got["amax"] = am[:c.B * Lo * c.C].cpu().reshape(c.B * Lo, c.C).long()
    return got, f


def judge_maxpool(c, got, ref):
    """everything bit-exact; got: y, y_am, dx_scan, dx_am, amax"""
    Ho, Wo = maxpool_out(c)
    k, pad = c.s + 1, (c.s + 1) // 2
    out = []

    def same(name, a, b):
        bad = a.double() != b.double()
        n = int(bad.sum())
        out.append(Finding(name, n == 0, float(n), 0.0, f"first difference at (row, channel) {tuple(int(v) for v in bad.nonzero()[0]) if n else None}"))
    same("y bit-equal to the reference", got["y"], ref["y"])
    same("y with argmax == y without", got["y_am"], got["y"])
    same("dx (re-scan) bit-equal to the reference", got["dx_scan"], ref["dx"])
    same("dx (saved argmax) bit-equal to the reference", got["dx_am"], ref["dx"])
    same("dx (saved argmax) == dx (re-scan)", got["dx_am"], got["dx_scan"])
    # the saved byte yy * k + xx -> the flat index torch's max_pool3d reports (t * H * W + yi * W + xi within one (clip, channel) volume)
    a = got["amax"].reshape(c.B, c.T, Ho, Wo, c.C).permute(0, 4, 1, 2, 3)
    ho = torch.arange(Ho).reshape(1, 1, 1, Ho, 1)
    wo = torch.arange(Wo).reshape(1, 1, 1, 1, Wo)
    t = torch.arange(c.T).reshape(1, 1, c.T, 1, 1)
    flat = t * c.H * c.W + (ho * c.s - pad + a // k) * c.W + (wo * c.s - pad + a % k)
    same("saved argmax == the first maximum in scan order (torch max_pool3d indices)", flat, ref["idx"])
    return out


def check_maxpool_case(c, regime, run=None):
    p = make_maxpool_problem(c, regime)
    if run is None:
        dev = torch.device("cuda:0")
        run = lambda c, p: gpu_maxpool(c, p, dev)
    got, f = run(c, p)
    return f + judge_maxpool(c, got, maxpool_reference(p, c))


# =====================================================================================================================
# im2col
# =====================================================================================================================
ImCase = collections.namedtuple("ImCase", "B Cin T H W kernel stride padding ldo")
STEM = ((3, 7, 7), (2, 4, 4), (1, 3, 3))


def im2col_kernel(c):
    """`rows_form` of pvrl_im2col3d_bf16 restated -> 'rows' or 'generic(<the first clause that fails>)'"""
    kt, kh, kw = c.kernel
    Wo = (c.W + 2 * c.padding[2] - kw) // c.stride[2] + 1
    clauses = [("W%4", c.W % 4 == 0), ("pitch", c.W + 4 + kw <= 256), ("lines", c.Cin * kt * kh <= 64), ("pw", c.padding[2] <= 4),
               ("kw", kw <= 8), ("reach", (Wo - 1) * c.stride[2] - c.padding[2] + kw - 1 + 4 < 256)]
    bad = [n for n, ok in clauses if not ok]
    return "rows" if not bad else f"generic({bad[0]})"


IM2COL_CASES = [ImCase(2, 3, 5, 12, 24, *STEM, 448), ImCase(1, 3, 3, 8, 240, *STEM, 512), ImCase(1, 3, 4, 8, 244, *STEM, 448),
                ImCase(2, 3, 5, 12, 22, *STEM, 512), ImCase(1, 3, 3, 8, 248, *STEM, 448),
                ImCase(1, 3, 3, 9, 24, (3, 7, 9), (2, 4, 4), (1, 3, 4), 576), ImCase(1, 2, 3, 14, 24, (3, 11, 3), (2, 4, 2), (1, 5, 1), 256),
                ImCase(2, 1, 3, 10, 20, *STEM, 448), ImCase(1, 1, 1, 7, 8, (1, 3, 3), (1, 1, 1), (0, 1, 1), 16)]


def im2col_case_id(c):
    return (f"im2col-B{c.B}xC{c.Cin}-{c.T}x{c.H}x{c.W}-k{'x'.join(map(str, c.kernel))}-s{'x'.join(map(str, c.stride))}-ldo{c.ldo}-"
            f"{im2col_kernel(c)}")


def im2col_expected(frames, c, operand):
    """unfold of the once-rounded input -> [(b, to, ho, wo), K], column ((ch kt + a) kh + y) kw + x"""
    x = _rnd(frames, operand)
    pt, ph, pw = c.padding
    xp = F.pad(x, (pw, pw, ph, ph, pt, pt))
    u = xp.unfold(2, c.kernel[0], c.stride[0]).unfold(3, c.kernel[1], c.stride[1]).unfold(4, c.kernel[2], c.stride[2])
    K = c.Cin * c.kernel[0] * c.kernel[1] * c.kernel[2]
    return u.permute(0, 2, 3, 4, 1, 5, 6, 7).reshape(-1, K)


def gpu_im2col(c, frames, dev):
    L_, ptr, stream = _abi()
    want_rows = im2col_expected(frames, c, BF).shape[0]
    fr = guarded_input(frames.reshape(-1, c.W), torch.float32, dev, 0)
    ob = Guarded("im2col out", [want_rows], c.ldo, BF, device=dev)
    L_.call("pvrl_im2col3d_bf16", ptr(fr), c.B, c.Cin, c.T, c.H, c.W, *c.kernel, *c.stride, *c.padding, ptr(ob.seg(0)), c.ldo, stream())
    torch.cuda.synchronize()
    return ob.seg(0).float().cpu(), ob.check()


def check_im2col_case(c, run=None, operand=None):
    operand = BF if operand is None else operand
    frames = torch.randn(c.B, c.Cin, c.T, c.H, c.W, generator=_gen("im2col", tuple(c)))
    if run is None:
        dev = torch.device("cuda:0")
        run = lambda c, fr: gpu_im2col(c, fr, dev)
    got, f = run(c, frames)
    want = im2col_expected(frames, c, operand)
    K = want.shape[1]
    bad = got[:, :K] != want
    n = int(bad.sum())
    f.append(Finding("columns bit-equal to unfold of the once-rounded input", n == 0, float(n), 0.0,
                     f"first difference at (row, column) {tuple(int(v) for v in bad.nonzero()[0]) if n else None}"))
    z = float(got[:, K:].abs().max()) if c.ldo > K else 0.0
    f.append(Finding("padding columns K .. ldo exactly zero", z == 0.0, z, 0.0, ""))
    return f


# =====================================================================================================================
# LayerNorm of any width (ln_g)
# =====================================================================================================================
LnCase = collections.namedtuple("LnCase", "M C Cpad y16 dy16 res fused kernel")
# y16: the forward writes the 16-bit operand type (else fp32); dy16: 16-bit dy; res: with dres; fused: with the fused dx16 + rowscale16


def ln_names(M, C, Cpad, y16, dy16, res):
    """pvrl_layernorm_g_fwd / _bwd restated: NJ from Cpad, RPI per NJ; live<r>: the highest in-flight row index r of an iteration that
    holds a real row in the backward (blocks = min(ceil(M / 4), 1024), rows of an iteration are 4 * blocks apart)"""
    nj = -(-Cpad // 64)
    NJ = 2 if nj <= 2 else 4 if nj <= 4 else 6 if nj <= 6 else 12
    rf = {2: 4, 4: 4, 6: 2, 12: 1}[NJ]
    rb = {2: 4, 4: 2, 6: 2, 12: 1}[NJ]
    blocks = min(-(-M // 4), 1024)
    live = min(rb - 1, (M - 1) // (4 * blocks))
    return [f"ln_fwd<{'op' if y16 else 'f32'},{NJ},{rf}>", f"ln_bwd<{'op' if dy16 else 'f32'},{NJ},{rb},{'res' if res else 'nores'}>.live{live}"]


def _ln(M, C, Cpad, y16=False, dy16=False, res=True, fused=False):
    return LnCase(M, C, Cpad, y16, dy16, res, fused, "+".join(ln_names(M, C, Cpad, y16, dy16, res)))


def _build_ln_cases():
    c = []
    widths = [(96, 128), (192, 256), (384, 384), (768, 768), (1, 64), (65, 128), (700, 768)]
    ms = [1, 3, 9, 300]
    for i, (C, Cpad) in enumerate(widths):
        for j in range(2):
            k = 2 * i + j
            c.append(_ln(ms[k % 4], C, Cpad, y16=k % 2 == 1, dy16=k % 3 == 1, res=k % 4 != 3, fused=k % 3 == 0))
    # the backward's in-flight rows: r = 1 on three waves only; r = 2 and r = 3 of RPI = 4; RPI = 2
    c += [_ln(4099, 96, 128), _ln(8197, 96, 128, dy16=True, res=False), _ln(12291, 96, 128, y16=True, fused=True),
          _ln(4101, 192, 256, fused=True), _ln(4101, 384, 384, dy16=True)]
    return c


LN_CASES = _build_ln_cases()


def ln_case_id(c):
    return f"ln_g-M{c.M}-C{c.C}-Cpad{c.Cpad}{'-fused16' if c.fused else ''}-{c.kernel}"


def _build_ln_tests():
    tests, seen = [], set()
    for c in LN_CASES:
        regs = ["randn"]
        new = [k for k in c.kernel.split("+") if k not in seen]
        if new and c.M <= 4200:
            seen.update(new)
            regs += [r for r in LN_REGIMES if r != "randn"]
        tests += [(c, r) for r in regs]
    return tests


LN_TESTS = _build_ln_tests()


def ln_draws(c):
    return 1 if c.M >= MIN_ROWS else -(-MIN_ROWS // c.M)


def make_ln_problem(c, regime, operand=None, draw=0):
    operand = BF if operand is None else operand
    g = _gen("ln", c.M, c.C, c.Cpad, regime, draw)
    M, C = c.M, c.C
    x = torch.randn(M, C, generator=g)
    if regime == "offset":
        x = 100.0 + 0.01 * x
    elif regime == "constant":
        const = torch.rand(M, generator=g) < 0.5
        const[0] = True
        x = torch.where(const[:, None], x[:, :1].expand_as(x) * 3.0, x)
    elif regime == "hot":
        x = x * 200.0
    elif regime == "one_live":
        live = torch.zeros(M, C)
        live[torch.arange(M), torch.randint(0, C, (M,), generator=g)] = 1.0
        x = x * live
    dy = torch.randn(M, C, generator=g)
    return dict(x=x, gamma=1 + 0.1 * torch.randn(C, generator=g), beta=0.1 * torch.randn(C, generator=g),
                dy=_rnd(dy, operand) if c.dy16 else dy, dres=torch.randn(M, C, generator=g), rowscale=0.5 + torch.rand(M, generator=g),
                dgamma0=torch.randn(C, generator=g), dbeta0=torch.randn(C, generator=g))


def _ln_eval(p, c, dt):
    """layer_norm and its gradients in dtype dt -> y, mean, rstd, dx (+ dres), dgamma, dbeta (start + gradient)"""
    x = p["x"].to(dt).requires_grad_(True)
    gm, bt = p["gamma"].to(dt).requires_grad_(True), p["beta"].to(dt).requires_grad_(True)
    y = F.layer_norm(x, (c.C,), gm, bt, EPS)
    gx, gg, gb = torch.autograd.grad(y, [x, gm, bt], p["dy"].to(dt))
    xd = x.detach()
    mu = xd.mean(-1, keepdim=True)
    rstd = torch.rsqrt((xd - mu).pow(2).mean(-1, keepdim=True) + EPS)
    if c.res:
        gx = gx + p["dres"].to(dt)
    return dict(y=y.detach(), mean=mu, rstd=rstd, dx=gx, dgamma=(p["dgamma0"].to(dt) + gg)[None], dbeta=(p["dbeta0"].to(dt) + gb)[None])


def ln_reference(p, c):
    return _ln_eval(p, c, torch.float64)


def _tree64(t):
    """wave_sum of csrc/common.h restated: lane partials [.., 64] -> [.., 1], halves added pairwise (xor 32, 16, .. 1)"""
    n = 64
    while n > 1:
        n //= 2
        t = t[..., :n] + t[..., n:2 * n]
    return t


def _wave_row_sum(v, layout):
    """the row sum of v [M, C] in the kernels' order: the lane's own channels one after the other, then `_tree64` over the 64 lanes.
    layout "g" (mvit.hip ln_g_*): lane l holds channels l + 64 j; "n4" / "n" (norm.hip, C a multiple of 256): lane l holds channels
    4 l + 256 j + e, added as (v0 + v1) + (v2 + v3) per j ("n4": the forward's mean) or one after the other ("n")"""
    M, C = v.shape
    if layout == "g":
        nj = -(-C // 64)
        t = F.pad(v, (0, nj * 64 - C)).reshape(M, nj, 64)
        acc = torch.zeros(M, 64)
        for j in range(nj):
            acc = acc + t[:, j]
        return _tree64(acc)
    t = v.reshape(M, C // 256, 64, 4)
    acc = torch.zeros(M, 64)
    for j in range(C // 256):
        if layout == "n4":
            acc = acc + ((t[:, j, :, 0] + t[:, j, :, 1]) + (t[:, j, :, 2] + t[:, j, :, 3]))
        else:
            for e in range(4):
                acc = acc + t[:, j, :, e]
    return _tree64(acc)


def ln_model(p, c, operand, defect=None, flip=False, layout="g"):
    """the kernels' arithmetic restated in fp32 (ln_g_fwd_kernel / ln_g_bwd_kernel; layout "n": ln_fwd_rows / ln_bwd_rows of norm.hip):
    two passes, mean = sum * fl(1 / C), variance from the centred values, every row sum in the kernels' ORDER (`_wave_row_sum`: a lane's
    channels, then a six-level tree over the lanes), the backward from THESE mean / rstd; 16-bit outputs rounded once.
    Why not plain torch: (1) torch layer_norm happens to return the exact mean of a constant row; sum * fl(1 / C) does not, and rstd =
    eps^-0.5 amplifies that residue by |x| 2^-24 / sqrt(eps) in y.  (2) In the `offset` regime (mean 100 over a spread of 0.01) the last
    levels of the lane tree add partial sums of ~C * 100 / 2, whose fp32 spacing is what the mean's error is made of; torch's vectorised
    sum keeps 32 short accumulators and is ~8x closer -- measured on MI355X: kernel / torch mean error 7.96, y 8.15 against the factor 8
    of the Y rule, at C = 768 in the bf16 flavour.  Both belong to every implementation that sums a wave's row this way, so they are in
    the model, and plain torch stays the yardstick Y.
    flip: the channels are dealt to the lanes in reverse order (a second implementation for the host test).  defect: `LN_DEFECTS` of the
    host test."""
    fl = (lambda t: t.flip(-1)) if flip else (lambda t: t)
    x, gm, bt, dy = fl(p["x"]), fl(p["gamma"]), fl(p["beta"]), fl(p["dy"])
    invC = torch.tensor(1.0 / c.C)
    rsum = lambda v, first=False: _wave_row_sum(v, "g" if layout == "g" else ("n4" if first else "n"))
    mu = rsum(x, True) * invC
    var = rsum((x - mu).pow(2)) * invC
    rs = torch.rsqrt(var.clamp_min(1e-30)) if defect == "rstd_without_eps" else torch.rsqrt(var + EPS)
    xh = (x - mu) * rs
    g = dy * gm
    dx = fl(rs * (g - rsum(g) * invC - xh * (rsum(g * xh) * invC)))
    if c.res:
        dx = dx + p["dres"]
    dgr = dy * xh
    if defect == "second_inflight_row_missing_from_dgamma":
        blocks = min(-(-c.M // 4), 1024)
        rb = int(c.kernel.split("+")[1].split(",")[2])
        dgr = dgr * ((torch.arange(c.M) // (4 * blocks)) % rb != 1)[:, None]
    m = dict(y=fl(xh * gm + bt), mean=mu, rstd=rs, dx=dx, dgamma=(p["dgamma0"] + fl(dgr.sum(0)))[None], dbeta=(p["dbeta0"] + fl(dy.sum(0)))[None])
    m["y16"] = _rnd(m["y"], operand)
    m["dx16"] = _rnd(m["dx"] * p["rowscale"][:, None], operand)
    return m


def ln_yardstick(p, c):
    """plain fp32 torch layer_norm and its autograd: Y"""
    return _ln_eval(p, c, torch.float32)


LN_DEFECTS = ("second_inflight_row_missing_from_dgamma", "rstd_without_eps")


def judge_ln_tensor(name, x, ref, mod, yard, sixteen=False):
    """the shared row judge: x, ref, mod, yard [rows, W]"""
    rk, i = rowerr(x, ref)
    rm = rowerr(mod, ref)[0]
    ry = 0.0 if sixteen else rowerr(yard, ref)[0]
    bound = max(ROW_FACTOR * rm, REL_Y_FACTOR * ry)
    return [Finding(name + " rowerr", rk <= bound, rk, bound, f"model rowerr {rm:.3e}, fp32 yardstick {ry:.3e}, ratio kernel/model "
                    f"{rk / max(rm, 1e-300):.2f}, worst row {i}")]


def judge_ln(c, got, ref, mod, yard):
    out = []
    if c.y16:
        out += judge_ln_tensor("y (16-bit)", got["y"], ref["y"], mod["y16"], None, sixteen=True)
    else:
        out += judge_ln_tensor("y (fp32)", got["y"], ref["y"], mod["y"], yard["y"])
    for n in ("mean", "rstd", "dx", "dgamma", "dbeta"):
        out += judge_ln_tensor(n + (" (start + gradient)" if n in ("dgamma", "dbeta") else ""), got[n], ref[n], mod[n], yard[n])
    if c.fused:
        out += judge_ln_tensor("dx16 = R16(rowscale dx)", got["dx16"], ref["dx"] * got["rowscale"].double()[:, None], mod["dx16"], None, sixteen=True)
    if c.Cpad > c.C:
        z = max(float(got["ypad"].abs().max()), float(got["dxpad"].abs().max()))
        out.append(Finding("padding columns C .. Cpad of y, dx (and dx16) are zero", z == 0.0, z, 0.0, ""))
    return out


def gpu_ln(c, p, dev):
    L_, ptr, stream = _abi()
    M, C, Cpad = c.M, c.C, c.Cpad
    f32 = torch.float32
    ydt = BF if c.y16 else f32
    padc = lambda t: F.pad(t, (0, Cpad - C))
    x = guarded_input(padc(p["x"]), f32, dev, 8)
    gm, bt = (guarded_input(p[n][None], f32, dev, 0) for n in ("gamma", "beta"))
    b = dict(y=Guarded("y", [M], Cpad, ydt, 8, device=dev), mean=Guarded("mean", [M], 1, f32, device=dev), rstd=Guarded("rstd", [M], 1, f32, device=dev),
             dx=Guarded("dx", [M], Cpad, f32, 4, device=dev), dgamma=Guarded("dgamma", [1], C, f32, device=dev),
             dbeta=Guarded("dbeta", [1], C, f32, device=dev))
    if c.fused:
        b["dx16"] = Guarded("dx16", [M], Cpad, BF, 8, device=dev)
    L_.call("pvrl_layernorm_g_fwd", ptr(x), Cpad + 8, ptr(gm), ptr(bt), EPS, ptr(b["y"].seg(0)), Cpad + 8, int(not c.y16), M, C, Cpad,
            ptr(b["mean"].seg(0)), ptr(b["rstd"].seg(0)), stream())
    dy = guarded_input(padc(p["dy"]), BF if c.dy16 else f32, dev, 8)
    dres = guarded_input(padc(p["dres"]), f32, dev, 4) if c.res else None
    rsc = guarded_input(p["rowscale"][:, None], f32, dev, 0) if c.fused else None
    b["dgamma"].seg(0).copy_(p["dgamma0"][None])
    b["dbeta"].seg(0).copy_(p["dbeta0"][None])
    nbytes = int(L_.call("pvrl_layernorm_g_bwd_workspace_bytes", M, C))
    ws = pc._workspace(nbytes, dev)
    L_.call("pvrl_layernorm_g_bwd", ptr(dy), Cpad + 8, int(not c.dy16), ptr(x), Cpad + 8, ptr(b["mean"].seg(0)), ptr(b["rstd"].seg(0)), ptr(gm),
            ptr(dres), Cpad + 4, ptr(b["dx"].seg(0)), Cpad + 4, ptr(b["dx16"].seg(0)) if c.fused else None, Cpad + 8, ptr(rsc), M, C, Cpad,
            ptr(b["dgamma"].seg(0)), ptr(b["dbeta"].seg(0)), ptr(ws), nbytes, stream())
    torch.cuda.synchronize()
    f = pc._ws_check("layernorm_g_bwd", ws, nbytes)
    for g in b.values():
        f += g.check()
    cpu = lambda t: t.float().cpu()
    got = {n: cpu(b[n].seg(0)) for n in b}
    got["ypad"], got["dxpad"] = got["y"][:, C:], got["dx"][:, C:]
    if c.fused:
        got["dxpad"] = torch.cat((got["dxpad"], got["dx16"][:, C:]), 1)
        got["dx16"] = got["dx16"][:, :C]
    got["y"], got["dx"] = got["y"][:, :C], got["dx"][:, :C]
    return got, f


def check_ln_case(c, regime, run=None, operand=None):
    """small M: `ln_draws` draws, rows of all draws judged together (one dgamma / dbeta row per draw)"""
    operand = BF if operand is None else operand
    if run is None:
        dev = torch.device("cuda:0")
        run = lambda c, p: gpu_ln(c, p, dev)
    findings, G, R, M_, Y = [], [], [], [], []
    for d in range(ln_draws(c)):
        p = make_ln_problem(c, regime, operand, d)
        got, f = run(c, p)
        got["rowscale"] = p["rowscale"]
        findings += [x for x in f if d == 0 or not x.ok]
        G.append(got)
        R.append(ln_reference(p, c))
        M_.append(ln_model(p, c, operand))
        Y.append(ln_yardstick(p, c))
    cat = lambda parts: {k: torch.cat([q[k] for q in parts]) for k in parts[0]}
    return findings + judge_ln(c, cat(G), cat(R), cat(M_), cat(Y))


# =====================================================================================================================
# the split-row LayerNorm of csrc/norm.hip (pvrl_layernorm_fwd / _bwd and their _split forms, C = 512 / 768)
# =====================================================================================================================
NormCase = collections.namedtuple("NormCase", "C rows16 rows32 y16 dy16 in_lo in_hi dxs_rows dxsum kernel")
# rows [0, rows16) live in a 16-bit matrix, the rest in an fp32 one.  in_lo / in_hi: that part of dx_in is there (else it reads as zeros);
# dxs_rows: rows of the emitted 16-bit copy R16(dxs_scale[row] dx_out[row]) (None: no copy); dxsum: column sums of those rows as well


def norm_names(C, rows16, rows32, y16, dy16, in_lo, in_hi):
    """norm.hip restated: ln_bwd_nblk / ln_bwd_nblk_hi; the first nb_lo workgroups walk the 16-bit rows two per wave and iteration
    (LN_BWD_RPW16), the last nb_hi the fp32 rows; `.r2`: the second in-flight row of some wave is live, `.it2`: a second loop iteration"""
    M = rows16 + rows32
    nblk = min((M + 3) // 4 + 1, 512)
    if rows16 <= 0:
        nb_hi = nblk
    elif rows16 >= M:
        nb_hi = 0
    else:
        nb_hi = min((M - rows16 + 3) // 4, max(nblk // 8, 1))
    nb_lo = nblk - nb_hi
    names = [f"nfwd<{C},{'op' if y16 else 'f32'}>" + (".lo" if rows16 else "") + (".lo_odd" if rows16 % 2 else "") + (".hi" if rows32 else "")]
    b = f"nbwd<{C},{'op' if dy16 else 'f32'}>"
    if rows16:
        names.append(b + ".lo_" + ("in" if in_lo else "noin") + (".it2" if rows16 > 8 * nb_lo else ".r2" if rows16 > 4 * nb_lo else ""))
    if rows32:
        names.append(b + ".hi_" + ("in" if in_hi else "noin") + (".it2" if rows32 > 4 * nb_hi else ""))
    return names


def _norm(C, rows16, rows32, y16=True, dy16=False, in_lo=True, in_hi=True, dxs_rows=None, dxsum=False):
    return NormCase(C, rows16, rows32, y16, dy16, in_lo, in_hi, dxs_rows, dxsum, "+".join(norm_names(C, rows16, rows32, y16, dy16, in_lo, in_hi)))


def _build_norm_cases():
    c = []
    splits = [(0, 5), (7, 0), (1, 1), (3, 2), (2045, 3), (5009, 31)]
    for i, C in enumerate((512, 768)):
        for j, (a, b) in enumerate(splits):
            k = i * len(splits) + j
            M = a + b
            dxs_rows = (None, M, max(1, M - 1), max(1, a - 1) if a > 1 else 1)[k % 4]
            c.append(_norm(C, a, b, y16=k % 2 == 0, dy16=k % 3 == 0, in_lo=k % 4 in (0, 1), in_hi=k % 4 in (0, 2), dxs_rows=dxs_rows,
                           dxsum=dxs_rows is not None and k % 2 == 1))
    # the combinations the cyclic assignment leaves out at the large sizes
    c += [_norm(768, 2045, 3, y16=False, dy16=True, in_lo=False, in_hi=False, dxs_rows=2045, dxsum=True),
          _norm(512, 5009, 31, y16=True, dy16=True, in_lo=True, in_hi=False, dxs_rows=5040, dxsum=True)]
    # a second loop iteration over the fp32 rows of a split matrix: 98 workgroups, 12 of them on the 90 fp32 rows
    c.append(_norm(768, 301, 90, dy16=True, in_lo=False, in_hi=True, dxs_rows=350, dxsum=True))
    return c


NORM_CASES = _build_norm_cases()


def norm_case_id(c):
    return (f"norm-C{c.C}-{c.rows16}+{c.rows32}-in{'L' if c.in_lo else ''}{'H' if c.in_hi else ''}-dxs{c.dxs_rows}{'-dxsum' if c.dxsum else ''}-"
            f"{c.kernel}")


def _build_norm_tests():
    tests, seen = [], set()
    for c in NORM_CASES:
        regs = ["randn"]
        new = [k for k in c.kernel.split("+") if k not in seen]
        if new:
            seen.update(new)
            regs += [r for r in LN_REGIMES if r != "randn"]
        tests += [(c, r) for r in regs]
    return tests


NORM_TESTS = _build_norm_tests()


def norm_draws(c):
    M = c.rows16 + c.rows32
    return 1 if M >= MIN_ROWS else -(-MIN_ROWS // M)


def make_norm_problem(c, regime, operand=None, draw=0):
    """x [M, C]: rows [0, rows16) 16-bit-valued; din (the incoming residual gradient, zero where the part is absent) likewise"""
    operand = BF if operand is None else operand
    M = c.rows16 + c.rows32
    lc = LnCase(M, c.C, c.C, c.y16, c.dy16, True, False, "")
    p = make_ln_problem(lc, regime, operand, ("norm", c.rows16, draw))
    lo = torch.arange(M) < c.rows16
    p["x"] = torch.where(lo[:, None], _rnd(p["x"], operand), p["x"])
    din = torch.where(lo[:, None], _rnd(p["dres"], operand), p["dres"])
    p["din"] = din * torch.where(lo, float(c.in_lo), float(c.in_hi))[:, None]
    p["dxsum0"] = torch.randn(c.C, generator=_gen("dxsum0", tuple(c[:3]), regime, draw))
    return p


def _norm_eval(p, c, dt, operand=None, flip=False):
    """dt fp64: the reference; fp32: plain torch (the yardstick).  operand given: the kernels' arithmetic (`ln_model`) with the 16-bit
    rows of dx_out rounded once"""
    M = c.rows16 + c.rows32
    lc = LnCase(M, c.C, c.C, c.y16, c.dy16, False, False, "")
    m = ln_model(p, lc, operand, flip=flip, layout="n") if operand is not None else _ln_eval(p, lc, dt)
    o = m["dx"] + p["din"].to(m["dx"].dtype)
    n = c.dxs_rows or 0
    out = dict(y=m["y16"] if (operand is not None and c.y16) else m["y"], mean=m["mean"], rstd=m["rstd"], dgamma=m["dgamma"], dbeta=m["dbeta"],
               dx_lo=o[:c.rows16], dx_hi=o[c.rows16:], dxs=o[:n] * p["rowscale"][:n, None].to(o.dtype),
               dxsum=(p["dxsum0"].to(o.dtype) + o[:n].sum(0))[None])
    if operand is not None:
        out["dx_lo"], out["dxs"] = _rnd(out["dx_lo"], operand), _rnd(out["dxs"], operand)
    return out


def gpu_norm(c, p, dev):
    """forward, immediate backward and deferred backward + batched reduce through procedurevrl_amd.ops -> (outputs, findings)"""
    from procedurevrl_amd import ops
    M, C, a = c.rows16 + c.rows32, c.C, c.rows16
    f32 = torch.float32
    gi = lambda t, dt, extra: guarded_input(t, dt, dev, extra)
    x_lo, x_hi = (gi(p["x"][:a], BF, 8) if a else None), (gi(p["x"][a:], f32, 4) if c.rows32 else None)
    gm, bt = gi(p["gamma"][None], f32, 0)[0], gi(p["beta"][None], f32, 0)[0]
    split = a > 0
    xs = ops.SplitRows(x_lo, x_hi) if split else x_hi
    yb = Guarded("y", [M], C, BF if c.y16 else f32, 8, device=dev)
    _, mean, rstd = ops.layernorm_fwd(xs, gm, bt, EPS, out=yb.seg(0))
    dy = gi(p["dy"], BF if c.dy16 else f32, 8)
    di_lo = gi(p["din"][:a], BF, 8) if (a and c.in_lo) else None
    di_hi = gi(p["din"][a:], f32, 4) if (c.rows32 and c.in_hi) else None
    if split:
        dx_in = ops.SplitRows(di_lo, di_hi, n_lo=a, n_hi=c.rows32) if (di_lo is not None or di_hi is not None) else None
    else:
        dx_in = di_hi
    rsc = gi(p["rowscale"][:, None], f32, 0)[:, 0] if c.dxs_rows else None
    runs = []
    for tag in ("immediate", "deferred"):
        b = dict(dgamma=Guarded(f"dgamma ({tag})", [1], C, f32, device=dev), dbeta=Guarded(f"dbeta ({tag})", [1], C, f32, device=dev))
        if a:
            b["dx_lo"] = Guarded(f"dx_out, 16-bit rows ({tag})", [a], C, BF, 8, device=dev)
        if c.rows32:
            b["dx_hi"] = Guarded(f"dx_out, fp32 rows ({tag})", [c.rows32], C, f32, 4, device=dev)
        if c.dxs_rows:
            b["dxs"] = Guarded(f"dxs ({tag})", [c.dxs_rows], C, BF, 8, device=dev)
        if c.dxsum:
            b["dxsum"] = Guarded(f"dxsum ({tag})", [1], C, f32, device=dev)
            b["dxsum"].seg(0).copy_(p["dxsum0"][None])
        b["dgamma"].seg(0).copy_(p["dgamma0"][None])
        b["dbeta"].seg(0).copy_(p["dbeta0"][None])
        if split:
            dx_out = ops.SplitRows(b["dx_lo"].seg(0) if a else None, b["dx_hi"].seg(0) if c.rows32 else None, n_lo=a, n_hi=c.rows32)
        else:
            dx_out = b["dx_hi"].seg(0)
        items = [] if tag == "deferred" else None
        ops.layernorm_bwd(dy, xs, mean, rstd, gm, b["dgamma"].seg(0)[0], b["dbeta"].seg(0)[0], dx_in=dx_in, dx_out=dx_out, beta_acc=1.0,
                          dxs=b["dxs"].seg(0) if c.dxs_rows else None, dxs_scale=rsc, dxsum=b["dxsum"].seg(0)[0] if c.dxsum else None, defer=items)
        if items is not None:
            ops.layernorm_bwd_reduce_batched(items)
        runs.append(b)
    torch.cuda.synchronize()
    f = yb.check()
    for b in runs:
        for g in b.values():
            f += g.check()
    cpu = lambda t: t.float().cpu()
    got = {n: cpu(g.seg(0)) for n, g in runs[0].items()}
    for n in ("dx_lo", "dx_hi", "dxs"):
        got.setdefault(n, torch.zeros(0, C))
    got.setdefault("dxsum", None)
    got.update(y=cpu(yb.seg(0)), mean=cpu(mean)[:, None], rstd=cpu(rstd)[:, None])
    for n, g in runs[1].items():
        same = torch.equal(g.seg(0), runs[0][n].seg(0))
        f.append(Finding(f"{n}: deferred reduce bit-equal to the immediate one", same, 0.0 if same else 1.0, 0.0, ""))
    return got, f


def judge_norm(c, got, ref, mod, yard):
    out = judge_ln_tensor("y (16-bit)" if c.y16 else "y (fp32)", got["y"], ref["y"], mod["y"], None if c.y16 else yard["y"], sixteen=c.y16)
    for n in ("mean", "rstd", "dgamma", "dbeta"):
        out += judge_ln_tensor(n + (" (start + gradient)" if n[0] == "d" else ""), got[n], ref[n], mod[n], yard[n])
    if c.rows16:
        out += judge_ln_tensor("dx_out, 16-bit rows", got["dx_lo"], ref["dx_lo"], mod["dx_lo"], None, sixteen=True)
    if c.rows32:
        out += judge_ln_tensor("dx_out, fp32 rows", got["dx_hi"], ref["dx_hi"], mod["dx_hi"], yard["dx_hi"])
    if c.dxs_rows:
        out += judge_ln_tensor("dxs = R16(scale dx_out)", got["dxs"], ref["dxs"], mod["dxs"], None, sixteen=True)
    if c.dxsum:
        out += judge_ln_tensor("dxsum (start + column sums)", got["dxsum"], ref["dxsum"], mod["dxsum"], yard["dxsum"])
    return out


def check_norm_case(c, regime, run=None, operand=None):
    operand = BF if operand is None else operand
    if run is None:
        dev = torch.device("cuda:0")
        run = lambda c, p: gpu_norm(c, p, dev)
    findings, G, R, M_, Y = [], [], [], [], []
    for d in range(norm_draws(c)):
        p = make_norm_problem(c, regime, operand, d)
        got, f = run(c, p)
        findings += [x for x in f if d == 0 or not x.ok]
        G.append(got)
        R.append(_norm_eval(p, c, torch.float64))
        M_.append(_norm_eval(p, c, torch.float32, operand))
        Y.append(_norm_eval(p, c, torch.float32))
    cat = lambda parts: {k: (torch.cat([q[k] for q in parts]) if parts[0][k] is not None else None) for k in parts[0]}
    return findings + judge_norm(c, cat(G), cat(R), cat(M_), cat(Y))


# =====================================================================================================================
# refusals: PVRL_EINVAL and the guarded outputs untouched
# =====================================================================================================================
def check_refusals():
    from procedurevrl_amd._lib import PvrlError
    L_, ptr, stream = _abi()
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

    def pool(what, B=1, H=1, thw=(2, 4, 4), stride=(1, 2, 2), ld=3 * D, col0=D, short=0, null_conv=False, fwd=True, bwd=True):
        # buffers sized for the nearest valid geometry, so that even a call that was wrongly accepted stays inside them
        vthw = tuple(max(1, abs(v)) for v in thw)
        rows = max(1, B) * vthw[0] * vthw[1] * vthw[2] + max(1, B)
        z = lambda *s, dt=BF: torch.zeros(*s, device=dev, dtype=dt)
        wide = 3 * max(1, H) * D + 136
        qkv, dqkv = z(rows + 4, wide), z(rows + 4, wide)
        ntok = max(1, B) * max(1, H) * (vthw[0] * vthw[1] * vthw[2] + 1)
        y, cv, dc, dy = z(ntok, D), z(ntok, D), z(ntok, D), z(ntok, D)
        f32 = torch.float32
        w, gm, bt = z(D, 27, dt=f32), z(D, dt=f32), z(D, dt=f32)
        dw, dg, db = z(D, 27, dt=f32), z(D, dt=f32), z(D, dt=f32)
        nbytes = int(L_.call("pvrl_mvit_pool_bwd_workspace_bytes"))
        ws = torch.zeros(nbytes, device=dev, dtype=torch.uint8)
        if fwd:
            attempt(f"pvrl_mvit_pool_fwd {what}", lambda: L_.call(
                "pvrl_mvit_pool_fwd", ptr(qkv), ld, col0, B, H, *thw, *stride, ptr(w), ptr(gm), ptr(bt), EPS, ptr(y),
                None if null_conv else ptr(cv), stream()), [y, cv])
        if bwd:
            attempt(f"pvrl_mvit_pool_bwd {what}", lambda: L_.call(
                "pvrl_mvit_pool_bwd", ptr(dy), None if null_conv else ptr(cv), ptr(qkv), ptr(dqkv), ld, col0, B, H, *thw, *stride, ptr(w),
                ptr(gm), EPS, ptr(dc), ptr(dw), ptr(dg), ptr(db), ptr(ws), nbytes - short, stream()), [dqkv, dc, dw, dg, db])

    pool("ld % 4 != 0", ld=3 * D + 2)
    pool("col0 % 4 != 0", col0=D + 2, ld=3 * D + 8)
    pool("stride 0", stride=(1, 0, 2))
    pool("negative stride", stride=(-1, 2, 2))
    pool("T = 0", thw=(0, 4, 4))
    pool("Ww = -3", thw=(2, 4, -3))
    pool("H = 0", H=0)
    pool("workspace one byte short", short=1, fwd=False)
    pool("conv_out = NULL", null_conv=True)

    def maxpool(what, s=2, C=8, ldi=8, ldo=8, with_argmax=False):
        B, T, H, W = 1, 1, 4, 4
        f32 = torch.float32
        z = lambda *sh, dt=f32: torch.zeros(*sh, device=dev, dtype=dt)
        x, y, dy, dx = z(B * T * H * W + B, 16), z(B * T * H * W + B, 16), z(B * T * H * W + B, 16), z(B * T * H * W + B, 16)
        am = z(B * T * H * W * 16, dt=torch.uint8) if with_argmax else None
        attempt(f"pvrl_mvit_maxpool_fwd {what}", lambda: L_.call("pvrl_mvit_maxpool_fwd", ptr(x), ldi, B, T, H, W, s, C, ptr(y), ldo, ptr(am),
                                                                 stream()), [y] + ([am] if with_argmax else []))
        attempt(f"pvrl_mvit_maxpool_bwd {what}", lambda: L_.call("pvrl_mvit_maxpool_bwd", ptr(x), ldi, ptr(dy), ldo, B, T, H, W, s, C, ptr(dx),
                                                                 ptr(am), stream()), [dx])

    maxpool("s = 1", s=1)
    maxpool("C % 4 != 0", C=6)
    maxpool("ldi < C", C=12, ldi=8, ldo=12)
    maxpool("ldo < C", C=12, ldi=12, ldo=8)
    maxpool("s = 15 with a saved argmax (the byte holds yy * k + xx, k <= 15)", s=15, with_argmax=True)
    return out
