"""Row kernels -- LayerNorm (csrc/norm.hip), the loss head (csrc/loss.hip) and the row helpers of csrc/elementwise.hip -- against an fp64
reference, PER ROW, on hard inputs, at the sizes where each kernel takes another path, inside guard bands.

Used by tests/test_row_kernels_gpu.py (pytest -m gpu: the HIP kernels through procedurevrl_amd.ops / the C ABI) and by
tests/test_row_kernels_harness_host.py (no GPU: the CPU models stand in for the kernels, planted defects show that the rule bites).

Metric, rule and guard bands are those of tests/attn_checks.py (`rowerr`, `agg`, `judge_tensor`, `Guarded`, `guarded_input`, ROW_FACTOR):
a tensor passes when rowerr(kernel) <= ROW_FACTOR * rowerr(model) against the fp64 reference on the same, already rounded inputs.  The
model is a CPU fp32 restatement of the kernel's contract that rounds where the kernel rounds (16-bit parts read as stored, outputs rounded
once).  In the `randn` regime the aggregate keeps the flat bounds of tests/kernel_checks.py (TOL_F32, TOL_BF16, 1e-4 for dgamma / dbeta /
dxsum); elsewhere it follows the model.  A vector output (mean, rstd, inv_norm, row_loss, dgamma, dbeta, dxsum) is judged element by
element relative to the rms of the reference vector; a row loss that is a sum of cancelling terms (KL, soft CE, MIL-NCE, MSE) is
normalised by the fp64 sum of the absolute terms.  Cases with fewer than MIN_ROWS rows run on several seeded draws (attn_checks.n_draws).

Two models per fp32 tensor.  `kernel`: the kernel's own order of summation (LayerNorm: a lane's 4 l + 256 j elements, then the xor
butterfly over 64 lanes; backward column sums: per (workgroup, wave) in the grid-stride order of `ln_bwd_assign`; loss kernels: 256
strided partial sums, a butterfly per wave, then the four waves).  `torch`: plain fp32 torch (F.layer_norm, softmax, sum).  For
softmax_rows and the GELU derivative, which use __expf, the second model is exp2(x * log2 e) in fp32.  The yardstick is the `kernel`
model; tests/test_row_kernels_harness_host.py measures the spread of the two on every case it runs and asserts <= ROW_FACTOR / 2, and
a tensor named in WIDE takes the larger of the two models' errors instead.

Bit-exact contracts (one correctly rounded expression; no tolerance): cast_scale, group_bcast, embed_table, cast_weight_pad, the 16-bit
copy of cast_weight, deferred against immediate reduction, soft_ce with a given against a synthesised target, and kl_topk staged
against unstaged on the same row.

Measured on the CPU (pytest tests/test_row_kernels_harness_host.py -s prints these; both operand types, every regime):
  spread of the two models, worst case (larger rowerr / smaller rowerr):
    layernorm_fwd   y 5148 (`const`: the kernel-order sum of a constant row is exact where torch's is not, and rstd = eps^-1/2 amplifies the
                    residue; <= 1.83 elsewhere), mean 219 (`const`; <= 1.82 elsewhere), rstd 7.0 (`const`; 2.34 in `outlier`)
    layernorm_bwd   dx_hi 1.10, dbeta 1.82, dxsum 1.59, dgamma 4.42 (`outlier`: one column of xhat near sqrt(C))
    kl_topk         row_loss 2.17 (K = 6), target 1.63, dpred 1.49;   soft_ce row_loss 1.40, dx 1.99
    l2norm 1.26, softmax_rows 1.00, mse 1.42, gelu_f32 1.00, milnce 1.15, group_reduce 1.00, gemv_rows 2.49 (R = 1, C = 65),
    batch_sum: 16-bit addends sum exactly in one order and not in the other (one model's error is zero)
    -> WIDE = the tensors above ROW_FACTOR / 2: their yardstick is the larger of the two models' errors.
  planted defects, finding that caught each, value / bound (fp16 | bf16 operand type):
    one-pass variance, `offset`: rstd 3.3e3 | 3.3e3          eps dropped, `tiny`: y 7.9e5; `const`: rstd inf (not finite)
    eps 1e-5 for 1e-6, `tiny`: y 1.1e6; `const`: rstd 9.3e5   odd last 16-bit row takes its neighbour's statistics: y 70.8 | 9.3, mean 1.1e6
    second row slot missing from dgamma (2045 + 3): dgamma 5.7e4 | 5.9e4      dx_in not added on the fp32 part: dx_hi 5.8e6, names row 13
    dxs scaled by the next row's factor: dxs 675 | 91         dxsum over all rows (dxs_rows = 8 of 14): dxsum 2.9e6
    one row of a 16-bit y off by 1 %: 10.9 | 1.5
    kl_topk: tied top value counted once: target 3.5e5; boundary tie drops the (k+1)-th entry: 4.1e5; ceil(topk / 2) candidates per thread: 6.7e5
    soft_ce with S = 1 for a target that does not sum to 1: dx 1.2e6
"""
import collections
import zlib

import torch
import torch.nn.functional as F

from attn_checks import rowerr, agg, judge_tensor, Finding, report, ROW_FACTOR, Guarded, guarded_input, MIN_ROWS  # noqa: F401
from procedurevrl_amd._lib import OPERAND

BF = torch.bfloat16 if OPERAND == "bf16" else torch.float16
TOL_BF16 = 1e-2 if OPERAND == "bf16" else 1.5e-3          # kernel_checks.TOL_BF16
TOL_F32 = 2e-5                                             # kernel_checks.TOL_F32
TOL_COLSUM = 1e-4                                          # kernel_checks: dgamma / dbeta / column sums
F32 = torch.float32
LOG2E = 1.4426950408889634

# "<entry> <tensor>" whose yardstick is the larger of the two models' errors (spread above ROW_FACTOR / 2 on the CPU, or one model exact)
WIDE = {"layernorm_fwd y", "layernorm_fwd mean", "layernorm_fwd rstd", "layernorm_bwd dgamma", "gemv_rows y", "batch_sum G", "kl_topk row_loss"}


def _r16(x, dt):
    return x.to(dt).float()


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) % (1 << 31))


def tol16(dt):
    return 1e-2 if dt == torch.bfloat16 else 1.5e-3


def n_draws(rows):
    """attn_checks.n_draws for a tensor of `rows` rows"""
    return 1 if rows >= MIN_ROWS else min(256, -(-MIN_ROWS // rows))


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' orders of summation
# ---------------------------------------------------------------------------------------------------------------------
def tree64(t):
    """wave_sum of csrc/common.h: lane partials [.., 64] -> [..]; xor 32, 16, .. 1"""
    n = 64
    while n > 1:
        n //= 2
        t = t[..., :n] + t[..., n:2 * n]
    return t[..., 0]


def wave_row_sum(v, pairs=False):
    """norm.hip: lane l holds elements 4 l + 256 j + e of a row [M, C]; summed per lane one after the other (pairs: (v0 + v1) + (v2 + v3)
    per j, the forward's mean), then `tree64`"""
    M, C = v.shape
    t = v.reshape(M, C // 256, 64, 4)
    acc = torch.zeros(M, 64, dtype=v.dtype)
    for j in range(C // 256):
        if pairs:
            acc = acc + ((t[:, j, :, 0] + t[:, j, :, 1]) + (t[:, j, :, 2] + t[:, j, :, 3]))
        else:
            for e in range(4):
                acc = acc + t[:, j, :, e]
    return tree64(acc)


def block_sum(v):
    """loss.hip block_reduce: thread t sums elements t, t + 256, ..; butterfly per wave; red[0] + red[1] + red[2] + red[3].  [rows, K] -> [rows]"""
    rows, K = v.shape
    nk = -(-K // 256)
    t = F.pad(v, (0, nk * 256 - K)).reshape(rows, nk, 256)
    acc = torch.zeros(rows, 256, dtype=v.dtype)
    for j in range(nk):
        acc = acc + t[:, j]
    w = tree64(acc.reshape(rows, 4, 64))
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


# ---------------------------------------------------------------------------------------------------------------------
# verdicts
# ---------------------------------------------------------------------------------------------------------------------
def _2d(t):
    return None if t is None else (t.double().reshape(-1, 1) if t.dim() < 2 else t.double().reshape(-1, t.shape[-1]))


def judge(name, x, ref, mod, mod2=None, agg_bound=None, norm=None, where=None, key=None):
    """the rule of attn_checks.judge_tensor for one tensor [rows, W] or a vector [n] (a "row" = one element).  mod2: the second model,
    used only for a tensor whose `key` ("<entry> <tensor>") is in WIDE.  norm [rows]: divide every row by it first (sums of cancelling terms)."""
    x, ref, mod, mod2 = _2d(x), _2d(ref), _2d(mod), _2d(mod2)
    if norm is not None:
        nv = norm.double().reshape(-1, 1).clamp_min(1e-300)
        x, ref, mod, mod2 = x / nv, ref / nv, mod / nv, (None if mod2 is None else mod2 / nv)
    if mod2 is not None and key in WIDE and rowerr(mod2, ref)[0] > rowerr(mod, ref)[0]:
        mod = mod2
    loc = where if where is not None else (lambda flat, S: f"row {flat}")
    return judge_tensor(None, name, x[None], ref[None], mod[None], None, agg_bound, where=loc)


def bits_equal(name, a, b, detail=""):
    """-> [Finding]: a and b hold the same bits (same dtype)"""
    idt = {2: torch.int16, 4: torch.int32}[a.element_size()]
    a, b = a.contiguous().cpu().view(idt), b.contiguous().cpu().view(idt)
    nd = int((a != b).sum()) if a.shape == b.shape else a.numel() + 1
    first = tuple(int(v) for v in (a != b).nonzero()[0]) if 0 < nd <= a.numel() else None
    return [Finding(name + ": elements whose bits differ", nd == 0, float(nd), 0.0, f"first at {first} {detail}")]


def r16_once(v, dt):
    """fp64 -> the 16-bit type in ONE rounding to nearest even (subnormals included), as a 16-bit tensor.  (fp64 -> fp32 -> 16 bits rounds
    twice; v_fma_mix*_f16 of gfx950 rounds the exact fp32 product once.)"""
    mant, emin = (10, -14) if dt == torch.float16 else (7, -126)
    v = v.double()
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** emin)))
    q = torch.exp2(e - mant)
    return (torch.round(v / q) * q).to(dt)          # torch.round: half to even; the result is representable, so .to() is exact


def bits_among(name, got, candidates):
    """-> [Finding]: every element of `got` holds the bits of one of the candidate tensors (each a legitimate rounding of the contract)"""
    idt = {2: torch.int16, 4: torch.int32}[got.element_size()]
    g = got.contiguous().cpu().view(idt)
    ok = torch.zeros_like(g, dtype=torch.bool)
    for cnd in candidates:
        ok |= g == cnd.contiguous().cpu().view(idt)
    nd = int((~ok).sum())
    first = tuple(int(v) for v in (~ok).nonzero()[0]) if nd else None
    return [Finding(name + ": elements whose bits differ", nd == 0, float(nd), 0.0, f"first at {first}")]


def untouched(g):
    """-> [Finding]: nothing at all was written into the Guarded buffer g"""
    nd = int((g.buf.view(g.idt).cpu() != g.before).sum())
    return [Finding(f"{g.name}: elements written although the call was refused", nd == 0, float(nd), 0.0, "")]


def spread(mod, mod2, ref, norm=None):
    """larger / smaller of the two models' rowerr (inf when only one is exact)"""
    a, b, r = _2d(mod), _2d(mod2), _2d(ref)
    if norm is not None:
        nv = norm.double().reshape(-1, 1).clamp_min(1e-300)
        a, b, r = a / nv, b / nv, r / nv
    ea, eb = rowerr(a, r)[0], rowerr(b, r)[0]
    if max(ea, eb) == 0.0:
        return 1.0, ea, eb
    return max(ea, eb) / max(min(ea, eb), 1e-300), ea, eb


# =====================================================================================================================
# LayerNorm (csrc/norm.hip)
# =====================================================================================================================
LN_FWD_RPW16, LN_BWD_RPW16, LN_BWD_MAX_BLOCKS, LN_RED_MAX = 2, 2, 512, 40
LN_REGIMES = ("randn", "offset", "tiny", "tiny_eps5", "outlier", "const")
DY_REGIMES = ("randn", "scaled")


def ln_fwd_grid(M, rows16):
    """pvrl_layernorm_fwd_split: (workgroups on the 16-bit rows, 4 waves x 2 rows; workgroups on the fp32 rows, one row per wave)"""
    return -(-rows16 // (4 * LN_FWD_RPW16)), -(-(M - rows16) // 4)


def ln_bwd_nblk(M):
    return min((M + 3) // 4 + 1, LN_BWD_MAX_BLOCKS)


def ln_bwd_nblk_hi(M, rows16):
    if rows16 <= 0:
        return ln_bwd_nblk(M)
    if rows16 >= M:
        return 0
    nblk = ln_bwd_nblk(M)
    return min((M - rows16 + 3) // 4, max(nblk // 8, 1))


def ln_bwd_assign(M, rows16):
    """row -> (workgroup, wave, slot, iteration) of ln_bwd_kernel, four long tensors [M].  The first nb_lo workgroups walk the 16-bit
    rows two per wave and iteration (slot 0: row, slot 1: row + 4 nb_lo), the last nb_hi the fp32 rows one per wave and iteration"""
    nblk, nb_hi = ln_bwd_nblk(M), ln_bwd_nblk_hi(M, rows16)
    nb_lo = nblk - nb_hi
    row = torch.arange(M)
    lo = row < rows16
    s_lo, s_hi = max(4 * nb_lo, 1), max(4 * nb_hi, 1)
    r_hi = (row - rows16).clamp_min(0)
    k_lo, k_hi = row // s_lo, r_hi // s_hi
    blk = torch.where(lo, (row % s_lo) // 4, nb_lo + (r_hi % s_hi) // 4)
    wave = torch.where(lo, row % 4, r_hi % 4)
    slot = torch.where(lo, k_lo % LN_BWD_RPW16, torch.zeros_like(row))
    it = torch.where(lo, k_lo // LN_BWD_RPW16, k_hi)
    return blk, wave, slot, it


def ln_bwd_path(M, rows16):
    """text: workgroup counts and where the last row of each part fell"""
    nblk, nb_hi = ln_bwd_nblk(M), ln_bwd_nblk_hi(M, rows16)
    blk, wave, slot, it = ln_bwd_assign(M, rows16)
    s = f"{nblk} workgroups ({nblk - nb_hi} on 16-bit rows, {nb_hi} on fp32 rows)"
    if rows16 > 0:
        r = rows16 - 1
        s += f"; last 16-bit row {r}: workgroup {int(blk[r])} wave {int(wave[r])} slot {int(slot[r])} iteration {int(it[r])}"
        s += f", rows in a second slot {int(((slot == 1) & (torch.arange(M) < rows16)).sum())}"
    if rows16 < M:
        s += f"; last fp32 row {M - 1}: workgroup {int(blk[M - 1])} wave {int(wave[M - 1])} iteration {int(it[M - 1])}"
    return s


_LN_FIELDS = "kind C R B split y16 dy16 in_lo in_hi dxs_rows scaled dxsum beta_acc sum_beta ld save_stats stats_arg path"
LnCase = collections.namedtuple("LnCase", _LN_FIELDS)
# kind "fwd" / "bwd".  split: a pvrl_rows matrix with R 16-bit rows and B fp32 rows (B = 0: the fp32 part is absent); not split: R = 0,
# B = M fp32 rows through pvrl_layernorm_fwd / _bwd.  in_lo / in_hi: that part of dx_in is there.  dxs_rows: rows of the emitted 16-bit copy
# (None: none), scaled: with dxs_scale, dxsum: with the column sums; beta_acc / sum_beta: the accumulate factors of dgamma, dbeta / dxsum.
# ld: leading dimensions C + 4 on every matrix.  save_stats / stats_arg (forward, plain): ops.layernorm_fwd(save_stats=, stats=)


def _ln(kind, C, R, B, split=None, y16=False, dy16=True, in_lo=True, in_hi=True, dxs_rows=None, scaled=False, dxsum=False, beta_acc=0.0,
        sum_beta=None, ld=False, save_stats=True, stats_arg=False, path=""):
    split = (R > 0) if split is None else split
    return LnCase(kind, C, R, B, split, y16, dy16, in_lo, in_hi, dxs_rows, scaled, dxsum, beta_acc, beta_acc if sum_beta is None else sum_beta,
                  ld, save_stats, stats_arg, path)


def ln_fwd_path(c):
    nb_lo, nb_hi = ln_fwd_grid(c.R + c.B, c.R)
    p = f"wg{nb_lo}+{nb_hi}"
    if c.R % 2:
        p += ".odd_last_row_alone"
    return p


def ln_eps(c, regime):
    if regime == "tiny":
        return 1e-6
    if regime == "tiny_eps5":
        return 1e-5
    return 1e-5 if c.C == 512 else 1e-6


def ln_case_id(c):
    M = c.R + c.B
    shape = f"{c.R}+{c.B if c.B else 'none'}" if c.split else f"M{M}"
    if c.kind == "fwd":
        s = f"layernorm_fwd{'_split' if c.split else ''}-C{c.C}-{shape}-{'y16' if c.y16 else 'yf32'}"
        s += ("" if c.save_stats else "-nostats") + ("-statsarg" if c.stats_arg else "")
    else:
        s = f"layernorm_bwd{'_split' if c.split else ''}-C{c.C}-{shape}-{'dy16' if c.dy16 else 'dyf32'}-in{'L' if c.in_lo else ''}{'H' if c.in_hi else ''}"
        if c.dxs_rows is not None:
            s += f"-dxs{c.dxs_rows}{'s' if c.scaled else ''}{'-dxsum' if c.dxsum else ''}"
        s += f"-beta{c.beta_acc:g}" + (f"-sumbeta{c.sum_beta:g}" if c.sum_beta != c.beta_acc else "")
    return s + ("-ld+4" if c.ld else "") + "-" + c.path


def _build_ln_fwd_cases():
    cases = []
    for C in (512, 768, 1024):
        for y16 in (False, True):
            for i, M in enumerate((1, 3, 4, 5, 77)):
                cases.append(_ln("fwd", C, 0, M, y16=y16, ld=i % 2 == 1))
            for i, R in enumerate((1, 2, 7, 8, 9, 13)):
                for j, B in enumerate((0, 1, 4, 5)):
                    cases.append(_ln("fwd", C, R, B, split=True, y16=y16, ld=(i + j) % 2 == 1))
    cases.append(_ln("fwd", 768, 13, 5, split=True, y16=True, ld=True))                 # C + 4 on x, x16 and y (named case)
    cases.append(_ln("fwd", 768, 0, 5, save_stats=False))
    cases.append(_ln("fwd", 768, 0, 77, y16=True, stats_arg=True))
    seen, out = set(), []
    for c in cases:
        c = c._replace(path=ln_fwd_path(c))
        if ln_case_id(c) not in seen:
            seen.add(ln_case_id(c))
            out.append(c)
    return out


LN_FWD_CASES = _build_ln_fwd_cases()
# the split backward's boundary cases: R + B -> what it reaches
LN_BWD_SPLIT = [(13, 1, "smallest"), (2044, 3, "no_second_slot"), (2045, 3, "one_wave_second_row"), (4088, 3, "both_slots_full"),
                (4089, 3, "second_iteration"), (8, 300, "fp32_part_loops_9x"), (2000, 300, "capped_nb_hi_partial_second_slot")]
LN_BWD_PLAIN = [(1, "one_row"), (4, "one_wg"), (5, "two_wg"), (77, "ragged"), (2048, "grid_cap_one_pass"), (2049, "grid_cap_second_iteration"),
                (4100, "third_iteration")]


def _build_ln_bwd_cases():
    cases = []
    for i, (M, what) in enumerate(LN_BWD_PLAIN):
        for dy16 in (True, False):
            for has_in in (True, False):
                cases.append(_ln("bwd", 768, 0, M, dy16=dy16, in_hi=has_in, ld=(i + dy16 + has_in) % 2 == 1, path=what))
    for C in (512, 1024):
        for M, what in ((2048, "grid_cap_one_pass"), (2049, "grid_cap_second_iteration")):
            cases.append(_ln("bwd", C, 0, M, dy16=True, ld=C == 512, path=what))
    combos = [(True, True), (False, True), (True, False), (False, False)]
    for i, (R, B, what) in enumerate(LN_BWD_SPLIT):
        for j in range(2):                      # two dx_in combinations per shape, all four over the table; fp32 dy on three shapes
            in_lo, in_hi = combos[(2 * i + j) % 4]
            cases.append(_ln("bwd", 768, R, B, dy16=not (j == 1 and i in (0, 3, 5)), in_lo=in_lo, in_hi=in_hi, ld=(i + j) % 2 == 0, path=what))
    for C in (512, 1024):
        for (R, B, what) in LN_BWD_SPLIT[1:5]:
            cases.append(_ln("bwd", C, R, B, ld=C == 1024, path=what))
    # the emitted copy: dxs_rows in {M, R - 5, 1}, with / without scale, with the column sums, accumulate on / off, and check_layernorm's
    # (beta_acc, dxsum_beta) combinations (0, 0), (1, 1), (0, 1)
    for (R, B) in ((0, 77), (13, 1), (2045, 3)):
        M = R + B
        for k, rows in enumerate((M, max(1, (R if R else M) - 5), 1)):
            cases.append(_ln("bwd", 768, R, B, dxs_rows=rows, scaled=k != 1, dxsum=k != 2, beta_acc=float(k % 2), ld=k == 0, path="dxs"))
        cases.append(_ln("bwd", 768, R, B, dxs_rows=max(1, (R if R else M) - 5), scaled=True, dxsum=True, beta_acc=0.0, sum_beta=1.0, path="dxs"))
        cases.append(_ln("bwd", 768, R, B, dy16=False, dxs_rows=M, scaled=False, dxsum=True, beta_acc=1.0, path="dxs"))
    return cases


LN_BWD_CASES = _build_ln_bwd_cases()


def _build_ln_tests():
    """every case runs `randn`; the first case of each (kind, path family, output type) also runs the other regimes at C = 768, and the
    boundary cases at C = 512 / 1024 run `offset` as well; backward cases add the `scaled` dy regime where the path is new"""
    tests, seen = [], set()
    for c in LN_FWD_CASES:
        tests.append((c, "randn", "randn"))
        key = (c.split, c.R % 2, c.B > 0, c.y16, c.R > 8 or c.B > 4)
        if c.C == 768 and key not in seen and c.save_stats and not c.stats_arg:
            seen.add(key)
            tests += [(c, r, "randn") for r in LN_REGIMES[1:]]
        elif c.C != 768 and (c.R, c.B) in ((13, 5), (0, 77)):
            tests += [(c, "offset", "randn"), (c, "tiny", "randn")]
    seen = set()
    for c in LN_BWD_CASES:
        tests.append((c, "randn", "randn"))
        key = (c.path, c.dxs_rows is None)
        if c.C == 768 and key not in seen:
            seen.add(key)
            tests += [(c, "randn", "scaled"), (c, "offset", "scaled"), (c, "const", "randn")]
            if c.R + c.B <= 100:
                tests += [(c, "tiny", "randn"), (c, "outlier", "randn")]
    return tests


LN_TESTS = _build_ln_tests()


def ln_test_id(t):
    c, regime, dyr = t
    return f"{ln_case_id(c)}-{regime}" + ("-dy_scaled" if dyr == "scaled" else "")


def make_ln_problem(c, regime, dy_regime="randn", operand=None, draw=0):
    """CPU fp32 tensors, already rounded where the kernel reads 16 bits.  The backward's mean / rstd inputs are the `kernel` model's"""
    operand = BF if operand is None else operand
    M, C, R = c.R + c.B, c.C, c.R
    g = _gen("ln", c.kind, C, R, c.B, regime, dy_regime, draw)
    x = torch.randn(M, C, generator=g)
    if regime == "randn":
        x = x * 2 + 0.3
    elif regime == "offset":
        x = x + 100.0
    elif regime in ("tiny", "tiny_eps5"):
        x = x * 1e-3
    elif regime == "outlier":
        x[:, int(torch.randint(0, C, (1,), generator=g))] = 300.0
    elif regime == "const":
        x[::7] = (x[::7, :1] * 3.0).expand(-1, C)
    lo = (torch.arange(M) < R)[:, None]
    x = torch.where(lo, _r16(x, operand), x)
    p = dict(x=x, gamma=torch.randn(C, generator=g), beta=torch.randn(C, generator=g), eps=ln_eps(c, regime), operand=operand)
    if c.kind == "fwd":
        return p
    dy = torch.randn(M, C, generator=g)
    if dy_regime == "scaled":
        dy = dy * torch.pow(10.0, torch.rand(M, 1, generator=g) * 6 - 3)
    p["dy"] = _r16(dy, operand) if c.dy16 else dy
    din = torch.randn(M, C, generator=g)
    din = torch.where(lo, _r16(din, operand), din)
    p["din"] = din * torch.where(lo, float(c.in_lo), float(c.in_hi))
    p["scale"] = torch.rand(M, generator=g) + 0.5
    p["dgamma0"], p["dbeta0"], p["dxsum0"] = (torch.randn(C, generator=g) for _ in range(3))
    st = ln_fwd_eval(p, c, "kernel")
    p["mean"], p["rstd"] = st["mean"], st["rstd"]
    return p


LN_FWD_DEFECTS = ("one_pass_variance", "eps_dropped", "eps_1e-5_for_1e-6", "odd_last_row_takes_neighbours_stats")
LN_BWD_DEFECTS = ("second_slot_missing_from_dgamma", "dx_in_not_added_on_fp32_part", "dxs_scaled_by_next_rows_factor", "dxsum_over_all_rows")


def ln_fwd_eval(p, c, mode, defect=None):
    """mode "ref" (fp64), "kernel" (ln_fwd_rows restated in fp32), "torch" (F.layer_norm) -> y (rounded once if 16-bit and not ref), mean, rstd"""
    C, eps, x = c.C, p["eps"], p["x"]
    if defect == "eps_dropped":
        eps = 0.0
    elif defect == "eps_1e-5_for_1e-6":
        eps = 1e-5
    if mode == "ref":
        xd = x.double()
        mu = xd.mean(1, keepdim=True)
        rs = torch.rsqrt((xd - mu).pow(2).mean(1, keepdim=True) + p["eps"])
        return dict(y=(xd - mu) * rs * p["gamma"].double() + p["beta"].double(), mean=mu[:, 0], rstd=rs[:, 0])
    if mode == "torch":
        mu = x.mean(1, keepdim=True)
        rs = torch.rsqrt(x.var(1, unbiased=False, keepdim=True) + eps)
        y = F.layer_norm(x, (C,), p["gamma"], p["beta"], eps)
    else:
        invC = torch.tensor(1.0 / C)
        mu = (wave_row_sum(x, pairs=True) * invC)[:, None]
        if defect == "one_pass_variance":
            var = (wave_row_sum(x * x) * invC)[:, None] - mu * mu
        else:
            var = (wave_row_sum((x - mu).pow(2)) * invC)[:, None]
        rs = torch.rsqrt(var + eps)
        if defect == "odd_last_row_takes_neighbours_stats" and c.R % 2 and c.R >= 3:
            mu, rs = mu.clone(), rs.clone()
            mu[c.R - 1], rs[c.R - 1] = mu[c.R - 2], rs[c.R - 2]
        y = (x - mu) * rs * p["gamma"] + p["beta"]
    if c.y16:
        y = _r16(y, p["operand"])
    return dict(y=y, mean=mu[:, 0], rstd=rs[:, 0])


def ln_bwd_eval(p, c, mode, defect=None):
    """the backward from the GIVEN fp32 mean / rstd: mode "ref" fp64 arithmetic; "kernel": ln_bwd_rows / ln_bwd_kernel in fp32, row sums in
    lane order, column sums per (workgroup, wave) of `ln_bwd_assign`; "torch": plain fp32 sums.
    -> dx_lo (rounded once), dx_hi, dgamma, dbeta, dxs (rounded once), dxsum"""
    dt = torch.float64 if mode == "ref" else torch.float32
    M, C, R = c.R + c.B, c.C, c.R
    x, dy, gm = p["x"].to(dt), p["dy"].to(dt), p["gamma"].to(dt)
    mu, rs = p["mean"].to(dt)[:, None], p["rstd"].to(dt)[:, None]
    xh = (x - mu) * rs
    gy = dy * gm
    if mode == "kernel":
        invC = torch.tensor(1.0 / C)
        c1, c2 = (wave_row_sum(gy) * invC)[:, None], (wave_row_sum(gy * xh) * invC)[:, None]
    else:
        c1, c2 = gy.mean(1, keepdim=True), (gy * xh).mean(1, keepdim=True)
    din = p["din"].to(dt)
    if defect == "dx_in_not_added_on_fp32_part":
        din = din * (torch.arange(M) < R)[:, None].to(dt)
    o = rs * (gy - c1 - xh * c2) + din
    n = c.dxs_rows or 0
    dg_rows, db_rows, ds_rows = dy * xh, dy, (o if defect == "dxsum_over_all_rows" else o * (torch.arange(M) < n)[:, None].to(dt))
    blk, wave, slot, it = ln_bwd_assign(M, R)
    if defect == "second_slot_missing_from_dgamma":
        dg_rows = dg_rows * (slot != 1)[:, None].to(dt)

    def colsum(v):
        if mode != "kernel":
            return v.sum(0)
        part = torch.zeros(ln_bwd_nblk(M) * 4, C).index_add_(0, blk * 4 + wave, v).reshape(-1, 4, C)
        return (((part[:, 0] + part[:, 1]) + part[:, 2]) + part[:, 3]).sum(0)
    sc = p["scale"].to(dt) if c.scaled else torch.ones(M, dtype=dt)
    if defect == "dxs_scaled_by_next_rows_factor":
        sc = torch.roll(sc, -1)
    out = dict(dx_lo=o[:R], dx_hi=o[R:], dgamma=c.beta_acc * p["dgamma0"].to(dt) + colsum(dg_rows),
               dbeta=c.beta_acc * p["dbeta0"].to(dt) + colsum(db_rows), dxs=o[:n] * sc[:n, None],
               dxsum=c.sum_beta * p["dxsum0"].to(dt) + colsum(ds_rows))
    if mode != "ref":
        out["dx_lo"], out["dxs"] = _r16(out["dx_lo"], p["operand"]), _r16(out["dxs"], p["operand"])
    return out


def _abi():
    from procedurevrl_amd import ops
    from procedurevrl_amd._lib import lib
    return lib(), ops._ptr, ops._stream, ops


def gpu_ln_fwd(c, p, dev):
    L, P, S, ops = _abi()
    M, C, R, e = c.R + c.B, c.C, c.R, (4 if c.ld else 0)
    gi = lambda t, dt: guarded_input(t, dt, dev, e)
    gm, bt = guarded_input(p["gamma"][None], F32, dev, 0)[0], guarded_input(p["beta"][None], F32, dev, 0)[0]
    yb = Guarded("y", [M], C, BF if c.y16 else F32, e, device=dev)
    mb, rb = Guarded("mean", [M], 1, F32, device=dev), Guarded("rstd", [M], 1, F32, device=dev)
    if c.split:
        lo, hi = (gi(p["x"][:R], BF) if R else None), (gi(p["x"][R:], F32) if c.B else None)
        L.call("pvrl_layernorm_fwd_split", *ops._ptr_ld(lo), R, *ops._ptr_ld(hi), P(gm), P(bt), float(p["eps"]), P(yb.seg(0)), C + e,
               int(not c.y16), P(mb.seg(0)), P(rb.seg(0)), M, C, S())
        stats = True
    else:
        x = gi(p["x"], F32)
        stats = c.save_stats
        if c.stats_arg:
            ops.layernorm_fwd(x, gm, bt, p["eps"], out=yb.seg(0), stats=(mb.seg(0), rb.seg(0)))
        elif c.save_stats:      # the wrapper allocates its own statistics: go through the C ABI to keep them inside guard bands
            L.call("pvrl_layernorm_fwd", P(x), C + e, P(gm), P(bt), float(p["eps"]), P(yb.seg(0)), C + e, int(not c.y16), P(mb.seg(0)),
                   P(rb.seg(0)), M, C, S())
        else:
            _, m_, r_ = ops.layernorm_fwd(x, gm, bt, p["eps"], out=yb.seg(0), save_stats=False)
            assert m_ is None and r_ is None
    torch.cuda.synchronize()
    f = yb.check()
    got = dict(y=yb.seg(0).float().cpu(), mean=None, rstd=None)
    if stats:
        f += mb.check() + rb.check()
        got.update(mean=mb.seg(0).cpu()[:, 0], rstd=rb.seg(0).cpu()[:, 0])
    else:
        f += untouched(mb) + untouched(rb)
    return got, f


def gpu_ln_bwd(c, p, dev):
    """immediate backward and deferred backward + batched reduce through procedurevrl_amd.ops -> (outputs of the immediate run, findings)"""
    L, P, S, ops = _abi()
    M, C, R, e = c.R + c.B, c.C, c.R, (4 if c.ld else 0)
    gi = lambda t, dt: guarded_input(t, dt, dev, e)
    vec = lambda t: guarded_input(t[None], F32, dev, 0)[0]
    col = lambda t: guarded_input(t[:, None], F32, dev, 0)[:, 0]
    gm, mean, rstd = vec(p["gamma"]), col(p["mean"]), col(p["rstd"])
    x_lo, x_hi = (gi(p["x"][:R], BF) if R else None), (gi(p["x"][R:], F32) if c.B else None)
    xs = ops.SplitRows(x_lo, x_hi) if c.split else x_hi
    dy = gi(p["dy"], BF if c.dy16 else F32)
    di_lo = gi(p["din"][:R], BF) if (R and c.in_lo) else None
    di_hi = gi(p["din"][R:], F32) if (c.B and c.in_hi) else None
    if c.split:
        dx_in = ops.SplitRows(di_lo, di_hi, n_lo=R, n_hi=c.B) if (di_lo is not None or di_hi is not None) else None
    else:
        dx_in = di_hi
    n = c.dxs_rows
    # the scale vector has exactly dxs_rows entries; INPUT_GUARD values follow
    rsc = col(p["scale"][:n]) if (n and c.scaled) else None
    nbytes = int(L.call("pvrl_layernorm_bwd_workspace_bytes", M, C))
    f = [Finding("workspace bytes == nblk * 3 * C * 4 (the restated grid)", nbytes == ln_bwd_nblk(M) * 3 * C * 4, float(nbytes),
                 float(ln_bwd_nblk(M) * 3 * C * 4), ln_bwd_path(M, R))]
    runs = []
    for tag in ("immediate", "deferred"):
        b = dict(dgamma=Guarded(f"dgamma ({tag})", [1], C, F32, device=dev), dbeta=Guarded(f"dbeta ({tag})", [1], C, F32, device=dev))
        if R:
            b["dx_lo"] = Guarded(f"dx_out, 16-bit rows ({tag})", [R], C, BF, e, device=dev)
        if c.B:
            b["dx_hi"] = Guarded(f"dx_out, fp32 rows ({tag})", [c.B], C, F32, e, device=dev)
        if n:       # M rows, of which rows >= dxs_rows must keep the pattern
            b["dxs"] = Guarded(f"dxs ({tag})", [M], C, BF, e, unowned=[(0, n, M, 0, C)] if n < M else (), device=dev)
        if c.dxsum:
            b["dxsum"] = Guarded(f"dxsum ({tag})", [1], C, F32, device=dev)
            b["dxsum"].seg(0).copy_(p["dxsum0"][None])
        b["dgamma"].seg(0).copy_(p["dgamma0"][None])
        b["dbeta"].seg(0).copy_(p["dbeta0"][None])
        if c.split:
            dx_out = ops.SplitRows(b["dx_lo"].seg(0) if R else None, b["dx_hi"].seg(0) if c.B else None, n_lo=R, n_hi=c.B)
        else:
            dx_out = b["dx_hi"].seg(0)
        items = [] if tag == "deferred" else None
        ops.layernorm_bwd(dy, xs, mean, rstd, gm, b["dgamma"].seg(0)[0], b["dbeta"].seg(0)[0], dx_in=dx_in, dx_out=dx_out, beta_acc=c.beta_acc,
                          dxs=b["dxs"].seg(0)[:n] if n else None, dxs_scale=rsc, dxsum=b["dxsum"].seg(0)[0] if c.dxsum else None,
                          dxsum_beta=c.sum_beta if c.dxsum else None, defer=items)
        if items is not None:
            ops.layernorm_bwd_reduce_batched(items)
        runs.append(b)
    torch.cuda.synchronize()
    for b in runs:
        for g in b.values():
            f += g.check()
    got = {k: g.seg(0).float().cpu() for k, g in runs[0].items()}
    for k in ("dx_lo", "dx_hi"):
        got.setdefault(k, torch.zeros(0, C))
    got["dxs"] = got["dxs"][:n] if n else torch.zeros(0, C)
    for k in ("dgamma", "dbeta", "dxsum"):
        got[k] = got[k][0] if k in got else None
    for k, g in runs[1].items():
        f += bits_equal(f"{k}: deferred + batched reduce against immediate", g.seg(0)[:n] if k == "dxs" else g.seg(0),
                        runs[0][k].seg(0)[:n] if k == "dxs" else runs[0][k].seg(0))
    return got, f


def _cat(parts):
    return {k: (torch.cat([q[k] for q in parts]) if parts[0][k] is not None else None) for k in parts[0]}


def check_ln_case(c, regime, dy_regime="randn", run=None, operand=None, spreads=None):
    """one LayerNorm case x regime -> list of Finding.  run(c, p) -> (outputs, findings): the GPU by default.  spreads (dict): collects the
    spread of the two models per tensor (host test)"""
    operand = BF if operand is None else operand
    if run is None:
        dev = torch.device("cuda:0")
        run = (lambda c, p: gpu_ln_fwd(c, p, dev)) if c.kind == "fwd" else (lambda c, p: gpu_ln_bwd(c, p, dev))
    ev = ln_fwd_eval if c.kind == "fwd" else ln_bwd_eval
    M = c.R + c.B
    findings, G, R_, A, T = [], [], [], [], []
    for d in range(n_draws(M)):
        p = make_ln_problem(c, regime, dy_regime, operand, d)
        got, f = run(c, p)
        findings += [x for x in f if d == 0 or not x.ok]
        G.append(got); R_.append(ev(p, c, "ref")); A.append(ev(p, c, "kernel")); T.append(ev(p, c, "torch"))
    got, ref, mod, mod2 = _cat(G), _cat(R_), _cat(A), _cat(T)
    rn = regime == "randn" and dy_regime == "randn"
    t16 = tol16(operand)
    blk, wave, slot, it = ln_bwd_assign(M, c.R)

    def where(n, off):
        """rows of a tensor with n rows per draw, the first of which is row `off` of the matrix"""
        def w(flat, S):
            d, r = divmod(flat, max(n, 1))
            s = f"row {r + off}" + (f" (draw {d})" if d else "")
            if c.kind == "bwd":
                r += off
                s += f": workgroup {int(blk[r])} wave {int(wave[r])} slot {int(slot[r])} iteration {int(it[r])}"
            return s
        return w
    column = lambda flat, S: f"column {flat % c.C}" + (f" (draw {flat // c.C})" if flat >= c.C else "")
    out = []

    def J(name, key, sixteen=False, tol=None, wh=None):
        if got.get(key) is None or got[key].numel() == 0:
            return
        m2 = None if sixteen else mod2[key]
        if spreads is not None and m2 is not None:
            spreads.setdefault(f"layernorm_{c.kind} {name}", []).append(spread(mod[key], m2, ref[key])[0])
        out.extend(judge(name, got[key], ref[key], mod[key], m2, tol if rn else None, where=wh, key=f"layernorm_{c.kind} {name}"))
    if c.kind == "fwd":
        J("y", "y", sixteen=c.y16, tol=t16 if c.y16 else TOL_F32, wh=where(M, 0))
        J("mean", "mean", tol=TOL_F32, wh=where(M, 0))
        J("rstd", "rstd", tol=TOL_F32, wh=where(M, 0))
    else:
        out.append(Finding("path", True, 0.0, 0.0, ln_bwd_path(M, c.R)))
        J("dx_lo", "dx_lo", sixteen=True, tol=t16, wh=where(c.R, 0))
        J("dx_hi", "dx_hi", tol=TOL_F32, wh=where(c.B, c.R))
        J("dgamma", "dgamma", tol=TOL_COLSUM, wh=column)
        J("dbeta", "dbeta", tol=TOL_COLSUM, wh=column)
        J("dxs", "dxs", sixteen=True, tol=t16, wh=where(c.dxs_rows or 0, 0))
        J("dxsum", "dxsum", tol=TOL_COLSUM, wh=column)
    return findings + out


def check_ln_reduce_batched():
    """73 deferred LayerNorm backwards of mixed C and mixed want_sum (more than LN_RED_MAX = 40: two launches) reduced by ONE call,
    compared bit for bit, item by item, with the immediate form"""
    L, P, S, ops = _abi()
    dev = torch.device("cuda:0")
    items, want, f = [], [], []
    for i in range(73):
        C, M = (768, 1024, 512)[i % 3], (5, 13, 77)[i % 3]
        c = _ln("bwd", C, 0, M, dxs_rows=M if i % 2 else None, dxsum=bool(i % 2), beta_acc=float(i % 4 == 1))
        p = make_ln_problem(c, "randn", "randn", BF, i)
        x, dy = p["x"].to(dev), p["dy"].to(dev, BF)
        mean, rstd, gm = p["mean"].to(dev), p["rstd"].to(dev), p["gamma"].to(dev)
        pair = []
        for deferred in (False, True):
            dg, db, ds = (Guarded(f"item {i} {n}", [1], C, F32, device=dev) for n in ("dgamma", "dbeta", "dxsum"))
            for g_, v in ((dg, p["dgamma0"]), (db, p["dbeta0"]), (ds, p["dxsum0"])):
                g_.seg(0).copy_(v[None])
            dxs = torch.empty(M, C, device=dev, dtype=BF) if c.dxsum else None
            ops.layernorm_bwd(dy, x, mean, rstd, gm, dg.seg(0)[0], db.seg(0)[0], beta_acc=c.beta_acc, dxs=dxs,
                              dxsum=ds.seg(0)[0] if c.dxsum else None, defer=items if deferred else None)
            pair.append((dg, db, ds if c.dxsum else None))
        want.append(pair)
    ops.layernorm_bwd_reduce_batched(items)
    torch.cuda.synchronize()
    bad = 0
    for i, (imm, dfr) in enumerate(want):
        for a, d in zip(imm, dfr):
            if a is None:
                continue
            r = bits_equal(f"item {i} {d.name}", d.seg(0), a.seg(0)) + d.check()
            bad += sum(not x.ok for x in r)
            f += [x for x in r if not x.ok]
    f.append(Finding("73 deferred items (two launches of <= 40): outputs that differ from the immediate form", bad == 0, float(bad), 0.0, ""))
    return f


def check_ln_nonfinite():
    """gscale / nonfinite of pvrl_layernorm_bwd: one inf planted in dy -> the flag reads 1, dgamma is non-finite in that column only;
    without it the flag keeps its pattern; gscale = 0.5 halves dgamma / dbeta / dxsum exactly and nothing else"""
    L, P, S, ops = _abi()
    dev = torch.device("cuda:0")
    f = []
    for (R, B) in ((0, 77), (13, 3)):
        c = _ln("bwd", 768, R, B, dy16=False, dxs_rows=R + B, dxsum=True)
        M, C = R + B, 768
        p = make_ln_problem(c, "randn", "randn", BF, 7)
        res = {}
        for tag, gs, plant in (("plain", None, False), ("half", 0.5, False), ("inf", None, True)):
            dy = p["dy"].clone()
            if plant:
                dy[M // 2, 300] = float("inf")
            xs = ops.SplitRows(p["x"][:R].to(dev, BF), p["x"][R:].to(dev)) if R else p["x"].to(dev)
            b = {n: Guarded(f"{n} ({tag})", [1], C, F32, device=dev) for n in ("dgamma", "dbeta", "dxsum")}
            flag = Guarded(f"nonfinite ({tag})", [1], 1, F32, device=dev)
            if plant:
                flag.seg(0).zero_()
            dxs = Guarded(f"dxs ({tag})", [M], C, BF, device=dev)
            dxo = Guarded(f"dx ({tag})", [M], C, F32, device=dev)
            dlo = Guarded(f"dx_lo ({tag})", [max(R, 1)], C, BF, device=dev)
            dx_out = ops.SplitRows(dlo.seg(0), dxo.seg(0)[R:]) if R else dxo.seg(0)
            gsd = torch.full((1,), gs, device=dev) if gs is not None else None
            ops.layernorm_bwd(dy.to(dev), xs, p["mean"].to(dev), p["rstd"].to(dev), p["gamma"].to(dev), b["dgamma"].seg(0)[0],
                              b["dbeta"].seg(0)[0], dx_out=dx_out, dxs=dxs.seg(0), dxsum=b["dxsum"].seg(0)[0], gscale=gsd,
                              nonfinite=flag.seg(0)[0])
            torch.cuda.synchronize()
            res[tag] = {n: g.seg(0).cpu()[0] for n, g in b.items()}
            res[tag]["dxs"], res[tag]["dx"] = dxs.seg(0).cpu(), dxo.seg(0).cpu()[R:]
            if plant:
                v = float(flag.seg(0).cpu())
                f.append(Finding(f"{R}+{B}: nonfinite flag after an inf in dy", v == 1.0, v, 1.0, ""))
                nf = ~torch.isfinite(res[tag]["dgamma"])
                ok = bool(nf[300]) and int(nf.sum()) == 1
                f.append(Finding(f"{R}+{B}: dgamma non-finite in the planted column only", ok, float(nf.sum()), 1.0, f"columns {nf.nonzero().flatten().tolist()[:8]}"))
            else:
                f += untouched(flag)
        for n in ("dgamma", "dbeta", "dxsum"):
            f += bits_equal(f"{R}+{B}: {n} with gscale = 0.5 against 0.5 * {n}", res["half"][n], res["plain"][n] * 0.5)
        for n in ("dxs", "dx"):
            f += bits_equal(f"{R}+{B}: {n} unchanged by gscale", res["half"][n], res["plain"][n])
    return f


# =====================================================================================================================
# kl_topk (csrc/loss.hip)
# =====================================================================================================================
KL_TOPK_MAX, KL_STAGE_MAX = 8, 12288
KL_REGIMES = ("randn", "hot", "tie_inside", "tie_across", "all_equal", "one_thread")
KlCase = collections.namedtuple("KlCase", "K topk rows ld nulls path")     # nulls: subset of "ldt" (row_loss, dpred, target_out null)


def kl_path(K, topk):
    s = "staged" if K <= KL_STAGE_MAX else "unstaged"
    if K < 256:
        s += ".idle_threads"
    if topk == KL_TOPK_MAX:
        s += ".topk_max"
    if 0 < K < max(topk, 1):
        s += ".K_below_topk"
    return s


def _kl(K, topk, ld=False, nulls=""):
    return KlCase(K, topk, max(8, min(48, 98304 // K)), ld, nulls, kl_path(K, topk))


def kl_case_id(c):
    return f"kl_topk-K{c.K}-top{c.topk}-rows{c.rows}" + ("-ld+4" if c.ld else "") + (f"-null_{c.nulls}" if c.nulls else "") + "-" + c.path


KL_KS = (5, 6, 255, 256, 257, 778, 9871, 12288, 12289)


def kl_regime_ok(c, regime):
    K, k = c.K, c.topk
    if regime in ("randn", "hot", "all_equal"):
        return True
    if regime == "tie_inside":
        return k >= 2 and K > k
    if regime == "tie_across":
        return k >= 1 and K > k + 1
    return k >= 1 and K >= 3 + 256 * k          # one_thread


def _build_kl_tests():
    tests = []
    for K in KL_KS:
        for k in (0, 1, 5, 8):
            c = _kl(K, k)
            tests.append((c, "randn"))
            regs = KL_REGIMES[1:] if k == 5 or (k == 8 and K in (257, 12289, 9871)) or (k == 1 and K in (256, 12288)) else ()
            tests += [(c, r) for r in regs if kl_regime_ok(c, r)]
    for K in (778, 12289):
        tests += [(_kl(K, 5, ld=True), "randn"), (_kl(K, 5, ld=True), "tie_across")]
    for nulls in ("l", "d", "t", "ld", "lt", "dt", "ldt"):
        tests.append((_kl(257, 5, nulls=nulls), "randn"))
    return tests


KL_TESTS = _build_kl_tests()


def make_kl_problem(c, regime, draw=0):
    g = _gen("kl", c.K, c.topk, regime, draw)
    rows, K, k = c.rows, c.K, c.topk
    pred, teacher = torch.randn(rows, K, generator=g) * 3, torch.randn(rows, K, generator=g) * 4
    if regime == "hot":
        pred, teacher = pred / 3 * 8, teacher / 4 * 10
    elif regime == "all_equal":
        teacher = torch.full((rows, K), 1.5)
    elif regime == "tie_inside":
        top = teacher.max(1).values + 1.0
        idx = torch.stack([torch.randperm(K, generator=g)[:2] for _ in range(rows)])
        teacher[torch.arange(rows), idx[:, 0]] = top
        teacher[torch.arange(rows), idx[:, 1]] = top
    elif regime == "tie_across":
        srt = teacher.sort(1, descending=True)
        kth, other = srt.values[:, k - 1], srt.indices[:, K - 1 - int(torch.randint(0, max(K - k - 1, 1), (1,), generator=g))]
        teacher[torch.arange(rows), other] = kth
    elif regime == "one_thread":
        top = teacher.max(1).values
        for i in range(k):
            teacher[:, 3 + 256 * i] = top + 1.0 + 0.5 * i
    # on a grid of 2^-9 > 1e-3: two logits are exactly equal (a tie, kept or dropped together in fp32 as in fp64) or clearly apart
    teacher = torch.round(teacher * 512.0) / 512.0
    return dict(pred=pred, teacher=teacher, grad_scale=1.0 / rows)


def kl_input_conditions(p, c):
    """-> [Finding]: among the top k + 2 teacher logits (one more than needed), neighbours are exactly equal (meant ties) or differ by >= 1e-3; every kept logit
    lies within 80 of the row maximum (no kept probability underflows in fp32)"""
    k = min(c.topk, c.K)
    if k == 0:
        return []
    srt = p["teacher"].double().sort(1, descending=True).values[:, :min(k + 2, c.K)]
    d = srt[:, :-1] - srt[:, 1:]
    bad = int(((d != 0) & (d < 1e-3)).sum())
    far = float((srt[:, 0] - srt[:, k - 1]).max())
    return [Finding("inputs: distinct top logits closer than 1e-3", bad == 0, float(bad), 0.0, ""),
            Finding("inputs: kept logit below the row maximum", far <= 80.0, far, 80.0, "")]


KL_DEFECTS = ("tied_top_value_counted_once", "boundary_tie_drops_k_plus_1", "half_the_candidates_per_thread")


def kl_eval(p, c, mode, defect=None):
    """the semantics of kernel_checks.ref_kl_topk (keep the entries equal to one of the top-k values, a duplicated top value counted as
    often as it occurs among them; renormalise; KL per row).  mode "ref" fp64, "kernel" fp32 with `block_sum`, "torch" plain fp32.
    -> row_loss, target, dpred, norm (sum of the absolute loss terms)"""
    dt = torch.float64 if mode == "ref" else torch.float32
    rsum = (lambda v: block_sum(v)[:, None]) if mode == "kernel" else (lambda v: v.sum(1, keepdim=True))
    pred, tch = p["pred"].to(dt), p["teacher"].to(dt)
    K, k = c.K, min(c.topk, c.K)
    e = torch.exp(tch - tch.max(1, keepdim=True).values)
    t = e * (1.0 / rsum(e))
    if k > 0:
        top = t.topk(k, dim=1).values
        if defect == "half_the_candidates_per_thread":      # each of the 256 threads keeps ceil(k / 2) of its own elements
            nk = -(-K // 256)
            tt = F.pad(t, (0, nk * 256 - K), value=-1.0).reshape(-1, nk, 256)
            keep = tt.topk(min(-(-k // 2), nk), dim=1).values.reshape(t.shape[0], -1)
            top = keep.topk(k, dim=1).values
        mult = (t[:, None, :] == top[:, :, None]).to(dt).sum(1)
        if defect == "tied_top_value_counted_once":
            mult = mult.clamp_max(1.0)
        if defect == "boundary_tie_drops_k_plus_1":         # exactly k entries survive
            order = t.argsort(dim=1, descending=True, stable=True)
            keepm = torch.zeros_like(t).scatter_(1, order[:, :k], 1.0)
            mult = mult * keepm
        tg = t * mult
        tg = tg / rsum(tg)
    else:
        tg = t
    pm = pred.max(1, keepdim=True).values
    pe = torch.exp(pred - pm)
    pse = rsum(pe)
    logp = pred - pm - torch.log(pse)
    terms = torch.where(tg > 0, tg * (torch.log(tg.clamp_min(1e-300 if dt == torch.float64 else 1e-45)) - logp), torch.zeros_like(tg))
    tot = rsum(tg)
    return dict(row_loss=rsum(terms)[:, 0], target=tg, dpred=p["grad_scale"] * (pe * (1.0 / pse) * tot - tg), norm=terms.abs().sum(1))


def _kl_call(c, p, dev, K=None):
    """pvrl_kl_topk on guarded buffers, over the first K columns (default: all) -> {name: Guarded}"""
    L, P, S, ops = _abi()
    e = 4 if c.ld else 0
    rows = c.rows
    Kp = p["pred"].shape[1]
    K = Kp if K is None else K
    pd, td = guarded_input(p["pred"], F32, dev, e), guarded_input(p["teacher"], F32, dev, e)
    b = dict(row_loss=Guarded("row_loss", [rows], 1, F32, device=dev),
             dpred=Guarded("dpred", [rows], Kp, F32, e, unowned=[(0, 0, rows, K, Kp)] if K < Kp else (), device=dev),
             target=Guarded("target_out", [rows], Kp, F32, e, unowned=[(0, 0, rows, K, Kp)] if K < Kp else (), device=dev))
    use = lambda ch, n: None if ch in c.nulls else b[n].seg(0)
    rl, dp, tg = use("l", "row_loss"), use("d", "dpred"), use("t", "target")
    L.call("pvrl_kl_topk", P(pd), Kp + e, P(td), Kp + e, rows, K, c.topk, float(p["grad_scale"]), P(rl), P(dp), Kp + e, P(tg), Kp + e, S())
    torch.cuda.synchronize()
    return b


def gpu_kl(c, p, dev):
    b = _kl_call(c, p, dev)
    f, got = [], {}
    for ch, n in (("l", "row_loss"), ("d", "dpred"), ("t", "target")):
        if ch in c.nulls:
            f += untouched(b[n])
            got[n] = None
        else:
            f += b[n].check()
            got[n] = b[n].seg(0).cpu()
    if got["row_loss"] is not None:
        got["row_loss"] = got["row_loss"][:, 0]
    return got, f


def check_kl_case(c, regime, run=None, spreads=None):
    if run is None:
        dev = torch.device("cuda:0")
        run = lambda c, p: gpu_kl(c, p, dev)
    pre, f, G, R_, A, T = [], [], [], [], [], []
    for d in range(n_draws(c.rows)):
        p = make_kl_problem(c, regime, d)
        cond = kl_input_conditions(p, c)
        pre += [x for x in cond if d == 0 or not x.ok]
        if not all(x.ok for x in cond):
            return pre
        got, fd = run(c, p)
        f += [x for x in fd if d == 0 or not x.ok]
        G.append(got); R_.append(kl_eval(p, c, "ref")); A.append(kl_eval(p, c, "kernel")); T.append(kl_eval(p, c, "torch"))
    got, ref, mod, mod2 = _cat(G), _cat(R_), _cat(A), _cat(T)
    flat = 1e-4 if regime == "randn" else None        # kernel_checks.check_loss
    out = pre + f
    for name, nrm in (("row_loss", ref["norm"]), ("target", None), ("dpred", None)):
        if got.get(name) is None:
            continue
        if spreads is not None:
            spreads.setdefault("kl_topk " + name, []).append(spread(mod[name], mod2[name], ref[name], nrm)[0])
        out += judge(name, got[name], ref[name], mod[name], mod2[name], flat, norm=nrm, key="kl_topk " + name)
    return out


def check_kl_staged_against_unstaged():
    """the same 12288 columns through the staged kernel (K = 12288 of a 12289-wide matrix) and through the unstaged one (K = 12289, the last
    column so low that it contributes an exact zero everywhere): identical bits, as the kernel's comment promises"""
    dev = torch.device("cuda:0")
    f = []
    for topk in (0, 5, 8):
        c = _kl(12289, topk)
        p = make_kl_problem(c, "tie_inside" if topk else "randn")
        p["teacher"][:, 12288] = -1e30
        p["pred"][:, 12288] = -1e30
        un = _kl_call(c, p, dev)
        st = _kl_call(c, p, dev, K=12288)
        for n in ("row_loss", "dpred", "target"):
            f += un[n].check() + st[n].check()
            f += bits_equal(f"topk {topk} {n}: staged against unstaged", st[n].seg(0)[:, :min(12288, st[n].cols)], un[n].seg(0)[:, :min(12288, un[n].cols)])
    return f


def check_kl_refusals():
    """topk = 9 and K = 0: PVRL_EINVAL, outputs untouched"""
    from procedurevrl_amd._lib import PvrlError
    L, P, S, ops = _abi()
    dev = torch.device("cuda:0")
    f = []
    x = torch.randn(4, 64).to(dev)
    for name, K, topk in (("topk = 9", 64, 9), ("K = 0", 0, 5), ("topk = -1", 64, -1)):
        b = [Guarded("row_loss", [4], 1, F32, device=dev), Guarded("dpred", [4], 64, F32, device=dev), Guarded("target_out", [4], 64, F32, device=dev)]
        try:
            L.call("pvrl_kl_topk", P(x), 64, P(x), 64, 4, K, topk, 1.0, P(b[0].seg(0)), P(b[1].seg(0)), 64, P(b[2].seg(0)), 64, S())
            msg = "returned 0"
        except PvrlError as e:
            msg = str(e)
        torch.cuda.synchronize()
        f.append(Finding(f"pvrl_kl_topk {name}: status", msg.endswith("status -1"), 0.0, 0.0, msg))
        for g in b:
            f += untouched(g)
    return f


# =====================================================================================================================
# soft_ce
# =====================================================================================================================
CeCase = collections.namedtuple("CeCase", "K rows mode hot dx path")      # mode "given" / "synth"
CE_TESTS = [CeCase(K, 32, mode, hot, dx, mode + (".hot" if hot else "") + ("" if dx else ".dx_null"))
            for K in (97, 257, 300, 1000) for (mode, hot, dx) in (("given", False, True), ("synth", False, True), ("given", True, True), ("synth", True, False))]
CE_DEFECTS = ("target_sum_taken_as_1",)


def ce_case_id(c):
    return f"soft_ce-K{c.K}-rows{c.rows}-{c.path}"


def make_ce_problem(c, draw=0):
    g = _gen("ce", c.K, c.mode, c.hot, draw)
    rows, K = c.rows, c.K
    x = torch.randn(rows, K, generator=g) * (40.0 if c.hot else 3.0)
    labels = torch.randint(0, K, (rows,), generator=g)
    partner = torch.arange(rows - 1, -1, -1)
    partner[0], partner[1] = -1, rows + 3               # both read as "no partner": the row itself
    lam = torch.rand(rows, generator=g)
    on, off = 1.0 - 0.1 + 0.1 / K, 0.1 / K
    pe = torch.where((partner < 0) | (partner >= rows), torch.arange(rows), partner)
    oh = lambda l: torch.where(torch.arange(K)[None] == l[:, None], torch.tensor(on), torch.tensor(off))
    synth = oh(labels) * lam[:, None] + oh(labels[pe]) * (1 - lam)[:, None]          # two rounded products and a rounded sum (mixup_target)
    p = dict(x=x, labels=labels, partner=partner, lam=lam, lam_partner=1 - lam, on=on, off=off, synth=synth, grad_scale=1.0 / rows)
    # the given target of the EPIC noun head does not sum to 1
    p["target"] = synth if c.mode == "synth" else torch.rand(rows, K, generator=g) * (torch.rand(rows, K, generator=g) < 0.1) * 0.7
    return p


def ce_eval(p, c, mode, defect=None):
    dt = torch.float64 if mode == "ref" else torch.float32
    rsum = (lambda v: block_sum(v)[:, None]) if mode == "kernel" else (lambda v: v.sum(1, keepdim=True))
    x, t = p["x"].to(dt), p["target"].to(dt)
    mx = x.max(1, keepdim=True).values
    e = torch.exp(x - mx)
    se = rsum(e)
    ts = torch.ones_like(se) if defect == "target_sum_taken_as_1" else rsum(t)
    lz = mx + torch.log(se)
    terms = t * (lz - x)
    return dict(row_loss=rsum(terms)[:, 0], dx=p["grad_scale"] * (ts * (e * (1.0 / se)) - t), norm=terms.abs().sum(1))


def _ce_call(c, p, dev, given):
    from procedurevrl_amd._lib import struct_dtype
    import numpy as np
    L, P, S, ops = _abi()
    rows, K = c.rows, c.K
    xd = guarded_input(p["x"], F32, dev, 4)
    b = dict(row_loss=Guarded("row_loss", [rows], 1, F32, device=dev), dx=Guarded("dx", [rows], K, F32, 4, device=dev))
    dx = b["dx"].seg(0) if c.dx else None
    if given:
        td = guarded_input(p["target"], F32, dev, 4)
        L.call("pvrl_soft_ce", P(xd), K + 4, rows, K, P(td), K + 4, None, None, 0.0, 0.0, float(p["grad_scale"]), P(b["row_loss"].seg(0)), P(dx),
               K + 4, S())
    else:
        d = np.zeros(rows, dtype=struct_dtype("pvrl_mix_desc"))
        d["partner"], d["kind"] = p["partner"].numpy(), 1
        d["lam"], d["lam_partner"] = p["lam"].numpy(), p["lam_partner"].numpy()
        desc = torch.from_numpy(d.view(np.uint8)).to(dev)
        lab = p["labels"].to(dev)
        L.call("pvrl_soft_ce", P(xd), K + 4, rows, K, None, 0, P(lab), P(desc), float(p["on"]), float(p["off"]), float(p["grad_scale"]),
               P(b["row_loss"].seg(0)), P(dx), K + 4, S())
    torch.cuda.synchronize()
    return b


def gpu_ce(c, p, dev):
    b = _ce_call(c, p, dev, c.mode == "given")
    f = b["row_loss"].check() + (b["dx"].check() if c.dx else untouched(b["dx"]))
    if c.mode == "synth":           # the same target handed over densely: identical bits
        b2 = _ce_call(c, p, dev, True)
        f += bits_equal("row_loss: synthesised against given target", b["row_loss"].seg(0), b2["row_loss"].seg(0))
        if c.dx:
            f += bits_equal("dx: synthesised against given target", b["dx"].seg(0), b2["dx"].seg(0))
    return dict(row_loss=b["row_loss"].seg(0).cpu()[:, 0], dx=b["dx"].seg(0).cpu() if c.dx else None), f


def check_ce_case(c, run=None, spreads=None):
    if run is None:
        dev = torch.device("cuda:0")
        run = lambda c, p: gpu_ce(c, p, dev)
    out, G, R_, A, T = [], [], [], [], []
    for d in range(n_draws(c.rows)):
        p = make_ce_problem(c, d)
        got, fd = run(c, p)
        out += [x for x in fd if d == 0 or not x.ok]
        G.append(got); R_.append(ce_eval(p, c, "ref")); A.append(ce_eval(p, c, "kernel")); T.append(ce_eval(p, c, "torch"))
    got, ref, mod, mod2 = _cat(G), _cat(R_), _cat(A), _cat(T)
    for name, nrm in (("row_loss", ref["norm"]), ("dx", None)):
        if got.get(name) is None:
            continue
        if spreads is not None:
            spreads.setdefault("soft_ce " + name, []).append(spread(mod[name], mod2[name], ref[name], nrm)[0])
        out += judge(name, got[name], ref[name], mod[name], mod2[name], None if c.hot else TOL_F32, norm=nrm, key="soft_ce " + name)
    return out


# =====================================================================================================================
# the other loss kernels and the row helpers: one table, one driver
# =====================================================================================================================
# an entry: make(case) -> p; evals(p, mode) -> {tensor: value} (+ "norm:<tensor>"); gpu(p, dev) -> (got, findings); flat: {tensor: bound}
SimpleCase = collections.namedtuple("SimpleCase", "entry shape opt path")


def simple_case_id(c):
    return f"{c.entry}-{c.shape}" + (f"-{c.opt}" if c.opt else "") + "-" + c.path


def _sum_modes(mode):
    dt = torch.float64 if mode == "ref" else torch.float32
    rsum = (lambda v: block_sum(v)[:, None]) if mode == "kernel" else (lambda v: v.sum(1, keepdim=True))
    return dt, rsum


def _exp_fast(v, mode):
    """__expf kernels: "kernel" model plain exp, second model exp2(x * log2 e) in fp32"""
    return torch.exp2(v * LOG2E) if mode == "torch" else torch.exp(v)


# ---- l2norm -------------------------------------------------------------------------------------------------------------
def _l2_make(c, draw=0):
    g = _gen("l2", c.shape, draw)
    M, D = 33, c.shape
    x = torch.randn(M, D, generator=g) * torch.pow(10.0, torch.rand(M, 1, generator=g) * 4 - 2)
    return dict(x=x, dy=torch.randn(M, D, generator=g))


def _l2_eval(p, c, mode):
    dt, rsum = _sum_modes(mode)
    x, dy = p["x"].to(dt), p["dy"].to(dt)
    inv = 1.0 / torch.sqrt(rsum(x * x))
    y = x * inv
    # the backward reads y and inv as stored: fp32 values of the `kernel` model in every mode (inputs of that kernel)
    yk, ik = (y, inv) if mode == "kernel" else (p["_y"].to(dt), p["_inv"].to(dt))
    dx = ik * (dy - yk * rsum(dy * yk))
    return dict(y=y, inv_norm=inv[:, 0], dx=dx)


def _l2_gpu(p, c, dev):
    L, P, S, ops = _abi()
    M, D = p["x"].shape
    xd, dyd = guarded_input(p["x"], F32, dev, 4), guarded_input(p["dy"], F32, dev, 4)
    yin, iin = guarded_input(p["_y"], F32, dev, 4), guarded_input(p["_inv"], F32, dev, 0)
    yb, ib, db = Guarded("y", [M], D, F32, 4, device=dev), Guarded("inv_norm", [M], 1, F32, device=dev), Guarded("dx", [M], D, F32, 4, device=dev)
    L.call("pvrl_l2norm_fwd", P(xd), D + 4, P(yb.seg(0)), D + 4, P(ib.seg(0)), M, D, S())
    L.call("pvrl_l2norm_bwd", P(dyd), D + 4, P(yin), D + 4, P(iin), P(db.seg(0)), D + 4, M, D, S())
    torch.cuda.synchronize()
    return dict(y=yb.seg(0).cpu(), inv_norm=ib.seg(0).cpu()[:, 0], dx=db.seg(0).cpu()), yb.check() + ib.check() + db.check()


def _l2_prep(p, c):
    x = p["x"]
    inv = 1.0 / torch.sqrt(block_sum(x * x)[:, None])
    p["_y"], p["_inv"] = x * inv, inv
    return p


# ---- softmax_rows -------------------------------------------------------------------------------------------------------
def _sm_make(c, draw=0):
    g = _gen("sm", c.shape, draw)
    return dict(x=torch.randn(9, c.shape, generator=g) * 40.0)


def _sm_eval(p, c, mode):
    dt, rsum = _sum_modes(mode)
    x = p["x"].to(dt)
    e = _exp_fast(x - x.max(1, keepdim=True).values, mode)
    if mode == "torch":
        rsum = lambda v: block_sum(v)[:, None]
    return dict(y=e * (1.0 / rsum(e)))


def _sm_gpu(p, c, dev):
    L, P, S, ops = _abi()
    M, N = p["x"].shape
    xd = guarded_input(p["x"], F32, dev, 4)
    yb = Guarded("y", [M], N, F32, 4, device=dev)
    L.call("pvrl_softmax_rows_f32", P(xd), N + 4, P(yb.seg(0)), N + 4, M, N, S())
    torch.cuda.synchronize()
    return dict(y=yb.seg(0).cpu()), yb.check()


# ---- mse ----------------------------------------------------------------------------------------------------------------
def _mse_make(c, draw=0):
    g = _gen("mse", c.shape, draw)
    return dict(a=torch.randn(1, c.shape, generator=g), b=torch.randn(1, c.shape, generator=g), gs=0.37)


def _mse_eval(p, c, mode):
    dt, rsum = _sum_modes(mode)
    a, b = p["a"].to(dt), p["b"].to(dt)
    n = a.numel()
    d = a - b
    gs = torch.tensor(p["gs"], dtype=dt) * 2.0 / n
    out = {"loss": rsum(d * d)[:, 0] / n, "norm:loss": (d * d).sum(1) / n}
    if c.opt != "nograd":
        out.update(da=(gs * d).reshape(-1), db=(-gs * d).reshape(-1))
    return out


def _mse_gpu(p, c, dev):
    L, P, S, ops = _abi()
    n = p["a"].numel()
    ad, bd = guarded_input(p["a"], F32, dev, 0), guarded_input(p["b"], F32, dev, 0)
    lb, da, db = Guarded("loss", [1], 1, F32, device=dev), Guarded("da", [1], n, F32, device=dev), Guarded("db", [1], n, F32, device=dev)
    grad = c.opt != "nograd"
    L.call("pvrl_mse", P(ad), P(bd), n, p["gs"] if grad else 0.0, P(lb.seg(0)), P(da.seg(0)) if grad else None, P(db.seg(0)) if grad else None, S())
    torch.cuda.synchronize()
    got = dict(loss=lb.seg(0).cpu()[0])
    f = lb.check()
    if grad:
        got.update(da=da.seg(0).cpu()[0], db=db.seg(0).cpu()[0])
        f += da.check() + db.check()
    else:
        f += untouched(da) + untouched(db)
    return got, f


# ---- gelu_f32 -----------------------------------------------------------------------------------------------------------
def _gelu_make(c, draw=0):
    g = _gen("gelu", c.shape, draw)
    n = c.shape
    x = (torch.rand(n, generator=g) * 20 - 10)
    x[:5] = torch.tensor([0.0, -10.0, 10.0, 1e-4, -1e-4])[:min(5, n)] if n >= 5 else x[:5]
    return dict(x=x, dy=torch.randn(n, generator=g))


def _gelu_eval(p, c, mode):
    dt = torch.float64 if mode == "ref" else torch.float32
    x, dy = p["x"].to(dt), p["dy"].to(dt)
    cdf = 0.5 * (1.0 + torch.erf(x * 0.70710678118654752))
    pdf = 0.3989422804014327 * (_exp_fast(-0.5 * x * x, mode) if mode != "ref" else torch.exp(-0.5 * x * x))
    return dict(gelu=0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752)), dgelu=dy * (cdf + x * pdf))


def _gelu_gpu(p, c, dev):
    L, P, S, ops = _abi()
    n = p["x"].numel()
    xd, dyd = guarded_input(p["x"][None], F32, dev, 0), guarded_input(p["dy"][None], F32, dev, 0)
    a, b = Guarded("gelu", [1], n, F32, device=dev), Guarded("dgelu", [1], n, F32, device=dev)
    L.call("pvrl_gelu_f32", P(xd), None, P(a.seg(0)), n, S())
    L.call("pvrl_gelu_f32", P(xd), P(dyd), P(b.seg(0)), n, S())
    torch.cuda.synchronize()
    return dict(gelu=a.seg(0).cpu()[0], dgelu=b.seg(0).cpu()[0]), a.check() + b.check()


# ---- milnce -------------------------------------------------------------------------------------------------------------
def _mil_make(c, draw=0):
    n, C = c.shape
    g = _gen("milnce", n, C, draw)
    v = F.normalize(torch.randn(n, 32, generator=g), dim=1)
    t = F.normalize(torch.randn(n * C, 32, generator=g), dim=1)
    return dict(x=(v @ t.t()) / 0.02, gs=1.0 / n)


def _mil_eval(p, c, mode):
    n, C = c.shape
    dt, rsum = _sum_modes(mode)
    x = p["x"].to(dt).reshape(n, n, C)
    i = torch.arange(n)
    diag = x[i, i]                                                  # [n, C]
    rowcol = torch.stack([x.reshape(n, n * C), x.permute(1, 0, 2).reshape(n, n * C)], 2).reshape(n, 2 * n * C)   # row i and column i, interleaved as summed
    mx = rowcol.max(1, keepdim=True).values
    if mode == "kernel":        # one partial per thread holds exp(row) + exp(col) of its elements
        e = torch.exp(rowcol - mx).reshape(n, n * C, 2)
        den = mx[:, 0] + torch.log(block_sum(e[:, :, 0] + e[:, :, 1]))
    else:
        den = mx[:, 0] + torch.log(torch.exp(rowcol - mx).sum(1))
    nm = diag.max(1, keepdim=True).values
    nom = nm[:, 0] + torch.log(rsum(torch.exp(diag - nm))[:, 0])
    gx = torch.exp(x - den[:, None, None]) + torch.exp(x - den[None, :, None])
    gx[i, i] = gx[i, i] - torch.exp(diag - nom[:, None])
    return dict(nom=nom, den=den, dx=(p["gs"] * gx).reshape(n, n * C))


def _mil_gpu(p, c, dev):
    L, P, S, ops = _abi()
    n, C = c.shape
    xd = guarded_input(p["x"], F32, dev, 0)
    nb, db, gb = Guarded("nom", [n], 1, F32, device=dev), Guarded("den", [n], 1, F32, device=dev), Guarded("dx", [n], n * C, F32, device=dev)
    L.call("pvrl_milnce", P(xd), n, C, p["gs"], P(nb.seg(0)), P(db.seg(0)), P(gb.seg(0)), S())
    torch.cuda.synchronize()
    return dict(nom=nb.seg(0).cpu()[:, 0], den=db.seg(0).cpu()[:, 0], dx=gb.seg(0).cpu()), nb.check() + db.check() + gb.check()


# ---- batch_sum / group_reduce / gemv_rows -------------------------------------------------------------------------------
def _bs_make(c, draw=0):
    B, rows, C = c.shape
    g = _gen("bs", c.shape, c.opt, draw)
    dx = torch.randn(B * rows, C, generator=g)
    return dict(dx=_r16(dx, BF) if c.opt == "16" else dx)


def _bs_eval(p, c, mode):
    B, rows, C = c.shape
    x = p["dx"].reshape(B, rows, C)
    if mode == "ref":
        return dict(G=x.double().sum(0))
    if mode == "torch":
        return dict(G=x.sum(0))
    a = torch.zeros(rows, C)
    for b in range(B):
        a = a + x[b]
    return dict(G=a)


def _bs_gpu(p, c, dev):
    L, P, S, ops = _abi()
    B, rows, C = c.shape
    six = c.opt == "16"
    xd = guarded_input(p["dx"], BF if six else F32, dev, 8)
    gb = Guarded("G", [rows], C, F32, device=dev)
    L.call("pvrl_batch_sum_bf16" if six else "pvrl_batch_sum", P(xd), C + 8, B, rows, C, P(gb.seg(0)), S())
    torch.cuda.synchronize()
    return dict(G=gb.seg(0).cpu()), gb.check()


def _gr_make(c, draw=0):
    groups, G, C = c.shape
    g = _gen("gr", c.shape, c.opt, draw)
    x = torch.randn(groups * G, C, generator=g)
    return dict(x=_r16(x, BF) if c.opt[0] == "h" else x, scale=torch.rand(groups * G, generator=g) + 0.5, resid=torch.randn(groups, C, generator=g),
                alpha=0.125)


def _gr_eval(p, c, mode):
    groups, G, C = c.shape
    dt = torch.float64 if mode == "ref" else torch.float32
    x = (p["x"].to(dt) * p["scale"].to(dt)[:, None]).reshape(groups, G, C)
    if mode == "kernel":
        a = torch.zeros(groups, C)
        for t in range(G):
            a = a + x[:, t]
    else:
        a = x.sum(1)
    out = a * p["alpha"] + p["resid"].to(dt)
    if c.opt[1] == "h" and mode != "ref":
        out = _r16(out, BF)
    return dict(out=out)


def _gr_gpu(p, c, dev):
    L, P, S, ops = _abi()
    groups, G, C = c.shape
    xd = guarded_input(p["x"], BF if c.opt[0] == "h" else F32, dev, 4)
    # out: a view into a larger matrix (rows R : M, as engine.py passes dqkv[R:M]): the segment behind the guard rows, ld C + 4
    ob = Guarded("out", [groups], C, BF if c.opt[1] == "h" else F32, 4, device=dev)
    sc, rs = guarded_input(p["scale"][:, None], F32, dev, 0), guarded_input(p["resid"], F32, dev, 4)
    ops.group_reduce(xd, groups, G, scale=sc[:, 0], alpha=p["alpha"], resid=rs, out=ob.seg(0))
    torch.cuda.synchronize()
    return dict(out=ob.seg(0).float().cpu()), ob.check()


def _gv_make(c, draw=0):
    R, C = c.shape
    g = _gen("gv", c.shape, c.opt, draw)
    W = torch.randn(R, C, generator=g)
    return dict(W=_r16(W, BF) if c.opt == "16" else W, x=torch.randn(C, generator=g), y0=torch.randn(R, generator=g), beta=1.0, gs=0.5)


def _gv_eval(p, c, mode):
    dt = torch.float64 if mode == "ref" else torch.float32
    prod = p["W"].to(dt) * p["x"].to(dt)[None]
    if mode == "kernel":
        R, C = prod.shape
        t = F.pad(prod, (0, -C % 64)).reshape(R, -1, 64)
        acc = torch.zeros(R, 64)
        for j in range(t.shape[1]):
            acc = acc + t[:, j]
        s = tree64(acc)
    else:
        s = prod.sum(1)
    return dict(y=p["beta"] * p["y0"].to(dt) + s * p["gs"])


def _gv_gpu(p, c, dev):
    L, P, S, ops = _abi()
    R, C = c.shape
    Wd = guarded_input(p["W"], BF if c.opt == "16" else F32, dev, 8)
    xd = guarded_input(p["x"][None], F32, dev, 0)[0]
    yb = Guarded("y", [R], 1, F32, device=dev)
    yb.seg(0).copy_(p["y0"][:, None])
    ops.gemv_rows(Wd, xd, out=yb.seg(0)[:, 0], beta=p["beta"], gscale=torch.full((1,), p["gs"], device=dev))
    torch.cuda.synchronize()
    return dict(y=yb.seg(0).cpu()[:, 0]), yb.check()


SIMPLE = {
    "l2norm": dict(make=lambda c, d=0: _l2_prep(_l2_make(c, d), c), rows=lambda c: 33, ev=_l2_eval, gpu=_l2_gpu, flat=dict()),
    "softmax_rows": dict(rows=lambda c: 9, make=_sm_make, ev=_sm_eval, gpu=_sm_gpu, flat=dict()),
    "mse": dict(rows=lambda c: 1, make=_mse_make, ev=_mse_eval, gpu=_mse_gpu, flat=dict(loss=TOL_F32, da=TOL_F32, db=TOL_F32)),
    "gelu_f32": dict(rows=lambda c: c.shape, make=_gelu_make, ev=_gelu_eval, gpu=_gelu_gpu, flat=dict()),
    "milnce": dict(rows=lambda c: c.shape[0], make=_mil_make, ev=_mil_eval, gpu=_mil_gpu, flat=dict()),
    "batch_sum": dict(rows=lambda c: c.shape[1], make=_bs_make, ev=_bs_eval, gpu=_bs_gpu, flat=dict(G=TOL_F32)),
    "group_reduce": dict(rows=lambda c: c.shape[0], make=_gr_make, ev=_gr_eval, gpu=_gr_gpu, flat=dict()),
    "gemv_rows": dict(rows=lambda c: c.shape[0], make=_gv_make, ev=_gv_eval, gpu=_gv_gpu, flat=dict(y=1e-5)),
}
GRID_CAP = 8192 * 256            # elementwise.hip grid_for: threads of the largest grid; loss.hip's elementwise kernels: 4096 * 256


def _build_simple_cases():
    S = SimpleCase
    cs = [S("l2norm", D, "", "ld+4" + (".idle_threads" if D < 256 else "")) for D in (1, 255, 257, 512, 1000)]
    cs += [S("softmax_rows", N, "", "logits_x40.ld+4" + (".idle_threads" if N < 256 else "")) for N in (1, 255, 257, 9871)]
    cs += [S("mse", n, opt, "one_workgroup") for n in (1, 255, 257, 4096) for opt in ("", "nograd")]
    cs += [S("gelu_f32", 1000, "", "below_cap"), S("gelu_f32", 4096 * 256 + 5, "", "past_the_4096_workgroup_cap")]
    cs += [S("milnce", (n, C), "", "past_the_4096_workgroup_cap" if n * n * C > 4096 * 256 else "below_cap")
           for (n, C) in ((1, 1), (4, 3), (24, 5), (128, 64), (130, 64))]
    for B in (1, 5):
        cs.append(S("batch_sum", (B, 3, 8), "32", "ragged"))
        cs.append(S("batch_sum", (B, 3, 8), "16", "ragged"))
        cs.append(S("batch_sum", (B, 2731, 3072), "32", "past_the_8192_workgroup_cap"))
        cs.append(S("batch_sum", (B, 2731, 3072), "16", "below_cap"))
    cs.append(S("batch_sum", (1, 5462, 3072), "16", "past_the_8192_workgroup_cap"))
    for opt in ("ff", "fh", "hf", "hh"):      # TIn / TOut: f fp32, h the 16-bit operand type
        cs += [S("group_reduce", (5, G, 768), opt, "view_out") for G in (1, 8)]
    cs.append(S("group_reduce", (2731, 1, 768), "hf", "past_the_8192_workgroup_cap"))
    cs.append(S("group_reduce", (2731, 8, 768), "fh", "past_the_8192_workgroup_cap"))
    cs += [S("gemv_rows", (R, C), opt, "wg%d" % (-(-R // 4))) for R in (1, 3, 4, 5) for C in (1, 63, 65) for opt in ("32", "16")]
    return cs


SIMPLE_CASES = _build_simple_cases()


def check_simple_case(c, run=None, spreads=None):
    E = SIMPLE[c.entry]
    if run is None:
        dev = torch.device("cuda:0")
        run = lambda c, p: E["gpu"](p, c, dev)
    out, G, R_, A, T = [], [], [], [], []
    for d in range(n_draws(E["rows"](c))):
        p = E["make"](c, d)
        got, fd = run(c, p)
        out += [x for x in fd if d == 0 or not x.ok]
        G.append(got)
        for acc, m in ((R_, "ref"), (A, "kernel"), (T, "torch")):
            acc.append(E["ev"](p, c, m))
    got, ref, mod, mod2 = _cat(G), _cat(R_), _cat(A), _cat(T)
    for name in got:
        nrm = ref.get("norm:" + name)
        sixteen = c.entry == "group_reduce" and c.opt[1] == "h"
        flat = TOL_BF16 if sixteen else E["flat"].get(name)
        if spreads is not None and not sixteen:
            spreads.setdefault(f"{c.entry} {name}", []).append(spread(mod[name], mod2[name], ref[name], nrm)[0])
        out += judge(name, got[name], ref[name], mod[name], None if sixteen else mod2[name], flat, norm=nrm, key=f"{c.entry} {name}")
    return out


# =====================================================================================================================
# bit-exact helpers: cast_scale, group_bcast, embed_table, cast_weight_pad, cast_weight
# =====================================================================================================================
EXACT_CASES = [("cast_scale", (3, 8), "rowscale"), ("cast_scale", (16400, 1024), "rowscale"), ("cast_scale", (16400, 1024), "norowscale"),
               ("cast_scale", (77, 768), "norowscale"),
               ("group_bcast", (5, 8, 768), "below_cap"), ("group_bcast", (3, 1, 5), "ragged"), ("group_bcast", (342, 8, 768), "past_the_8192_workgroup_cap"),
               ("embed_table", (9, 4, 768), "below_cap"), ("embed_table", (197, 14, 768), "past_the_8192_workgroup_cap"),
               ("cast_weight_pad", (70, 45, 96, 64), "bias"), ("cast_weight_pad", (33, 100, 64, 128), "nobias"), ("cast_weight_pad", (1, 1, 32, 32), "bias"),
               ("cast_weight", (300, 130), "with_t"), ("cast_weight", (65, 31), "no_t")]


def exact_case_id(c):
    return f"{c[0]}-{'x'.join(str(v) for v in c[1])}-{c[2]}"


def check_exact_case(c):
    """contract = one correctly rounded expression: bit equality with the fp32 torch restatement; outputs in guard bands (row-offset views)"""
    L, P, S, ops = _abi()
    dev = torch.device("cuda:0")
    entry, shape, opt = c
    g = _gen("exact", c)
    if entry == "cast_scale":
        M, C = shape
        x = torch.randn(M, C, generator=g) * 3
        rs = torch.rand(M, generator=g) * 2
        ob = Guarded("out", [M], C, BF, 8, device=dev)
        xd = guarded_input(x, F32, dev, 4)
        rd = guarded_input(rs[:, None], F32, dev, 0)[:, 0] if opt == "rowscale" else None
        ops.cast_scale(xd, rd, out=ob.seg(0))
        torch.cuda.synchronize()
        if opt != "rowscale":
            return ob.check() + bits_equal("out = R16(x)", ob.seg(0), x.to(BF))
        # the product rounded to fp32 and then to 16 bits (v_pk_mul_f32 + v_cvt_pk), or the exact product rounded once (v_fma_mix*_f16):
        # the compiler picks per element; both are correct roundings of rowscale * x
        return ob.check() + bits_among("out = R16(rowscale * x), rounded once or through fp32", ob.seg(0),
                                       [(rs[:, None] * x).to(BF), r16_once(rs.double()[:, None] * x.double(), BF)])
    if entry == "group_bcast":
        groups, G, C = shape
        x, sc = torch.randn(groups, C, generator=g), torch.rand(groups * G, generator=g) + 0.5
        ob = Guarded("out", [groups * G], C, BF, 4, device=dev)
        ops.group_bcast(guarded_input(x, F32, dev, 4), groups, G, scale=guarded_input(sc[:, None], F32, dev, 0)[:, 0], alpha=0.125, out=ob.seg(0))
        torch.cuda.synchronize()
        a, xr = (torch.tensor(0.125) * sc)[:, None], x.repeat_interleave(G, 0)
        return ob.check() + bits_among("out = R16(fl(alpha * scale) * x), rounded once or through fp32", ob.seg(0),
                                       [(a * xr).to(BF), r16_once(a.double() * xr.double(), BF)])
    if entry == "embed_table":
        N, T, C = shape
        pos, tim, bias = torch.randn(1 + N, C, generator=g), torch.randn(T, C, generator=g), torch.randn(C, generator=g)
        eb = Guarded("E", [N * T], C, F32, device=dev)
        pd, td, bd = guarded_input(pos, F32, dev, 0), guarded_input(tim, F32, dev, 0), guarded_input(bias[None], F32, dev, 0)
        L.call("pvrl_embed_table", P(pd), P(td), P(bd), P(eb.seg(0)), N, T, C, S())
        torch.cuda.synchronize()
        want = ((bias + pos[1:, None, :]) + tim[None, :, :]).reshape(N * T, C)
        return eb.check() + bits_equal("E = (bias + pos) + time", eb.seg(0), want)
    if entry == "cast_weight_pad":
        N, K, Np, Kp = shape
        w, bias = torch.randn(N, K, generator=g), torch.randn(N, generator=g)
        ob = Guarded("out", [Np], Kp, BF, 0, unowned=[(0, N, Np, 0, Kp), (0, 0, N, K, Kp)], device=dev)
        tb = Guarded("out_t", [Kp], Np, BF, 0, unowned=[(0, K, Kp, 0, Np), (0, 0, K, N, Np)], device=dev)
        bb = Guarded("out_b", [1], Np, F32, 0, unowned=[(0, 0, 1, N, Np)], device=dev)
        wd, bd = guarded_input(w, F32, dev, 0), guarded_input(bias[None], F32, dev, 0)[0]
        if opt == "bias":
            ops.cast_weight_pad(wd, ob.seg(0), tb.seg(0), bias=bd, out_b=bb.seg(0)[0])
        else:
            ops.cast_weight_pad(wd, ob.seg(0), tb.seg(0))
        torch.cuda.synchronize()
        f = ob.check() + tb.check() + (bb.check() if opt == "bias" else untouched(bb))
        f += bits_equal("out[:N, :K] = R16(w)", ob.seg(0)[:N, :K], w.to(BF)) + bits_equal("out_t[:K, :N] = R16(w)^T", tb.seg(0)[:K, :N], w.t().to(BF))
        if opt == "bias":
            f += bits_equal("out_b[:N] = bias", bb.seg(0)[0, :N], bias)
        return f
    R, C = shape
    w = torch.randn(R, C, generator=g)
    ob, tb = Guarded("out", [R], C, BF, 0, device=dev), Guarded("out_t", [C], R, BF, 0, device=dev)
    ops.cast_weight(guarded_input(w, F32, dev, 0), out=ob.seg(0), out_t=tb.seg(0) if opt == "with_t" else None, need_t=opt == "with_t")
    torch.cuda.synchronize()
    f = ob.check() + bits_equal("out = R16(w)", ob.seg(0), w.to(BF))
    return f + ((tb.check() + bits_equal("out_t = R16(w)^T", tb.seg(0), w.t().to(BF))) if opt == "with_t" else untouched(tb))
