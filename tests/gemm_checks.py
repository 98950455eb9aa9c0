"""The GEMM kernels -- csrc/gemm_nt.hip, gemm_nt_core.h, gemm_nt8_core.h, gemm_nt_skinny.h, gemm_tn.hip, gemm_tn_core.h, gemm_tn8_core.h and
cls_chain.hip -- against an fp64 reference PER (OUTPUT ROW, 64-COLUMN BLOCK), exactly where the inputs allow it, through every dispatch
path, inside guard bands.

Used by tests/test_gemm_gpu.py (pytest -m gpu: the HIP kernels through the C ABI, `lib().call`, so that every workspace and output buffer
is the harness's own) and tests/test_gemm_harness_host.py (no GPU: the rounding model stands in for the kernel, planted defects show that
the rules bite).  Metric (`rowerr`, `agg`), tolerance rule (`judge_tensor`, ROW_FACTOR, REL_Y_FACTOR), guard bands (`Guarded`,
`guarded_input`) and workspace tails (WS_TAIL, WS_FILL) are those of tests/attn_checks.py and tests/pool_attn_checks.py, imported; this
is the GEMM counterpart of tests/mvit_pool_checks.py -- read those docstrings first.  Only what differs is said here.

Why.  tests/kernel_checks.py judges these kernels by the aggregate relative L2 norm alone.  Their typical bug is LOCAL -- a tail sub-tile,
a seam of the persistent kernel, the last K-tile, one split's partial: one wrong 64-row sub-tile of one 256-column tile in 100100 x 384
moves that norm by sqrt(64 * 256 / (100100 * 384)) = 2e-2 of its own relative error, so a 10 % error there reads 2e-3 against the 1e-2 bound.

Segments.  A row of every judged tensor is (output row, 64-column block): the 64 x 64 wave block is the unit of every kernel (the fp32
kernels of cls_chain.hip / gemm_f32_small own 16 columns per workgroup: rows of 16 when N is not a multiple of 64).

Regimes.
  exact   A / P integers in [-2, 2], W / Q integers in [-2, 2] / 4, bias, bias2, aux multiples of 1/4, rowscale in {0.5, 1, 2}, beta in
          {0, 0.5, 1}, gscale a power of two.  With K <= 3072 every partial sum is a multiple of 1/16 below 2^14: fp32 accumulation is
          exact IN ANY ORDER, across splits too.  F32, RESID_F32, dW, dbias and the fp32 small kernels must EQUAL the fp64 result, BF16,
          RESID_16, both table forms and the `u` output of GELU / QGELU its ONE RNE rounding to the operand type (|c| <= 3072: true for
          fp16 too).  Zero tolerance: any wrong row, column, k range, split, table row or sub-tile assignment fails.  (The activation
          outputs -- g of GELU / QGELU, out0 of DGELU / DQGELU -- are not exactly representable: they take the rules below here as well.)
  k_edge  as `exact`, A non-zero only in columns {0, 63, 64, K - 64, K - 1}; TN: P non-zero only in rows {0, 63, 64, Ms - 1, Ms, M - 1}
          (Ms the slice height): a dropped first / last stage, a stage lost at a persistent seam.
  randn   N(0, 1) x 0.05 N(0, 1), what kernel_checks measures.
  hot     rows of A and rows of W (TN: columns of P and of Q) scaled by 2^(i mod 13 - 6): a row mix-up is an order of magnitude; the
          row scale undoes A's part.
  cancel  the second half of K (TN: of M) is the negated first half + 2^-6 N(0, 1) on one operand, a copy on the other: the result is
          small against sum |a w|.
Every (family, epilogue) pair that exists runs `exact`; every family runs each other regime at least once (`NT_TESTS`, `TN_TESTS`, ...).

Rules for what is not exact.  Reference: fp64 on the 16-bit-valued operands, in FULL for every case.  Model, restated from
nt_epilogue_at / gemm_nt_skinny_kernel / the reduce kernels: fp32 accumulation in K-tile order (TN: per slice in 64-row stages, then the
reduce kernel's own order: tn_reduce_kernel and tn_reduce_grouped_kernel slice by slice, tn_reduce_small_kernel and
tn_reduce_into_kernel four interleaved chains combined (0 + 1) + (2 + 3)), the fp32 epilogue as written (GELU from the unrounded fp32 sum;
without a row scale bias2 is folded into bias, with one it is added late), one rounding where the output is 16-bit.
  16-bit outputs   rowerr(kernel) <= ROW_FACTOR rowerr(model)
  fp32 outputs     rowerr(kernel) <= max(ROW_FACTOR rowerr(model), REL_Y_FACTOR Y), Y = the segment error of plain fp32 torch.matmul on
                   the CPU (+ the same fp32 epilogue) against fp64.
  aggregate        `randn`: the kernel_checks bounds (TOL_BF16; 1e-4 fp32 NT / TN; 1e-5 batched fp32; TOL_F32 small kernels), else as the rows.
  derived bound    ELEMENTWISE, always valid, no model:  |c - c64| <= K 2^-23 sum_i |a_i w_i| |rs| + E  (2^-23, not 2^-24: what the
                   MFMA rounds to inside a K = 32 step cannot be checked here), + ulp16 / 2 for a 16-bit output; GELU: 1.13 x that (ulp16 / 2 of u included: g may be taken from the rounded u) + 5.4e-7,
                   GELU' / the other activation forms: 1.13 x that + 1.9e-7 |rs v| (QuickGELU: 2^-21 |g|, rcp and exp at 1 ulp) -- the fit
                   errors of common.h.  E = 2^-22 (|rs| (|acc| + |bias|) + |aux| + |bias2|) covers the at most four fp32 roundings of the
                   epilogue itself: without it the bound is violated by ANY fp32 implementation wherever the bias dominates the product
                   (`hot`: |a w| ~ 2^-12, bias ~ 1).  TN: M in place of K, |gscale| in place of |rs|, E from beta dW.
`DERIVED_ONLY`: fp32 tensors a correct kernel exceeded the factor rule on, to be judged by the derived bound alone.  EMPTY: on MI355X
(fp16 flavour) every fp32 tensor of every case passed the factor rule, so no measured ratio is recorded here.

Guards.  Outputs live in larger buffers (ld = N + 8, GUARD_ROWS pattern rows in front and behind, pattern in the pad columns), dW of
gemm_tn_into has ldw > k_valid with pattern behind n_valid / k_valid; inputs carry INPUT_GUARD behind M rows and K columns (lda = K + 8),
aux / table / bias / rowscale likewise; workspaces are EXACTLY the queried size + WS_TAIL bytes of WS_FILL and pre-filled with WS_FILL
(nobody zeroes the 256-byte "zero page" at the end of the TN workspace: a kernel reading it would show); every TN / grouped case runs
TWICE, bit-identical; gscale and the non-finite flag are part of every TN case (`TN_INF`: an inf in P raises the flag of ITS problem
only); grouped == per-problem bit for bit on whole-256 shapes.
M = 0 (TN): all three kernels guard every load by the slice's row count (gemm_tn_kernel: nsteps <= 0 loads nothing; tn_rt8_pair and
tn8_pair: `rows <= 0` writes the zero partial and returns), so the case is IN: dW = beta dW, dbias = beta dbias.

Dispatch, restated: `nt_names` (launch_nt, nt_skinny_ok, nt_tail_plan, nt8_plan), `tn_plan` / `tn_names` (pvrl_gemm_tn_plan_splits,
tn_use_rt, tn_use_tn8, the reduce choice of gemm_tn_impl), `group_plan`, `f32_names` (f32_small_plan, cls_ksplit), `cls_names`; `cus` =
CUs per XCD, lowered by PVRL_COMPUTE_CUS as in common.h.  test_gemm_harness_host.py pins the set of names the tables reach.
The low-CU leg (`low_cu_main`, ONE fresh child process with PVRL_COMPUTE_CUS=4) runs the persistent families where 4 CUs per XCD give
full rounds, ragged tails of both factors and multi-tile walks, and checks both plan queries against the restated plans.
LEFT to the end-to-end checks (kernel_checks.check_gemm_tn_grouped_block_size, e2e_checks): the 2 GiB clause of tn_use_tn8 ((slice rows +
64) x row pitch >= 2^31 bytes: a > 1 GiB operand), the 31-bit byte counts of tile_rsrc / srdA, and grids beyond 2^16 workgroups --
none is reachable below 2e7 outputs.

MEASURED (MI355X, fp16 flavour): tests/test_gemm_gpu.py as a whole -- 402 tests, the child process of the low-CU leg included (4.8 s) --
takes 68 s of wall time; the slowest single test is the 100000 x 384 x 64 case (2.6 s), the fp64 references dominate.
"""
import collections
import functools
import math
import os
import subprocess
import sys

import torch
import torch.nn.functional as F

import pool_attn_checks as pc
from attn_checks import Finding, Guarded, guarded_input, rowerr, agg, judge_tensor, ROW_FACTOR, report  # noqa: F401 (re-exported)
from pool_attn_checks import REL_Y_FACTOR, WS_TAIL, WS_FILL  # noqa: F401
from mvit_pool_checks import ulp16, _gen, _rnd
from procedurevrl_amd._lib import OPERAND

BF = torch.bfloat16 if OPERAND == "bf16" else torch.float16
F32 = torch.float32
REGIMES = ("exact", "k_edge", "randn", "hot", "cancel")
DERIVED_ONLY = set()            # (entry, tensor) names: see the module docstring
GELU_FIT, DGELU_FIT, GELU_SLOPE = 5.4e-7, 1.9e-7, 1.13       # csrc/common.h


def tol16(operand):
    return 1e-2 if operand == torch.bfloat16 else 1.5e-3         # kernel_checks.TOL_BF16


def device_cus():
    """CUs per XCD as pvrl_compute_cus_per_xcd() computes it (no GPU: MI355X's 32)"""
    n = 256
    if torch.cuda.is_available():
        n = torch.cuda.get_device_properties(0).multi_processor_count
        n = n if n >= 8 else 256
    c = n // 8
    e = os.environ.get("PVRL_COMPUTE_CUS", "")
    if e.isdigit() and 0 < int(e) < c:
        c = int(e)
    return c


def cdiv(a, b):
    return -(-a // b)


# =====================================================================================================================
# dispatch, restated
# =====================================================================================================================
EPI_CODE = dict(bf16=0, gelu=1, qgelu=2, resid_f32=3, f32=4, dgelu=5, dqgelu=6, resid_16=7)
# epilogue variants ("x.tab": aux is the fp32 row-modulo table) and what each carries: (bias, rowscale, bias2).  Both forms of bias2
# (folded: no row scale; late: behind it) occur with an fp32 and with a 16-bit output.
EPIS = collections.OrderedDict([
    ("bf16", (1, 1, 0)), ("gelu", (1, 0, 0)), ("qgelu", (1, 0, 0)), ("resid_f32", (1, 1, 1)), ("resid_f32.tab", (1, 0, 1)),
    ("f32", (1, 1, 0)), ("dgelu", (0, 1, 0)), ("dqgelu", (0, 0, 0)), ("resid_16", (1, 0, 1)), ("resid_16.tab", (1, 1, 1))])
F32_OUT = ("resid_f32", "resid_f32.tab", "f32")


def nt_tail_plan(cm, tiles_n, cus):
    T = cm * tiles_n
    full = T // cus * cus
    L, f = T - full, 1
    if L > 0:
        f = 4 if 4 * L <= cus else 2 if 2 * L <= cus else 1
    if f == 1:
        full, L = T, 0
    return full, L, f, full + f * L


def nt8_plan(cm, tiles_n, cus):
    T = cm * tiles_n
    full, L = T, 0
    if T % cus and 2 * (T % cus) <= cus:
        full, L = T // cus * cus, T % cus
    return full, L, full + 2 * L


def _xcd_panels(tiles_m):
    """the distinct panel counts of the 8 XCDs' lists (ceil and floor of tiles_m / 8; 0 = an XCD without work)"""
    qm, rm = tiles_m >> 3, tiles_m & 7
    return sorted({qm + 1, qm} if rm else {qm}, reverse=True)


def nt_names(M, N, K, epi, rowmod, cus):
    """the kernel of launch_nt<EPI> and, for the two 256 x 256 forms, what its per-XCD work lists hold"""
    base = epi.split(".")[0]
    if M <= 192 and K % 256 == 0 and N % 16 == 0:
        return [f"skinny<{cdiv(M, 48)}>" + (".ragged" if M % 16 else "")]
    if N == 768 and 4096 <= M < 20000:
        return ["tile<2,6>.n768"]
    if M >= 4096 and N % 256 == 0:
        tiles_n, tiles_m = N // 256, cdiv(M, 256)
        cms = [cm for cm in _xcd_panels(tiles_m) if cm > 0]
        if K >= 128 and not (base == "resid_16" and rowmod):
            stride = min(nt8_plan(cms[0], tiles_n, cus)[2], cus)
            out = set()
            for cm in cms:
                full, L, _ = nt8_plan(cm, tiles_n, cus)
                out.add("nt8.full_then_half" if full and L else "nt8.half_only" if L else "nt8.full")
                if full > stride:
                    out.add("nt8.walk")
            if (K // 64) & 1:
                out.add("nt8.oddk")
            return sorted(out)
        return sorted({f"tile<4,4>.f{nt_tail_plan(cm, tiles_n, cus)[2]}" for cm in cms})
    if M >= 4096:
        if N % 384 == 0 and M >= 100000:
            return ["tile<2,6>.m100k"]
        if N % 320 == 0:
            return ["tile<2,5>"]
    if M >= 2048 and (N % 256 == 0 or base in ("gelu", "qgelu")):
        return ["tile<4,2>"]
    return ["tile<2,2>"]


def nt_family(kernel):
    k = kernel.split("+")[0]
    return "skinny" if k.startswith("skinny") else "nt8" if k.startswith("nt8") else k.split(".")[0]


def tn_use_rt(N, K):
    return N % 128 == 0 and K % 128 == 0 and N * K >= 256 * 256


def tn_slice_rows(M, splits):
    return cdiv(cdiv(M if M > 0 else 1, splits), 64) * 64


def tn_use_tn8(N, K, slice_rows, ldp, ldq):
    return N % 256 == 0 and K % 256 == 0 and (slice_rows + 64) * max(ldp, ldq) * 2 < (1 << 31) - 4096


def tn_plan(M, N, K, cus):
    """pvrl_gemm_tn_plan_splits"""
    if tn_use_rt(N, K):
        tiles = cdiv(N, 256) * cdiv(K, 256)
        s = 128 if tiles == 1 else 8 * cus // tiles
        return max(1, min(s, M // 64))
    tiles = (N // 128) * (K // 128)
    s = 8 * max(1, cdiv(128, tiles))
    minrows = 2048 if tiles == 1 else 256
    while s > 8 and M // s < minrows:
        s -= 8
    return s


def tn_names(M, N, K, splits, into, has_bias, beta, beta_bias, n_valid=None, k_valid=None, ldw=None, cus=32):
    """the product kernel and the reduce launch(es) of gemm_tn_impl"""
    n_valid, k_valid, ldw = n_valid or N, k_valid or K, ldw or K
    splits = splits or tn_plan(M, N, K, cus)
    if tn_use_rt(N, K):
        kern = "tn8" if tn_use_tn8(N, K, tn_slice_rows(M, splits), N + 8, K + 8) else "tn_rt8"
    else:
        kern = "tn<2,2>"
    if into and (ldw != K or n_valid != N or k_valid != K or beta_bias != beta):
        red = "reduce_into.two_betas" if (beta_bias != beta and has_bias) else "reduce_into.bias" if has_bias else "reduce_into"
    elif N * K // 4 + (N if has_bias else 0) < 64 * 256 and splits >= 8:
        red = "reduce_small"
    else:
        red = "reduce"
    return [kern, red]


def group_plan(shapes, cus):
    """pvrl_gemm_tn_grouped_plan_splits; shapes: [(M, N, K), ...]"""
    T = sum(cdiv(N, 256) * cdiv(K, 256) for _, N, K in shapes)
    smax = min([32] + [max(1, M // 64) for M, _, _ in shapes])
    best, best_eff, ncu = 1, 0.0, 8 * cus
    for s in range(1, smax + 1):
        eff = T * s / (ncu * cdiv(T * s, ncu))
        if eff >= 0.97:
            return s
        if eff > best_eff + 1e-9:
            best, best_eff = s, eff
    return best


def group_names(shapes, splits):
    all8 = all(tn_use_tn8(N, K, tn_slice_rows(M, splits), N + 8, K + 8) for M, N, K in shapes)
    return ["tn8_grouped" if all8 else "tn_rt8_grouped", "reduce_grouped"]


def cls_ksplit(N, K):
    return 4 if (K >= 2048 and K % 1024 == 0 and N // 16 < 128) else 1


def f32_small_plan(M, N, K):
    """-> (splits, kchunk) of f32_small_plan"""
    tiles, splits = cdiv(N, 64) * cdiv(M, 64), 1
    if tiles < 128 and K >= 512:
        splits = max(1, min(256 // tiles, K // 128))
    kchunk = cdiv(cdiv(K, splits), 32) * 32
    return cdiv(K, kchunk), kchunk


def cls_kernel(M, K, ksplit):
    kw = K // ksplit // 8
    return f"MT{1 if M <= 16 else 2 if M <= 32 else 3},KU{6 if kw % 96 == 0 else 2 if kw % 32 == 0 else 1}"


def f32_names(M, N, K):
    """pvrl_gemm_nt_f32_small (lda, ldb multiples of 4 and 16-byte aligned operands, as the harness passes them)"""
    if K % 128 == 0 and cls_ksplit(N, K) == 1:
        return [f"cls_gemm<{cls_kernel(M, K, 1)}>"]
    return ["f32_small.split" if f32_small_plan(M, N, K)[0] > 1 else "f32_small"]


def cls_names(M, N, K, gelu):
    ks = cls_ksplit(N, K)
    return [f"cls_linear<{cls_kernel(M, K, ks)}>" + (f".pass{cdiv(M, 48)}" if M > 48 else "") + (".ksplit4" if ks > 1 else "") +
            (".gelu" if gelu else "")]


# =====================================================================================================================
# NT: cases
# =====================================================================================================================
NtCase = collections.namedtuple("NtCase", "M N K epi rowmod kernel")


def _nt(M, N, K, epi, cus=32):
    rowmod = (7 if M < 100 else 37) if epi.endswith(".tab") else 0
    return NtCase(M, N, K, epi, rowmod, "+".join(nt_names(M, N, K, epi, rowmod, cus)))


def nt_case_id(c):
    return f"nt-{c.M}x{c.N}x{c.K}-{c.epi}-{c.kernel}"


# (shape, family): the FIRST shape of a family runs `exact` with every epilogue and the other regimes with a few; the others run `exact`
# and `k_edge` with three epilogues each (rotating).  Large M = 4096 + 256 j + r, r in {1, 37, 129, 255}.
NT_SHAPES = [
    ((130, 256, 256), "skinny"), ((37, 128, 256), "skinny"), ((96, 128, 512), "skinny"),
    ((300, 128, 64), "tile<2,2>"), ((193, 384, 192), "tile<2,2>"),
    ((2100, 256, 128), "tile<4,2>"), ((2085, 128, 64), "tile<4,2>"),
    ((4133, 640, 64), "tile<2,5>"),
    ((4225, 768, 128), "tile<2,6>"),
    ((4389, 1024, 64), "tile<4,4>"), ((4097, 256, 64), "tile<4,4>"), ((8703, 1024, 64), "tile<4,4>"),
    ((4225, 512, 128), "nt8"), ((4351, 256, 192), "nt8"), ((4133, 1024, 256), "nt8"), ((4097, 2816, 128), "nt8"),
]
NT_HUGE = _nt(100000, 384, 64, "f32")           # the second tile<2,6> condition, F32 only


def _build_nt_tests(shapes, cus=32, regimes=REGIMES):
    tests, seen, rot = [], set(), 0
    names = list(EPIS)
    for (M, N, K), fam in shapes:
        if fam not in seen:
            seen.add(fam)
            for e in names:
                tests.append((_nt(M, N, K, e, cus), "exact"))
            for i, r in enumerate(x for x in regimes if x != "exact"):
                for e in (names[(rot + 3 * i) % 10], names[(rot + 3 * i + 5) % 10]):
                    tests.append((_nt(M, N, K, e, cus), r))
        else:
            for i, r in enumerate(x for x in ("exact", "k_edge") if x in regimes):
                for e in (names[(rot + i) % 10], names[(rot + i + 3) % 10], names[(rot + i + 7) % 10]):
                    tests.append((_nt(M, N, K, e, cus), r))
            if (N, K) == (2816, 128) and "randn" in regimes:
                tests.append((_nt(M, N, K, "gelu", cus), "randn"))
        rot += 1
    return tests


NT_TESTS = _build_nt_tests(NT_SHAPES) + [(NT_HUGE, "exact"), (NT_HUGE, "randn")]
# the persistent families at 4 CUs per XCD (the data-parallel configuration)
LOW_CUS = 4
LOW_NT_SHAPES = [((4230, 512, 128), "nt8"), ((4230, 512, 192), "nt8"), ((4230, 1024, 128), "nt8"),
                 ((4230, 512, 64), "tile<4,4>"), ((8321, 256, 64), "tile<4,4>")]
LOW_NT_TESTS = [(c, r) for c, r in _build_nt_tests(LOW_NT_SHAPES, LOW_CUS, ("exact", "k_edge", "randn"))
                if r != "exact" or c.epi in ("bf16", "gelu", "resid_f32", "f32", "dgelu", "resid_16.tab")]
# batched: 13 problems = two launches; ragged M, differing shapes
BATCH_SHAPES = [(130, 128, 64), (300, 256, 128), (257, 128, 192), (128, 384, 64), (1, 128, 64), (129, 128, 128), (500, 256, 64),
                (255, 128, 256), (64, 256, 192), (383, 128, 64), (100, 128, 128), (256, 256, 64), (131, 384, 128)]
BATCH_EPIS = ("bf16", "f32", "resid_f32")


# =====================================================================================================================
# NT: inputs, reference, model
# =====================================================================================================================
def _edge_cols(K):
    return sorted({c for c in (0, 63, 64, K - 64, K - 1) if 0 <= c < K})


def _hot(n):
    return torch.exp2((torch.arange(n) % 13 - 6).float())


def _tile_mm32(A, B, step):
    """fp32 A B^T accumulated K-tile by K-tile (`step` columns per tile) in tile order"""
    acc = torch.zeros(A.shape[0], B.shape[0])
    for k0 in range(0, A.shape[1], step):
        acc += A[:, k0:k0 + step] @ B[:, k0:k0 + step].t()
    return acc


@functools.lru_cache(maxsize=2)
def nt_core(M, N, K, regime, operand, kstep=64):
    """the operands of a shape x regime and everything every epilogue of it shares: A, W (16-bit-valued fp32; operand None: fp32
    values for the fp32 kernels), c64 = A W^T in fp64, absaw = |A| |W|^T, acc32 = the model's fp32 sum in K-tile order, y32 = plain fp32
    torch.matmul.  Computed once, never modified."""
    g = _gen("nt", M, N, K, regime)
    if regime in ("exact", "k_edge"):
        A = torch.randint(-2, 3, (M, K), generator=g).float()
        W = torch.randint(-2, 3, (N, K), generator=g).float() / 4
        if regime == "k_edge":
            keep = torch.zeros(K)
            keep[_edge_cols(K)] = 1.0
            A = A * keep
    else:
        A = torch.randn(M, K, generator=g)
        W = torch.randn(N, K, generator=g) * 0.05
        if regime == "hot":
            A, W = A * _hot(M)[:, None], W * _hot(N)[:, None]
        elif regime == "cancel":
            h = K // 2
            A[:, h:2 * h] = -A[:, :h] + 2.0 ** -6 * torch.randn(M, h, generator=g)
            W[:, h:2 * h] = W[:, :h]
    if operand is not None:
        A, W = _rnd(A, operand), _rnd(W, operand)
    Ad, Wd = A.double(), W.double()
    return dict(A=A, W=W, c64=Ad @ Wd.t(), absaw=Ad.abs() @ Wd.abs().t(), acc32=_tile_mm32(A, W, kstep), y32=A @ W.t())


def nt_extras(c, regime, operand):
    """bias, bias2 [N], rs [M], aux: fp32 [M, N] / the fp32 table [rowmod, N] / 16-bit-valued [M, N] (residual rows, stored pre-activation)"""
    g = _gen("ntx", c.M, c.N, c.K, c.epi, regime)
    M, N = c.M, c.N
    base = c.epi.split(".")[0]
    has_b, has_rs, has_b2 = EPIS[c.epi]
    rows = c.rowmod if c.rowmod else M
    if regime in ("exact", "k_edge"):
        bias, bias2 = (torch.randint(-4, 5, (N,), generator=g).float() / 4 for _ in range(2))
        rs = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (M,), generator=g)]
        aux = torch.randint(-8, 9, (rows, N), generator=g).float() / 4
    else:
        bias, bias2 = torch.randn(N, generator=g), torch.randn(N, generator=g)
        rs = torch.rand(M, generator=g) + 0.5
        if regime == "hot":
            rs = rs / _hot(M)
        aux = torch.randn(rows, N, generator=g) * (2.0 if base in ("dgelu", "dqgelu") else 1.0)
    if base in ("dgelu", "dqgelu") or c.epi == "resid_16":
        aux = _rnd(aux, operand)
    return dict(bias=bias if has_b else None, bias2=bias2 if has_b2 else None, rs=rs if has_rs else None,
                aux=aux if base not in ("bf16", "gelu", "qgelu", "f32") else None)


def _gelu_grad(u):
    return 0.5 * (1 + torch.erf(u * 0.7071067811865476)) + u * torch.exp(-0.5 * u * u) * 0.3989422804014327


def _act(base, v):
    return F.gelu(v) if base == "gelu" else v * torch.sigmoid(1.702 * v)


def _dact(base, u):
    if base == "dgelu":
        return _gelu_grad(u)
    s = torch.sigmoid(1.702 * u)
    return s * (1 + 1.702 * u * (1 - s))


def nt_epilogue(c, x, acc, defect=None, operand=None):
    """the epilogue of nt_epilogue_at in acc's precision (fp64: the reference; fp32: the model, before the output rounding) ->
    dict(out0[, out1]).  defect: see test_gemm_harness_host.py."""
    dt = acc.dtype
    base = c.epi.split(".")[0]
    z = lambda t: 0.0 if t is None else t.to(dt)
    bias, b2 = z(x["bias"]), x["bias2"]
    rs = 1.0 if x["rs"] is None else x["rs"].to(dt)[:, None]
    if base in ("bf16", "f32"):
        return dict(out0=rs * (acc + bias))
    if base in ("gelu", "qgelu"):
        v = acc + bias
        return dict(out0=v, out1=_act(base, _rnd(v, operand) if defect == "gelu_from_rounded_u" else v))
    if base in ("dgelu", "dqgelu"):
        u = x["aux"].to(dt)
        d = _act("gelu" if base == "dgelu" else "qgelu", u) if defect == "dgelu_from_gelu_table" else _dact(base, u)
        return dict(out0=rs * (acc + bias) * d)
    aux = x["aux"].to(dt)
    if c.rowmod:
        idx = torch.arange(c.M) % c.rowmod
        if defect == "table_row_off_by_one_at_the_wrap":          # row rowmod takes table row 1, not 0 (and every later wrap)
            idx = torch.where((idx == 0) & (torch.arange(c.M) > 0), torch.ones_like(idx), idx)
        aux = aux[idx]
    late = x["rs"] is not None and b2 is not None
    if b2 is not None and not late:
        bias = bias + b2.to(dt)
    out = rs * (acc + bias) + aux
    if late:
        out = out + (rs * b2.to(dt) if defect == "rowscale_on_bias2" else b2.to(dt))
    return dict(out0=out)


def nt_round(c, outs, operand):
    return outs if c.epi in F32_OUT else {k: _rnd(v, operand) for k, v in outs.items()}


def nt_model(c, core, x, operand, acc=None, defect=None):
    """the kernels' rounding model (module docstring); acc: another fp32 accumulation (the variants of the host test)"""
    acc = core["acc32"] if acc is None else acc
    if defect == "bias_after_rounding" and x["bias"] is not None:
        y = dict(x, bias=None)
        o = nt_round(c, nt_epilogue(c, y, acc, operand=operand), operand)
        rs = 1.0 if x["rs"] is None else x["rs"][:, None]
        return {k: v + rs * x["bias"] for k, v in o.items()}
    return nt_round(c, nt_epilogue(c, x, acc, defect, operand), operand)


def nt_derived(c, core, x, ref, operand):
    """the elementwise bound of the module docstring per output -> dict of fp64 tensors"""
    rs = 1.0 if x["rs"] is None else x["rs"].double().abs()[:, None]
    base = c.epi.split(".")[0]
    mag = lambda t: 0.0 if t is None else t.double().abs()
    aux = mag(x["aux"])
    if c.rowmod:
        aux = aux[torch.arange(c.M) % c.rowmod]
    v = core["c64"].abs() + mag(x["bias"])
    acc_b = c.K * 2.0 ** -23 * core["absaw"]
    half = (lambda t, b: 0.0) if c.epi in F32_OUT else (lambda t, b: ulp16(t.abs() + b, operand) / 2)
    if base in ("gelu", "qgelu"):
        bu = acc_b + 2.0 ** -22 * v
        fit = GELU_FIT if base == "gelu" else 2.0 ** -21 * ref["out1"].abs() + 2.0 ** -22 * v
        b0 = bu + half(ref["out0"], bu)
        bg = GELU_SLOPE * b0 + fit + 2.0 ** -22 * v           # (1.13 x the bound of the 16-bit u: the activation may be taken from the rounded u)
        return dict(out0=b0, out1=bg + half(ref["out1"], bg))
    if base in ("dgelu", "dqgelu"):
        b = GELU_SLOPE * (rs * acc_b + 2.0 ** -22 * rs * v) + (DGELU_FIT if base == "dgelu" else 2.0 ** -20) * rs * v
        return dict(out0=b + half(ref["out0"], b))
    b = rs * acc_b + 2.0 ** -22 * (rs * v + (aux if base.startswith("resid") else 0.0) + mag(x["bias2"]))
    return dict(out0=b + half(ref["out0"], b))


# =====================================================================================================================
# verdicts
# =====================================================================================================================
def _seg(t, w=64):
    """[M, N] -> [M, N / w, w]: a row of the judged tensor = (output row, w-column block)"""
    w = w if t.shape[-1] % w == 0 else 16 if t.shape[-1] % 16 == 0 else t.shape[-1]
    return t.reshape(t.shape[0], t.shape[-1] // w, w)


def _loc(flat, S):
    return f"(row {flat // S}, column block {flat % S})"


def judge_exact(name, x, want):
    """bit equality of values (-0 == +0); the first mismatch by (row, column)"""
    bad = ~(x.double() == want.double())
    n = int(bad.sum())
    where = tuple(int(v) for v in bad.nonzero()[0]) if n else None
    rows = int(bad.any(-1).sum()) if n else 0
    return [Finding(name + " EXACT", n == 0, float(n), 0.0, f"{rows} rows differ; first at (row, column) {where}" +
                    (f": got {x[where].item()!r}, want {want[where].item()!r}" if n else ""))]


def judge_derived(name, x, ref, bound):
    err = (x.double() - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    slack = err - bound
    i = int(slack.argmax())
    e, b = err.reshape(-1)[i].item(), (bound + 0 * err).reshape(-1)[i].item()
    return [Finding(name + " elementwise (derived bound)", e <= b, e, b,
                    f"worst entry (row {i // x.shape[-1]}, column {i % x.shape[-1]}); {int((slack > 0).sum())} entries over their bound")]


def judge_f32(name, x, ref, mod, yard, agg_bound):
    """fp32 outputs: rowerr <= max(ROW_FACTOR model, REL_Y_FACTOR Y) per segment; the aggregate alike unless `agg_bound` is given"""
    xs, rs_, ms, ys = _seg(x), _seg(ref), _seg(mod), _seg(yard)
    if ref.abs().max().item() < 1e-10:
        return judge_tensor(None, name, xs, rs_, ms, None, agg_bound, 0.0, where=_loc)
    rk, i = rowerr(xs, rs_)
    rm, ry = rowerr(ms, rs_)[0], rowerr(ys, rs_)[0]
    bound = max(ROW_FACTOR * rm, REL_Y_FACTOR * ry)
    ak, am, ay = agg(x, ref), agg(mod, ref), agg(yard, ref)
    ab = max(ROW_FACTOR * am, REL_Y_FACTOR * ay) if agg_bound is None else agg_bound
    return [Finding(name + " rowerr", rk <= bound, rk, bound, f"model {rm:.3e} (x{rk / max(rm, 1e-300):.2f}), fp32 yardstick {ry:.3e} "
                    f"(x{rk / max(ry, 1e-300):.2f}), worst {_loc(i, xs.shape[1])}"),
            Finding(name + " aggregate L2", ak <= ab, ak, ab, f"model {am:.3e}, yardstick {ay:.3e}")]


def judge_16(name, x, ref, mod, agg_bound):
    return judge_tensor(None, name, _seg(x), _seg(ref), _seg(mod), None, agg_bound, 0.0, where=_loc)


def judge_nt(c, regime, got, core, x, operand, entry="nt"):
    """got: out0[, out1] CPU fp32 [M, N] -> list of Finding"""
    ref = nt_epilogue(c, x, core["c64"])
    mod = nt_model(c, core, x, operand)
    yard = nt_round(c, nt_epilogue(c, x, core["y32"], operand=operand), operand)
    der = nt_derived(c, core, x, ref, operand)
    base = c.epi.split(".")[0]
    f32 = c.epi in F32_OUT
    out = []
    for k in got:
        name = f"{c.epi} {k}"
        exact = regime in ("exact", "k_edge") and not (k == "out1" or base in ("dgelu", "dqgelu"))
        if exact:
            out += judge_exact(name, got[k], ref[k] if f32 else _rnd(ref[k].float(), operand))
            continue
        out += judge_derived(name, got[k], ref[k], der[k])
        if (entry, k) in DERIVED_ONLY:
            continue
        ab = None if regime != "randn" else ((1e-5 if entry == "batched" else 1e-4) if f32 else tol16(operand))
        out += judge_f32(name, got[k], ref[k], mod[k], yard[k], ab) if f32 else judge_16(name, got[k], ref[k], mod[k], ab)
    return out


# =====================================================================================================================
# NT on the GPU
# =====================================================================================================================
def _vec(t, dev):
    return None if t is None else guarded_input(t[None], F32, dev, 0)


def _nt_buffers(c, core, x, dev):
    M, N = c.M, c.N
    base = c.epi.split(".")[0]
    odt = F32 if c.epi in F32_OUT else BF
    b = dict(A=guarded_input(core["A"], BF, dev, 8), W=guarded_input(core["W"], BF, dev, 8), bias=_vec(x["bias"], dev),
             bias2=_vec(x["bias2"], dev), rs=_vec(x["rs"], dev), aux=None,
             out0=Guarded(f"{c.epi} out0", [M], N, odt, 8, device=dev),
             out1=Guarded(f"{c.epi} out1", [M], N, odt, 8, device=dev) if base in ("gelu", "qgelu") else None)
    if x["aux"] is not None:
        b["aux"] = guarded_input(x["aux"], BF if (base in ("dgelu", "dqgelu") or c.epi == "resid_16") else F32, dev, 8)
    return b


def gpu_nt(c, core, x, dev):
    """pvrl_gemm_nt_bf16 -> (outputs as CPU fp32, guard findings)"""
    L_, ptr, stream = pc._abi()
    b = _nt_buffers(c, core, x, dev)
    o1 = b["out1"]
    L_.call("pvrl_gemm_nt_bf16", ptr(b["A"]), c.K + 8, ptr(b["W"]), c.K + 8, c.M, c.N, c.K, EPI_CODE[c.epi.split(".")[0]], ptr(b["bias"]),
            ptr(b["rs"]), ptr(b["aux"]), c.N + 8 if b["aux"] is not None else 0, c.rowmod, ptr(b["out0"].seg(0)), c.N + 8,
            ptr(o1.seg(0)) if o1 else None, c.N + 8 if o1 else 0, ptr(b["bias2"]), stream())
    torch.cuda.synchronize()
    f = b["out0"].check() + (o1.check() if o1 else [])
    got = dict(out0=b["out0"].seg(0).float().cpu())
    if o1:
        got["out1"] = o1.seg(0).float().cpu()
    return got, f


def check_nt_case(c, regime, run=None, operand=None):
    """one case x regime -> list of Finding.  run(c, core, x) -> (outputs, findings): the host test passes a stand-in for the GPU."""
    operand = BF if operand is None else operand
    if run is None:
        dev = torch.device("cuda:0")
        run = lambda c, core, x: gpu_nt(c, core, x, dev)
    core = nt_core(c.M, c.N, c.K, regime, operand)
    x = nt_extras(c, regime, operand)
    got, f = run(c, core, x)
    return f + judge_nt(c, regime, got, core, x, operand)


def check_nt_batched(epi, regime, run=None, operand=None):
    """pvrl_gemm_nt_batched_bf16 over BATCH_SHAPES (13 problems: two launches), each problem judged like a lone NT case"""
    operand = BF if operand is None else operand
    cases = [NtCase(M, N, K, "f32" if epi == "f32" else epi, 0, "batched") for M, N, K in BATCH_SHAPES]
    cores = [nt_core.__wrapped__(c.M, c.N, c.K, regime, operand) for c in cases]
    xs = []
    for c in cases:
        x = nt_extras(c, regime, operand)
        xs.append(dict(x, bias2=None))                              # the batched form has no second bias
    if run is None:
        from procedurevrl_amd._lib import NtProblem
        dev = torch.device("cuda:0")
        L_, ptr, stream = pc._abi()
        arr = (NtProblem * len(cases))()
        bufs = []
        for a, c, core, x in zip(arr, cases, cores, xs):
            b = _nt_buffers(c, core, x, dev)
            bufs.append(b)
            pv = lambda t: None if t is None else t.data_ptr()
            a.A, a.lda, a.W, a.ldw, a.M, a.N, a.K = pv(b["A"]), c.K + 8, pv(b["W"]), c.K + 8, c.M, c.N, c.K
            a.bias, a.rowscale, a.aux, a.aux_ld = pv(b["bias"]), pv(b["rs"]), pv(b["aux"]), c.N + 8 if b["aux"] is not None else 0
            a.out0, a.ld0 = b["out0"].seg(0).data_ptr(), c.N + 8
        import ctypes
        L_.call("pvrl_gemm_nt_batched_bf16", len(cases), ctypes.cast(arr, ctypes.c_void_p), EPI_CODE[epi], stream())
        torch.cuda.synchronize()
        results = [(dict(out0=b["out0"].seg(0).float().cpu()), b["out0"].check()) for b in bufs]
    else:
        results = [run(c, core, x) for c, core, x in zip(cases, cores, xs)]
    out = []
    for i, (c, core, x, (got, f)) in enumerate(zip(cases, cores, xs, results)):
        fs = f + judge_nt(c, regime, got, core, x, operand, entry="batched")
        out += [Finding(f"problem {i} ({c.M}x{c.N}x{c.K}) " + q.tensor, q.ok, q.value, q.bound, q.detail) for q in fs]
    return out


# =====================================================================================================================
# TN
# =====================================================================================================================
TnCase = collections.namedtuple("TnCase", "M N K splits into bias beta beta_bias n_valid k_valid ldw gexp kernel")
# splits: None = planned.  into: pvrl_gemm_tn_into_bf16 with (n_valid, k_valid, ldw).  gexp: gscale = 2^gexp.


def _tn(M, N, K, splits=None, bias=True, beta=0.0, into=None, beta_bias=None, gexp=0, cus=32):
    nv, kv, ldw = into if into else (N, K, K)
    bb = beta if beta_bias is None else beta_bias
    names = tn_names(M, N, K, splits, into is not None, bias, beta, bb, nv, kv, ldw, cus)
    return TnCase(M, N, K, splits, into is not None, bias, beta, bb, nv, kv, ldw, gexp, "+".join(names))


def tn_case_id(c):
    s = "plan" if c.splits is None else f"s{c.splits}"
    into = f"-into{c.n_valid}x{c.k_valid}ld{c.ldw}" if c.into else ""
    return f"tn-{c.M}x{c.N}x{c.K}-{s}{into}-b{c.beta}-bb{c.beta_bias}{'' if c.bias else '-nobias'}-{c.kernel}"


def _build_tn_cases(cus=32):
    c = []
    # tn<2,2>: splits a multiple of 8 (slice s lives on XCD s % 8); 24 slices of 333 rows: 64-row slices, most of them empty
    for i, M in enumerate((0, 1, 63, 64, 65, 333, 1569)):
        c.append(_tn(M, 128, (128, 256)[i % 2], None if i % 2 else 8, bias=i % 3 != 2, beta=(0.0, 0.5, 1.0)[i % 3], gexp=(0, -3, 2)[i % 3], cus=cus))
    c += [_tn(333, 256, 128, 24, beta=1.0, gexp=-3, cus=cus), _tn(1569, 384, 128, None, cus=cus)]
    # tn_rt8: half tiles (N or K = 128 mod 256)
    for i, (M, N, K) in enumerate([(0, 384, 256), (1, 256, 384), (63, 128, 512), (64, 384, 384), (65, 640, 128), (333, 384, 256), (1569, 256, 384)]):
        c.append(_tn(M, N, K, (None, 1, 3)[i % 3], bias=i % 3 != 1, beta=(0.5, 0.0, 1.0)[i % 3], gexp=(-3, 0, 2)[i % 3], cus=cus))
    c += [_tn(333, 384, 256, 7, beta=1.0, cus=cus), _tn(1569, 384, 384, None, beta=0.5, gexp=2, cus=cus)]     # 7 slices of 333 rows: 64 rows each, one empty
    # tn8: whole 256 x 256 tiles
    for i, (M, N, K) in enumerate([(0, 256, 256), (1, 512, 256), (63, 256, 512), (64, 256, 256), (65, 512, 512), (333, 256, 256), (1569, 512, 256)]):
        c.append(_tn(M, N, K, (1, None, 5)[i % 3], bias=i % 3 != 2, beta=(1.0, 0.0, 0.5)[i % 3], gexp=(2, 0, -3)[i % 3], cus=cus))
    c += [_tn(333, 256, 256, 8, beta=0.5, cus=cus), _tn(1569, 256, 512, None, beta=1.0, gexp=-3, cus=cus)]
    # the three reduce_into forms on each product kernel: un-padded destination with ldw > k_valid, two betas, no bias
    for (M, N, K, nv, kv) in [(333, 128, 128, 96, 100), (1569, 384, 256, 288, 255), (333, 256, 256, 192, 193), (65, 256, 512, 256, 441)]:
        sp = 8 if N * K < 65536 else None
        c += [_tn(M, N, K, sp, into=(nv, kv, kv + 3), beta=1.0, gexp=-3, cus=cus),
              _tn(M, N, K, sp, into=(nv, kv, kv + 5), beta=0.5, beta_bias=1.0, cus=cus),
              _tn(M, N, K, sp, bias=False, into=(nv, kv, K + 8), beta=0.0, gexp=2, cus=cus)]
    c.append(_tn(64, 128, 128, 8, into=(128, 128, 128), beta=0.0, beta_bias=1.0, cus=cus))      # `into` only through the second beta
    return c


TN_CASES = _build_tn_cases()


def _build_tn_tests(cases, regimes=REGIMES):
    """every case runs `exact`; the first to reach a (kernel, reduce) pair not seen before runs every regime, the others `k_edge` too"""
    tests, seen = [], set()
    for c in cases:
        regs = ["exact"]
        if c.kernel not in seen and c.M >= 333:
            seen.add(c.kernel)
            regs += [r for r in regimes if r != "exact"]
        elif c.M > 64 and "k_edge" in regimes:
            regs.append("k_edge")
        tests += [(c, r) for r in regs]
    return tests


TN_TESTS = _build_tn_tests(TN_CASES)
LOW_TN_CASES = [_tn(4230, 512, 256, None, beta=0.5, gexp=-3, cus=LOW_CUS), _tn(4230, 384, 256, None, cus=LOW_CUS),
                _tn(4230, 512, 512, 3, bias=False, beta=1.0, cus=LOW_CUS)]
LOW_TN_TESTS = [(c, r) for c in LOW_TN_CASES for r in ("exact", "k_edge", "randn")]

# grouped launches: (list of (M, N, K, bias, beta, gexp), forced splits or None)
GroupCase = collections.namedtuple("GroupCase", "probs splits kernel")


def _group(probs, splits=None, cus=32):
    shapes = [p[:3] for p in probs]
    s = splits or group_plan(shapes, cus)
    return GroupCase(tuple(probs), splits, "+".join(group_names(shapes, s)))


GROUP_CASES = [
    _group([(1569, 512, 256, True, 0.0, 0), (1000, 256, 512, True, 1.0, -3), (333, 256, 256, False, 0.5, 2)]),
    _group([(1569, 256, 256, True, 0.5, 0), (65, 256, 512, True, 0.0, 2)], splits=3),            # 65 rows in 3 slices: two of them empty
    _group([(333, 384, 256, True, 1.0, -3)]),                                                       # one N = 384 problem: the register-transposed grouped kernel
    _group([(1569, 256, 256, True, 0.0, 0), (700, 384, 128, False, 0.5, 2), (64, 128, 384, True, 1.0, 0)], splits=2),
]
LOW_GROUP_CASES = [_group([(4230, 512, 256, True, 0.5, -3), (4230, 256, 512, True, 0.0, 0), (1569, 256, 256, False, 1.0, 2)], cus=LOW_CUS),
                   _group([(4230, 384, 256, True, 0.0, 0), (1000, 256, 256, True, 1.0, 0)], cus=LOW_CUS)]


def group_case_id(c):
    return "group-" + "_".join(f"{M}x{N}x{K}" for M, N, K, *_ in c.probs) + f"-{'plan' if c.splits is None else 's%d' % c.splits}-{c.kernel}"


GROUP_TESTS = [(c, r) for c in GROUP_CASES for r in ("exact", "k_edge", "randn")] + [(GROUP_CASES[0], "hot"), (GROUP_CASES[2], "cancel")]


def tn_edge_rows(M, Ms):
    return sorted({r for r in (0, 63, 64, Ms - 1, Ms, M - 1) if 0 <= r < M})


@functools.lru_cache(maxsize=4)
def tn_core(M, N, K, regime, operand, Ms):
    """P [M, N], Q [M, K] (16-bit-valued) and what every variant of the shape shares: c64 = P^T Q, abspq, colsum64, abscol, y32"""
    g = _gen("tn", M, N, K, regime)
    if regime in ("exact", "k_edge"):
        P = torch.randint(-2, 3, (M, N), generator=g).float()
        Q = torch.randint(-2, 3, (M, K), generator=g).float() / 4
        if regime == "k_edge":
            keep = torch.zeros(M)
            keep[tn_edge_rows(M, Ms)] = 1.0
            P = P * keep[:, None]
    else:
        P = torch.randn(M, N, generator=g)
        Q = torch.randn(M, K, generator=g) * (1.0 if regime == "hot" else 0.05)
        if regime == "hot":
            P, Q = P * _hot(N)[None, :], Q * _hot(K)[None, :] * 0.05
        elif regime == "cancel":
            h = M // 2
            P[h:2 * h] = -P[:h] + 2.0 ** -6 * torch.randn(h, N, generator=g)
            Q[h:2 * h] = Q[:h]
    P, Q = _rnd(P, operand), _rnd(Q, operand)
    Pd, Qd = P.double(), Q.double()
    return dict(P=P, Q=Q, c64=Pd.t() @ Qd, abspq=Pd.abs().t() @ Qd.abs(), col64=Pd.sum(0), abscol=Pd.abs().sum(0), y32=P.t() @ Q,
                ycol=P.sum(0))


def tn_starts(N, K, regime, key):
    """what dW and dbias hold before the call"""
    g = _gen("tn0", N, K, regime, key)
    if regime in ("exact", "k_edge"):
        return torch.randint(-8, 9, (N, K), generator=g).float() / 4, torch.randint(-8, 9, (N,), generator=g).float() / 4
    return torch.randn(N, K, generator=g), torch.randn(N, generator=g)


def tn_partials(P, Q, splits, Ms, defect=None):
    """the product kernels restated: per slice an fp32 sum in 64-row stages -> part [splits, N, K], cpart [splits, N]"""
    M = P.shape[0]
    part = torch.zeros(splits, P.shape[1], Q.shape[1])
    cpart = torch.zeros(splits, P.shape[1])
    for s in range(splits):
        for m0 in range(s * Ms, min(M, (s + 1) * Ms), 64):
            m1 = min(M, (s + 1) * Ms, m0 + 64)
            part[s] += P[m0:m1].t() @ Q[m0:m1]
            cpart[s] += P[m0:m1].sum(0)
    return part, cpart


def _chain4(part):
    """tn_reduce_small_kernel / tn_reduce_into_kernel: chains s = sl, sl + 4, ... combined (0 + 1) + (2 + 3)"""
    a = []
    for sl in range(4):
        t = torch.zeros_like(part[0])
        for s in range(sl, part.shape[0], 4):
            t = t + part[s]
        a.append(t)
    return (a[0] + a[1]) + (a[2] + a[3])


def _chain1(part, zero_start):
    a = torch.zeros_like(part[0]) if zero_start else part[0].clone()
    for s in range(0 if zero_start else 1, part.shape[0]):
        a = a + part[s]
    return a


def tn_reduce(kind, part, cpart, gscale, beta, beta_bias, dW0, db0, reverse=False, defect=None):
    """the reduce kernels restated in fp32 -> (dW, dbias) over the padded N x K (the caller cuts n_valid / k_valid)"""
    if reverse:
        part, cpart = part.flip(0), cpart.flip(0)
    if defect == "one_splits_partial_dropped":
        part = torch.cat((part[:1], part[2:]))
    if defect == "dbias_misses_the_last_slice":
        cpart = cpart[:-1]
    if defect == "beta_bias_takes_beta":
        beta_bias = beta
    if kind in ("reduce", "reduce_grouped"):
        w, b = _chain1(part, False), _chain1(cpart, True)
    else:
        w, b = _chain4(part), _chain4(cpart)
    w, b = w * gscale, b * gscale
    return (w + beta * dW0 if beta != 0 else w), (b + beta_bias * db0 if beta_bias != 0 else b)


def tn_splits(c, cus=None):
    return c.splits or tn_plan(c.M, c.N, c.K, device_cus() if cus is None else cus)


def _pad_start(t0, N, K):
    out = torch.zeros(N, K)
    out[:t0.shape[0], :t0.shape[1]] = t0
    return out


def tn_expect(c, core, starts, splits, operand, reverse=False, defect=None):
    """-> (ref, mod, yard, derived): dicts dW [n_valid, k_valid], dbias [n_valid]"""
    gs = 2.0 ** c.gexp
    nv, kv = c.n_valid, c.k_valid
    w0, b0 = starts
    ref = dict(dW=c.beta * w0.double() + gs * core["c64"][:nv, :kv], dbias=c.beta_bias * b0.double() + gs * core["col64"][:nv])
    part, cpart = tn_partials(core["P"], core["Q"], splits, tn_slice_rows(c.M, splits))
    kind = c.kernel.split("+")[1].split(".")[0]
    mw, mb = tn_reduce(kind, part, cpart, gs, c.beta, c.beta_bias, _pad_start(w0, c.N, c.K), _pad_start(b0[:, None], c.N, 1)[:, 0], reverse, defect)
    mod = dict(dW=mw[:nv, :kv], dbias=mb[:nv])
    yard = dict(dW=(gs * core["y32"])[:nv, :kv] + c.beta * w0, dbias=(gs * core["ycol"])[:nv] + c.beta_bias * b0)
    n = max(c.M, 1)
    der = dict(dW=gs * n * 2.0 ** -23 * core["abspq"][:nv, :kv] + 2.0 ** -22 * (ref["dW"].abs() + c.beta * w0.double().abs()),
               dbias=gs * n * 2.0 ** -23 * core["abscol"][:nv] + 2.0 ** -22 * (ref["dbias"].abs() + c.beta_bias * b0.double().abs()))
    return ref, mod, yard, der


def judge_tn(c, regime, got, core, starts, splits, operand, name=""):
    ref, mod, yard, der = tn_expect(c, core, starts, splits, operand)
    out = []
    keys = ("dW", "dbias") if c.bias else ("dW",)
    for k in keys:
        x, r, m, y, d = (t[k] if t[k].dim() == 2 else t[k][None] for t in (got, ref, mod, yard, der))
        if regime in ("exact", "k_edge"):
            out += judge_exact(name + k, x, r)
            continue
        out += judge_derived(name + k, x, r, d)
        if ("tn", k) not in DERIVED_ONLY:
            out += judge_f32(name + k, x, r, m, y, 1e-4 if regime == "randn" else None)
    return out


def _rows_in(x, dev):
    """guarded_input for the TN operands; M = 0: the guard rows alone (an empty view has no address)"""
    if x.shape[0] == 0:
        return torch.full((4, x.shape[1] + 8), 1000.0).to(dev, BF)
    return guarded_input(x, BF, dev, 8)


def _scalar(v, dev):
    """one fp32 value in front of guard values"""
    t = torch.full((8,), 1000.0, device=dev)
    t[0] = v
    return t


def _tn_outputs(c, starts, dev):
    dW = Guarded("dW", [c.n_valid], c.k_valid, F32, c.ldw - c.k_valid, device=dev)
    dW.seg(0).copy_(starts[0])
    db = None
    if c.bias:
        db = Guarded("dbias", [1], c.n_valid, F32, 0, device=dev)
        db.seg(0).copy_(starts[1][None])
    return dW, db


def gpu_tn(c, core, starts, splits, dev):
    """pvrl_gemm_tn_bf16 / _into_bf16, TWICE -> (outputs of the first run as CPU fp32, findings: guards, workspace tail, plan, flag, repeat)"""
    L_, ptr, stream = pc._abi()
    P, Q = _rows_in(core["P"], dev), _rows_in(core["Q"], dev)
    f = []
    if c.splits is None:
        plan = int(L_.call("pvrl_gemm_tn_plan_splits", c.M, c.N, c.K))
        f.append(Finding("pvrl_gemm_tn_plan_splits == the restated plan", plan == splits, float(plan), float(splits), ""))
        splits = plan
    nbytes = int(L_.call("pvrl_gemm_tn_workspace_bytes", c.N, c.K, splits))
    runs = []
    for rep in range(2):
        ws = pc._workspace(nbytes, dev)
        dW, db = _tn_outputs(c, starts, dev)
        gsc, flag = _scalar(2.0 ** c.gexp, dev), _scalar(0.0, dev)
        if c.into:
            L_.call("pvrl_gemm_tn_into_bf16", ptr(P), c.N + 8, ptr(Q), c.K + 8, c.M, c.N, c.K, splits, c.beta, ptr(dW.seg(0)), c.ldw,
                    c.n_valid, c.k_valid, ptr(db.seg(0)) if db else None, c.beta_bias, ptr(ws), nbytes, ptr(gsc), ptr(flag), stream())
        else:
            L_.call("pvrl_gemm_tn_bf16", ptr(P), c.N + 8, ptr(Q), c.K + 8, c.M, c.N, c.K, splits, c.beta, ptr(dW.seg(0)),
                    ptr(db.seg(0)) if db else None, ptr(ws), nbytes, ptr(gsc), ptr(flag), stream())
        torch.cuda.synchronize()
        fl = flag.cpu()
        ok = fl[0].item() == 0.0 and bool((fl[1:] == 1000.0).all())
        fr = pc._ws_check("tn workspace", ws, nbytes) + dW.check() + (db.check() if db else []) + \
            [Finding("non-finite flag stays 0, its neighbours untouched", ok, fl[0].item(), 0.0, "")]
        f += [q for q in fr if rep == 0 or not q.ok]
        runs.append(dict(dW=dW.seg(0).cpu(), dbias=db.seg(0)[0].cpu() if db else None))
    same = all(runs[0][k] is None or torch.equal(runs[0][k].view(torch.int32), runs[1][k].view(torch.int32)) for k in runs[0])
    f.append(Finding("second run bit-identical", same, 0.0 if same else 1.0, 0.0, ""))
    return runs[0], f, splits


def check_tn_case(c, regime, run=None, operand=None, cus=None):
    operand = BF if operand is None else operand
    splits = tn_splits(c, cus)
    core = tn_core(c.M, c.N, c.K, regime, operand, tn_slice_rows(c.M, splits))
    w0, b0 = tn_starts(c.N, c.K, regime, 0)
    starts = (w0[:c.n_valid, :c.k_valid].contiguous(), b0[:c.n_valid].contiguous())
    if run is None:
        got, f, splits = gpu_tn(c, core, starts, splits, torch.device("cuda:0"))
    else:
        got, f = run(c, core, starts, splits)
    return f + judge_tn(c, regime, got, core, starts, splits, operand)


def _group_cases(g, splits, regime, operand):
    """the problems of a group as TnCase (for the judges), their cores and starts"""
    out = []
    for i, (M, N, K, bias, beta, gexp) in enumerate(g.probs):
        c = TnCase(M, N, K, splits, False, bias, beta, beta, N, K, K, gexp, g.kernel)
        out.append((c, tn_core.__wrapped__(M, N, K, regime, operand, tn_slice_rows(M, splits)), tn_starts(N, K, regime, i)))
    return out


def gpu_group(items, splits, dev, inf_in=None):
    """pvrl_gemm_tn_grouped_bf16 once -> ([outputs], [flags], findings).  inf_in: index of the problem whose P carries an inf"""
    import ctypes
    from procedurevrl_amd._lib import TnProblem
    L_, ptr, stream = pc._abi()
    arr = (TnProblem * len(items))()
    keep = []
    for i, (a, (c, core, starts)) in enumerate(zip(arr, items)):
        Pc = core["P"]
        if inf_in == i:
            Pc = Pc.clone()
            Pc[c.M // 2, 3] = float("inf")
        P, Q = _rows_in(Pc, dev), _rows_in(core["Q"], dev)
        dW, db = _tn_outputs(c, starts, dev)
        gsc, flag = _scalar(2.0 ** c.gexp, dev), _scalar(0.0, dev)
        a.P, a.ldp, a.Q, a.ldq, a.M, a.N, a.K, a.beta = P.data_ptr(), c.N + 8, Q.data_ptr(), c.K + 8, c.M, c.N, c.K, c.beta
        a.dW, a.dbias, a.gscale, a.nonfinite = dW.seg(0).data_ptr(), db.seg(0).data_ptr() if db else None, gsc.data_ptr(), flag.data_ptr()
        keep.append((P, Q, dW, db, gsc, flag))
    ap = ctypes.cast(arr, ctypes.c_void_p)
    nbytes = int(L_.call("pvrl_gemm_tn_grouped_workspace_bytes", len(items), ap, splits))
    ws = pc._workspace(nbytes, dev)
    L_.call("pvrl_gemm_tn_grouped_bf16", len(items), ap, splits, ptr(ws), nbytes, stream())
    torch.cuda.synchronize()
    f = pc._ws_check("grouped workspace", ws, nbytes)
    outs, flags = [], []
    for i, (P, Q, dW, db, gsc, flag) in enumerate(keep):
        if inf_in != i:
            f += dW.check() + (db.check() if db else [])
        outs.append(dict(dW=dW.seg(0).cpu(), dbias=db.seg(0)[0].cpu() if db else None))
        flags.append(flag.cpu())
    return outs, flags, f


def check_group_case(g, regime, run=None, cus=None, operand=None):
    """the grouped launch twice (bit-identical), each problem judged like a lone TN case; whole-256 groups: bit-equal to pvrl_gemm_tn_bf16
    per problem at the same slice count.  run(items, splits) -> [outputs]: the host test's stand-in."""
    cus = device_cus() if cus is None else cus
    shapes = [p[:3] for p in g.probs]
    splits = g.splits or group_plan(shapes, cus)
    operand = BF if operand is None else operand
    items = _group_cases(g, splits, regime, operand)
    f = []
    if run is None:
        import ctypes
        from procedurevrl_amd._lib import TnProblem
        dev = torch.device("cuda:0")
        outs, flags, f = gpu_group(items, splits, dev)
        outs2, _, f2 = gpu_group(items, splits, dev)
        f += [q for q in f2 if not q.ok]
        same = all(o[k] is None or torch.equal(o[k].view(torch.int32), p[k].view(torch.int32)) for o, p in zip(outs, outs2) for k in o)
        f.append(Finding("second grouped run bit-identical", same, 0.0 if same else 1.0, 0.0, ""))
        ok = all(fl[0].item() == 0.0 and bool((fl[1:] == 1000.0).all()) for fl in flags)
        f.append(Finding("non-finite flags stay 0", ok, 0.0 if ok else 1.0, 0.0, ""))
        if g.splits is None:
            L_, ptr, stream = pc._abi()
            arr = (TnProblem * len(items))()
            z = torch.zeros(16, device=dev)
            for a, (M, N, K, *_) in zip(arr, g.probs):
                a.P, a.ldp, a.Q, a.ldq, a.M, a.N, a.K, a.dW = z.data_ptr(), N + 8, z.data_ptr(), K + 8, M, N, K, z.data_ptr()
            plan = int(L_.call("pvrl_gemm_tn_grouped_plan_splits", len(items), ctypes.cast(arr, ctypes.c_void_p)))
            f.append(Finding("pvrl_gemm_tn_grouped_plan_splits == the restated plan", plan == splits, float(plan), float(splits), ""))
        if g.kernel.startswith("tn8_grouped"):
            for i, (c, core, starts) in enumerate(items):
                lone, fl, _ = gpu_tn(c._replace(splits=splits), core, starts, splits, dev)
                f += [q for q in fl if not q.ok]
                eq = all(lone[k] is None or torch.equal(lone[k].view(torch.int32), outs[i][k].view(torch.int32)) for k in lone)
                f.append(Finding(f"problem {i}: grouped == pvrl_gemm_tn_bf16 bit for bit", eq, 0.0 if eq else 1.0, 0.0, ""))
    else:
        outs = run(items, splits)
    for i, ((c, core, starts), got) in enumerate(zip(items, outs)):
        f += judge_tn(c, regime, got, core, starts, splits, operand, name=f"problem {i} ({c.M}x{c.N}x{c.K}) ")
    return f


def check_group_inf():
    """TN_INF: an inf in P of problem 1 of GROUP_CASES[0]: its flag is raised, its dW is not finite; the other problems are EXACT and
    their flags stay 0"""
    g = GROUP_CASES[0]
    splits = g.splits or group_plan([p[:3] for p in g.probs], device_cus())
    items = _group_cases(g, splits, "exact", BF)
    outs, flags, f = gpu_group(items, splits, torch.device("cuda:0"), inf_in=1)
    for i, ((c, core, starts), got) in enumerate(zip(items, outs)):
        if i == 1:
            bad = not bool(torch.isfinite(got["dW"]).all())
            f.append(Finding("problem 1: flag raised", flags[i][0].item() == 1.0, flags[i][0].item(), 1.0, ""))
            f.append(Finding("problem 1: dW carries the inf", bad, 0.0 if bad else 1.0, 0.0, ""))
        else:
            f.append(Finding(f"problem {i}: flag stays 0", flags[i][0].item() == 0.0, flags[i][0].item(), 0.0, ""))
            f += judge_tn(c, "exact", got, core, starts, splits, BF, name=f"problem {i} ")
    return f


# =====================================================================================================================
# the fp32 kernels: pvrl_gemm_nt_f32_small (both arms) and pvrl_cls_linear_f32
# =====================================================================================================================
SmallCase = collections.namedtuple("SmallCase", "entry M N K gelu resid alpha kernel")


def _f32(M, N, K, alpha=1.0):
    return SmallCase("f32_small", M, N, K, False, False, alpha, "+".join(f32_names(M, N, K)))


def _cls(M, N, K, gelu=False, resid=False):
    return SmallCase("cls_linear", M, N, K, gelu, resid, 1.0, "+".join(cls_names(M, N, K, gelu)))


SMALL_CASES = [_f32(5, 40, 32), _f32(33, 100, 96, 0.5), _f32(32, 64, 600, 2.0), _f32(70, 130, 2048), _f32(65, 9, 520, 0.25),
               _f32(5, 512, 768, 2.0), _f32(50, 40, 128), _f32(17, 64, 256, 0.5), _f32(30, 2100, 2048),
               _cls(16, 64, 128), _cls(3, 128, 256, gelu=True), _cls(32, 64, 768, resid=True), _cls(17, 128, 128, gelu=True),
               _cls(50, 64, 256, resid=True), _cls(33, 256, 2048), _cls(100, 64, 2048, gelu=True), _cls(7, 2048, 2048, resid=True)]
SMALL_TESTS = [(c, r) for c in SMALL_CASES for r in REGIMES]


def small_case_id(c):
    return f"{c.entry}-{c.M}x{c.N}x{c.K}{'-gelu' if c.gelu else ''}{'-resid' if c.resid else ''}-a{c.alpha}-{c.kernel}"


def small_extras(c, regime):
    g = _gen("small", c.M, c.N, c.K, c.entry, regime)
    if regime in ("exact", "k_edge"):
        q = lambda *s: torch.randint(-4, 5, s, generator=g).float() / 4
        h = lambda n: torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (n,), generator=g)]
        return dict(bias=q(c.N), rs=h(c.M), bs=h(c.M), aux=q(c.M, c.N))
    return dict(bias=torch.randn(c.N, generator=g), rs=torch.rand(c.M, generator=g) + 0.5, bs=torch.rand(c.M, generator=g) + 0.5,
                aux=torch.randn(c.M, c.N, generator=g))


def small_epilogue(c, x, acc):
    dt = acc.dtype
    s = c.alpha * acc
    if c.gelu:
        u = s + x["bias"].to(dt)
        return dict(out=F.gelu(u), u=u)
    if c.resid:
        return dict(out=(x["rs"].to(dt)[:, None] * s + x["bs"].to(dt)[:, None] * x["bias"].to(dt)) + x["aux"].to(dt))
    return dict(out=s + x["bias"].to(dt))


def small_kstep(c):
    """the columns one fp32 partial sum of the kernel covers: a wave's K / (8 ksplit) in the MFMA kernel, a K chunk of the FMA kernel"""
    if c.kernel.startswith("f32_small"):
        return f32_small_plan(c.M, c.N, c.K)[1]
    return c.K // 8 // (cls_ksplit(c.N, c.K) if c.entry == "cls_linear" else 1)


def judge_small(c, regime, got, core, x, operand):
    ref = small_epilogue(c, x, core["c64"])
    mod = small_epilogue(c, x, core["acc32"])
    yard = small_epilogue(c, x, core["y32"])
    v = abs(c.alpha) * core["c64"].abs() + x["bias"].double().abs()
    e = 2.0 ** -22 * ((x["rs"].double().abs()[:, None] * v + x["aux"].double().abs()) if c.resid else v)
    b = abs(c.alpha) * (x["rs"].double().abs()[:, None] if c.resid else 1.0) * c.K * 2.0 ** -23 * core["absaw"] + e
    out = []
    if regime in ("exact", "k_edge"):
        if not c.gelu:
            return judge_exact("out", got["out"], ref["out"])
        out += judge_exact("out16_pre", got["u16"], _rnd(ref["u"].float(), operand))
    if c.gelu:
        b = GELU_SLOPE * b + 2.0 ** -22 * (1.0 + ref["out"].abs())           # erff of the device library: a few ulp
    out += judge_derived("out", got["out"], ref["out"], b)
    out += judge_f32("out", got["out"], ref["out"], mod["out"], yard["out"], 2e-5 if regime == "randn" else None)
    if got.get("g16") is not None:
        out += judge_derived("out16_act", got["g16"], ref["out"], b + ulp16(ref["out"].abs() + b, operand) / 2)
        if regime not in ("exact", "k_edge"):
            out += judge_derived("out16_pre", got["u16"], ref["u"], b + ulp16(ref["u"].abs() + b, operand) / 2)
    return out


def gpu_small(c, core, x, dev):
    L_, ptr, stream = pc._abi()
    M, N, K = c.M, c.N, c.K
    A, B = guarded_input(core["A"], F32, dev, 8), guarded_input(core["W"], F32, dev, 8)
    bias = _vec(x["bias"], dev)
    out = Guarded("out", [M], N, F32, 8, device=dev)
    f, got = [], {}
    if c.entry == "f32_small":
        nbytes = int(L_.call("pvrl_gemm_nt_f32_small_workspace_bytes", M, N, K))
        ws = pc._workspace(nbytes, dev)
        L_.call("pvrl_gemm_nt_f32_small", ptr(A), K + 8, ptr(B), K + 8, ptr(bias), c.alpha, ptr(out.seg(0)), N + 8, M, N, K,
                ptr(ws) if nbytes else None, nbytes, stream())
    else:
        nbytes = int(L_.call("pvrl_cls_linear_f32_workspace_bytes", M, N, K))
        ws = pc._workspace(nbytes, dev)
        o16 = [Guarded(n, [M], N, BF, 8, device=dev) for n in ("out16_pre", "out16_act")] if c.gelu else None
        rs, bs = (_vec(x[k], dev) if c.resid else None for k in ("rs", "bs"))          # (named: they must outlive the launch)
        aux = guarded_input(x["aux"], F32, dev, 8) if c.resid else None
        L_.call("pvrl_cls_linear_f32", ptr(A), K + 8, ptr(B), K + 8, ptr(bias), M, N, K, int(c.gelu), ptr(rs), ptr(bs), ptr(aux), N + 8,
                ptr(out.seg(0)), N + 8, ptr(o16[0].seg(0)) if o16 else None, ptr(o16[1].seg(0)) if o16 else None, N + 8,
                ptr(ws) if nbytes else None, nbytes, stream())
        if o16:
            torch.cuda.synchronize()
            f += o16[0].check() + o16[1].check()
            got.update(u16=o16[0].seg(0).float().cpu(), g16=o16[1].seg(0).float().cpu())
    torch.cuda.synchronize()
    f += out.check() + pc._ws_check("workspace", ws, nbytes)
    got["out"] = out.seg(0).cpu()
    return got, f


def check_small_case(c, regime, run=None, operand=None):
    operand = BF if operand is None else operand
    core = nt_core(c.M, c.N, c.K, regime, None, small_kstep(c))
    x = small_extras(c, regime)
    if run is None:
        dev = torch.device("cuda:0")
        run = lambda c, core, x: gpu_small(c, core, x, dev)
    got, f = run(c, core, x)
    return f + judge_small(c, regime, got, core, x, operand)


# =====================================================================================================================
# the low-CU leg: runs in a fresh child process with PVRL_COMPUTE_CUS=4 (tests/test_gemm_gpu.py)
# =====================================================================================================================
def low_cu_main():
    """-> exit status: 0 when every finding of the persistent families at LOW_CUS CUs per XCD is ok"""
    cus = device_cus()
    bad = 0

    def verdict(name, findings):
        nonlocal bad
        fails = [f for f in findings if not f.ok]
        bad += len(fails)
        print(f"== {name}: {len(findings)} findings, {len(fails)} failed" + ("\n" + report(fails) if fails else ""), flush=True)
    verdict("PVRL_COMPUTE_CUS took effect", [Finding("CUs per XCD", cus == LOW_CUS, float(cus), float(LOW_CUS), "")])
    if cus != LOW_CUS:
        return 1
    for c, r in LOW_NT_TESTS:
        verdict(f"{nt_case_id(c)}-{r}", check_nt_case(c, r))
    for c, r in LOW_TN_TESTS:
        verdict(f"{tn_case_id(c)}-{r}", check_tn_case(c, r))
    for g in LOW_GROUP_CASES:
        for r in ("exact", "randn"):
            verdict(f"{group_case_id(g)}-{r}", check_group_case(g, r))
    return 1 if bad else 0


def run_low_cu_child(timeout=600):
    """ONE fresh child process with PVRL_COMPUTE_CUS=4 -> (status, output)"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = (f"import sys; sys.path[:0] = [{os.path.dirname(here)!r}, {here!r}]; import gemm_checks; sys.exit(gemm_checks.low_cu_main())")
    env = dict(os.environ, PVRL_COMPUTE_CUS=str(LOW_CUS))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    return r.returncode, r.stdout
