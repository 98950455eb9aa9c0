"""PVRL_EPI_GELU_ONLY (include/pvrl.h): out0 = GELU_erf(acc + bias) and no second output -- on every path pvrl_gemm_nt_bf16 dispatches to
(gemm_checks.NT_SHAPES: the few-row kernel, every tile of launch_tile, the persistent 8-wave kernel), the 16 bits PVRL_EPI_GELU writes to
its out1 from the same operands and bias.  The two-output epilogue is judged element by element against the rounding model by the parity
suite (tests/test_gemm_gpu.py) on these shapes; equality to it is the whole check here, within whichever operand type the library was
built for.  Guard rows behind the output and eight guard columns (ld0 = N + 8) must keep their pattern: one allocation covers the ragged
last row tile and the leading dimension.

On the commit before this one pvrl_gemm_nt_bf16 answers code 8 with PVRL_EINVAL."""
import ctypes

import pytest
import torch

import gemm_checks as gc
from gemm_checks import BF, F32, Guarded, guarded_input

DEV = "cuda:0"
CASES = [(shape, fam, regime) for shape, fam in gc.NT_SHAPES for regime in ("randn", "hot")]


def _raw():
    """-> (the ctypes function itself: returns the status instead of raising, lib, ptr, stream)"""
    L, ptr, stream = gc.pc._abi()
    return L._fn["pvrl_gemm_nt_bf16"][0], L, ptr, stream


def _operands(M, N, K, regime):
    core = gc.nt_core(M, N, K, regime, BF)
    bias = gc.nt_extras(gc._nt(M, N, K, "gelu"), regime, BF)["bias"]
    dev = torch.device(DEV)
    return guarded_input(core["A"], BF, dev, 8), guarded_input(core["W"], BF, dev, 8), guarded_input(bias[None], F32, dev, 0)


def _run(fn, ptr, stream, A, W, bias, M, N, K, epi, out0, ld0, out1=None, ld1=0):
    return fn(ptr(A), K + 8, ptr(W), K + 8, M, N, K, epi, ptr(bias), None, None, 0, 0, ptr(out0), ld0,
              ptr(out1) if out1 is not None else None, ld1, None, stream())


@pytest.mark.gpu
@pytest.mark.parametrize("shape,family,regime", CASES, ids=[f"{m}x{n}x{k}-{fam}-{r}" for (m, n, k), fam, r in CASES])
def test_one_output_gelu_equals_the_second_output_of_the_two_output_epilogue(shape, family, regime):
    M, N, K = shape
    fn, L, ptr, stream = _raw()
    # the case runs on the path its family names, with PVRL_EPI_GELU's kernel family (the dispatch the harness models)
    assert gc.nt_family(gc._nt(M, N, K, "gelu").kernel) == family
    A, W, bias = _operands(M, N, K, regime)
    u = Guarded("gelu out0", [M], N, BF, 8, device=DEV)
    g = Guarded("gelu out1", [M], N, BF, 8, device=DEV)
    g1 = Guarded("gelu_only out0", [M], N, BF, 8, device=DEV)
    assert _run(fn, ptr, stream, A, W, bias, M, N, K, L.PVRL_EPI_GELU, u.seg(0), N + 8, g.seg(0), N + 8) == 0
    assert _run(fn, ptr, stream, A, W, bias, M, N, K, L.PVRL_EPI_GELU_ONLY, g1.seg(0), N + 8) == 0      # out1 = nullptr is accepted
    torch.cuda.synchronize()
    bad = [f for f in u.check() + g.check() + g1.check() if not f.ok]
    assert not bad, gc.report(bad)
    want, got = g.seg(0), g1.seg(0)
    assert torch.isfinite(want.float()).all()
    ne = int((want.view(torch.int16) != got.view(torch.int16)).sum())
    print(f"[{M}x{N}x{K} {family} {regime}] differing 16-bit patterns: {ne} of {M * N}")
    assert ne == 0 and torch.equal(got, want)
    assert float(want.float().abs().max()) > 0.0 and not torch.equal(want, u.seg(0))         # (the comparison is not of two blanks)


@pytest.mark.gpu
def test_bad_arguments_are_refused_with_the_outputs_untouched():
    (M, N, K), regime = (300, 128, 64), "randn"
    fn, L, ptr, stream = _raw()
    A, W, bias = _operands(M, N, K, regime)
    out = Guarded("gelu_only out0", [M], N, BF, 8, device=DEV)
    before = out.buf.view(torch.int16).clone()
    assert _run(fn, ptr, stream, A, W, bias, M, N, K, L.PVRL_EPI_GELU_ONLY, out.seg(0), N + 4) == -1       # ld0 % 8 != 0: PVRL_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(out.buf.view(torch.int16), before)
    # the batched entry point takes the plain epilogues only
    from procedurevrl_amd._lib import NtProblem
    prob = (NtProblem * 1)()
    prob[0].A, prob[0].lda, prob[0].W, prob[0].ldw = A.data_ptr(), K + 8, W.data_ptr(), K + 8
    prob[0].M, prob[0].N, prob[0].K = M, N, K
    prob[0].bias, prob[0].out0, prob[0].ld0 = bias.data_ptr(), out.seg(0).data_ptr(), N + 8
    assert L._fn["pvrl_gemm_nt_batched_bf16"][0](1, ctypes.addressof(prob), L.PVRL_EPI_GELU_ONLY, stream()) == -1
    torch.cuda.synchronize()
    assert torch.equal(out.buf.view(torch.int16), before)
    # (and a good call on the same buffers still goes through)
    assert _run(fn, ptr, stream, A, W, bias, M, N, K, L.PVRL_EPI_GELU_ONLY, out.seg(0), N + 8) == 0
    torch.cuda.synchronize()
    assert not [f for f in out.check() if not f.ok]
