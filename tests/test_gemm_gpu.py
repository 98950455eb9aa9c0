"""The GEMM kernels (csrc/gemm_nt*.h/.hip, gemm_tn*.h/.hip, cls_chain.hip) against an fp64 reference per (output row, 64-column block), EXACT
where the inputs allow it, through every dispatch path, inside guard bands (tests/gemm_checks.py; pytest -m gpu).  One test per case x
input regime; the id names the shape, the epilogue, the kernel instantiation(s) the case reaches and the regime.

MEASURED on MI355X (fp16 flavour, the built default): the whole file, 402 tests, takes 68 s of wall time (the child process of the low-CU
leg 4.8 s, the 100000 x 384 x 64 case 2.6 s, everything else under 1.6 s a test); the fp64 references dominate.
"""
import pytest

import gemm_checks as gc


def _verdict(name, findings):
    print(f"\n== {name}\n{gc.report(findings)}")
    bad = [f for f in findings if not f.ok]
    assert not bad, name + "\n" + gc.report(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("case,regime", gc.NT_TESTS, ids=[f"{gc.nt_case_id(c)}-{r}" for c, r in gc.NT_TESTS])
def test_gemm_nt(case, regime):
    _verdict(f"{gc.nt_case_id(case)}-{regime}", gc.check_nt_case(case, regime))


@pytest.mark.gpu
@pytest.mark.parametrize("regime", gc.REGIMES)
@pytest.mark.parametrize("epi", gc.BATCH_EPIS)
def test_gemm_nt_batched_thirteen_problems_two_launches(epi, regime):
    _verdict(f"batched-{epi}-{regime}", gc.check_nt_batched(epi, regime))


@pytest.mark.gpu
@pytest.mark.parametrize("case,regime", gc.TN_TESTS, ids=[f"{gc.tn_case_id(c)}-{r}" for c, r in gc.TN_TESTS])
def test_gemm_tn(case, regime):
    _verdict(f"{gc.tn_case_id(case)}-{regime}", gc.check_tn_case(case, regime))


@pytest.mark.gpu
@pytest.mark.parametrize("case,regime", gc.GROUP_TESTS, ids=[f"{gc.group_case_id(c)}-{r}" for c, r in gc.GROUP_TESTS])
def test_gemm_tn_grouped(case, regime):
    _verdict(f"{gc.group_case_id(case)}-{regime}", gc.check_group_case(case, regime))


@pytest.mark.gpu
def test_gemm_tn_grouped_an_inf_in_one_problem_raises_only_its_flag():
    _verdict("grouped inf", gc.check_group_inf())


@pytest.mark.gpu
@pytest.mark.parametrize("case,regime", gc.SMALL_TESTS, ids=[f"{gc.small_case_id(c)}-{r}" for c, r in gc.SMALL_TESTS])
def test_fp32_small_gemm_and_cls_linear(case, regime):
    _verdict(f"{gc.small_case_id(case)}-{regime}", gc.check_small_case(case, regime))


@pytest.mark.gpu
def test_persistent_kernels_with_four_compute_cus_per_xcd():
    """one fresh child process with PVRL_COMPUTE_CUS=4 (the data-parallel configuration): nt8, tile<4,4>, tn8 / tn_rt8 and the grouped
    launches where 4 CUs give full rounds, ragged tails of both factors and multi-tile walks; both plan queries against the restated plans"""
    status, out = gc.run_low_cu_child()
    print(out)
    assert status == 0, f"the child ended with status {status}\n{out[-4000:]}"
