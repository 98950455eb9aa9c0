"""The long-sequence attention kernels (pvrl_attn_long_fwd / _bwd) against an fp64 reference, row by row, under the tolerance rule of
tests/attn_checks.py, on its softmax regimes and on three aimed at the online rescale, inside guard bands (tests/attn_long_checks.py;
pytest -m gpu).  One test per case x input regime."""
import pytest

import attn_checks as ac
import attn_long_checks as alc


def _verdict(name, findings):
    print(f"\n== {name}\n{ac.report(findings)}")
    bad = [f for f in findings if not f.ok]
    assert not bad, f"{name}\n" + ac.report(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("case,regime", alc.TESTS, ids=[f"{alc.case_id(c)}-{r}" for c, r in alc.TESTS])
def test_attn_long(case, regime):
    _verdict(f"{alc.case_id(case)}-{regime}", alc.check_case(case, regime))


@pytest.mark.gpu
@pytest.mark.parametrize("case,regime", alc.SHORT_TOO, ids=[f"{alc.case_id(c)}-{r}" for c, r in alc.SHORT_TOO])
def test_attn_long_agrees_with_the_short_kernels(case, regime):
    _verdict(f"{alc.case_id(case)}-{regime} vs pvrl_attn_fwd / _bwd", alc.check_against_short(case, regime))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [alc._long(1, 3, 513, 12), alc._long(0, 3, alc.QT + 1, 2, ldd_extra=4)], ids=alc.case_id)
def test_attn_long_backward_is_bit_equal_from_run_to_run(case):
    _verdict(alc.case_id(case), alc.check_backward_twice(case))


@pytest.mark.gpu
def test_attn_long_refuses_s_0_and_s_above_the_limit():
    _verdict("refusals", alc.check_refusals())
