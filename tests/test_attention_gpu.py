"""The attention kernels (pvrl_attn_fwd / _bwd, pvrl_attn_cls_*, pvrl_attn_t8_*) against an fp64 reference, row by row, on hard softmax
inputs, through every dispatch path, inside guard bands (tests/attn_checks.py; pytest -m gpu).  One test per case x input regime;
the id names the entry point, the shape, the kernel instantiation the case is meant to reach, and the regime."""
import pytest

import attn_checks as ac


@pytest.mark.gpu
@pytest.mark.parametrize("case,regime", ac.TESTS, ids=[f"{ac.case_id(c)}-{r}" for c, r in ac.TESTS])
def test_attention(case, regime):
    findings = ac.check_case(case, regime)
    print(f"\n== {ac.case_id(case)}-{regime}\n{ac.report(findings)}")
    bad = [f for f in findings if not f.ok]
    assert not bad, f"{ac.case_id(case)} [{regime}]\n" + ac.report(bad)


@pytest.mark.gpu
def test_masked_sequences_longer_than_208_are_refused():
    findings = ac.check_masked_too_long()
    assert all(f.ok for f in findings), ac.report(findings)
