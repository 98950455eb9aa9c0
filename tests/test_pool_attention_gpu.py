"""The MViTv2 pooling-attention kernels (pvrl_mvit_attn_fwd / _bwd) and the decomposed relative-position kernels (pvrl_mvit_rel_fwd /
_bwd) against an fp64 reference, row by row, on hard softmax inputs, through every dispatch path, inside guard bands, alone and chained
as the engine runs them (tests/pool_attn_checks.py; pytest -m gpu).  One test per case x input regime; the id names the shape, the
kernel instantiations the case is meant to reach, and the regime."""
import pytest

import pool_attn_checks as pc


@pytest.mark.gpu
@pytest.mark.parametrize("case,regime", pc.TESTS, ids=[f"{pc.case_id(c)}-{r}" for c, r in pc.TESTS])
def test_pool_attention(case, regime):
    findings = pc.check_case(case, regime)
    print(f"\n== {pc.case_id(case)}-{regime}\n{pc.report(findings)}")
    bad = [f for f in findings if not f.ok]
    assert not bad, f"{pc.case_id(case)} [{regime}]\n" + pc.report(bad)


@pytest.mark.gpu
def test_invalid_geometries_leading_dimensions_and_short_workspaces_are_refused():
    findings = pc.check_refusals()
    print("\n" + pc.report(findings))
    assert all(f.ok for f in findings), pc.report(findings)
