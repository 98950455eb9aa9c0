"""The MViTv2 pooling-operator kernels of csrc/mvit.hip -- attention_pool, the max-pool skip, im2col and the any-width LayerNorm -- and the
split-row LayerNorm of csrc/norm.hip against an fp64 reference, token by token, on hard inputs, through every dispatch path, inside guard bands (tests/mvit_pool_checks.py;
pytest -m gpu).  One test per case x input regime; the id names the shape, the kernel instantiations the case reaches, and the regime."""
import pytest

import mvit_pool_checks as mc


def _verdict(name, findings):
    print(f"\n== {name}\n{mc.report(findings)}")
    bad = [f for f in findings if not f.ok]
    assert not bad, name + "\n" + mc.report(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("case,regime", mc.POOL_TESTS, ids=[f"{mc.pool_case_id(c)}-{r}" for c, r in mc.POOL_TESTS])
def test_attention_pool(case, regime):
    _verdict(f"{mc.pool_case_id(case)}-{regime}", mc.check_pool_case(case, regime))


@pytest.mark.gpu
@pytest.mark.parametrize("case", mc.TAP_CASES, ids=[mc.pool_case_id(c) for c in mc.TAP_CASES])
def test_attention_pool_exact_tap_map(case):
    _verdict("taps " + mc.pool_case_id(case), mc.check_tap_map(case))


@pytest.mark.gpu
@pytest.mark.parametrize("case,regime", mc.MAXPOOL_TESTS, ids=[f"{mc.maxpool_case_id(c)}-{r}" for c, r in mc.MAXPOOL_TESTS])
def test_maxpool_skip(case, regime):
    _verdict(f"{mc.maxpool_case_id(case)}-{regime}", mc.check_maxpool_case(case, regime))


@pytest.mark.gpu
@pytest.mark.parametrize("case", mc.IM2COL_CASES, ids=[mc.im2col_case_id(c) for c in mc.IM2COL_CASES])
def test_im2col(case):
    _verdict(mc.im2col_case_id(case), mc.check_im2col_case(case))


@pytest.mark.gpu
@pytest.mark.parametrize("case,regime", mc.LN_TESTS, ids=[f"{mc.ln_case_id(c)}-{r}" for c, r in mc.LN_TESTS])
def test_layernorm_g(case, regime):
    _verdict(f"{mc.ln_case_id(case)}-{regime}", mc.check_ln_case(case, regime))


@pytest.mark.gpu
@pytest.mark.parametrize("case,regime", mc.NORM_TESTS, ids=[f"{mc.norm_case_id(c)}-{r}" for c, r in mc.NORM_TESTS])
def test_layernorm_split_rows(case, regime):
    _verdict(f"{mc.norm_case_id(case)}-{regime}", mc.check_norm_case(case, regime))


@pytest.mark.gpu
def test_invalid_geometries_leading_dimensions_and_short_workspaces_are_refused():
    findings = mc.check_refusals()
    print("\n" + mc.report(findings))
    assert all(f.ok for f in findings), mc.report(findings)
