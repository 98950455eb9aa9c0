"""The clipping kernels of csrc/optim.hip through the C ABI (harness, reference and the derivation of the two bars: tests/clip_checks.py):
pvrl_sumsq_f32 + pvrl_clip_coef at every size where the pass takes another path and as three runs in one workspace, in six regimes;
their refusals; pvrl_adam_step_clip / pvrl_sgd_step_clip against the entry points without `clip` and against the existing models."""
import pytest

import clip_checks as cc
import optim_checks as oc


def _ok(findings):
    bad = [f for f in findings if not f.ok]
    assert not bad, cc.report(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("ns", cc.CASES, ids=[cc.case_id(ns) for ns in cc.CASES])
@pytest.mark.parametrize("regime", cc.REGIMES)
def test_norm_and_coefficient(ns, regime):
    f = cc.check_case(ns, regime)
    worst = {w: max((x.value for x in f if w in x.tensor and "relative" in x.tensor), default=0.0) for w in ("norm", "coef")}
    print(cc.case_id(ns), regime, "worst relative distance", worst, "bars", cc.NORM_BAR, cc.COEF_BAR)
    _ok(f)


@pytest.mark.gpu
def test_refusals_leave_everything_untouched():
    _ok(cc.check_refusals())


@pytest.mark.gpu
@pytest.mark.parametrize("case", oc.ADAM_CASES, ids=[oc.adam_case_id(c) for c in oc.ADAM_CASES])
def test_adam_step_clip_null_and_one_are_the_plain_step(case):
    _ok(cc.check_null_and_one_equal_plain("adam", case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", oc.SGD_CASES, ids=[oc.sgd_case_id(c) for c in oc.SGD_CASES])
def test_sgd_step_clip_null_and_one_are_the_plain_step(case):
    _ok(cc.check_null_and_one_equal_plain("sgd", case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", oc.ADAM_CASES, ids=[oc.adam_case_id(c) for c in oc.ADAM_CASES])
def test_adam_step_clip_with_a_coefficient(case):
    """*clip = 0.37f: the existing reference and bound for the gradient g * gscale * 0.37, every side condition of the update entries"""
    _ok(oc.check_adam_case(cc.clipped_case(case), run=cc.gpu_adam_clipped(case)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", oc.SGD_CASES, ids=[oc.sgd_case_id(c) for c in oc.SGD_CASES])
def test_sgd_step_clip_with_a_coefficient(case):
    _ok(oc.check_sgd_case(cc.clipped_case(case), run=cc.gpu_sgd_clipped(case)))
