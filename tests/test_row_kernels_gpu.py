"""LayerNorm (csrc/norm.hip), the loss head (csrc/loss.hip) and the row helpers of csrc/elementwise.hip against an fp64 reference, row by
row, on hard inputs, at every size where a kernel takes another path, inside guard bands (tests/row_checks.py; pytest -m gpu).  One test
per case x input regime; the id names the entry point, the shape and the path the case is meant to reach."""
import pytest

import row_checks as rc


def _verdict(name, findings):
    print(f"\n== {name}  [library flavour: {rc.OPERAND} operands]\n{rc.report(findings)}")
    bad = [f for f in findings if not f.ok]
    assert not bad, name + "\n" + rc.report(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("case,regime,dy_regime", rc.LN_TESTS, ids=[rc.ln_test_id(t) for t in rc.LN_TESTS])
def test_layernorm(case, regime, dy_regime):
    _verdict(rc.ln_test_id((case, regime, dy_regime)), rc.check_ln_case(case, regime, dy_regime))


@pytest.mark.gpu
def test_layernorm_bwd_reduce_batched_73_items_equal_the_immediate_form():
    _verdict("layernorm_bwd_reduce_batched-73_items", rc.check_ln_reduce_batched())


@pytest.mark.gpu
def test_layernorm_bwd_gscale_and_nonfinite_flag():
    _verdict("layernorm_bwd-gscale-nonfinite", rc.check_ln_nonfinite())


@pytest.mark.gpu
@pytest.mark.parametrize("case,regime", rc.KL_TESTS, ids=[f"{rc.kl_case_id(c)}-{r}" for c, r in rc.KL_TESTS])
def test_kl_topk(case, regime):
    _verdict(f"{rc.kl_case_id(case)}-{regime}", rc.check_kl_case(case, regime))


@pytest.mark.gpu
def test_kl_topk_staged_and_unstaged_give_the_same_bits():
    _verdict("kl_topk-K12288_of_12289-staged_against_unstaged", rc.check_kl_staged_against_unstaged())


@pytest.mark.gpu
def test_kl_topk_refuses_topk_above_8_and_an_empty_row():
    _verdict("kl_topk-refusals", rc.check_kl_refusals())


@pytest.mark.gpu
@pytest.mark.parametrize("case", rc.CE_TESTS, ids=[rc.ce_case_id(c) for c in rc.CE_TESTS])
def test_soft_ce(case):
    _verdict(rc.ce_case_id(case), rc.check_ce_case(case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", rc.SIMPLE_CASES, ids=[rc.simple_case_id(c) for c in rc.SIMPLE_CASES])
def test_loss_kernels_and_row_helpers(case):
    _verdict(rc.simple_case_id(case), rc.check_simple_case(case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", rc.EXACT_CASES, ids=[rc.exact_case_id(c) for c in rc.EXACT_CASES])
def test_bit_exact_helpers(case):
    _verdict(rc.exact_case_id(case), rc.check_exact_case(case))
