"""The input pipeline and the layout kernels of csrc/elementwise.hip against their kernel-order models, pixel by pixel and bit for bit, on
every path, inside guard bands (tests/input_checks.py; pytest -m gpu).  One test per case; the id names the entry point, the shape and
the path the case reaches."""
import pytest

import input_checks as ic


def _verdict(name, findings):
    print(f"\n== {name}  [library flavour: {ic.OPERAND} operands]\n{ic.report(findings)}")
    bad = [f for f in findings if not f.ok]
    assert not bad, name + "\n" + ic.report(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ic.DEC_CASES, ids=[ic.dec_case_id(c) for c in ic.DEC_CASES])
def test_decoded_clips(case):
    _verdict(ic.dec_case_id(case), ic.check_dec_case(case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ic.PAT_CASES, ids=[ic.pat_case_id(c) for c in ic.PAT_CASES])
def test_patchify(case):
    _verdict(ic.pat_case_id(case), ic.check_pat_case(case))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ic.CT_CASES, ids=[ic.ct_case_id(s) for s in ic.CT_CASES])
def test_cast_transpose(shape):
    _verdict(ic.ct_case_id(shape), ic.check_ct_case(shape))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ic.R1_CASES, ids=[ic.r1_case_id(c) for c in ic.R1_CASES])
def test_rank1_add(case):
    _verdict(ic.r1_case_id(case), ic.check_r1_case(case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ic.BAT_CASES, ids=[ic.bat_case_id(c) for c in ic.BAT_CASES])
def test_batched_forms_equal_the_one_item_entry_points(case):
    _verdict(ic.bat_case_id(case), ic.check_bat_case(case))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ic.CWM_CASES, ids=[ic.cwm_case_id(k) for k in ic.CWM_CASES])
def test_cast_weights_multi(kind):
    _verdict(ic.cwm_case_id(kind), ic.check_cwm_case(kind))


@pytest.mark.gpu
def test_refusals_return_einval_and_write_nothing():
    _verdict("input pipeline and patchify: refusals", ic.check_refusals())


@pytest.mark.gpu
def test_check_decoded_raises_on_device_clips():
    _verdict("ops._check_decoded on device clips", ic.check_decoded_validation("cuda:0"))
