"""The long-sequence attention harness (tests/attn_long_checks.py) tested without a GPU.

  - the tolerance rule inherited from tests/attn_checks.py is FAIR to a correct streamed kernel: `model_online` -- tile order, P rounded
    against the running maximum, fp32 rescale of l and the accumulator -- stays within ROW_FACTOR of oracle/rounded_oracle.AttnMFMA
    (which knows nothing of tiles) in every regime, at one ragged second tile (S = 65) and at a ragged eighth (S = 450);
  - the rule BITES on an online softmax: a stale factor on l, an unmasked ragged tile and one P.V tile left unscaled each fail it;
  - the attention dispatch of the undivided schemes is pinned at 416 / 417; the regimes do to the scores what their names say.
"""
import pytest
import torch

import attn_checks as ac
import attn_long_checks as alc
from procedurevrl_amd import ops

OPERANDS = [torch.float16, torch.bfloat16]


@pytest.mark.parametrize("operand", OPERANDS, ids=["fp16", "bf16"])
@pytest.mark.parametrize("S", [65, 450])
@pytest.mark.parametrize("regime", alc.REGIMES)
def test_a_correct_streamed_kernel_passes(regime, S, operand):
    findings = alc.judge_host(alc._long(0, 3, S, 2), regime, operand)
    assert all(f.ok for f in findings), ac.report(findings)


@pytest.mark.parametrize("operand", OPERANDS, ids=["fp16", "bf16"])
def test_a_correct_streamed_kernel_passes_with_a_shared_cls_row_and_the_odd_scale(operand):
    for regime in ("randn", "ramp", "late_peak", "early_peak"):
        findings = alc.judge_host(alc._long(1, 4, 130, 2, T=2, scale=ac.ODD_SCALE), regime, operand)
        assert all(f.ok for f in findings), ac.report(findings)


# defect -> the regimes in which the rule must see it (S = 450: seven full key tiles and a ragged eighth of two keys).  (`unmasked` is
# invisible where the true scores of the last keys are far below the maximum anyway and near the zero the padding scores: ramp_rev.)
DEFECTS = {"stale_l": ("ramp", "late_peak"), "unmasked": ("randn", "hot"), "unscaled_pv": ("ramp", "late_peak")}


@pytest.mark.parametrize("operand", OPERANDS, ids=["fp16", "bf16"])
@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_planted_defect_fails_the_rule(defect, operand):
    for regime in DEFECTS[defect]:
        findings = alc.judge_host(alc._long(0, 3, 450, 2), regime, operand, defect=defect)
        fwd = [f for f in findings if f.tensor.startswith(("o ", "lse"))]
        assert any(not f.ok for f in fwd), f"{defect} went unnoticed in `{regime}`:\n" + ac.report(findings)


def test_dispatch_is_pinned_at_416():
    assert ops.ATTN_MAX_S == 416
    assert not ops.attn_uses_long(1) and not ops.attn_uses_long(416)
    assert ops.attn_uses_long(417) and ops.attn_uses_long(alc.MAX_S)
    assert (alc.KT, alc.QT, alc.MAX_S) == (ops.ATTN_LONG_KT, ops.ATTN_LONG_QT, ops.ATTN_LONG_MAX_S)
    assert alc.QT % 16 == 0 and alc.KT % 32 == 0 and alc.MAX_S == 8192


def test_regimes_do_what_they_say():
    c = alc._long(1, 4, 450, 2, T=2)
    items = ac.choose_items(c)
    for regime in alc.NEW_REGIMES:
        q, k, v, do, _ = ac.gathered_inputs(c, alc.make_problem(c, regime, torch.float16), items)
        s = (q.double() @ k.double().transpose(-1, -2)) * c.scale
        tile_max = torch.stack([s[..., j:j + alc.KT].amax(-1) for j in range(0, c.S, alc.KT)], -1)       # [items, S, tiles]
        if regime == "ramp":            # every full key tile raises every query's running maximum (the ragged one holds two keys)
            assert (tile_max[..., 1:-1] > tile_max[..., :-2]).all() and (tile_max[..., -1] > tile_max[..., -3]).all()
        elif regime == "ramp_rev":
            assert (tile_max[..., 1:] < tile_max[..., :-1]).all()
        else:
            peak = c.S - 1 if regime == "late_peak" else 0
            rest = torch.cat([s[..., :peak], s[..., peak + 1:]], -1).amax(-1)
            assert (s[..., peak] - rest).min().item() >= 30.0
    ids = [f"{alc.case_id(c)}-{r}" for c, r in alc.TESTS]
    assert len(set(ids)) == len(ids)


def test_case_table_holds_the_issue_s_cases():
    have = {(c.mode, c.nseq, c.S, c.H, c.T) for c, _ in alc.TESTS}
    for S in (1, alc.KT - 1, alc.KT, alc.KT + 1, 2 * alc.KT + 1, alc.QT + 1, 417, 513):
        assert (0, 3, S, 2, 1) in have
    assert {(0, 2, 785, 12, 1), (1, 2, 1569, 2, 1), (1, 3, 513, 12, 1), (1, 4, 450, 2, 2), (0, 1, 6273, 1, 1)} <= have
    assert [r for c, r in alc.TESTS if c.S == 6273] == ["randn"]
    for c in {c for c, _ in alc.TESTS if c.S != 6273}:
        assert set(alc.NEW_REGIMES) <= {r for cc, r in alc.TESTS if cc == c} or c.ldd_extra == 4
    assert any(c.scale == ac.ODD_SCALE for c, _ in alc.TESTS) and any(c.ldd_extra == 4 for c, _ in alc.TESTS)
