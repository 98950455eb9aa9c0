"""The attention test harness (tests/attn_checks.py) tested without a GPU: the rounding model stands in for the kernel.

  - the tolerance rule is PASSABLE by something that is not the kernels' model: another legitimate implementation of the same contract
    (attn_checks.model_variant) stays within it in every input regime;
  - the rule BITES: local defects planted into the model's outputs at the suite's largest spatial shape (88 sequences x 12 heads x 197
    tokens) all fail it, while the aggregate relative L2 norm the older checks use lets them through -- the reason this harness exists;
  - a wrong lse entry, a write outside the owned rows and an unwritten owned row are each reported.
"""
import pytest
import torch

import attn_checks as ac
from oracle import rounded_oracle as rorc

TENSORS = ("o", "dq", "dk", "dv")


def _solve(c, regime, operand, items=None):
    prob = ac.make_problem(c, regime, operand)
    items = ac.choose_items(c) if items is None else items
    q, k, v, do, mask = ac.gathered_inputs(c, prob, items)
    ref = ac.reference(q, k, v, do, c.scale, mask)
    mod = ac.model(q, k, v, do, c.scale, mask, operand)
    return items, (q, k, v, do), mask, ref, mod


@pytest.mark.parametrize("operand", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("S", [32, 77, 197])
@pytest.mark.parametrize("regime", ac.REGIMES)
def test_another_implementation_of_the_contract_passes(regime, S, operand):
    c = ac._attn(0, 4, S, 3, causal=regime == "one_live", pad=regime == "one_live")
    items, inp, mask, ref, mod = _solve(c, regime, operand)
    var = ac.model_variant(*inp, c.scale, mask, operand)
    findings = ac.judge(c, regime, dict(var, lse=ref["lse32"]), ref, mod, items, inp, operand)
    assert all(f.ok for f in findings), ac.report(findings)


# --- planted defects at 88 x 12 x 197 ---------------------------------------------------------------------------------
BIG = ac._attn(1, 88, 197, 12, T=8)
H, S = BIG.H, BIG.S


def _zero_row(x):
    x[(37 * H + 5), 60] = 0.0


def _item_times(f):
    def go(x):
        x[(51 * H + 7)] *= f
    return go


def _swap_heads(x):
    a, b = 20 * H + 3, 20 * H + 9
    x[[a, b], 100] = x[[b, a], 100]


def _last_row_of_neighbour(x):
    x[(87 * H + 11), S - 1] = x[(86 * H + 11), S - 1]


DEFECTS = [("one output row zeroed", _zero_row, True), ("one (sequence, head) item scaled by 1.10", _item_times(1.10), True),
           ("one item scaled by 1.01", _item_times(1.01), True), ("row 100 of two heads swapped", _swap_heads, True),
           ("last row taken from the neighbouring sequence", _last_row_of_neighbour, False)]


@pytest.fixture(scope="module")
def big():
    items = torch.arange(BIG.nseq * BIG.H)
    _, inp, mask, ref, mod = _solve(BIG, "randn", torch.float16, items)
    return items, ref, mod


def test_the_model_itself_is_far_inside_the_old_bounds(big):
    """the honest error at this shape: 2e-4 .. 3e-4 aggregate, so the flat 1.5e-2 backward bound is ~50x the rounding noise"""
    items, ref, mod = big
    for t in TENSORS:
        assert ac.agg(mod[t], ref[t]) < 5e-4, t


@pytest.mark.parametrize("defect", DEFECTS, ids=[d[0].replace(" ", "_") for d in DEFECTS])
def test_planted_defect_fails_the_row_rule(big, defect):
    name, plant, old_bound_passes = defect
    items, ref, mod = big
    for t in TENSORS:
        x = mod[t].clone()
        plant(x)
        row = ac.judge_tensor(BIG, t, x, ref[t], mod[t], items, ac.AGG_BWD)[0]
        assert not row.ok, f"{name} in {t} went unnoticed: {ac.report([row])}"
        if old_bound_passes:        # ... and is invisible to the aggregate norm at the backward checks' bound
            assert ac.agg(x, ref[t]) <= ac.AGG_BWD, (name, t, ac.agg(x, ref[t]))


def test_wrong_lse_entry_fails():
    c = ac._attn(0, 4, 77, 3)
    items, inp, mask, ref, mod = _solve(c, "peaked", torch.float16)
    lse = ref["lse32"].clone()
    assert ac.judge_lse(c, lse, ref, items)[0].ok
    lse[5, 40] += 1e-3
    f = ac.judge_lse(c, lse, ref, items)[0]
    assert not f.ok and "token 40" in f.detail, ac.report([f])
    lse[5, 40] = float("nan")
    assert not ac.judge_lse(c, lse, ref, items)[0].ok


def test_guard_band_violation_and_unwritten_row_fail():
    def fresh():
        g = ac.Guarded("dqkv", [10, 3], 16, torch.float16, extra_cols=8, unowned=[(0, 8, 10, 0, 16)])
        g.seg(0)[:8] = 1.0
        g.seg(1)[:] = 2.0
        return g
    assert all(f.ok for f in fresh().check())
    g = fresh()
    g.buf[ac.GUARD_ROWS + 10, 0] = 1.0                  # the first element past the end of segment 0
    assert [f.ok for f in g.check()] == [False, True]
    g = fresh()
    g.seg(0)[3, 15] = 1.0                                # (the last owned column: fine)
    g.buf[ac.GUARD_ROWS + 3, 16] = 1.0                  # the first extra column
    assert [f.ok for f in g.check()] == [False, True]
    g = fresh()
    g.seg(0)[9, 2] = 5.0                                # a row the header declares untouched
    assert [f.ok for f in g.check()] == [False, True]
    g = fresh()
    g.seg(1)[1] = float("nan")                          # an owned row that was never written
    assert [f.ok for f in g.check()] == [True, False]
    for dt in (torch.float16, torch.bfloat16, torch.float32):      # the pattern is a finite number in every element type
        assert torch.isfinite(ac.Guarded("x", [1], 4, dt).buf[0].float()).all()


def test_input_guard_rows_hold_large_values():
    x = torch.zeros(5, 16)
    v = ac.guarded_input(x, torch.float16, "cpu")
    assert v.shape == (5, 16) and v.stride(0) == 24
    full = torch.as_strided(v, (5 + ac.GUARD_ROWS, 24), (24, 1))
    assert (full[5:] == ac.INPUT_GUARD).all() and (full[:, 16:] == ac.INPUT_GUARD).all()


# every instantiation that pvrl_attn_fwd / pvrl_attn_bwd / pvrl_attn_bwd_fused_launch / pvrl_attn_bwd_s32_launch / pvrl_attn_cls_* /
# pvrl_attn_t8_* can launch, written out by hand from the launch_* lines of csrc/attn_mfma.hip (masks stop at S = 208: no _gen beyond <13,8>)
EVERY_KERNEL = """
fwd_1_4 fwd_2_4 fwd_2_4_s32 fwd_3_4 fwd_5_4 fwd_13_8 fwd_13_8_s197 fwd_17_8 fwd_26_8
fwd_1_4_gen fwd_2_4_gen fwd_3_4_gen fwd_5_4_gen fwd_13_8_gen
bwd2p_1_4 bwd2p_2_4 bwd2p_2_4_s32 bwd2p_3_4 bwd2p_5_4 bwd2p_13_8 bwd2p_13_8_s197 bwd2p_17_8 bwd2p_26_8
bwd2p_1_4_gen bwd2p_2_4_gen bwd2p_3_4_gen bwd2p_5_4_gen bwd2p_13_8_gen
fused_0 fused_7 s32 cls_fwd cls_bwd cls_bwd_nodq t8_fwd t8_bwd
""".split()


def test_case_table_reaches_every_instantiation():
    reached = set()
    for c in ac.CASES:
        reached.update(c.kernel.split("+"))
    assert reached == set(EVERY_KERNEL), (sorted(set(EVERY_KERNEL) - reached), sorted(reached - set(EVERY_KERNEL)))
    # every case runs the friendly and the peaked regime; every kernel sees every other regime at least once
    by_kernel = {}
    for c, r in ac.TESTS:
        for k in c.kernel.split("+"):
            by_kernel.setdefault(k, set()).add(r)
    for c in ac.CASES:
        assert {(c, "randn"), (c, "peaked")} <= set(ac.TESTS)
    for k, regs in by_kernel.items():
        assert {"randn", "hot", "peaked", "offset", "equal"} <= regs, (k, regs)
        if k.endswith("_gen"):
            assert "one_live" in regs, k
    ids = [f"{ac.case_id(c)}-{r}" for c, r in ac.TESTS]
    assert len(set(ids)) == len(ids)


def test_large_cases_keep_first_last_and_eight_random_items():
    c = ac._attn(1, 88, 197, 12, T=8)
    items = ac.choose_items(c)
    assert len(items) == 10 and items[0] == 0 and items[-1] == 88 * 12 - 1 and len(set(items.tolist())) == 10
    small = ac._attn(0, 5, 17, 3)
    assert ac.choose_items(small).tolist() == list(range(15))


def test_masked_rounding_model_without_rounding_is_masked_softmax():
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(2, 3, 9, 64, generator=g) for _ in range(3))
    mask = torch.triu(torch.ones(9, 9, dtype=torch.bool), 1)
    assert rorc.OPERAND is None
    want = torch.softmax(((q @ k.transpose(-1, -2)) * 0.125).masked_fill(mask, float("-inf")), -1) @ v
    torch.testing.assert_close(rorc.AttnMFMA.apply(q, k, v, 0.125, mask), want, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(rorc.AttnMFMA.apply(q, k, v, 0.125), torch.softmax((q @ k.transpose(-1, -2)) * 0.125, -1) @ v,
                               rtol=1e-5, atol=1e-6)


def test_small_cases_are_run_on_enough_draws():
    for c in ac.CASES:
        rows = c.nseq * c.H * (1 if c.entry == "cls" else c.S)
        d = ac.n_draws(c)
        assert d == 1 if rows >= ac.MIN_ROWS else (rows * d >= ac.MIN_ROWS or d == 256), c
    tiny = ac.Case("cls", 1, 1, 2, 2, 1, ac.POW2, False, False, 8, True, "cls_fwd+cls_bwd")
    assert ac.n_draws(tiny) == 192
    # the coordinates of a row of a further draw name the draw
    assert ac._where(tiny, torch.tensor([0, 1, 2, 3]), 3, 1) == "(sequence 0, head 1, token 0; draw 1)"
