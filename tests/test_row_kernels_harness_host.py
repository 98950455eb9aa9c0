"""The row-kernel harness (tests/row_checks.py) without a GPU: the CPU models stand in for the kernels.  The rule is fair (a second
legitimate fp32 implementation passes it, and the two models' errors stay within ROW_FACTOR / 2 of each other), it bites (every planted
defect fails in the regime named, and the finding names the row), and the case table holds what it claims."""
import pytest
import torch

import row_checks as rc

OPERANDS = (torch.float16, torch.bfloat16)


def _ln_case(kind, **kw):
    """the first case of the table with these fields"""
    table = rc.LN_FWD_CASES if kind == "fwd" else rc.LN_BWD_CASES
    return next(c for c in table if all(getattr(c, k) == v for k, v in kw.items()))


def _ln_stand_in(mode="torch", defect=None):
    def run(c, p):
        ev = rc.ln_fwd_eval if c.kind == "fwd" else rc.ln_bwd_eval
        return ev(p, c, mode, defect), []
    return run


LN_FAIR = [_ln_case("fwd", C=768, R=0, B=5, y16=False, save_stats=True), _ln_case("fwd", C=768, R=13, B=5, y16=False),
           _ln_case("fwd", C=768, R=13, B=5, y16=True), _ln_case("fwd", C=512, R=0, B=77, y16=False), _ln_case("fwd", C=1024, R=9, B=4, y16=False),
           _ln_case("bwd", C=768, R=13, B=1), _ln_case("bwd", C=768, R=2045, B=3, dxs_rows=None), _ln_case("bwd", C=768, R=0, B=2049, dy16=False),
           _ln_case("bwd", C=768, R=8, B=300), _ln_case("bwd", C=768, R=13, B=1, dxs_rows=14), _ln_case("bwd", C=1024, R=4089, B=3),
           _ln_case("bwd", C=512, R=0, B=2048)]
SPREADS = {}


@pytest.mark.parametrize("operand", OPERANDS, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", LN_FAIR, ids=[rc.ln_case_id(c) for c in LN_FAIR])
def test_layernorm_second_model_passes_the_rule(case, operand):
    for regime in rc.LN_REGIMES:
        for dyr in (rc.DY_REGIMES if case.kind == "bwd" and regime in ("randn", "offset") else ("randn",)):
            sp = {}
            f = rc.check_ln_case(case, regime, dyr, run=_ln_stand_in("torch"), operand=operand, spreads=sp)
            bad = [x for x in f if not x.ok]
            assert not bad, f"{regime} / dy {dyr}\n" + rc.report(bad)
            for k, v in sp.items():
                SPREADS.setdefault(k, []).extend(v)
                assert max(v) <= rc.ROW_FACTOR / 2 or k in rc.WIDE, f"{k}: spread {max(v):.2f} in {regime} / dy {dyr}"


def _loss_stand_in(ev, mode="torch", defect=None, keys=None):
    def run(c, p):
        o = ev(p, c, mode, defect)
        return {k: v for k, v in o.items() if not k.startswith("norm") and (keys is None or k in keys)}, []
    return run


KL_FAIR = [(rc._kl(6, 5), "randn"), (rc._kl(257, 8), "hot"), (rc._kl(778, 5), "tie_inside"), (rc._kl(778, 5), "tie_across"),
           (rc._kl(12289, 5), "all_equal"), (rc._kl(9871, 5), "one_thread"), (rc._kl(12288, 0), "randn"), (rc._kl(255, 1), "hot")]


@pytest.mark.parametrize("case,regime", KL_FAIR, ids=[f"{rc.kl_case_id(c)}-{r}" for c, r in KL_FAIR])
def test_kl_topk_second_model_passes_the_rule(case, regime):
    sp = {}
    f = rc.check_kl_case(case, regime, run=_loss_stand_in(rc.kl_eval), spreads=sp)
    bad = [x for x in f if not x.ok]
    assert not bad, rc.report(bad)
    for k, v in sp.items():
        SPREADS.setdefault(k, []).extend(v)
        assert max(v) <= rc.ROW_FACTOR / 2 or k in rc.WIDE, f"{k}: spread {max(v):.2f}"


def test_kl_topk_fp32_and_fp64_references_keep_the_same_entries_under_the_input_conditions():
    """... and not without the second condition: K = 6, topk = 5 at teacher x 40 underflows a kept probability in fp32"""
    for c, regime in rc.KL_TESTS:
        p = rc.make_kl_problem(c, regime)
        cond = rc.kl_input_conditions(p, c)
        assert all(x.ok for x in cond), rc.kl_case_id(c) + " " + regime + "\n" + rc.report(cond)
        a, b = rc.kl_eval(p, c, "ref")["target"], rc.kl_eval(p, c, "torch")["target"]
        assert torch.equal(a > 0, b > 0), rc.kl_case_id(c) + " " + regime
    c = rc._kl(6, 5)
    found = False
    for d in range(64):
        p = rc.make_kl_problem(c, "randn", d)
        p["teacher"] = p["teacher"] * 10.0                # N(0, 40^2)
        if not all(x.ok for x in rc.kl_input_conditions(p, c)):
            found = found or not torch.equal(rc.kl_eval(p, c, "ref")["target"] > 0, rc.kl_eval(p, c, "torch")["target"] > 0)
    assert found


@pytest.mark.parametrize("case", rc.CE_TESTS[:8], ids=[rc.ce_case_id(c) for c in rc.CE_TESTS[:8]])
def test_soft_ce_second_model_passes_the_rule(case):
    sp = {}
    f = rc.check_ce_case(case, run=_loss_stand_in(rc.ce_eval, keys=("row_loss", "dx") if case.dx else ("row_loss",)), spreads=sp)
    bad = [x for x in f if not x.ok]
    assert not bad, rc.report(bad)
    for k, v in sp.items():
        SPREADS.setdefault(k, []).extend(v)
        assert max(v) <= rc.ROW_FACTOR / 2 or k in rc.WIDE, f"{k}: spread {max(v):.2f}"


SIMPLE_FAIR = [c for c in rc.SIMPLE_CASES if not c.path.startswith("past_the") and not (c.entry == "batch_sum" and c.shape[1] > 100)]


@pytest.mark.parametrize("case", SIMPLE_FAIR, ids=[rc.simple_case_id(c) for c in SIMPLE_FAIR])
def test_helper_second_model_passes_the_rule(case):
    E = rc.SIMPLE[case.entry]
    sp = {}
    f = rc.check_simple_case(case, run=lambda c, p: ({k: v for k, v in E["ev"](p, c, "torch").items() if not k.startswith("norm")}, []), spreads=sp)
    bad = [x for x in f if not x.ok]
    assert not bad, rc.report(bad)
    for k, v in sp.items():
        SPREADS.setdefault(k, []).extend(v)
        assert max(v) <= rc.ROW_FACTOR / 2 or k in rc.WIDE, f"{k}: spread {max(v):.2f}"


def test_print_the_measured_spreads():
    """(runs after the fairness tests of this module: the worst spread per tensor, as quoted in row_checks.SPREADS)"""
    for k in sorted(SPREADS):
        print(f"spread {k}: worst {max(SPREADS[k]):.2f} over {len(SPREADS[k])} problems")


# ---------------------------------------------------------------------------------------------------------------------
# the rule bites
# ---------------------------------------------------------------------------------------------------------------------
def _caught(findings, tensor):
    bad = [x for x in findings if not x.ok and x.tensor.startswith(tensor)]
    assert bad, f"not caught on {tensor}:\n" + rc.report(findings)
    print("\n" + rc.report(bad))
    return bad[0]


LN_PLANTED = [
    # defect, case, regime, tensor that must fail, (row that must be named or None)
    ("one_pass_variance", _ln_case("fwd", C=768, R=0, B=77, y16=False, save_stats=True, stats_arg=False), "offset", "rstd", None),
    ("eps_dropped", _ln_case("fwd", C=768, R=0, B=77, y16=False, save_stats=True, stats_arg=False), "tiny", "y", None),
    ("eps_dropped", _ln_case("fwd", C=768, R=0, B=77, y16=False, save_stats=True, stats_arg=False), "const", "rstd", None),
    ("eps_1e-5_for_1e-6", _ln_case("fwd", C=768, R=0, B=77, y16=False, save_stats=True, stats_arg=False), "tiny", "y", None),
    ("eps_1e-5_for_1e-6", _ln_case("fwd", C=768, R=0, B=77, y16=False, save_stats=True, stats_arg=False), "const", "rstd", None),
    ("odd_last_row_takes_neighbours_stats", _ln_case("fwd", C=768, R=13, B=5, y16=True), "randn", "y", "row 12"),
    ("odd_last_row_takes_neighbours_stats", _ln_case("fwd", C=768, R=7, B=1, y16=False), "randn", "mean", "row 6"),
    ("second_slot_missing_from_dgamma", _ln_case("bwd", C=768, R=2045, B=3, dxs_rows=None), "randn", "dgamma", None),
    ("dx_in_not_added_on_fp32_part", _ln_case("bwd", C=768, R=13, B=1, in_hi=True, dxs_rows=None), "randn", "dx_hi", "row 13"),
    ("dxs_scaled_by_next_rows_factor", _ln_case("bwd", C=768, R=13, B=1, scaled=True), "randn", "dxs", None),
    ("dxsum_over_all_rows", _ln_case("bwd", C=768, R=13, B=1, dxsum=True, dxs_rows=8), "randn", "dxsum", None),
]


@pytest.mark.parametrize("defect,case,regime,tensor,row", LN_PLANTED, ids=[f"{d}-{r}-{rc.ln_case_id(c)}" for d, c, r, _, _ in LN_PLANTED])
def test_layernorm_planted_defect_is_caught(defect, case, regime, tensor, row):
    for operand in OPERANDS:
        clean = rc.check_ln_case(case, regime, run=_ln_stand_in("kernel"), operand=operand)
        assert all(x.ok for x in clean), rc.report(clean)
        f = rc.check_ln_case(case, regime, run=_ln_stand_in("kernel", defect), operand=operand)
        hit = _caught(f, tensor)
        print(f"{defect} [{regime}, {operand}]: {tensor} {hit.value / max(hit.bound, 1e-300):.3g} x the bound")
        if row is not None:
            assert row in hit.detail, hit.detail


def test_single_row_off_by_one_per_cent_is_seen_at_16_bit_output():
    case = _ln_case("fwd", C=768, R=13, B=5, y16=True)

    def run(c, p):
        o = rc.ln_fwd_eval(p, c, "kernel")
        o["y"][5] = rc._r16(o["y"][5] * 1.01, p["operand"])
        return o, []
    for operand in OPERANDS:
        hit = _caught(rc.check_ln_case(case, "randn", run=run, operand=operand), "y rowerr")
        assert "row 5" in hit.detail
        print(f"1 % on one row [{operand}]: {hit.value / hit.bound:.2f} x the bound")


KL_PLANTED = [("tied_top_value_counted_once", rc._kl(778, 5), "tie_inside"), ("boundary_tie_drops_k_plus_1", rc._kl(778, 5), "tie_across"),
              ("half_the_candidates_per_thread", rc._kl(9871, 5), "one_thread"), ("half_the_candidates_per_thread", rc._kl(778, 1), "one_thread")]


@pytest.mark.parametrize("defect,case,regime", KL_PLANTED[:3], ids=[f"{d}-{rc.kl_case_id(c)}-{r}" for d, c, r in KL_PLANTED[:3]])
def test_kl_topk_planted_defect_is_caught(defect, case, regime):
    clean = rc.check_kl_case(case, regime, run=_loss_stand_in(rc.kl_eval, "kernel"))
    assert all(x.ok for x in clean), rc.report(clean)
    f = rc.check_kl_case(case, regime, run=_loss_stand_in(rc.kl_eval, "kernel", defect))
    hit = _caught(f, "target rowerr")
    print(f"{defect}: target {hit.value / max(hit.bound, 1e-300):.3g} x the bound; {hit.detail}")
    _caught(f, "dpred")


def test_soft_ce_planted_defect_is_caught():
    case = next(c for c in rc.CE_TESTS if c.mode == "given" and c.dx and not c.hot)
    clean = rc.check_ce_case(case, run=_loss_stand_in(rc.ce_eval, "kernel"))
    assert all(x.ok for x in clean), rc.report(clean)
    hit = _caught(rc.check_ce_case(case, run=_loss_stand_in(rc.ce_eval, "kernel", "target_sum_taken_as_1")), "dx rowerr")
    print(f"target_sum_taken_as_1: dx {hit.value / max(hit.bound, 1e-300):.3g} x the bound")


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
def test_ids_are_unique():
    for ids in ([rc.ln_test_id(t) for t in rc.LN_TESTS], [f"{rc.kl_case_id(c)}-{r}" for c, r in rc.KL_TESTS], [rc.ce_case_id(c) for c in rc.CE_TESTS],
                [rc.simple_case_id(c) for c in rc.SIMPLE_CASES], [rc.exact_case_id(c) for c in rc.EXACT_CASES]):
        assert len(ids) == len(set(ids)), [i for i in ids if ids.count(i) > 1][:5]


def test_case_table_holds_the_issue_s_cases():
    fwd = {(c.C, c.split, c.R, c.B, c.y16) for c in rc.LN_FWD_CASES}
    for C in (512, 768, 1024):
        for y16 in (False, True):
            for M in (1, 3, 4, 5, 77):
                assert (C, False, 0, M, y16) in fwd
            for R in (1, 2, 7, 8, 9, 13):
                for B in (0, 1, 4, 5):
                    assert (C, True, R, B, y16) in fwd
    assert any(c.ld and c.split and c.R and c.B for c in rc.LN_FWD_CASES)
    assert any(not c.save_stats for c in rc.LN_FWD_CASES) and any(c.stats_arg for c in rc.LN_FWD_CASES)
    bwd = rc.LN_BWD_CASES
    for M, _ in rc.LN_BWD_PLAIN:
        for dy16 in (True, False):
            for has_in in (True, False):
                assert any(c.C == 768 and not c.split and c.B == M and c.dy16 == dy16 and c.in_hi == has_in and c.dxs_rows is None for c in bwd)
    for R, B, _ in rc.LN_BWD_SPLIT:
        assert any(c.C == 768 and c.R == R and c.B == B for c in bwd)
    split = [c for c in bwd if c.split and c.dxs_rows is None and c.C == 768]
    assert {(c.in_lo, c.in_hi) for c in split} == {(True, True), (False, True), (True, False), (False, False)}
    assert len({(c.R, c.B) for c in split if not c.dy16}) >= 2
    dxs = [c for c in bwd if c.dxs_rows is not None]
    for (R, B) in ((0, 77), (13, 1), (2045, 3)):
        mine = [c for c in dxs if (c.R, c.B) == (R, B)]
        assert {c.dxs_rows for c in mine} >= {R + B, max(1, (R or R + B) - 5), 1}
        assert {c.scaled for c in mine} == {True, False} and any(c.dxsum for c in mine)
        assert {(c.beta_acc, c.sum_beta) for c in mine if c.dxsum} >= {(0.0, 0.0), (1.0, 1.0), (0.0, 1.0)}
    for C in (512, 1024):
        assert any(c.C == C and c.B == 2049 and not c.split for c in bwd) and any(c.C == C and c.R == 4089 for c in bwd)
    regs = {(r, d) for _, r, d in rc.LN_TESTS}
    assert {r for r, _ in regs} == set(rc.LN_REGIMES) and ("randn", "scaled") in regs
    kl = {(c.K, c.topk) for c, r in rc.KL_TESTS if r == "randn" and not c.ld and not c.nulls}
    assert kl == {(K, k) for K in rc.KL_KS for k in (0, 1, 5, 8)}
    assert {r for _, r in rc.KL_TESTS} == set(rc.KL_REGIMES)
    assert {c.nulls for c, _ in rc.KL_TESTS} >= {"l", "d", "t", "ld", "lt", "dt", "ldt"} and any(c.ld for c, _ in rc.KL_TESTS)
    assert {c.K for c in rc.CE_TESTS} == {97, 257, 300, 1000} and {c.mode for c in rc.CE_TESTS} == {"given", "synth"}
    assert any(not c.dx for c in rc.CE_TESTS) and any(c.hot for c in rc.CE_TESTS)
    simple = {(c.entry, c.shape) for c in rc.SIMPLE_CASES}
    for entry, shapes in (("l2norm", (1, 255, 257, 512, 1000)), ("softmax_rows", (1, 255, 257, 9871)), ("mse", (1, 255, 257, 4096)),
                          ("gelu_f32", (4096 * 256 + 5,)), ("milnce", ((1, 1), (4, 3), (24, 5), (128, 64), (130, 64))),
                          ("gemv_rows", tuple((R, C) for R in (1, 3, 4, 5) for C in (1, 63, 65)))):
        for s in shapes:
            assert (entry, s) in simple, (entry, s)
    assert {c.opt for c in rc.SIMPLE_CASES if c.entry == "group_reduce"} == {"ff", "fh", "hf", "hh"}
    assert {c.shape[1] for c in rc.SIMPLE_CASES if c.entry == "group_reduce"} == {1, 8}
    assert {(c.shape[0], c.opt) for c in rc.SIMPLE_CASES if c.entry == "batch_sum" and c.shape[1] == 2731} == {(1, "32"), (5, "32"), (1, "16"), (5, "16")}
    assert {c[0] for c in rc.EXACT_CASES} == {"cast_scale", "group_bcast", "embed_table", "cast_weight_pad", "cast_weight"}
    assert ("cast_scale", (16400, 1024), "rowscale") in rc.EXACT_CASES and ("cast_scale", (16400, 1024), "norowscale") in rc.EXACT_CASES


def test_cases_past_a_grid_cap_are_past_it():
    for c in rc.SIMPLE_CASES:
        if c.entry == "batch_sum":
            B, rows, C = c.shape
            assert (rows * (C // (8 if c.opt == "16" else 4)) > rc.GRID_CAP) == c.path.startswith("past_the"), c
        if c.entry == "group_reduce":
            assert (c.shape[0] * c.shape[2] > rc.GRID_CAP) == c.path.startswith("past_the"), c
        if c.entry == "milnce":
            assert (c.shape[0] ** 2 * c.shape[1] > 4096 * 256) == c.path.startswith("past_the"), c
    for entry, shape, opt in rc.EXACT_CASES:
        n = {"cast_scale": lambda s: s[0] * s[1] // 8, "group_bcast": lambda s: s[0] * s[1] * s[2], "embed_table": lambda s: s[0] * s[1] * s[2]}.get(entry)
        if n is not None and opt.startswith("past_the"):
            assert n(shape) > rc.GRID_CAP
    assert 16400 * 1024 // 8 > rc.GRID_CAP


def test_layernorm_cases_land_where_they_say():
    def last(M, R):
        blk, wave, slot, it = rc.ln_bwd_assign(M, R)
        lo = torch.arange(M) < R
        return dict(nblk=rc.ln_bwd_nblk(M), nb_hi=rc.ln_bwd_nblk_hi(M, R), slot2=int((slot[lo] == 1).sum()), it_lo=int(it[lo].max()) if R else 0,
                    it_hi=int(it[~lo].max()) if R < M else 0)
    assert last(13 + 1, 13) == dict(nblk=5, nb_hi=1, slot2=0, it_lo=0, it_hi=0)
    assert last(2044 + 3, 2044) == dict(nblk=512, nb_hi=1, slot2=0, it_lo=0, it_hi=0)
    assert last(2045 + 3, 2045) == dict(nblk=512, nb_hi=1, slot2=1, it_lo=0, it_hi=0)
    assert last(4088 + 3, 4088) == dict(nblk=512, nb_hi=1, slot2=2044, it_lo=0, it_hi=0)
    assert last(4089 + 3, 4089) == dict(nblk=512, nb_hi=1, slot2=2044, it_lo=1, it_hi=0)
    assert last(8 + 300, 8) == dict(nblk=78, nb_hi=9, slot2=0, it_lo=0, it_hi=8)
    d = last(2000 + 300, 2000)
    assert (d["nblk"], d["nb_hi"], d["it_lo"], d["it_hi"]) == (512, 64, 0, 1) and 0 < d["slot2"] < 4 * (512 - 64)
    assert last(2048, 0)["it_hi"] == 0 and last(2049, 0)["it_hi"] == 1 and last(4100, 0)["it_hi"] == 2 and last(2048, 0)["nblk"] == 512
    # every row is owned by exactly one (workgroup, wave, slot, iteration), and workgroups stay inside the grid
    for M, R in ((2300, 2000), (4092, 4089), (308, 8), (2049, 0), (14, 13), (7, 7)):
        blk, wave, slot, it = rc.ln_bwd_assign(M, R)
        key = ((blk * 4 + wave) * 2 + slot) * 64 + it
        assert len(set(key.tolist())) == M and int(blk.max()) < rc.ln_bwd_nblk(M)
        nb_lo = rc.ln_bwd_nblk(M) - rc.ln_bwd_nblk_hi(M, R)
        assert bool((blk[:R] < nb_lo).all()) and bool((blk[R:] >= nb_lo).all())
    # forward: an odd rows16 leaves a wave whose only row is the last one
    for c in rc.LN_FWD_CASES:
        assert ("odd_last_row_alone" in c.path) == (c.R % 2 == 1)
        assert c.path.startswith(f"wg{-(-c.R // 8)}+{-(-c.B // 4)}")
    assert {c.R for c in rc.LN_FWD_CASES if "odd_last_row_alone" in c.path} == {1, 7, 9, 13}
    # kl_topk paths
    assert rc.kl_path(12288, 5).startswith("staged") and rc.kl_path(12289, 5).startswith("unstaged") and "idle_threads" in rc.kl_path(255, 5)
    assert "topk_max" in rc.kl_path(257, 8)
    for c, r in rc.KL_TESTS:
        if r == "one_thread":
            assert c.K >= 3 + 256 * c.topk
