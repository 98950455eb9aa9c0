"""The pooling-operator harness (tests/mvit_pool_checks.py) tested without a GPU: the rounding model stands in for the kernel.

  - the rules are PASSABLE: the model itself and the legitimate variant (forward LN statistics from the rounded conv output) pass every
    judge in every regime, for fp16 and bf16; a hand-written two-pass fp32 LayerNorm passes the LayerNorm judge; the plain selection
    model passes the bit-exact max-pool judge (ties and plateaus included);
  - the rules BITE: each of the nine planted defects below fails;
  - RECORDED (`OLD_CHECKS_PASS`): FOUR of the nine pass today's checks of tests/mvit_checks.py -- the 1 % token stays under the flat
    6e-3 bound even on the planted geometry; ties never occur in its fp32 `randn` max-pool input; its LayerNorm has M <= 300, where no
    second in-flight row is live; and it never compares rstd.  The other five exceed the flat bounds WHEN EVALUATED ON THE PLANTED
    GEOMETRY (odd T, odd plane); mvit_checks itself runs no odd plane under a stride, so the dropped dgrad row (5) is invisible on its own
    shapes as well.
  - the dispatch restatements reach exactly the hand-written list of instantiations, and the case tables hold the edges they are there for.
"""
import pytest
import torch

import mvit_pool_checks as mc

OPERANDS = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]


# ---------------------------------------------------------------------------------------------------------------------
# (a) the model and the legitimate variant pass
# ---------------------------------------------------------------------------------------------------------------------
def _pool_run(operand, **kw):
    return lambda c, p: (mc.pool_model(p, c, operand, **kw), [])


HOST_POOL_CASES = [mc._pool(2, 2, (5, 7, 7), (1, 2, 2)), mc._pool(1, 3, (3, 6, 10), (1, 1, 1)), mc._pool(2, 1, (5, 5, 7), (2, 2, 2)),
                   mc._pool(2, 2, (1, 1, 1), (1, 2, 2)), mc._pool(1, 2, (1, 3, 3), (1, 8, 8))]


@pytest.mark.parametrize("operand", OPERANDS, ids=IDS)
@pytest.mark.parametrize("regime", mc.POOL_REGIMES)
@pytest.mark.parametrize("variant", [False, True], ids=["model", "variant"])
def test_model_and_variant_pass_every_pool_judge(variant, regime, operand):
    for c in HOST_POOL_CASES:
        findings = mc.check_pool_case(c, regime, run=_pool_run(operand, variant=variant), operand=operand)
        assert all(f.ok for f in findings), mc.pool_case_id(c) + "\n" + mc.report(findings)
        names = " ".join(f.tensor for f in findings)
        for n in ("conv_out elementwise", "y rowerr", "dX rowerr", "dw", "dgamma", "dbeta"):
            assert n in names, (n, names)


@pytest.mark.parametrize("operand", OPERANDS, ids=IDS)
def test_model_passes_the_exact_tap_map(operand):
    c = mc._pool(1, 2, (3, 5, 4), (1, 2, 2))
    findings = mc.check_tap_map(c, run=_pool_run(operand), operand=operand)
    assert all(f.ok for f in findings), mc.report([f for f in findings if not f.ok])
    assert sum("conv_out bit-equal" in f.tensor for f in findings) == 27 and sum("dX bit-equal" in f.tensor for f in findings) == 27


def _maxpool_run(last=False):
    def run(c, p):
        m = mc.maxpool_model(p, c, last=last)
        return dict(y=m["y"], y_am=m["y"], dx_scan=m["dx"], dx_am=m["dx"], amax=m["amax"]), []
    return run


@pytest.mark.parametrize("case,regime", mc.MAXPOOL_TESTS, ids=[f"{mc.maxpool_case_id(c)}-{r}" for c, r in mc.MAXPOOL_TESTS])
def test_selection_model_passes_the_maxpool_judge(case, regime):
    findings = mc.check_maxpool_case(case, regime, run=_maxpool_run())
    assert all(f.ok for f in findings), mc.report(findings)


def _ln_stand_in(c, m, operand):
    got = dict(y=m["y16"] if c.y16 else m["y"], mean=m["mean"], rstd=m["rstd"], dx=m["dx"], dgamma=m["dgamma"], dbeta=m["dbeta"],
               ypad=torch.zeros(c.M, c.Cpad - c.C), dxpad=torch.zeros(c.M, c.Cpad - c.C))
    if c.fused:
        got["dx16"] = m["dx16"]
    return got, []


def _ln_run(operand, kind):
    """kind "flip": the kernels' two-pass arithmetic with the channels summed in reverse; "torch": plain fp32 torch layer_norm"""
    def run(c, p):
        if kind == "flip":
            return _ln_stand_in(c, mc.ln_model(p, c, operand, flip=True), operand)
        m = mc.ln_yardstick(p, c)
        m["y16"] = mc._rnd(m["y"], operand)
        m["dx16"] = mc._rnd(m["dx"] * p["rowscale"][:, None], operand)
        return _ln_stand_in(c, m, operand)
    return run


HOST_LN_CASES = [mc._ln(300, 96, 128), mc._ln(9, 192, 256, y16=True, dy16=True, fused=True), mc._ln(3, 768, 768, res=False),
                 mc._ln(1, 65, 128, fused=True), mc._ln(3, 1, 64)]


@pytest.mark.parametrize("operand", OPERANDS, ids=IDS)
@pytest.mark.parametrize("regime", mc.LN_REGIMES)
@pytest.mark.parametrize("kind", ["flip", "torch"])
def test_a_second_layernorm_implementation_passes(kind, regime, operand):
    for c in HOST_LN_CASES:
        findings = mc.check_ln_case(c, regime, run=_ln_run(operand, kind), operand=operand)
        assert all(f.ok for f in findings), mc.ln_case_id(c) + "\n" + mc.report(findings)
        names = " ".join(f.tensor for f in findings)
        for n in ("y (", "mean", "rstd", "dx rowerr", "dgamma", "dbeta"):
            assert n in names, (n, names)


def _norm_run(operand, kind):
    def run(c, p):
        if kind == "flip":
            return mc._norm_eval(p, c, torch.float32, operand, flip=True), []
        m = mc._norm_eval(p, c, torch.float32)
        m["dx_lo"], m["dxs"] = mc._rnd(m["dx_lo"], operand), mc._rnd(m["dxs"], operand)
        m["y"] = mc._rnd(m["y"], operand) if c.y16 else m["y"]
        return m, []
    return run


HOST_NORM_CASES = [mc._norm(512, 3, 2, dxs_rows=4, dxsum=True), mc._norm(768, 0, 5, y16=False, in_hi=False),
                   mc._norm(768, 300, 90, dy16=True, in_lo=False, dxs_rows=390, dxsum=True)]


@pytest.mark.parametrize("operand", OPERANDS, ids=IDS)
@pytest.mark.parametrize("regime", mc.LN_REGIMES)
@pytest.mark.parametrize("kind", ["flip", "torch"])
def test_a_second_split_row_layernorm_passes(kind, regime, operand):
    for c in HOST_NORM_CASES:
        findings = mc.check_norm_case(c, regime, run=_norm_run(operand, kind), operand=operand)
        assert all(f.ok for f in findings), mc.norm_case_id(c) + "\n" + mc.report(findings)


def test_split_row_defects_fail():
    """a 16-bit dx_out row that lost its incoming gradient, dxsum over one row too many, dxs without its row scale"""
    c = mc._norm(768, 300, 90, dxs_rows=389, dxsum=True)
    for plant, tensor in (("din", "dx_out, 16-bit rows"), ("sum", "dxsum"), ("scale", "dxs")):
        def run(c, p, plant=plant):
            m = mc._norm_eval(p, c, torch.float32, torch.float16)
            if plant == "din":
                m["dx_lo"][7] = mc._rnd(m["dx_lo"][7] - p["din"][7], torch.float16)
            elif plant == "sum":
                m["dxsum"] = m["dxsum"] + m["dx_hi"][c.dxs_rows - c.rows16][None]
            else:
                m["dxs"][5] = mc._rnd(m["dxs"][5] / p["rowscale"][5], torch.float16)
            return m, []
        bad = [f.tensor for f in mc.check_norm_case(c, "randn", run=run, operand=torch.float16) if not f.ok]
        assert len(bad) == 1 and bad[0].startswith(tensor), (plant, bad)


def test_im2col_expected_matches_conv3d():
    """the unfold reference times a weight matrix IS Conv3d: pins the column order ((c kt + a) kh + y) kw + x"""
    c = mc.IM2COL_CASES[0]
    g = torch.Generator().manual_seed(5)
    fr = torch.randn(c.B, c.Cin, c.T, c.H, c.W, generator=g).to(torch.float16).double()
    w = torch.randn(4, c.Cin, *c.kernel, generator=g).double()
    cols = mc.im2col_expected(fr, c, torch.float64)
    ref = torch.nn.functional.conv3d(fr, w, None, c.stride, c.padding)
    assert (cols.double() @ w.reshape(4, -1).t() - ref.permute(0, 2, 3, 4, 1).reshape(-1, 4)).abs().max() < 1e-10
    findings = mc.check_im2col_case(c, run=lambda c, f: (torch.nn.functional.pad(mc.im2col_expected(f, c, torch.float16), (0, c.ldo - cols.shape[1])), []),
                                    operand=torch.float16)
    assert all(f.ok for f in findings)


# ---------------------------------------------------------------------------------------------------------------------
# (b), (c) the planted defects
# ---------------------------------------------------------------------------------------------------------------------
BIG = mc._pool(2, 2, (5, 15, 15), (1, 2, 2))          # odd T, odd plane; 4 x 321 pooled tokens, 4 x 1126 input tokens


@pytest.fixture(scope="module")
def big():
    p = mc.make_pool_problem(BIG, "randn", torch.float16)
    return p, mc.pool_reference(p, BIG), mc.pool_model(p, BIG, torch.float16)


def _old_pool_bounds_pass(x, ref):
    """mvit_checks.check_mvit_pool: whole-tensor relative L2 of y (tokens, cls), dX (tokens, cls), dw, dgamma, dbeta; conv_out is not looked at"""
    ok = True
    for n, b in (("y", mc.AGG_FWD), ("dX", mc.AGG_BWD)):
        ok &= mc.agg(x[n][:, :-1], ref[n][:, :-1]) <= b and mc.agg(x[n][:, -1], ref[n][:, -1]) <= b
    for n in ("dw", "dgamma", "dbeta"):      # there dw etc. start at zero: compare the gradients
        ok &= mc.agg(x[n], ref[n]) <= mc.AGG_BWD
    return bool(ok)


def _new_pool_rule_passes(p, ref, mod, x):
    return all(f.ok for f in mc.judge_pool(BIG, "randn", x, ref, mod, p, torch.float16))


def _one_token_1pct(p, ref, mod):
    x = dict(mod)
    x["y"] = mod["y"].clone()
    x["y"][2, 100] *= 1.01
    return x


POOL_PLANTS = {
    "1_border_tokens_use_the_transposed_tap": lambda p, ref, mod: mc.pool_model(p, BIG, torch.float16, defect="border_taps_transposed"),
    "2_last_frame_from_the_t_sum": lambda p, ref, mod: mc.pool_model(p, BIG, torch.float16, defect="last_frame_from_t_sum"),
    "3_cls_token_through_the_conv": lambda p, ref, mod: mc.pool_model(p, BIG, torch.float16, defect="cls_through_conv"),
    "4_one_token_of_y_off_by_1pct": _one_token_1pct,
    "5_dgrad_drops_output_row_Ho-1_on_an_odd_plane": lambda p, ref, mod: mc.pool_model(p, BIG, torch.float16, defect="dgrad_drops_last_output_row"),
    "6_wgrad_skips_the_last_frame_when_T_is_odd": lambda p, ref, mod: mc.pool_model(p, BIG, torch.float16, defect="wgrad_skips_last_frame"),
}
# (c) which of the nine pass TODAY's checks of tests/mvit_checks.py: 1 - 6 by its flat aggregate bounds evaluated on BIG (asserted below),
# 7 - 9 because it never exercises them (asserted in their own tests: the defect changes nothing on its kind of input)
OLD_CHECKS_PASS = {"1_border_tokens_use_the_transposed_tap": False, "2_last_frame_from_the_t_sum": False, "3_cls_token_through_the_conv": False,
                   "4_one_token_of_y_off_by_1pct": True, "5_dgrad_drops_output_row_Ho-1_on_an_odd_plane": False,
                   "6_wgrad_skips_the_last_frame_when_T_is_odd": False,
                   "7_maxpool_ties_to_the_last_maximum": True, "8_ln_g_bwd_second_inflight_row_missing_from_dgamma": True,
                   "9_rstd_without_eps_on_a_constant_row": True}


def test_the_model_passes_and_is_inside_the_old_bounds(big):
    p, ref, mod = big
    assert _new_pool_rule_passes(p, ref, mod, mod) and _old_pool_bounds_pass(mod, ref)


@pytest.mark.parametrize("name", sorted(POOL_PLANTS))
def test_planted_pool_defect_fails(big, name):
    p, ref, mod = big
    x = POOL_PLANTS[name](p, ref, mod)
    assert not _new_pool_rule_passes(p, ref, mod, x), name
    assert _old_pool_bounds_pass(x, ref) == OLD_CHECKS_PASS[name], name


def test_planted_structural_defects_fail_the_tap_map_too():
    c = mc._pool(1, 1, (3, 5, 5), (1, 2, 2))
    for d in ("border_taps_transposed", "last_frame_from_t_sum", "cls_through_conv"):
        findings = mc.check_tap_map(c, run=_pool_run(torch.float16, defect=d), operand=torch.float16)
        assert any(not f.ok for f in findings), d


def test_maxpool_ties_to_the_last_maximum_fail():
    c = mc.MAXPOOL_CASES[0]
    bad = mc.check_maxpool_case(c, "ties", run=_maxpool_run(last=True))
    assert any(not f.ok and "dx" in f.tensor for f in bad) and any(not f.ok and "argmax" in f.tensor for f in bad)
    assert all(f.ok for f in mc.check_maxpool_case(c, "randn", run=_maxpool_run(last=True)))      # fp32 randn has no ties: today's check cannot see it
    assert OLD_CHECKS_PASS["7_maxpool_ties_to_the_last_maximum"]


def _ln_defect_run(defect, operand=torch.float16):
    return lambda c, p: _ln_stand_in(c, mc.ln_model(p, c, operand, defect=defect), operand)


def test_second_inflight_row_missing_from_dgamma_fails():
    c = mc._ln(4099, 96, 128)
    assert c.kernel.endswith("live1")
    bad = mc.check_ln_case(c, "randn", run=_ln_defect_run("second_inflight_row_missing_from_dgamma"), operand=torch.float16)
    assert [f.tensor for f in bad if not f.ok] == ["dgamma (start + gradient) rowerr"], mc.report(bad)
    # at the largest M of mvit_checks (300) no second in-flight row holds a real row: the same defect changes nothing there
    small = mc._ln(300, 96, 128)
    assert all(f.ok for f in mc.check_ln_case(small, "randn", run=_ln_defect_run("second_inflight_row_missing_from_dgamma"), operand=torch.float16))
    assert OLD_CHECKS_PASS["8_ln_g_bwd_second_inflight_row_missing_from_dgamma"]


def test_rstd_without_eps_on_a_constant_row_fails():
    c = mc._ln(300, 96, 128)
    bad = mc.check_ln_case(c, "constant", run=_ln_defect_run("rstd_without_eps"), operand=torch.float16)
    assert "rstd rowerr" in [f.tensor for f in bad if not f.ok], mc.report(bad)
    # in `randn` no row is constant and eps changes rstd by 5e-7 relative: inside the rule, as it should be
    assert all(f.ok for f in mc.check_ln_case(c, "randn", run=_ln_defect_run("rstd_without_eps"), operand=torch.float16))
    assert all(f.ok for f in mc.check_ln_case(c, "randn", run=_ln_defect_run(None), operand=torch.float16))
    assert OLD_CHECKS_PASS["9_rstd_without_eps_on_a_constant_row"]          # mvit_checks compares y, dx, dgamma, dbeta: never rstd


def test_four_of_the_nine_defects_pass_todays_checks():
    assert len(OLD_CHECKS_PASS) == 9 and sum(OLD_CHECKS_PASS.values()) == EXPECTED_OLD_PASS


EXPECTED_OLD_PASS = 4


# ---------------------------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------------------------
EVERY_POOL_KERNEL = """fwd_t<dense> fwd_t<sparse> fwd dgrad_t<true,1> dgrad_t<false,2> dgrad_t<false,4> dgrad_t<false,8> dgrad_t<false,0> dgrad
wgrad_t wgrad ln_bwd ln_bwd.loop""".split()


def test_pool_case_table_reaches_every_instantiation_and_edge():
    reached = set()
    for c in mc.POOL_CASES:
        reached.update(c.kernel.split("+"))
    assert reached == set(EVERY_POOL_KERNEL)
    by_kernel = {}
    for c, r in mc.POOL_TESTS:
        for k in c.kernel.split("+"):
            by_kernel.setdefault(k, set()).add(r)
    for k, regs in by_kernel.items():
        assert set(mc.POOL_REGIMES) <= regs or k == "ln_bwd.loop", (k, regs)
    assert all((c, "randn") in mc.POOL_TESTS for c in mc.POOL_CASES)
    assert {mc.fwd_grid(c) for c in mc.POOL_CASES} >= {8, 9, 17}
    assert {c.H for c in mc.POOL_CASES} >= {1, 2, 3, 8}
    assert {(c.slot, c.pad) for c in mc.POOL_CASES} == {(s, p) for s in (0, 1, 2) for p in (False, True)}
    assert {c.thw[0] for c in mc.POOL_CASES if c.stride[0] == 1} >= {1, 2, 3, 5}
    tapk = set()
    for c in mc.TAP_CASES:
        tapk.update(c.kernel.split("+"))
    assert tapk >= set(EVERY_POOL_KERNEL) - {"ln_bwd.loop"}
    ids = [f"{mc.pool_case_id(c)}-{r}" for c, r in mc.POOL_TESTS]
    assert len(set(ids)) == len(ids)
    for c in mc.POOL_CASES:
        o = mc.out_thw(c.thw, c.stride)
        rows = c.B * c.H * (o[0] * o[1] * o[2] + 1)
        assert rows * mc.pool_draws(c) >= mc.MIN_ROWS or mc.pool_draws(c) == 256


def test_dispatch_restatements_on_known_geometries():
    assert mc.pool_names(1, 1, (8, 56, 56), (1, 8, 8))[:3] == ["fwd_t<dense>", "dgrad_t<false,8>", "wgrad_t"]          # block 0's k / v pooling
    assert mc.pool_names(1, 1, (8, 66, 66), (1, 1, 1))[3] == "ln_bwd.loop" and mc.pool_names(1, 1, (8, 64, 64), (1, 1, 1))[3] == "ln_bwd.loop"
    assert mc.pool_names(1, 1, (8, 64, 63), (1, 1, 1))[3] == "ln_bwd"
    assert mc.pool_names(1, 1, (2, 6, 8), (1, 2, 4))[1] == "dgrad_t<false,0>" and mc.pool_names(1, 1, (4, 6, 6), (2, 2, 2))[1] == "dgrad"
    kinds = [mc.im2col_kernel(c) for c in mc.IM2COL_CASES]
    assert {"rows", "generic(W%4)", "generic(pitch)", "generic(kw)", "generic(lines)"} == set(kinds)
    assert mc.ln_names(4099, 96, 128, False, False, True)[1].endswith("live1") and mc.ln_names(4096, 96, 128, False, False, True)[1].endswith("live0")
    assert mc.ln_names(8197, 96, 128, False, False, True)[1].endswith("live2") and mc.ln_names(12291, 96, 128, False, False, True)[1].endswith("live3")
    assert mc.ln_names(4101, 192, 256, False, False, True)[1] == "ln_bwd<f32,4,2,res>.live1"
    assert mc.ln_names(4101, 384, 384, False, True, False)[1] == "ln_bwd<op,6,2,nores>.live1"
    live = {c.kernel.rsplit(".", 1)[1] for c in mc.LN_CASES}
    assert live == {"live0", "live1", "live2", "live3"}
    assert {(c.C, c.Cpad) for c in mc.LN_CASES} >= {(96, 128), (192, 256), (384, 384), (768, 768), (1, 64), (65, 128), (700, 768)}
    assert {(c.s, c.H, c.W) for c in mc.MAXPOOL_CASES} == {(2, 8, 6), (2, 7, 5), (2, 1, 1), (2, 2, 3), (4, 8, 8), (4, 6, 10), (3, 7, 7)}
    assert {c.T for c in mc.MAXPOOL_CASES} == {1, 3} and {c.C for c in mc.MAXPOOL_CASES} == {4, 96, 192}
    assert all(c.ldi != c.ldo for c in mc.MAXPOOL_CASES)
    # norm.hip: both widths on every split, the 512-workgroup cap (M > 2044), a live second in-flight row and a second loop iteration
    assert {(c.C, c.rows16, c.rows32) for c in mc.NORM_CASES} >= {(C, a, b) for C in (512, 768) for a, b in
                                                                  ((0, 5), (7, 0), (1, 1), (3, 2), (2045, 3), (5009, 31))}
    nk = set()
    for c in mc.NORM_CASES:
        nk.update(c.kernel.split("+"))
    for C in (512, 768):
        for dy in ("op", "f32"):
            for part in ("lo_in", "lo_noin", "hi_in", "hi_noin"):
                assert any(k.startswith(f"nbwd<{C},{dy}>.{part}") for k in nk), (C, dy, part)
        assert any(k.startswith(f"nbwd<{C},") and k.endswith(".r2") for k in nk) and any(k.startswith(f"nbwd<{C},") and k.endswith(".it2") for k in nk)
    assert mc.norm_names(768, 301, 90, True, True, False, True)[2] == "nbwd<768,op>.hi_in.it2" and "nbwd<768,op>.hi_in.it2" in nk
    assert mc.norm_names(768, 2045, 3, True, False, True, True)[1] == "nbwd<768,f32>.lo_in.r2"          # 512 workgroups, 1 of them on the fp32 rows
    assert mc.norm_names(768, 2044, 0, True, False, True, True)[1] == "nbwd<768,f32>.lo_in"
    assert any(c.dxs_rows is not None and c.dxs_rows < c.rows16 + c.rows32 for c in mc.NORM_CASES) and any(c.dxsum for c in mc.NORM_CASES)
