"""The GEMM harness (tests/gemm_checks.py) tested without a GPU: the rounding model stands in for the kernel, for fp16 and bf16.

  (a) the rules are PASSABLE: the model passes every judge in every regime (which also proves the `exact` / `k_edge` claim: fp32 sums of
      those inputs ARE exact, across splits and with every epilogue); so do two legitimate variants -- K summed in reverse tile order with
      GELU taken from the rounded `u`, split-K partials summed in reverse -- each reduce order judged against the other one's model, and
      plain fp32 torch.matmul for the fp32 kernels;
  (b) the rules BITE: each of the twelve planted defects of `NT_DEFECTS` / `TN_DEFECTS` fails;
  (c) RECORDED (`OLD_CHECKS_PASS`): which of them today's tests/kernel_checks.py formulas (aggregate relative L2 against its flat bounds)
      let through on the planted geometry (1093 x 512 x 192; TN 1569 x 384 x 256 in 5 / 24 slices), per operand type;
  (d) the dispatch restatements reach exactly the hand-written lists of names, and the case tables hold the edges they are there for.
"""
import pytest
import torch

import gemm_checks as gc

OPERANDS = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
HOST_NT_SHAPES = [(300, 128, 64), (1093, 512, 192)]


def _bad(findings):
    return [f for f in findings if not f.ok]


# ---------------------------------------------------------------------------------------------------------------------
# (a) the model and the legitimate variants pass
# ---------------------------------------------------------------------------------------------------------------------
def _reverse_k(core):
    A, W = core["A"], core["W"]
    acc = torch.zeros(A.shape[0], W.shape[0])
    for k0 in reversed(range(0, A.shape[1], 64)):
        acc += A[:, k0:k0 + 64] @ W[:, k0:k0 + 64].t()
    return acc


def _nt_run(operand, variant):
    def run(c, core, x):
        if not variant:
            return gc.nt_model(c, core, x, operand), []
        return gc.nt_model(c, core, x, operand, acc=_reverse_k(core), defect="gelu_from_rounded_u"), []
    return run


@pytest.mark.parametrize("operand", OPERANDS, ids=IDS)
@pytest.mark.parametrize("regime", gc.REGIMES)
@pytest.mark.parametrize("variant", [False, True], ids=["model", "reverse_k"])
def test_model_and_variant_pass_every_nt_judge(variant, regime, operand):
    for (M, N, K) in HOST_NT_SHAPES:
        for epi in gc.EPIS:
            c = gc._nt(M, N, K, epi)
            findings = gc.check_nt_case(c, regime, run=_nt_run(operand, variant), operand=operand)
            assert not _bad(findings), gc.nt_case_id(c) + "\n" + gc.report(_bad(findings))
            names = " ".join(f.tensor for f in findings)
            exact = regime in ("exact", "k_edge") and epi not in ("dgelu", "dqgelu")
            assert ("EXACT" in names) == exact and (exact or "derived bound" in names), names


@pytest.mark.parametrize("operand", OPERANDS, ids=IDS)
@pytest.mark.parametrize("regime", gc.REGIMES)
def test_model_passes_the_batched_judge(regime, operand):
    for epi in gc.BATCH_EPIS:
        findings = gc.check_nt_batched(epi, regime, run=_nt_run(operand, False), operand=operand)
        assert not _bad(findings) and len(findings) >= 13, gc.report(_bad(findings))


def _tn_run(operand, how, defect=None):
    """how: "model"; "reverse" (partials summed in reverse); "other" (the other reduce kernel's order)"""
    def run(c, core, starts, splits):
        if how == "other":
            kind = c.kernel.split("+")[1]
            c = c._replace(kernel=c.kernel.split("+")[0] + ("+reduce_small" if kind == "reduce" else "+reduce"))
        return gc.tn_expect(c, core, starts, splits, operand, reverse=how == "reverse", defect=defect)[1], []
    return run


@pytest.mark.parametrize("operand", OPERANDS, ids=IDS)
@pytest.mark.parametrize("how", ["model", "reverse", "other"])
def test_model_reversed_partials_and_each_reduce_restatement_pass_every_tn_judge(how, operand):
    for c, regime in gc.TN_TESTS:
        findings = gc.check_tn_case(c, regime, run=_tn_run(operand, how), operand=operand, cus=32)
        assert not _bad(findings), f"{gc.tn_case_id(c)}-{regime}\n" + gc.report(_bad(findings))


@pytest.mark.parametrize("operand", OPERANDS, ids=IDS)
def test_model_passes_the_grouped_judge(operand):
    def run(items, splits):
        return [gc.tn_expect(c, core, starts, splits, operand)[1] for c, core, starts in items]
    for g, regime in gc.GROUP_TESTS:
        findings = gc.check_group_case(g, regime, run=run, cus=32, operand=operand)
        assert not _bad(findings), f"{gc.group_case_id(g)}-{regime}\n" + gc.report(_bad(findings))


def _small_run(operand, which):
    def run(c, core, x):
        m = gc.small_epilogue(c, x, core[which])
        got = dict(out=m["out"])
        if c.gelu:
            got.update(u16=gc._rnd(m["u"], operand), g16=gc._rnd(m["out"], operand))
        return got, []
    return run


@pytest.mark.parametrize("operand", OPERANDS, ids=IDS)
@pytest.mark.parametrize("which", ["acc32", "y32"], ids=["model", "torch_matmul"])
def test_model_and_plain_matmul_pass_the_fp32_kernels_judge(which, operand):
    for c, regime in gc.SMALL_TESTS:
        findings = gc.check_small_case(c, regime, run=_small_run(operand, which), operand=operand)
        assert not _bad(findings), f"{gc.small_case_id(c)}-{regime}\n" + gc.report(_bad(findings))


# ---------------------------------------------------------------------------------------------------------------------
# (b) planted defects fail
# ---------------------------------------------------------------------------------------------------------------------
PM, PN, PK = 1093, 512, 192         # four 256-row panels + a ragged fifth of 69 rows; two 256-column tiles; three K-tiles
# defect -> the epilogue it is planted in
NT_DEFECTS = {
    "fragment_of_the_ragged_last_tile_zero": "bf16", "last_k_tile_of_one_tile_dropped": "f32", "last_row_from_the_row_before": "gelu",
    "two_tail_sub_tiles_swapped": "resid_f32", "table_row_off_by_one_at_the_wrap": "resid_16.tab", "rowscale_on_bias2": "resid_f32",
    "bias_after_rounding": "bf16", "dgelu_from_gelu_table": "dgelu"}
ACC_DEFECTS = ("fragment_of_the_ragged_last_tile_zero", "last_k_tile_of_one_tile_dropped", "last_row_from_the_row_before",
               "two_tail_sub_tiles_swapped")


def _defective_acc(core, defect):
    acc = core["acc32"].clone()
    if defect == "fragment_of_the_ragged_last_tile_zero":          # rows 1024 .. 1039, columns 272 .. 287: its sum never happened
        acc[1024:1040, 272:288] = 0.0
    elif defect == "last_k_tile_of_one_tile_dropped":              # tile (panel 2, column tile 1)
        acc[512:768, 256:512] -= core["A"][512:768, PK - 64:] @ core["W"][256:512, PK - 64:].t()
    elif defect == "last_row_from_the_row_before":
        acc[PM - 1] = acc[PM - 2]
    elif defect == "two_tail_sub_tiles_swapped":                   # the 64-row sub-tiles 1 and 2 of tile (panel 3, column tile 0)
        acc[832:896, :256], acc[896:960, :256] = acc[896:960, :256].clone(), acc[832:896, :256].clone()
    return acc


def _nt_defect_run(operand, defect):
    def run(c, core, x):
        if defect in ACC_DEFECTS:
            return gc.nt_model(c, core, x, operand, acc=_defective_acc(core, defect)), []
        got = gc.nt_model(c, core, x, operand, defect=defect)
        return ({k: gc._rnd(v, operand) for k, v in got.items()} if defect == "bias_after_rounding" else got), []
    return run


@pytest.mark.parametrize("operand", OPERANDS, ids=IDS)
@pytest.mark.parametrize("defect", list(NT_DEFECTS))
def test_planted_nt_defects_fail(defect, operand):
    c = gc._nt(PM, PN, PK, NT_DEFECTS[defect])
    regimes = ("randn",) if defect in ("bias_after_rounding",) else ("randn", "exact", "hot")
    for regime in regimes:
        findings = gc.check_nt_case(c, regime, run=_nt_defect_run(operand, defect), operand=operand)
        assert _bad(findings), f"{defect} passes in {regime}\n" + gc.report(findings)


TM_, TN_, TK_ = 1569, 384, 256
TN_DEFECTS = ("one_splits_partial_dropped", "dbias_misses_the_last_slice", "beta_bias_takes_beta", "column_k_valid_written")


def _tn_defect_case(defect):
    if defect in ("beta_bias_takes_beta", "column_k_valid_written"):
        return gc._tn(TM_, TN_, TK_, None, into=(288, 255, 260), beta=0.5, beta_bias=1.0)
    return gc._tn(TM_, TN_, TK_, 5, beta=0.5, gexp=-3)             # five slices of 320 rows, the last one 289


def _tn_defect_run(operand, defect):
    def run(c, core, starts, splits):
        if defect != "column_k_valid_written":
            return gc.tn_expect(c, core, starts, splits, operand, defect=defect)[1], []
        got = gc.tn_expect(c, core, starts, splits, operand)[1]
        dW = gc.Guarded("dW", [c.n_valid], c.k_valid, torch.float32, c.ldw - c.k_valid)
        dW.seg(0).copy_(got["dW"])
        r0 = dW.rows[0][0]
        dW.buf[r0:r0 + c.n_valid, c.k_valid] = 0.0            # the reduce's `k + e < kv` guard is off by one
        return got, dW.check()
    return run


@pytest.mark.parametrize("operand", OPERANDS, ids=IDS)
@pytest.mark.parametrize("defect", TN_DEFECTS)
def test_planted_tn_defects_fail(defect, operand):
    c = _tn_defect_case(defect)
    for regime in ("randn", "exact"):
        findings = gc.check_tn_case(c, regime, run=_tn_defect_run(operand, defect), operand=operand, cus=32)
        assert _bad(findings), f"{defect} passes in {regime}\n" + gc.report(findings)


# ---------------------------------------------------------------------------------------------------------------------
# (c) what today's aggregate checks make of the same defects
# ---------------------------------------------------------------------------------------------------------------------
# defect -> (passes kernel_checks' formula with fp16 operands, with bf16 operands): `randn`, the planted geometry, ||x - ref|| / ||ref||
# over the whole tensor against TOL_BF16 (16-bit outputs) / 1e-4 (fp32 outputs, dW, dbias)
OLD_CHECKS_PASS = {
    "fragment_of_the_ragged_last_tile_zero": (False, False), "last_k_tile_of_one_tile_dropped": (False, False),
    "last_row_from_the_row_before": (False, False), "two_tail_sub_tiles_swapped": (False, False),
    "table_row_off_by_one_at_the_wrap": (False, False), "rowscale_on_bias2": (False, False), "bias_after_rounding": (True, True),
    "dgelu_from_gelu_table": (False, False), "one_splits_partial_dropped": (False, False), "dbias_misses_the_last_slice": (False, False),
    "beta_bias_takes_beta": (False, False), "column_k_valid_written": (True, True)}


def _old_formula(x, ref, bound):
    return gc.agg(x, ref) <= bound


def _old_nt(defect, operand):
    c = gc._nt(PM, PN, PK, NT_DEFECTS[defect])
    core, x = gc.nt_core(c.M, c.N, c.K, "randn", operand), gc.nt_extras(c, "randn", operand)
    got, _ = _nt_defect_run(operand, defect)(c, core, x)
    ref = gc.nt_epilogue(c, x, core["c64"])
    bound = 1e-4 if c.epi in gc.F32_OUT else gc.tol16(operand)
    return all(_old_formula(got[k], ref[k], bound) for k in got)


def _old_tn(defect, operand):
    c = _tn_defect_case(defect)
    splits = gc.tn_splits(c, 32)
    core = gc.tn_core(c.M, c.N, c.K, "randn", operand, gc.tn_slice_rows(c.M, splits))
    w0, b0 = gc.tn_starts(c.N, c.K, "randn", 0)
    starts = (w0[:c.n_valid, :c.k_valid].contiguous(), b0[:c.n_valid].contiguous())
    got, _ = _tn_defect_run(operand, defect)(c, core, starts, splits)
    ref = gc.tn_expect(c, core, starts, splits, operand)[0]
    return all(_old_formula(got[k], ref[k], 1e-4) for k in ("dW", "dbias"))


def test_what_the_aggregate_norm_lets_through_is_as_recorded():
    now = {d: tuple((_old_nt if d in NT_DEFECTS else _old_tn)(d, op) for op in OPERANDS) for d in OLD_CHECKS_PASS}
    assert now == OLD_CHECKS_PASS, now
    assert set(OLD_CHECKS_PASS) == set(NT_DEFECTS) | set(TN_DEFECTS)


# ---------------------------------------------------------------------------------------------------------------------
# (d) dispatch and case tables
# ---------------------------------------------------------------------------------------------------------------------
def _names(cases):
    return sorted({n for c in cases for n in c.kernel.split("+")})


def test_nt_tables_reach_exactly_these_kernels():
    assert _names(c for c, _ in gc.NT_TESTS) == sorted([
        "skinny<1>.ragged", "skinny<2>", "skinny<3>.ragged", "tile<2,2>", "tile<4,2>", "tile<2,5>", "tile<2,6>.n768", "tile<2,6>.m100k",
        "tile<4,4>.f4", "tile<4,4>.f2", "tile<4,4>.f1", "nt8.half_only", "nt8.full", "nt8.full_then_half", "nt8.oddk"])
    assert _names(c for c, _ in gc.LOW_NT_TESTS) == sorted([
        "tile<4,4>.f4", "tile<4,4>.f2", "tile<4,4>.f1", "nt8.full", "nt8.full_then_half", "nt8.walk", "nt8.oddk"])
    # every (family, epilogue) pair that exists runs `exact`; every family runs every regime
    fams, reg = {}, {}
    for c, r in gc.NT_TESTS:
        reg.setdefault(gc.nt_family(c.kernel), set()).add(r)
        if r == "exact":
            fams.setdefault(gc.nt_family(c.kernel), set()).add(c.epi)
    for fam in ("skinny", "tile<2,2>", "tile<4,2>", "tile<2,5>", "tile<2,6>", "tile<4,4>"):
        assert fams[fam] == set(gc.EPIS), (fam, fams[fam])
    assert fams["nt8"] == set(gc.EPIS) - {"resid_16.tab"}             # the fp32-table form lives in the one-tile kernel only (launch_nt)
    for fam in fams:
        assert reg[fam] == set(gc.REGIMES), (fam, reg[fam])


def test_nt_shapes_hold_their_edges():
    big = [s for s, _ in gc.NT_SHAPES if s[0] >= 4096]
    assert {(M - 4096) % 256 for M, _, _ in big} == {1, 37, 129, 255}
    assert all(256 <= N <= 1024 or N == 2816 for _, N, _ in big) and sum(N == 2816 for _, N, _ in big) == 1
    assert {K for _, _, K in big} == {64, 128, 192, 256}
    assert all(M * N <= 2e7 for (M, N, K), _ in gc.NT_SHAPES + gc.LOW_NT_SHAPES)
    assert (gc.NT_HUGE.M, gc.NT_HUGE.N, gc.NT_HUGE.K, gc.NT_HUGE.epi) == (100000, 384, 64, "f32")
    assert len(gc.BATCH_SHAPES) >= 13 and any(M % 128 for M, _, _ in gc.BATCH_SHAPES)
    # the restated plans at the shapes the names stand for
    assert gc.nt8_plan(3, 11, 32) == (32, 1, 34) and gc.nt8_plan(2, 11, 32) == (22, 0, 22)          # 4097 x 2816: a full round, then two half items
    assert gc.nt8_plan(3, 2, 4) == (4, 2, 8) and gc.nt8_plan(3, 4, 4) == (12, 0, 12)               # 4230 x 512 / x 1024 at 4 CUs
    assert gc.nt_tail_plan(3, 4, 32)[2] == 2 and gc.nt_tail_plan(2, 4, 32)[2] == 4 and gc.nt_tail_plan(5, 4, 32)[2] == 1
    assert gc.nt_tail_plan(5, 1, 4) == (4, 1, 4, 8) and gc.nt_tail_plan(3, 2, 4) == (4, 2, 2, 8)


def test_tn_tables_reach_exactly_these_kernels_and_hold_their_edges():
    assert sorted({c.kernel for c in gc.TN_CASES}) == sorted(
        ["tn<2,2>+reduce_small"] + [f"{k}+{r}" for k in ("tn<2,2>", "tn_rt8", "tn8")
                                    for r in ("reduce_into", "reduce_into.bias", "reduce_into.two_betas")] + ["tn_rt8+reduce", "tn8+reduce"])
    assert sorted({g.kernel for g in gc.GROUP_CASES}) == ["tn8_grouped+reduce_grouped", "tn_rt8_grouped+reduce_grouped"]
    assert any(len(g.probs) == 1 and g.probs[0][1] == 384 and g.kernel.startswith("tn_rt8_grouped") for g in gc.GROUP_CASES)
    plain = [c for c in gc.TN_CASES if not c.into]
    for k in ("tn<2,2>", "tn_rt8", "tn8"):
        mine = [c for c in plain if c.kernel.startswith(k + "+")]
        assert {c.M for c in mine} == {0, 1, 63, 64, 65, 333, 1569}, k
        assert any(c.splits is None for c in mine) and any(c.splits is not None and 0 < c.M // c.splits < 64 for c in mine), k
    assert any(c.splits == 1 for c in plain if c.kernel.startswith("tn_rt8")) and any(c.splits == 1 for c in plain if c.kernel.startswith("tn8"))
    assert any(c.N % 256 == 128 for c in plain if c.kernel.startswith("tn_rt8")) and any(c.K % 256 == 128 for c in plain if c.kernel.startswith("tn_rt8"))
    assert all(c.ldw > c.k_valid for c in gc.TN_CASES if c.into and c.k_valid < c.K)
    assert {c.beta for c in gc.TN_CASES} == {0.0, 0.5, 1.0} and {c.gexp for c in gc.TN_CASES} == {0, -3, 2}
    assert gc.tn_plan(1569, 256, 384, 32) == 24 and gc.tn_plan(333, 256, 256, 32) == 5 and gc.tn_plan(1569, 128, 128, 32) == 8
    assert gc.tn_plan(4230, 512, 256, 4) == 16 and gc.group_plan([(4230, 512, 256), (4230, 256, 512), (1569, 256, 256)], 4) == 19
    assert sorted({c.kernel for c in gc.LOW_TN_CASES}) == ["tn8+reduce", "tn_rt8+reduce"]


def test_fp32_kernel_tables_reach_exactly_these_kernels():
    assert sorted({c.kernel for c in gc.SMALL_CASES}) == sorted([
        "f32_small", "f32_small.split", "cls_gemm<MT1,KU6>", "cls_gemm<MT2,KU2>", "cls_gemm<MT3,KU1>", "cls_linear<MT1,KU1>",
        "cls_linear<MT1,KU2>", "cls_linear<MT1,KU2>.gelu", "cls_linear<MT2,KU1>.gelu", "cls_linear<MT2,KU6>", "cls_linear<MT3,KU2>.ksplit4",
        "cls_linear<MT3,KU2>.pass2", "cls_linear<MT3,KU2>.pass3.ksplit4.gelu"])
    assert gc.f32_small_plan(32, 64, 600) == (4, 160) and gc.f32_small_plan(5, 40, 32) == (1, 32)
    assert gc.f32_names(70, 130, 2048) == ["f32_small.split"]          # K % 128 == 0, but four K slices are not the cls kernel's shape
