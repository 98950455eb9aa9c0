"""The pooling-attention / rel-pos harness (tests/pool_attn_checks.py) tested without a GPU: the rounding model stands in for the kernel.

  - the rule is PASSABLE: `model_variant` (normalised P rounded, D from the unrounded o) stays within it in every regime for fp16 and
    bf16, and a second fp32 implementation of the rel terms (channels summed in reverse) passes the rel rule;
  - the rule BITES: defects planted at 2 x 4 heads, Lq = 2048, keys (2, 4, 4) (two dK / dV query slices) each fail the row rule; whether
    today's aggregate bound (mvit_checks.check_mvit_attention: 6e-3 / 1.5e-2) lets the defect through is recorded with each;
  - a wrong lse entry fails, and so does an lse left in the natural-log domain (the kernel's is base 2);
  - the dispatch restatement reaches exactly the hand-written list of instantiations.
"""
import pytest
import torch

import pool_attn_checks as pc

OPERANDS = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]


def _variant_run(operand):
    """stands in for the GPU in pc.check_case: the variant model's outputs in the kernels' output form"""
    def run(c, p):
        if c.kind == "attn":
            return pc.model_variant(p, c, operand), []
        osc = 1.0 / pc.SCALE
        start = [p["start_" + n] for n in ("Rh", "Rw", "Rt")]
        hi, lo = pc.rel_fwd_model(p, c, operand, osc, flip=True)
        alone = dict(hi=hi, lo=lo, **pc.rel_bwd_model(p, c, operand, p["drel_in"], p["dq0"], start, flip=True))
        chain = pc.chain_model(p, c, operand, variant=True)
        for i, n in enumerate(("dRh", "dRw", "dRt")):
            chain[n] = start[i] + chain[n]
        return alone, chain, []
    return run


@pytest.mark.parametrize("operand", OPERANDS, ids=IDS)
@pytest.mark.parametrize("shape", [(9, 1, 65, (1, 3, 5)), (3, 1, 130, (2, 15, 15)), (1, 1, 200, (7, 16, 14))], ids=["9x65", "3x130", "1x200"])
@pytest.mark.parametrize("regime", pc.REGIMES)
def test_another_implementation_of_the_contract_passes(regime, shape, operand):
    c = pc._attn(*shape)
    findings = pc.check_case(c, regime, run=_variant_run(operand), operand=operand)
    assert all(f.ok for f in findings), pc.report(findings)
    assert {f.tensor.split()[0] for f in findings} >= {"o", "dq", "dk", "dv", "drel", "delta", "lse"}


@pytest.mark.parametrize("operand", OPERANDS, ids=IDS)
@pytest.mark.parametrize("regime", pc.REGIMES)
def test_second_rel_implementation_and_chain_variant_pass(regime, operand):
    """the rel terms with the channels summed in reverse order pass the rel rule; the chain through the variant model passes too"""
    for c in (pc._rel(3, 3, (3, 4, 8), (3, 4, 2)), pc._rel(1, 2, (2, 24, 24), (2, 12, 12))):
        findings = pc.check_case(c, regime, run=_variant_run(operand), operand=operand)
        assert all(f.ok for f in findings), pc.case_id(c) + "\n" + pc.report(findings)
        names = " ".join(f.tensor for f in findings)
        for n in ("rel (decoded relp)", "rel_bwd dQ", "rel_bwd dRt", "chain o", "chain dq", "chain dk", "chain dv", "chain dRh"):
            assert n in names, n


def test_equal_keys_give_dq_equal_to_dO_on_patch_rows():
    c = pc._attn(2, 1, 65, (2, 4, 4))
    p = pc.make_problem(c, "equal", torch.float16)
    ref = pc.reference(p, c)
    assert (ref["dq"][:, :c.Lq] - p["do"][:, :c.Lq].double()).abs().max() < 1e-12 and ref["dq"][:, c.Lq].abs().max() < 1e-12
    assert ref["dk"].abs().max() > 1e-3 and ref["drel"].abs().max() > 1e-3          # v differs per key: these are not zero


# --- planted defects at 2 x 4, Lq = 2048, keys (2, 4, 4) --------------------------------------------------------------
BIG = pc._attn(2, 4, 2048, (2, 4, 4))
TENSORS = ("o", "dq", "dk", "dv", "drel")


@pytest.fixture(scope="module")
def big():
    assert BIG.kernel.endswith("bwd_kv1.z2")
    p = pc.make_problem(BIG, "randn", torch.float16)
    return p, pc.reference(p, BIG), pc.pool_model(p, BIG, torch.float16, keep_ds=True)


def _verdicts(p, ref, mod, x, t):
    """-> (row rule passes, today's aggregate bound passes) for tensor t"""
    row = pc.ac.judge_tensor(None, t, x, ref[t], mod[t], None, pc.AGG_BWD, where=pc._loc(BIG))[0]
    return row.ok, pc.agg(x, ref[t]) <= (pc.AGG_FWD if t == "o" else pc.AGG_BWD)


def test_the_model_itself_passes_and_is_far_inside_the_old_bounds(big):
    p, ref, mod = big
    for t in TENSORS:
        assert pc.agg(mod[t], ref[t]) < 1.5e-3, (t, pc.agg(mod[t], ref[t]))


def test_dropped_z_slice_fails(big):
    """the second of the two query slices (query tiles 33 .. 64 of 65) missing from dk of one item: 1/16 of the gradient's terms"""
    p, ref, mod = big
    ntiles = -(-(BIG.Lq + 1) // 32)
    q0 = -(-ntiles // 2) * 32
    item = 5
    part = pc.SCALE * (mod["ds"][item, q0:].t() @ p["q"][item, q0:])
    x = mod["dk"].clone()
    x[item] = pc._rnd(x[item] - part, torch.float16)
    row_ok, old_ok = _verdicts(p, ref, mod, x, "dk")
    assert not row_ok
    assert not old_ok          # recorded: half of one item's dk is 25 % of the norm here, the aggregate bound sees it too (8 items only)


def _zero_row(x):
    x[3, x.shape[1] // 2] = 0.0


def _item_101(x):
    x[6] *= 1.01


# Recorded with every defect: the tensors in which today's aggregate bound (6e-3 for o, 1.5e-2 for the gradients) lets it through while
# the row rule fails.  (This shape has 16,392 query rows but only 264 key rows, so one zeroed key row is 6 % of dk's norm.)
@pytest.mark.parametrize("name,plant,old_bound_passes", [("one_row_zeroed", _zero_row, {"dq", "drel"}),
                                                         ("one_item_scaled_by_1.01", _item_101, set(TENSORS))])
def test_local_defect_fails_the_row_rule(big, name, plant, old_bound_passes):
    p, ref, mod = big
    passed_old = set()
    for t in TENSORS:
        x = mod[t].clone()
        plant(x)
        row_ok, old_ok = _verdicts(p, ref, mod, x, t)
        assert not row_ok, f"{name} in {t} went unnoticed"
        passed_old |= {t} if old_ok else set()
    assert passed_old == old_bound_passes


@pytest.mark.parametrize("name,kw,tensors,old_bound_passes", [
    ("bias_of_one_key_from_its_neighbours_column", "E", ("o", "dq", "dk", "dv", "drel"), set()),
    ("cls_query_given_a_bias", dict(cls_bias=True), ("o", "dq", "dk", "dv"), {"dq", "dk"}),
    ("residual_q_added_to_the_cls_row", dict(cls_resid=True), ("o", "dq"), set())])
def test_structural_defect_fails_the_row_rule(big, name, kw, tensors, old_bound_passes):
    """`tensors`: those the defect reaches (the cls query's bias does not reach drel, its residual reaches o and dq only)"""
    p, ref, mod = big
    if kw == "E":
        E = pc.key_map(BIG.k_thw)
        E[9] = E[10]
        kw = dict(E_kernel=E)
    bad = pc.pool_model(p, BIG, torch.float16, **kw)
    passed_old = set()
    for t in tensors:
        row_ok, old_ok = _verdicts(p, ref, mod, bad[t], t)
        assert not row_ok, f"{name}: {t} went unnoticed"
        passed_old |= {t} if old_ok else set()
    assert passed_old == old_bound_passes


def test_unwritten_drel_column_fails(big):
    p, ref, mod = big
    x = mod["drel"].clone()
    x[2, 700, x.shape[-1] - 1] = float("nan")
    row_ok, old_ok = _verdicts(p, ref, mod, x, "drel")
    assert not row_ok and not old_ok          # recorded: a NaN also fails the aggregate norm


def test_wrong_lse_entry_and_natural_log_lse_fail():
    c = pc._attn(2, 1, 65, (2, 4, 4))
    p = pc.make_problem(c, "peaked", torch.float16)
    ref = pc.reference(p, c)
    where = pc._loc(c, "query")
    stored = ref["lse32"] / pc.LN2                      # what the kernel stores: base 2
    assert pc.ac.judge_lse(None, stored * pc.LN2, ref, None, where=where)[0].ok
    bad = stored.clone()
    bad[1, 40] += 2e-3
    f = pc.ac.judge_lse(None, bad * pc.LN2, ref, None, where=where)[0]
    assert not f.ok and "clip 1, head 0, query 40" in f.detail, pc.report([f])
    assert not pc.ac.judge_lse(None, ref["lse32"] * pc.LN2, ref, None, where=where)[0].ok          # a natural-log lse read as base 2


# every instantiation the cases are meant to reach, written out by hand from the launch lines of csrc/attn_pool.hip (pvrl_mvit_attn_fwd /
# _bwd: <1> for JP = 32, <2> for JP = 64; kv_splits) and csrc/mvit_rel.hip (pvrl_mvit_rel_fwd / _bwd; rel_axes).  The slice and chunk
# counts are run-time values: 1, 2, an uneven 3 and the clamp at 16 for the slices, 1, 2, 3 and 8 for the chunks.
EVERY_KERNEL = """
fwd1 fwd2 bwd_q1 bwd_q2 bwd_kv1.z1 bwd_kv1.z2 bwd_kv1.z3 bwd_kv1.z16 bwd_kv2.z1 bwd_kv2.z2
rel_fwd rel_bwd_q_lds rel_bwd_q_gather rel_table.c1 rel_table.c2 rel_table.c3 rel_table.c8
""".split()


def test_case_table_reaches_every_instantiation():
    reached = set()
    for c in pc.CASES:
        reached.update(c.kernel.split("+"))
    assert reached == set(EVERY_KERNEL), (sorted(set(EVERY_KERNEL) - reached), sorted(reached - set(EVERY_KERNEL)))
    by_kernel = {}
    for c, r in pc.TESTS:
        for k in c.kernel.split("+"):
            by_kernel.setdefault(k, set()).add(r)
    for c in pc.CASES:
        assert {(c, "randn"), (c, "peaked")} <= set(pc.TESTS)
    for k, regs in by_kernel.items():
        assert set(pc.REGIMES) <= regs, (k, regs)
    ids = [f"{pc.case_id(c)}-{r}" for c, r in pc.TESTS]
    assert len(set(ids)) == len(ids)


def test_dispatch_restatement_on_known_geometries():
    assert pc.attn_names(2047, (1, 3, 5))[2] == "bwd_kv1.z1" and pc.attn_names(2048, (1, 3, 5))[2] == "bwd_kv1.z2"
    assert pc.attn_names(32800, (1, 3, 5))[2] == "bwd_kv1.z16"
    assert pc.attn_names(130, (2, 15, 15))[0] == "fwd1" and pc.attn_names(130, (3, 15, 15))[0] == "fwd2"
    assert pc.rel_chunks(2, (2, 24, 24)) == (512, [1, 1, 3])              # 1152 queries per time coordinate: 512 + 512 + 128
    assert pc.rel_chunks(1, (1, 23, 25)) == (512, [1, 1, 2])              # 575: 512 + 63
    assert sum(pc.table_rows((1, 64, 64), (1, 4, 4))) == 255
    assert pc.rel_names(1, (1, 64, 64), (1, 4, 4), False)[1] == "rel_bwd_q_gather"
    assert pc.rel_names(2, (2, 6, 6), (2, 3, 3), True)[1] == "rel_bwd_q_gather" and pc.rel_names(2, (2, 6, 6), (2, 3, 3), False)[1] == "rel_bwd_q_lds"


def test_small_cases_are_run_on_enough_draws():
    for c in pc.CASES:
        Lk = c.k_thw[0] * c.k_thw[1] * c.k_thw[2]
        rows = c.B * c.H * (min(c.Lq, Lk) + 1)
        d = pc.n_draws(c)
        assert d == 1 if rows >= pc.MIN_ROWS else (rows * d >= pc.MIN_ROWS or d == 256), c


def test_token_major_layout_round_trips():
    x = torch.randn(6, 8, pc.D)
    t = pc.to_tok(x, 2, 3)
    assert t.shape == (2 * 7 + 2, 3 * pc.D) and torch.equal(pc.from_tok(t, 2, 3), x)
    assert torch.equal(t[7 + 2, pc.D:2 * pc.D], x[4, 2]) and torch.equal(t[14 + 1, 2 * pc.D:], x[5, 7])          # (b 1, h 1, q 2); cls of (b 1, h 2)
