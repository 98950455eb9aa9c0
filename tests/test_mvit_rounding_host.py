"""oracle/mvit_rounded_oracle.py and the rule of tests/mvit_rounding_checks.py, without a GPU: the model without rounding IS the fp32 oracle,
its variant passes the rule in both operand types, ROW_FACTOR covers the spread of model and variant, and every planted defect fails a named
finding.  `pytest -s` prints the spreads and the defect table recorded below and in mvit_rounding_checks' docstring.

Defects (a switch on the model that stands in for the HIP path; `fixture` case unless said; the stand-in runs every draw, as the engine
does).  value / bound of the NAMED finding under the defect, and the worst value / bound of today's flat bounds
(mvit_checks.small_golden_findings) on the same run -- below 1 there means the flat suite does not see the defect:
  defect                named finding (bound)                                         bf16   fp16    flat bf16  flat fp16
  x2_16bit              block 0 output: 16-bit-valued share (0.01)                    1.00   1.00    0.97       0.96
  rel_single            block 0 rel: zero-lo share (0.5)                              1.00   1.00    0.87       0.66
  table_grad_16bit      d blocks.1.attn.rel_pos_w: coarse share (0.05)                1.00   1.00    0.87       0.88
  dxn_16bit             block 3 dxn = dqkv W_qkv: 16-bit-valued share (0.01)          1.00   1.00    0.86       0.89
  droppath_after_cast   DropPath copies that are not R(factor x gradient) (0.01)      0.64   0.64    (**)       (**)
  stem_partial_16bit    d patch_embed.proj.weight: coarse share (0.05)                1.00   0.98    0.87       0.88
  resid_16bit           block 0 output error ratio (1.3)                              1.36   1.37    1.16 (*)   0.93
  no_grad_scale (down)  d blocks.1.attn.rel_pos_w: e / allowed (1)                    inert  2.09    -          0.88 (at k = 0)
What this says.  The size of the error resolves a whole class of 16-bit tensors that should be fp32 (resid_16bit) and a backward in the
wrong units (no_grad_scale, which only the 2^-12 / 2^12 cases see).  It does NOT resolve one more rounding of a tensor that already carries
some twenty-five per block: by their error alone the six single-site defects read 1.21 / 1.13 (x2_16bit, features ratio against 1.3),
1.06 / 0.96 (rel_single), and 0.31, 0.27, 0.25, 0.23 of the per-parameter bound (table_grad_16bit, dxn_16bit, droppath_after_cast,
stem_partial_16bit) -- less than the spread between two legitimate orders.  They are caught per site instead, by facts read off the path
itself (mvit_rounding_checks: `per site`), which a 16-bit tensor, a missing lo half, the factor behind the cast or a 16-bit accumulator
changes from ~0 to ~1.
(*) the whole stream in bf16 also trips the flat bound of one tensor (pool_q.weight, which the healthy model already fills to 0.87): for
resid_16bit the flat half is asserted in the fp16 flavour only.  (**) the flat bounds are written for the fixture's own inputs; the healthy
model on the `droppath` inputs already reads 1.5 (bf16) / 2.3 (fp16) by that formula, so that half is dropped for this defect alone.
"""
import pytest
import torch

import e2e_checks as ec
import mvit_checks as mc
import mvit_rounding_checks as rc
from attn_checks import ROW_FACTOR
from oracle import mvit_oracle as mo
from oracle import mvit_rounded_oracle as mro
from oracle import rounded_oracle as ro

OPERANDS = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]


def _step(fn, double=False, sites=False):
    g = rc.fixture()
    cast = (lambda t: t.double()) if double else (lambda t: t.clone())
    p = {k: cast(v).requires_grad_(True) for k, v in rc.state().items()}
    outs = []
    mro.SITES = sites
    try:
        feat = fn(p, cast(g["x"]), g["mvit"], block_outputs=outs)
        (feat * cast(g["gout"])).sum().backward()
    finally:
        mro.SITES = False
    return feat.detach(), [o.detach() for o in outs], {k: v.grad for k, v in p.items()}


def test_without_rounding_it_is_the_fp32_oracle():
    """OPERAND None: features, the four block outputs and all 105 gradients BIT-EQUAL to mvit_oracle on tests/golden/mvit_small.pt, which pins
    the new module to the reference through the existing golden"""
    assert ro.OPERAND is None and (ec.TOL_RATIO, ec.TOL_RATIO_GRAD) == (rc.TOL_RATIO, rc.TOL_RATIO_GRAD) == (1.3, 1.6)
    ref, got = _step(mo.forward_features), _step(mro.forward_features)
    assert torch.equal(got[0], ref[0])
    assert len(got[1]) == 4 and all(torch.equal(a, b) for a, b in zip(got[1], ref[1]))
    assert len(got[2]) == rc.N_PARAMS and len(rc.fixture()["grads"]) == 73
    assert [k for k in ref[2] if not torch.equal(got[2][k], ref[2][k])] == []


def test_custom_sites_without_rounding_compute_the_same_function():
    """the custom Functions (PoolLN, RelPair, PoolAttn, DQAdd) are by-passed above; forced on without rounding they order their sums
    differently (the softmax backward through D, the pool LayerNorm's backward from statistics, rel as a pair, table gradients item by item),
    so they are compared in fp64 at 1e-6 of each tensor's norm (observed 3e-15; in fp32 the same comparison reads 2e-6)"""
    ref, got = _step(mo.forward_features, double=True), _step(mro.forward_features, double=True, sites=True)
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-300))
    assert rel(got[0], ref[0]) < 1e-6 and all(rel(a, b) < 1e-6 for a, b in zip(got[1], ref[1]))
    top = max(float(v.norm()) for v in ref[2].values())
    for k, r in ref[2].items():
        assert float((got[2][k] - r).norm()) <= 1e-6 * float(r.norm()) + 1e-12 * top, k


def test_droppath_case_sits_on_both_sides_of_the_pruned_slice():
    dp = rc.inputs("droppath")["droppath"]
    assert dp[0] is None and all(d is not None for d in dp[1:])
    assert any((s == 0).any() and (s > 0).any() for d in dp[1:3] for s in d), "a middle block drops one clip and keeps another"
    for s in dp[-1]:                     # rs_a and rs_m of the last block: each drops a clip and keeps another
        assert bool((s == 0).any()) and bool((s > 0).any())
    assert not bool(((dp[-1][0] == 0) & (dp[-1][1] == 0)).any()), "every clip keeps one branch of the last block"


@pytest.mark.parametrize("operand", OPERANDS, ids=IDS)
def test_model_is_covariant_under_a_power_of_two(operand):
    """what lets the `down` / `up` cases reuse `fixture`'s oracle runs"""
    i = rc.inputs("fixture")
    a = rc.references("fixture", operand)["model"]
    for k in rc.K_OF.values():
        b = rc.oracle_step(i["x"], i["gout"] * 2.0 ** k, None, operand)
        assert [n for n in a["grads"] if not torch.equal(a["grads"][n] * 2.0 ** k, b["grads"][n])] == []


@pytest.mark.parametrize("base", ["fixture", "droppath"])
@pytest.mark.parametrize("operand", OPERANDS, ids=IDS)
def test_variant_passes_and_row_factor_covers_the_spread(operand, base):
    r = rc.references(base, operand)
    findings, table = rc.judge(base, operand, r["variant"], models=("model",))
    rc.report(f"variant as the HIP path, {base} {operand}", findings, table, top=3)
    assert rc.failures(findings) == []
    sp = rc.spreads(base, operand)
    print(f"[spread {base} {operand}] " + ", ".join(f"{s:.2f} {k}" for s, k, _, _ in sp[:3]))
    assert sp[0][0] <= ROW_FACTOR / 2, sp[:3]


# defect -> (case, substring of the finding that names the tensor, does the defect act in that flavour: {operand: bool}, is the flat half asserted)
BF, FP = torch.bfloat16, torch.float16
RESOLVED = {
    "resid_16bit": ("fixture", "block 0 output (", {BF: True, FP: True}, {BF: False, FP: True}),
    "no_grad_scale": ("down", "d blocks.1.attn.rel_pos_w: abs", {BF: False, FP: True}, {BF: False, FP: True}),
    "x2_16bit": ("fixture", "block 0 output: share", {BF: True, FP: True}, {BF: True, FP: True}),
    "rel_single": ("fixture", "block 0 rel:", {BF: True, FP: True}, {BF: True, FP: True}),
    "table_grad_16bit": ("fixture", "d blocks.1.attn.rel_pos_w: share", {BF: True, FP: True}, {BF: True, FP: True}),
    "dxn_16bit": ("fixture", "block 3 dxn = dqkv W_qkv:", {BF: True, FP: True}, {BF: True, FP: True}),
    "droppath_after_cast": ("droppath", "DropPath: largest share", {BF: True, FP: True}, {BF: False, FP: False}),
    "stem_partial_16bit": ("fixture", "d patch_embed.proj.weight: share", {BF: True, FP: True}, {BF: True, FP: True}),
}


@pytest.mark.parametrize("defect", sorted(RESOLVED))
@pytest.mark.parametrize("operand", OPERANDS, ids=IDS)
def test_planted_defect(operand, defect):
    assert set(RESOLVED) == set(rc.DEFECTS)
    case, named, resolved, flat_half = RESOLVED[defect]
    i = rc.inputs(case)

    def step(d, k=i["k"]):
        j = rc.inputs(rc.base_case(case), d)
        return rc.oracle_step(j["x"], j["gout"] * 2.0 ** k, j["droppath"], operand, defect=defect)
    got = rc.step_on_draws(step)
    findings, _ = rc.judge(case, operand, got)
    (label, v, b), = [f for f in findings if named in f[0]]
    flat = None
    if flat_half[operand]:          # today's flat bounds on the step the flat suite runs: the fixture's inputs at k = 0
        at0 = got if i["k"] == 0 else step(0, 0)
        flat = max(fv / fb for _, fv, fb in mc.small_golden_findings(rc.fixture(), at0["feat"], at0["grads"], f16=operand == torch.float16))
    print(f"[defect {defect} {operand}] {label}: {v:.2f} / {b:g}; flat bounds' worst value / bound: {flat if flat is None else round(flat, 2)}")
    if resolved[operand]:
        assert not v <= b, f"the rule does not fail {named} under {defect}"
    else:           # no_grad_scale with bf16 operands, which never scale: the switch is inert and the run is the healthy model's
        assert rc.failures(findings) == []
    if flat is not None:
        assert flat <= 1.0, "the defect does not stay under today's flat bounds"
