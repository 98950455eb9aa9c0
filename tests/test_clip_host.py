"""Global-norm gradient clipping without a GPU: the config key reaches the optimiser, the slot-count query is a pure host function, and the
kernel checks of tests/clip_checks.py pass on a Python model of the two kernels and reject each planted defect."""
import pytest
import torch

import clip_checks as cc
import optim_checks as oc


def _model_and_cfg(extra=()):
    from test_host_logic import _small_model
    cfg, model = _small_model(text=False)
    cfg.merge_from_list(list(extra))
    return cfg, model


def test_key_defaults_to_off():
    from procedurevrl_amd.config import get_cfg
    from procedurevrl_amd.optimizer import construct_optimizer
    cfg = get_cfg()
    assert cfg.SOLVER.CLIP_GRAD_L2NORM == 0.0 and isinstance(cfg.SOLVER.CLIP_GRAD_L2NORM, float)
    cfg, model = _model_and_cfg()
    opt = construct_optimizer(model, cfg)
    assert opt.clip_grad_l2norm == 0.0
    assert "clip" not in " ".join(str(k) for k in opt.state_dict()["fused"]) and set(opt.state_dict()) == {"param_groups", "state", "fused"}


def test_key_reaches_the_optimiser_from_a_yaml_and_from_an_override(tmp_path):
    from procedurevrl_amd.config import get_cfg
    from procedurevrl_amd.optimizer import construct_optimizer
    y = tmp_path / "clip.yaml"
    y.write_text("SOLVER:\n  CLIP_GRAD_L2NORM: 1.0\n")
    cfg, model = _model_and_cfg()
    cfg.merge_from_file(str(y))
    assert construct_optimizer(model, cfg).clip_grad_l2norm == 1.0
    for text, want in (("0.5", 0.5), ("2", 2.0), ("1e-2", 1e-2)):               # `KEY VAL` strings, an int among them: the float default type-checks
        cfg, model = _model_and_cfg(["SOLVER.CLIP_GRAD_L2NORM", text])
        opt = construct_optimizer(model, cfg)
        assert opt.clip_grad_l2norm == want and isinstance(opt.clip_grad_l2norm, float)
    with pytest.raises(ValueError):
        get_cfg().merge_from_list(["SOLVER.CLIP_GRAD_L2NORM", "True"])
    opt.clip_grad_l2norm = 3.0                                                 # ... and can be set directly, as grad_scale is
    assert opt.clip_grad_l2norm == 3.0


def test_a_negative_value_is_refused():
    from procedurevrl_amd.optimizer import construct_optimizer
    cfg, model = _model_and_cfg(["SOLVER.CLIP_GRAD_L2NORM", "-1.0"])
    with pytest.raises(ValueError, match="CLIP_GRAD_L2NORM"):
        construct_optimizer(model, cfg)


@pytest.mark.parametrize("n", cc.NS + (0, -3, 2, 1025, cc.PASS, cc.PASS - 1, cc.PASS + 1024, 134_600_000))
def test_slot_count_query_runs_without_a_gpu(n):
    from procedurevrl_amd._lib import lib
    assert lib().call("pvrl_sumsq_slots", n) == cc.slots_model(n)


def test_slot_counts_are_what_the_paths_claim():
    assert [cc.slots_model(n) for n in cc.NS] == [1, 1, 1, 1, 1, 1, 1, 256, 2048]
    assert cc.slots_model(cc.PASS) == 2048 == cc.slots_model(cc.PASS + 5) and cc.slots_model(cc.PASS - 1024) == 2047
    ids = [cc.case_id(ns) for ns in cc.CASES]
    assert len(set(ids)) == len(ids)
    assert {i.rsplit("-", 1)[1] for i in ids[:-1]} == {"tail_only", "no_tail", "tail", "tail_on_second_pass", "loop_and_tail"}
    # what FusedOptimizer sizes its workspace by: the count is subadditive over unions of parameter spans (multiples of 64 elements)
    for a, b in ((64, 64), (64, 1024), (1088, 960), (cc.PASS, 64), (262144, 262144 + 64)):
        assert cc.slots_model(a + b) <= cc.slots_model(a) + cc.slots_model(b)


@pytest.mark.parametrize("ns", cc.CASES, ids=[cc.case_id(ns) for ns in cc.CASES])
@pytest.mark.parametrize("regime", cc.REGIMES)
def test_model_of_the_kernels_passes_the_kernel_checks(ns, regime):
    bad = [f for f in cc.check_case(ns, regime, run=cc.model_run()) if not f.ok]
    assert not bad, cc.report(bad)


PLANTED = [("norm_without_gscale", (1027,), "random", "norm"), ("norm_without_gscale", cc.MULTI, "large", "norm"),
           ("coef_not_clamped", (1027,), "random", "coef at max_norm"), ("coef_not_clamped", (5,), "zero", "coef at max_norm"),
           ("eps_dropped", (1027,), "random", "coef at max_norm"), ("eps_dropped", (1024,), "zero", "coef at max_norm"),
           ("tail_not_summed", (1027,), "random", "norm"), ("tail_not_summed", (3,), "small", "norm"),
           ("tail_not_summed", (262147,), "non_finite", "flag"), ("tail_not_summed", (cc.PASS + 5,), "large", "norm"),
           ("second_run_overwrites_first", cc.MULTI, "random", "norm"), ("second_run_overwrites_first", cc.MULTI, "small", "norm")]


@pytest.mark.parametrize("defect,ns,regime,word", PLANTED, ids=[f"{d}-{cc.case_id(ns)}-{r}" for d, ns, r, _ in PLANTED])
def test_planted_defect_is_caught(defect, ns, regime, word):
    bad = [f for f in cc.check_case(ns, regime, run=cc.model_run(defect)) if not f.ok]
    assert bad, f"{defect} was not caught on {cc.case_id(ns)}, {regime}"
    assert any(word in f.tensor for f in bad), cc.report(bad)
    print(f"defect {defect} on {cc.case_id(ns)}, {regime}: " + cc.report(bad[:1]))


def test_every_defect_is_planted_and_the_positions_cover_what_the_issue_names():
    assert {d for d, *_ in PLANTED} == set(cc.DEFECTS)
    assert cc.positions((1027,)) == [(0, 0), (0, 1024), (0, 1026)] and cc.positions((4,)) == [(0, 0), (0, 3)]
    pos = cc.positions(cc.MULTI)
    assert (0, 0) in pos and (0, 1026) in pos and {r for r, _ in pos} == {0, 1, 2} and (1, 2) in pos and (2, 262146) in pos


def test_reference_is_the_fp64_formula():
    xs = [torch.full((4,), 2.0 ** 70)]
    assert cc.ref_norm(xs, 0.25) == 2.0 ** 69                                   # 0.25 * sqrt(4 * 2^140): no overflow
    assert cc.ref_coef(2.0, 1.0) == 1.0 / (2.0 + 1e-6) and cc.ref_coef(0.5, 1.0) == 1.0 and cc.ref_coef(0.0, 1.0) == 1.0
    g = [torch.tensor([3.0, 4.0]) * 0.25]
    total, coef = cc.reference_clip_(g, 0.25, 0.625)                            # raw gradient (3, 4): norm 5 * 0.25
    assert total == 1.25 and abs(coef - 0.5) < 1e-6 and torch.allclose(g[0], torch.tensor([0.375, 0.5]), rtol=1e-6)
    c = oc.ADAM_CASES[0]
    assert cc.clipped_case(c).gscale == c.gscale * oc.f32(cc.CLIP)
