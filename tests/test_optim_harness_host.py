"""The optimiser-kernel harness (tests/optim_checks.py) without a GPU.  The derived bound is fair: two fp32 CPU restatements of each
update kernel (every operation rounded / every a * b + c contracted) and torch.optim itself (foreach=False: its own Tensor.lerp_,
addcmul_, addcdiv_) stay at ratio <= 1 on every case the GPU test runs.  It bites: every planted defect fails, and the table printed at
the end names the finding that caught it.  The case tables hold what they claim."""
import pytest

import optim_checks as oc

RATIOS = {}          # (entry, stand-in) -> worst |x - ref| / bound
DEFECTS = []         # (entry, defect, case id, finding, value, bound)


def _worst(findings):
    return max(f.value for f in findings if "/ bound" in f.tensor)


def _stand_ins(check, case, entry, table):
    for name, run in table:
        f = check(case, run=run)
        bad = [x for x in f if not x.ok]
        assert not bad, f"{name}\n" + oc.report(bad)
        RATIOS[(entry, name)] = max(RATIOS.get((entry, name), 0.0), _worst(f))
        assert _worst(f) <= 1.0, (name, _worst(f))          # the stand-ins stay below 1, not merely below 1 + 2^-10


ADAM_STAND_INS = [("model, every operation rounded", lambda c, q: (oc.adam_model(c, q, "plain"), [])),
                  ("model, every a * b + c contracted", lambda c, q: (oc.adam_model(c, q, "fma"), [])),
                  ("torch.optim", lambda c, q: (oc.adam_torch_optim(c, q), []))]
SGD_STAND_INS = [("model, every operation rounded", lambda c, q: (oc.sgd_model(c, q, "plain"), [])),
                 ("model, every a * b + c contracted", lambda c, q: (oc.sgd_model(c, q, "fma"), [])),
                 ("torch.optim", lambda c, q: (oc.sgd_torch_optim(c, q), []))]


@pytest.mark.parametrize("case", oc.ADAM_CASES, ids=[oc.adam_case_id(c) for c in oc.ADAM_CASES])
def test_adam_models_and_torch_optim_stay_inside_the_bound(case):
    _stand_ins(oc.check_adam_case, case, "adamw_step" if case.decoupled else "adam_step", ADAM_STAND_INS)


WIDE = [oc.AdamCase(1 << 18, regime, step, b1, 1e-2, gs, dec)
        for regime in ("randn", "eps_bound", "underflow", "cancel") for step, b1, gs, dec in ((1, 0.9, 1.0, 1), (2, 0.3, 0.25, 0),
                                                                                               (1000, 0.9, 0.25, 1), (100000, 0.3, 1.0, 0))
        if not (regime == "cancel" and (step == 1 or not dec))]


@pytest.mark.parametrize("case", WIDE, ids=[oc.adam_case_id(c) for c in WIDE])
def test_adam_bound_over_2_to_the_18_elements(case):
    _stand_ins(oc.check_adam_case, case, ("adamw_step" if case.decoupled else "adam_step") + " (2^18 elements)", ADAM_STAND_INS)


@pytest.mark.parametrize("case", oc.SGD_CASES, ids=[oc.sgd_case_id(c) for c in oc.SGD_CASES])
def test_sgd_models_and_torch_optim_stay_inside_the_bound(case):
    _stand_ins(oc.check_sgd_case, case, "sgd_step", SGD_STAND_INS)


def test_scan_and_grad_scale_models_pass():
    for n in oc.SCAN_NS:
        bad = [f for f in oc.check_scan_case(n, run=oc.scan_model) if not f.ok]
        assert not bad, oc.report(bad)
    for n in oc.GSB_NS:
        bad = [f for f in oc.check_gsb_case(n, run=oc.gsb_model) if not f.ok]
        assert not bad, oc.report(bad)


# ---------------------------------------------------------------------------------------------------------------------
# the rule bites
# ---------------------------------------------------------------------------------------------------------------------
def _adam_case(**kw):
    return next(c for c in oc.ADAM_CASES if all(getattr(c, k) == v for k, v in kw.items()))


ADAM_PLANTED = [("bias_correction_from_step_minus_1", dict(n=1027, regime="randn", step=2)),
                ("bias_correction_from_step_minus_1", dict(n=1027, regime="randn", step=1000)),
                ("w2_replaced_by_b2", dict(n=1027, regime="randn")),
                ("eps_inside_the_sqrt", dict(n=1027, regime="eps_bound")),
                ("eps_inside_the_sqrt", dict(n=1027, regime="randn")),
                ("coupled_decay_in_adamw_mode", dict(n=1027, regime="randn", decoupled=1, wd=1e-2)),
                ("gscale_after_the_weight_decay_term", dict(n=1027, regime="randn", decoupled=0, wd=1e-2, gscale=0.25)),
                ("tail_not_updated", dict(n=1027, regime="randn")),
                ("tail_not_updated", dict(n=1027, regime="underflow")),
                ("tail_updated_twice", dict(n=1027, regime="randn")),
                ("tail_not_updated", dict(n=3)), ("tail_updated_twice", dict(n=262147))]


def _caught(entry, defect, cid, findings, must_name=None):
    bad = [f for f in findings if not f.ok]
    assert bad, f"{defect} was not caught on {cid}"
    w = max(bad, key=lambda f: f.value / max(f.bound, 1e-300) if f.bound else f.value)
    if must_name is not None:
        assert any(must_name(f) for f in bad), oc.report(bad)
    DEFECTS.append((entry, defect, cid, w.tensor, w.value, w.bound))


@pytest.mark.parametrize("defect,where", ADAM_PLANTED, ids=[f"{d}-{'-'.join(f'{k}{v}' for k, v in w.items())}" for d, w in ADAM_PLANTED])
def test_adam_planted_defect_is_caught(defect, where):
    c = _adam_case(**where)
    f = oc.check_adam_case(c, run=lambda c, q: (oc.adam_model(c, q, "plain", defect), []))
    tail = (lambda f: f"worst element {c.n - c.n % 4}" in f.detail or f"worst element {c.n - 1}" in f.detail or
            f"worst element {c.n - 2}" in f.detail) if defect.startswith("tail") else None       # the finding names a tail element
    _caught("adam_step", defect, oc.adam_case_id(c), f, tail)


SGD_PLANTED = [("stride_of_half_the_grid", lambda c: c.n == oc.SGD_GRID + 259 and c.momentum != 0),
               ("stride_of_half_the_grid", lambda c: c.n == oc.SGD_GRID + 259 and c.momentum == 0),
               ("first_step_ignores_a_loaded_buffer", lambda c: c.n == 257 and c.momentum != 0 and not c.first and c.nesterov),
               ("first_step_ignores_a_loaded_buffer", lambda c: c.n == 257 and c.momentum != 0 and not c.first and not c.nesterov),
               ("nesterov_uses_buf_alone", lambda c: c.n == 257 and c.nesterov and c.first),
               ("nesterov_uses_buf_alone", lambda c: c.n == 257 and c.nesterov and not c.first)]


@pytest.mark.parametrize("defect,pick", SGD_PLANTED, ids=[f"{d}-{i}" for i, (d, _) in enumerate(SGD_PLANTED)])
def test_sgd_planted_defect_is_caught(defect, pick):
    c = next(c for c in oc.SGD_CASES if pick(c))
    f = oc.check_sgd_case(c, run=lambda c, q: (oc.sgd_model(c, q, "plain", defect), []))
    half = (lambda f: int(f.detail.split()[2]) >= oc.SGD_GRID // 2) if defect.startswith("stride") else None
    _caught("sgd_step", defect, oc.sgd_case_id(c), f, half)


def test_scan_and_grad_scale_planted_defects_are_caught():
    for defect, n, word in (("tail_not_scanned", 1027, "at index 1026"), ("tail_not_scanned", 3, "at index 2"),
                            ("tail_not_scanned", oc.SCAN_GRID + 5, f"at index {oc.SCAN_GRID + 4}"),
                            ("snan_with_a_zero_quiet_bit_missed", 1024, "0x7f800001")):
        f = oc.check_scan_case(n, run=lambda x, flag: oc.scan_model(x, flag, defect))
        _caught("nonfinite_flag_f32", defect, oc.scan_case_id(n), f, lambda f: word in f.tensor)
    for defect, n, word in (("S_from_ceil", 65, "S ("), ("inv_written_for_the_first_1024_slots_only", 1024, "inv slots"),
                            ("inv_written_for_the_first_1024_slots_only", 1, "inv slots"), ("nan_dropped_by_fmaxf", 63, "(nan)")):
        f = oc.check_gsb_case(n, run=lambda g, t, ninv: oc.gsb_model(g, t, ninv, defect))
        _caught("grad_scale_begin", defect, oc.gsb_case_id(n), f, lambda f: word in f.tensor)
        assert all(word in f.tensor for f in f if not f.ok), oc.report([f for f in f if not f.ok][:5])


# ---------------------------------------------------------------------------------------------------------------------
# the case tables
# ---------------------------------------------------------------------------------------------------------------------
def test_case_tables_hold_what_the_harness_claims():
    A, S = oc.ADAM_CASES, oc.SGD_CASES
    assert len(set(A)) == len(A) and len({oc.adam_case_id(c) for c in A}) == len(A) and len({oc.sgd_case_id(c) for c in S}) == len(S)
    for dec in (0, 1):
        assert {c.n for c in A if c.regime == "randn" and c.decoupled == dec} >= set(oc.ADAM_NS)
        assert {c.regime for c in A if c.n == 1027 and c.decoupled == dec} == set(oc.ADAM_REGIMES)
        for b1 in (0.9, 0.3):
            assert {c.step for c in A if c.beta1 == b1 and c.decoupled == dec} == set(oc.ADAM_STEPS), (dec, b1)
        assert {(c.wd, c.gscale) for c in A if c.decoupled == dec and c.regime == "randn"} == {(0.0, 1.0), (0.0, 0.25), (1e-2, 1.0), (1e-2, 0.25)}
    assert {oc.adam_path(n) for n in oc.ADAM_NS} == {"tail_only", "one_wg_no_tail", "one_wg_tail", "one_wg_tail_on_second_pass",
                                                    "256_wgs_tail_on_second_pass"}
    assert [oc.adam_path(n) for n in (1023, 1024, 1027)] == ["one_wg_tail", "one_wg_no_tail", "one_wg_tail_on_second_pass"]
    for c in A:          # the regimes are what their names say
        q, k = oc.make_adam_problem(c), oc._adam_k(c)
        gg = q["g"].double() * k.gscale
        if c.step == 1:
            assert not q["m"].any() and not q["v"].any()
        if c.regime == "eps_bound":
            assert float(q["v"].double().sqrt().max()) / k.bc2_sqrt < 1e-3 * k.eps and float(gg.abs().max()) < 1e-3 * k.eps
        if c.regime == "underflow":
            assert float((k.w2 * gg * gg).max()) < 2.0 ** -126 and float(q["v"].max()) < 2.0 ** -126
        if c.regime == "cancel":
            assert float(((gg - q["m"].double()).abs() / q["m"].double().abs()).max()) <= 4 * 2.0 ** -23
        if c.regime == "zero_grad_slots":
            assert c.n - c.n % 4 in range(*oc.ZERO_SLOTS[1]) and oc.ZERO_SLOTS[1][1] == c.n
    assert {c.n for c in S} == set(oc.SGD_PATHS)
    assert {(c.momentum, c.dampening, c.nesterov) for c in S if c.n > oc.SGD_GRID} == set(oc.SGD_CONFIGS)
    assert {(c.momentum, c.dampening, c.nesterov, c.first, c.gscale) for c in S if c.n == 257} == \
        {(m, d, n, f, g) for (m, d, n) in oc.SGD_CONFIGS for f in ((1, 0) if m else (0,)) for g in (1.0, 0.25)}
    for n in oc.SCAN_NS:
        pos = oc.scan_positions(n)
        assert 0 in pos and n - 1 in pos and (n < 4 or n - 4 in pos) and (n <= oc.SCAN_GRID or oc.SCAN_GRID in pos)
    assert any(n > oc.SCAN_GRID for n in oc.SCAN_NS)


def test_grad_scale_contract_in_exact_arithmetic():
    T = oc.GSB_TARGET
    assert oc.gsb_allowed(1.0, True, T) == {256.0, 128.0}                         # exactly a power of two: the seam
    assert oc.gsb_allowed(1.5, True, T) == {128.0}
    assert oc.gsb_allowed(1.0 + 2.0 ** -23, True, T) == {256.0, 128.0}
    assert oc.gsb_allowed(1.0 - 2.0 ** -24, True, T) == {256.0, 128.0}
    assert oc.gsb_allowed(1.0 + 2.0 ** -19, True, T) == {128.0}
    assert oc.gsb_allowed(1.0 - 2.0 ** -19, True, T) == {256.0}
    assert oc.gsb_allowed(0.0, True, T) == {2.0 ** 100} == oc.gsb_allowed(1e-35, True, T)
    assert oc.gsb_allowed(1.0, False, T) == {2.0 ** -100} == oc.gsb_allowed(3.3e38, True, T)
    for n in oc.GSB_NS:
        labels = [label for label, _, _ in oc.gsb_launches(n)]
        assert any("max_negative_in_the_last" in s for s in labels) and any("only_non_finite" in s for s in labels)
        assert any("thread_1023" in s for s in labels) == (n >= 1024)
        assert {ninv for _, _, ninv in oc.gsb_launches(n)} == set(oc.GSB_NINV)
    g = next(g for label, g, _ in oc.gsb_launches(40000) if "thread_1023" in label)
    assert int(g.abs().argmax()) % 1024 == 1023 and int(g.abs().argmax()) + 1024 >= 40000


def test_print_the_measured_ratios_and_the_defect_table():
    """(runs after the tests above: the figures quoted in the docstring of optim_checks.py)"""
    for (entry, name), r in sorted(RATIOS.items()):
        print(f"ratio {entry}, {name}: worst {r:.3f}")
        assert r <= 1.0
    for entry, defect, cid, tensor, value, bound in DEFECTS:
        print(f"defect {entry} {defect} on {cid}: {tensor}: {value:.3g} (bound {bound:.3g})")
    planted = {d for _, d, *_ in DEFECTS}
    if RATIOS:          # the whole module ran
        assert planted >= set(oc.ADAM_DEFECTS) | set(oc.SGD_DEFECTS) | set(oc.SCAN_DEFECTS) | set(oc.GSB_DEFECTS), planted
