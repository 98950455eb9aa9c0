"""Mixup / CutMix host side (procedurevrl_amd/mixup.py) against the reference's own lib/datasets/mixup.py, recorded in
tests/golden/mixup.pt: seeded the same way, the plan makes the same draws (lam, use_cutmix, cut box) in every mode; a numpy
float32 application of the plan reproduces the reference's mixed batch bit for bit (the arithmetic pvrl_mix_clips does), and
the plan's weights rebuild mixup_target's dense targets bit for bit -- int labels and the EPIC-Kitchens verb / noun dict."""
import numpy as np
import pytest
import torch

from mixup_checks import apply_plan_numpy, dense_target, fixture_input, fixture_plans, load_fixture
from procedurevrl_amd import mixup as mx

FX = load_fixture()
CASES = sorted(FX["cases"])


@pytest.mark.parametrize("name", CASES)
def test_plan_makes_the_reference_draws(name):
    mode = FX["cases"][name]["kwargs"]["mode"]
    B = FX["shape"][0]
    for c, plan in fixture_plans(FX, name):
        assert list(plan.partner) == list(range(B - 1, -1, -1))
        boxes = list(c["boxes"])
        lam_p, cut_p = c["params_lam"].numpy(), c["params_cutmix"].numpy()
        if mode == "batch":
            lam_p, cut_p = float(lam_p), bool(cut_p)
            if lam_p == 1.0:
                assert (plan.kind == mx.NONE).all() and not boxes
            elif cut_p:
                (box, lam_c), = boxes
                assert (plan.kind == mx.CUT).all() and (plan.box == np.array(box)).all()
                assert (plan.lam == np.float32(lam_c)).all()
            else:
                assert (plan.kind == mx.BLEND).all() and not boxes and (plan.lam == np.float32(lam_p)).all()
            lam = c["lam"]                      # what the reference handed mixup_target: a float
            assert (plan.lam == np.float32(lam)).all() and (plan.lam_partner == np.float32(1.0 - lam)).all()
        else:
            n = len(lam_p)
            assert n == (B if mode == "elem" else B // 2)
            for i in range(n):
                members = (i,) if mode == "elem" else (i, B - 1 - i)
                if lam_p[i] == 1.0:
                    want = mx.NONE
                elif cut_p[i]:
                    want = mx.CUT
                    box, _ = boxes.pop(0)       # the reference draws the boxes in clip order
                    for m in members:
                        assert list(plan.box[m]) == box, (name, i)
                else:
                    want = mx.BLEND
                for m in members:
                    assert plan.kind[m] == want, (name, i, plan.kind)
            assert not boxes
            lam = c["lam"].view(-1).numpy()     # the per-clip fp32 vector handed to mixup_target
            assert (plan.lam == lam).all() and (plan.lam_partner == (np.float32(1) - lam)).all()


def test_fixture_covers_every_mode_and_kind():
    seen = set()
    for name in CASES:
        for _, plan in fixture_plans(FX, name):
            seen.update((plan.mode, int(k)) for k in plan.kind)
    assert {(m, k) for m in ("batch", "pair", "elem") for k in (mx.NONE, mx.BLEND, mx.CUT)} <= seen | {("pair", mx.NONE)}


@pytest.mark.parametrize("name", CASES)
def test_numpy_application_of_the_plan_is_the_reference_mix_bit_for_bit(name):
    checked = 0
    for i, (c, plan) in enumerate(fixture_plans(FX, name)):
        if "out" not in c:
            continue
        got = apply_plan_numpy(fixture_input(FX, i).numpy(), plan)
        assert np.array_equal(got.view(np.int32), c["out"].numpy().view(np.int32)), (name, i)
        checked += 1
    if name in ("batch_ek", "pair_ek", "elem_ek"):
        assert checked


@pytest.mark.parametrize("name", CASES)
def test_plan_weights_rebuild_mixup_target(name):
    for c, plan in fixture_plans(FX, name):
        if "target" not in c:
            continue
        assert plan.on == pytest.approx(1 - FX["smoothing"] + FX["smoothing"] / FX["num_classes"], abs=0)
        assert torch.equal(dense_target(plan, c["labels"], FX["num_classes"]), c["target"])
        for k, width in mx.EPIC_WIDTHS.items():
            assert torch.equal(dense_target(plan, c["epic_labels"][k], width), c["epic_target"][k]), (name, k)


def test_epic_noun_targets_do_not_sum_to_one():
    """the reference quirk the loss kernel must carry: 300-wide noun one-hots with off = smoothing / NUM_CLASSES (10 here)"""
    c, plan = fixture_plans(FX, "batch_ek")[0]
    s = c["epic_target"]["noun"].double().sum(1)
    assert torch.allclose(s, torch.full_like(s, 0.9 + 300 * 0.1 / FX["num_classes"]), atol=1e-5)
    assert torch.allclose(c["epic_target"]["verb"].double().sum(1), torch.full_like(s, 0.9 + 97 * 0.1 / FX["num_classes"]), atol=1e-5)


def test_cut_box_slices_frames_and_rows_and_is_clamped():
    """drawn on (H, W) = (8, 12), applied to (T, H) = (4, 8): boxes reach past T and H in the fixture, and the clamped slice
    is what the reference mixed"""
    B, C, T, H, W = FX["shape"]
    over_t = over_h = False
    for name in CASES:
        for c, plan in fixture_plans(FX, name):
            for b in range(B):
                if plan.kind[b] == mx.CUT:
                    over_t |= plan.box[b][1] > T
                    over_h |= plan.box[b][3] > H
    assert over_t and over_h


@pytest.mark.parametrize("mode", ["batch", "pair", "elem"])
def test_odd_batch_raises(mode):
    with pytest.raises(AssertionError):
        mx.Mixup(mixup_alpha=0.1, cutmix_alpha=1.0, mode=mode).plan(5, (5, 3, 4, 8, 8))


def test_prob_zero_is_the_identity_with_smoothed_one_hots():
    np.random.seed(0)
    plan = mx.Mixup(mixup_alpha=0.1, cutmix_alpha=1.0, prob=0.0, num_classes=10).plan(4, (4, 3, 4, 8, 8))
    assert plan.is_identity and (plan.lam == 1).all() and (plan.lam_partner == 0).all()
    lab = torch.tensor([3, 1, 4, 1])
    assert torch.equal(dense_target(plan, lab, 10), torch.full((4, 10), 0.1 / 10).scatter_(1, lab.view(-1, 1), 0.9 + 0.1 / 10))


def test_descriptors_carry_the_plan():
    np.random.seed(4)
    plan = mx.Mixup(mixup_alpha=0.1, cutmix_alpha=1.0, mode="elem").plan(6, (6, 3, 8, 16, 16))
    d = plan.descriptors()
    assert d.dtype == np.int32 and d.shape == (6, 8)
    assert (d[:, 0] == plan.partner).all() and (d[:, 1] == plan.kind).all() and (d[:, 2:6] == plan.box).all()
    assert (d[:, 6].view(np.float32) == plan.lam).all() and (d[:, 7].view(np.float32) == plan.lam_partner).all()


def test_descriptor_bytes_are_the_header_layout():
    """the layout contract once more, outside the code under test: `pvrl_mix_desc` is {int32 partner, kind, t0, t1, h0, h1; float lam,
    lam_partner} and the kinds are the PVRL_MIX_* numbers of include/pvrl.h, written out here as literals"""
    import struct
    plan = mx.MixPlan("elem", np.array([3, 2, 1, 0], np.int32), np.array([mx.CUT, mx.BLEND, mx.NONE, mx.CUT], np.int32),
                      np.array([[1, 9, 2, 7], [0, 0, 0, 0], [0, 0, 0, 0], [4, 5, 0, 16]], np.int32),
                      np.array([0.75, 0.3, 1.0, 0.984375], np.float32), np.array([0.25, 0.7, 0.0, 0.015625], np.float32), 0.91, 0.01)
    want = (struct.pack("<6i2f", 3, 2, 1, 9, 2, 7, 0.75, 0.25) + struct.pack("<6i2f", 2, 1, 0, 0, 0, 0, 0.3, 0.7)
            + struct.pack("<6i2f", 1, 0, 0, 0, 0, 0, 1.0, 0.0) + struct.pack("<6i2f", 0, 2, 4, 5, 0, 16, 0.984375, 0.015625))
    d = plan.descriptors()
    assert d.dtype == np.int32 and d.shape == (4, 8) and d.tobytes() == want and len(want) == 4 * 32


def test_finetune_loss_under_mixup_needs_the_plan_and_num_seg_is_refused():
    from procedurevrl_amd import train_net as tn
    from procedurevrl_amd.config import get_cfg
    cfg = get_cfg()
    cfg.MIXUP.ENABLED = True
    with pytest.raises(NotImplementedError, match="mix="):
        tn.finetune_loss(torch.randn(4, 10), torch.randint(0, 10, (4,)), cfg)
    cfg.MODEL.NUM_SEG = 2
    with pytest.raises(NotImplementedError, match="NUM_SEG"):
        tn.check_mixup_cfg(cfg)
    cfg.MODEL.NUM_SEG = 0
    tn.check_mixup_cfg(cfg)
    cfg.MODEL.LOSS_FUNC = "smooth"                 # tools/train_net.py:126-143: `smooth` comes before MIXUP
    assert not tn.mixup_active(cfg)


def test_mixup_from_the_ek_config():
    from procedurevrl_amd.config import get_cfg
    from procedurevrl_amd.losses import SoftTargetCrossEntropy, get_loss_func
    cfg = get_cfg()
    cfg.merge_from_list(["MIXUP.ENABLED", "True", "MIXUP.ALPHA", "0.1", "MODEL.NUM_CLASSES", "97"])
    m = mx.mixup_from_cfg(cfg)
    assert (m.mixup_alpha, m.cutmix_alpha, m.cutmix_minmax, m.mix_prob, m.switch_prob, m.mode) == (0.1, 1.0, None, 1.0, 0.5, "batch")
    assert m.label_smoothing == 0.1 and m.num_classes == 97
    assert get_loss_func("soft_target_cross_entropy") is SoftTargetCrossEntropy
