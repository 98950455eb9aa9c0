"""Mixup / CutMix on the GPU: `pvrl_mix_clips` reproduces the reference's mixed batches (tests/golden/mixup.pt, written by
the reference's own lib/datasets/mixup.py) bit for bit in every mode and kind, the DecodedClips input path mixes what
frames_u8_to_f32 produces, `pvrl_soft_ce` (dense and synthesised targets) matches a float64 soft-target cross entropy, and
train() with MIXUP.ENABLED fine-tunes the EPIC-Kitchens heads on the mixed batches (tools/train_net.py:137-143)."""
import json

import numpy as np
import pytest
import torch

from mixup_checks import apply_plan_numpy, dense_target, fixture_input, fixture_plans, load_fixture
from procedurevrl_amd import mixup as mx

FX = load_fixture()
DEV = "cuda"


def _bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _soft_ce64(x, t):
    """timm SoftTargetCrossEntropy in float64: (loss, d loss / d x)"""
    x = x.detach().double().cpu().requires_grad_(True)
    loss = torch.sum(-t.double().cpu() * torch.log_softmax(x, dim=-1), dim=-1).mean()
    loss.backward()
    return loss.detach(), x.grad


def _close(got, want, rel=1e-5):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max()) <= rel * max(1.0, float(want.abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FX["cases"]))
def test_mix_clips_matches_the_reference_bit_for_bit(name):
    from procedurevrl_amd import ops
    for i, (c, plan) in enumerate(fixture_plans(FX, name)):
        x0 = fixture_input(FX, i)
        x = x0.to(DEV)
        out = ops.mix_clips(x, plan)
        torch.cuda.synchronize()
        assert out.data_ptr() == x.data_ptr()                         # in place
        if "out" in c:
            assert _bits_equal(out, c["out"]), (name, i)
        assert _bits_equal(out, torch.from_numpy(apply_plan_numpy(x0.numpy(), plan))), (name, i)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["batch", "pair", "elem"])
def test_mix_clips_scalar_path_and_untouched_pairs(mode):
    """W % 4 != 0 takes the scalar kernel; a pair whose descriptors are both NONE is left as it was"""
    from procedurevrl_amd import ops
    shape = (6, 3, 5, 9, 10)
    for seed in range(6):
        np.random.seed(seed)
        plan = mx.Mixup(mixup_alpha=0.3, cutmix_alpha=1.0, prob=0.7, mode=mode).plan(shape[0], shape)
        x0 = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
        x = ops.mix_clips(x0.to(DEV), plan)
        assert _bits_equal(x, torch.from_numpy(apply_plan_numpy(x0.numpy(), plan))), (mode, seed)
    with pytest.raises(Exception):
        ops.mix_clips(torch.zeros((5,) + shape[1:], device=DEV), plan)


@pytest.mark.gpu
def test_decoded_clips_are_materialised_then_mixed():
    from procedurevrl_amd import ops
    from procedurevrl_amd.transform import DecodedClips
    g = torch.Generator().manual_seed(5)
    B, T, H0, W0, crop = 4, 4, 20, 24, 16
    frames = torch.randint(0, 256, (B, T, H0, W0, 3), generator=g, dtype=torch.uint8).to(DEV)
    params = [[20, 24, 1, 3, 0], [20, 24, 4, 0, 1], [20, 24, 0, 8, 1], [20, 24, 2, 5, 0]]
    clips = DecodedClips(frames, params, [0.45, 0.45, 0.45], [0.225, 0.225, 0.225], crop)
    for mode, seed in (("batch", 3), ("elem", 31), ("pair", 21)):
        np.random.seed(seed)
        plan = mx.Mixup(mixup_alpha=0.1, cutmix_alpha=1.0, mode=mode).plan(B, clips.shape)
        want = ops.mix_clips(ops.frames_u8_to_f32(clips), plan)
        got = ops.mix_clips(clips, plan)
        assert got.shape == (B, 3, T, crop, crop) and got.dtype == torch.float32
        assert _bits_equal(got, want), mode


def _targets(c):
    """(labels, dense fixture target, width) of the int and the EPIC verb / noun labels of a fixture call"""
    yield c["labels"], c["target"], FX["num_classes"]
    for k, width in mx.EPIC_WIDTHS.items():
        yield c["epic_labels"][k], c["epic_target"][k], width


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["batch_ek", "batch_prob", "pair_minmax", "elem_ek", "elem_prob"])
def test_soft_target_cross_entropy_matches_float64(name):
    from procedurevrl_amd.losses import SoftTargetCrossEntropy
    loss_fn = SoftTargetCrossEntropy()
    g = torch.Generator().manual_seed(17)
    n = 0
    for c, plan in fixture_plans(FX, name):
        if "target" not in c:
            continue
        for labels, target, width in _targets(c):
            x0 = 3.0 * torch.randn(len(labels), width, generator=g)
            want_loss, want_grad = _soft_ce64(x0, target)
            for form in ("dense", "synthesised"):
                x = x0.to(DEV).requires_grad_(True)
                if form == "dense":
                    loss = loss_fn(x, target.to(DEV))
                else:
                    loss = loss_fn(x, labels=labels.to(DEV), plan=plan)
                (2.0 * loss).backward()                              # the incoming gradient scales dx
                assert _close(loss, want_loss), (name, width, form, float(loss), float(want_loss))
                assert _close(x.grad, 2.0 * want_grad), (name, width, form)
                n += 1
    assert n >= 6


@pytest.mark.gpu
def test_soft_target_cross_entropy_wide_rows_and_unnormalised_targets():
    """K > the 256 threads of a row, targets summing to S != 1 (the gradient is S * softmax - t)"""
    from procedurevrl_amd.losses import SoftTargetCrossEntropy
    g = torch.Generator().manual_seed(3)
    for rows, K in ((3, 1000), (8, 300), (5, 7)):
        x0 = 2.0 * torch.randn(rows, K, generator=g)
        t = torch.rand(rows, K, generator=g) ** 4
        t = t / t.sum(1, keepdim=True) * torch.linspace(0.5, 3.0, rows).view(-1, 1)
        x = x0.to(DEV).requires_grad_(True)
        loss = SoftTargetCrossEntropy()(x, t.to(DEV))
        loss.backward()
        want_loss, want_grad = _soft_ce64(x0, t)
        assert _close(loss, want_loss) and _close(x.grad, want_grad), (rows, K)


def _mixup_run(tmp_path, capsys, monkeypatch, extra):
    """train() on EPIC-Kitchens labels with MIXUP.ENABLED; records every step's mix (inputs before / after, plan) and loss inputs"""
    from procedurevrl_amd import train_net as tn
    from test_train_loop_gpu import _finetune_cfg
    cfg = _finetune_cfg(tmp_path, "Epickitchens")
    cfg.merge_from_list(["MIXUP.ENABLED", "True", "MIXUP.ALPHA", "0.1", "LOG_PERIOD", "1", "TRAIN.EVAL_PERIOD", "100",
                         "SOLVER.MAX_EPOCH", "3", "RNG_SEED", "3"] + extra)
    steps = []
    real_from_cfg, real_loss = tn.mixup_from_cfg, tn.finetune_loss

    def from_cfg(c):
        m = real_from_cfg(c)

        def call(x):
            before = x.detach().clone()
            out, plan = m(x)
            steps.append({"before": before.cpu(), "after": out.detach().clone().cpu(), "plan": plan})
            return out, plan
        return call

    def loss(pred, labels, c, mix=None):
        steps[-1].update(pred=[p.detach().clone().cpu() for p in pred], labels={k: v.cpu() for k, v in labels.items()}, mix=mix)
        return real_loss(pred, labels, c, mix=mix)

    monkeypatch.setattr(tn, "mixup_from_cfg", from_cfg)
    monkeypatch.setattr(tn, "finetune_loss", loss)
    torch.manual_seed(0)
    tn.train(cfg)
    out = capsys.readouterr().out
    lines = [json.loads(l.split("json_stats: ", 1)[1]) for l in out.splitlines() if "json_stats: " in l and '"train_iter"' in l]
    return cfg, steps, lines


def _step_loss64(cfg, s, targets):
    lv, _ = _soft_ce64(s["pred"][0], targets["verb"])
    ln, _ = _soft_ce64(s["pred"][1], targets["noun"])
    return float(0.5 * (lv + ln))


@pytest.mark.gpu
def test_train_with_mixup_on_epic_kitchens(tmp_path, capsys, monkeypatch):
    cfg, steps, lines = _mixup_run(tmp_path, capsys, monkeypatch, [])
    assert len(steps) == len(lines) == 6                                  # 3 epochs x 2 iterations, one line each
    assert all(np.isfinite(l["loss"]) for l in lines)
    for key in ("verb_loss", "noun_loss", "verb_top1_acc", "noun_top5_acc", "top1_acc", "top5_acc"):
        assert key in lines[-1]
    # train() seeds np.random with RNG_SEED: the plans are the draws of a Mixup seeded the same way, step after step
    np.random.seed(cfg.RNG_SEED)
    m = mx.mixup_from_cfg(cfg)
    for s in steps:
        p = m.plan(s["before"].shape[0], tuple(s["before"].shape))
        assert s["mix"] is s["plan"]
        assert (p.kind == s["plan"].kind).all() and (p.box == s["plan"].box).all() and (p.lam == s["plan"].lam).all()
        assert _bits_equal(s["after"], torch.from_numpy(apply_plan_numpy(s["before"].numpy(), s["plan"])))
    assert any(not s["plan"].is_identity for s in steps)
    # the logged loss of a pinned step = the float64 soft-target CE of its logits against the reference-semantics targets
    for k in (2, 5):
        s = steps[k]
        t = {name: dense_target(s["plan"], s["labels"][name], w) for name, w in mx.EPIC_WIDTHS.items()}
        want = _step_loss64(cfg, s, t)
        assert abs(lines[k]["loss"] - want) <= 1e-5 * max(1.0, abs(want)) + 5e-6, (k, lines[k]["loss"], want)


@pytest.mark.gpu
def test_train_with_mixup_prob_zero_leaves_inputs_and_smooths_targets(tmp_path, capsys, monkeypatch):
    cfg, steps, lines = _mixup_run(tmp_path, capsys, monkeypatch, ["MIXUP.PROB", "0.0"])
    assert len(steps) == len(lines) == 6
    off = 0.1 / cfg.MODEL.NUM_CLASSES
    for k, s in enumerate(steps):
        assert s["plan"].is_identity and _bits_equal(s["after"], s["before"])
        t = {name: torch.full((len(s["labels"][name]), w), off).scatter_(1, s["labels"][name].view(-1, 1).long(), 0.9 + off)
             for name, w in mx.EPIC_WIDTHS.items()}
        want = _step_loss64(cfg, s, t)
        assert abs(lines[k]["loss"] - want) <= 1e-5 * max(1.0, abs(want)) + 5e-6, (k, lines[k]["loss"], want)
