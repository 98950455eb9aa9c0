"""Shared pieces of the Mixup tests: the golden fixture (tests/golden/mixup.pt, written by golden/make_golden_mixup.py from
the reference's lib/datasets/mixup.py), a numpy float32 model of `pvrl_mix_clips` and the reference-semantics dense target."""
import os

import numpy as np
import torch

from procedurevrl_amd import mixup as mx

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mixup.pt")


def load_fixture():
    return torch.load(FIXTURE, weights_only=False)


def fixture_input(fx, call_index):
    """the batch the fixture's call `call_index` mixed (regenerated from its torch seed)"""
    torch.manual_seed(fx["x_seed"] + call_index)
    return torch.randn(fx["shape"])


def fixture_plans(fx, name):
    """[(call record, plan drawn by procedurevrl_amd.mixup with the case's seed)] for every recorded call of a case"""
    case = fx["cases"][name]
    m = mx.Mixup(label_smoothing=fx["smoothing"], num_classes=fx["num_classes"], **case["kwargs"])
    np.random.seed(case["seed"])
    return [(c, m.plan(fx["shape"][0], fx["shape"])) for c in case["calls"]]


def apply_plan_numpy(x, plan):
    """numpy float32 model of pvrl_mix_clips: two rounded products and a rounded sum per blended element, copies inside the
    cut box (sliced on the T and H axes, clamped by the slicing); every source is the unmixed batch"""
    x = np.asarray(x, dtype=np.float32)
    out = x.copy()
    for b in range(plan.batch_size):
        p = int(plan.partner[b])
        if plan.kind[b] == mx.BLEND:
            out[b] = x[b] * np.float32(plan.lam[b]) + x[p] * np.float32(plan.lam_partner[b])
        elif plan.kind[b] == mx.CUT:
            yl, yh, xl, xh = (int(v) for v in plan.box[b])
            out[b][:, yl:yh, xl:xh] = x[p][:, yl:yh, xl:xh]
    return out


def dense_target(plan, labels, width):
    """mixup_target's y1 * lam + y2 * (1 - lam) of the smoothed one-hots, in fp32 torch: [B, width]"""
    labels = torch.as_tensor(labels).long().view(-1).cpu()
    y1 = torch.full((labels.numel(), width), plan.off, dtype=torch.float32).scatter_(1, labels.view(-1, 1), plan.on)
    y2 = y1[torch.as_tensor(plan.partner).long()]
    return y1 * torch.from_numpy(plan.lam).view(-1, 1) + y2 * torch.from_numpy(plan.lam_partner).view(-1, 1)
