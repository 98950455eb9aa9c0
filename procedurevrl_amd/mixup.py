"""Mixup / CutMix of the fine-tuning loop (reference: lib/datasets/mixup.py `Mixup`, `mixup_target`; timm's
SoftTargetCrossEntropy; called at tools/train_net.py:137-143).

As in the input pipeline (`transform.py`), the host only DRAWS the random numbers -- the same `np.random` calls, in the same
order and with the same numpy scalar types, as the reference's `_params_per_batch`, `_params_per_elem`, `rand_bbox`,
`rand_bbox_minmax` and `cutmix_bbox_and_lam`, so a run seeded the same way mixes the same way -- into a `MixPlan` of one
descriptor per clip (`pvrl_mix_desc` of include/pvrl.h: partner, kind, cut box, the two weights).  `pvrl_mix_clips` applies
the plan in place on the GPU and `pvrl_soft_ce` synthesises the mixed targets from the hard labels and the plan.

Clip b is always mixed with clip B-1-b, and every mode reads only unmixed clips (the reference's `x.flip(0)` copy in 'batch'
mode, `x_orig` in 'pair' / 'elem').  Kept on purpose, as the reference has them:
  * the cut box is drawn on img_shape[-2:] = (H, W) but applied as `x[:, :, yl:yh, xl:xh]` to [B, C, T, H, W] clips, so it
    slices FRAMES and ROWS (clamped to T and H by the slicing) over all columns, and `lam` is corrected by the H * W area;
  * the EPIC-Kitchens targets are 97 / 300-wide one-hots with off = smoothing / MODEL.NUM_CLASSES, so noun rows need not
    sum to 1 (the loss kernel does not assume they do).
"""
import numpy as np
import torch

from ._lib import header_constants, struct_dtype

NONE, BLEND, CUT = (header_constants()["PVRL_MIX_" + k] for k in ("NONE", "BLEND", "CUT"))
EPIC_WIDTHS = {"verb": 97, "noun": 300}          # mixup_target's one-hot widths for the EPIC-Kitchens label dict


def _box_and_lam(img_shape, lam, minmax, correct_lam):
    """-> ((yl, yh, xl, xh), lam): the draws of `cutmix_bbox_and_lam` (count=None, margin 0).  `lam` keeps the type the caller
    gives it (a Python float in 'batch' mode, np.float32 in 'pair' / 'elem'): the box size is computed in that type."""
    img_h, img_w = img_shape[-2:]
    if minmax is not None:
        ch = np.random.randint(int(img_h * minmax[0]), int(img_h * minmax[1]), size=None)
        cw = np.random.randint(int(img_w * minmax[0]), int(img_w * minmax[1]), size=None)
        yl = np.random.randint(0, img_h - ch, size=None)
        xl = np.random.randint(0, img_w - cw, size=None)
        yh, xh = yl + ch, xl + cw
    else:
        r = np.sqrt(1 - lam)
        ch, cw = int(img_h * r), int(img_w * r)
        cy = np.random.randint(0, img_h, size=None)
        cx = np.random.randint(0, img_w, size=None)
        yl, yh = np.clip(cy - ch // 2, 0, img_h), np.clip(cy + ch // 2, 0, img_h)
        xl, xh = np.clip(cx - cw // 2, 0, img_w), np.clip(cx + cw // 2, 0, img_w)
    if correct_lam or minmax is not None:
        lam = 1. - (yh - yl) * (xh - xl) / float(img_h * img_w)
    return (int(yl), int(yh), int(xl), int(xh)), lam


class MixPlan:
    """What one Mixup call does to a batch of B clips.  Per clip b: `partner` (B-1-b), `kind` (NONE / BLEND / CUT), `box`
    (yl, yh, xl, xh as drawn: applied to the T and H axes), `lam` / `lam_partner` (fp32 weights of the clip and of its
    partner, in the blend and in the mixed target).  `on` / `off` are the smoothed one-hot values of `mixup_target`."""

    def __init__(self, mode, partner, kind, box, lam, lam_partner, on, off):
        self.mode = mode
        self.partner, self.kind, self.box = partner, kind, box
        self.lam, self.lam_partner = lam, lam_partner
        self.on, self.off = on, off
        self._dev = {}

    @property
    def batch_size(self):
        return len(self.kind)

    @property
    def is_identity(self):
        return not bool((self.kind != NONE).any())

    def descriptors(self):
        """int32 [B, 8]: the `pvrl_mix_desc` array, filled by field name and viewed as int32 (the two weights show as the
        bits of their fp32 values)."""
        d = np.zeros(self.batch_size, dtype=struct_dtype("pvrl_mix_desc"))
        d["partner"], d["kind"], d["lam"], d["lam_partner"] = self.partner, self.kind, self.lam, self.lam_partner
        d["t0"], d["t1"], d["h0"], d["h1"] = np.asarray(self.box).reshape(-1, 4).T
        return d.view(np.int32).reshape(self.batch_size, 8)

    def device_descriptors(self, device):
        """the descriptors on `device` (uploaded once per device, asynchronously from pinned memory)"""
        key = str(device)
        if key not in self._dev:
            host = torch.from_numpy(self.descriptors())
            if torch.device(device).type == "cuda":
                host = host.pin_memory()
            self._dev[key] = host.to(device, non_blocking=True)
        return self._dev[key]


class Mixup:
    """lib/datasets/mixup.py `Mixup` with the reference's constructor.  `plan(batch_size, img_shape)` makes the draws;
    `__call__(x)` draws for x's shape and mixes x in place on the GPU -> (x, plan).  An odd batch raises."""

    def __init__(self, mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch',
                 correct_lam=True, label_smoothing=0.1, num_classes=1000):
        self.mixup_alpha = mixup_alpha
        self.cutmix_alpha = cutmix_alpha
        self.cutmix_minmax = cutmix_minmax
        if cutmix_minmax is not None:
            assert len(cutmix_minmax) == 2
            self.cutmix_alpha = 1.0              # minmax forces cutmix on, as in the reference
        self.mix_prob = prob
        self.switch_prob = switch_prob
        self.label_smoothing = label_smoothing
        self.num_classes = num_classes
        if mode not in ("batch", "pair", "elem"):
            raise ValueError(f"MIXUP.MODE {mode!r}: expected 'batch', 'pair' or 'elem'")
        self.mode = mode
        self.correct_lam = correct_lam
        self.mixup_enabled = True

    def _no_mixer(self):
        raise AssertionError("One of mixup_alpha > 0., cutmix_alpha > 0., cutmix_minmax not None should be true.")

    def _draw_batch(self):
        """-> (lam, use_cutmix) of `_params_per_batch`: a Python float and a bool"""
        lam, use_cutmix = 1., False
        if self.mixup_enabled and np.random.rand() < self.mix_prob:
            both = self.mixup_alpha > 0. and self.cutmix_alpha > 0.
            if both:
                use_cutmix = np.random.rand() < self.switch_prob
                a = self.cutmix_alpha if use_cutmix else self.mixup_alpha
            elif self.mixup_alpha > 0.:
                a = self.mixup_alpha
            elif self.cutmix_alpha > 0.:
                use_cutmix, a = True, self.cutmix_alpha
            else:
                self._no_mixer()
            lam = float(np.random.beta(a, a))
        return lam, use_cutmix

    def _draw_elems(self, n):
        """-> (lam float32 [n], use_cutmix bool [n]) of `_params_per_elem`"""
        lam = np.ones(n, dtype=np.float32)
        use_cutmix = np.zeros(n, dtype=bool)
        if self.mixup_enabled:
            if self.mixup_alpha > 0. and self.cutmix_alpha > 0.:
                use_cutmix = np.random.rand(n) < self.switch_prob
                lam_cut = np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=n)
                lam_mix = np.random.beta(self.mixup_alpha, self.mixup_alpha, size=n)
                drawn = np.where(use_cutmix, lam_cut, lam_mix)
            elif self.mixup_alpha > 0.:
                drawn = np.random.beta(self.mixup_alpha, self.mixup_alpha, size=n)
            elif self.cutmix_alpha > 0.:
                use_cutmix = np.ones(n, dtype=bool)
                drawn = np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=n)
            else:
                self._no_mixer()
            lam = np.where(np.random.rand(n) < self.mix_prob, drawn.astype(np.float32), lam)
        return lam, use_cutmix

    def plan(self, batch_size, img_shape):
        """Draw the mix of a batch of `batch_size` clips of shape img_shape (only its last two sizes, (H, W), are read)."""
        B = int(batch_size)
        assert B % 2 == 0, 'Batch size should be even when using this'
        partner = (B - 1 - np.arange(B)).astype(np.int32)
        kind = np.full(B, NONE, dtype=np.int32)
        box = np.zeros((B, 4), dtype=np.int32)
        if self.mode == "batch":
            lam, use_cutmix = self._draw_batch()
            if lam != 1.:
                if use_cutmix:
                    b, lam = _box_and_lam(img_shape, lam, self.cutmix_minmax, self.correct_lam)
                    kind[:], box[:] = CUT, b
                else:
                    kind[:] = BLEND
            # the reference's weights: x * lam and x.flip(0) * (1. - lam), the complement taken in double, then fp32
            w = np.full(B, lam, dtype=np.float32)
            wp = np.full(B, 1. - lam, dtype=np.float32)
        else:
            n = B if self.mode == "elem" else B // 2
            lam_b, use_cutmix = self._draw_elems(n)
            for i in range(n):
                lam = lam_b[i]
                if lam == 1.:
                    continue
                members = (i,) if self.mode == "elem" else (i, B - 1 - i)
                if use_cutmix[i]:
                    b, lam = _box_and_lam(img_shape, lam, self.cutmix_minmax, self.correct_lam)
                    lam_b[i] = lam
                    for m in members:
                        kind[m], box[m] = CUT, b
                else:
                    for m in members:
                        kind[m] = BLEND
            if self.mode == "pair":
                lam_b = np.concatenate((lam_b, lam_b[::-1]))
            # per-clip weights: lam and (1 - lam), the complement taken in fp32 (the reference's float32 lam tensor)
            w = lam_b.astype(np.float32)
            wp = (np.float32(1) - w).astype(np.float32)
        off = self.label_smoothing / self.num_classes
        on = 1. - self.label_smoothing + off
        return MixPlan(self.mode, partner, kind, box, w, wp, on, off)

    def __call__(self, x):
        """x fp32 [B, C, T, H, W] on the GPU (or transform.DecodedClips, materialised first) -> (mixed x, plan)"""
        from . import ops
        plan = self.plan(x.shape[0], tuple(x.shape))
        return ops.mix_clips(x, plan), plan


def mixup_from_cfg(cfg):
    """tools/train_net.py:137-139: the Mixup the reference builds every iteration"""
    m = cfg.MIXUP
    minmax = list(m.CUTMIX_MINMAX) if m.CUTMIX_MINMAX is not None else None
    return Mixup(mixup_alpha=m.ALPHA, cutmix_alpha=m.CUTMIX_ALPHA, cutmix_minmax=minmax, prob=m.PROB,
                 switch_prob=m.SWITCH_PROB, mode=m.MODE, label_smoothing=0.1, num_classes=cfg.MODEL.NUM_CLASSES)

