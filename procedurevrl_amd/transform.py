"""Input side of the hot path: the reference's CPU workers normalise, rescale, crop and flip every
decoded clip in fp32 and ship 154 MB per 32-clip batch over PCIe (lib/datasets/howto100m.py:437-452,
lib/datasets/utils.py:110-160,309-326, lib/datasets/transform.py:8-191).  Here the host only DRAWS the random numbers
-- same numpy calls in the same order as the reference, so a seeded run picks the same crops -- and the decoded
uint8 frames (38 MB per batch) go to the GPU, where `pvrl_frames_u8_patchify` does normalise + bilinear short-side
rescale + crop + flip fused into the patch-embed im2col.
"""
import math

import numpy as np
import torch


def spatial_sampling_params(height, width, spatial_idx=-1, min_scale=256, max_scale=320, crop_size=224,
                            random_horizontal_flip=True, inverse_uniform_sampling=False):
    """The draws of utils.spatial_sampling (utils.py:110-160) for one clip of `height` x `width` frames.
    -> (new_h, new_w, y_off, x_off, flip).  Uses np.random exactly like transform.py:31-37,103-108,142."""
    assert spatial_idx in [-1, 0, 1, 2]
    # random_short_side_scale_jitter (transform.py:8-61)
    if inverse_uniform_sampling and spatial_idx == -1:
        size = int(round(1.0 / np.random.uniform(1.0 / max_scale, 1.0 / min_scale)))
    else:
        size = int(round(np.random.uniform(min_scale, max_scale)))
    new_h, new_w = height, width
    if not ((width <= height and width == size) or (height <= width and height == size)):
        new_w = new_h = size
        if width < height:
            new_h = int(math.floor((float(height) / width) * size))
        else:
            new_w = int(math.floor((float(width) / height) * size))
    if spatial_idx == -1:
        # random_crop (transform.py:84-118)
        y_off = x_off = 0
        if not (new_h == crop_size and new_w == crop_size):
            if new_h > crop_size:
                y_off = int(np.random.randint(0, new_h - crop_size))
            if new_w > crop_size:
                x_off = int(np.random.randint(0, new_w - crop_size))
        flip = 0
        if random_horizontal_flip:
            flip = int(np.random.uniform() < 0.5)      # horizontal_flip(0.5, ...) (transform.py:121-147)
    else:
        # uniform_crop (transform.py:150-191)
        y_off = int(math.ceil((new_h - crop_size) / 2))
        x_off = int(math.ceil((new_w - crop_size) / 2))
        if new_h > new_w:
            if spatial_idx == 0:
                y_off = 0
            elif spatial_idx == 2:
                y_off = new_h - crop_size
        else:
            if spatial_idx == 0:
                x_off = 0
            elif spatial_idx == 2:
                x_off = new_w - crop_size
        flip = 0
    if new_h < crop_size or new_w < crop_size:
        raise ValueError(f"rescaled frame {new_h}x{new_w} is smaller than the crop {crop_size}")
    return new_h, new_w, y_off, x_off, flip


class DecodedClips:
    """A batch of decoded clips waiting for the fused GPU input kernel: `frames` uint8 [B, T, H0, W0, 3] (decoder
    order, on the GPU), `params` int32 [B, 5] = (new_h, new_w, y_off, x_off, flip) per clip.  Quacks like the fp32
    tensor [B, 3, T, crop, crop] the reference's loader would have produced (`.shape`, `.device`, `.is_cuda`)."""

    def __init__(self, frames, params, mean, std, crop_size):
        assert frames.dtype == torch.uint8 and frames.dim() == 5 and frames.shape[-1] == 3
        self.frames = frames.contiguous()
        p = torch.as_tensor(params, dtype=torch.int32).reshape(-1, 5)
        assert p.shape[0] == frames.shape[0]
        self.params_host = p.cpu()
        self.params = p.to(frames.device)
        self.mean = [float(v) for v in mean]
        self.std = [float(v) for v in std]
        self.crop = int(crop_size)

    @property
    def shape(self):
        B, T = self.frames.shape[:2]
        return torch.Size((B, 3, T, self.crop, self.crop))

    @property
    def device(self):
        return self.frames.device

    @property
    def is_cuda(self):
        return self.frames.is_cuda

    def contiguous(self):
        return self

    def float(self):
        return self


def decoded_train_batch(cfg, frames_u8):
    """A training batch of decoded clips, uint8 [B, T, H0, W0, 3] -> DecodedClips, with the draws of the reference's
    loader made per clip in its order (lib/datasets/epickitchens.py:149-192).  With DATA.USE_RAND_AUGMENT every clip draws
    its seed, its RandAugment plan and then its scale / crop / flip (`randaugment.epic_train_clip_draws`), and the frames
    (on the GPU) are augmented by `ops.rand_augment_u8` before they are wrapped: augmented frames are just frames.
    Without it only `spatial_sampling_params` draws."""
    B, T, H0, W0, _ = frames_u8.shape
    d = cfg.DATA
    if d.USE_RAND_AUGMENT:
        from . import ops
        from .randaugment import RandAugPlan, epic_train_clip_draws
        draws = [epic_train_clip_draws(cfg, T, H0, W0) for _ in range(B)]
        frames_u8 = ops.rand_augment_u8(frames_u8, RandAugPlan([plan for plan, _ in draws]))
        params = [p for _, p in draws]
    else:
        params = [spatial_sampling_params(H0, W0, -1, d.TRAIN_JITTER_SCALES[0], d.TRAIN_JITTER_SCALES[1], d.TRAIN_CROP_SIZE,
                                          d.RANDOM_FLIP, d.INV_UNIFORM_SAMPLE) for _ in range(B)]
    return DecodedClips(frames_u8, params, d.MEAN, d.STD, d.TRAIN_CROP_SIZE)


class DecodedViews(DecodedClips):
    """Decoded clips that SHARE source slabs: `frames` uint8 [S, T, H0, W0, 3], `params` int32 [B, 5] and `src` int32 [B] with
    0 <= src[b] < S -- output clip b is `params[b]` applied to slab `src[b]` (the three spatial crops of a test view from one
    decoded copy).  `shape[0]` is B, the number of output clips; `ops.frames_u8_patchify` / `ops.frames_u8_to_f32` dispatch on
    the class to the `_views` kernels, which are bit-equal to the plain ones on `frames[src]`."""

    def __init__(self, frames, params, src, mean, std, crop_size):
        assert frames.dtype == torch.uint8 and frames.dim() == 5 and frames.shape[-1] == 3
        self.frames = frames.contiguous()
        p = torch.as_tensor(params, dtype=torch.int32).reshape(-1, 5)
        s = torch.as_tensor(src, dtype=torch.int32).reshape(-1)
        assert s.shape[0] == p.shape[0]
        self.params_host = p.cpu()
        self.params = p.to(frames.device)
        self.src_host = s.cpu()
        self.src = s.to(frames.device)
        self.mean = [float(v) for v in mean]
        self.std = [float(v) for v in std]
        self.crop = int(crop_size)

    @property
    def shape(self):
        return torch.Size((self.src_host.shape[0], 3, self.frames.shape[1], self.crop, self.crop))


def _test_crop_index(num_crops, clip_index):
    """lib/datasets/epickitchens.py:131-135: crop `index % 3` of three, the centre crop when there is one; anything else is
    left undefined by the reference."""
    if num_crops == 3:
        return clip_index % 3
    if num_crops == 1:
        return 1
    raise NotImplementedError(f"TEST.NUM_SPATIAL_CROPS = {num_crops}: the reference defines 1 and 3 (epickitchens.py:131-135)")


def decoded_test_views(cfg, frames_u8):
    """The test batch of decoded temporal views, uint8 [S, T, H0, W0, 3] (one slab per view) -> DecodedViews of
    S * TEST.NUM_SPATIAL_CROPS clips in the reference's index order: clip s * K + k is crop k of slab s
    (epickitchens.py:124-135 decodes the view once per crop; here the crops name the one uploaded slab).  The params are
    `spatial_sampling_params(H0, W0, k, c, c, c)` with c = DATA.TEST_CROP_SIZE, called per clip as the reference calls
    spatial_sampling: each call consumes one np.random.uniform draw even though min == max."""
    S, T, H0, W0, _ = frames_u8.shape
    K, c = int(cfg.TEST.NUM_SPATIAL_CROPS), int(cfg.DATA.TEST_CROP_SIZE)
    crops = [_test_crop_index(K, k) for k in range(K)]
    params = [spatial_sampling_params(H0, W0, k, c, c, c) for _ in range(S) for k in crops]
    src = [s for s in range(S) for _ in crops]
    return DecodedViews(frames_u8, params, src, cfg.DATA.MEAN, cfg.DATA.STD, c)


def decoded_test_batch(cfg, frames_u8, clip_index):
    """The one-slab-per-clip form of `decoded_test_views`, for a loader that already replicated the view per crop:
    uint8 [B, T, H0, W0, 3] and the B dataset indices -> DecodedClips, crop index `clip_index % K`."""
    B, T, H0, W0, _ = frames_u8.shape
    K, c = int(cfg.TEST.NUM_SPATIAL_CROPS), int(cfg.DATA.TEST_CROP_SIZE)
    idx = [int(i) for i in (clip_index.tolist() if torch.is_tensor(clip_index) else clip_index)]
    assert len(idx) == B
    params = [spatial_sampling_params(H0, W0, _test_crop_index(K, i), c, c, c) for i in idx]
    return DecodedClips(frames_u8, params, cfg.DATA.MEAN, cfg.DATA.STD, c)
