"""Shared pieces of the RandAugment tests: the golden fixture (tests/golden/randaug.pt and randaug_more.pt, written by
golden/make_golden_randaug.py from the reference's lib/datasets/autoaugment.py and the installed Pillow), the seeded inputs
it was recorded on, and a numpy model of every op that reproduces Pillow bit for bit: float64 (one rounding per
operation, no fused multiply-add) for the affine gathers and the AutoContrast table, float32 for `Image.blend` (whose
alpha is a C float), integers for the rest."""
import os

import numpy as np
import torch

from procedurevrl_amd import randaugment as ra

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "randaug.pt")
_FX = None


def load_fixture():
    global _FX
    if _FX is None:
        _FX = torch.load(FIXTURE, weights_only=False)
        more = torch.load(FIXTURE[:-3] + "_more.pt", weights_only=False)      # the second file of pixel cases
        assert more["pillow"] == _FX["pillow"]
        _FX["pixels"] = _FX["pixels"] + more["pixels"]
    return _FX


def make_input(content, height, width, seed, frames=3):
    """uint8 [frames, height, width, 3] test clip.  golden/make_golden_randaug.py imports this function, and the fixture
    stores a checksum of every input it was recorded on."""
    rng = np.random.RandomState(seed)
    if content == "noise":
        x = rng.randint(0, 256, size=(frames, height, width, 3))
    elif content == "ramp":
        yy, xx = np.mgrid[0:height, 0:width]
        x = np.stack([np.stack([(xx * 255) // max(1, width - 1) + 3 * f, (yy * 255) // max(1, height - 1),
                                ((xx + yy) * 255) // max(1, width + height - 2)], axis=-1) for f in range(frames)])
        x = np.clip(x + rng.randint(0, 3, size=x.shape), 0, 255)
    elif content == "narrow":
        x = rng.randint(60, 181, size=(frames, height, width, 3))
    elif content == "constchan":
        x = rng.randint(0, 256, size=(frames, height, width, 3))
        x[..., 1] = 77
    else:
        raise ValueError(content)
    return np.ascontiguousarray(x.astype(np.uint8))


def checksum(x):
    x = np.asarray(x, dtype=np.int64).reshape(-1)
    return int((x * (np.arange(x.size, dtype=np.int64) % 251 + 1)).sum())


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
def _affine(img, coef, resample, fill):
    """Pillow's ImagingGenericTransform with affine_transform and the bilinear / bicubic 8-bit filters (Geometry.c)"""
    H, W, _ = img.shape
    a, b, c, d, e, f = (np.float64(v) for v in coef)
    yy, xx = np.mgrid[0:H, 0:W]
    xin = xx + 0.5
    yin = yy + 0.5
    sx = a * xin + b * yin + c
    sy = d * xin + e * yin + f
    inside = (sx >= 0.0) & (sx < W) & (sy >= 0.0) & (sy < H)
    sx = sx - 0.5
    sy = sy - 0.5
    x0 = np.floor(sx).astype(np.int64)
    y0 = np.floor(sy).astype(np.int64)
    dx = (sx - x0)[..., None]
    dy = (sy - y0)[..., None]
    src = img.astype(np.float64)

    def at(yi, xi):
        return src[np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1)]

    if resample == ra.BILINEAR:
        def lerp(p, q, t):
            return p + (q - p) * t
        v = lerp(lerp(at(y0, x0), at(y0, x0 + 1), dx), lerp(at(y0 + 1, x0), at(y0 + 1, x0 + 1), dx), dy)
        out = v.astype(np.int64)                                         # (UINT8)v: in [0, 255], truncated
    else:
        def cubic(v1, v2, v3, v4, t):
            p1 = v2
            p2 = -v1 + v3
            p3 = 2 * (v1 - v2) + v3 - v4
            p4 = -v1 + v2 - v3 + v4
            return p1 + t * (p2 + t * (p3 + t * p4))
        rows = [cubic(at(y0 + j, x0 - 1), at(y0 + j, x0), at(y0 + j, x0 + 1), at(y0 + j, x0 + 2), dx) for j in (-1, 0, 1, 2)]
        v = cubic(rows[0], rows[1], rows[2], rows[3], dy)
        out = np.where(v <= 0.0, 0, np.where(v >= 255.0, 255, np.trunc(np.clip(v, 0, 255)))).astype(np.int64)
    out = np.where(inside[..., None], out, np.asarray(fill, dtype=np.int64))
    return out.astype(np.uint8)


def _histograms(img):
    return [np.bincount(img[..., ch].reshape(-1), minlength=256).astype(np.int64) for ch in range(3)]


def _luma(img):
    r, g, b = (img[..., ch].astype(np.int64) for ch in range(3))
    return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16            # Pillow's L24 rgb -> L conversion


def _autocontrast_lut(h):
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256)
    scale = np.float64(255.0) / np.float64(hi - lo)
    offset = np.float64(-lo) * scale
    v = np.arange(256, dtype=np.float64) * scale + offset
    return np.clip(np.trunc(v), 0, 255).astype(np.int64)


def _equalize_lut(h):
    nz = h[h != 0]
    if nz.size <= 1:
        return np.arange(256)
    step = int(nz.sum() - nz[-1]) // 255
    if not step:
        return np.arange(256)
    n = step // 2 + np.concatenate(([0], np.cumsum(h)[:-1]))
    return np.minimum(n // step, 255)                                   # Image.point clips the table to 8 bits


def _blend(deg, img, factor):
    """Image.blend(degenerate, image, factor) (Blend.c): alpha is a C float, so the product and the sum are float32"""
    alpha = np.float32(factor)
    d = deg.astype(np.int32)
    t = d.astype(np.float32) + alpha * (img.astype(np.int32) - d).astype(np.float32)
    return np.where(t <= 0.0, 0, np.where(t >= 255.0, 255, np.trunc(np.clip(t, 0, 255)))).astype(np.uint8)


def _smooth(img):
    """ImageFilter.SMOOTH: (1 1 1; 1 5 1; 1 1 1) / 13, rounded; the one-pixel border is copied"""
    H, W, _ = img.shape
    out = img.copy()
    if H < 3 or W < 3:
        return out
    s = img.astype(np.int64)
    acc = 4 * s[1:-1, 1:-1]
    for j in range(3):
        for i in range(3):
            acc = acc + s[j:H - 2 + j, i:W - 2 + i]
    out[1:-1, 1:-1] = ((2 * acc + 13) // 26).astype(np.uint8)            # floor(acc / 13 + 0.5), exactly
    return out


def apply_op(img, op, fill=(128, 128, 128)):
    """uint8 [H, W, 3] -> what Pillow returns for `op` (a randaugment.RaOp)"""
    k = op.kind
    if k == ra.NONE:
        return img.copy()
    if k == ra.AFFINE:
        return _affine(img, op.args, op.resample, fill)
    if k in (ra.AUTOCONTRAST, ra.EQUALIZE):
        make = _autocontrast_lut if k == ra.AUTOCONTRAST else _equalize_lut
        return np.stack([make(h)[img[..., ch]] for ch, h in enumerate(_histograms(img))], axis=-1).astype(np.uint8)
    if k in (ra.INVERT, ra.POSTERIZE, ra.SOLARIZE, ra.SOLARIZE_ADD):
        i = np.arange(256)
        if k == ra.INVERT:
            lut = 255 - i
        elif k == ra.POSTERIZE:
            lut = i & ~(2 ** (8 - op.args[0]) - 1)
        elif k == ra.SOLARIZE:
            lut = np.where(i < op.args[0], i, 255 - i)
        else:
            lut = np.where(i < op.args[1], np.minimum(255, i + op.args[0]), i)
        return lut[img].astype(np.uint8)
    if k == ra.COLOR:
        deg = np.repeat(_luma(img)[..., None], 3, axis=-1)
    elif k == ra.CONTRAST:
        L = _luma(img)
        mean = int(float(L.sum()) / L.size + 0.5)
        deg = np.full(img.shape, mean, dtype=np.int64)
    elif k == ra.BRIGHTNESS:
        deg = np.zeros(img.shape, dtype=np.int64)
    elif k == ra.SHARPNESS:
        deg = _smooth(img)
    else:
        raise ValueError(k)
    return _blend(deg, img, op.args[0])


def apply_clip_plan(frames, plan):
    """uint8 [T, H, W, 3] -> the clip after every layer of a randaugment.ClipPlan"""
    out = []
    for t in range(frames.shape[0]):
        img = np.ascontiguousarray(frames[t])
        for op in plan.ops[t]:
            img = apply_op(img, op, plan.fill)
        out.append(img)
    return np.stack(out)


def apply_plan(frames, plan):
    """uint8 [B, T, H, W, 3] -> numpy model of ops.rand_augment_u8 for a randaugment.RandAugPlan"""
    frames = np.asarray(frames)
    return np.stack([apply_clip_plan(frames[b], plan.clips[b]) for b in range(frames.shape[0])])
