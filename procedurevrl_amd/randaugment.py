"""RandAugment of the EPIC-Kitchens fine-tuning clips (reference: lib/datasets/autoaugment.py `rand_augment_transform`,
`RandAugment`, `AugmentOp`; called per decoded frame at lib/datasets/epickitchens.py:149-162).

As in the rest of the input pipeline (`transform.py`, `mixup.py`), the host only DRAWS: `clip_plan` makes the reference's
`random` / `np.random` calls in the reference's order and resolves every chosen op to numbers -- the six affine
coefficients PIL would compute, an enhance factor, a threshold -- into one descriptor per frame and layer (`pvrl_ra_desc`
of include/pvrl.h).  `pvrl_rand_augment_u8` does the pixel work on the decoded uint8 clip, bit-equal to PIL.

Kept on purpose, as the reference has them (every `AugmentOp.__call__` re-seeds `random` and `np.random` with the clip's
seed before its probability draw):
  * all ops of all frames of a clip see the same `random.random()`: either every chosen op applies or none does, and
    every applied op draws the same magnitude, sign and resample mode;
  * `RandAugment.__call__` picks its ops with `np.random.choice` on the global state: frame 0 draws from whatever state
    the process had, frames 1..T-1 right after `np.random.seed(seed)`, so they all get the same ops (frame 0 often not);
  * EK's "rand-m15-mstd0.5-inc1" draws its magnitude from gauss(15, 0.5) and clips it to 10: always the strongest
    setting (PosterizeIncreasing keeps 0 bits: a black frame; SolarizeIncreasing's threshold is 0: an invert);
  * `inc0` selects the increasing transforms too (the reference tests `bool("0")`);
  * after the last frame `np.random` is freshly seeded with `seed`, so the crop / scale / flip draws that follow are a
    function of `seed` as well (`epic_train_clip_draws`).
"""
import math
import random
import re
from collections import namedtuple

import numpy as np
import torch

from ._lib import header_constants, struct_dtype

# PVRL_RA_* of include/pvrl.h
(NONE, AFFINE, AUTOCONTRAST, EQUALIZE, INVERT, POSTERIZE, SOLARIZE, SOLARIZE_ADD, COLOR, CONTRAST, BRIGHTNESS, SHARPNESS,
 BILINEAR, BICUBIC) = (header_constants()["PVRL_RA_" + k] for k in (
    "NONE", "AFFINE", "AUTOCONTRAST", "EQUALIZE", "INVERT", "POSTERIZE", "SOLARIZE", "SOLARIZE_ADD", "COLOR", "CONTRAST", "BRIGHTNESS",
    "SHARPNESS", "BILINEAR", "BICUBIC"))       # the last two: PIL's Image.BILINEAR / Image.BICUBIC
NEEDS_STATS = (AUTOCONTRAST, EQUALIZE, CONTRAST)
GEOMETRIC = ('Rotate', 'ShearX', 'ShearY', 'TranslateXRel', 'TranslateYRel')

MAX_LEVEL = 10.
_FILL = (128, 128, 128)
_RANDOM_INTERPOLATION = (BILINEAR, BICUBIC)
EK_CONFIG = "rand-m15-mstd0.5-inc1"              # epickitchens.py:155

# The transforms in the order `np.random.choice` indexes them: (name, has an "...Increasing" variant, weight of the `w0`
# set).  Names, order and weights are the reference's; they decide which op a draw means.
_TRANSFORM_TABLE = (
    ('AutoContrast', False, .025), ('Equalize', False, .005), ('Invert', False, 0), ('Rotate', False, .3),
    ('Posterize', True, 0), ('Solarize', True, .005), ('SolarizeAdd', False, .005), ('Color', True, .025),
    ('Contrast', True, .005), ('Brightness', True, .005), ('Sharpness', True, .025), ('ShearX', False, .2),
    ('ShearY', False, .2), ('TranslateXRel', False, .1), ('TranslateYRel', False, .1))
RAND_TRANSFORMS = tuple(name for name, _, _ in _TRANSFORM_TABLE)
RAND_INCREASING_TRANSFORMS = tuple(name + 'Increasing' if inc else name for name, inc, _ in _TRANSFORM_TABLE)
_WEIGHT_SETS = {0: tuple(w for _, _, w in _TRANSFORM_TABLE)}

# One op of one frame.  `name`: the reference's transform name; `applied`: whether its probability draw let it run;
# `level_args`: what AugmentOp hands the op function (degrees, factor, pct, threshold, bits ...); `resample`: BILINEAR /
# BICUBIC for a geometric op, else None; `kind` / `args`: the PVRL_RA_* kind the kernel runs and its resolved numbers
# (AFFINE: PIL's six coefficients; enhance ops: the factor; POSTERIZE: bits; SOLARIZE: threshold; SOLARIZE_ADD: add, threshold).
RaOp = namedtuple("RaOp", "name applied level_args resample kind args")
_SKIPPED = (False, (), None, NONE, ())           # the RaOp fields of an op whose probability draw kept it from running


def _either_sign(v):
    """one `random.random()`: above one half the value changes sign"""
    return -v if random.random() > 0.5 else v


# How a strength in [0, 1] (level / MAX_LEVEL) becomes the op's argument.  A signed form draws its sign when it is called.
_STRENGTH_TO_ARG = {
    'Rotate': lambda s, hp: _either_sign(s * 30.),                                  # degrees
    'ShearX': lambda s, hp: _either_sign(s * 0.3),
    'TranslateXRel': lambda s, hp: _either_sign(s * hp.get('translate_pct', 0.45)),  # fraction of the frame's extent
    'Color': lambda s, hp: s * 1.8 + 0.1,                                           # blend factor 0.1 .. 1.9
    'ColorIncreasing': lambda s, hp: 1.0 + _either_sign(s * .9),                    # the same range, away from 1
    'Posterize': lambda s, hp: int(s * 4),                                          # bits kept
    'PosterizeIncreasing': lambda s, hp: 4 - int(s * 4),
    'Solarize': lambda s, hp: int(s * 256),                                         # threshold
    'SolarizeIncreasing': lambda s, hp: 256 - int(s * 256),
    'SolarizeAdd': lambda s, hp: int(s * 110),
}
for _like, _names in (('ShearX', ('ShearY',)), ('TranslateXRel', ('TranslateYRel',)), ('Color', ('Contrast', 'Brightness', 'Sharpness')),
                      ('ColorIncreasing', ('ContrastIncreasing', 'BrightnessIncreasing', 'SharpnessIncreasing'))):
    for _n in _names:
        _STRENGTH_TO_ARG[_n] = _STRENGTH_TO_ARG[_like]
_NO_ARG = ('AutoContrast', 'Equalize', 'Invert')


def rotate_matrix(degrees, width, height):
    """The output-to-input affine map of PIL's `Image.rotate(degrees)` (no `expand`, no `center`): a turn about the frame's
    centre with the sine and cosine rounded to 15 decimals.  None where PIL returns a copy (a multiple of 360).  PIL
    transposes instead for 180 degrees, and for 90 / 270 on a square frame; RandAugment's angles stay within +-30 degrees."""
    turn = degrees % 360.0
    if turn == 0:
        return None
    if turn == 180 or (turn in (90, 270) and width == height):
        raise NotImplementedError("PIL rotates by this angle with a transpose; RandAugment never asks for it")
    cx, cy = width / 2, height / 2
    rad = -math.radians(turn)
    cos, sin = round(math.cos(rad), 15), round(math.sin(rad), 15)
    # the centre maps to itself: rotate (-cx, -cy), then move back
    return (cos, sin, (cos * -cx + sin * -cy) + cx, -sin, cos, (-sin * -cx + cos * -cy) + cy)


def resolve_op(name, level_args, resample, width, height):
    """The RaOp of an APPLIED op: what the op functions of autoaugment.py:44-158 ask PIL for, given the arguments AugmentOp
    hands them (`level_args`), the resolved resample mode and the frame size"""
    level_args = tuple(level_args)
    base = name[:-len('Increasing')] if name.endswith('Increasing') else name
    kind, args = None, tuple(level_args)
    if base == 'Rotate':
        m = rotate_matrix(level_args[0], width, height)
        kind, args = (NONE, ()) if m is None else (AFFINE, m)
    elif base == 'ShearX':
        kind, args = AFFINE, (1, level_args[0], 0, 0, 1, 0)
    elif base == 'ShearY':
        kind, args = AFFINE, (1, 0, 0, level_args[0], 1, 0)
    elif base == 'TranslateXRel':
        kind, args = AFFINE, (1, 0, level_args[0] * width, 0, 1, 0)
    elif base == 'TranslateYRel':
        kind, args = AFFINE, (1, 0, 0, 0, 1, level_args[0] * height)
    elif base == 'Posterize':
        kind, args = (NONE, ()) if level_args[0] >= 8 else (POSTERIZE, (level_args[0],))
    elif base == 'Solarize':
        kind = SOLARIZE
    elif base == 'SolarizeAdd':
        kind, args = SOLARIZE_ADD, (level_args[0], 128)
    else:
        kind = {'AutoContrast': AUTOCONTRAST, 'Equalize': EQUALIZE, 'Invert': INVERT, 'Color': COLOR, 'Contrast': CONTRAST,
                'Brightness': BRIGHTNESS, 'Sharpness': SHARPNESS}[base]
    if name in GEOMETRIC:
        if resample not in (BILINEAR, BICUBIC):
            raise NotImplementedError(f"resample mode {resample}: the kernel interpolates bilinear (2) or bicubic (3)")
    else:
        resample = None
    return RaOp(name, True, level_args, resample, kind, tuple(args))


RaConfig = namedtuple("RaConfig", "magnitude num_layers transforms weights magnitude_std")
_SECTION = re.compile(r"(\D*)(\d.*)")
_SECTION_VALUE = {'m': int, 'n': int, 'w': int, 'mstd': float,
                  'inc': lambda digits: True}     # the reference tests the string's truth: "inc0" selects them too


def parse_config(config_str, hparams=None):
    """The `rand-...` grammar -> RaConfig.  Sections are separated by '-': `m` magnitude (default 10), `n` ops per frame
    (default 2), `mstd` standard deviation of the magnitude, `inc` the transforms that grow stronger with the magnitude,
    `w` the index of a weight set for the choice.  A section without a digit says nothing.  As in the reference a
    `magnitude_std` in `hparams` goes before `mstd`, and the weights are those of the plain names also under `inc`."""
    variant, *sections = config_str.split('-')
    if variant != 'rand':
        raise ValueError(f"{config_str!r} is no RandAugment config: it starts with {variant!r}, not 'rand'")
    found = {}
    for section in sections:
        m = _SECTION.match(section)
        if m is None:
            continue
        key, digits = m.groups()
        if key not in _SECTION_VALUE:
            raise ValueError(f"unknown RandAugment config section {section!r}")
        if key == 'mstd' and key in found:          # the first mstd holds, the last of every other key
            continue
        found[key] = _SECTION_VALUE[key](digits)
    weights = None
    if 'w' in found:
        if found['w'] not in _WEIGHT_SETS:
            raise ValueError(f"RandAugment weight set {found['w']}: there is only set 0")
        weights = np.asarray(_WEIGHT_SETS[found['w']], dtype=np.float64)
        weights = weights / np.sum(weights)
    return RaConfig(found.get('m', MAX_LEVEL), found.get('n', 2), RAND_INCREASING_TRANSFORMS if 'inc' in found else RAND_TRANSFORMS,
                    weights, (hparams or {}).get('magnitude_std', found.get('mstd', 0)))


def _draw_op(name, seed, conf, hparams, width, height):
    """One op call on one frame.  The order of the draws is the reference's: both generators are re-seeded, then one
    `random.random()` decides at probability one half whether the op runs at all; a running op draws its magnitude (where
    the config has a deviation), its sign (where it has one) and its resample mode (where it is geometric and
    `hparams['interpolation']` leaves a choice)."""
    if seed is not None:
        np.random.seed(seed)
        random.seed(seed)
    if random.random() > 0.5:
        return RaOp(name, *_SKIPPED)
    level = random.gauss(conf.magnitude, conf.magnitude_std) if conf.magnitude_std and conf.magnitude_std > 0 else conf.magnitude
    strength = min(MAX_LEVEL, max(0, level)) / MAX_LEVEL
    level_args = () if name in _NO_ARG else (_STRENGTH_TO_ARG[name](strength, hparams),)
    resample = None
    if name in GEOMETRIC:
        resample = hparams.get('interpolation', _RANDOM_INTERPOLATION)
        resample = int(random.choice(resample) if isinstance(resample, (list, tuple)) else resample)
    return resolve_op(name, level_args, resample, width, height)


class ClipPlan:
    """What RandAugment does to the T frames of one clip: `ops[t][l]` is the RaOp of frame t, layer l; `fill` the colour
    the geometric ops put where they read outside the frame."""

    def __init__(self, seed, ops, fill, width, height):
        self.seed, self.ops, self.fill = seed, ops, tuple(int(v) for v in fill)
        self.width, self.height = int(width), int(height)

    @property
    def num_frames(self):
        return len(self.ops)

    @property
    def num_layers(self):
        return len(self.ops[0]) if self.ops else 0

    @property
    def is_identity(self):
        return all(op.kind == NONE for fr in self.ops for op in fr)


def clip_plan(seed, T, width, height, config_str=EK_CONFIG, hparams=None):
    """The draws of `[rand_augment_transform(config_str, hparams, seed)(frame) for frame in frames]` for T frames of
    `width` x `height` pixels.  Frame 0's ops are chosen from the ambient `np.random` state.  `hparams` is only read."""
    hparams = {} if hparams is None else hparams
    conf = parse_config(config_str, hparams)
    ops = []
    for _ in range(int(T)):
        chosen = np.random.choice(len(conf.transforms), conf.num_layers, replace=conf.weights is None, p=conf.weights)
        ops.append([_draw_op(conf.transforms[int(i)], seed, conf, hparams, width, height) for i in chosen])
    return ClipPlan(seed, ops, hparams.get('img_mean', _FILL), width, height)


def identity_plan(T, width, height, num_layers=2):
    """a clip plan that leaves every frame as it is"""
    return ClipPlan(None, [[RaOp('none', *_SKIPPED)] * num_layers for _ in range(T)], _FILL, width, height)


DESC_DTYPE = struct_dtype("pvrl_ra_desc")


class RandAugPlan:
    """The clip plans of a batch: what `ops.rand_augment_u8` applies to uint8 [B, T, H, W, 3]."""

    def __init__(self, clips):
        clips = list(clips)
        assert clips, "an empty batch has no plan"
        c0 = clips[0]
        for c in clips:
            if (c.num_frames, c.num_layers, c.fill, c.width, c.height) != (c0.num_frames, c0.num_layers, c0.fill, c0.width, c0.height):
                raise ValueError("the clip plans of one batch share T, the layer count, the fill colour and the frame size")
        self.clips = clips
        self._dev = {}

    batch_size = property(lambda self: len(self.clips))
    num_frames = property(lambda self: self.clips[0].num_frames)
    num_layers = property(lambda self: self.clips[0].num_layers)
    fill = property(lambda self: self.clips[0].fill)
    width = property(lambda self: self.clips[0].width)
    height = property(lambda self: self.clips[0].height)

    @property
    def is_identity(self):
        return all(c.is_identity for c in self.clips)

    def descriptors(self):
        """`pvrl_ra_desc` [layers, B * T]: layer-major, so one layer's launch reads a contiguous run"""
        B, T, L = self.batch_size, self.num_frames, self.num_layers
        d = np.zeros((L, B * T), dtype=DESC_DTYPE)
        for b, clip in enumerate(self.clips):
            for t, frame in enumerate(clip.ops):
                for l, op in enumerate(frame):
                    e = d[l, b * T + t]
                    e["kind"] = op.kind
                    if op.kind == AFFINE:
                        e["resample"] = op.resample
                        e["c"] = op.args
                    elif op.kind in (COLOR, CONTRAST, BRIGHTNESS, SHARPNESS):
                        e["c"][0] = op.args[0]
                    elif op.kind in (POSTERIZE, SOLARIZE, SOLARIZE_ADD):
                        e["iarg"][:len(op.args)] = op.args
        return d

    def device_descriptors(self, device):
        """the descriptors on `device` (uploaded once per device, asynchronously from pinned memory)"""
        key = str(device)
        if key not in self._dev:
            host = torch.from_numpy(self.descriptors().view(np.uint8).reshape(-1))
            if torch.device(device).type == "cuda":
                host = host.pin_memory()
            self._dev[key] = host.to(device, non_blocking=True)
        return self._dev[key]


def ek_hparams(cfg):
    """what the EPIC-Kitchens training clips set (epickitchens.py:154-156): the fill colour is the rounded data mean.  The
    reference also passes a `translate_const`, which only the absolute translations would read; RandAugment has none."""
    return dict(img_mean=tuple(min(255, round(255 * x)) for x in cfg.DATA.MEAN))


def epic_train_clip_draws(cfg, T, H0, W0):
    """Every draw of one EPIC-Kitchens training clip of T decoded H0 x W0 frames, in the order of epickitchens.py:149-192:
    the seed, the RandAugment plan, then the scale / crop / flip of `spatial_sampling`.  -> (ClipPlan, (new_h, new_w, y_off, x_off, flip))"""
    from .transform import spatial_sampling_params
    seed = random.randint(0, 100000000)
    plan = clip_plan(seed, T, W0, H0, EK_CONFIG, ek_hparams(cfg))
    params = spatial_sampling_params(H0, W0, -1, cfg.DATA.TRAIN_JITTER_SCALES[0], cfg.DATA.TRAIN_JITTER_SCALES[1],
                                     cfg.DATA.TRAIN_CROP_SIZE, cfg.DATA.RANDOM_FLIP, cfg.DATA.INV_UNIFORM_SAMPLE)
    return plan, params
