"""Generate tests/golden/randaug.pt and randaug_more.pt by running the UNMODIFIED reference RandAugment (lib/datasets/autoaugment.py) on the
installed Pillow.

Run where a reference checkout is available (PVRL_REFERENCE_DIR, default ../reference next to this repository):
    python tests/golden/make_golden_randaug.py
The module is loaded from its file as it is; nothing of its source is copied, only recorded draws and outputs are stored
(and the Pillow version that computed them).  The draws are recorded by wrapping, on the loaded module, what the reference
calls: `AugmentOp.__call__` (which op was chosen), the op functions of `NAME_TO_OP` (the arguments an applied op was given)
and `_interpolation` (the resample mode it resolved to); their behaviour is untouched.

  ek        256 consecutive EPIC-Kitchens training clips of T = 3 after random.seed(0); np.random.seed(0), in the order of
            lib/datasets/epickitchens.py:149-192: the seed, the per-frame op calls, then the draws of spatial_sampling
            (the reference's lib/datasets/transform.py functions, in the order lib/datasets/utils.py:143-152 calls them).
  configs   a few clips for other config strings
  pixels    every op through the reference's AugmentOp on seeded inputs (tests/randaug_checks.py `make_input`, not
            stored: only a checksum is), at magnitude 10 (both signs, both resample modes) and at a mid magnitude
  layers    two ops in a row
"""
import importlib.util
import os
import random
import sys

import numpy as np
import PIL
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("PVRL_REFERENCE_DIR", os.path.join(ROOT, "..", "reference"))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from randaug_checks import checksum, make_input  # noqa: E402

EK_CONFIG = "rand-m15-mstd0.5-inc1"                      # epickitchens.py:155
EK = dict(T=3, H0=36, W0=48, mean=[0.45, 0.45, 0.45], crop=28, jitter=[32, 40], clips=256)
OTHER_CONFIGS = [("rand-m9-n3-mstd0.5", 11, 6), ("rand-m7-w0", 12, 8), ("rand-m5-inc1", 13, 6)]
OTHER_HPARAMS = dict(img_mean=(124, 116, 104))
FILL = (114, 115, 116)
SIZES = [(40, 56), (37, 50)]
CONTENTS = ["noise", "ramp", "narrow", "constchan"]
GEOMETRIC = ["Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel"]
SIGNED = ["ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing"]
PLAIN = ["AutoContrast", "Equalize", "Invert", "PosterizeIncreasing", "SolarizeIncreasing", "SolarizeAdd"]
MID = ["AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast", "Brightness",
       "Sharpness", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel"]
BILINEAR, BICUBIC = int(Image.BILINEAR), int(Image.BICUBIC)


def _load(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Recorder:
    """wraps the loaded autoaugment module; `calls` collects one record per AugmentOp call"""

    def __init__(self, ref):
        self.ref, self.calls, self.cur = ref, [], None
        rec = self
        for name, fn in list(ref.NAME_TO_OP.items()):
            def op(img, *args, _fn=fn, **kwargs):
                rec.cur["applied"], rec.cur["args"] = True, tuple(args)
                return _fn(img, *args, **kwargs)
            op.ra_name = name
            ref.NAME_TO_OP[name] = op
        orig_interp, orig_call = ref._interpolation, ref.AugmentOp.__call__

        def interp(kwargs):
            out = orig_interp(kwargs)
            rec.cur["resample"] = int(out)
            return out

        def call(self, img):
            rec.cur = {"name": self.aug_fn.ra_name, "applied": False, "args": (), "resample": None}
            rec.calls.append(rec.cur)
            return orig_call(self, img)
        ref._interpolation, ref.AugmentOp.__call__ = interp, call

    def take(self):
        out, self.calls = self.calls, []
        return out


def record_np_draws(fn):
    """run fn() with np.random.uniform / randint recording what they return"""
    draws = []
    orig_u, orig_r = np.random.uniform, np.random.randint

    def uniform(*a, **k):
        v = orig_u(*a, **k)
        draws.append(("uniform", float(v)))
        return v

    def randint(*a, **k):
        v = orig_r(*a, **k)
        draws.append(("randint", int(v)))
        return v
    np.random.uniform, np.random.randint = uniform, randint
    try:
        out = fn()
    finally:
        np.random.uniform, np.random.randint = orig_u, orig_r
    return draws, out


def record_ek(ref, tfm, rec):
    random.seed(0)
    np.random.seed(0)
    T, H0, W0, crop = EK["T"], EK["H0"], EK["W0"], EK["crop"]
    pil = [Image.fromarray(np.zeros((H0, W0, 3), dtype=np.uint8)) for _ in range(T)]
    clips = []
    for _ in range(EK["clips"]):
        aa_params = dict(translate_const=int(crop * 0.45), img_mean=tuple([min(255, round(255 * x)) for x in EK["mean"]]))
        seed = random.randint(0, 100000000)
        frames = []
        for frame in pil:
            ref.rand_augment_transform(EK_CONFIG, aa_params, seed)(frame)
            frames.append(rec.take())

        def spatial():
            x = torch.zeros(3, T, H0, W0)
            x, _ = tfm.random_short_side_scale_jitter(images=x, min_size=EK["jitter"][0], max_size=EK["jitter"][1],
                                                      inverse_uniform_sampling=False)
            size = tuple(x.shape[-2:])
            x, _ = tfm.random_crop(x, crop)
            tfm.horizontal_flip(0.5, x)
            return size
        draws, size = record_np_draws(spatial)
        clips.append({"seed": seed, "frames": frames, "spatial_draws": draws, "scaled": size})
    return clips


def record_config(ref, rec, config, seed, n):
    random.seed(seed)
    np.random.seed(seed)
    pil = [Image.fromarray(np.zeros((24, 32, 3), dtype=np.uint8)) for _ in range(3)]
    clips = []
    for _ in range(n):
        hp = dict(OTHER_HPARAMS)
        s = random.randint(0, 100000000)
        frames = []
        for frame in pil:
            ref.rand_augment_transform(config, hp, s)(frame)
            frames.append(rec.take())
        clips.append({"seed": s, "frames": frames})
    return {"seed": seed, "width": 32, "height": 24, "hparams": dict(OTHER_HPARAMS), "clips": clips}


def run_ops(ref, rec, x, specs):
    """specs: [(name, magnitude, resample or None, wanted sign or None)] applied in a row to every frame of x.
    -> (records of the first frame's calls, output uint8 [T, H, W, 3])"""
    ops = []
    for name, mag, resample, sign in specs:
        hp = dict(img_mean=FILL)
        if resample is not None:
            hp["interpolation"] = resample
        for seed in range(64):                                   # the sign is the op's first draw after its re-seed
            op = ref.AugmentOp(name, prob=1.0, magnitude=mag, hparams=hp, seed=seed)
            op(Image.fromarray(x[0]))
            r = rec.take()[0]
            if sign is None or name not in GEOMETRIC + SIGNED or (r["args"][0] - (1.0 if name in SIGNED else 0.0)) * sign > 0:
                break
        else:
            raise AssertionError((name, sign))
        ops.append(op)
    out, first = [], None
    for t in range(x.shape[0]):
        img = Image.fromarray(x[t])
        for op in ops:
            img = op(img)
        calls = rec.take()
        first = first or calls
        assert [(c["name"], c["args"], c["resample"]) for c in calls] == [(c["name"], c["args"], c["resample"]) for c in first]
        out.append(np.array(img))
    return first, np.stack(out)


def main():
    ref = _load("ref_autoaugment", "lib", "datasets", "autoaugment.py")
    tfm = _load("ref_transform", "lib", "datasets", "transform.py")
    rec = Recorder(ref)
    fx = {"pillow": PIL.__version__, "fill": FILL, "ek_config": EK_CONFIG, "ek": dict(EK), "configs": {}, "pixels": [], "layers": []}
    fx["ek"]["clips"] = record_ek(ref, tfm, rec)

    # coverage of the recorded EPIC-Kitchens plans
    applied = [c for clip in fx["ek"]["clips"] for fr in clip["frames"] for c in fr if c["applied"]]
    names = {c["name"] for c in applied}
    assert names == set(ref._RAND_INCREASING_TRANSFORMS) and len(names) == 15, names
    signed = [c["args"][0] for c in applied if c["name"] in GEOMETRIC]
    assert min(signed) < 0 < max(signed)
    assert {c["resample"] for c in applied if c["name"] in GEOMETRIC} == {BILINEAR, BICUBIC}
    differs = sum([c["name"] for c in clip["frames"][0]] != [c["name"] for c in clip["frames"][1]] for clip in fx["ek"]["clips"])
    assert differs >= 1
    n_applied = sum(any(c["applied"] for c in clip["frames"][0]) for clip in fx["ek"]["clips"])
    for config, seed, n in OTHER_CONFIGS:
        fx["configs"][config] = record_config(ref, rec, config, seed, n)

    def pixel_case(content, size, in_seed, specs, where):
        x = make_input(content, size[0], size[1], in_seed, frames=1 if size == (8, 12) else 3)
        calls, out = run_ops(ref, rec, x, specs)
        fx[where].append({"content": content, "height": size[0], "width": size[1], "in_seed": in_seed, "in_sum": checksum(x),
                          "ops": [(c["name"], c["args"], c["resample"]) for c in calls], "out": torch.from_numpy(out)})

    k = 0

    def nxt():
        nonlocal k
        k += 1
        return CONTENTS[(k // 2) % 4], SIZES[k % 2], 100 + k      # every content at both sizes
    for name in GEOMETRIC:
        for sign in (1, -1):
            for res in (BILINEAR, BICUBIC):
                pixel_case(*nxt(), [(name, 10, res, sign)], "pixels")
    for name in SIGNED:
        for sign in (1, -1):
            pixel_case(*nxt(), [(name, 10, None, sign)], "pixels")
    for name in PLAIN:
        pixel_case(*nxt(), [(name, 10, None, None)], "pixels")
    for i, name in enumerate(MID):                                # magnitude 5, mstd 0: the non-increasing level functions
        pixel_case(*nxt(), [(name, 5, (BILINEAR, BICUBIC)[i % 2], (1, -1)[(i // 2) % 2])], "pixels")
    for name, content, size in [("AutoContrast", "narrow", SIZES[0]), ("AutoContrast", "narrow", SIZES[1]),
                                ("AutoContrast", "constchan", SIZES[1]), ("Equalize", "constchan", SIZES[0]),
                                ("Equalize", "narrow", SIZES[1]), ("Equalize", "noise", (8, 12)), ("Equalize", "ramp", SIZES[0])]:
        pixel_case(content, size, 300 + len(fx["pixels"]), [(name, 10, None, None)], "pixels")
    pixel_case("ramp", SIZES[1], 401, [("SolarizeAdd", 10, None, None), ("Rotate", 10, BICUBIC, -1)], "layers")
    pixel_case("noise", SIZES[0], 402, [("ShearX", 10, BILINEAR, 1), ("Equalize", 10, None, None)], "layers")
    pixel_case("narrow", SIZES[1], 403, [("AutoContrast", 10, None, None), ("TranslateYRel", 10, BILINEAR, 1)], "layers")

    # two files, each under the 1 MiB a committed file may have: the mid-magnitude and histogram cases go to the second
    n10 = len(GEOMETRIC) * 4 + len(SIGNED) * 2 + len(PLAIN)
    more = {"pillow": PIL.__version__, "pixels": fx["pixels"][n10:]}
    fx["pixels"] = fx["pixels"][:n10]
    size = 0
    for name, obj in (("randaug.pt", fx), ("randaug_more.pt", more)):
        path = os.path.join(HERE, name)
        torch.save(obj, path)
        size = max(size, os.path.getsize(path))
        print(f"wrote {path} ({os.path.getsize(path)} bytes), Pillow {PIL.__version__}")
    print(f"  ek: {len(fx['ek']['clips'])} clips, {n_applied} applied, frame 0 differs from frame 1 in {differs}")
    print("  applied ops:", {n: sum(c["name"] == n for c in applied) for n in sorted(names)})
    print(f"  pixels: {len(fx['pixels'])} + {len(more['pixels'])} cases, layers: {len(fx['layers'])}")
    assert size < (1 << 20), "a committed file stays under 1 MiB"


if __name__ == "__main__":
    main()
