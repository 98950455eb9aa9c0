"""RandAugment on the host: `randaugment.clip_plan` / `epic_train_clip_draws` make the reference's draws (every recorded
op call and spatial draw of tests/golden/randaug.pt, written by the reference's own lib/datasets/autoaugment.py), the numpy
model of tests/randaug_checks.py reproduces every recorded Pillow output with zero differing values, and
`transform.decoded_train_batch` without USE_RAND_AUGMENT draws what `spatial_sampling_params` draws."""
import random

import numpy as np
import pytest
import torch

from randaug_checks import apply_clip_plan, apply_op, checksum, load_fixture, make_input
from procedurevrl_amd import randaugment as ra
from procedurevrl_amd.config import get_cfg
from procedurevrl_amd.transform import decoded_train_batch, spatial_sampling_params

FX = load_fixture()


def _calls(plan):
    """the plan in the fixture's form: per frame [(name, applied, args, resample)]"""
    return [[(op.name, op.applied, tuple(op.level_args), op.resample) for op in frame] for frame in plan.ops]


def _recorded(frames):
    return [[(c["name"], c["applied"], tuple(c["args"]), c["resample"]) for c in frame] for frame in frames]


def _ek_cfg():
    ek = FX["ek"]
    cfg = get_cfg()
    cfg.DATA.USE_RAND_AUGMENT = True
    cfg.DATA.MEAN, cfg.DATA.TRAIN_CROP_SIZE, cfg.DATA.TRAIN_JITTER_SCALES = list(ek["mean"]), ek["crop"], list(ek["jitter"])
    cfg.DATA.RANDOM_FLIP, cfg.DATA.INV_UNIFORM_SAMPLE = True, False
    return cfg


def test_epic_train_clip_draws_reproduce_every_recorded_clip():
    ek, cfg = FX["ek"], _ek_cfg()
    assert FX["ek_config"] == ra.EK_CONFIG
    random.seed(0)
    np.random.seed(0)
    applied = differ = 0
    for i, clip in enumerate(ek["clips"]):
        plan, (new_h, new_w, y_off, x_off, flip) = ra.epic_train_clip_draws(cfg, ek["T"], ek["H0"], ek["W0"])
        assert plan.seed == clip["seed"], i
        assert _calls(plan) == _recorded(clip["frames"]), i
        assert plan.fill == (115, 115, 115)
        # the reference's spatial draws: the jittered size, then randint per axis that is larger than the crop, then the flip
        draws = list(clip["spatial_draws"])
        assert draws.pop(0)[0] == "uniform" and (new_h, new_w) == tuple(clip["scaled"]), i
        want_flip = int(draws.pop()[1] < 0.5)
        offs = [v for k, v in draws]
        assert all(k == "randint" for k, _ in draws)
        got = ([y_off] if new_h > ek["crop"] else []) + ([x_off] if new_w > ek["crop"] else [])
        assert got == offs and flip == want_flip, i
        applied += not plan.is_identity
        differ += [op.name for op in plan.ops[0]] != [op.name for op in plan.ops[1]]
        # every op of a clip shares one probability draw; frames 1.. share their ops
        assert len({op.applied for fr in plan.ops for op in fr}) == 1
        assert all(_calls(plan)[t] == _calls(plan)[1] for t in range(2, ek["T"]))
    assert 0 < applied < len(ek["clips"]) and differ > 0


@pytest.mark.parametrize("config", sorted(FX["configs"]))
def test_clip_plan_follows_the_config_grammar(config):
    rec = FX["configs"][config]
    random.seed(rec["seed"])
    np.random.seed(rec["seed"])
    for i, clip in enumerate(rec["clips"]):
        seed = random.randint(0, 100000000)
        assert seed == clip["seed"]
        plan = ra.clip_plan(seed, len(clip["frames"]), rec["width"], rec["height"], config, dict(rec["hparams"]))
        assert _calls(plan) == _recorded(clip["frames"]), (config, i)
        assert plan.fill == tuple(rec["hparams"]["img_mean"])


def test_config_grammar_values():
    c = ra.parse_config("rand-m9-n3-mstd0.5")
    assert (c.magnitude, c.num_layers, c.transforms, c.weights, c.magnitude_std) == (9, 3, ra.RAND_TRANSFORMS, None, 0.5)
    assert ra.parse_config("rand-m9-mstd0.5-mstd2", {"magnitude_std": 1.5}).magnitude_std == 1.5     # hparams go first
    assert ra.parse_config("rand-mstd0.5-mstd2-m3-m4-x")[::4] == (4, 0.5)          # first mstd, last m, "x" says nothing
    c = ra.parse_config("rand-m7-w0-inc0")
    assert (c.magnitude, c.num_layers, c.magnitude_std) == (7, 2, 0) and c.transforms is ra.RAND_INCREASING_TRANSFORMS
    assert abs(float(np.sum(c.weights)) - 1.0) < 1e-12 and len(c.weights) == 15
    assert c.weights[ra.RAND_TRANSFORMS.index("Rotate")] == 0.3 / 1.0 and c.weights[ra.RAND_TRANSFORMS.index("Invert")] == 0
    assert ra.parse_config("rand").magnitude == 10 and len(set(ra.RAND_TRANSFORMS) - set(ra.RAND_INCREASING_TRANSFORMS)) == 6
    for bad in ("rand-q3", "augmix-m3", "rand-w1", "rand-3m"):
        with pytest.raises(ValueError):
            ra.parse_config(bad)


def test_rotate_matrix_follows_pil():
    from PIL import Image
    assert ra.rotate_matrix(360.0, 50, 37) is None
    with pytest.raises(NotImplementedError):
        ra.rotate_matrix(180, 50, 37)
    with pytest.raises(NotImplementedError):
        ra.rotate_matrix(90, 40, 40)
    x = make_input("noise", 37, 50, 9, frames=1)[0]
    for deg, resample in ((90, ra.BILINEAR), (270, ra.BICUBIC), (-17.5, ra.BICUBIC)):      # 90 / 270 off a square: the general path
        op = ra.resolve_op("Rotate", (deg,), resample, 50, 37)
        want = np.array(Image.fromarray(x).rotate(deg, resample=resample, fillcolor=(1, 2, 3)))
        assert np.array_equal(apply_op(x, op, (1, 2, 3)), want), deg


def _case_plan(case):
    frames = case["out"].shape[0]
    ops = [ra.resolve_op(name, args, resample, case["width"], case["height"]) for name, args, resample in case["ops"]]
    return ra.ClipPlan(None, [list(ops) for _ in range(frames)], FX["fill"], case["width"], case["height"])


@pytest.mark.parametrize("where", ["pixels", "layers"])
def test_numpy_model_equals_pillow_on_every_recorded_output(where):
    assert len(FX[where]) >= (56 if where == "pixels" else 3)
    kinds = set()
    for i, case in enumerate(FX[where]):
        x = make_input(case["content"], case["height"], case["width"], case["in_seed"], frames=case["out"].shape[0])
        assert checksum(x) == case["in_sum"], "the seeded input is not the one the fixture was recorded on"
        plan = _case_plan(case)
        got = apply_clip_plan(x, plan)
        want = case["out"].numpy()
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert int((got != want).sum()) == 0, (where, i, case["ops"])
        kinds.update(op.kind for op in plan.ops[0])
    if where == "pixels":
        assert kinds == set(range(1, 12))          # every kernel kind has a Pillow output behind it


def test_descriptors_match_the_header_layout():
    assert ra.DESC_DTYPE.itemsize == 64
    np.random.seed(3)
    clips = [ra.clip_plan(7, 3, 50, 37), ra.clip_plan(3, 3, 50, 37)]
    plan = ra.RandAugPlan(clips)
    d = plan.descriptors()
    assert d.shape == (2, 6)
    for b, clip in enumerate(clips):
        for t, frame in enumerate(clip.ops):
            for l, op in enumerate(frame):
                e = d[l, b * 3 + t]
                assert e["kind"] == op.kind
                if op.kind == ra.AFFINE:
                    assert tuple(e["c"]) == tuple(float(v) for v in op.args) and e["resample"] == op.resample
    with pytest.raises(ValueError):
        ra.RandAugPlan([clips[0], ra.clip_plan(3, 2, 50, 37)])


def test_descriptor_bytes_are_the_header_layout():
    """the layout contract once more, outside the code under test: `pvrl_ra_desc` is {int32 kind, resample, iarg[2]; double c[6]} and
    the kinds are the PVRL_RA_* numbers of include/pvrl.h, written out here as literals.  [layers][frames], layer-major."""
    import struct
    op = lambda kind, args, resample=None: ra.RaOp("x", True, (), resample, kind, args)
    frames = [[op(ra.AFFINE, (1.0, 0.25, -3.5, 0.0, 1.0, 2.0), ra.BICUBIC), op(ra.POSTERIZE, (4,))],
              [op(ra.SOLARIZE_ADD, (110, 128)), op(ra.COLOR, (1.75,))]]
    d = ra.RandAugPlan([ra.ClipPlan(0, frames, (128, 128, 128), 50, 37)]).descriptors()
    assert d.shape == (2, 2) and d.dtype == ra.DESC_DTYPE
    want = (struct.pack("<ii2i6d", 1, 3, 0, 0, 1.0, 0.25, -3.5, 0.0, 1.0, 2.0)         # layer 0: frame 0 AFFINE / BICUBIC
            + struct.pack("<ii2i6d", 7, 0, 110, 128, 0, 0, 0, 0, 0, 0)                 #          frame 1 SOLARIZE_ADD
            + struct.pack("<ii2i6d", 5, 0, 4, 0, 0, 0, 0, 0, 0, 0)                     # layer 1: frame 0 POSTERIZE
            + struct.pack("<ii2i6d", 8, 0, 0, 0, 1.75, 0, 0, 0, 0, 0))                 #          frame 1 COLOR
    assert d.tobytes() == want and len(want) == 4 * 64


def test_decoded_train_batch_without_randaugment_draws_as_before():
    cfg = get_cfg()
    assert cfg.DATA.USE_RAND_AUGMENT is False
    cfg.DATA.TRAIN_JITTER_SCALES, cfg.DATA.TRAIN_CROP_SIZE = [40, 56], 32
    frames = torch.zeros((3, 2, 36, 48, 3), dtype=torch.uint8)
    random.seed(5)
    np.random.seed(5)
    py_state = random.getstate()
    clips = decoded_train_batch(cfg, frames)
    after = np.random.get_state()
    np.random.seed(5)
    want = [spatial_sampling_params(36, 48, -1, 40, 56, 32, cfg.DATA.RANDOM_FLIP, cfg.DATA.INV_UNIFORM_SAMPLE) for _ in range(3)]
    assert clips.params_host.tolist() == [list(w) for w in want]
    now = np.random.get_state()
    assert after[2] == now[2] and np.array_equal(after[1], now[1])              # and nothing more was drawn
    assert random.getstate() == py_state                                        # Python's generator is not touched
    assert clips.frames.data_ptr() == frames.data_ptr() and clips.crop == 32 and clips.shape == (3, 3, 2, 32, 32)
