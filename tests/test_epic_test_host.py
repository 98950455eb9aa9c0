"""Host side of the EPIC-Kitchens multi-view test leg (no GPU): the test-batch builders of transform.py against the crops the
reference's own chain produced (tests/golden/epic_test.pt, written by tests/golden/make_golden_epic_test.py), the meter's final
metrics against the reference meter's logged strings, `all_gather_unaligned` at world 1, the synthetic test dataset's batch
contract and the host-side validation of the shared-slab index."""
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "epic_test.pt")


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLD, weights_only=False)


def _cfg(extra=()):
    from procedurevrl_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_list(["DATA.TEST_CROP_SIZE", "32", "TEST.NUM_ENSEMBLE_VIEWS", "2", "TEST.NUM_SPATIAL_CROPS", "3",
                         "TEST.DATASET", "Epickitchens", "TRAIN.DATASET", "Epickitchens"] + list(extra))
    return cfg


# (new_h, new_w) of the short side rescaled to 32, and the left / centre / right (top / middle / bottom) offsets of
# transform.py:150-191 -- checked below against the reference's pixels, not only against these numbers
WANT = {"landscape": [(32, 44, 0, 0, 0), (32, 44, 0, 6, 0), (32, 44, 0, 12, 0)],
        "portrait": [(44, 32, 0, 0, 0), (44, 32, 6, 0, 0), (44, 32, 12, 0, 0)]}


@pytest.mark.parametrize("which", [0, 1])
def test_decoded_test_views_params_and_src(gold, which):
    from oracle import timesformer_oracle as orc
    from procedurevrl_amd.transform import DecodedViews, decoded_test_views
    case = gold["crops"][which]
    cfg = _cfg(["DATA.MEAN", str(gold["mean"]), "DATA.STD", str(gold["std"])])
    fr = case["frames"]
    frames = torch.stack([fr, fr.flip(0)])                                  # two temporal views of one size
    np.random.seed(3)
    views = decoded_test_views(cfg, frames)
    after = np.random.uniform()
    np.random.seed(3)
    np.random.uniform(size=6)                                               # one draw per clip, even at min == max
    assert after == np.random.uniform()
    assert isinstance(views, DecodedViews) and tuple(views.shape) == (6, 3, 2, 32, 32)
    assert views.src_host.tolist() == [0, 0, 0, 1, 1, 1] and views.src.dtype == torch.int32
    assert views.params_host.tolist() == [list(p) for p in WANT[case["name"]]] * 2
    # the offsets are the ones the reference's crops imply: the same chain on the CPU from these params gives its pixels
    for k in range(3):
        got = orc.input_pipeline(fr, tuple(views.params_host[k].tolist()), gold["mean"], gold["std"], 32)
        err = float((got - case["crops"][k]).norm() / case["crops"][k].norm())
        assert err <= 1e-6, (case["name"], k, err)


def test_one_crop_is_the_centre_crop_and_two_are_undefined(gold):
    from procedurevrl_amd.transform import decoded_test_batch, decoded_test_views
    fr = gold["crops"][0]["frames"]
    one = decoded_test_views(_cfg(["TEST.NUM_SPATIAL_CROPS", "1"]), torch.stack([fr, fr]))
    assert one.src_host.tolist() == [0, 1] and one.params_host.tolist() == [list(WANT["landscape"][1])] * 2
    with pytest.raises(NotImplementedError):
        decoded_test_views(_cfg(["TEST.NUM_SPATIAL_CROPS", "2"]), torch.stack([fr, fr]))
    with pytest.raises(NotImplementedError):
        decoded_test_batch(_cfg(["TEST.NUM_SPATIAL_CROPS", "2"]), torch.stack([fr, fr]), [0, 1])


def test_decoded_test_batch_takes_the_crop_from_the_clip_index(gold):
    from procedurevrl_amd.transform import DecodedClips, DecodedViews, decoded_test_batch
    fr = gold["crops"][1]["frames"]
    clips = decoded_test_batch(_cfg(), torch.stack([fr] * 4), torch.tensor([5, 3, 7, 10]))
    assert isinstance(clips, DecodedClips) and not isinstance(clips, DecodedViews) and tuple(clips.shape) == (4, 3, 2, 32, 32)
    assert clips.params_host.tolist() == [list(WANT["portrait"][k]) for k in (2, 0, 1, 1)]
    one = decoded_test_batch(_cfg(["TEST.NUM_SPATIAL_CROPS", "1"]), torch.stack([fr] * 2), [4, 5])
    assert one.params_host.tolist() == [list(WANT["portrait"][1])] * 2


def test_src_index_out_of_range_raises_before_any_launch(gold, monkeypatch):
    from procedurevrl_amd import ops
    from procedurevrl_amd.transform import DecodedViews

    class NoLaunch:
        def call(self, *a):
            raise AssertionError("launched")
    monkeypatch.setattr(ops, "lib", lambda: NoLaunch())
    fr = gold["crops"][0]["frames"]
    frames = torch.stack([fr, fr])                                          # S = 2
    for src in ([0, 2, 1], [0, -1, 1]):
        views = DecodedViews(frames, [WANT["landscape"][0]] * 3, src, gold["mean"], gold["std"], 32)
        with pytest.raises(ValueError):
            ops.frames_u8_patchify(views)
        with pytest.raises(ValueError):
            ops.frames_u8_to_f32(views)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_finalize_metrics_reproduces_the_reference_strings(gold, which, capsys):
    from procedurevrl_amd.multiview import EPICTestMeter
    c = gold["meter"][which]
    m = EPICTestMeter(c["num_videos"], c["num_clips"], gold["num_cls"], len(c["batches"]), device="cpu")
    for name in ("verb_video_preds", "noun_video_preds", "verb_video_labels", "noun_video_labels", "clip_count"):
        assert getattr(m, name).shape == c[name].shape and getattr(m, name).dtype == c[name].dtype
        getattr(m, name).copy_(c[name])
    m.metadata[:] = c["metadata"]
    preds, labels, metadata = m.finalize_metrics(ks=(1, 5))
    assert m.stats == c["stats"]
    assert "json_stats: " in capsys.readouterr().out
    assert np.array_equal(preds[0], c["verb_video_preds"].numpy()) and np.array_equal(preds[1], c["noun_video_preds"].numpy())
    assert np.array_equal(labels[0], c["verb_video_labels"].numpy()) and np.array_equal(labels[1], c["noun_video_labels"].numpy())
    assert metadata.dtype == object and list(metadata) == c["metadata"]
    with pytest.raises(NotImplementedError):
        m.finalize_metrics(compute_recall=True)
    m.bad_clip_id.fill_(1)
    with pytest.raises(ValueError):
        m.finalize_metrics()


def test_all_gather_unaligned_world_1():
    from procedurevrl_amd import distributed as du
    obj = (["P01_0", "P01_1"], [3, 4])
    out = du.all_gather_unaligned(obj)
    assert out == [obj] and out[0] is obj


def test_synthetic_epic_test_batch_contract():
    from procedurevrl_amd.datasets import SyntheticTestClips, construct_loader
    cfg = _cfg(["DATA.NUM_FRAMES", "2", "TEST.BATCH_SIZE", "4", "NUM_GPUS", "1"])
    loader = construct_loader(cfg, "test", num_videos=2)
    assert len(loader.dataset) == 12
    seen = {}
    for inputs, labels, video_idx, meta in loader:
        n = inputs.shape[0]
        assert tuple(inputs.shape) == (n, 3, 2, 32, 32) and video_idx.dtype == torch.int64
        assert isinstance(labels, dict) and set(labels) == {"verb", "noun"}
        assert labels["verb"].shape == (n,) and labels["verb"].dtype == torch.int64 and labels["noun"].dtype == torch.int64
        assert int(labels["verb"].max()) < 97 and int(labels["noun"].max()) < 300
        assert isinstance(meta["narration_id"], list) and all(isinstance(s, str) for s in meta["narration_id"])
        for i, v, nn, s in zip(video_idx.tolist(), labels["verb"].tolist(), labels["noun"].tolist(), meta["narration_id"]):
            assert s == "P01_{}".format(i // 6)
            assert seen.setdefault(i // 6, (v, nn)) == (v, nn)                 # fixed per video
    assert sorted(seen) == [0, 1]
    # every other test dataset is what it was
    plain = SyntheticTestClips(_cfg(["TEST.DATASET", "kinetics", "DATA.NUM_FRAMES", "2"]), 2)[7]
    assert torch.is_tensor(plain[1]) and plain[3] == {}
