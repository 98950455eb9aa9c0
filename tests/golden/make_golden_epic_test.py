"""Generate tests/golden/epic_test.pt by running the UNMODIFIED reference EPIC-Kitchens test meter and test-crop chain.

Run where a reference checkout is available (PVRL_REFERENCE_DIR, default ../reference next to this repository):
    python tests/golden/make_golden_epic_test.py
The reference modules (lib/utils/meters.py, lib/utils/metrics.py, lib/datasets/utils.py, lib/datasets/transform.py) are loaded
from their files as they are, behind empty `lib` packages and stubs for what is not installed or not needed (ipdb, fvcore, sklearn,
cv2, lib.utils.logging / misc); nothing of their source is copied, only inputs and recorded outputs are stored.

  meter   cases run through the reference `EPICTestMeter` (update_stats per batch, then finalize_metrics): the per-batch clip
          ids, the per-clip predictions / labels / narration ids, and every accumulator, the metadata and the logged stats
          strings afterwards.
            a  V = 4 videos x 3 clips, batches of 7 and 5, ids shuffled: the clips of a video are never adjacent within a batch
               and videos straddle the two batches
            b  V = 5 x 6 clips in loader order, batches of 4 (the shape of the end-to-end GPU test)
            c  V = 4 x 6 clips, two "rank" batches of 3 concatenated per iteration, as `du.all_gather` hands them over under a
               non-shuffling DistributedSampler (rank r sees indices r, r + 2, ...)
          Predictions are randn * 10^U(-2, 2) with |x| floored at 1e-3: the spread makes the order of the fp32 additions show in
          the last bits, the floor keeps every partial sum away from denormals (no flush-to-zero difference in a bit-equality
          test); no two of a video's top six scores tie, so top-k is unambiguous on any device.  A video's labels are the
          classes at chosen ranks of its summed scores, so that the accuracies are not all zero.
  crops   reference tensor_normalize -> spatial_sampling(spatial_idx = 0, 1, 2, min = max = crop = 32) of one landscape
          (T = 2, 40 x 56) and one portrait (T = 2, 56 x 40) uint8 source: the three fp32 [3, T, 32, 32] outputs each.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("PVRL_REFERENCE_DIR", os.path.join(ROOT, "..", "reference"))
sys.dont_write_bytecode = True

NUM_CLS = [97, 300]
MEAN, STD, CROP = [0.45, 0.45, 0.45], [0.225, 0.225, 0.225], 32
VERB_RANK, NOUN_RANK = [0, 3, 20, 0, 2], [0, 0, 1, 30, 4]      # rank of the true class in a video's summed scores, by video % 5
LOGGED = []


def _install_stubs():
    for name, sub in (("lib", ""), ("lib.utils", "utils"), ("lib.datasets", "datasets")):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, "lib", sub) if sub else os.path.join(REF, "lib")]
        sys.modules[name] = m
    sys.modules["ipdb"] = types.ModuleType("ipdb")
    sys.modules["cv2"] = types.ModuleType("cv2")
    fv, fvc = types.ModuleType("fvcore"), types.ModuleType("fvcore.common")
    timer, fio = types.ModuleType("fvcore.common.timer"), types.ModuleType("fvcore.common.file_io")

    class Timer:
        def reset(self):
            pass

        def pause(self):
            pass

        def seconds(self):
            return 0.0
    timer.Timer, fio.PathManager = Timer, None
    sys.modules.update({"fvcore": fv, "fvcore.common": fvc, "fvcore.common.timer": timer, "fvcore.common.file_io": fio})
    sk, skm = types.ModuleType("sklearn"), types.ModuleType("sklearn.metrics")
    skm.average_precision_score = None
    sys.modules.update({"sklearn": sk, "sklearn.metrics": skm})
    import logging as pylog
    log = types.ModuleType("lib.utils.logging")
    log.get_logger = pylog.getLogger
    log.log_json_stats = lambda stats: LOGGED.append(dict(stats))
    sys.modules["lib.utils.logging"] = log
    sys.modules["lib.utils.misc"] = types.ModuleType("lib.utils.misc")


def make_preds(g, n, c):
    x = torch.randn(n, c, generator=g) * 10.0 ** (torch.rand(n, c, generator=g) * 4.0 - 2.0)
    return torch.where(x.abs() < 1e-3, torch.where(x < 0, -1e-3, 1e-3).to(x.dtype), x)


def run_meter(meters, name, V, num_clips, batches, seed):
    g = torch.Generator().manual_seed(seed)
    ids = [i for b in batches for i in b]
    assert sorted(ids) == list(range(V * num_clips)), name
    vid = torch.tensor(ids) // num_clips
    verb, noun = make_preds(g, len(ids), NUM_CLS[0]), make_preds(g, len(ids), NUM_CLS[1])
    # a video's label is the class at a chosen rank of its summed scores: hits at top-1, hits only at top-5 and misses all occur
    order = [torch.zeros(V, p.shape[1], dtype=torch.float64).index_add_(0, vid, p.double()).argsort(1, descending=True)
             for p in (verb, noun)]
    video_verb = torch.stack([order[0][v, VERB_RANK[v % 5]] for v in range(V)])
    video_noun = torch.stack([order[1][v, NOUN_RANK[v % 5]] for v in range(V)])
    verb_label, noun_label = video_verb[vid], video_noun[vid]
    narration = ["P01_{}".format(int(v)) for v in vid]
    m = meters.EPICTestMeter(V, num_clips, NUM_CLS, len(batches))
    at = 0
    for b in batches:
        sl = slice(at, at + len(b))
        m.update_stats((verb[sl], noun[sl]), (verb_label[sl], noun_label[sl]), {"narration_id": narration[sl]}, torch.tensor(b))
        at += len(b)
    del LOGGED[:]
    preds, labels, metadata = m.finalize_metrics(ks=(1, 5))
    assert len(LOGGED) == 1
    for p in preds:                                         # no ties among a video's top six scores
        top = torch.from_numpy(p).topk(7, dim=1).values
        assert bool((top[:, :6] > top[:, 1:7]).all()), name
    assert bool((m.clip_count == num_clips).all())
    return {"name": name, "num_videos": V, "num_clips": num_clips, "batches": [list(b) for b in batches],
            "verb_preds": verb, "noun_preds": noun, "verb_labels": verb_label, "noun_labels": noun_label, "narration_id": narration,
            "verb_video_preds": torch.from_numpy(preds[0]), "noun_video_preds": torch.from_numpy(preds[1]),
            "verb_video_labels": torch.from_numpy(labels[0]), "noun_video_labels": torch.from_numpy(labels[1]),
            "clip_count": m.clip_count.clone(), "metadata": [str(x) for x in metadata], "stats": dict(LOGGED[0])}


def meter_cases(meters):
    a = [[0, 3, 1, 6, 4, 2, 7], [9, 5, 10, 8, 11]]
    for b in a:                                             # clips of one video never adjacent within a batch
        assert all(x // 3 != y // 3 for x, y in zip(b, b[1:]))
    assert {i // 3 for i in a[0]} & {i // 3 for i in a[1]}  # a video straddles both batches
    b = [list(range(s, min(s + 4, 30))) for s in range(0, 30, 4)]
    c = [[6 * it + r + 2 * k for r in range(2) for k in range(3)] for it in range(4)]
    return [run_meter(meters, "a", 4, 3, a, 1), run_meter(meters, "b", 5, 6, b, 2), run_meter(meters, "c", 4, 6, c, 3)]


def crop_cases(dsu):
    out = []
    for name, (h, w), seed in (("landscape", (40, 56), 11), ("portrait", (56, 40), 12)):
        g = torch.Generator().manual_seed(seed)
        frames = torch.randint(0, 256, (2, h, w, 3), generator=g, dtype=torch.uint8)
        np.random.seed(seed)
        crops = []
        for k in range(3):
            x = dsu.tensor_normalize(frames, MEAN, STD).permute(3, 0, 1, 2)       # epickitchens.py:166-169
            crops.append(dsu.spatial_sampling(x, spatial_idx=k, min_scale=CROP, max_scale=CROP, crop_size=CROP).contiguous())
        out.append({"name": name, "frames": frames, "crops": torch.stack(crops)})
    return out


def main():
    _install_stubs()
    meters = importlib.import_module("lib.utils.meters")
    dsu = importlib.import_module("lib.datasets.utils")
    fx = {"num_cls": NUM_CLS, "mean": MEAN, "std": STD, "crop": CROP, "meter": meter_cases(meters), "crops": crop_cases(dsu)}
    path = os.path.join(HERE, "epic_test.pt")
    torch.save(fx, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    for c in fx["meter"]:
        print(" ", c["name"], c["stats"])
    assert os.path.getsize(path) < (1 << 20), "a committed file stays under 1 MiB"


if __name__ == "__main__":
    main()
