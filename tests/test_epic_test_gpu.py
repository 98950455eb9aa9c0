"""The EPIC-Kitchens multi-view test leg on the GPU.

* `pvrl_frames_u8_patchify_views` / `pvrl_frames_u8_to_f32_views` (several output clips naming one source slab) are bit-equal
  to the plain kernels on physically replicated frames, and meet the reference's own crops (tests/golden/epic_test.pt) by the
  criteria of kernel_checks.check_input_pipeline.
* `pvrl_view_ensemble` is bit-equal to the accumulators the reference's `EPICTestMeter` loop recorded, at every class count;
  the max mode equals `TestMeter(ensemble_method="max")`; an empty batch and out-of-range clip ids write nothing.
* `EPICTestMeter.update_stats` does not synchronise; `test(cfg)` end to end and on two ranks (gloo, one GPU) equals the
  reference loop replayed on the CPU over the model's recorded outputs.
"""
import os
import pickle
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "epic_test.pt")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACCS = ("verb_video_preds", "noun_video_preds", "verb_video_labels", "noun_video_labels", "clip_count")


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLD, weights_only=False)


# ---------------------------------------------------------------------------------------------------------------- views kernels
@pytest.mark.parametrize("which", [0, 1])
def test_views_kernels_equal_replicated_frames_and_the_reference_crops(gold, which):
    from kernel_checks import BF, rel
    from oracle import timesformer_oracle as orc
    from procedurevrl_amd import ops
    from procedurevrl_amd.transform import DecodedClips, DecodedViews, spatial_sampling_params
    case = gold["crops"][which]
    fr = case["frames"]                                                     # landscape / portrait, T = 2
    T, H0, W0, _ = fr.shape
    other = torch.randint(0, 256, fr.shape, generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    frames = torch.stack([other, fr])                                       # S = 2: the fixture's source is slab 1
    src = [1, 0, 1, 1, 0, 0]                                                # not monotonic: output clip != slab
    crop_of = [0, 0, 1, 2, 1, 2]                                            # crops 0, 1, 2 of either slab, in order of appearance
    params = [spatial_sampling_params(H0, W0, k, 32, 32, 32) for k in crop_of]
    views = DecodedViews(frames.to(DEV), params, src, gold["mean"], gold["std"], 32)
    plain = DecodedClips(frames[src].to(DEV), params, gold["mean"], gold["std"], 32)
    assert tuple(views.shape) == tuple(plain.shape) == (6, 3, T, 32, 32)
    rows_v, rows_p = ops.frames_u8_patchify(views), ops.frames_u8_patchify(plain)
    f32_v, f32_p = ops.frames_u8_to_f32(views), ops.frames_u8_to_f32(plain)
    assert rows_v.shape == rows_p.shape == (6 * 4 * T, 768) and torch.equal(rows_v, rows_p)
    assert torch.equal(f32_v, f32_p)
    # against the reference's crops of slab 1 (clips 0, 2, 3): the criteria of kernel_checks.check_input_pipeline
    ref = case["crops"]                                                     # [3 crops, 3, T, 32, 32]
    err = rel(f32_v[[0, 2, 3]], ref)
    print(f"fp32 views vs reference crops ({case['name']}): rel {err:.3e}")
    got = rows_v.view(6, 4 * T, 768)[[0, 2, 3]].reshape(-1, 768).float().cpu()
    ref_b = orc.patch_rows(ref).to(BF).float()
    d = (got - ref_b).abs()
    ulps = float((d / (ref_b.abs().clamp_min(2.0 ** -10) * 2.0 ** -7)).max())
    frac = float((d > 0).float().mean())
    print(f"patch rows vs reference crops ({case['name']}): {ulps:.3f} bf16 ulp, {frac:.3e} not bit-equal")
    assert err <= 1e-6 and ulps <= 1.01 and frac <= 2e-2


# -------------------------------------------------------------------------------------------------------------- ensemble kernel
def _accumulators(V, C, fill=0.0):
    return (torch.full((V, C), fill, device=DEV), torch.zeros(V, dtype=torch.long, device=DEV),
            torch.zeros(V, dtype=torch.long, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV))


def _head(c, C):
    """per-clip predictions, labels and the recorded accumulators of fixture case `c` for a head of C classes (5: the first
    five verb columns -- sums are per element, so the recorded columns are the reference's result for them)"""
    name = "noun" if C == 300 else "verb"
    return c[name + "_preds"].to(DEV)[:, :C], c[name + "_labels"].to(DEV), c[name + "_video_preds"][:, :C], c[name + "_video_labels"]


@pytest.mark.parametrize("C", [97, 300, 5])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_view_ensemble_is_bit_equal_to_the_reference_loop(gold, which, C):
    from procedurevrl_amd import ops
    c = gold["meter"][which]
    preds, labels, want_preds, want_labels = _head(c, C)                    # (C = 5: rows stay 97 floats apart)
    assert preds.stride(0) == (300 if C == 300 else 97)
    vp, vl, cnt, bad = _accumulators(c["num_videos"], C)
    at = 0
    for b in c["batches"]:
        ids = torch.tensor(b, device=DEV)
        ops.view_ensemble(preds[at:at + len(b)], ids, labels[at:at + len(b)], c["num_clips"], vp, vl, cnt, bad)
        at += len(b)
    assert torch.equal(vp.cpu(), want_preds) and torch.equal(vl.cpu(), want_labels)
    assert torch.equal(cnt.cpu(), c["clip_count"]) and int(bad.item()) == 0


@pytest.mark.parametrize("which", [0, 2])
def test_view_ensemble_max_mode_equals_test_meter(gold, which):
    from procedurevrl_amd import ops
    from procedurevrl_amd.test_net import TestMeter
    c = gold["meter"][which]
    preds, labels = c["verb_preds"], c["verb_labels"]
    ref = TestMeter(c["num_videos"], c["num_clips"], 97, ensemble_method="max")
    vp, vl, cnt, bad = _accumulators(c["num_videos"], 97)
    at = 0
    for b in c["batches"]:
        sl = slice(at, at + len(b))
        ref.update_stats(preds[sl], labels[sl], torch.tensor(b))
        ops.view_ensemble(preds[sl].to(DEV), torch.tensor(b, device=DEV), labels[sl].to(DEV), c["num_clips"], vp, vl, cnt, bad,
                          mode="max")
        at += len(b)
    assert torch.equal(vp.cpu(), ref.video_preds) and torch.equal(vl.cpu(), ref.video_labels)
    assert torch.equal(cnt.cpu(), ref.clip_count) and int(bad.item()) == 0
    assert float(vp.min()) >= 0.0 and float(vp.max()) > 0.0                 # (the accumulator's own zeros take part in the max)


def test_view_ensemble_empty_batch_and_bad_ids_write_nothing(gold):
    from procedurevrl_amd import ops
    c = gold["meter"][0]                                                    # 4 videos x 3 clips: valid ids are 0..11
    V, nc = c["num_videos"], c["num_clips"]
    vp, vl, cnt, bad = _accumulators(V, 97, fill=0.25)
    vl.fill_(7)
    cnt.fill_(2)
    snap = (vp.clone(), vl.clone(), cnt.clone())
    same = lambda: all(torch.equal(a, b) for a, b in zip((vp, vl, cnt), snap))
    e = torch.zeros(0, dtype=torch.long, device=DEV)
    ops.view_ensemble(torch.zeros(0, 97, device=DEV), e, e, nc, vp, vl, cnt, bad)
    assert same() and int(bad.item()) == 0
    preds, labels = c["verb_preds"][:3].to(DEV), c["verb_labels"][:3].to(DEV)
    ops.view_ensemble(preds, torch.tensor([V * nc, -1, 2 ** 40], device=DEV), labels, nc, vp, vl, cnt, bad)
    assert same() and int(bad.item()) != 0
    # a bad row between good ones: the good ones are folded in as if it were not there
    ops.view_ensemble(preds, torch.tensor([0, V * nc, 1], device=DEV), labels, nc, vp, vl, cnt, bad)
    want = (snap[0][0].cpu() + c["verb_preds"][0]) + c["verb_preds"][2]
    assert torch.equal(vp[0].cpu(), want) and torch.equal(vp[1:], snap[0][1:])
    assert cnt.tolist() == [4, 2, 2, 2] and vl.tolist() == [int(c["verb_labels"][2]), 7, 7, 7]


# ------------------------------------------------------------------------------------------------------------------------ meter
def _feed(meter, c, upto=None):
    at = 0
    for b in c["batches"][:upto]:
        sl = slice(at, at + len(b))
        meter.update_stats((c["verb_preds"][sl].to(DEV), c["noun_preds"][sl].to(DEV)),
                           (c["verb_labels"][sl].to(DEV), c["noun_labels"][sl].to(DEV)),
                           {"narration_id": c["narration_id"][sl]}, torch.tensor(b, device=DEV), b)
        at += len(b)


def test_meter_matches_the_reference_meter_and_rejects_a_bad_clip_id(gold):
    from procedurevrl_amd.multiview import EPICTestMeter
    c = gold["meter"][0]
    m = EPICTestMeter(c["num_videos"], c["num_clips"], gold["num_cls"], len(c["batches"]), device=DEV)
    assert all(getattr(m, a).device == torch.device(DEV) for a in ACCS)
    _feed(m, c)
    for a in ACCS:
        assert torch.equal(getattr(m, a).cpu(), c[a]), a
    assert list(m.metadata) == c["metadata"]
    m.finalize_metrics()
    assert m.stats == c["stats"]
    # a clip id of exactly V * num_clips: every accumulator and the metadata stay as they are, and finalize_metrics raises
    snap = [getattr(m, a).clone() for a in ACCS]
    bad_id = c["num_videos"] * c["num_clips"]
    m.update_stats((c["verb_preds"][:1].to(DEV), c["noun_preds"][:1].to(DEV)), (c["verb_labels"][:1].to(DEV), c["noun_labels"][:1].to(DEV)),
                   {"narration_id": ["P09_9"]}, torch.tensor([bad_id], device=DEV), [bad_id])
    assert all(torch.equal(getattr(m, a), s) for a, s in zip(ACCS, snap)) and list(m.metadata) == c["metadata"]
    with pytest.raises(ValueError):
        m.finalize_metrics()
    m.reset()
    assert all(int(getattr(m, a).abs().sum()) == 0 for a in ACCS) and int(m.bad_clip_id.item()) == 0


def test_update_stats_does_not_synchronise(gold):
    from procedurevrl_amd.multiview import EPICTestMeter
    c = gold["meter"][1]
    m = EPICTestMeter(c["num_videos"], c["num_clips"], gold["num_cls"], len(c["batches"]), device=DEV)
    b = c["batches"][0]
    args = ((c["verb_preds"][:len(b)].to(DEV), c["noun_preds"][:len(b)].to(DEV)),
            (c["verb_labels"][:len(b)].to(DEV), c["noun_labels"][:len(b)].to(DEV)),
            {"narration_id": c["narration_id"][:len(b)]}, torch.tensor(b, device=DEV), b)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                                   # the mode has teeth here: a read-back raises
            args[3][0].item()
        m.update_stats(*args)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(m.clip_count.sum()) == len(b)


# ------------------------------------------------------------------------------------------------------------------ end to end
def _epic_cfg(tmp, extra=()):
    from procedurevrl_amd.config import get_cfg
    from procedurevrl_amd.datasets import synthetic_label_emb
    cfg = get_cfg()
    cfg.merge_from_list(["MODEL.MODEL_NAME", "vit_base_patch16_224_develop", "MODEL.PRETRAINED", "False", "MODEL.NUM_CLASSES", "10",
                         "MODEL.DROP_PATH", "0.0", "TIMESFORMER.DEPTH", "2", "DATA.TRAIN_CROP_SIZE", "32", "DATA.TEST_CROP_SIZE", "32",
                         "DEV.MATCH_LANG_EMB", "False", "DEV.ORDER_PRETRAIN_ENABLED", "False", "TRAIN.DATASET", "Epickitchens",
                         "TEST.DATASET", "Epickitchens", "TRAIN.ENABLE", "False", "TEST.ENABLE", "True", "TEST.NUM_ENSEMBLE_VIEWS", "2",
                         "TEST.NUM_SPATIAL_CROPS", "3", "SYNTHETIC.ENABLE", "True", "OUTPUT_DIR", str(tmp)] + list(extra))
    cfg.DEV.TEST_LANG_EMB = synthetic_label_emb(16, seed=3)
    return cfg


def _recording_build_model(monkeypatch, record):
    """test(cfg) builds its own model: have it record every eval forward's (verb, noun)"""
    from procedurevrl_amd import multiview
    orig = multiview.build_model

    def build(cfg):
        model = orig(cfg)
        model.register_forward_hook(lambda _m, _i, out: record.append((out[0].float().cpu().clone(), out[1].float().cpu().clone())))
        return model
    monkeypatch.setattr(multiview, "build_model", build)


def _replay(record, batches, V, num_clips, labels_of):
    """the reference loop (meters.py:1040-1047) on the CPU over recorded outputs; batches: the clip ids of every update"""
    vp, npd = torch.zeros(V, 97), torch.zeros(V, 300)
    vl, nl, cnt = torch.zeros(V).long(), torch.zeros(V).long(), torch.zeros(V).long()
    meta = [0] * V
    for (verb, noun), ids in zip(record, batches):
        for ind, cid in enumerate(ids):
            vid = int(cid) // num_clips
            vl[vid], nl[vid] = labels_of[cid]
            vp[vid] += verb[ind]
            npd[vid] += noun[ind]
            meta[vid] = "P01_{}".format(vid)
            cnt[vid] += 1
    return dict(zip(ACCS, (vp, npd, vl, nl, cnt))), meta


def _stats_of(acc):
    from procedurevrl_amd.train_net import multitask_topk_accuracies, topk_accuracies
    v = topk_accuracies(acc["verb_video_preds"], acc["verb_video_labels"], (1, 5))
    n = topk_accuracies(acc["noun_video_preds"], acc["noun_video_labels"], (1, 5))
    a = multitask_topk_accuracies((acc["verb_video_preds"], acc["noun_video_preds"]),
                                  (acc["verb_video_labels"], acc["noun_video_labels"]), (1, 5))
    out = {"split": "test_final"}
    for name, t in (("verb", v), ("noun", n), ("action", a)):
        for k, x in zip((1, 5), t):
            out["{}_top{}_acc".format(name, k)] = "{:.2f}".format(float(x))
    return out


def _labels_of(cfg, num_videos):
    from procedurevrl_amd.datasets import SyntheticTestClips
    ds = SyntheticTestClips(cfg, num_videos)
    return {i: (int(ds[i][1]["verb"]), int(ds[i][1]["noun"])) for i in range(len(ds))}


def test_epic_test_end_to_end_equals_the_replayed_reference_loop(tmp_path, monkeypatch):
    from procedurevrl_amd.multiview import EPICTestMeter, test
    cfg = _epic_cfg(tmp_path, ["NUM_GPUS", "1", "TEST.BATCH_SIZE", "4", "SYNTHETIC.NUM_VIDEOS", "5"])
    record = []
    _recording_build_model(monkeypatch, record)
    meter = test(cfg)
    assert isinstance(meter, EPICTestMeter) and len(record) == 8            # 30 clips in batches of 4: videos straddle batches
    batches = [list(range(s, min(s + 4, 30))) for s in range(0, 30, 4)]
    want, meta = _replay(record, batches, 5, 6, _labels_of(cfg, 5))
    for a in ACCS:
        assert torch.equal(getattr(meter, a).cpu(), want[a]), a
    assert list(meter.metadata) == meta and meter.stats == _stats_of(want)
    with open(tmp_path / "scores" / "validation.pkl", "rb") as f:
        rows = pickle.load(f)
    assert len(rows) == 8
    labels_of = _labels_of(cfg, 5)
    for r, (verb, noun), ids in zip(rows, record, batches):
        assert set(r) == {"verb_output", "noun_output", "verb_label", "noun_label", "narration_id"}
        assert not r["verb_output"].is_cuda and torch.equal(r["verb_output"], verb) and torch.equal(r["noun_output"], noun)
        assert r["verb_label"].tolist() == [labels_of[i][0] for i in ids] and r["noun_label"].tolist() == [labels_of[i][1] for i in ids]
        assert r["narration_id"] == ["P01_{}".format(i // 6) for i in ids]


def _two_rank_job(cfg):
    """what launch_job runs in every rank: the real test(cfg); rank 0 leaves its meter behind"""
    import torch.distributed as dist
    from procedurevrl_amd.multiview import test
    meter = test(cfg)
    if dist.get_rank() == 0:
        torch.save({"acc": {a: getattr(meter, a).cpu() for a in ACCS}, "metadata": list(meter.metadata), "stats": meter.stats},
                   os.path.join(cfg.OUTPUT_DIR, "rank0.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_equal_the_single_process_run(tmp_path, monkeypatch):
    """4 videos x 6 clips, 3 clips per rank and iteration (the sampler pads nothing): the gathered batch of iteration i is clips
    [6i, 6i+2, 6i+4, 6i+1, 6i+3, 6i+5].  The single-process run is fed the same clips in the same order and the same batches of
    three, so every addition happens in the same order on the same numbers: equal to the bit."""
    import socket
    from procedurevrl_amd.datasets import SyntheticTestClips
    from procedurevrl_amd.multiview import test
    monkeypatch.setenv("PVRL_SINGLE_DEVICE", "1")
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import run_net
    two = tmp_path / "two"
    two.mkdir()
    cfg2 = _epic_cfg(two, ["NUM_GPUS", "2", "DIST_BACKEND", "gloo", "TEST.BATCH_SIZE", "6", "SYNTHETIC.NUM_VIDEOS", "4"])
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    run_net.launch_job(cfg=cfg2, init_method=f"tcp://127.0.0.1:{port}", func=_two_rank_job)
    r0 = torch.load(two / "rank0.pt", weights_only=False)
    with open(two / "scores" / "validation.pkl", "rb") as f:
        rows = pickle.load(f)
    order = [6 * it + r + 2 * k for it in range(4) for r in range(2) for k in range(3)]
    assert [n for r in rows for n in r["narration_id"]] == ["P01_{}".format(i // 6) for i in order]
    assert all(r["verb_output"].shape == (6, 97) and r["noun_label"].shape == (6,) for r in rows)
    one = tmp_path / "one"
    one.mkdir()
    cfg1 = _epic_cfg(one, ["NUM_GPUS", "1", "TEST.BATCH_SIZE", "3", "SYNTHETIC.NUM_VIDEOS", "4"])
    loader = torch.utils.data.DataLoader(SyntheticTestClips(cfg1, 4), batch_size=3, sampler=order)
    meter = test(cfg1, test_loader=loader)
    assert torch.equal(meter.clip_count.cpu(), torch.full((4,), 6))
    for a in ACCS:
        assert torch.equal(getattr(meter, a).cpu(), r0["acc"][a]), a
    assert list(meter.metadata) == r0["metadata"] and meter.stats == r0["stats"]
