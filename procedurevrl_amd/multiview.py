"""Multi-view evaluation entry point with the EPIC-Kitchens leg (reference: tools/test_net.py `perform_test` :32-158 with its
dict-label branch :83-106 and scores file :127-137, `test` :161-221 with the meter choice :193-200; lib/utils/meters.py
`EPICTestMeter` :980-1147).  `test(cfg)` is what `tools/run_net.py` runs: for TEST.DATASET "Epickitchens" (dict labels, the eval
forward returns (verb, noun)) it builds `EPICTestMeter` and runs the loop below; every other dataset goes to `test_net.test`, which
is unchanged.

`EPICTestMeter` keeps its accumulators on the device and folds each batch in with `pvrl_view_ensemble`, one launch per head, in the
order -- and therefore to the bits -- of the reference's per-clip loop; nothing is read back before `finalize_metrics`, so the eval
forwards are enqueued ahead."""
import os
import pickle

import numpy as np
import torch

from . import checkpoint as cu
from . import distributed as du
from . import test_net
from .build import build_model
from .train_net import log_json_stats, multitask_topk_accuracies, topk_accuracies


class EPICTestMeter:
    """lib/utils/meters.py:980-1147: the verb / noun multi-view ensemble.  The tensor attributes (the reference's names) live on
    `device`; `metadata` is the reference's numpy object array of narration ids, filed on the host."""

    def __init__(self, num_videos, num_clips, num_cls=(97, 300), overall_iters=0, device=None):
        self.num_clips = num_clips
        self.overall_iters = overall_iters
        self.verb_video_preds = torch.zeros((num_videos, num_cls[0]), device=device)
        self.noun_video_preds = torch.zeros((num_videos, num_cls[1]), device=device)
        self.verb_video_labels = torch.zeros((num_videos), device=device).long()
        self.noun_video_labels = torch.zeros((num_videos), device=device).long()
        self.metadata = np.zeros(num_videos, dtype=object)
        self.clip_count = torch.zeros((num_videos), device=device).long()
        self.bad_clip_id = torch.zeros(1, dtype=torch.int32, device=device)     # set by the kernel, read in finalize_metrics
        self.stats = {}

    def reset(self):
        for t in (self.clip_count, self.verb_video_preds, self.verb_video_labels, self.noun_video_preds, self.noun_video_labels,
                  self.bad_clip_id):
            t.zero_()
        self.metadata.fill(0)

    def update_stats(self, preds, labels, metadata, clip_ids, clip_ids_host):
        """preds (verb [N, 97], noun [N, 300]) fp32, labels (verb, noun) int64 [N] and clip_ids int64 [N] on the meter's device;
        metadata {"narration_id": N strings} and clip_ids_host (the same N ids as host ints) file the narration ids.  Enqueues two
        launches and returns: no read-back, no synchronisation."""
        from . import ops
        ops.view_ensemble(preds[0].detach(), clip_ids, labels[0], self.num_clips, self.verb_video_preds, self.verb_video_labels,
                          self.clip_count, self.bad_clip_id)
        ops.view_ensemble(preds[1].detach(), clip_ids, labels[1], self.num_clips, self.noun_video_preds, self.noun_video_labels,
                          None, self.bad_clip_id)
        limit = self.metadata.shape[0] * self.num_clips
        for ind, cid in enumerate(clip_ids_host):
            if 0 <= int(cid) < limit:                       # (a bad id files nothing, like the kernel; finalize_metrics raises)
                self.metadata[int(cid) // self.num_clips] = metadata["narration_id"][ind]

    def finalize_metrics(self, ks=(1, 5), compute_recall=False):
        if compute_recall:
            raise NotImplementedError("the mean-recall variant (meters.py:1096-1122) is not implemented")
        if int(self.bad_clip_id.item()) != 0:
            raise ValueError("a clip id outside [0, num_videos * num_clips) = [0, {}) reached the test meter".format(
                self.metadata.shape[0] * self.num_clips))
        vp, npd, vl, nl = self.verb_video_preds, self.noun_video_preds, self.verb_video_labels, self.noun_video_labels
        verb_topks = topk_accuracies(vp, vl, ks)
        noun_topks = topk_accuracies(npd, nl, ks)
        action_topks = multitask_topk_accuracies((vp, npd), (vl, nl), ks)
        self.stats = {"split": "test_final"}
        for name, topks in (("verb", verb_topks), ("noun", noun_topks), ("action", action_topks)):
            for k, topk in zip(ks, topks):
                self.stats["{}_top{}_acc".format(name, k)] = "{:.{prec}f}".format(float(topk), prec=2)
        log_json_stats(self.stats)
        return (vp.cpu().numpy().copy(), npd.cpu().numpy().copy()), (vl.cpu().numpy().copy(), nl.cpu().numpy().copy()), \
            self.metadata.copy()


@torch.no_grad()
def perform_test(test_loader, model, test_meter, cfg):
    """tools/test_net.py:32-158.  Other datasets: `test_net.perform_test`.  EPIC-Kitchens (dict labels, :83-106): world > 1 gathers
    the verb / noun outputs, labels and clip ids with `du.all_gather`, the narration ids and the host copy of the clip ids with one
    `du.all_gather_unaligned`; every batch's gathered outputs, labels and narration ids become one record of
    OUTPUT_DIR/scores/<EPICKITCHENS.TEST_SPLIT>.pkl (:127-137), kept on the device while the loop runs and moved to the host once
    after it.  Deliberate deviation: the reference appends a record only when NUM_GPUS > 1, so on one GPU it pickles an empty
    list; here the list is filled at every world size."""
    if cfg.TEST.DATASET not in ["Epickitchens"]:
        return test_net.perform_test(test_loader, model, test_meter, cfg)
    model.eval()
    dev = next(model.parameters()).device
    world = du.get_world_size()
    results_lst = []
    for inputs, labels, video_idx, meta in test_loader:
        inputs = inputs.to(dev, non_blocking=True)
        ids_host = video_idx.view(-1).tolist()              # (the loader's tensor is on the host: no read-back)
        video_idx = video_idx.to(dev).view(-1)
        verb_labels, noun_labels = labels["verb"].to(dev).view(-1), labels["noun"].to(dev).view(-1)
        preds = model(inputs)
        verb_preds, noun_preds = preds[0].float(), preds[1].float()
        narration = list(meta["narration_id"])
        if world > 1:
            verb_preds, noun_preds, verb_labels, noun_labels, video_idx = du.all_gather(
                [verb_preds, noun_preds, verb_labels, noun_labels, video_idx])
            gathered = du.all_gather_unaligned((narration, ids_host))
            narration = [n for part, _ in gathered for n in part]
            ids_host = [i for _, part in gathered for i in part]
        test_meter.update_stats((verb_preds, noun_preds), (verb_labels, noun_labels), {"narration_id": narration}, video_idx, ids_host)
        results_lst.append({"verb_output": verb_preds, "noun_output": noun_preds, "verb_label": verb_labels, "noun_label": noun_labels,
                            "narration_id": narration})
    if du.is_master_proc():
        results_lst = [{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in r.items()} for r in results_lst]
        scores_path = os.path.join(cfg.OUTPUT_DIR, "scores")
        os.makedirs(scores_path, exist_ok=True)
        with open(os.path.join(scores_path, cfg.EPICKITCHENS.TEST_SPLIT + ".pkl"), "wb") as f:
            pickle.dump(results_lst, f)
    test_meter.finalize_metrics(ks=(1, 5))
    return test_meter


def test(cfg, test_loader=None):
    """tools/test_net.py:161-221 with the meter choice of :193-200: `EPICTestMeter` for TEST.DATASET "Epickitchens", otherwise
    exactly `test_net.test`.  (`test_loader` may be injected by tests.)"""
    if cfg.TEST.DATASET not in ["Epickitchens"]:
        return test_net.test(cfg, test_loader)
    du.init_distributed_training(cfg)
    torch.manual_seed(cfg.RNG_SEED)
    model = build_model(cfg)
    cu.load_test_checkpoint(cfg, model)
    if test_loader is None:
        from .datasets import construct_loader
        test_loader = construct_loader(cfg, "test")
    num_clips = cfg.TEST.NUM_ENSEMBLE_VIEWS * cfg.TEST.NUM_SPATIAL_CROPS
    assert len(test_loader.dataset) % num_clips == 0
    meter = EPICTestMeter(len(test_loader.dataset) // num_clips, num_clips, [97, 300], len(test_loader),
                          next(model.parameters()).device)
    perform_test(test_loader, model, meter, cfg)
    return meter
