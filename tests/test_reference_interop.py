"""Checkpoint interop with the REFERENCE's own save / load code (lib/utils/checkpoint.py), pinned by tests/golden/checkpoint.pt: a `.pyth`
written by the reference's save_checkpoint loads into this implementation with identical tensors, and a `.pyth` written here has the
layout the reference's load_checkpoint reads (every model_state key of the reference model with its shape and dtype, so that nothing is
left "not loaded", and the epoch it returns).  The fixture stores the reference file without its tensor payloads: the weights are
seeded_state(seed) by name, as in every fixture here (tests/golden/make_golden.py).  No GPU needed: state_dict plumbing only."""
import os
from collections import OrderedDict

import torch

from oracle import timesformer_oracle as orc

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _ref_checkpoint():
    g = torch.load(os.path.join(GOLDEN, "checkpoint.pt"), weights_only=False)
    shapes = {k: shp for k, shp, _ in g["model_state"]}
    sd = orc.seeded_state(shapes, g["seed"])
    ms = OrderedDict((k, sd[k].to(getattr(torch, dt))) for k, _, dt in g["model_state"])
    assert abs(float(sum(v.double().abs().sum() for v in ms.values())) - g["checksum"]) <= 1e-9 * g["checksum"]
    body = {"epoch": g["epoch"], "model_state": ms, "optimizer_state": g["optimizer_state"], "cfg": g["cfg"]}
    return g, OrderedDict((k, body[k]) for k in g["keys"])


def _my_model(cfg_ref, label_path):
    from procedurevrl_amd.build import MODEL_REGISTRY
    from procedurevrl_amd import vit  # noqa: F401
    from procedurevrl_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_list(["MODEL.MODEL_NAME", "vit_base_patch16_224_develop", "MODEL.PRETRAINED", "False", "MODEL.NUM_CLASSES",
                         str(cfg_ref.MODEL.NUM_CLASSES), "MODEL.TEXT_MODEL", "clip_vit_b_16", "TIMESFORMER.DEPTH",
                         str(cfg_ref.TIMESFORMER.DEPTH), "DATA.TRAIN_CROP_SIZE", str(cfg_ref.DATA.TRAIN_CROP_SIZE),
                         "DEV.MATCH_LANG_EMB", "True", "DEV.ORDER_PRETRAIN_ENABLED", "True", "NUM_GPUS", "0",
                         "SYNTHETIC.TEXT_LAYERS", "1"])
    cfg.TRAIN.LABEL_EMB = label_path
    return cfg, MODEL_REGISTRY.get(cfg.MODEL.MODEL_NAME)(cfg)


def test_reference_checkpoint_loads_here_and_ours_loads_there(tmp_path):
    from procedurevrl_amd import checkpoint as cu
    from procedurevrl_amd.config import CfgNode
    g, ck_r = _ref_checkpoint()
    assert g["path"] == os.path.join("checkpoints", "checkpoint_epoch_00005.pyth")
    path = str(tmp_path / "job_ref" / g["path"])
    os.makedirs(os.path.dirname(path))
    torch.save(ck_r, path)
    cfg_r = CfgNode.load_cfg(g["cfg"])
    K = cfg_r.MODEL.NUM_CLASSES
    label_path = str(tmp_path / "label_emb.pth")
    torch.save(torch.nn.functional.normalize(torch.randn(K, 512), dim=1), label_path)
    cfg_m, model_m = _my_model(cfg_r, label_path)
    # same key set on both sides (the text tower is part of the reference's state_dict as well)
    assert set(model_m.state_dict().keys()) == set(ck_r["model_state"].keys())
    epoch = cu.load_checkpoint(path, model_m, data_parallel=False, optimizer=None)
    assert epoch == 4
    sr, sm = ck_r["model_state"], model_m.state_dict()
    for k in sr:
        assert torch.equal(sr[k], sm[k]), k
    # ... and back: a checkpoint written here, in the layout the reference's load_checkpoint reads -- it copies every model_state entry
    # whose key and shape match its model's, and returns `epoch`
    from procedurevrl_amd.optimizer import construct_optimizer
    with torch.no_grad():
        for p in model_m.parameters():
            p.add_(0.01)
    opt_m = construct_optimizer(model_m, cfg_m)
    path2 = cu.save_checkpoint(str(tmp_path / "job_mine"), model_m, opt_m, 7, cfg_m)
    assert os.path.basename(path2) == "checkpoint_epoch_00008.pyth"
    ck = torch.load(path2, map_location="cpu", weights_only=False)
    assert set(ck.keys()) == {"epoch", "model_state", "optimizer_state", "cfg"}
    assert ck["epoch"] == 7
    ref_layout = {k: (tuple(shp), dt) for k, shp, dt in g["model_state"]}
    mine = ck["model_state"]
    assert set(mine) == set(ref_layout)
    for k, v in mine.items():
        assert (tuple(v.shape), str(v.dtype).replace("torch.", "")) == ref_layout[k], k
    sm = model_m.state_dict()
    for k in sm:
        assert torch.equal(mine[k], sm[k]), k
