"""MODEL.ACT_CHECKPOINT without a GPU: the key reaches the TimeSformer engine (`EncoderEngine.act_checkpoint`), every reference yaml
leaves it off, the MViT engine refuses it by name instead of ignoring it, and `EncoderEngine.saved_nbytes` counts a storage once.

On the commit before this one: no `act_checkpoint` attribute, no refusal, no `saved_nbytes`."""
import os

import pytest
import torch
import yaml

from procedurevrl_amd.config import get_cfg

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _vit(**model_keys):
    from procedurevrl_amd.build import build_model
    cfg = get_cfg()
    cfg.MODEL.MODEL_NAME = "vit_base_patch16_224_develop"
    cfg.MODEL.PRETRAINED = False
    cfg.MODEL.NUM_CLASSES = 16
    cfg.TIMESFORMER.DEPTH = 2
    cfg.DATA.TRAIN_CROP_SIZE = 32
    cfg.DATA.NUM_FRAMES = 2
    cfg.DEV.MATCH_LANG_EMB = True
    cfg.DEV.TEST_LANG_EMB = torch.randn(16, 512)
    cfg.NUM_GPUS = 0
    for k, v in model_keys.items():
        setattr(cfg.MODEL, k, v)
    return build_model(cfg)


def _reference_yaml(tmp_path):
    ref = torch.load(os.path.join(GOLD, "reference_configs.pt"), weights_only=False)
    files = []
    for rel, mapping in sorted(ref.items()):
        os.makedirs(tmp_path / os.path.dirname(rel), exist_ok=True)
        (tmp_path / rel).write_text(yaml.safe_dump(mapping))
        files.append(str(tmp_path / rel))
    return files


def test_the_key_reaches_the_engine_and_defaults_to_off():
    assert get_cfg().MODEL.ACT_CHECKPOINT is False
    assert _vit().model.engine.act_checkpoint is False
    assert _vit(ACT_CHECKPOINT=True).model.engine.act_checkpoint is True


def test_the_flag_is_part_of_the_graph_key():
    eng = _vit().model.engine
    x = torch.zeros(1, 3, 2, 32, 32)
    off = eng._graph_key(x, True, True)
    eng.act_checkpoint = True
    on = eng._graph_key(x, True, True)
    assert off != on
    eng.act_checkpoint = False
    assert eng._graph_key(x, True, True) == off


def test_the_eight_reference_yaml_files_leave_it_off(tmp_path):
    files = _reference_yaml(tmp_path)
    assert len(files) == 8
    for f in files:
        cfg = get_cfg()
        cfg.merge_from_file(f)
        assert cfg.MODEL.ACT_CHECKPOINT is False, f


def test_mvit_refuses_the_key_by_name(tmp_path):
    from procedurevrl_amd import mvit
    f = [p for p in _reference_yaml(tmp_path) if p.endswith(os.path.join("HowTo100M", "procedurevrl_mvitv2_adamw.yaml"))]
    assert len(f) == 1
    cfg = get_cfg()
    cfg.merge_from_file(f[0])
    mvit._check_cfg(cfg)                        # the shipped configuration passes
    cfg.MODEL.ACT_CHECKPOINT = True
    with pytest.raises(NotImplementedError, match="ACT_CHECKPOINT"):
        mvit._check_cfg(cfg)
    with pytest.raises(NotImplementedError, match="ACT_CHECKPOINT"):
        mvit.MViT_encoder(cfg)


def test_saved_nbytes_counts_a_shared_storage_once():
    from procedurevrl_amd.engine import _X, storage_nbytes
    eng = _vit().model.engine
    assert eng.saved_nbytes() == 0              # nothing saved
    p0, p1, c = torch.zeros(6, 8, dtype=torch.float16), torch.zeros(6, 8, dtype=torch.float16), torch.zeros(2, 8)
    full = torch.zeros(8, 8)
    stats = (torch.zeros(6), torch.zeros(6))
    dp = dict(s3_all=torch.zeros(8))
    eng.saved = dict(B=2, T=1, blocks=[dict(x0=_X(p0, c), x1=_X(p1, c), st_t=stats, dp=dp, lse_t=None, pruned=False),   # x1.c is x0.c
                                       dict(ckpt=True, x0=_X(full[:6], full[6:], full), dp=dp), None],
                     norm_stats=stats, a_pe=None)
    want = 2 * 6 * 8 * 2 + 2 * 8 * 4 + 8 * 8 * 4 + 2 * 6 * 4 + 8 * 4
    assert eng.saved_nbytes() == want
    assert storage_nbytes(eng.saved["blocks"][1]) == 8 * 8 * 4 + 8 * 4       # a stage's two views and the buffer itself: one storage
    seen = set()
    assert storage_nbytes(eng.saved["blocks"][0], seen) + storage_nbytes(eng.saved["blocks"][1], seen) + \
        storage_nbytes(eng.saved["norm_stats"], seen) == want                # `seen` carries over: dp and the statistics count once
    eng.saved = None
