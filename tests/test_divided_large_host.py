"""Divided space-time attention for crops above 320^2, the parts that need no GPU: the one attention dispatch rule (ops.attn_family),
the limit errors the engine raises before anything is launched, and the module tree of a TimeSformer-HR model (16 x 448^2) against the
key list the reference recorded in tests/golden/divided_large.pt."""
import os

import pytest
import torch

from procedurevrl_amd import ops
from procedurevrl_amd.config import get_cfg

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _model(attention_type="divided_space_time", crop=336, frames=2, depth=2):
    from procedurevrl_amd.build import MODEL_REGISTRY
    from procedurevrl_amd import vit  # noqa: F401
    cfg = get_cfg()
    cfg.MODEL.MODEL_NAME = "vit_base_patch16_224_develop"
    cfg.MODEL.PRETRAINED = False
    cfg.MODEL.NUM_CLASSES = 16
    cfg.TIMESFORMER.DEPTH = depth
    cfg.TIMESFORMER.ATTENTION_TYPE = attention_type
    cfg.DATA.TRAIN_CROP_SIZE = crop
    cfg.DATA.NUM_FRAMES = frames
    cfg.DEV.MATCH_LANG_EMB = True
    cfg.DEV.TEST_LANG_EMB = torch.randn(16, 512)
    cfg.NUM_GPUS = 0
    return MODEL_REGISTRY.get(cfg.MODEL.MODEL_NAME)(cfg)


@pytest.fixture(scope="module")
def gold():
    return torch.load(os.path.join(GOLD, "divided_large.pt"), weights_only=False)


def test_one_dispatch_rule_416_whole_417_streamed():
    assert ops.ATTN_MAX_S == 416 and ops.ATTN_CLS_MAX_S == 4096
    assert ops.attn_family(1) == ops.attn_family(416) == "whole"
    assert ops.attn_family(417) == ops.attn_family(442) == ops.attn_family(785) == ops.attn_family(ops.ATTN_LONG_MAX_S) == "streamed"
    assert not ops.attn_uses_long(416) and ops.attn_uses_long(417)
    with pytest.raises(NotImplementedError, match="ATTN_LONG_MAX_S"):
        ops.attn_family(ops.ATTN_LONG_MAX_S + 1)


@pytest.mark.parametrize("S,long_name", [(416, "attn_fwd"), (417, "attn_long_fwd"), (442, "attn_long_fwd")])
@pytest.mark.parametrize("scheme", ["divided", "undivided"])
def test_every_scheme_launches_what_the_rule_says(monkeypatch, scheme, S, long_name):
    """the divided spatial branch (mode 1, T sequences per cls row) and the undivided path (T = 1) reach the kernels through
    ops.attn_seq_fwd / _bwd alone: recorded here with the four entry points replaced, no library and no GPU involved"""
    calls = []
    for name in ("attn_fwd", "attn_long_fwd", "attn_bwd", "attn_long_bwd"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append((_n, a, k)) or (None, None, None))
    T = 3 if scheme == "divided" else 1
    kw = dict(mode=1, T=T, cls_base=7)
    ops.attn_seq_fwd("qkv", 2 * T, S, 12, 0.125, **kw)
    ops.attn_seq_bwd("qkv", "o", "oc", "do", "doc", "lse", 2 * T, S, 12, 0.125, **kw)
    assert [c[0] for c in calls] == [long_name, long_name.replace("fwd", "bwd")]
    assert calls[0][1] == ("qkv", 2 * T, S, 12, 0.125) and calls[0][2] == kw
    assert calls[1][1] == ("qkv", "o", "oc", "do", "doc", "lse", 2 * T, S, 12, 0.125) and calls[1][2] == kw


def test_the_engine_has_no_second_copy_of_the_rule():
    import inspect
    from procedurevrl_amd import engine
    src = inspect.getsource(engine)
    assert "attn_uses_long" not in src and "> ops.ATTN_MAX_S" not in src
    assert "ops.attn_long_fwd" not in src and "ops.attn_long_bwd" not in src
    assert src.count("ops.attn_seq_fwd(") == 2 and src.count("ops.attn_seq_bwd(") == 2       # divided spatial + undivided, each way


# ---- limits: NotImplementedError at construction, naming the limit and the key
def test_divided_frame_beyond_the_streamed_limit_is_refused_at_construction():
    with pytest.raises(NotImplementedError, match=r"DATA\.TRAIN_CROP_SIZE.*8282 tokens.*ATTN_LONG_MAX_S = 8192"):
        _model(crop=1456, depth=1)                      # 91 x 91 patches + cls


def test_divided_frame_beyond_the_cls_query_limit_is_refused_with_prune_attn_on(monkeypatch):
    monkeypatch.delenv("PVRL_PRUNE_ATTN", raising=False)
    monkeypatch.delenv("PVRL_PRUNE_LAST", raising=False)
    with pytest.raises(NotImplementedError, match=r"DATA\.TRAIN_CROP_SIZE.*4097 tokens.*ATTN_CLS_MAX_S = 4096.*PVRL_PRUNE_ATTN"):
        _model(crop=1024, depth=1)                      # 64 x 64 patches + cls
    monkeypatch.setenv("PVRL_PRUNE_ATTN", "0")          # the last block on the streamed kernels: inside their limit
    m = _model(crop=1024, depth=1)
    assert m.model.pos_embed.shape == (1, 4097, 768) and not m.model.engine.prune_attn
    m.model.engine.prune_attn = True                    # ... and a forward checks again, with the flags the engine has then
    with pytest.raises(NotImplementedError, match="ATTN_CLS_MAX_S"):
        m.model.engine._check_geometry(4096, 2)


def test_divided_too_many_frames_are_refused_at_construction():
    with pytest.raises(NotImplementedError, match=r"DATA\.NUM_FRAMES: 417 frames.*ATTN_MAX_S = 416"):
        _model(crop=32, frames=417, depth=1)
    _model(crop=32, frames=416, depth=1)


@pytest.mark.parametrize("attention_type,crop,frames,S", [("joint_space_time", 224, 42, 8233), ("space_only", 1456, 2, 8282)])
def test_undivided_sequence_beyond_the_streamed_limit_is_refused_at_construction(attention_type, crop, frames, S):
    with pytest.raises(NotImplementedError, match=rf"DATA\.TRAIN_CROP_SIZE.*{S} tokens.*ATTN_LONG_MAX_S = 8192"):
        _model(attention_type, crop=crop, frames=frames, depth=1)


def test_a_forward_checks_its_own_input_before_the_first_launch(monkeypatch):
    """a test crop larger than the model's: the input's geometry is checked ahead of every launch (no library is loaded here: the
    first thing behind the check would be)"""
    from procedurevrl_amd import engine as eng_mod
    m = _model(crop=224, frames=2, depth=1)
    eng = m.model.engine
    monkeypatch.setattr(eng, "_refresh_weights", lambda: (_ for _ in ()).throw(AssertionError("a launch before the check")))
    x = torch.empty(1, 3, 2, 1456, 1456, device="meta")
    with pytest.raises(NotImplementedError, match=r"DATA\.TEST_CROP_SIZE.*ATTN_LONG_MAX_S"):
        eng._forward(x, False)
    assert eng_mod.EncoderEngine._check_geometry(eng, 441, 2) is None          # 336^2 through a 224^2 model: allowed


# ---- the HR model's module tree
def test_hr_model_has_the_reference_keys_and_embedding_shapes(gold):
    f = gold["div_s442"]
    model = _model(crop=448, frames=16)                  # TimeSformer-HR: 16 x 448^2; construction from cfg does not raise
    sd = model.state_dict()
    assert sorted(sd.keys()) == f["state_keys"] == gold["div_s442_t3_droppath"]["state_keys"]
    # the fixture's embeddings are [1, (crop / 16)^2 + 1, 768] and [1, frames, 768]: the same pattern at 448 / 16
    assert f["state_shapes"] == {"model.pos_embed": (1, (f["crop"] // 16) ** 2 + 1, 768), "model.time_embed": (1, f["T"], 768)}
    assert tuple(sd["model.pos_embed"].shape) == (1, (448 // 16) ** 2 + 1, 768) == (1, 785, 768)
    assert tuple(sd["model.time_embed"].shape) == (1, 16, 768)
    eng = model.model.engine
    assert not eng.undivided and ops.attn_family(model.model.patch_embed.num_patches + 1) == "streamed"
    assert gold["div_eval_resized"]["state_shapes"]["model.pos_embed"] == (1, 197, 768)       # the resized case: a 224^2 model
