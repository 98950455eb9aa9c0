"""TIMESFORMER.ATTENTION_TYPE 'space_only' / 'joint_space_time' at the model level, without a GPU: the module tree the reference builds
(lib/models/vit.py:100-111,215-217,273-281; key lists recorded from the reference in tests/golden/attn_types.pt), what load_pretrained
does to it (lib/models/helpers.py:216-238), and the DropPath granularity of the undivided block."""
import os

import pytest
import torch

from procedurevrl_amd.config import get_cfg

GOLD = os.path.join(os.path.dirname(__file__), "golden")
UNDIVIDED = {"joint_space_time": "joint_s33", "space_only": "space_only"}


def _model(attention_type, depth=2, crop=32, frames=8):
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
    return cfg, MODEL_REGISTRY.get(cfg.MODEL.MODEL_NAME)(cfg)


@pytest.fixture(scope="module")
def gold():
    return torch.load(os.path.join(GOLD, "attn_types.pt"), weights_only=False)


@pytest.mark.parametrize("attention_type", sorted(UNDIVIDED))
def test_state_dict_keys_equal_the_reference_model(gold, attention_type):
    _, model = _model(attention_type)           # construction from cfg does not raise
    keys = sorted(model.state_dict().keys())
    assert keys == gold[UNDIVIDED[attention_type]]["state_keys"]
    assert not any("temporal" in k for k in keys)
    assert ("model.time_embed" in keys) == (attention_type != "space_only")
    vt = model.model
    assert hasattr(vt, "time_drop") == (attention_type != "space_only") and hasattr(vt, "pos_drop")
    assert vt.no_weight_decay() == {"pos_embed", "cls_token", "time_embed"}           # vit.py:452-453, whatever the scheme
    assert vt.engine.undivided and vt.engine.space_only == (attention_type == "space_only")
    assert {n for n, _ in vt.named_parameters()} == set(vt.grad_store().names) | {"head.weight", "head.bias"}


def test_an_unknown_scheme_is_refused():
    with pytest.raises(AssertionError):
        _model("divided")


def test_divided_space_time_still_builds_what_it_built(gold):
    _, model = _model("divided_space_time")
    keys = sorted(model.state_dict().keys())
    joint = gold["joint_s33"]["state_keys"]
    temporal = [f"model.blocks.{i}.{m}.{p}" for i in range(2) for m, ps in (("temporal_norm1", ("weight", "bias")), ("temporal_fc", ("weight", "bias")),
                ("temporal_attn.qkv", ("weight", "bias")), ("temporal_attn.proj", ("weight", "bias"))) for p in ps]
    assert keys == sorted(joint + temporal)
    e2e = torch.load(os.path.join(GOLD, "e2e.pt"), weights_only=False)["state_keys"]
    assert set(keys) <= set(e2e)                 # (the pre-training fixture adds the order transformer and the text tower)
    for blk in model.model.blocks:
        assert float(blk.temporal_fc.weight.abs().sum()) == 0.0 and float(blk.temporal_fc.bias.abs().sum()) == 0.0
    assert not model.model.engine.undivided


@pytest.mark.parametrize("attention_type", sorted(UNDIVIDED))
def test_load_pretrained_creates_no_temporal_keys(tmp_path, attention_type, capsys):
    import sys
    sys.path.insert(0, GOLD)
    from make_golden import imagenet_vit_shapes
    from oracle import timesformer_oracle as orc
    from procedurevrl_amd.checkpoint import load_pretrained
    cfg, model = _model(attention_type, frames=4)
    inner = model.model
    state = orc.seeded_state(imagenet_vit_shapes(2), 5)
    state["time_embed"] = torch.randn(1, 8, 768)          # a video checkpoint's: 8 frames against the model's 4
    ck = tmp_path / "vit.pth"
    torch.save(state, ck)
    cfg.TIMESFORMER.PRETRAINED_MODEL = str(ck)
    before = sorted(inner.state_dict().keys())
    load_pretrained(inner, cfg)
    said = capsys.readouterr().out
    assert sorted(inner.state_dict().keys()) == before
    assert "temporal" not in said                          # neither missing nor unexpected: the clone is the divided scheme's alone
    assert torch.equal(inner.blocks[1].attn.qkv.weight, state["blocks.1.attn.qkv.weight"])
    if attention_type == "space_only":                     # no time_embed to resize: the checkpoint's is an unexpected key
        assert "time_embed" in said.split("Unexpected_keys")[1]
    else:                                                  # nearest resize 8 -> 4 (helpers.py:216-220)
        assert torch.equal(inner.time_embed, state["time_embed"][:, ::2])


def test_divided_load_pretrained_still_clones_the_spatial_weights(tmp_path):
    import sys
    sys.path.insert(0, GOLD)
    from make_golden import imagenet_vit_shapes
    from oracle import timesformer_oracle as orc
    from procedurevrl_amd.checkpoint import load_pretrained
    cfg, model = _model("divided_space_time")
    state = orc.seeded_state(imagenet_vit_shapes(2), 5)
    ck = tmp_path / "vit.pth"
    torch.save(state, ck)
    cfg.TIMESFORMER.PRETRAINED_MODEL = str(ck)
    load_pretrained(model.model, cfg)
    blk = model.model.blocks[0]
    assert torch.equal(blk.temporal_attn.qkv.weight, blk.attn.qkv.weight) and torch.equal(blk.temporal_norm1.bias, blk.norm1.bias)


def test_undivided_droppath_is_one_draw_per_sample_and_branch():
    from procedurevrl_amd.engine import EncoderEngine
    B, N, T = 3, 4, 2
    sa = torch.arange(B, dtype=torch.float32) + 10
    sm = torch.arange(B, dtype=torch.float32) + 100
    d = EncoderEngine.expand_droppath_undivided(sa, sm, B, N, T)
    assert d["s2_all"].shape == d["s3_all"].shape == (B * N * T + B,)
    for b in range(B):
        rows = list(range(b * N * T, (b + 1) * N * T)) + [B * N * T + b]
        assert (d["s2_all"][rows] == sa[b]).all() and (d["s3_all"][rows] == sm[b]).all()
