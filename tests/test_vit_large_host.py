"""`vit_large_patch16_224_develop` (embed_dim 1024, 16 heads) at the model level, without a GPU: the registry, the module tree the
reference builds at that width (key list recorded from the reference's VisionTransformer in tests/golden/vit_large.pt), what
load_pretrained does to it from a timm-layout ViT-L state dict (against what the reference's lib/models/helpers.py:load_pretrained did,
recorded in the same fixture), the refusal of widths the kernels do not serve, and the optimiser's parameter groups."""
import os
import sys

import pytest
import torch

from procedurevrl_amd.config import get_cfg

GOLD = os.path.join(os.path.dirname(__file__), "golden")
NAME = "vit_large_patch16_224_develop"


def _model(attention_type="divided_space_time", depth=2, crop=32, frames=8, K=16):
    from procedurevrl_amd.build import MODEL_REGISTRY
    from procedurevrl_amd import vit  # noqa: F401
    cfg = get_cfg()
    cfg.MODEL.MODEL_NAME = NAME
    cfg.MODEL.PRETRAINED = False
    cfg.MODEL.NUM_CLASSES = K
    cfg.TIMESFORMER.DEPTH = depth
    cfg.TIMESFORMER.ATTENTION_TYPE = attention_type
    cfg.DATA.TRAIN_CROP_SIZE = crop
    cfg.DATA.NUM_FRAMES = frames
    cfg.DEV.MATCH_LANG_EMB = True
    cfg.DEV.TEST_LANG_EMB = torch.randn(K, 512)
    cfg.NUM_GPUS = 0
    return cfg, MODEL_REGISTRY.get(cfg.MODEL.MODEL_NAME)(cfg)


@pytest.fixture(scope="module")
def gold():
    return torch.load(os.path.join(GOLD, "vit_large.pt"), weights_only=False)


def test_the_registry_has_the_large_model_next_to_the_base_one():
    from procedurevrl_amd.build import MODEL_REGISTRY
    from procedurevrl_amd import vit
    assert MODEL_REGISTRY.get(NAME) is vit.vit_large_patch16_224_develop
    assert MODEL_REGISTRY.get("vit_base_patch16_224_develop") is vit.vit_base_patch16_224_develop


@pytest.mark.parametrize("case", ["l_small", "l_joint"])
def test_state_dict_keys_and_shapes_equal_the_reference_at_width_1024(gold, case):
    f = gold[case]
    _, model = _model(f["type"], depth=f["depth"], crop=f["crop"], frames=f["T"], K=f["K"])
    assert sorted(model.state_dict().keys()) == f["state_keys"]
    vt = model.model
    assert (vt.embed_dim, vt.num_heads, len(vt.blocks)) == (1024, 16, 2) == (f["width"], f["heads"], f["depth"])
    assert tuple(vt.blocks[0].attn.qkv.weight.shape) == (3072, 1024) and tuple(vt.blocks[1].mlp.fc1.weight.shape) == (4096, 1024)
    assert tuple(vt.patch_embed.proj.weight.shape) == (1024, 3, 16, 16)          # K of the patch-embed GEMM stays 3 * 16 * 16 pixels
    assert tuple(vt.head.weight.shape) == (512, 1024)                            # the head projects to the label embedding's 512
    assert vt.engine.C == 1024 and vt.engine.H == 16 and vt.engine.scale == 0.125
    assert vt.engine.undivided == (f["type"] != "divided_space_time")
    # the seeded state the GPU tests load is the one the fixture's features came from
    from oracle import timesformer_oracle as orc
    sd = orc.seeded_state({k: tuple(v.shape) for k, v in model.state_dict().items()}, f["seed"])
    assert abs(float(sum(v.double().abs().sum() for v in sd.values())) - f["wsum"]) <= 1e-9 * f["wsum"]


def test_per_block_parameter_count_at_width_1024_and_the_vit_l16_config_line():
    """a spatial block is timm's ViT-L block (12,596,224 parameters), the divided scheme adds the temporal branch; the documented config
    line `MODEL.MODEL_NAME vit_large_patch16_224_develop TIMESFORMER.DEPTH 24` merges into the cfg and sets the depth the model is built
    with (built at depth 3 here: 24 blocks are 1.7 GB of fp32 parameters and say no more)"""
    cfg = get_cfg()
    cfg.merge_from_list(["MODEL.MODEL_NAME", NAME, "TIMESFORMER.DEPTH", "24"])
    assert cfg.MODEL.MODEL_NAME == NAME and cfg.TIMESFORMER.DEPTH == 24
    _, model = _model(depth=3)
    per_block = sum(p.numel() for p in model.model.blocks[0].parameters())
    C = 1024
    spatial = 2 * C + (3 * C * C + 3 * C) + (C * C + C) + 2 * C + (8 * C * C + 5 * C)
    assert spatial == 12596224 and per_block == spatial + 2 * C + (4 * C * C + 4 * C) + (C * C + C)
    assert all(sum(p.numel() for p in b.parameters()) == per_block for b in model.model.blocks)
    assert len(model.model.blocks) == 3 and len(model.model.drop_path_rates) == 3
    assert 24 * spatial == 302309376                        # ViT-L/16's 24 spatial blocks, the 304 M model less embeddings and head


def test_load_pretrained_from_a_timm_layout_vit_l_dict_matches_the_reference_loader(gold, tmp_path):
    """the same tensors change and end up with the same contents: classifier dropped (1000 != 512 rows), pos_embed resized 196 -> 49
    patches and time_embed 8 -> 4 frames by nearest neighbour, attn / norm1 cloned into temporal_attn / temporal_norm1"""
    sys.path.insert(0, GOLD)
    from make_golden import imagenet_vit_shapes, tensor_stats
    from oracle import timesformer_oracle as orc
    from procedurevrl_amd.checkpoint import load_pretrained
    g = gold["pretrained"]
    state = orc.seeded_state(imagenet_vit_shapes(g["depth"], dim=g["width"]), g["seed"])
    state["time_embed"] = torch.randn(1, g["ckpt_frames"], g["width"], generator=torch.Generator().manual_seed(g["seed"]))
    cfg, model = _model(depth=g["depth"], crop=g["crop"], frames=g["frames"], K=g["K"])
    inner = model.model
    for layout in ("timm", "pyth"):
        ck = tmp_path / f"vit_large_{layout}.pth"
        # a `.pyth` of this project: {model_state: keys with the registered model's `model.` prefix} (checkpoint.save_checkpoint)
        torch.save(state if layout == "timm" else {"epoch": 0, "model_state": {"model." + k: v for k, v in state.items()}}, ck)
        _, fresh = _model(depth=g["depth"], crop=g["crop"], frames=g["frames"], K=g["K"])
        inner = fresh.model
        before = {k: v.clone() for k, v in inner.state_dict().items()}
        cfg.TIMESFORMER.PRETRAINED_MODEL = str(ck)
        load_pretrained(inner, cfg)
        after = inner.state_dict()
        changed = sorted(k for k in after if not torch.equal(after[k], before[k]))
        assert changed == g["changed"], layout
        for k in changed:
            got, ref = tensor_stats(after[k]), g["stats"][k]
            assert all(abs(a - b) <= 1e-9 * max(1.0, abs(b)) for a, b in zip(got, ref)), (layout, k, got, ref)
        blk = inner.blocks[1]
        assert torch.equal(blk.temporal_attn.qkv.weight, blk.attn.qkv.weight) and torch.equal(blk.temporal_norm1.bias, blk.norm1.bias)
        assert torch.equal(inner.time_embed, state["time_embed"][:, ::2])
        assert float(blk.temporal_fc.weight.detach().abs().sum()) == 0.0
    # the undivided scheme clones nothing
    cfg_j, joint = _model("joint_space_time", depth=g["depth"], crop=g["crop"], frames=g["frames"], K=g["K"])
    cfg_j.TIMESFORMER.PRETRAINED_MODEL = str(tmp_path / "vit_large_timm.pth")
    keys = sorted(joint.model.state_dict().keys())
    load_pretrained(joint.model, cfg_j)
    assert sorted(joint.model.state_dict().keys()) == keys and not any("temporal" in k for k in keys)


def test_a_width_the_kernels_do_not_serve_raises_not_implemented_naming_the_supported_pairs():
    from procedurevrl_amd import ops
    from procedurevrl_amd.vit import VisionTransformer
    cfg, _ = _model()
    with pytest.raises(NotImplementedError) as e:
        VisionTransformer(img_size=32, num_classes=16, embed_dim=384, depth=1, num_heads=6, mlp_ratio=4, qkv_bias=True, num_frames=8, cfg=cfg)
    msg = str(e.value)
    assert "(384, 6)" in msg and "(768, 12)" in msg and "(1024, 16)" in msg
    for pair in ((768, 16), (1024, 12), (1280, 20)):       # head_dim != 64, or a width without a LayerNorm instantiation
        with pytest.raises(NotImplementedError, match=r"\(768, 12\), \(1024, 16\)"):
            ops.check_encoder_width(*pair)
    for pair in ops.ENCODER_WIDTHS:
        ops.check_encoder_width(*pair)


def test_optimizer_groups_cover_every_parameter_once():
    from procedurevrl_amd.optimizer import construct_optimizer
    cfg, model = _model()
    cfg.SOLVER.OPTIMIZING_METHOD = "adamw"
    opt = construct_optimizer(model, cfg)
    seen = [id(p) for grp in opt.param_groups for p in grp["params"]]
    want = [id(p) for p in model.parameters()]           # lib/models/optimizer.py:18-91 groups every named parameter, the frozen head too
    assert len(seen) == len(set(seen)) and sorted(seen) == sorted(want)
    assert sum(p.numel() for grp in opt.param_groups for p in grp["params"]) == sum(p.numel() for p in model.parameters())
