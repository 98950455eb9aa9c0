"""Generate tests/golden/vit_large.pt by running the UNMODIFIED reference's lib.models.vit.VisionTransformer at ViT-L's width
(embed_dim 1024, 16 heads; lib/models/vit.py:186-189 takes both), the recipe of make_golden_attn_types.py: make_golden's
`import_reference`, `load_seeded`, `CaptureRNG`.  No reference source text is copied; weights and inputs are regenerated from the stored
seeds on both sides (oracle.timesformer_oracle.seeded_state keyed by parameter name; torch.Generator streams), each case holds only the
features, selected parameter gradients, the sum |grad| of every parameter, the captured DropPath draws and the state_dict key list.

    python tests/golden/make_golden_vit_large.py

The reference registers the base model only; its wrapper (vit.py:473-506) is a module with the encoder as `.model`, which `Wrapper` below
restates so that the state_dict keys carry the `model.` prefix of a registered model.

Cases (width 1024, depth 2: one unpruned and one pruned block; features = forward_features(x), loss = sum(features * dfeat), dfeat [B, 1024]):
    l_small    divided_space_time, eval, 2 clips of 8 x 32^2 (M = 66 rows)
    l_nt8      divided_space_time, training, 4 clips of 8 x 192^2 (M = 4,612 rows, S = 145), MODEL.DROP_PATH 0.5, the reference's torch.rand
               draws captured (three for block 1: temporal, spatial, mlp; block 0's rate is 0)
    l_nt8_nodrop   the same clips and weights at MODEL.DROP_PATH 0: the step a HIP graph can replay (a captured step draws its own DropPath,
               so the reference's draws cannot be pinned under it)
    l_stream   divided_space_time, training, 2 clips of 2 x 336^2 (S = 442: the streamed spatial kernels)
    l_joint    joint_space_time, eval, 2 clips of 8 x 32^2
`pretrained`: lib/models/helpers.py:load_pretrained on the width-1024 encoder with a seeded state dict in timm's vit_large_patch16_224 layout
plus a video checkpoint's time_embed (the URL download replaced by the synthetic dict): which tensors change, and their statistics.
"""
import importlib
import os
import sys
import tempfile
from functools import partial

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import make_golden as mg  # noqa: E402
from oracle import timesformer_oracle as orc  # noqa: E402

WIDTH, HEADS = 1024, 16
KEEP = ["model.cls_token", "model.time_embed", "model.patch_embed.proj.bias", "model.norm.weight", "model.norm.bias",
        "model.blocks.0.norm1.weight", "model.blocks.0.temporal_norm1.bias", "model.blocks.0.temporal_fc.bias",
        "model.blocks.0.temporal_attn.qkv.bias", "model.blocks.0.attn.qkv.bias", "model.blocks.0.attn.proj.bias",
        "model.blocks.0.mlp.fc1.bias", "model.blocks.1.temporal_attn.proj.bias", "model.blocks.1.norm2.bias",
        "model.blocks.1.attn.qkv.bias", "model.blocks.1.mlp.fc2.bias"]
CASES = [dict(name="l_small", type="divided_space_time", B=2, crop=32, T=8, drop_path=0.0, train=False, seed=61),
         dict(name="l_nt8", type="divided_space_time", B=4, crop=192, T=8, drop_path=0.5, train=True, seed=62),
         dict(name="l_nt8_nodrop", type="divided_space_time", B=4, crop=192, T=8, drop_path=0.0, train=True, seed=62),
         dict(name="l_stream", type="divided_space_time", B=2, crop=336, T=2, drop_path=0.0, train=True, seed=63),
         dict(name="l_joint", type="joint_space_time", B=2, crop=32, T=8, drop_path=0.0, train=False, seed=64)]
DEPTH, K = 2, 16
PRETRAINED = dict(seed=92, depth=2, crop=112, K=16, frames=4, ckpt_frames=8)


class Wrapper(torch.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.model = inner


def inputs_of(case):
    """the case's clip batch and feature gradient, from its seed (the test regenerates them with this function's twin)"""
    g = torch.Generator().manual_seed(1000 + case["seed"])
    x = torch.randn(case["B"], 3, case["T"], case["crop"], case["crop"], generator=g)
    dfeat = torch.randn(case["B"], WIDTH, generator=g)
    return x, dfeat


def build(defaults, vit, tmpdir, attention_type, crop, frames, drop_path, depth=DEPTH):
    cfg = defaults.get_cfg()
    cfg.MODEL.PRETRAINED = False
    cfg.MODEL.NUM_CLASSES = K
    cfg.MODEL.DROP_PATH = drop_path
    cfg.TIMESFORMER.DEPTH = depth
    cfg.TIMESFORMER.ATTENTION_TYPE = attention_type
    cfg.DATA.TRAIN_CROP_SIZE = crop
    cfg.DATA.NUM_FRAMES = frames
    cfg.DEV.MATCH_LANG_EMB = True
    cfg.NUM_GPUS = 0
    g = torch.Generator().manual_seed(78)
    label = torch.randn(K, 512, generator=g) * 0.38
    path = os.path.join(tmpdir, "test_emb.pth")
    torch.save(label / label.norm(dim=1, keepdim=True), path)
    cfg.DEV.TEST_LANG_EMB = path
    inner = vit.VisionTransformer(img_size=crop, num_classes=K, patch_size=16, embed_dim=WIDTH, depth=depth, num_heads=HEADS, mlp_ratio=4,
                                  qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), drop_rate=0.0, attn_drop_rate=0.0,
                                  drop_path_rate=drop_path, num_frames=frames, attention_type=attention_type, label_emb=cfg.TRAIN.LABEL_EMB,
                                  mlp=cfg.MODEL.MLP, text_model=cfg.MODEL.TEXT_MODEL, lp=cfg.MODEL.TEXT_LP, num_seg=cfg.MODEL.NUM_SEG,
                                  extra_tr=cfg.MODEL.EXTRA_TR, drope=cfg.MODEL.DROP_E, cfg=cfg)
    return Wrapper(inner)


def make_case(defaults, vit, case, tmpdir):
    model = build(defaults, vit, tmpdir, case["type"], case["crop"], case["T"], case["drop_path"])
    sd = mg.load_seeded(model, case["seed"])
    model.train(case["train"])
    x, dfeat = inputs_of(case)
    with mg.CaptureRNG() as cap:
        feat = model.model.forward_features(x)
    draws = [d[1].reshape(-1).clone() for d in cap.log if d[0] == "rand"]
    assert len(draws) == len(cap.log) == (3 if case["drop_path"] else 0)        # block 1's three DropPath calls (block 0's rate is 0)
    (feat * dfeat).sum().backward()
    named = dict(model.named_parameters())
    return dict(case, depth=DEPTH, K=K, width=WIDTH, heads=HEADS, wsum=mg.checksum(sd), feat=feat.detach().clone(), draws=draws,
                grads={k: named[k].grad.clone() for k in KEEP if k in named},
                grad_sums={k: float(p.grad.double().abs().sum()) for k, p in named.items() if p.grad is not None},
                no_grad=sorted(k for k, p in named.items() if p.grad is None),
                state_keys=sorted(model.state_dict().keys()))


def make_pretrained(defaults, vit, tmpdir):
    helpers = importlib.import_module("lib.models.helpers")
    P = PRETRAINED
    inner = build(defaults, vit, tmpdir, "divided_space_time", P["crop"], P["frames"], 0.0, depth=P["depth"]).model
    fake = orc.seeded_state(mg.imagenet_vit_shapes(P["depth"], dim=WIDTH), P["seed"])
    fake["time_embed"] = torch.randn(1, P["ckpt_frames"], WIDTH, generator=torch.Generator().manual_seed(P["seed"]))
    helpers.model_zoo.load_url = lambda *a, **k: {k2: v.clone() for k2, v in fake.items()}
    inner.default_cfg = dict(url="https://synthetic/jx_vit_large_p16_224.pth", num_classes=1000, first_conv="patch_embed.proj",
                             classifier="head")
    before = {k: v.clone() for k, v in inner.state_dict().items()}
    helpers.load_pretrained(inner, num_classes=inner.num_classes, in_chans=3, filter_fn=None, img_size=P["crop"],
                            num_patches=(P["crop"] // 16) ** 2, attention_type="divided_space_time", pretrained_model="",
                            num_frames=P["frames"], pre_num=0)
    after = inner.state_dict()
    changed = sorted(k for k in after if not torch.equal(after[k], before[k]))
    return dict(P, width=WIDTH, changed=changed, stats={k: mg.tensor_stats(after[k]) for k in changed})


def main():
    defaults, vit, tfm, dist, losses = mg.import_reference()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for case in CASES:
            out[case["name"]] = make_case(defaults, vit, case, tmp)
            print(case["name"], "features", tuple(out[case["name"]]["feat"].shape), "keys", len(out[case["name"]]["state_keys"]))
        out["pretrained"] = make_pretrained(defaults, vit, tmp)
        print("pretrained: changed", len(out["pretrained"]["changed"]))
    path = os.path.join(HERE, "vit_large.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
