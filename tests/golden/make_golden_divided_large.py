"""Generate tests/golden/divided_large.pt by running the UNMODIFIED reference encoder with TIMESFORMER.ATTENTION_TYPE
'divided_space_time' on crops above 320^2 (lib/models/vit.py:129-157,365-423), the recipe of make_golden_attn_types.py: make_golden's
`import_reference`, `load_seeded`, `CaptureRNG`.  No reference source text is copied; weights and inputs are regenerated from the stored
seeds on both sides (oracle.timesformer_oracle.seeded_state keyed by parameter name; torch.Generator streams), each case holds only the
features, selected parameter gradients, the sum |grad| of every parameter, the captured DropPath draws and the state_dict key list.

    python tests/golden/make_golden_divided_large.py

336^2 is the smallest crop whose frame has more than 416 tokens (21 x 21 patches + cls = 442): the spatial attention of these cases
cannot take the whole-sequence kernels.  Cases (width 768, depth 2: one unpruned and one pruned block; features = forward_features(x),
loss = sum(features * dfeat)):
    div_s442               eval mode, 2 clips of 2 x 336^2 (two sequences share a cls row)
    div_s442_t3_droppath   training mode, 2 clips of 3 x 336^2, MODEL.DROP_PATH 0.5, the reference's torch.rand draws captured (three
                           per block with a non-zero rate: temporal, spatial, mlp)
    div_eval_resized       eval mode, 2 clips of 2 x 336^2 through a model built for 224^2 (nearest-neighbour pos_embed resize,
                           vit.py:375-386); features only

The pos_embed gradient ([1, 442, 768] fp32, 1.36 MB) is kept element-wise in `div_s442` alone and there on every POS_ROW_STEP-th token
row, so that the fixture stays under 1 MiB; sum |grad| of the whole tensor is in `grad_sums` of both cases.
"""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import make_golden as mg  # noqa: E402

KEEP = ["model.cls_token", "model.time_embed", "model.patch_embed.proj.bias", "model.norm.weight", "model.norm.bias",
        "model.blocks.0.norm1.weight", "model.blocks.0.temporal_norm1.bias", "model.blocks.0.temporal_fc.bias",
        "model.blocks.0.temporal_attn.qkv.bias", "model.blocks.0.attn.qkv.bias", "model.blocks.0.attn.proj.bias",
        "model.blocks.0.mlp.fc1.bias", "model.blocks.1.temporal_attn.proj.bias", "model.blocks.1.norm2.bias",
        "model.blocks.1.attn.qkv.bias", "model.blocks.1.mlp.fc2.bias"]
POS_ROW_STEP = 2
CASES = [dict(name="div_s442", B=2, crop=336, model_crop=336, T=2, drop_path=0.0, train=False, seed=51, grads=True, pos_rows=True),
         dict(name="div_s442_t3_droppath", B=2, crop=336, model_crop=336, T=3, drop_path=0.5, train=True, seed=52, grads=True,
              pos_rows=False),
         dict(name="div_eval_resized", B=2, crop=336, model_crop=224, T=2, drop_path=0.0, train=False, seed=53, grads=False,
              pos_rows=False)]
DEPTH, K = 2, 16


def inputs_of(case):
    """the case's clip batch and feature gradient, from its seed (the test regenerates them with this function's twin)"""
    g = torch.Generator().manual_seed(1000 + case["seed"])
    x = torch.randn(case["B"], 3, case["T"], case["crop"], case["crop"], generator=g)
    dfeat = torch.randn(case["B"], 768, generator=g)
    return x, dfeat


def make_case(defaults, vit, case, tmpdir):
    cfg = defaults.get_cfg()
    cfg.MODEL.MODEL_NAME = "vit_base_patch16_224_develop"
    cfg.MODEL.PRETRAINED = False
    cfg.MODEL.NUM_CLASSES = K
    cfg.MODEL.DROP_PATH = case["drop_path"]
    cfg.TIMESFORMER.DEPTH = DEPTH
    cfg.TIMESFORMER.ATTENTION_TYPE = "divided_space_time"
    cfg.DATA.TRAIN_CROP_SIZE = case["model_crop"]
    cfg.DATA.NUM_FRAMES = case["T"]
    cfg.DEV.MATCH_LANG_EMB = True
    cfg.NUM_GPUS = 0
    g = torch.Generator().manual_seed(78)
    label = torch.randn(K, 512, generator=g) * 0.38
    path = os.path.join(tmpdir, "test_emb.pth")
    torch.save(label / label.norm(dim=1, keepdim=True), path)
    cfg.DEV.TEST_LANG_EMB = path
    model = vit.vit_base_patch16_224_develop(cfg)
    sd = mg.load_seeded(model, case["seed"])
    model.train(case["train"])
    x, dfeat = inputs_of(case)
    with mg.CaptureRNG() as cap:
        feat = model.model.forward_features(x)
    draws = [d[1].reshape(-1).clone() for d in cap.log if d[0] == "rand"]
    assert len(draws) == len(cap.log) == (3 if case["train"] else 0)        # block 1's three DropPath calls (block 0's rate is 0)
    out = dict(case, depth=DEPTH, K=K, wsum=mg.checksum(sd), feat=feat.detach().clone(), draws=draws,
               state_keys=sorted(model.state_dict().keys()),
               state_shapes={k: tuple(v.shape) for k, v in model.state_dict().items() if k in ("model.pos_embed", "model.time_embed")})
    if case["grads"]:
        (feat * dfeat).sum().backward()
        named = dict(model.named_parameters())
        out["grads"] = {k: named[k].grad.clone() for k in KEEP}
        if case["pos_rows"]:
            out["pos_row_step"] = POS_ROW_STEP
            out["pos_embed_grad_rows"] = named["model.pos_embed"].grad[:, ::POS_ROW_STEP].clone()
        out["grad_sums"] = {k: float(p.grad.double().abs().sum()) for k, p in named.items() if p.grad is not None}
        out["no_grad"] = sorted(k for k, p in named.items() if p.grad is None)
    return out


def main():
    defaults, vit, tfm, dist, losses = mg.import_reference()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for case in CASES:
            out[case["name"]] = make_case(defaults, vit, case, tmp)
            print(case["name"], "features", tuple(out[case["name"]]["feat"].shape), "keys", len(out[case["name"]]["state_keys"]))
    path = os.path.join(HERE, "divided_large.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
