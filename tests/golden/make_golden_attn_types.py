"""Generate tests/golden/attn_types.pt by running the UNMODIFIED reference encoder with TIMESFORMER.ATTENTION_TYPE 'joint_space_time' and
'space_only' (lib/models/vit.py:100,124-127,215-217,393-416), the recipe of make_golden.py: its `import_reference`, `load_seeded`,
`CaptureRNG`.  No reference source text is copied; weights and inputs are regenerated from the stored seeds on both sides
(oracle.timesformer_oracle.seeded_state keyed by parameter name; torch.Generator streams), each case holds only the features, selected
parameter gradients, the sum |grad| of every parameter, the captured DropPath draws and the state_dict key list.

    python tests/golden/make_golden_attn_types.py

Cases (width 768, depth 2; features = forward_features(x), loss = sum(features * dfeat)):
    joint_s33        joint_space_time, 2 clips of 8 x 32^2    (S = 33: the whole-sequence attention kernels)
    joint_s513       joint_space_time, 2 clips of 32 x 64^2   (S = 513: the streamed kernels)
    space_only       space_only, 2 clips of 8 x 32^2
    joint_droppath   joint_space_time in training mode, 4 clips of 8 x 32^2, MODEL.DROP_PATH 0.5, the reference's torch.rand draws captured
"""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import make_golden as mg  # noqa: E402

KEEP = ["model.cls_token", "model.pos_embed", "model.time_embed", "model.patch_embed.proj.bias", "model.norm.weight", "model.norm.bias",
        "model.blocks.0.norm1.weight", "model.blocks.0.attn.qkv.bias", "model.blocks.0.attn.proj.bias", "model.blocks.0.mlp.fc1.bias",
        "model.blocks.1.norm2.bias", "model.blocks.1.attn.qkv.bias", "model.blocks.1.mlp.fc2.bias"]
CASES = [dict(name="joint_s33", type="joint_space_time", B=2, crop=32, T=8, drop_path=0.0, train=False, seed=41),
         dict(name="joint_s513", type="joint_space_time", B=2, crop=64, T=32, drop_path=0.0, train=False, seed=42),
         dict(name="space_only", type="space_only", B=2, crop=32, T=8, drop_path=0.0, train=False, seed=43),
         dict(name="joint_droppath", type="joint_space_time", B=4, crop=32, T=8, drop_path=0.5, train=True, seed=44)]
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
    cfg.TIMESFORMER.ATTENTION_TYPE = case["type"]
    cfg.DATA.TRAIN_CROP_SIZE = case["crop"]
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
    (feat * dfeat).sum().backward()
    named = dict(model.named_parameters())
    draws = [d[1].reshape(-1).clone() for d in cap.log if d[0] == "rand"]
    assert len(draws) == len(cap.log) == (2 if case["train"] else 0)        # block 1's two DropPath calls (block 0's rate is 0)
    return dict(case, depth=DEPTH, K=K, wsum=mg.checksum(sd), feat=feat.detach().clone(), draws=draws,
                grads={k: named[k].grad.clone() for k in KEEP if k in named},
                grad_sums={k: float(p.grad.double().abs().sum()) for k, p in named.items() if p.grad is not None},
                no_grad=sorted(k for k, p in named.items() if p.grad is None),
                state_keys=sorted(model.state_dict().keys()))


def main():
    defaults, vit, tfm, dist, losses = mg.import_reference()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for case in CASES:
            out[case["name"]] = make_case(defaults, vit, case, tmp)
            print(case["name"], "features", tuple(out[case["name"]]["feat"].shape), "keys", len(out[case["name"]]["state_keys"]))
    path = os.path.join(HERE, "attn_types.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
