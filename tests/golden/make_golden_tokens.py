"""Generate tests/golden/tokens.pt (and its two siblings, see FILES) by running the UNMODIFIED reference's
VisionTransformer.forward_features(x, cls=False) (lib/models/vit.py:365-423): the encoder's normalised output of EVERY token, the recipe
of make_golden_attn_types.py / make_golden_vit_large.py: make_golden's `import_reference`, `load_seeded`, `CaptureRNG`.  No reference
source text is copied; weights, clips and the token gradient are regenerated from the stored seeds on both sides
(oracle.timesformer_oracle.seeded_state keyed by parameter name; torch.Generator streams).

    python tests/golden/make_golden_tokens.py

Per case: the tokens `tok` = forward_features(x, cls=False) [B, 1 + N*T, C] ([B, 1 + N, C] for space_only), `feat` = forward_features(x)
of the same model on the same draws (its row 0), and of the loss sum(tok * dtok): the KEEP gradients, the sum |grad| of every parameter,
the list of parameters without a gradient, the captured DropPath draws and the state_dict key list.

Cases (depth 2):
    tok_div         divided_space_time, eval, 2 clips of 8 x 32^2
    tok_div_train   divided_space_time, training, 4 clips of 8 x 32^2, MODEL.DROP_PATH 0.5, the reference's torch.rand draws captured
                    (three for block 1: temporal, spatial, mlp; block 0's rate is 0)
    tok_stream      divided_space_time, eval, 2 clips of 2 x 336^2 (S = 442: the streamed spatial kernels).  883 tokens per clip: only the
                    token rows STREAM_ROWS (0 and every 8th) are stored, and of pos_embed's gradient only the rows STREAM_POS_ROWS
    tok_joint       joint_space_time, eval, 2 clips of 8 x 32^2
    tok_space       space_only, eval, 2 clips of 8 x 32^2
    tok_large       divided_space_time, eval, 2 clips of 8 x 32^2 at width 1024 / 16 heads (make_golden_vit_large.build)
FILES: no committed file may exceed 1 MiB, so the cases are spread over three: tokens.pt, tokens_train.pt, tokens_stream.pt.
"""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import make_golden as mg  # noqa: E402
import make_golden_vit_large as mgl  # noqa: E402
from make_golden_attn_types import KEEP as KEEP_ATTN  # noqa: E402

# make_golden_attn_types.KEEP plus the divided scheme's temporal parameters
KEEP = KEEP_ATTN + ["model.blocks.0.temporal_norm1.bias", "model.blocks.0.temporal_fc.bias", "model.blocks.1.temporal_attn.proj.bias"]
CASES = [dict(name="tok_div", type="divided_space_time", B=2, crop=32, T=8, drop_path=0.0, train=False, seed=71, width=768, heads=12),
         dict(name="tok_div_train", type="divided_space_time", B=4, crop=32, T=8, drop_path=0.5, train=True, seed=72, width=768, heads=12),
         dict(name="tok_stream", type="divided_space_time", B=2, crop=336, T=2, drop_path=0.0, train=False, seed=73, width=768, heads=12),
         dict(name="tok_joint", type="joint_space_time", B=2, crop=32, T=8, drop_path=0.0, train=False, seed=74, width=768, heads=12),
         dict(name="tok_space", type="space_only", B=2, crop=32, T=8, drop_path=0.0, train=False, seed=75, width=768, heads=12),
         dict(name="tok_large", type="divided_space_time", B=2, crop=32, T=8, drop_path=0.0, train=False, seed=76, width=1024, heads=16)]
FILES = {"tokens": ["tok_div", "tok_joint", "tok_space"], "tokens_train": ["tok_div_train", "tok_large"], "tokens_stream": ["tok_stream"]}
DEPTH, K = 2, 16
STREAM_ROWS = list(range(0, 883, 8))            # of tok_stream's 883 tokens per clip
STREAM_POS_ROWS = list(range(0, 442, 8))        # of its pos_embed gradient's 442 rows


def n_tokens(case):
    N = (case["crop"] // 16) ** 2
    return 1 + (N if case["type"] == "space_only" else N * case["T"])


def inputs_of(case):
    """the case's clip batch and token gradient, from its seed (the tests regenerate them with this function's twin)"""
    g = torch.Generator().manual_seed(1000 + case["seed"])
    x = torch.randn(case["B"], 3, case["T"], case["crop"], case["crop"], generator=g)
    dtok = torch.randn(case["B"], n_tokens(case), case["width"], generator=g)
    return x, dtok


def make_case(defaults, vit, case, tmpdir):
    mgl.WIDTH, mgl.HEADS = case["width"], case["heads"]         # (build() reads them: the reference registers the base width only)
    model = mgl.build(defaults, vit, tmpdir, case["type"], case["crop"], case["T"], case["drop_path"], depth=DEPTH)
    sd = mg.load_seeded(model, case["seed"])
    model.train(case["train"])
    x, dtok = inputs_of(case)
    torch.manual_seed(case["seed"])
    with mg.CaptureRNG() as cap:
        tok = model.model.forward_features(x, cls=False)
    draws = [d[1].reshape(-1).clone() for d in cap.log if d[0] == "rand"]
    assert len(draws) == len(cap.log) == (3 if case["drop_path"] else 0)
    assert tuple(tok.shape) == (case["B"], n_tokens(case), case["width"])
    (tok * dtok).sum().backward()
    torch.manual_seed(case["seed"])                              # the same draws again
    with torch.no_grad():
        feat = model.model.forward_features(x)
    named = dict(model.named_parameters())
    grads = {k: named[k].grad.clone() for k in KEEP if k in named}
    tok = tok.detach().clone()
    rows = None
    if case["name"] == "tok_stream":
        rows = STREAM_ROWS
        tok = tok[:, rows].clone()
        grads["model.pos_embed"] = grads["model.pos_embed"][:, STREAM_POS_ROWS].clone()
    return dict(case, depth=DEPTH, K=K, wsum=mg.checksum(sd), tok=tok, rows=rows, feat=feat.clone(), draws=draws, grads=grads,
                grad_sums={k: float(p.grad.double().abs().sum()) for k, p in named.items() if p.grad is not None},
                no_grad=sorted(k for k, p in named.items() if p.grad is None),
                state_keys=sorted(model.state_dict().keys()))


def main():
    defaults, vit, tfm, dist, losses = mg.import_reference()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for case in CASES:
            out[case["name"]] = c = make_case(defaults, vit, case, tmp)
            print(case["name"], "tokens", tuple(c["tok"].shape), "row 0 == features", torch.equal(c["tok"][:, 0], c["feat"]),
                  "no_grad", c["no_grad"])
    for fname, names in FILES.items():
        path = os.path.join(HERE, fname + ".pt")
        torch.save({n: out[n] for n in names}, path)
        print("wrote", path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
