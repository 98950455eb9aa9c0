"""Shared by tests/test_tokens_host.py and tests/test_tokens_gpu.py: the all-token fixtures (tests/golden/tokens*.pt, written by
tests/golden/make_golden_tokens.py from the UNMODIFIED reference's forward_features(x, cls=False)), their regenerated inputs, and the
all-token forward COMPOSED from oracle/rounded_oracle.py's own pieces (`block`, the rounding points R / RW / RB / RX, `attention_core`,
`GeluStore`): that oracle's forward_features returns row 0 only and stays as it is.  TEST INFRASTRUCTURE, not product code."""
import torch
import torch.nn.functional as F
from einops import rearrange

import e2e_checks as ec
from oracle import rounded_oracle as rorc
from oracle import timesformer_oracle as orc

FILES = ("tokens", "tokens_train", "tokens_stream")         # (no committed file above 1 MiB: make_golden_tokens.FILES)
CASES = ("tok_div", "tok_div_train", "tok_stream", "tok_joint", "tok_space", "tok_large")


def load():
    out = {}
    for name in FILES:
        out.update(ec.load(name))
    return out


def n_tokens(f):
    N = (f["crop"] // 16) ** 2
    return 1 + (N if f["type"] == "space_only" else N * f["T"])


def inputs(f):
    """twin of make_golden_tokens.inputs_of"""
    g = torch.Generator().manual_seed(1000 + f["seed"])
    x = torch.randn(f["B"], 3, f["T"], f["crop"], f["crop"], generator=g)
    return x, torch.randn(f["B"], n_tokens(f), f["width"], generator=g)


def rows_of(f, tok):
    """the token rows of `tok` [B, S, C] the fixture stores (tok_stream: 0 and every 8th)"""
    return tok if f["rows"] is None else tok[:, f["rows"]]


def make_model(f, act_checkpoint=False, drop_path=None):
    """the case's model on the CPU with the fixture's seeded weights -> (model, the same weights under the oracle's keys)"""
    from procedurevrl_amd import vit  # noqa: F401  (registers the models)
    from procedurevrl_amd.build import MODEL_REGISTRY
    cfg = ec.make_cfg(f["depth"], f["crop"], f["K"], drop_path=f["drop_path"] if drop_path is None else drop_path, frames=f["T"])
    cfg.MODEL.MODEL_NAME = "vit_large_patch16_224_develop" if f["width"] == 1024 else "vit_base_patch16_224_develop"
    cfg.MODEL.ACT_CHECKPOINT = bool(act_checkpoint)
    cfg.TIMESFORMER.ATTENTION_TYPE = f["type"]
    cfg.DEV.TEST_LANG_EMB = torch.randn(f["K"], 512)
    cfg.TRAIN.LABEL_EMB = ""
    model = MODEL_REGISTRY.get(cfg.MODEL.MODEL_NAME)(cfg)
    assert sorted(model.state_dict().keys()) == f["state_keys"]
    sd = orc.seeded_state({k: tuple(v.shape) for k, v in model.state_dict().items()}, f["seed"])
    assert abs(float(sum(v.double().abs().sum() for v in sd.values())) - f["wsum"]) <= 1e-9 * f["wsum"]
    model.load_state_dict(sd, strict=True)
    return model, {k[len("model."):]: v for k, v in sd.items()}


def droppath_oracle(f):
    """the reference's captured draws of block 1's three DropPath calls (block 0's rate is 0) -> the oracle's per-block (s1, s2, s3)"""
    if not f["draws"]:
        return None
    keep = 1.0 - f["drop_path"]
    return [None, tuple(torch.floor(keep + u.float()) / keep for u in f["draws"])]


def undivided_block(sd, pre, x, num_heads):
    """engine._block_fwd_undivided (Block.forward of 'space_only' / 'joint_space_time', vit.py:124-127) on [samples, 1 + S, C], with the
    rounding points of that path, written with rounded_oracle's pieces the way its `block` states the divided one: 16-bit LayerNorm
    output, qkv and attention output, the MFMA attention, 16-bit weight copies; the cls rows' projection and MLP in fp32 on the master
    weights (csrc/cls_chain.hip); the patch rows of the stream stored 16-bit after both residual adds."""
    C = x.shape[-1]
    rounding = rorc.OPERAND is not None
    ln = lambda t, n: F.layer_norm(t, (C,), sd[pre + n + ".weight"], sd[pre + n + ".bias"], orc.LN_EPS_VIT)
    lin = lambda t, n: F.linear(t, rorc.RW(sd[pre + n + ".weight"]), sd[pre + n + ".bias"])
    linf = lambda t, n: F.linear(t, sd[pre + n + ".weight"], sd[pre + n + ".bias"])
    h = rorc.R(ln(x, "norm1"))
    o = rorc.R(rorc.attention_core(rorc.R(lin(h, "attn.qkv")), x.shape[0], x.shape[1], C, num_heads, mfma=True))
    res = rorc.RB(lin(o, "attn.proj"))
    if rounding:
        res = torch.cat((rorc._value_of(linf(o[:, :1], "attn.proj"), res[:, :1]), res[:, 1:]), 1)
    x = x + res
    x = torch.cat((x[:, :1], rorc.RX(x[:, 1:])), 1)
    hf = ln(x, "norm2")
    u = rorc.RB(lin(rorc.R(hf), "mlp.fc1"))
    g = rorc.RW(rorc.GeluStore.apply(u)) if rounding else F.gelu(u)
    y = rorc.RB(lin(g, "mlp.fc2"))
    if rounding:
        y = torch.cat((rorc._value_of(linf(F.gelu(linf(hf[:, :1], "mlp.fc1")), "mlp.fc2"), y[:, :1]), y[:, 1:]), 1)
    x = x + y
    return torch.cat((x[:, :1], rorc.RX(x[:, 1:])), 1)


def oracle_tokens(f, sd, x, rounded=None, grad=False):
    """norm(x) of every token [B, 1 + N*T, C] ([B, 1 + N, C] for space_only) on the CPU: rounded_oracle.forward_features' embedding prologue
    and blocks, then the final norm over ALL rows.  `rounded` None: plain fp32 (the reference's arithmetic); a 16-bit dtype: the HIP
    datapath's rounding points, the 16-bit patch rows of the split residual stream included.  `grad`: keep the autograd graph (sd holds
    leaves that require a gradient: tests/grad_scale_checks.py back-propagates a chosen dtok through it)."""
    scheme, heads, depth = f["type"], f["heads"], f["depth"]
    dp = droppath_oracle(f)
    prev_resid = rorc.RESID
    rorc.RESID = "both" if rounded is not None else None
    try:
        with rorc.operand(rounded), torch.set_grad_enabled(bool(grad)):
            B, _, T, _, _ = x.shape
            xx = rearrange(rorc.R(x), "b c t h w -> (b t) c h w")
            xx = rorc.RB(F.conv2d(xx, rorc.RW(sd["patch_embed.proj.weight"]), sd["patch_embed.proj.bias"], stride=16))
            Wp = xx.size(-1)
            xx = xx.flatten(2).transpose(1, 2)
            xx = torch.cat((sd["cls_token"].expand(xx.size(0), -1, -1), xx), dim=1) + sd["pos_embed"]
            if scheme == "space_only":          # every frame a sample of its own, no time embedding; the mean over the frames in front of the norm
                xx = torch.cat((xx[:, :1], rorc.RX(xx[:, 1:])), dim=1)
                for i in range(depth):
                    xx = undivided_block(sd, f"blocks.{i}.", xx, heads)
                xx = rearrange(xx, "(b t) n m -> b t n m", b=B, t=T).mean(1)
            else:
                cls_tokens = xx[:B, 0, :].unsqueeze(1)
                xx = rearrange(xx[:, 1:], "(b t) n m -> (b n) t m", b=B, t=T) + sd["time_embed"]
                xx = rearrange(xx, "(b n) t m -> b (n t) m", b=B, t=T)
                xx = torch.cat((cls_tokens, rorc.RX(xx)), dim=1)
                for i in range(depth):
                    if scheme == "divided_space_time":
                        xx = rorc.block(sd, f"blocks.{i}.", xx, B, T, Wp, heads, None if dp is None else dp[i])
                    else:
                        xx = undivided_block(sd, f"blocks.{i}.", xx, heads)
            return F.layer_norm(xx, (xx.shape[-1],), sd["norm.weight"], sd["norm.bias"], orc.LN_EPS_VIT)
    finally:
        rorc.RESID = prev_resid


def patch_err(f, tok):
    """relative L2 error of the PATCH rows (every stored token row but row 0) of `tok` [B, S, C] against the fixture"""
    return ec.rel(rows_of(f, tok)[:, 1:], f["tok"][:, 1:])


# The error of the composed rounded oracle's PATCH rows against the fixture, patch_err(f, oracle_tokens(f, sd, x, dtype)), computed on the
# CPU per case and operand flavour (tests/test_tokens_host.py derives them again and holds these constants to what it finds).  The
# patch rows come out of the 16-bit residual stream, so their error is not the cls rows' (row 0 of the same runs: 2.0e-4 .. 4.7e-4 fp16,
# 1.7e-3 .. 3.4e-3 bf16).  The HIP path's absolute bar is PATCH_MARGIN x these: 1.5 x, the margin the project's gradient bars carry
# over what was observed (e2e_checks: "~1.5x the largest value observed").
ORACLE_PATCH_ERR = {
    "f16": dict(tok_div=7.017e-4, tok_div_train=6.598e-4, tok_stream=7.061e-4, tok_joint=6.314e-4, tok_space=5.368e-4, tok_large=7.480e-4),
    "bf16": dict(tok_div=5.619e-3, tok_div_train=5.285e-3, tok_stream=5.635e-3, tok_joint=5.013e-3, tok_space=4.269e-3, tok_large=5.987e-3),
}
PATCH_MARGIN = 1.5


def patch_bar(name):
    return PATCH_MARGIN * ORACLE_PATCH_ERR[ec.OPERAND][name]
