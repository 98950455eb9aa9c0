"""The MViTv2 encoder step against the fp32 oracle, PRICED BY THE ROUNDING MODEL oracle/mvit_rounded_oracle.py: features, every block's
output and every parameter gradient.  TEST INFRASTRUCTURE.

Used by tests/test_mvit_rounding_gpu.py (pytest -m gpu: MViTEngine on the device) and tests/test_mvit_rounding_host.py (no GPU: the model's
`VARIANT` and its planted `DEFECTS` stand in for the HIP path).  The flat bounds of tests/mvit_checks.py stay as they are; they detect
regressions.  This rule argues correctness: the kernels are held per row to their rounding models elsewhere (pool_attn_checks,
mvit_pool_checks), here the COMPOSITION MViTEngine makes of them is -- which tensor is 16-bit between kernels, which row scale goes in before a
cast, the S-scaled backward of the fp16 flavour.  The model is always the reference for the size of the error; the HIP path never sets its own
bound.

Cases (all on the reduced 4-block geometry of tests/golden/mvit_small.pt: 4 frames, crop 64, every block flavour):
  fixture    the fixture's own x and gout, 2 clips
  droppath   3 clips of seeded randn, per-clip DropPath draws pinned at rate 0.3 (`DROPPATH_SEED`: the last block's attention branch
             drops clips 0 and 2 and keeps clip 1, its MLP branch the other way round, so rs_a / rs_m sit on both sides of the pruned slice)
  unpruned   `fixture` with engine.prune_last = False (the model is the same: it computes exact zeros where the pruned engine skips)
  down / up  `fixture` with the incoming gradient times 2^-12 / 2^12 (moves S in the fp16 flavour).  The fp32 oracle and the model are exactly
             covariant under a power of two (the model's backward is fed S g with S from begin_scaled's formula, which moves the other way),
             so their gradients are `fixture`'s times 2^k; tests/test_mvit_rounding_host.py checks that bit for bit.
Rule.  e(t) = ||t - fp32 oracle's t||, rel = e / ||oracle's t||.
  features        rel(HIP) / rel(model) <= e2e_checks.TOL_RATIO, and HIP is closer to the model than to the oracle
  per block       the same ratio on each block's output (engine.saved["blocks"][i + 1]["x"], x_final), so that a failure names a block; the
                  pruned last block defines its cls rows only, and only those are compared
  worst gradient  max over parameters of rel(HIP) / max over parameters of rel(model) <= e2e_checks.TOL_RATIO_GRAD, over all parameters but
                  the eight of `NOT_LIVE`, which `live` asserts by name: the four norm_k.bias (true gradient 0: a common shift of all keys
                  is softmax-invariant) and the last block's pool_q.weight and rel_pos_h / w / t (exactly zero: only its cls query reaches
                  the features).  Their relative error has no meaning; the absolute rule below judges them like the rest.
  every parameter all `N_PARAMS` = 105 encoder parameters (the 73 of the fixture's `grads` among them), none skipped: the ABSOLUTE error
                  e(HIP) <= ROW_FACTOR max(e(model), e(variant)), ROW_FACTOR = 4 (attn_checks).  Absolute errors need no special case for
                  norm_k.bias.  Where e(model) = e(variant) = 0 exactly -- no rounded operand reaches the gradient: norm.bias, the column
                  sums of gout -- the bound is REL_Y_FACTOR Y instead, Y = e(fp32 oracle) against the fp64 oracle, the reference's own error
                  (REL_Y_FACTOR = 8 as in pool_attn_checks); everywhere else `judge` asserts 8 Y < 4 max(e(model), e(variant)), so that
                  floor is never what a rounded tensor is held to.  The last block's structural zeros: bound 0, the engine writes exact zeros.
  small tensors   a parameter of fewer than attn_checks.MIN_ROWS = 384 elements (LayerNorm vectors, rel_pos_t, narrow biases) is one or two
                  rows: its error on one input is one draw.  As attn_checks.n_draws has it, EVERY path -- the HIP engine, the model, the
                  variant, the fp32 oracle -- runs the case on `N_DRAWS` seeded inputs (`step_on_draws`), and such a parameter's e is taken
                  over all draws together (root of the summed squares): same inputs for all, same bounds.  ROW_FACTOR is justified the
                  project's way: the host test asserts spread = larger / smaller of e(model), e(variant) <= ROW_FACTOR / 2 for every
                  parameter on every case.
  per site        The rule above prices the TOTAL rounding error; ONE more rounding of a tensor that already carries some twenty-five per
                  block moves it by 0 to 20 % (tests/test_mvit_rounding_host.py has the figures), so the composition's single choices are
                  read off the path itself -- off engine.saved and, in the backward, through `BackwardProbe` (wrapped entry points, no
                  switch in product code); the model reports the same facts through mvit_rounded_oracle.TAPS:
                    block outputs are fp32, not 16-bit-valued: share of entries that survive a round trip through the operand type <= 1 %
                    (an fp32 value does with probability 2^-13 / 2^-16; a stream stored 16-bit reads 100 %);
                    rel is a hi + lo pair: share of entries with a zero lo half <= 50 % (a pair: ~0.1 %; a single value: 100 %);
                    dxn = dqkv W_qkv is fp32 where dim != dim_out: the 16-bit-valued share of the `aux` the skip projection's backward GEMM
                    adds dxs W_skip to <= 1 % (the model: of the attention branch's input gradient), and of the sum norm1's backward reads;
                    every DropPath factor goes in BEFORE the cast: each 16-bit gradient copy that carries one (ln_bwd's fused copy,
                    cast_scale; their number is asserted) equals R(factor x the fp32 gradient it was made from) on >= 99 % of its entries
                    (the other order, R(gradient) x factor, differs on 30 to 64 % of the live rows' entries);
                    the accumulated gradients (`ACCUMULATED`: the stem weight, the rel_pos_h / w / t tables of blocks 0-2) are fp32 sums: share
                    of entries whose low 8 mantissa bits vanish <= 5 % (2^-8 for a sum of many 22-bit products, ten times that allowed for
                    border entries that sum few terms; a 16-bit accumulator or a sum of two 16-bit partials reads 98 to 100 %).
Measured spreads (host, pooled over the draws, worst parameter per case; `pytest -s tests/test_mvit_rounding_host.py`):
  case       bf16                                 fp16
  fixture    1.25 blocks.3.attn.qkv.bias          1.46 blocks.0.attn.norm_k.bias
  droppath   1.24 blocks.0.attn.rel_pos_w         1.39 blocks.0.attn.norm_k.bias
  (on one draw alone the norm_k.bias rows read up to 2.00: they are why the small tensors are pooled)
Observed on MI355X (tests/test_mvit_rounding_gpu.py, `-s`):
  statistic (bound)                          fp16: fixture, droppath             bf16: fixture, droppath
  features ratio (1.3)                       0.969, 0.999                        0.955, 0.979
  closer to the model than the oracle (1)    0.807, 0.812                        0.623, 0.724
  block outputs ratio (1.3)                  0.971 .. 1.008                      0.951 .. 1.000
  worst gradient ratio (1.6)                 0.980, 0.972                        1.013, 1.014
  per site: 16-bit-valued share of block outputs and of dxn (blocks 1, 3) 0.000; zero-lo share of rel <= 0.001; DropPath copies that
  differ from R(factor x gradient) 0.000; coarse share <= 0.016 (blocks.1.attn.rel_pos_h; patch_embed.proj.weight 0.014), both flavours
  the five largest e / allowed of a parameter (1):
    fp16 fixture   0.295 blocks.2.attn.norm_k.bias, 0.272 blocks.3.attn.norm_k.bias, 0.270 blocks.2.attn.rel_pos_h,
                   0.270 blocks.3.attn.norm_k.weight, 0.267 blocks.3.attn.norm_q.weight
    fp16 droppath  0.264 blocks.1.attn.norm_v.bias, 0.264 blocks.1.attn.norm_q.bias, 0.261 blocks.2.norm1.weight,
                   0.260 blocks.1.attn.norm_q.weight, 0.259 blocks.0.attn.norm_q.weight
    bf16 fixture   0.284 blocks.0.attn.norm_k.bias, 0.274 blocks.3.attn.norm_k.bias, 0.265 blocks.1.attn.norm_k.bias,
                   0.258 blocks.2.norm1.weight, 0.256 blocks.3.mlp.fc2.bias
    bf16 droppath  0.300 blocks.3.attn.norm_k.bias, 0.262 blocks.3.norm2.weight, 0.255 blocks.0.attn.pool_q.weight,
                   0.255 blocks.3.attn.proj.weight, 0.254 blocks.1.proj.weight
  `unpruned`, `down` and `up` read as `fixture` to three digits (the last block's 33-row output: 1.008 / 1.000).
  The tensors VERDICT.md asked about, relative error observed | predicted by the rounding model (fixture; droppath):
    fp16  patch_embed.proj.weight 5.90e-3 | 6.35e-3 (1.67e-2 | 1.74e-2)   rel_pos_h 1.06e-2 | 1.20e-2 (1.78e-2 | 1.82e-2)
          rel_pos_w 1.23e-2 | 1.26e-2 (2.53e-2 | 2.60e-2)                 rel_pos_t 9.21e-3 | 9.62e-3 (2.13e-2 | 1.86e-2)
    bf16  patch_embed.proj.weight 2.13e-2 | 2.19e-2 (4.45e-2 | 4.40e-2)   rel_pos_h 4.34e-2 | 4.28e-2 (5.78e-2 | 5.62e-2)
          rel_pos_w 3.84e-2 | 3.85e-2 (6.56e-2 | 6.47e-2)                 rel_pos_t 2.91e-2 | 2.94e-2 (5.49e-2 | 5.43e-2)
  They are operand rounding: block 0's tables and the stem sit behind every rounding of four blocks' backward, and their sums over all
  queries / rows cancel.
"""
import functools
import math
import os

import torch

import e2e_checks as ec
from attn_checks import ROW_FACTOR, MIN_ROWS
from oracle import mvit_oracle as mo
from oracle import mvit_rounded_oracle as mro
from oracle import rounded_oracle as ro
from oracle import timesformer_oracle as orc

TOL_RATIO, TOL_RATIO_GRAD = ec.TOL_RATIO, ec.TOL_RATIO_GRAD          # 1.3 on features and block outputs (observed 0.95-1.01), 1.6 on the worst gradient (0.97-1.01)
REL_Y_FACTOR = 8.0           # pool_attn_checks.REL_Y_FACTOR; with ROW_FACTOR = 4: largest e / allowed observed 0.30 (five largest: docstring)
N_PARAMS = 105
N_DRAWS = 8
LIVE_RMS = 1e-4
SITE_SHARE = 0.01            # an fp32 value is a 16-bit one when its low 13 (fp16) / 16 (bf16) mantissa bits vanish: 2^-13 of the entries at most
COARSE_SHARE = 0.05          # 8 zero low mantissa bits: 2^-8 = 0.4 % of the entries of an fp32 sum of many 22-bit products
SCALE_TARGET = 256.0         # grads.GradStore.SCALE_TARGET
DROPPATH_RATE, DROPPATH_SEED = 0.3, 3
CASES = ("fixture", "droppath", "unpruned", "down", "up")
K_OF = {"down": -12, "up": 12}
NAMED = ("patch_embed.proj.weight", "blocks.0.attn.rel_pos_h", "blocks.0.attn.rel_pos_w", "blocks.0.attn.rel_pos_t")


@functools.lru_cache(None)
def fixture():
    return torch.load(os.path.join(os.path.dirname(__file__), "golden", "mvit_small.pt"), weights_only=False)


@functools.lru_cache(None)
def state():
    g = fixture()
    sd = orc.seeded_state(mo.encoder_shapes(g["mvit"], g["cfg"]["frames"], g["cfg"]["crop"]), g["seed"])
    assert len(sd) == N_PARAMS and set(g["grads"]) <= set(sd)
    return sd


def droppath_draws(B, seed=DROPPATH_SEED):
    """per block (s_attn, s_mlp) = floor(keep + U) / keep, or None where the rate is 0 (MViTEngine.draw_droppath's formula, draws pinned)"""
    gen = torch.Generator().manual_seed(seed)
    depth = fixture()["cfg"]["depth"]
    out = []
    for rate in torch.linspace(0, DROPPATH_RATE, depth).tolist():
        keep = 1.0 - rate
        out.append(None if rate == 0.0 else tuple(torch.floor(keep + torch.rand(B, generator=gen)) / keep for _ in range(2)))
    return out


def base_case(name):
    """the case whose oracle runs serve `name`"""
    return "droppath" if name == "droppath" else "fixture"


@functools.lru_cache(None)
def inputs(name, draw=0):
    """-> dict(x, gout, droppath, prune, k): gout is the gradient fed at k = 0; the HIP path is fed gout * 2^k"""
    g = fixture()
    c = g["cfg"]
    if name == "droppath":
        gen = torch.Generator().manual_seed(23 + 1000 * draw)
        x = torch.randn(3, 3, c["frames"], c["crop"], c["crop"], generator=gen)
        gout = torch.randn(3, g["gout"].shape[1], generator=gen)
        return dict(x=x, gout=gout, droppath=droppath_draws(3), prune=True, k=0)
    x = g["x"] if draw == 0 else torch.randn(g["x"].shape, generator=torch.Generator().manual_seed(29 + 1000 * draw))
    return dict(x=x, gout=g["gout"], droppath=None, prune=name != "unpruned", k=K_OF.get(name, 0))


def scale_of(gout, operand):
    """S of GradStore.begin_scaled in exact arithmetic (1 unless the operands are fp16: the bf16 flavour does not scale)"""
    if operand != torch.float16:
        return 1.0
    a = min(max(float(gout.abs().max()), 1e-30), 3e38)
    return 2.0 ** min(max(math.floor(math.log2(SCALE_TARGET / a)), -100), 100)


DEFECTS = mro.DEFECTS + ("no_grad_scale",)      # the last one lives here: the fp16 flavour's backward run in true units (S = 1)


def oracle_step(x, gout, droppath, operand=None, variant=False, defect=None, double=False):
    """one step on the CPU -> dict(feat, blocks, grads).  operand None: mvit_oracle (fp32, or fp64 with `double`); else the rounding model,
    run as the engine runs: its backward fed S * gout, its gradients divided by S.  defect: one of `DEFECTS` (host test)."""
    cast = (lambda t: t.double()) if double else (lambda t: t.clone())
    p = {k: cast(v).requires_grad_(True) for k, v in state().items()}
    dp = None if droppath is None else [None if d is None else tuple(cast(s) for s in d) for d in droppath]
    outs = []
    if operand is None:
        feat = mo.forward_features(p, cast(x), fixture()["mvit"], block_outputs=outs, droppath=dp)
        S = 1.0
    else:
        S = 1.0 if defect == "no_grad_scale" else scale_of(gout, operand)
        mro.VARIANT, mro.DEFECT, mro.TAPS = variant, None if defect == "no_grad_scale" else defect, {}
        try:
            with ro.operand(operand):
                feat = mro.forward_features(p, x, fixture()["mvit"], block_outputs=outs, droppath=dp)
                feat.backward(gout * S)
        finally:
            sites, mro.TAPS = mro.TAPS, None
            mro.VARIANT, mro.DEFECT = False, None
    if operand is None:
        feat.backward(cast(gout))
        sites = None
    return dict(feat=feat.detach(), blocks=[o.detach() for o in outs], grads={k: v.grad / S for k, v in p.items()}, sites=sites)


def step_on_draws(step):
    """step(draw) -> what oracle_step / hip_step return; -> draw 0's result with `draws` = the gradients of the small tensors on draws 1 ..
    (every path that is judged runs ALL the draws: same inputs for the HIP path, the model and the variant)"""
    got = step(0)
    got["draws"] = [{k: v for k, v in step(d)["grads"].items() if small(k)} for d in range(1, N_DRAWS)]
    return got


def _err(a, b):
    return float((a.double() - b.double()).norm())


def _rel(a, b):
    return _err(a, b) / max(float(b.double().norm()), 1e-300)


def small(name):
    return state()[name].numel() < MIN_ROWS


def pooled(got, refs, f=1.0):
    """per parameter ||g - f ref|| / f; small tensors: over all N_DRAWS draws together (root of the summed squares)"""
    out = {}
    for k, r in refs[0].items():
        e2 = _err(got["grads"][k], r * f) ** 2
        if small(k):
            assert len(got["draws"]) == N_DRAWS - 1, "small tensors are judged over all draws: run step_on_draws"
            e2 += sum(_err(g[k], refs[d + 1][k] * f) ** 2 for d, g in enumerate(got["draws"]))
        out[k] = e2 ** 0.5 / f
    return out


@functools.lru_cache(None)
def references(base, operand):
    """everything the rule needs on the CPU for the case `base` (shared by the cases built on it and left unchanged): the fp32 oracle's step,
    the model's and the variant's (each on all draws), Y per parameter, and per parameter the pooled e(model) / e(variant)"""
    def run(**kw):
        def step(d):
            i = inputs(base, d)
            return oracle_step(i["x"], i["gout"], i["droppath"], **kw)
        return step_on_draws(step)
    ref, mod, var = run(), run(operand=operand), run(operand=operand, variant=True)
    i = inputs(base)
    r64 = oracle_step(i["x"], i["gout"], i["droppath"], double=True)
    refs = [ref["grads"]] + ref["draws"]
    return dict(ref=ref, refs=refs, model=mod, variant=var, Y={k: _err(ref["grads"][k], r64["grads"][k]) for k in ref["grads"]},
                em=pooled(mod, refs), ev=pooled(var, refs))


def spreads(base, operand):
    """-> [(spread, parameter, e(model), e(variant))], largest first (pooled errors); both errors zero: spread 1"""
    r = references(base, operand)
    rows = []
    for k in r["em"]:
        a, b = max(r["em"][k], r["ev"][k]), min(r["em"][k], r["ev"][k])
        rows.append((1.0 if a == 0.0 else a / max(b, 1e-300), k, r["em"][k], r["ev"][k]))
    return sorted(rows, reverse=True)


# the parameters the worst-gradient statistic leaves out, by name: a true gradient of 0 (norm_k.bias: a common shift of all keys is
# softmax-invariant) and the last block's structural zeros (only its cls query reaches the features)
NOT_LIVE = sorted([f"blocks.{i}.attn.norm_k.bias" for i in range(4)] +
                  ["blocks.3.attn.pool_q.weight", "blocks.3.attn.rel_pos_h", "blocks.3.attn.rel_pos_w", "blocks.3.attn.rel_pos_t"])


def live(ref_grads):
    """parameters of the worst-gradient rule (module docstring); exactly the complement of NOT_LIVE, or the rule is not applied at all"""
    rms = {k: float(v.norm()) / v.numel() ** 0.5 for k, v in ref_grads.items()}
    top = max(rms.values())
    lv = [k for k in ref_grads if rms[k] > LIVE_RMS * top]
    assert sorted(set(ref_grads) - set(lv)) == NOT_LIVE, sorted(set(ref_grads) - set(lv))
    return lv


# the gradients that are sums over all queries / all rows through accumulating or split reductions (rel_bwd_table_kernel, the stem's
# gemm_tn_into): hundreds of 16-bit x 16-bit products each, so their fp32 sums fill the mantissa.  (The last block's tables are exactly
# zero; a weight gradient of the pruned last block is a sum over the B cls rows only and is legitimately coarse with bf16 operands.)
# (rel_pos_t has 288 entries, a handful of which decide its share: like its error, the share is taken over all draws, 2,304 entries.)
ACCUMULATED = ("patch_embed.proj.weight",) + tuple(f"blocks.{i}.attn.rel_pos_{a}" for i in range(3) for a in "hwt")


def coarse_share(t):
    """share of the non-zero entries of an fp32 tensor whose low 8 mantissa bits are zero: 2^-8 for an fp32 sum of many products, ~1 for a sum
    formed in (or from a few partials of) a 16-bit type"""
    t = t.detach().float().contiguous()
    nz = t != 0
    return float(((t.view(torch.int32) & 0xFF) == 0)[nz].float().mean()) if bool(nz.any()) else 0.0


def judge(name, operand, got, models=("model", "variant")):
    """got: dict(feat [B, C], blocks list of [B, 1 + L, C] (cls FIRST; the last one may hold the cls row only), grads by name, draws, sites),
    all for the gradient gout * 2^k -> (findings [(label, value, bound)], table [(parameter, e(HIP) / bound, e(HIP), e(model), e(variant),
    rel(HIP), rel(model))]).  models: whose errors price a parameter (the host test judges the variant against the model alone)"""
    r = references(base_case(name), operand)
    ref, mod = r["ref"], r["model"]
    f = 2.0 ** inputs(name)["k"]
    out = []
    eh, emod = _rel(got["feat"], ref["feat"]), _rel(mod["feat"], ref["feat"])
    out.append((f"{name}: features error / rounding-model error ({eh:.2e} / {emod:.2e})", eh / emod, TOL_RATIO))
    out.append((f"{name}: features: closer to the rounding model than to the fp32 oracle", _rel(got["feat"], mod["feat"]) / eh, 1.0))
    assert len(got["blocks"]) == len(ref["blocks"])
    plan = mo.plan(fixture()["mvit"], fixture()["cfg"]["frames"], fixture()["cfg"]["crop"])[1]
    for i, b in enumerate(got["blocks"]):
        rows = slice(0, b.shape[1])
        eh, emod = _rel(b, ref["blocks"][i][:, rows]), _rel(mod["blocks"][i][:, rows], ref["blocks"][i][:, rows])
        out.append((f"{name}: block {i} output ({b.shape[1]} rows per clip) error / rounding-model error ({eh:.2e} / {emod:.2e})", eh / emod,
                    TOL_RATIO))
        out.append((f"{name}: block {i} output: share of entries that are exact {str(operand)[6:]} values (fp32 stream)",
                    mro.valued16(b, operand), SITE_SHARE))
        # per site, read off the path itself (module docstring): rel is a hi + lo pair; dxn is fp32 where the skip projection adds to it
        out.append((f"{name}: block {i} rel: share of entries whose lo half is zero (a pair, not one 16-bit value)",
                    1.0 - got["sites"]["rel_lo"][i], 0.5))
        if plan[i]["dim"] != plan[i]["dim_out"]:
            out.append((f"{name}: block {i} dxn = dqkv W_qkv: share of entries that are exact {str(operand)[6:]} values (fp32 where dim != dim_out)",
                        got["sites"]["dxn"][f"blocks.{i}."], SITE_SHARE))
            out.append((f"{name}: block {i} dxn + dxs W_skip as norm1's backward reads it: share of exact {str(operand)[6:]} values",
                        got["sites"]["dxn_sum"][f"blocks.{i}."], SITE_SHARE))
    dpi = inputs(name)["droppath"]
    if dpi is not None:                     # every DropPath factor goes into its 16-bit gradient copy BEFORE the cast: one site per factor
        casts = got["sites"].get("dp_cast", [])
        assert len(casts) == sum(2 for d in dpi if d is not None), (len(casts), "16-bit gradient copies with a DropPath factor")
        out.append((f"{name}: DropPath: largest share of a 16-bit gradient copy's entries that are not R(factor x fp32 gradient)", max(casts), SITE_SHARE))
    assert sorted(got["grads"]) == sorted(ref["grads"]) and len(got["grads"]) == N_PARAMS, "every encoder parameter is judged"
    lv = live(ref["grads"])
    wh = max((_rel(got["grads"][k], ref["grads"][k] * f), k) for k in lv)
    wm = max((_rel(mod["grads"][k], ref["grads"][k]), k) for k in lv)
    out.append((f"{name}: worst gradient error / rounding-model's ({wh[0]:.2e} {wh[1]} / {wm[0]:.2e} {wm[1]})", wh[0] / wm[0], TOL_RATIO_GRAD))
    table = []
    eg = pooled(got, r["refs"], f)
    for k in sorted(ref["grads"]):
        e, em, ev = eg[k], r["em"][k], r["ev"][k]
        bound = ROW_FACTOR * max(em if "model" in models else 0.0, ev if "variant" in models else 0.0)
        if em == 0.0 and ev == 0.0:         # no rounded operand reaches this gradient: the fp32 oracle's own error is all there is
            bound = REL_Y_FACTOR * r["Y"][k]
        else:                               # ... and where one does, that floor could never have been the binding term
            assert REL_Y_FACTOR * r["Y"][k] < ROW_FACTOR * max(em, ev), k
        ok = e <= bound
        nref = max(float(ref["grads"][k].norm()), 1e-300)
        table.append((k, (e / bound) if bound > 0 else (0.0 if ok else float("inf")), e, em, ev,
                      _err(got["grads"][k], ref["grads"][k] * f) / f / nref, _err(mod["grads"][k], ref["grads"][k]) / nref))
        out.append((f"{name}: d {k}: abs error {e:.3e} / allowed {bound:.3e} (model {em:.3e}, variant {ev:.3e}, Y {r['Y'][k]:.1e})",
                    table[-1][1], 1.0))
        if k in ACCUMULATED:            # (a small tensor: the share over all its draws together)
            ts = [got["grads"][k]] + ([g[k] for g in got["draws"]] if small(k) else [])
            out.append((f"{name}: d {k}: share of entries with 8 zero low mantissa bits (an fp32 sum, not a 16-bit accumulator)",
                        coarse_share(torch.cat([t.reshape(-1) for t in ts])), COARSE_SHARE))
    return out, table


def failures(findings):
    return [(label, v, b) for label, v, b in findings if not v <= b]


def report(tag, findings, table, top=5):
    """the figures that go beside the constants"""
    for label, v, b in findings:
        if ": d " not in label:
            print(f"[{tag}] {label}: {v:.3f} (<= {b:g})")
    print(f"[{tag}] largest coarse share of a gradient: " + "%.4f %s" % max((v, label.split(": d ")[1].split(":")[0]) for label, v, b in findings
                                                                          if "low mantissa" in label))
    for k, ratio, e, em, ev, relh, relm in sorted(table, key=lambda t: -t[1])[:top]:
        print(f"[{tag}]   d {k}: e / allowed {ratio:.3f}  (e {e:.3e}, model {em:.3e}, variant {ev:.3e}, rel {relh:.2e})")
    for k, ratio, e, em, ev, relh, relm in table:          # the tensors VERDICT.md asked about: observed next to predicted
        if k in NAMED:
            print(f"[{tag}]   d {k}: rel error observed {relh:.2e}, the rounding model predicts {relm:.2e}")


# ---------------------------------------------------------------------------------------------------------------------
# the HIP path (GPU)
# ---------------------------------------------------------------------------------------------------------------------
def build_engine_model():
    import mvit_checks as mc
    g = fixture()
    model, _ = mc._build_mvit(g, g["cfg"]["frames"], g["cfg"]["crop"])
    model.train()
    model.model.engine.use_graphs = False
    return model


def _tokens(t, B, C):
    """the engine's token matrix [B L + B, Cpad] (patch rows (b, l), then the B cls rows) -> [B, 1 + L, C], cls first"""
    L = t.shape[0] // B - 1
    t = t[:, :C].float().cpu()
    return torch.cat((t[B * L:].reshape(B, 1, C), t[:B * L].reshape(B, L, C)), 1)


class BackwardProbe:
    """reads two facts off a step's backward, the way grad_scale_checks.RowSumProbe does (wrapped entry points, no switch in product code):
    for every LayerNorm backward, how much of its incoming gradient is 16-bit-valued (1 when it IS a 16-bit tensor) -- the calls come in
    the order of MViTEngine._backward: the final norm, then per block from the last norm2, norm1 (`dxn_sum`); for the skip projection's
    backward GEMM (the only PVRL_EPI_RESID_F32 GEMM of the backward), the same share of its `aux`, which is dxn = dqkv W_qkv; and for every
    16-bit gradient copy that carries a DropPath factor (ln_bwd's fused copy, cast_scale), the share of its entries that differ from
    R(factor x the fp32 gradient it was made from)."""

    def __enter__(self):
        from procedurevrl_amd import ops, ops_mvit as om
        from procedurevrl_amd._lib import lib
        self.om, self.ops, self.ln, self.cs, self.gemm, self.calls, self.dp_cast, self.aux = om, ops, om.ln_bwd, ops.cast_scale, ops.gemm_nt, [], [], []
        resid_f32 = lib().PVRL_EPI_RESID_F32

        def differs(x16, x, rs):
            return float((x16.float() != (x * rs[:, None]).to(om.OP16).float()).float().mean())

        def ln_bwd(dy, *a, **kw):
            self.calls.append(1.0 if dy.dtype != torch.float32 else mro.valued16(dy, om.OP16))
            out = self.ln(dy, *a, **kw)
            if kw.get("want16") and kw.get("rowscale16") is not None:
                self.dp_cast.append(differs(out[1], out[0], kw["rowscale16"]))
            return out

        def gemm_nt(A, W, epi, *a, **kw):           # in the backward only the skip projection's GEMM adds into `aux`: aux is dxn = dqkv W_qkv
            if epi == resid_f32 and kw.get("aux") is not None:
                self.aux.append(1.0 if kw["aux"].dtype != torch.float32 else mro.valued16(kw["aux"], om.OP16))
            return self.gemm(A, W, epi, *a, **kw)

        def cast_scale(x, rowscale=None, out=None):
            res = self.cs(x, rowscale=rowscale, out=out)
            if rowscale is not None:
                self.dp_cast.append(differs(res, x, rowscale))
            return res
        om.ln_bwd, ops.cast_scale, ops.gemm_nt = ln_bwd, cast_scale, gemm_nt
        return self

    def __exit__(self, *a):
        self.om.ln_bwd, self.ops.cast_scale, self.ops.gemm_nt = self.ln, self.cs, self.gemm

    def dxn_sum(self, depth):
        assert len(self.calls) == 1 + 2 * depth, len(self.calls)
        return {f"blocks.{depth - 1 - j}.": self.calls[2 + 2 * j] for j in range(depth)}

    def dxn(self, plan):
        changes = [i for i in reversed(range(len(plan))) if plan[i]["dim"] != plan[i]["dim_out"]]
        assert len(self.aux) == len(changes), (len(self.aux), "PVRL_EPI_RESID_F32 GEMMs with an `aux` in the backward")
        return {f"blocks.{i}.": v for i, v in zip(changes, self.aux)}


def hip_step(model, name, graphs=False, draw=0):
    """one step of MViTEngine on the case's inputs -> what `judge` takes (blocks, sites: None when replayed from graphs)"""
    import mvit_checks as mc
    i = dict(inputs(base_case(name), draw), prune=inputs(name)["prune"], k=inputs(name)["k"])
    vt = model.model
    eng = vt.engine
    eng.prune_last, eng.use_graphs = i["prune"], graphs
    dp = None if i["droppath"] is None else [None if d is None else (d[0].to(mc.DEV), d[1].to(mc.DEV)) for d in i["droppath"]]
    model.zero_grad(set_to_none=True)
    feat = vt.forward_features(i["x"].to(mc.DEV), droppath=dp)
    blocks = sites = None
    dfeat = (i["gout"] * 2.0 ** i["k"]).to(mc.DEV)
    if not graphs:
        sv, B = eng.saved, i["x"].shape[0]
        plan = vt.video_encoder.plan
        mats = [sv["blocks"][j + 1]["x"] for j in range(len(plan) - 1)] + [sv["x_final"]]
        blocks = [_tokens(m, B, pl["dim_out"]) for m, pl in zip(mats, plan)]
        if i["prune"]:
            blocks[-1] = blocks[-1][:, :1]          # the pruned last block writes its cls rows only
        rel_lo = []
        for b in sv["blocks"]:                      # rel [BH, Lq, 2 JP]: hi | lo
            JP = b["rel"].shape[-1] // 2
            hi, lo = b["rel"][..., :JP].float(), b["rel"][..., JP:].float()
            rel_lo.append(float((lo != 0)[hi != 0].float().mean()))
        with BackwardProbe() as probe:
            feat.backward(dfeat)
        sites = dict(rel_lo=rel_lo, dxn=probe.dxn(plan), dxn_sum=probe.dxn_sum(len(plan)), dp_cast=probe.dp_cast)
    else:
        feat.backward(dfeat)
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().float().cpu().clone() for k, p in vt.video_encoder.named_parameters()}
    return dict(feat=feat.detach().float().cpu(), blocks=blocks, grads=grads, sites=sites)


def hip_case(model, name):
    """the case on all draws (small tensors are judged over all of them)"""
    return step_on_draws(lambda d: hip_step(model, name, draw=d))
