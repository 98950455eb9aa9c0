"""TIMESFORMER.ATTENTION_TYPE 'divided_space_time' on crops above 320^2 (more than 416 tokens per frame: the spatial attention takes
the streamed kernels, ops.attn_family) through the HIP encoder against the UNMODIFIED reference (tests/golden/divided_large.pt, written
by tests/golden/make_golden_divided_large.py): features and every parameter gradient at width 768, depth 2 (one unpruned and one pruned
block) under e2e_checks.TOL_ACT / TOL_GRAD / TOL_GSUM -- the bars the divided path meets at this depth at 224^2 -- with the last block
pruned, with its attention on all queries and unpruned; evaluation at a larger crop than the model was built for; HIP-graph replay; the
decoded-uint8 input path; a short training run; and the divided geometries at kernel level through the harnesses of attn_long_checks /
attn_checks under their own rule (pytest -m gpu).

On the commit before this one the engine tests fail in the first block:
    procedurevrl_amd._lib.PvrlError: pvrl_attn_fwd failed with status -1
(pvrl_attn_fwd keeps a whole sequence in LDS and refuses S = 442 > 416)."""
import os
import sys

import pytest
import torch

import attn_checks as ac
import attn_long_checks as alc
import e2e_checks as ec
from oracle import timesformer_oracle as orc

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
DEV = ec.DEV
PRUNE = {"pruned": (True, True), "attn_all_queries": (True, False), "unpruned": (False, False)}      # (prune_last, prune_attn)


@pytest.fixture(scope="module")
def gold():
    return ec.load("divided_large")


def _inputs(f):
    """twin of make_golden_divided_large.inputs_of"""
    g = torch.Generator().manual_seed(1000 + f["seed"])
    x = torch.randn(f["B"], 3, f["T"], f["crop"], f["crop"], generator=g)
    return x, torch.randn(f["B"], 768, generator=g)


def _model(f, prune=None):
    from procedurevrl_amd.build import build_model
    cfg = ec.make_cfg(f["depth"], f["model_crop"], f["K"], drop_path=f["drop_path"], frames=f["T"])
    cfg.TIMESFORMER.ATTENTION_TYPE = "divided_space_time"
    cfg.DATA.TEST_CROP_SIZE = f["crop"]
    cfg.DEV.TEST_LANG_EMB = torch.randn(f["K"], 512)
    cfg.TRAIN.LABEL_EMB = ""
    model = build_model(cfg, gpu_id=torch.device(DEV).index or 0)
    assert sorted(model.state_dict().keys()) == f["state_keys"]
    sd = orc.seeded_state({k: tuple(v.shape) for k, v in model.state_dict().items()}, f["seed"])
    assert abs(float(sum(v.double().abs().sum() for v in sd.values())) - f["wsum"]) <= 1e-9 * f["wsum"]
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV)
    eng = model.model.engine
    assert not eng.undivided
    if prune is not None:
        eng.prune_last, eng.prune_attn = prune
    return model


def _droppath(f, N):
    """the reference's captured torch.rand draws of block 1's three DropPath calls -- temporal [B * N], spatial [B * T], mlp [B]; block
    0's rate is 0 -- through the pinned-draw interface"""
    if not f["draws"]:
        return None
    from procedurevrl_amd.engine import EncoderEngine
    keep = 1.0 - f["drop_path"]
    s1, s2, s3 = (torch.floor(keep + u.float()) / keep for u in f["draws"])
    assert (s1.numel(), s2.numel(), s3.numel()) == (f["B"] * N, f["B"] * f["T"], f["B"])
    return [None, EncoderEngine.expand_droppath(s1.to(DEV), s2.to(DEV), s3.to(DEV), f["B"], N, f["T"])]


@pytest.mark.gpu
@pytest.mark.parametrize("prune", sorted(PRUNE))
@pytest.mark.parametrize("name", ["div_s442", "div_s442_t3_droppath"])
def test_features_and_gradients_match_the_reference(gold, name, prune):
    f = gold[name]
    model = _model(f, PRUNE[prune]).train()
    x, dfeat = _inputs(f)
    N = (f["crop"] // 16) ** 2
    assert N + 1 == 442
    feat = model.model.forward_features(x.to(DEV), droppath=_droppath(f, N))
    (feat * dfeat.to(DEV)).sum().backward()
    named = dict(model.named_parameters())
    res = [("features vs reference", ec.rel(feat, f["feat"]), ec.TOL_ACT)]
    res += [(f"grad {k[6:]}", ec.rel(named[k].grad, g), ec.TOL_GRAD) for k, g in f["grads"].items()]
    if "pos_embed_grad_rows" in f:
        res.append((f"grad pos_embed, every {f['pos_row_step']}th token row",
                    ec.rel(named["model.pos_embed"].grad[:, ::f["pos_row_step"]], f["pos_embed_grad_rows"]), ec.TOL_GRAD))
    worst, wk = 0.0, ""
    for k, s in f["grad_sums"].items():
        assert named[k].grad is not None, k
        e = abs(float(named[k].grad.double().abs().sum()) - s) / max(s, 1e-30)
        if e > worst:
            worst, wk = e, k
    res.append((f"worst sum |grad| over all {len(f['grad_sums'])} parameters ({wk})", worst, ec.TOL_GSUM))
    for label, e, tol in res:
        print(f"[{name}, {prune}] {label}: err={e:.3e} tol={tol:g}")
    assert sorted(k for k, p in named.items() if p.grad is None) == f["no_grad"]
    bad = [(label, e, tol) for label, e, tol in res if not e <= tol]
    assert not bad, bad


@pytest.mark.gpu
def test_eval_at_a_larger_test_crop_than_the_model_was_built_for(gold):
    """model at 224^2, DATA.TEST_CROP_SIZE 336: pos_embed resized by nearest neighbour (vit.py:375-386), eval mode"""
    f = gold["div_eval_resized"]
    model = _model(f).eval()
    assert tuple(model.model.pos_embed.shape) == (1, 197, 768)
    x, _ = _inputs(f)
    with torch.no_grad():
        feat = model.model.forward_features(x.to(DEV))
    e = ec.rel(feat, f["feat"])
    print(f"[div_eval_resized] features vs reference: err={e:.3e} tol={ec.TOL_ACT:g}")
    assert e <= ec.TOL_ACT
    # training with resized embeddings stays refused
    model.train()
    feat = model.model.forward_features(x.to(DEV))
    with pytest.raises(NotImplementedError, match="resized pos/time embeddings"):
        feat.sum().backward()


@pytest.mark.gpu
def test_graph_replay_of_the_streamed_divided_step_is_bit_equal(gold):
    f = gold["div_s442"]
    model = _model(f).train()
    eng = model.model.engine
    x, dfeat = _inputs(f)
    x, dfeat = x.to(DEV), dfeat.to(DEV)
    out = []
    for _ in range(eng.GRAPH_WARMUP + 3):
        model.zero_grad(set_to_none=True)
        feat = model.model.forward_features(x)
        (feat * dfeat).sum().backward()
        out.append((feat.detach().clone(), model.model.adopt_grads().flat.clone()))
    assert eng.use_graphs and len(eng._graphs) == 1, "the step was not captured"
    assert all("bwd" in g for g in eng._graphs.values())
    (f1, g1), (f2, g2) = out[-2], out[-1]                   # two replays
    assert torch.isfinite(f1).all() and torch.isfinite(g1).all()
    assert torch.equal(f1, f2) and torch.equal(g1, g2)
    assert torch.equal(out[0][0], f2) and torch.equal(out[0][1], g2), "replay differs from the eager launches"
    assert ec.rel(f2, f["feat"]) <= ec.TOL_ACT
    eng.release_graphs()
    assert len(eng._graphs) == 0


@pytest.mark.gpu
def test_decoded_uint8_clips_equal_the_materialised_tensor_bit_for_bit(gold):
    import numpy as np
    from procedurevrl_amd import ops
    from procedurevrl_amd.transform import DecodedClips, spatial_sampling_params
    f = gold["div_s442"]
    model = _model(f).eval()
    B, T, H0, W0, crop = 2, f["T"], 360, 480, f["crop"]
    g = torch.Generator().manual_seed(33)
    fr = torch.randint(0, 256, (B, T, H0, W0, 3), generator=g, dtype=torch.uint8).to(DEV)
    np.random.seed(5)
    prms = [spatial_sampling_params(H0, W0, -1, 340, 400, crop) for _ in range(B)]
    mean, std = model.model.cfg.DATA.MEAN, model.model.cfg.DATA.STD
    with torch.no_grad():
        got = model.model.forward_features(DecodedClips(fr, prms, mean, std, crop))
        x32 = ops.frames_u8_to_f32(DecodedClips(fr, prms, mean, std, crop))
        assert tuple(x32.shape) == (B, 3, T, crop, crop)
        want = model.model.forward_features(x32)
    assert torch.isfinite(got).all() and torch.equal(got, want)


@pytest.mark.gpu
def test_three_training_iterations_at_crop_336(tmp_path):
    """train_epoch raises at its log point on a non-finite loss or a skipped (bad) step: LOG_PERIOD 1 checks every iteration"""
    from procedurevrl_amd import train_net as tn
    from procedurevrl_amd.build import build_model
    from procedurevrl_amd.config import get_cfg
    from procedurevrl_amd.datasets import construct_loader, synthetic_label_emb
    from procedurevrl_amd.distributed import GradReducer
    from procedurevrl_amd.optimizer import construct_optimizer
    cfg = get_cfg()
    cfg.merge_from_list(["MODEL.MODEL_NAME", "vit_base_patch16_224_develop", "MODEL.PRETRAINED", "False",
                         "MODEL.NUM_CLASSES", "64", "MODEL.TEXT_MODEL", "clip_vit_b_16", "MODEL.LOSS_FUNC", "kldiv",
                         "MODEL.DROP_PATH", "0.1", "TIMESFORMER.DEPTH", "2", "TIMESFORMER.ATTENTION_TYPE", "divided_space_time",
                         "DATA.TRAIN_CROP_SIZE", "336", "DATA.NUM_FRAMES", "2", "DEV.MATCH_LANG_EMB", "True",
                         "DEV.ORDER_PRETRAIN_ENABLED", "True",
                         "TRAIN.BATCH_SIZE", "2", "TRAIN.TEXT", "synthetic", "NUM_GPUS", "1", "GLOBAL_BATCH_SIZE", "2",
                         "SOLVER.MAX_EPOCH", "1", "SOLVER.BASE_LR", "1e-4", "SOLVER.OPTIMIZING_METHOD", "adamw", "LOG_PERIOD", "1",
                         "SYNTHETIC.ENABLE", "True", "SYNTHETIC.NUM_VIDEOS", "6", "SYNTHETIC.TEXT_LAYERS", "2", "OUTPUT_DIR", str(tmp_path)])
    cfg.TRAIN.LABEL_EMB = synthetic_label_emb(64)
    torch.manual_seed(0)
    model = build_model(cfg)
    before = model.model.blocks[1].attn.qkv.weight.detach().clone()
    opt = construct_optimizer(model, cfg)
    line = tn.train_epoch(construct_loader(cfg, "train"), model, opt, GradReducer(model.model, enabled=False), 0, cfg, max_iters=3)
    assert line is not None and line["iter"].startswith("3/") and torch.isfinite(torch.tensor(line["loss"]))
    assert float(opt.dropped_steps()) == 0.0 if hasattr(opt, "dropped_steps") else True
    assert not torch.equal(model.model.blocks[1].attn.qkv.weight.detach(), before), "the encoder did not train"


# ---------------------------------------------------------------------------------------------------------------------
# kernel level: the divided geometries through the existing harnesses, under their rule (ROW_FACTOR, the lse bound)
# ---------------------------------------------------------------------------------------------------------------------
def _verdict(name, findings):
    print(f"\n== {name}\n{ac.report(findings)}")
    bad = [f for f in findings if not f.ok]
    assert not bad, f"{name}\n" + ac.report(bad)


# streamed kernels, mode 1 (cls_base = R = B * N * T > 0 in every case): 336^2 with two sequences per cls row, the first length the
# whole-sequence kernels refuse with an odd T, and TimeSformer-HR's 16 x 448^2 with every head column
HEAVY = ("randn", "peaked") + alc.NEW_REGIMES
LONG_TESTS = [(alc._long(1, 4, 442, 2, T=2), r) for r in alc.REGIMES] + [(alc._long(1, 6, 417, 2, T=3), r) for r in alc.REGIMES] + \
             [(alc._long(1, 16, 785, 12, T=16), r) for r in HEAVY]


@pytest.mark.gpu
@pytest.mark.parametrize("case,regime", LONG_TESTS, ids=[f"{alc.case_id(c)}-{r}" for c, r in LONG_TESTS])
def test_streamed_kernels_on_the_divided_geometries(case, regime):
    assert case.mode == 1 and case.T > 1 and (case.nseq // case.T) * (case.S - 1) * case.T > 0        # cls_base
    _verdict(f"{alc.case_id(case)}-{regime}", alc.check_case(case, regime))


# the pruned last block's cls-query kernels above 416 tokens (their own limit is ops.ATTN_CLS_MAX_S)
CLS_CASES = [ac.Case("cls", 1, B * T, S, H, T, ac.POW2, False, False, 8, z, "cls_fwd+cls_bwd" + ("" if z else "_nodq"))
             for (B, T, S, H) in [(2, 2, 442, 2), (1, 16, 442, 2), (2, 2, 785, 2), (1, 16, 785, 12)] for z in (True, False)]
CLS_TESTS = [(c, r) for c in CLS_CASES for r in ("randn", "peaked")]


@pytest.mark.gpu
@pytest.mark.parametrize("case,regime", CLS_TESTS, ids=[f"{ac.case_id(c)}-{r}" for c, r in CLS_TESTS])
def test_cls_query_kernels_above_416_tokens(case, regime):
    _verdict(f"{ac.case_id(case)}-{regime}", ac.check_case(case, regime))
