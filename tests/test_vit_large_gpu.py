"""`vit_large_patch16_224_develop` (embed_dim 1024, 16 heads) through the HIP encoder against the UNMODIFIED reference's VisionTransformer
at that width (tests/golden/vit_large.pt, written by tests/golden/make_golden_vit_large.py): features and every parameter gradient at
depth 2 (one unpruned and one pruned block) under e2e_checks.TOL_ACT / TOL_GRAD / TOL_GSUM -- the project's bars at this depth, per
operand flavour -- on the skinny / 128-tile GEMM paths (`l_small`), the persistent kernels at N, K in {1024, 3072, 4096} with DropPath
(`l_nt8`, also unpruned and in the bf16 flavour), the streamed spatial and cls-query attention with 16 heads (`l_stream`) and the undivided
block path (`l_joint`); HIP-graph replay; the decoded-uint8 input path; a short training run with a checkpoint resume (pytest -m gpu).

On the commit before this one every test fails at construction:
    AssertionError: kernels are built for ViT-B (C=768, head_dim=64)
(or, for the registered name, KeyError in the model registry).

Observed maxima on one MI355X (relative L2; fp16 operands, bars TOL_ACT 1e-3 / TOL_GRAD 2.5e-3 / TOL_GSUM 5e-3):
    case                          features   worst kept gradient   worst sum |grad| over all parameters
    l_small                       4.2e-4     8.7e-4                1.2e-4
    l_nt8                         2.2e-4     7.7e-4                1.1e-4
    l_nt8, PVRL_PRUNE_LAST=0      2.2e-4     7.5e-4                8.7e-5
    l_nt8, bf16 operands          1.9e-3     6.0e-3                8.9e-4      (bars 1e-2 / 2e-2 / 4e-2)
    l_nt8_nodrop, graph replay    2.3e-4     8.2e-4                7.8e-5
    l_stream                      2.6e-4     9.3e-4                7.4e-5
    l_joint                       4.9e-4     1.06e-3               7.6e-5"""
import os
import subprocess
import sys

import pytest
import torch

import e2e_checks as ec
from oracle import timesformer_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = ec.DEV
NAME = "vit_large_patch16_224_develop"
CASES = ["l_small", "l_nt8", "l_stream", "l_joint"]
ROWS = {"l_small": 66, "l_nt8": 4612, "l_stream": 2 * 441 * 2 + 2, "l_joint": 66}      # M = B * N * T + B


@pytest.fixture(scope="module")
def gold():
    return ec.load("vit_large")


def _inputs(f):
    """twin of make_golden_vit_large.inputs_of"""
    g = torch.Generator().manual_seed(1000 + f["seed"])
    x = torch.randn(f["B"], 3, f["T"], f["crop"], f["crop"], generator=g)
    return x, torch.randn(f["B"], f["width"], generator=g)


def _model(f):
    """the engine reads PVRL_PRUNE_LAST at construction: the caller sets it around this call"""
    from procedurevrl_amd.build import build_model
    cfg = ec.make_cfg(f["depth"], f["crop"], f["K"], drop_path=f["drop_path"], frames=f["T"])
    cfg.MODEL.MODEL_NAME = NAME
    cfg.TIMESFORMER.ATTENTION_TYPE = f["type"]
    cfg.DEV.TEST_LANG_EMB = torch.randn(f["K"], 512)
    cfg.TRAIN.LABEL_EMB = ""
    model = build_model(cfg, gpu_id=torch.device(DEV).index or 0)
    assert sorted(model.state_dict().keys()) == f["state_keys"]
    sd = orc.seeded_state({k: tuple(v.shape) for k, v in model.state_dict().items()}, f["seed"])
    assert abs(float(sum(v.double().abs().sum() for v in sd.values())) - f["wsum"]) <= 1e-9 * f["wsum"]
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV)
    eng = model.model.engine
    assert (eng.C, eng.H) == (1024, 16) and eng.undivided == (f["type"] != "divided_space_time")
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


def _errors(model, f, feat):
    """[(label, error, bar)]: features, the kept gradients, the worst sum |grad| over all parameters"""
    named = dict(model.named_parameters())
    res = [("features vs reference", ec.rel(feat, f["feat"]), ec.TOL_ACT)]
    res += [(f"grad {k[6:]}", ec.rel(named[k].grad, g), ec.TOL_GRAD) for k, g in f["grads"].items()]
    worst, wk = 0.0, ""
    for k, s in f["grad_sums"].items():
        assert named[k].grad is not None, k
        e = abs(float(named[k].grad.double().abs().sum()) - s) / max(s, 1e-30)
        if e > worst:
            worst, wk = e, k
    res.append((f"worst sum |grad| over all {len(f['grad_sums'])} parameters ({wk})", worst, ec.TOL_GSUM))
    assert sorted(k for k, p in named.items() if p.grad is None) == f["no_grad"]
    return res


def _step(model, f):
    x, dfeat = _inputs(f)
    N = (f["crop"] // 16) ** 2
    model.train(f["train"])
    model.zero_grad(set_to_none=True)
    feat = model.model.forward_features(x.to(DEV), droppath=_droppath(f, N))
    assert tuple(feat.shape) == (f["B"], 1024)
    (feat * dfeat.to(DEV)).sum().backward()
    return feat


def _verdict(tag, res):
    for label, e, tol in res:
        print(f"[{tag}] {label}: err={e:.3e} tol={tol:g}")
    bad = [(label, e, tol) for label, e, tol in res if not e <= tol]
    assert not bad, bad          # (observed on MI355X: at most 0.49 of the features' bar, 0.42 of the gradients', 0.03 of the sums': the table above)


PRUNED = [(c, "pruned") for c in CASES] + [("l_nt8", "unpruned")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,prune", PRUNED, ids=[f"{c}-{p}" for c, p in PRUNED])
def test_features_and_gradients_match_the_reference(gold, name, prune, monkeypatch):
    f = gold[name]
    assert f["B"] * (f["crop"] // 16) ** 2 * f["T"] + f["B"] == ROWS[name]
    monkeypatch.setenv("PVRL_PRUNE_LAST", "1" if prune == "pruned" else "0")
    model = _model(f)
    eng = model.model.engine
    assert eng.prune_last == (prune == "pruned") and eng.resid16 and eng.cls_fp32
    feat = _step(model, f)
    _verdict(f"{name}, {prune}", _errors(model, f, feat))


@pytest.mark.gpu
def test_l_nt8_in_the_bf16_flavour():
    """one library flavour per process: the case above in a child process with PVRL_OPERAND=bf16, under that flavour's e2e_checks bars"""
    env = dict(os.environ, PVRL_OPERAND="bf16")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_vit_large_gpu.py"), "-m", "gpu", "-q", "-x", "-s",
                        "-k", "test_features_and_gradients_match_the_reference and l_nt8-pruned", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-1000:]
    print(tail)
    assert r.returncode == 0, tail
    assert "1 passed" in r.stdout and "failed" not in r.stdout, tail


@pytest.mark.gpu
def test_graph_replay_of_the_l_nt8_step_stays_within_the_bars(gold):
    """two warm-up calls, then the captured step: its features and kept gradients under the same bars against the reference; afterwards
    release_graphs() leaves the model usable.  A captured step draws its own DropPath (pinned draws bypass the capture), so this is
    `l_nt8_nodrop`: l_nt8's clips and weights at MODEL.DROP_PATH 0, the reference run at that rate."""
    f = gold["l_nt8_nodrop"]
    assert f["drop_path"] == 0.0 and f["train"] and f["seed"] == gold["l_nt8"]["seed"] and f["wsum"] == gold["l_nt8"]["wsum"]
    model = _model(f).train()
    eng = model.model.engine
    assert eng.use_graphs and eng.GRAPH_WARMUP == 2
    x, dfeat = _inputs(f)
    x, dfeat = x.to(DEV), dfeat.to(DEV)
    out = []
    for _ in range(eng.GRAPH_WARMUP + 1):
        model.zero_grad(set_to_none=True)
        feat = model.model.forward_features(x)
        (feat * dfeat).sum().backward()
        out.append((feat.detach().clone(), model.model.adopt_grads().flat.clone()))
    assert len(eng._graphs) == 1 and all("bwd" in g for g in eng._graphs.values()), "the step was not captured"
    assert torch.equal(out[0][0], out[-1][0]) and torch.equal(out[0][1], out[-1][1]), "replay differs from the eager launches"
    _verdict("l_nt8_nodrop, graph replay", _errors(model, f, feat))
    eng.release_graphs()
    assert len(eng._graphs) == 0
    model.zero_grad(set_to_none=True)
    feat2 = model.model.forward_features(x)
    (feat2 * dfeat).sum().backward()
    assert torch.equal(feat2, out[0][0]) and torch.equal(model.model.adopt_grads().flat, out[0][1])


@pytest.mark.gpu
def test_decoded_uint8_clips_equal_the_materialised_tensor_bit_for_bit(gold):
    import numpy as np
    from procedurevrl_amd import ops
    from procedurevrl_amd.transform import DecodedClips, spatial_sampling_params
    f = gold["l_small"]
    model = _model(f).eval()
    B, T, H0, W0, crop = f["B"], f["T"], 48, 64, f["crop"]
    g = torch.Generator().manual_seed(33)
    fr = torch.randint(0, 256, (B, T, H0, W0, 3), generator=g, dtype=torch.uint8).to(DEV)
    np.random.seed(5)
    prms = [spatial_sampling_params(H0, W0, -1, 36, 44, crop) for _ in range(B)]
    mean, std = model.model.cfg.DATA.MEAN, model.model.cfg.DATA.STD
    with torch.no_grad():
        got = model.model.forward_features(DecodedClips(fr, prms, mean, std, crop))
        x32 = ops.frames_u8_to_f32(DecodedClips(fr, prms, mean, std, crop))
        assert tuple(x32.shape) == (B, 3, T, crop, crop)
        want = model.model.forward_features(x32)
        # the input kernels' bits do not depend on the model width: the same im2col operand either way ([rows, 768] pixels of a patch)
        a_u8 = ops.frames_u8_patchify(DecodedClips(fr, prms, mean, std, crop))
        a_f32 = ops.patchify(x32.contiguous())
    assert tuple(a_u8.shape) == (B * 4 * T, 768) and torch.equal(a_u8, a_f32)
    assert tuple(got.shape) == (B, 1024) and torch.isfinite(got).all() and torch.equal(got, want)


def _train_cfg(tmp):
    from procedurevrl_amd.config import get_cfg
    from procedurevrl_amd.datasets import synthetic_label_emb
    cfg = get_cfg()
    cfg.merge_from_list(["MODEL.MODEL_NAME", NAME, "MODEL.PRETRAINED", "False",
                         "MODEL.NUM_CLASSES", "64", "MODEL.TEXT_MODEL", "clip_vit_b_16", "MODEL.LOSS_FUNC", "kldiv",
                         "MODEL.DROP_PATH", "0.1", "TIMESFORMER.DEPTH", "2", "DATA.TRAIN_CROP_SIZE", "32",
                         "DEV.MATCH_LANG_EMB", "True", "DEV.ORDER_PRETRAIN_ENABLED", "True", "TRAIN.BATCH_SIZE", "2",
                         "TRAIN.TEXT", "synthetic", "NUM_GPUS", "1", "GLOBAL_BATCH_SIZE", "2", "SOLVER.MAX_EPOCH", "2",
                         "SOLVER.BASE_LR", "1e-4", "SOLVER.OPTIMIZING_METHOD", "adamw", "LOG_PERIOD", "1",
                         "TRAIN.CHECKPOINT_PERIOD", "1", "SYNTHETIC.ENABLE", "True", "SYNTHETIC.NUM_VIDEOS", "4",
                         "SYNTHETIC.TEXT_LAYERS", "2", "OUTPUT_DIR", str(tmp)])
    cfg.TRAIN.LABEL_EMB = synthetic_label_emb(64)
    return cfg


@pytest.mark.gpu
def test_four_training_steps_and_a_resume_after_the_second_reproduces_the_rest(tmp_path):
    """two epochs of two optimiser steps (pre-training head, depth 2, 32^2).  train_epoch raises at its log point on a non-finite loss or
    a skipped step: LOG_PERIOD 1 checks every iteration.  A `.pyth` saved after step 2, loaded into a fresh model and optimiser, gives
    steps 3-4 bit for bit: their losses, every weight and the optimiser's moments."""
    from procedurevrl_amd import checkpoint as cu
    from procedurevrl_amd import train_net as tn
    from procedurevrl_amd.build import build_model
    from procedurevrl_amd.datasets import construct_loader
    from procedurevrl_amd.distributed import GradReducer
    from procedurevrl_amd.optimizer import construct_optimizer

    def epoch(model, opt, cfg, e, losses):
        torch.manual_seed(100 + e)                   # the loader's shuffle, DropPath and the order transformer's draws
        seen = []
        orig = tn.log_json_stats
        tn.log_json_stats = lambda line: seen.append(line)
        try:
            line = tn.train_epoch(construct_loader(cfg, "train"), model, opt, GradReducer(model.model, enabled=False), e, cfg, max_iters=2)
        finally:
            tn.log_json_stats = orig
        assert line is not None and line["iter"].startswith("2/") and len(seen) == 2
        losses += [s["loss"] for s in seen]

    cfg = _train_cfg(tmp_path)
    torch.manual_seed(0)
    model = build_model(cfg)
    assert model.model.embed_dim == 1024 and model.model.engine.H == 16
    before = model.model.blocks[1].attn.qkv.weight.detach().clone()
    opt = construct_optimizer(model, cfg)
    losses = []
    epoch(model, opt, cfg, 0, losses)
    path = cu.save_checkpoint(str(tmp_path), model, opt, 0, cfg)
    assert path.endswith("checkpoint_epoch_00001.pyth")
    epoch(model, opt, cfg, 1, losses)
    assert len(losses) == 4 and all(torch.isfinite(torch.tensor(v)) for v in losses), losses
    assert float(opt.dropped_steps()) == 0.0
    assert not torch.equal(model.model.blocks[1].attn.qkv.weight.detach(), before), "the encoder did not train"

    cfg2 = _train_cfg(tmp_path)
    torch.manual_seed(7)                              # (another initialisation: everything that matters comes from the file)
    m2 = build_model(cfg2)
    o2 = construct_optimizer(m2, cfg2)
    assert cu.load_train_checkpoint(cfg2, m2, o2) == 1
    losses2 = []
    epoch(m2, o2, cfg2, 1, losses2)
    assert float(o2.dropped_steps()) == 0.0
    assert losses2 == losses[2:], (losses, losses2)
    for (k, a), (_, b) in zip(model.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    s1, s2 = opt.state_dict(), o2.state_dict()
    assert s1["fused"]["steps"] == s2["fused"]["steps"] == 4
    for k in s1["state"]:
        assert torch.equal(s1["state"][k]["exp_avg"], s2["state"][k]["exp_avg"]), k
        assert torch.equal(s1["state"][k]["exp_avg_sq"], s2["state"][k]["exp_avg_sq"]), k
