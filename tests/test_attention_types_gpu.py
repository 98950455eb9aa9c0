"""TIMESFORMER.ATTENTION_TYPE 'joint_space_time' / 'space_only' through the HIP encoder (engine.EncoderEngine's undivided block path)
against the UNMODIFIED reference (tests/golden/attn_types.pt, written by tests/golden/make_golden_attn_types.py): features and parameter
gradients at width 768, depth 2, held to e2e_checks.TOL_ACT / TOL_GRAD -- the bars the divided path meets at the same depth -- plus
HIP-graph replay and a short training run per scheme (pytest -m gpu).  The engine, like the divided path, produces no gradient for the
input frames; every parameter gradient is compared (selected tensors element-wise, sum |grad| of all of them)."""
import os
import sys

import pytest
import torch

import e2e_checks as ec
from oracle import timesformer_oracle as orc

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
DEV = ec.DEV


@pytest.fixture(scope="module")
def gold():
    return ec.load("attn_types")


def _inputs(f):
    """twin of make_golden_attn_types.inputs_of"""
    g = torch.Generator().manual_seed(1000 + f["seed"])
    x = torch.randn(f["B"], 3, f["T"], f["crop"], f["crop"], generator=g)
    return x, torch.randn(f["B"], 768, generator=g)


def _model(f):
    from procedurevrl_amd.build import build_model
    cfg = ec.make_cfg(f["depth"], f["crop"], f["K"], drop_path=f["drop_path"], frames=f["T"])
    cfg.TIMESFORMER.ATTENTION_TYPE = f["type"]
    cfg.DEV.TEST_LANG_EMB = torch.randn(f["K"], 512)
    cfg.TRAIN.LABEL_EMB = ""
    model = build_model(cfg, gpu_id=torch.device(DEV).index or 0)
    assert sorted(model.state_dict().keys()) == f["state_keys"]
    sd = orc.seeded_state({k: tuple(v.shape) for k, v in model.state_dict().items()}, f["seed"])
    assert abs(float(sum(v.double().abs().sum() for v in sd.values())) - f["wsum"]) <= 1e-9 * f["wsum"]
    model.load_state_dict(sd, strict=True)
    return model.to(DEV)


def _droppath(f, N):
    """the reference's captured torch.rand draws of block 1's two DropPath calls (block 0's rate is 0) -> forward(..., droppath=...)"""
    if not f["draws"]:
        return None
    from procedurevrl_amd.engine import EncoderEngine
    keep = 1.0 - f["drop_path"]
    s_attn, s_mlp = (torch.floor(keep + u.float()) / keep for u in f["draws"])
    return [None, EncoderEngine.expand_droppath_undivided(s_attn.to(DEV), s_mlp.to(DEV), f["B"], N, f["T"])]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["joint_s33", "joint_s513", "space_only", "joint_droppath"])
def test_features_and_gradients_match_the_reference(gold, name):
    f = gold[name]
    model = _model(f).train()
    x, dfeat = _inputs(f)
    N = (f["crop"] // 16) ** 2
    assert model.model.engine.undivided
    feat = model.model.forward_features(x.to(DEV), droppath=_droppath(f, N))
    (feat * dfeat.to(DEV)).sum().backward()
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
    for label, e, tol in res:
        print(f"[{name}] {label}: err={e:.3e} tol={tol:g}")
    bad = [(label, e, tol) for label, e, tol in res if not e <= tol]
    assert not bad, bad


@pytest.mark.gpu
def test_graph_replay_of_the_long_sequence_case_is_bit_equal(gold):
    f = gold["joint_s513"]
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


@pytest.mark.gpu
@pytest.mark.parametrize("attention_type", ["joint_space_time", "space_only"])
def test_three_training_iterations_on_the_synthetic_dataset(tmp_path, attention_type):
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
                         "MODEL.DROP_PATH", "0.1", "TIMESFORMER.DEPTH", "2", "TIMESFORMER.ATTENTION_TYPE", attention_type,
                         "DATA.TRAIN_CROP_SIZE", "32", "DEV.MATCH_LANG_EMB", "True", "DEV.ORDER_PRETRAIN_ENABLED", "True",
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
