"""Global-norm clipping through optimizer.FusedOptimizer (`clip_grad_l2norm`, SOLVER.CLIP_GRAD_L2NORM), the data-parallel path and the
training loop.  The setup is that of tests/test_optimizer_gpu.py -- depth-2 model, two parameter groups, a changing LR, grad_scale = 1/4,
one parameter without a gradient at step 2, five steps -- and the reference is torch.optim on the CPU behind torch's clip_grad_norm_
formula with the sum of squares in float64 (tests/clip_checks.py: `reference_clip_`, the two bars and where they come from)."""
import json
import math
import os
import socket

import pytest
import torch

import clip_checks as cc
import optim_checks as oc

TOL = 1e-6                                      # tests/test_optimizer_gpu.py's bar for parameters and moments
# ... plus the coefficient's: it multiplies the gradient, so its relative error (<= COEF_BAR) enters exp_avg / the momentum buffer / the
# parameter once and exp_avg_sq (the gradient squared) twice
CLIP_TOL = TOL + 2 * cc.COEF_BAR
NESTEROV, DAMPENED = (0.9, 0.0, True), (0.9, 0.1, False)
METHODS = [("adamw", NESTEROV), ("adam", NESTEROV), ("sgd", NESTEROV), ("sgd", DAMPENED)]
IDS = ["adamw", "adam", "sgd-nesterov", "sgd-dampened"]


def _named(model):
    return [(n, p) for n, p in model.named_parameters() if p.requires_grad]


def _lr(step):
    return 1e-3 * (1.0 + 0.37 * step)


def _rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.gpu
@pytest.mark.parametrize("method,sgd", METHODS, ids=IDS)
def test_threshold_below_the_norm_on_every_step(method, sgd):
    """max_norm = half the fp64 norm of step 0: every step is clipped.  Parameters and moments against the reference, grad_norm and
    clip_coef after each step within their bars; the parameter without a gradient at step 2 is left out of that step's norm (the
    reference skips `grad is None`, and the norm bar is far below what one parameter contributes)."""
    from procedurevrl_amd.optimizer import set_lr
    cfg, model, opt = cc.small_model(method, sgd)
    named = _named(model)
    grads = cc.make_grads(named)
    max_norm = oc.f32(0.5 * cc.ref_norm(list(grads[0].values()), opt.grad_scale))
    opt.clip_grad_l2norm = max_norm
    cpu, ref = cc.torch_reference(cfg, opt, named, method)
    worst = {}
    for step in range(cc.STEPS):
        set_lr(opt, _lr(step))
        for g in ref.param_groups:
            g["lr"] = _lr(step) * g["lr_mult"]
        cc.set_grads(named, cpu, grads[step])
        assert (cpu[cc.SKIP_NAME].grad is None) == (step == cc.SKIP_STEP)
        total, coef = cc.reference_clip_([cpu[n].grad for n, _ in named if cpu[n].grad is not None], opt.grad_scale, max_norm)
        opt.step()
        ref.step()
        gn, cf = float(opt.grad_norm), float(opt.clip_coef)
        print(f"{method} step {step}: grad_norm {gn!r} (fp64 {total!r}, {_rel(gn, total):.2e}), clip_coef {cf!r} (fp64 {coef!r}, {_rel(cf, coef):.2e})")
        assert coef < 0.75, "the step is meant to be clipped"
        assert _rel(gn, total) <= cc.NORM_BAR, (step, gn, total)
        assert _rel(cf, coef) <= cc.COEF_BAR, (step, cf, coef)
        if step == cc.SKIP_STEP:                  # with the skipped parameter's stale slot in the sum the norm would be visibly larger
            stale = cc.ref_norm(list(grads[step].values()) + [grads[step - 1][cc.SKIP_NAME]], opt.grad_scale)
            assert _rel(stale, total) > 100 * cc.NORM_BAR
        for n, p in named:
            d = float((p.detach().cpu() - cpu[n].detach()).abs().max() / cpu[n].detach().abs().max())
            worst["param"] = max(worst.get("param", 0.0), d)
    worst.update(cc.state_worst(opt, ref, cpu, named, method))
    print(method, worst, "bar", CLIP_TOL)
    for k, v in worst.items():
        assert v <= CLIP_TOL, (method, k, v, worst)
    assert set(opt.state_dict()) == {"param_groups", "state", "fused"} and set(opt.state_dict()["fused"]) == {"steps", "method"}


@pytest.mark.gpu
@pytest.mark.parametrize("method,sgd", METHODS, ids=IDS)
def test_threshold_far_above_the_norm_changes_nothing(method, sgd):
    """coef = 1: parameters, moments and step counts torch.equal to a second FusedOptimizer with clipping off, fed the same gradients"""
    from procedurevrl_amd.optimizer import set_lr
    runs = []
    for max_norm in (1e6, 0.0):
        cfg, model, opt = cc.small_model(method, sgd)
        named = _named(model)
        grads = cc.make_grads(named)
        opt.clip_grad_l2norm = max_norm
        for step in range(cc.STEPS):
            set_lr(opt, _lr(step))
            for n, p in named:
                p.grad = grads[step][n].to(p.device) if n in grads[step] else None
            opt.step()
        torch.cuda.synchronize()
        if max_norm:
            assert float(opt.clip_coef) == 1.0 and 0.0 < float(opt.grad_norm) < 1e3
        runs.append((opt.flat_p.cpu(), opt.buf1.cpu(), None if opt.buf2 is None else opt.buf2.cpu(), list(opt.param_steps)))
    a, b = runs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and (a[2] is None or torch.equal(a[2], b[2])) and a[3] == b[3]
    assert float(a[1].abs().max()) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["adamw", "sgd"])
def test_padding_slots_of_a_run_are_zero_and_add_nothing(method):
    """the norm pass reads whole runs of the flat buffer, padding included (optim_checks.OddSizes: parameters of 1, 63, 65, 21, 1000, 64 and
    645 elements in 64-element spans): the norm is that of the parameters' own elements, and the padding stays bit-zero"""
    from procedurevrl_amd.optimizer import FusedOptimizer
    model = oc.OddSizes(torch.device("cuda:0"))
    ps = list(model.parameters())
    opt = FusedOptimizer([{"params": ps[:3], "weight_decay": 3e-3}, {"params": ps[3:], "weight_decay": 1e-2}], model, method, lr=1e-3)
    opt.grad_scale, opt.clip_grad_l2norm = 0.25, 0.125
    gs = model.grad_store()
    gen = torch.Generator().manual_seed(11)
    for step in range(3):
        gr = [torch.randn(p.shape, generator=gen) * 0.05 for p in ps]
        opt.zero_grad(set_to_none=True)
        for p, g in zip(ps, gr):
            p.grad = g.to(p.device)               # a foreign tensor: adopt_grads copies it into the view
        opt.step()
        total = cc.ref_norm(gr, 0.25)
        assert _rel(float(opt.grad_norm), total) <= cc.NORM_BAR and _rel(float(opt.clip_coef), cc.ref_coef(total, 0.125)) <= cc.COEF_BAR
    pad = torch.zeros(gs.end, dtype=torch.bool)
    for i, p in enumerate(gs.params):
        a, b = gs.span(i)
        pad[a + p.numel():b] = True
    assert int(pad.sum()) > 0
    for t in (gs.flat, opt.flat_p, opt.buf1) + (() if opt.buf2 is None else (opt.buf2,)):
        assert not oc._bits(t[:gs.end].cpu()[pad]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("method,sgd", METHODS, ids=IDS)
def test_non_finite_gradient_drops_the_clipped_step(method, sgd):
    """an inf in one gradient: the norm pass itself raises the flag (the separate scan is off: check_grads = False) -- weights and state
    bit-unchanged, dropped_steps() advances, grad_norm is not finite -- and the next clean step matches the reference"""
    from procedurevrl_amd.optimizer import set_lr
    cfg, model, opt = cc.small_model(method, sgd)
    named = _named(model)
    grads = cc.make_grads(named, steps=3, seed=7)
    grads[cc.SKIP_STEP][cc.SKIP_NAME] = grads[0][cc.SKIP_NAME].clone()      # (here every parameter has a gradient in all three steps)
    max_norm = oc.f32(0.5 * cc.ref_norm(list(grads[0].values()), opt.grad_scale))
    opt.clip_grad_l2norm, opt.check_grads = max_norm, False
    cpu, ref = cc.torch_reference(cfg, opt, named, method)
    snap = lambda: (opt.flat_p.clone(), opt.buf1.clone(), None if opt.buf2 is None else opt.buf2.clone())
    for step, bad in ((0, False), (1, True), (2, False)):
        set_lr(opt, _lr(step))
        cc.set_grads(named, cpu, grads[step])
        before = snap() if step else None
        if bad:
            named[5][1].grad.view(-1)[3] = float("inf")
            opt.step()
            assert all(b is None or torch.equal(a, b) for a, b in zip(snap(), before)), "a step with an inf gradient changed weights or state"
            assert not math.isfinite(float(opt.grad_norm))
            assert opt.dropped_steps() == 1 and float(opt.skip_flag) == 0.0
            continue
        for g in ref.param_groups:
            g["lr"] = _lr(step) * g["lr_mult"]
        total, _ = cc.reference_clip_([cpu[n].grad for n, _ in named], opt.grad_scale, max_norm)
        opt.step()
        ref.step()
        assert _rel(float(opt.grad_norm), total) <= cc.NORM_BAR
        assert opt.dropped_steps() == (1 if step == 2 else 0)
    worst = max(float((p.detach().cpu() - cpu[n].detach()).abs().max() / cpu[n].detach().abs().max()) for n, p in named)
    st = cc.state_worst(opt, ref, cpu, named, method)             # (asserts equal step counts: the dropped step was taken back)
    assert worst <= CLIP_TOL and all(v <= CLIP_TOL for v in st.values()), (worst, st)


@pytest.mark.gpu
@pytest.mark.parametrize("method,sgd", METHODS, ids=IDS)
def test_launch_sequence(method, sgd):
    """clipping off: step() launches the entry points without `clip` and nothing of the norm (a scan per unchecked run when check_grads, one update per run,
    the flag roll); clipping on: one pass per run of ALL gradients, one pvrl_clip_coef in front of every update, and NO scan"""
    from procedurevrl_amd._lib import lib
    from procedurevrl_amd.optimizer import set_lr
    cfg, model, opt = cc.small_model(method, sgd)
    named = _named(model)
    grads = cc.make_grads(named, steps=1)[0]
    set_lr(opt, 1e-3)
    upd = "pvrl_sgd_step" if method == "sgd" else "pvrl_adam_step"
    gs = model.model.grad_store()
    seen = {}
    for label, max_norm, check in (("off", 0.0, False), ("off_checked", 0.0, True), ("on", 1.0, True), ("on_unchecked", 1.0, False)):
        opt.clip_grad_l2norm, opt.check_grads = max_norm, check
        for n, p in named:
            p.grad = grads[n].to(p.device)
        names, undo = cc.count_calls(lib())
        try:
            opt.step()
        finally:
            undo()
        seen[label] = [n for n in names if n != "pvrl_sumsq_slots"]             # (a host query, not a launch)
    torch.cuda.synchronize()
    n_upd = len(opt._runs(gs, opt.param_groups[0]["params"], [True] * len(gs.params))) + \
        len(opt._runs(gs, opt.param_groups[1]["params"], [True] * len(gs.params)))
    n_all = len(opt._runs(gs, gs.params, [True] * len(gs.params), by_step=False))
    n_scan = len(opt._runs(gs, [p for i, p in enumerate(gs.params) if i not in gs.fused_checked], [True] * len(gs.params), by_step=False))
    assert n_upd >= 2 and n_scan >= 1
    assert seen["off"] == [upd] * n_upd + ["pvrl_flag_roll"]
    assert seen["off_checked"] == ["pvrl_nonfinite_flag_f32"] * n_scan + [upd] * n_upd + ["pvrl_flag_roll"]
    want_on = ["pvrl_sumsq_f32"] * n_all + ["pvrl_clip_coef"] + [upd + "_clip"] * n_upd + ["pvrl_flag_roll"]
    assert seen["on"] == want_on == seen["on_unchecked"]
    assert opt.dropped_steps() == 0


# ---- data parallel: gloo, world 2, both ranks on one device -----------------------------------------------------------------------------
DP_STEPS = 2


def _dp_grads(named, rank):
    return cc.make_grads(named, steps=DP_STEPS, seed=40 + rank)


def _dp_max_norm(named):
    g0, g1 = _dp_grads(named, 0)[0], _dp_grads(named, 1)[0]
    return oc.f32(0.5 * cc.ref_norm([g0[n] + g1[n] for n in g0], 0.5))


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch.distributed as dist
    from procedurevrl_amd import distributed as du
    from procedurevrl_amd.optimizer import set_lr
    torch.cuda.set_device("cuda:0")
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    cfg, model, opt = cc.small_model("adamw", NESTEROV)
    vt = model.model
    named = _named(model)
    opt.grad_scale, opt.clip_grad_l2norm = 1.0 / world, _dp_max_norm(named)
    reducer = du.GradReducer(vt)
    assert reducer.enabled
    gs = vt.grad_store()
    view = {id(p): v for p, v in zip(gs.params, gs.views)}
    out = []
    for step, d in enumerate(_dp_grads(named, rank)):
        set_lr(opt, _lr(step))
        opt.zero_grad(set_to_none=True)
        for n, p in named:
            view[id(p)].copy_(d[n])
            p.grad = view[id(p)]
        for i in reversed(range(len(vt.blocks))):
            vt.engine.grad_hook(i)                                   # what engine.backward() calls after each block
        reducer.finish()
        assert gs.reduced_over_ranks
        opt.step()
        out.append(dict(p=opt.flat_p.cpu(), norm=opt.grad_norm.cpu(), coef=opt.clip_coef.cpu()))
    assert opt.dropped_steps() == 0
    torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_two_ranks_compute_one_norm_from_the_reduced_buffer(tmp_path):
    """after reducer.finish() the buffer holds the rank sums: both ranks hold torch.equal parameters, grad_norm and clip_coef, equal to a
    single process stepping on the summed gradients with grad_scale = 1/2"""
    import torch.multiprocessing as mp
    from procedurevrl_amd.optimizer import set_lr
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    cfg, model, opt = cc.small_model("adamw", NESTEROV)
    named = _named(model)
    opt.grad_scale, opt.clip_grad_l2norm = 0.5, _dp_max_norm(named)
    ga, gb = _dp_grads(named, 0), _dp_grads(named, 1)
    for step in range(DP_STEPS):
        set_lr(opt, _lr(step))
        for n, p in named:
            p.grad = (ga[step][n] + gb[step][n]).to(p.device)
        opt.step()
        one = dict(p=opt.flat_p.cpu(), norm=opt.grad_norm.cpu(), coef=opt.clip_coef.cpu())
        for k in ("p", "norm", "coef"):
            assert torch.equal(r0[step][k], r1[step][k]), f"step {step}: the ranks disagree about {k}"
            assert torch.equal(r0[step][k], one[k]), f"step {step}: {k} differs from the single process on the summed gradients"
        assert float(one["coef"]) < 0.75 and math.isfinite(float(one["norm"]))


# ---- the training loop ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("clip", [1.0, 0.0], ids=["on", "off"])
def test_train_loop_logs_the_norm_only_when_clipping(tmp_path, capsys, clip):
    from procedurevrl_amd import train_net as tn
    from test_train_loop_gpu import _cfg
    cfg = _cfg(tmp_path)
    cfg.merge_from_list(["SOLVER.CLIP_GRAD_L2NORM", str(clip), "SOLVER.MAX_EPOCH", "1", "TRAIN.CHECKPOINT_PERIOD", "10"])
    _, opt = tn.train(cfg, max_iters=2)
    lines = [json.loads(l.split("json_stats: ", 1)[1]) for l in capsys.readouterr().out.splitlines() if "json_stats: " in l and '"train_iter"' in l]
    assert len(lines) == 1 and opt.clip_grad_l2norm == clip
    plain = {"_type", "epoch", "iter", "dt", "loss", "top1_err", "top5_err", "lr", "clips_per_s"}
    if clip:
        assert set(lines[0]) == plain | {"grad_norm"}
        assert math.isfinite(lines[0]["grad_norm"]) and lines[0]["grad_norm"] > 0.0
        assert abs(lines[0]["grad_norm"] - float(opt.grad_norm)) <= 1e-5 * max(1.0, float(opt.grad_norm))     # (the line is rounded to 5 decimals)
    else:
        assert set(lines[0]) == plain
