"""The optimiser step of the full ViT-B pre-training model (AdamW, the flat buffers of every trainable parameter) with global-norm clipping
off and on (FusedOptimizer.clip_grad_l2norm), in one process on one optimiser: after warm-up the two settings ALTERNATE for at least seven
rounds of about a second each, timed with device events.  One real backward in front marks the parameters whose gradient producers raise
the skip flag themselves (GradStore.fused_checked: with clipping off and check_grads on, only the others are scanned); then every
parameter gets a gradient, as in a pre-training step.  Reported per setting: microseconds per step() and the gradient bytes the step reads
IN FRONT of the update kernels (off: the non-finite scan; on: the norm pass, which replaces it) -- the update kernels themselves move
28 bytes per parameter either way.  --reduced: as under data parallelism (GradStore.reduced_over_ranks: the scan covers everything).
A measurement, no threshold.
usage: python tools/probe/clip_ab.py [--rounds 7] [--seconds 1.0] [--max-norm 1.0] [--reduced]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch  # noqa: E402

from act_checkpoint_ab import spread, timed  # noqa: E402


def build():
    """bench.py's model: the ViT-B pre-training configuration with its language head"""
    from procedurevrl_amd.build import build_model
    from procedurevrl_amd.config import get_cfg
    from procedurevrl_amd.datasets import synthetic_label_emb
    from procedurevrl_amd.optimizer import construct_optimizer, set_lr
    cfg = get_cfg()
    cfg.MODEL.MODEL_NAME, cfg.MODEL.ARCH, cfg.MODEL.NUM_CLASSES = "vit_base_patch16_224_develop", "vit", 10588
    cfg.MODEL.PRETRAINED, cfg.MODEL.LOSS_FUNC, cfg.MODEL.DROP_PATH = False, "kldiv", 0.1
    cfg.DEV.MATCH_LANG_EMB = True
    cfg.DATA.NUM_FRAMES = 8
    cfg.NUM_GPUS = 1
    cfg.SOLVER.OPTIMIZING_METHOD, cfg.SOLVER.BASE_LR, cfg.SOLVER.WEIGHT_DECAY = "adamw", 5e-5, 1e-4
    torch.manual_seed(cfg.RNG_SEED)
    cfg.TRAIN.LABEL_EMB = synthetic_label_emb(10588, 512, seed=0)
    model = build_model(cfg, gpu_id=0).train()
    with torch.no_grad():
        for blk in model.model.blocks:
            torch.nn.init.normal_(blk.temporal_fc.weight, std=0.02)
    opt = construct_optimizer(model, cfg)
    set_lr(opt, cfg.SOLVER.BASE_LR)
    return model, opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--max-norm", type=float, default=1.0)
    ap.add_argument("--reduced", action="store_true")
    args = ap.parse_args()
    assert args.rounds >= 7, "at least seven alternating rounds"
    dev = torch.device("cuda:0")
    model, opt = build()
    vt = model.model
    g = torch.Generator(device=dev).manual_seed(1234)
    x = torch.randn(2, 3, 8, 224, 224, device=dev, generator=g)
    (vt.forward_features(x) * torch.randn(2, vt.engine.C, device=dev, generator=g)).sum().backward()      # fills GradStore.fused_checked
    gs = vt.adopt_grads()
    gs.flat[:gs.end].normal_(0.0, 1e-3, generator=g)
    for i, p in enumerate(gs.params):
        a, b = gs.span(i)
        gs.flat[a + p.numel():b].zero_()                        # the padding slots stay zero, as every writer leaves them
        p.grad = gs.views[i]
    gs.reduced_over_ranks = args.reduced
    had = [True] * len(gs.params)
    rest = [p for i, p in enumerate(gs.params) if args.reduced or i not in gs.fused_checked]
    read = {"off": 4 * sum(b - a for a, b, _ in opt._runs(gs, rest, had, by_step=False)) if opt.check_grads else 0,
            "on": 4 * sum(b - a for a, b, _ in opt._runs(gs, gs.params, had, by_step=False))}
    norms = {"off": 0.0, "on": args.max_norm}

    def step(name):
        def fn():
            opt.clip_grad_l2norm = norms[name]
            opt.step()
        return fn

    n = {}
    for name in norms:
        for _ in range(5):
            step(name)()
        n[name] = max(1, int(round(args.seconds * 1e3 / timed(step(name), 20))))
    us = {name: [] for name in norms}
    for _ in range(args.rounds):
        for name in norms:
            us[name].append(1e3 * timed(step(name), n[name]))
    nparam = sum(p.numel() for p in gs.params)
    print(f"[clip_ab] ViT-B pre-training model: {len(gs.params)} parameters, {nparam / 1e6:.1f} M elements ({gs.end / 1e6:.1f} M slots), adamw, "
          f"check_grads {opt.check_grads}, {len(gs.fused_checked)} parameters checked by their producers, reduced_over_ranks {args.reduced}; "
          f"{args.rounds} alternating rounds")
    med = {name: statistics.median(v) for name, v in us.items()}
    for name in norms:
        print(f"[clip_ab]   clipping {name:3s}: {med[name]:8.1f} us per step (spread {100 * spread(us[name]):.2f} %, {n[name]} steps per round), "
              f"{read[name] / 1e9:.3f} GB of gradients read in front of the update, {28 * gs.end / 1e9:.3f} GB moved by the update")
    print(f"[clip_ab]   on - off: {med['on'] - med['off']:+.1f} us, {(read['on'] - read['off']) / 1e9:+.3f} GB; grad_norm {float(opt.grad_norm):.6f}, "
          f"clip_coef {float(opt.clip_coef):.6f}, dropped steps {opt.dropped_steps()}")


if __name__ == "__main__":
    main()
