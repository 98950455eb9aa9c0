"""The all-token training step -- forward_features(x, cls=False), loss sum(tokens * dtok) -- against the cls step of the same build with
the last block unpruned (PVRL_PRUNE_LAST=0: the same blocks run in both; what differs is the final norm over every row, its backward,
and the gradient's entry), in one process on one model: the two steps have different HIP-graph keys, so both are captured; after warm-up
they ALTERNATE for at least seven rounds of about a second each, timed with device events.  A measurement, no threshold.
usage: python tools/probe/tokens_ab.py [--clips 32] [--frames 8] [--crop 224] [--depth 12] [--rounds 7] [--seconds 1.0]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch  # noqa: E402

from act_checkpoint_ab import build, spread, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=1.0)
    args = ap.parse_args()
    assert args.rounds >= 7, "at least seven alternating rounds"
    dev = torch.device("cuda:0")
    model = build("vit_base_patch16_224_develop", args.depth, args.frames, args.crop)
    vt, eng = model.model, model.model.engine
    eng.prune_last = False                          # (PVRL_PRUNE_LAST=0, before anything is captured)
    g = torch.Generator(device=dev).manual_seed(1234)
    x = torch.randn(args.clips, 3, args.frames, args.crop, args.crop, device=dev, generator=g)
    P = (args.crop // 16) ** 2 * args.frames
    dtok = torch.randn(args.clips, 1 + P, eng.C, device=dev, generator=g)
    dfeat = dtok[:, 0].contiguous()

    def cls_step():
        model.zero_grad(set_to_none=True)
        (vt.forward_features(x) * dfeat).sum().backward()

    def tok_step():
        model.zero_grad(set_to_none=True)
        (vt.forward_features(x, cls=False) * dtok).sum().backward()

    def tok_engine_step():                          # the engine alone: without autograd's own pass over the tokens (the product above)
        model.zero_grad(set_to_none=True)
        eng.forward(x, training=True, tokens=True)
        eng.backward(dtok, tokens=True)

    steps = dict(cls=cls_step, tokens=tok_step, tokens_engine=tok_engine_step)
    n = {}
    for name, step in steps.items():
        for _ in range(eng.GRAPH_WARMUP + 2):
            step()
        n[name] = max(1, int(round(args.seconds * 1e3 / timed(step, 2))))
    assert eng.use_graphs and len(eng._graphs) == 2 and all(v.get("bwd") is not None for v in eng._graphs.values()), "not replayed from HIP graphs"
    ms = {name: [] for name in steps}
    for _ in range(args.rounds):
        for name, step in steps.items():
            ms[name].append(timed(step, n[name]))
    print(f"[tokens_ab] ViT-B depth {args.depth}, {args.clips} clips of {args.frames} x {args.crop}^2, {args.rounds} alternating rounds, last block unpruned")
    med = {name: statistics.median(v) for name, v in ms.items()}
    for name in steps:
        print(f"[tokens_ab]   {name:14s} step {med[name]:9.3f} ms  {1e3 * args.clips / med[name]:8.1f} clips/s  (spread {100 * spread(ms[name]):.2f} %, "
              f"{n[name]} steps per round)")
    print(f"[tokens_ab]   all-token step - cls step: {med['tokens'] - med['cls']:+.3f} ms with autograd's loss product, "
          f"{med['tokens_engine'] - med['cls']:+.3f} ms for the engine alone")
    eng.release_graphs()


if __name__ == "__main__":
    main()
