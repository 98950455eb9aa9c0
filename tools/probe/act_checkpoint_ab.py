"""MODEL.ACT_CHECKPOINT off / on in one process on one model (EncoderEngine.act_checkpoint): the two settings have different HIP-graph
keys, so both steps are captured; after warm-up they ALTERNATE for at least seven rounds of about a second per setting, timed with
device events.  Per configuration: clips/s with the flag off (S) and on (Sc), the time of a training forward alone (F), the spread
across rounds, `saved_nbytes()` and the peak allocated bytes of each setting -- and the one derived condition

    step_time(on) - step_time(off) <= F        (beyond the printed spread)

The recompute is a strict subset of the forward's launches; if it costs more than a forward, something is redone that the forward
does not do (weight casts, W_e rebuilds, an eager fall-back of the backward graph).

Configurations: `headline` ViT-B 32 x 8 x 224^2; `hr` ViT-B 8 x 16 x 448^2; `large_hr` ViT-L 16 x 448^2 with the flag ON only, at the
smallest batch whose plain saved activations (22 token-matrix widths per block, counted from the shapes) exceed the device's memory.
usage: python tools/probe/act_checkpoint_ab.py [--configs headline,hr,large_hr] [--rounds 7] [--seconds 1.0] [--eval-forward] [--large-clips N]
`--eval-forward`: also the time of a forward that keeps nothing (engine.forward(save=False), eval mode) at each configuration's shape; run
it from a checkout of an earlier commit as well for a before / after of PVRL_EPI_GELU_ONLY."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch  # noqa: E402

CONFIGS = {     # name: (model, depth, clips, frames, crop, both settings)
    "headline": ("vit_base_patch16_224_develop", 12, 32, 8, 224, True),
    "hr": ("vit_base_patch16_224_develop", 12, 8, 16, 448, True),
    "large_hr": ("vit_large_patch16_224_develop", 24, None, 16, 448, False),
}
WIDTHS = 22     # token-matrix widths of 16-bit rows a plain forward saves per block


def plain_saved_bytes(clips, frames, crop, C, depth):
    return clips * ((crop // 16) ** 2 * frames + 1) * C * 2 * WIDTHS * depth


def build(name, depth, frames, crop):
    from procedurevrl_amd.build import build_model
    from procedurevrl_amd.config import get_cfg
    cfg = get_cfg()
    cfg.MODEL.MODEL_NAME, cfg.MODEL.ARCH, cfg.MODEL.NUM_CLASSES = name, "vit", 64
    cfg.MODEL.PRETRAINED, cfg.MODEL.LOSS_FUNC, cfg.MODEL.DROP_PATH = False, "kldiv", 0.1
    cfg.TIMESFORMER.DEPTH = depth
    cfg.DEV.MATCH_LANG_EMB = True
    cfg.DEV.TEST_LANG_EMB = torch.randn(64, 512)
    cfg.DATA.NUM_FRAMES, cfg.DATA.TRAIN_CROP_SIZE = frames, crop
    cfg.NUM_GPUS = 1
    torch.manual_seed(0)
    model = build_model(cfg, gpu_id=0)
    with torch.no_grad():
        for blk in model.model.blocks:
            torch.nn.init.normal_(blk.temporal_fc.weight, std=0.02)
    return model.train()


def timed(fn, n):
    """-> milliseconds per call of fn() over n calls, by device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def run(name, args):
    mname, depth, clips, frames, crop, both = CONFIGS[name]
    dev = torch.device("cuda:0")
    model = build(mname, depth, frames, crop)
    vt, eng = model.model, model.model.engine
    if clips is None:
        total, per = torch.cuda.mem_get_info()[1], plain_saved_bytes(1, frames, crop, eng.C, depth)
        clips = args.large_clips or total // per + 1
        print(f"[{name}] device memory {total / 1e9:.1f} GB; plain saved activations {per / 1e9:.2f} GB per clip, {clips * per / 1e9:.1f} GB at "
              f"{clips} clips: {'do not fit' if clips * per > total else 'WOULD FIT'} without the flag (the plain step is not attempted)")
    g = torch.Generator(device=dev).manual_seed(1234)
    x = torch.randn(clips, 3, frames, crop, crop, device=dev, generator=g)
    dfeat = torch.randn(clips, eng.C, device=dev, generator=g)
    flags = (False, True) if both else (True,)

    def step():
        model.zero_grad(set_to_none=True)
        feat = vt.forward_features(x)
        (feat * dfeat).sum().backward()

    def fwd_only():
        vt.forward_features(x)
        eng.saved = None

    res = {f: dict(ms=[]) for f in flags}
    for f in flags:
        eng.act_checkpoint = f
        eng.use_graphs = False                      # saved bytes and the allocator's peak from eager steps (a replay allocates nothing)
        step()
        vt.forward_features(x)
        res[f]["saved"] = eng.saved_nbytes()
        eng.saved = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        res[f]["peak"] = torch.cuda.max_memory_allocated() - base
        eng.use_graphs = True                       # warm-up: the eager calls of the key, its captures, one replay
        for _ in range(eng.GRAPH_WARMUP + 2):
            step()
        res[f]["n"] = max(1, int(round(args.seconds * 1e3 / timed(step, 2))))
        assert eng.use_graphs and all(v.get("bwd") is not None for v in eng._graphs.values()), "the step is not replayed from HIP graphs"
    fwd_ms = []
    for _ in range(args.rounds):
        for f in flags:
            eng.act_checkpoint = f
            res[f]["ms"].append(timed(step, res[f]["n"]))
        eng.act_checkpoint = flags[-1]
        fwd_ms.append(timed(fwd_only, max(1, 3 * res[flags[-1]]["n"])))
    F = statistics.median(fwd_ms)
    print(f"[{name}] {mname} depth {depth}, {clips} clips of {frames} x {crop}^2, {args.rounds} alternating rounds")
    for f in flags:
        r = res[f]
        ms = statistics.median(r["ms"])
        print(f"[{name}]   ACT_CHECKPOINT {str(f):5s}: {1e3 * clips / ms:9.1f} clips/s  step {ms:9.3f} ms (spread {100 * spread(r['ms']):.2f} %, "
              f"{r['n']} steps per round)  saved {r['saved'] / 1e9:8.3f} GB  peak allocated above resident {r['peak'] / 1e9:8.3f} GB")
    print(f"[{name}]   training forward alone (flag {flags[-1]}): F = {F:.3f} ms (spread {100 * spread(fwd_ms):.2f} %)")
    if both:
        off, on = statistics.median(res[False]["ms"]), statistics.median(res[True]["ms"])
        noise = spread(res[False]["ms"]) * off + spread(res[True]["ms"]) * on
        ok = on - off <= F + noise
        print(f"[{name}]   recompute cost {on - off:.3f} ms = {(on - off) / F:.3f} F (+{100 * (on / off - 1):.1f} % step time); "
              f"step(on) - step(off) <= F beyond the spread ({noise:.3f} ms): {'holds' if ok else 'VIOLATED'}")
    if args.eval_forward:
        model.eval()
        nosave = lambda: eng.forward(x, training=False, save=False)
        with torch.no_grad():
            for _ in range(eng.GRAPH_WARMUP + 2):
                nosave()
            n = max(1, int(round(args.seconds * 1e3 / timed(nosave, 2))))
            ev = [timed(nosave, n) for _ in range(args.rounds)]
        print(f"[{name}]   forward that keeps nothing (save=False, eval): {statistics.median(ev):.3f} ms (spread {100 * spread(ev):.2f} %)")
    eng.release_graphs()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="headline,hr,large_hr")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--eval-forward", action="store_true")
    ap.add_argument("--large-clips", type=int, default=None, help="large_hr: clips instead of the smallest batch the plain path cannot keep")
    args = ap.parse_args()
    assert args.rounds >= 7, "at least seven alternating rounds"
    for name in args.configs.split(","):
        run(name, args)
        import gc
        gc.collect()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
