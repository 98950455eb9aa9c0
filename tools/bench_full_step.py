"""Side measurement (not the bench.py contract): the reference's FULL pre-training step at real size -- b videos x 9 clips
through the encoder, the frozen 12-layer CLIP text tower, the order/diffusion transformer, KL(top-5) + MSE, backward,
fused AdamW ("exercised in a separate 36-clip = 4 x 9 full-step run").
usage: python tools/bench_full_step.py [--arch vit|mvit] [--videos 4] [--steps 8] [--model NAME[:DEPTH] ...] [--rounds 1]

`--model` (arch vit; may be given several times) names a registered TimeSformer and optionally its TIMESFORMER.DEPTH, e.g.
    --model vit_base_patch16_224_develop --model vit_large_patch16_224_develop:24 --rounds 3
builds every model in ONE process and times them in alternating rounds of `--steps` steps (same box, same run: the first model's figure is
the yardstick of the others); one JSON line per model, with the encoder's executed FLOPs as a fraction of the dense MFMA peak."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="vit", choices=["vit", "mvit"])
    ap.add_argument("--videos", type=int, default=4)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=6)   # graphs are captured on the 3rd step; the next one is slow once
    ap.add_argument("--model", action="append", default=None, metavar="NAME[:DEPTH]",
                    help="registered TimeSformer model(s) to time (arch vit); default vit_base_patch16_224_develop at the config's depth")
    ap.add_argument("--rounds", type=int, default=1, help="timed rounds of --steps steps per model, the models alternating")
    ap.add_argument("--host-profile", action="store_true", help="cProfile the host side of the timed steps (stderr)")
    args = ap.parse_args()
    import torch
    from procedurevrl_amd._lib import OPERAND
    models = args.model or ["vit_base_patch16_224_develop"]
    if args.arch == "mvit":
        models = ["MViT"]
    runs = [_Run(args, spec) for spec in models]
    for r in runs:
        for _ in range(args.warmup):
            r.step()
    torch.cuda.synchronize()
    prof = None
    if args.host_profile:
        import cProfile
        prof = cProfile.Profile()
    for _ in range(max(1, args.rounds)):
        for r in runs:
            r.timed_round(args.steps, prof)
    if prof is not None:
        import pstats
        pstats.Stats(prof, stream=sys.stderr).sort_stats("tottime").print_stats(35)
    for r in runs:
        print(json.dumps(r.result(OPERAND)))


def encoder_train_gflop(vt, frames, crop=224):
    """executed GFLOP per clip of the TimeSformer encoder's training step (3 x forward; the matrix products alone): per block and token
    row 16 C^2 multiply-adds of GEMMs (qkv 3 + fused temporal map 1 + qkv 3 + proj 1 + MLP 8), the spatial and the temporal attention, the
    patch embedding; less what the pruned last block leaves out (EncoderEngine.prune_last / prune_attn).  At ViT-B, 8 frames: 3 x 367 of
    the reference's 3 x 391.66 (its temporal_fc is folded into the projection here)."""
    eng = vt.engine
    C, depth = vt.embed_dim, len(vt.blocks)
    N = (crop // 16) ** 2
    R = N * frames
    blk = 2.0 * R * 16 * C * C + 4.0 * R * (N + 1) * C + 4.0 * R * frames * C
    w = depth * blk + 2.0 * R * 768 * C
    if getattr(eng, "prune_last", False) and not eng.undivided:
        w -= 2.0 * R * 9 * C * C
        if getattr(eng, "prune_attn", False):
            w -= 4.0 * R * (N + 1) * C + 2.0 * R * C * C
    return 3 * w / 1e9


class _Run:
    """one model's full pre-training step, its timed rounds and its result line"""

    def __init__(self, args, spec):
        import torch
        from procedurevrl_amd.build import build_model
        from procedurevrl_amd.config import get_cfg
        from procedurevrl_amd.datasets import SyntheticHowTo100M, synthetic_label_emb
        from procedurevrl_amd.optimizer import construct_optimizer, set_lr
        from procedurevrl_amd.vit import pretrain_loss
        self.args, self.torch = args, torch
        cfg = self._cfg(args, spec, get_cfg())
        cfg.TRAIN.LABEL_EMB = synthetic_label_emb(9871, 512, seed=0)
        torch.manual_seed(0)
        self.cfg = cfg
        model = self.model = build_model(cfg, gpu_id=0).train()
        vt = self.vt = model.model
        vt.text_model.eval()
        opt = construct_optimizer(model, cfg)
        set_lr(opt, 5e-5)
        dev = torch.device("cuda", 0)
        ds = SyntheticHowTo100M(cfg, num_videos=args.videos, seed=1)
        items = [ds[i] for i in range(args.videos)]
        inputs = torch.stack([it[0] for it in items]).to(dev)
        meta = {k: torch.stack([it[3][k] for it in items]).to(dev) for k in ("clip_text_ids", "clip_vis_feat")}
        meta = {k: v.view(-1, v.shape[-1]) for k, v in meta.items()}

        def step():
            pred, teacher, mse = model([inputs, meta])
            loss, l1, l2 = pretrain_loss(pred, teacher, mse, cfg)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            vt.adopt_grads()
            opt.step()
            return loss
        self.step = step
        self.per_step, self.dts, self.enq, self.loss = [], [], [], None

    def _cfg(self, args, spec, cfg):
        cfg.merge_from_list(["MODEL.PRETRAINED", "False", "MODEL.NUM_CLASSES", "9871", "MODEL.TEXT_MODEL", "clip_vit_b_16",
                             "MODEL.LOSS_FUNC", "kldiv", "MODEL.DROP_PATH", "0.1", "DEV.MATCH_LANG_EMB", "True",
                             "DEV.ORDER_PRETRAIN_ENABLED", "True", "NUM_GPUS", "1", "SOLVER.OPTIMIZING_METHOD", "adamw"])
        self.frames = 8
        if args.arch == "mvit":
            self.frames = 16
            self.name = "MViTv2-S"
            cfg.MODEL.MODEL_NAME, cfg.MODEL.ARCH = "MViT", "mvit"
            cfg.DATA.INPUT_CHANNEL_NUM = [3]
            mv = cfg.MVIT
            mv.ZERO_DECAY_POS_CLS, mv.USE_ABS_POS, mv.REL_POS_SPATIAL, mv.REL_POS_TEMPORAL = False, False, True, True
            mv.DEPTH, mv.NUM_HEADS, mv.EMBED_DIM = 16, 1, 96
            mv.PATCH_KERNEL, mv.PATCH_STRIDE, mv.PATCH_PADDING = [3, 7, 7], [2, 4, 4], [1, 3, 3]
            mv.DROPPATH_RATE, mv.MODE, mv.CLS_EMBED_ON = 0.0, "conv", True
            mv.DIM_MUL = [[1, 2.0], [3, 2.0], [14, 2.0]]
            mv.HEAD_MUL = [[1, 2.0], [3, 2.0], [14, 2.0]]
            mv.POOL_KVQ_KERNEL, mv.POOL_KV_STRIDE_ADAPTIVE = [3, 3, 3], [1, 8, 8]
            mv.POOL_Q_STRIDE = [[i, 1, 2, 2] if i in (1, 3, 14) else [i, 1, 1, 1] for i in range(16)]
            mv.DIM_MUL_IN_ATT, mv.RESIDUAL_POOLING = True, True
        else:
            name, _, depth = spec.partition(":")
            cfg.MODEL.MODEL_NAME = name
            if depth:
                cfg.TIMESFORMER.DEPTH = int(depth)
            self.name = "ViT-B TimeSformer" if name == "vit_base_patch16_224_develop" else f"{name}, depth {cfg.TIMESFORMER.DEPTH}"
        cfg.DATA.NUM_FRAMES = self.frames
        cfg.DATA.TRAIN_CROP_SIZE = cfg.DATA.TEST_CROP_SIZE = 224
        return cfg

    def timed_round(self, steps, prof=None):
        torch = self.torch
        torch.cuda.synchronize()
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        if prof is not None:
            prof.enable()
        t0 = time.perf_counter()
        evs[0].record()
        for k in range(steps):
            self.loss = self.step()
            evs[k + 1].record()
        self.enq.append((time.perf_counter() - t0) / steps)
        if prof is not None:
            prof.disable()
        torch.cuda.synchronize()
        self.dts.append((time.perf_counter() - t0) / steps)
        self.per_step += [round(evs[k].elapsed_time(evs[k + 1]), 1) for k in range(steps)]

    def result(self, operand):
        args, frames = self.args, self.frames
        dt = sum(self.dts) / len(self.dts)
        t_enq = sum(self.enq) / len(self.enq)
        clips = args.videos * 9
        out = {"metric": f"training clips/sec ({frames}f x 224^2, {self.name}), "
                         "FULL pre-training step", "value": round(clips / dt, 3), "unit": "clips/s", "n_gpus": 1,
               "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * dt, 3), "higher_is_better": True,
               "scaling": "weak", "vs_baseline": None, "dtype": operand, "data": "synthetic",
               "config": {"workload": f"full pre-training step (reference cfg shape): {args.videos} videos x 9 clips of "
                                      f"{frames}x224^2, frozen CLIP-text teacher (12 layers, ctx 77) + order / diffusion "
                                      "transformer + top-5 KL + MSE, fwd+bwd+AdamW (SURVEY 8d's separate 36-clip run)",
                          "clips_per_gpu": clips, "global_batch": clips, "parallelism": "dp1"},
               "per_step_ms": self.per_step, "host_enqueue_ms_per_step": round(1e3 * t_enq, 3), "loss": float(self.loss)}
        if len(self.dts) > 1:
            out["rounds"] = len(self.dts)
            out["clips_per_s_per_round"] = [round(clips / d, 2) for d in self.dts]
        if args.arch == "vit":
            g = encoder_train_gflop(self.vt, frames)
            out["encoder"] = {"embed_dim": self.vt.embed_dim, "num_heads": self.vt.num_heads, "depth": len(self.vt.blocks),
                              "parameters_m": round(sum(p.numel() for p in self.vt.blocks.parameters()) / 1e6, 1),
                              "executed_gflop_per_clip": round(g, 2), "frac_of_bf16_peak": round(clips / dt * g * 1e9 / 2.5e15, 4)}
            out["hbm_reserved_gb"] = round(self.torch.cuda.max_memory_reserved() / 2 ** 30, 1)
        return out


if __name__ == "__main__":
    main()
