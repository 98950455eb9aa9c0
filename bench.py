"""Headline benchmark: training clips/s of the TimeSformer ViT-B 8x224^2 step-matching path.

    python bench.py --gpus N --steps K --warmup W
(N > 1: launched by torch.distributed.run, one rank per GPU over RCCL).  A step is one full
training iteration over one synthetic batch resident in HBM: TimeSformer encoder forward, projection
head + step logits + top-5 KL loss + global InfoNCE over the all-gathered clip / text embeddings,
backward, gradient all-reduce (N > 1), fused AdamW step.
Prints ONE JSON line on rank 0 (see DESIGN.md "Measurement").  A plain run sets up, warms up, times the K steps and prints the
line; `--full` adds the per-kernel roofline, CPU baseline, sustained leg, side lines and parity probe.  `--dump-outputs DIR`
writes the last timed step's results as .npy files, for comparing two builds output for output.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

W_TRAIN_GFLOP = {8: 3 * 391.66 + 3 * 0.0008 + 3 * 0.0101}   # 3 x (encoder + head + logits) fwd GFLOP/clip
# the CPU baseline is 1 warm-up + the MEDIAN OF 3 timed 18-clip steps (~34 s each on 32 threads of an EPYC 9575F): the
# oracle keeps timing steps while this budget allows a further one (one warm-up and one timed step whatever it says)
CPU_BASELINE_BUDGET_S = 175.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32, help="clips per GPU (BASELINE config 2: 32)")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--classes", type=int, default=9871)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernel-timing", action="store_true")
    ap.add_argument("--host-profile", action="store_true", help="cProfile the host side of the timed steps (stderr)")
    ap.add_argument("--no-wgrad-overlap", action="store_true", help="weight-gradient GEMMs on the main stream (A/B switch)")
    ap.add_argument("--no-graphs", action="store_true", help="eager kernel launches instead of HIP-graph replay of the encoder")
    ap.add_argument("--no-wgrad-group", action="store_true", help="one launch per weight gradient instead of one per block")
    ap.add_argument("--no-side", action="store_true", help="skip the side measurements (configs[3] T=32 and configs[4] MViTv2-S) "
                                                           "that a --full single-GPU run appends to its JSON line")
    ap.add_argument("--all-sides", action="store_true", help="append the side lines (bf16 flavour, last block unpruned, full pre-training step, "
                                                             "configs[3] T = 32, configs[4] MViTv2-S) to a run that is not the default one")
    ap.add_argument("--sustained-steps", type=int, default=None,
                    help="back-to-back steps of the `sustained` leg after the timed region (default: 300 on a --full single-GPU run, else 0)")
    ap.add_argument("--world1-rccl", action="store_true",
                    help="one GPU, but through the N > 1 machinery: a 1-rank RCCL process group, the per-block gradient hook between staged "
                         "HIP-graph replays, RCCL's all-reduce / all-gather kernels on its own stream (what the data-parallel path costs a rank)")
    ap.add_argument("--parity-probe", action="store_true",
                    help="after the timed region: 2 clips of the SAME full-size model (12 blocks, 8x224^2, K=9871), one training "
                         "step vs the CPU oracle (checker only) -> `parity` in the JSON line (logits / loss / worst gradient error)")
    ap.add_argument("--from-host", action="store_true",
                    help="PCIe-inclusive variant (DESIGN section 5; never the headline `value`): every step's clips start in pinned HOST memory "
                         "and are copied to one of two device buffers on a copy stream while the previous step computes")
    ap.add_argument("--no-parity-probe", action="store_true", help="skip the 2-clip parity probe that --full appends to the default run and every --gpus N run")
    ap.add_argument("--arch", default="vit", choices=["vit", "mvit"],
                    help="vit = TimeSformer ViT-B, the BASELINE metric (configs[1]); mvit = MViTv2-S 16x224^2 (configs[4], side number)")
    ap.add_argument("--full", action="store_true",
                    help="also everything beyond the headline figure: the per-kernel timing / roofline leg, the CPU baseline, the "
                         "sustained leg, the side lines and the 2-clip parity probe (a plain run: set-up, warm-up, the timed steps, "
                         "the result line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32): loss, step "
                         "logits, clip embeddings, and fixed seeded samples of the updated parameters and of their gradients")
    args = ap.parse_args()
    if not args.full:
        # a plain run measures the headline and nothing else; the legs below stay reachable one by one through their own options
        args.no_kernel_timing = args.no_cpu_baseline = args.no_side = True
        args.no_parity_probe = args.no_parity_probe or not args.parity_probe

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` on its own: become N ranks, one process per GPU (the reference's launch_job spawns one
        # process per GPU the same way, lib/utils/misc.py:272-300 / tools/run_net.py:26-31) by re-executing under
        # torch.distributed.run exactly as the driver would launch it.
        return spawn_ranks(args.gpus)

    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("PVRL_DIST_BACKEND", "nccl")          # "gloo" = functional test of the N > 1 path on one GPU
    if os.environ.get("PVRL_SINGLE_DEVICE"):
        local_rank = 0
    comm_cus = 0
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        from procedurevrl_amd.distributed import reserve_comm_cus
        comm_cus = reserve_comm_cus(world)          # CUs per XCD left to RCCL (before the first launch / init_process_group)
        torch.cuda.set_device(local_rank)
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend=backend)
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    dp_path = world > 1
    if args.world1_rccl and world == 1:
        import socket
        sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=dev)
        dp_path = True

    from procedurevrl_amd import ops
    from procedurevrl_amd._lib import OPERAND            # the loaded library's 16-bit operand type: "bf16" | "f16"
    from procedurevrl_amd.config import get_cfg
    from procedurevrl_amd.build import build_model
    from procedurevrl_amd.datasets import synthetic_label_emb
    from procedurevrl_amd.distributed import AllGather, GradReducer
    from procedurevrl_amd.functional import kl_topk_loss, l2norm
    from procedurevrl_amd.losses import MILNCELoss
    from procedurevrl_amd.optimizer import construct_optimizer, set_lr

    cfg = get_cfg()
    cfg.MODEL.MODEL_NAME = "vit_base_patch16_224_develop"
    cfg.MODEL.ARCH = "vit"
    cfg.MODEL.NUM_CLASSES = args.classes
    cfg.MODEL.PRETRAINED = False
    cfg.MODEL.LOSS_FUNC = "kldiv"
    cfg.MODEL.DROP_PATH = 0.1
    cfg.DEV.MATCH_LANG_EMB = True
    cfg.DATA.NUM_FRAMES = args.frames
    if args.arch == "mvit":        # configs/HowTo100M/procedurevrl_mvitv2_adamw.yaml (MViTv2-S)
        if args.frames == 8:
            args.frames = 16
        cfg.MODEL.MODEL_NAME = "MViT"
        cfg.MODEL.ARCH = "mvit"
        cfg.DATA.NUM_FRAMES = args.frames
        cfg.DATA.INPUT_CHANNEL_NUM = [3]
        cfg.DATA.TRAIN_CROP_SIZE = cfg.DATA.TEST_CROP_SIZE = 224
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
    cfg.NUM_GPUS = 1
    cfg.SOLVER.OPTIMIZING_METHOD = "adamw"
    cfg.SOLVER.BASE_LR = 5e-5
    cfg.SOLVER.WEIGHT_DECAY = 1e-4
    torch.manual_seed(cfg.RNG_SEED + rank)
    cfg.TRAIN.LABEL_EMB = synthetic_label_emb(args.classes, 512, seed=0)   # tensor instead of a path (synthetic)
    model = build_model(cfg, gpu_id=local_rank)
    vt = model.model
    if args.arch == "vit":
        with torch.no_grad():   # randomise the branches that the reference zero-initialises so no kernel is idle
            for blk in vt.blocks:
                torch.nn.init.normal_(blk.temporal_fc.weight, std=0.02)
            torch.nn.init.trunc_normal_(vt.time_embed, std=0.02)
    model.train()
    if args.no_wgrad_overlap:
        vt.engine.overlap_wgrad = False
    if args.no_wgrad_group and hasattr(vt.engine, "group_wgrad"):
        vt.engine.group_wgrad = False
    graphs = hasattr(vt.engine, "use_graphs") and vt.engine.use_graphs and not args.no_graphs
    if hasattr(vt.engine, "use_graphs"):
        vt.engine.use_graphs = graphs
    optimizer = construct_optimizer(model, cfg)
    set_lr(optimizer, cfg.SOLVER.BASE_LR)
    optimizer.grad_scale = 1.0 / world
    reducer = GradReducer(vt, enabled=dp_path, find_unused=False)     # every parameter gets a gradient every step: no per-step host sync

    B = args.batch
    g = torch.Generator(device=dev).manual_seed(1234 + rank)
    frames = torch.randn(B, 3, args.frames, 224, 224, device=dev, generator=g)
    teacher = torch.randn(B, args.classes, device=dev, generator=g) * 4.0
    text_emb = l2norm(torch.randn(B, 512, device=dev, generator=g))        # stand-in for the frozen CLIP-text embeddings
    nce = MILNCELoss()

    host_frames = copy_stream = None
    if args.from_host:
        host_frames = frames.cpu().pin_memory()
        copy_stream = torch.cuda.Stream(device=dev)
        dev_bufs = [frames, torch.empty_like(frames)]
        staged = {"i": 0, "ev": None}

        def stage():            # the NEXT step's batch: host -> device on the copy stream, behind the consumer of the buffer it overwrites
            staged["i"] ^= 1
            copy_stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(copy_stream):
                dev_bufs[staged["i"]].copy_(host_frames, non_blocking=True)
                staged["ev"] = copy_stream.record_event()
        stage()

    last = {}

    def step():
        optimizer.zero_grad(set_to_none=True)
        if args.from_host:
            torch.cuda.current_stream().wait_event(staged["ev"])
            cur = dev_bufs[staged["i"]]
            pred = model(cur)
            stage()
        else:
            pred = model(frames)
        last["pred"] = pred
        loss = kl_topk_loss(pred, teacher, 5)                                # step matching (tools/train_net.py:152-160)
        v = vt.last_video_emb                                                # unit-norm clip embeddings [B, 512]
        v_all, t_all = (AllGather.apply(v), AllGather.apply(text_emb)) if dp_path else (v, text_emb)
        loss = loss + nce(v_all * (1.0 / 0.07 ** 0.5), t_all * (1.0 / 0.07 ** 0.5))   # global InfoNCE over all ranks' clips
        loss.backward()
        reducer.finish()
        optimizer.step()
        return loss

    def barrier():
        if dp_path:
            dist.barrier()
        torch.cuda.synchronize()

    if graphs:      # set-up, like building the model: the encoder's launch sequence is captured into HIP graphs on its
        for _ in range(vt.engine.GRAPH_WARMUP + 2):   # third call, whatever --warmup is; the first replay-only step after
            step()                                     # a capture is slow too (measured 0.1-1 s once), so it is set-up as well
        if not args.no_kernel_timing:                  # and one eager, event-instrumented step: the timed region ends with one
            ops.KERNEL_TIMING = []
            vt.engine.use_graphs = False
            step()
            ops.KERNEL_TIMING = None
            vt.engine.use_graphs = True
            step()
    for _ in range(args.warmup):
        loss = step()
    barrier()
    if dp_path:
        reducer.diag = True       # events around every chunk's collective and around the main stream's wait for them (`comm` in the line)
        reducer.diag_reset()
    # Per-kernel HIP events cannot be recorded inside a captured graph (ROCm refuses external event nodes), so with
    # graphs the LAST step of the timed region is issued eagerly -- the same kernels, launched one by one -- and carries
    # the events; without graphs every step does.
    timing_steps = set() if args.no_kernel_timing else ({args.steps - 1} if graphs else set(range(args.steps)))
    prof = None
    if args.host_profile:
        import cProfile
        prof = cProfile.Profile()
        prof.enable()
    t0 = time.perf_counter()
    timed_events = []
    for k in range(args.steps):
        if k in timing_steps:
            ops.KERNEL_TIMING = timed_events
            vt.engine.use_graphs = False
        loss, pred = step(), last["pred"]
        if k in timing_steps:
            ops.KERNEL_TIMING = None
            vt.engine.use_graphs = graphs
    if prof is not None:
        import pstats
        prof.disable()
        pstats.Stats(prof, stream=sys.stderr).sort_stats("tottime").print_stats(45)
    t_enq = time.perf_counter() - t0      # host time to enqueue the K steps (informational: launch-bound if ~ dt)
    barrier()
    dt = time.perf_counter() - t0
    t = torch.tensor([dt], device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t.item())
    if args.dump_outputs and rank == 0:     # now, before any further step (sustained / isolated legs) overwrites the graphs' buffers
        dump_outputs(args.dump_outputs, model, loss, pred, vt.last_video_emb)
    ops.KERNEL_TIMING = timed_events if timing_steps else None
    timing = ops.collect_kernel_timing() if timing_steps else None
    ops.KERNEL_TIMING = None
    comm_diag = None
    if dp_path:
        comm_diag = reducer.diag_summary()          # rank-local (the device is idle behind barrier())
        reducer.diag = False
        if comm_diag is not None and world > 1:     # ... and the slowest rank's exposed wait next to rank 0's
            ex = torch.tensor([comm_diag["exposed_ms_per_step"], comm_diag["allreduce_ms_per_step"]], device=dev, dtype=torch.float64)
            dist.all_reduce(ex, op=dist.ReduceOp.MAX)
            comm_diag["exposed_ms_per_step_max_over_ranks"] = round(float(ex[0]), 3)
            comm_diag["allreduce_ms_per_step_max_over_ranks"] = round(float(ex[1]), 3)
    # sustained leg: the timed region above is ~1 s on a chip that runs this step at its power limit -- does the figure hold?  N more
    # steps back to back (HIP-graph replays, nothing else), one event per 50-step window on the main stream, no host sync inside.
    default_run = world == 1 and args.arch == "vit" and args.frames == 8 and not args.no_side and not args.no_cpu_baseline
    n_sus = args.sustained_steps if args.sustained_steps is not None else (300 if default_run else 0)
    sustained = None
    if n_sus >= 100:
        win = 50
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(n_sus // win + 1)]
        barrier()
        evs[0].record()
        for k in range(n_sus // win):
            for _ in range(win):
                step()
            evs[k + 1].record()
        barrier()
        ms = [evs[k].elapsed_time(evs[k + 1]) for k in range(n_sus // win)]
        per_win = [round(B * world * win / (m * 1e-3), 1) for m in ms]
        sustained = {"steps": (n_sus // win) * win, "window": win, "clips_per_s_per_window": per_win,
                     "clips_per_s": round(B * world * (n_sus // win) * win / (sum(ms) * 1e-3), 2),
                     "last_window_vs_value": None}
    # isolated leg (untimed, not part of `value`): the same step with the weight-gradient GEMMs on the main stream, so
    # that a launch's event-timed duration is the kernel's own and not its share of a GPU it co-runs on with the dgrad
    # chain (under overlap the TN and NT kernels each see about half the CUs and their durations double)
    isolated = None
    if timing and getattr(vt.engine, "overlap_wgrad", False):
        vt.engine.use_graphs = False
        vt.engine.overlap_wgrad = False
        step(); barrier()
        ops.KERNEL_TIMING = []
        for _ in range(min(args.steps, 3)):
            step()
        barrier()
        iso = ops.collect_kernel_timing()
        ops.KERNEL_TIMING = None
        vt.engine.overlap_wgrad = True
        vt.engine.use_graphs = graphs
        def iso_of(kernel):
            if not iso or kernel not in iso["summary"]:
                return None
            k = iso["summary"][kernel]
            return {"achieved": k["tflops"], "frac": round(k["tflops"] / 2500.0, 4), "avg_launch_us": k["avg_us"],
                    "note": "same step, wgrad overlap off (kernel alone on the GPU)"}
        isolated = iso_of(timing["roofline"]["kernel"])
        if "runner_up" in timing["roofline"]:
            ru = iso_of(timing["roofline"]["runner_up"]["kernel"])
            if ru:
                timing["roofline"]["runner_up"]["isolated"] = ru

    if rank == 0:
        clips = B * world * args.steps
        value = clips / dt
        value_note = None
        if sustained:
            sustained["last_window_vs_value"] = round(sustained["clips_per_s_per_window"][-1] / value, 4)
            if sustained["clips_per_s_per_window"][-1] < 0.98 * value:      # the short region flattered the chip: report what holds
                value_note = (f"the {args.steps}-step timed region gave {value:.1f} clips/s but the last 50-step window of the sustained leg is "
                              f">2 % below it: `value` is the sustained figure over {sustained['steps']} steps")
                value = sustained["clips_per_s"]
                dt = args.steps * B * world / value
        wtrain = W_TRAIN_GFLOP.get(args.frames, W_TRAIN_GFLOP[8] * args.frames / 8) * 1e9
        if args.arch == "mvit":
            wtrain = 3 * 128.45e9 * args.frames / 16      # MViTv2-S forward 128.45 GFLOP/clip at 16 frames
        # what the kernels actually execute: with EncoderEngine.prune_last the LAST block's spatial projection and MLP (SURVEY 8d per
        # block and clip at T = 8: proj 1.86 + fc1 7.40 + fc2 7.40 GFLOP forward) run on the cls rows only, forward and both backward
        # GEMMs -- the reference computes them for all 1,569 tokens and reads one.  The hardware figures below count executed work.
        wexec = wtrain
        if args.arch == "vit" and getattr(vt.engine, "prune_last", False):
            wexec = wtrain - 3 * (1.86 + 7.40 + 7.40) * 1e9 * args.frames / 8
            if getattr(vt.engine, "prune_attn", False):     # ... its spatial attention for the cls query only (0.954 GFLOP of bmm per block
                wexec -= 3 * (0.95 + 5.58 / 3) * 1e9 * args.frames / 8      # and clip) and the query third of its spatial qkv GEMM (5.58 / 3)
        out = {
            "metric": f"training clips/sec ({args.frames}f x 224^2, ViT-B TimeSformer)" if args.arch == "vit" else
                      f"training clips/sec ({args.frames}f x 224^2, MViTv2-S)", "value": round(value, 3), "unit": "clips/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * dt / args.steps, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": OPERAND, "data": "synthetic",
            "config": {"workload": ("MViTv2-S " if args.arch == "mvit" else "TimeSformer ViT-B ") +
                                   f"{args.frames}x224^2, {B} clips/GPU, K={args.classes} step logits, "
                                   "top-5 KL + all-gather InfoNCE, fwd+bwd+AdamW (BASELINE configs[1]; configs[2] at 8 GPUs)",
                       "clips_per_gpu": B, "global_batch": B * world, "parallelism": f"dp{world}",
                       "last_block": ("cls rows only (projection, MLP, spatial attention: only x[:, 0] of its output is read, "
                                      "vit.py:418-421; side[1] = all tokens)") if getattr(vt.engine, "prune_last", False) else "all tokens"},
            "comm": None if not dp_path else {"backend": backend, "ranks": dist.get_world_size(),
                                             "rccl": rccl_version(torch) if backend == "nccl" else None,
                                             "cus_per_xcd_left_to_rccl": comm_cus, "compute_cus_per_xcd": os.environ.get("PVRL_COMPUTE_CUS"),
                                             "nccl_max_nchannels": os.environ.get("NCCL_MAX_NCHANNELS"),
                                             "grad_allreduce_mb": round(vt.grad_store().flat.numel() * 4 / 2 ** 20, 1),
                                             "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "default (4)"),
                                             "hook_group": getattr(vt.engine, "hook_group", None),
                                             **(comm_diag or {})},
            "inputs": "pinned host memory, copied per step on a copy stream (PCIe-inclusive)" if args.from_host else "resident in HBM",
            "loss": float(loss.item()), "hip_graphs": bool(graphs), "hbm_reserved_gb": round(torch.cuda.max_memory_reserved() / 2 ** 30, 1),
            "host_enqueue_ms_per_step": round(1e3 * t_enq / args.steps, 3), "sustained": sustained, "value_note": value_note,
            "end_to_end": {"tflops_per_gpu": round(value / world * wexec / 1e12, 2),
                           "frac_of_bf16_peak": round(value / world * wexec / 2.5e15, 4),
                           "w_train_gflop_per_clip": round(wtrain / 1e9, 2), "executed_gflop_per_clip": round(wexec / 1e9, 2)},
        }
        if timing:
            out["roofline"] = timing["roofline"]
            # HBM bytes per launch come from the committed PMC passes of THIS configuration (profiles/): configs[1] only
            base_cfg = args.arch == "vit" and args.frames == 8 and B == 32
            out["roofline"]["traffic"] = pmc_traffic(timing["roofline"]["kernel"]) if base_cfg else None
            if "runner_up" in out["roofline"]:
                out["roofline"]["runner_up"]["traffic"] = pmc_traffic(out["roofline"]["runner_up"]["kernel"]) if base_cfg else None
            if base_cfg:
                out["roofline"]["traffic_source"] = getattr(pmc_traffic, "note", None)
            if isolated:
                out["roofline"]["isolated"] = isolated
            out["kernels"] = timing["summary"]
        failed = []     # a failing checker leg is reported in the line AND turns the exit status red
        if not args.no_cpu_baseline and world == 1:      # (rank 0 at N = 1 only: the other ranks of a data-parallel run would sit in a barrier)
            try:
                out["cpu_baseline"] = cpu_baseline(args)
            except Exception as e:  # noqa
                out["cpu_baseline"] = {"error": repr(e)[:200]}
                failed.append("cpu_baseline")
        # north_star's tolerance, stated for THIS flavour in THIS line: the default single-GPU run (and --parity-probe) checks 2 clips of
        # the full-size model against the CPU oracle after the timed region (the oracle is the checker, never the path)
        # (world > 1: the probe runs on rank 0 below, after the process group is gone -- the other ranks must not sit in a collective
        #  for the half minute the CPU oracle takes)
        want_parity = (args.parity_probe or default_run or world > 1) and not args.no_parity_probe
    else:
        out, failed, want_parity = None, [], False
    if dp_path:
        dist.barrier()
        dist.destroy_process_group()
    status = 0
    if rank == 0:
        if want_parity:
            # the timed model's captured graphs and pools go NOW, with the device idle, not whenever the garbage collector gets to them in
            # the middle of the probe's own GPU work (that teardown aborted / hung the HIP runtime in the test suite)
            import gc
            torch.cuda.synchronize()
            if hasattr(vt.engine, "release_graphs"):
                vt.engine.release_graphs()
            last.clear()
            del model, vt, optimizer, reducer, frames, teacher, pred
            gc.collect()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            try:
                out["parity"] = parity_probe(args.arch, args.frames)
                # the default (fp16-operand) library is the one held to north_star's 1e-3: a headline that misses it is a failed run
                if OPERAND == "f16" and not out["parity"]["meets_1e-3_on_logits_and_loss"]:
                    failed.append("parity")
            except Exception as e:  # noqa
                out["parity"] = {"error": repr(e)[:200]}
                failed.append("parity")
        if default_run or args.all_sides:
            # other single-GPU lines, timed by the same script in child processes (their own model, graphs and memory), each with its
            # own 2-clip `parity` object.  Informational: `value` above is the headline metric; a failing side run is reported, never fatal.
            out["side"] = side_measurements(True)
        if failed:
            out["failed"] = failed
        print(json.dumps(out), flush=True)
        status = 3 if failed else 0
    return status


def parity_probe(arch="vit", frames=8):
    """north_star's contract (step logits and loss within 1e-3 of the reference's CPU path) checked in THIS process on the
    library flavour that was just timed: tests/e2e_checks builds the full-size model (12 blocks, 224^2, K = 9871), runs one
    training step on 2 clips (1 clip at 32 frames: the same number of tokens as 4) through the HIP path and through the CPU oracle
    (oracle/ = checker, pinned to the reference by tests/golden) and returns relative L2 errors.  MViTv2-S (configs[4]): the encoder's
    features and gradients on 2 clips of 16 x 224^2 under a fixed linear functional of the features (the loss head is the ViT wrapper's)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    if arch == "mvit":
        import mvit_checks as mc
        r = mc.bench_parity_two_clips(frames)
        r["north_star_tol"] = 1e-3
        r["meets_1e-3_on_logits_and_loss"] = bool(r["features_rel_err"] <= 1e-3 and r["loss_rel_err"] <= 1e-3)
        return r
    import e2e_checks as ec
    res = ec.check_bench_config_two_clips(frames)
    get = lambda key: next(e for l, e, _ in res if key in l)
    return {"logits_rel_err": float(f"{get('logits vs oracle'):.3e}"), "loss_rel_err": float(f"{get('loss vs oracle'):.3e}"),
            "worst_grad_rel_err": float(f"{get('all parameter gradients'):.3e}"), "north_star_tol": 1e-3,
            "meets_1e-3_on_logits_and_loss": bool(get("logits vs oracle") <= 1e-3 and get("loss vs oracle") <= 1e-3),
            "sample": f"{2 if frames <= 8 else 1} clip(s) of {frames} x 224^2, full-size model, one training step vs oracle/timesformer_oracle.py (fp32 CPU)"}


def dump_outputs(out_dir, model, loss, pred, video_emb, sample=1 << 21):
    """--dump-outputs: the last timed step's results as float32 .npy files -- the loss, the step logits [B, K], the unit-norm clip
    embeddings [B, 512], and the same `sample` positions (seeded, fixed for a given model) of every trainable parameter after the
    optimizer step and of its gradient, concatenated in named_parameters() order.  Any array over 4M elements is sampled the same way;
    the whole dump stays under 64 MB."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    params = [p for _, p in model.named_parameters() if p.requires_grad]
    flat = torch.cat([p.detach().reshape(-1).float() for p in params])
    grads = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().reshape(-1).float() for p in params])

    def pick(t, n):
        t = t.detach().reshape(-1).float() if t.numel() > n else t.detach().float()
        if t.numel() > n:
            idx = torch.randint(t.numel(), (n,), generator=torch.Generator().manual_seed(0)).sort()[0]
            t = t[idx.to(t.device)]
        return t.cpu().numpy().astype(np.float32)

    arrays = {"loss": loss.detach().float().reshape(1).cpu().numpy(), "logits": pick(pred, 1 << 22),
              "video_emb": pick(video_emb, 1 << 22), "params_sample": pick(flat, sample), "grads_sample": pick(grads, sample)}
    del flat, grads
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def side_measurements(all_sides=False):
    """The other single-GPU lines, each a child process of this same script under the driver's clock: configs[1] with bf16 operands
    (the type BASELINE's configs name; not held to 1e-3), configs[1] with the last block unpruned, and the reference's full pre-training
    step; with --all-sides also configs[3]
    and configs[4], whose per-kernel profiles are tracked under profiles/."""
    import subprocess
    res = []
    base = ["--full", "--no-cpu-baseline", "--no-side"]
    full = os.path.join(ROOT, "tools", "bench_full_step.py")
    lines = [
        ("configs[1] with bf16 operands (PVRL_OPERAND=bf16, libpvrl_hip.so): TimeSformer ViT-B 8x224^2, 32 clips/GPU",
         ["--steps", "20", "--warmup", "5", "--parity-probe"], {"PVRL_OPERAND": "bf16"}, None),
        ("configs[1] with the last block run over all 1,569 tokens of every clip, as the reference runs it (PVRL_PRUNE_LAST=0 "
         "PVRL_PRUNE_ATTN=0): what `value` would be without skipping the work whose results nothing reads (DESIGN section 3)",
         ["--steps", "20", "--warmup", "5"], {"PVRL_PRUNE_LAST": "0", "PVRL_PRUNE_ATTN": "0"}, None),
        ("the reference's FULL pre-training step (vit.py:283-352, train_net.py:152-181): 4 videos x 9 clips of 8x224^2, frozen "
         "12-layer CLIP-text teacher + order / diffusion transformer + top-5 KL + MSE + AdamW, head replayed from HIP graphs",
         ["--steps", "10", "--warmup", "6"], {}, full)]
    if all_sides:
        lines += [("configs[3]: TimeSformer ViT-B 32x224^2, 8 clips/GPU",
                   ["--steps", "10", "--warmup", "3", "--frames", "32", "--batch", "8", "--parity-probe"], {}, None),
                  ("configs[4]: MViTv2-S 16x224^2, 32 clips/GPU", ["--steps", "10", "--warmup", "3", "--arch", "mvit", "--parity-probe"], {}, None)]
    for name, extra, env, script in lines:
        cmd = [sys.executable, script] + extra if script else [sys.executable, os.path.abspath(__file__)] + base + extra
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=480, env=dict(os.environ, **env))
            line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
            d = json.loads(line)
            e = {"config": name, "metric": d["metric"], "value": d["value"], "unit": d["unit"], "dtype": d["dtype"],
                 "ms_per_step": d["ms_per_step"], "steps": d["steps"],
                 "frac_of_bf16_peak": d.get("end_to_end", {}).get("frac_of_bf16_peak")}
            if "roofline" in d:
                e["roofline"] = d["roofline"]
            if "parity" in d:
                e["parity"] = d["parity"]
            res.append(e)
        except Exception as e:  # noqa
            res.append({"config": name, "error": repr(e)[:160]})
    return res


def rccl_version(torch):
    try:
        v = torch.cuda.nccl.version()
        return ".".join(map(str, v)) if isinstance(v, (tuple, list)) else str(v)
    except Exception as e:  # noqa  (informational field only)
        return f"unknown ({type(e).__name__})"


def spawn_ranks(n):
    import socket
    import subprocess
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def csrc_sha16():
    """hash of the kernel sources a profile was taken from / the library was built from (tools/summarize_pmc.py stores it)"""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "procedurevrl_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def pmc_traffic(kernel):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes of this same command
    (profiles/rN_traffic.json: 2 x FETCH_SIZE + WRITE_SIZE, KiB units, gfx950 correction); None when absent OR when the profile was
    taken from other kernel sources than the ones this run uses (`_meta.csrc_sha16`): stale bytes are not reported.
    A weight-gradient launch = the (grouped) TN kernel + the partial-sum reduces it issues."""
    import re
    cands = sorted((f for f in os.listdir(os.path.join(ROOT, "profiles")) if re.fullmatch(r"r\d+_traffic\.json", f)),
                   key=lambda f: int(f[1:f.index("_")]), reverse=True)
    if not cands:
        return None
    t = json.load(open(os.path.join(ROOT, "profiles", cands[0])))
    meta = t.pop("_meta", {})
    if meta.get("csrc_sha16") != csrc_sha16():
        pmc_traffic.note = f"profiles/{cands[0]} was taken from other kernel sources (csrc sha {meta.get('csrc_sha16')}, now {csrc_sha16()}): re-profile"
        return None
    pmc_traffic.note = f"profiles/{cands[0]}"
    epi = {"op16": 0, "bf16": 0, "gelu": 1, "qgelu": 2, "resid_f32": 3, "f32": 4, "dgelu": 5, "dqgelu": 6}
    if kernel.startswith("gemm_tn"):
        cands = ([k for k in t if k.startswith("gemm_tn") and k.endswith("grouped_kernel")] if "grouped" in kernel else
                 [k for k in t if k.startswith("gemm_tn") and not k.endswith("grouped_kernel")])
        if not cands:
            return None
        want = max(cands, key=lambda k: t[k].get("launches", 0))
        b = t[want]["hbm_bytes_per_launch"]
        # a grouped launch is followed by ONE grouped reduce of its fp32 partials (tn_reduce_grouped_kernel); a lone
        # weight gradient by its own tn_reduce_kernel
        red = t.get("tn_reduce_grouped_kernel" if "grouped" in kernel else "tn_reduce_kernel")
        if red:
            b += red["hbm_bytes_per_launch"]
        return round(b, 0)
    e = epi.get(kernel[kernel.find("<") + 1:kernel.find(">")], -1)
    keys = [k for k in t if k.startswith(f"gemm_nt_kernel<{e},") or k.startswith(f"gemm_nt8_kernel<{e}>")]
    if not keys:
        return None
    main = max(keys, key=lambda k: t[k]["avg_us"])
    return round(t[main]["hbm_bytes_per_launch"], 0)


def cpu_baseline(args):
    """the CPU restatement of the reference's path (oracle/, pinned to the reference by golden vectors) timed on
    ALL physical cores of this host on BASELINE configs[0] -- 2 videos x 9 clips, the FULL pre-training step (text teacher + order
    transformer + KL + MSE + AdamW).  Bounded: the sample runs in a child process under a timeout; when it does not finish (eager
    PyTorch scales badly past a few dozen threads), the 4-clip contrastive-only step of earlier rounds on the same cores.
    The checker timed as a reported baseline: never the product, never the target."""
    import subprocess
    note = ""
    if args.arch == "vit" and args.frames == 8:
        code = ("import json, sys; sys.path.insert(0, %r); from oracle import timesformer_oracle as orc; "
                "print('CPUBASE ' + json.dumps(orc.timed_full_step(videos=2, frames=%d, classes=%d, budget_s=%.1f)))"
                % (ROOT, args.frames, args.classes, CPU_BASELINE_BUDGET_S))
        try:
            r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=CPU_BASELINE_BUDGET_S + 150)
            line = [l for l in r.stdout.splitlines() if l.startswith("CPUBASE ")]
            if line:
                return json.loads(line[-1][len("CPUBASE "):])
            note = f"; configs[0] full step failed (rc {r.returncode}), 4-clip contrastive step instead"
        except subprocess.TimeoutExpired:
            note = (f"; configs[0] (18 clips, full pre-training step) did not finish a warm-up and a timed step in "
                    f"{CPU_BASELINE_BUDGET_S + 150:.0f} s on these cores, 4-clip contrastive step instead")
    from oracle import timesformer_oracle as orc
    model, phys, logical = orc.host_cpu()
    r = orc.timed_train_step(clips=max(1, 32 // args.frames), frames=args.frames, classes=args.classes, threads=min(phys, logical), repeats=2)
    r["sample"] += f"; {r['cores']} threads (host: {phys} physical / {logical} logical cores, {model})" + note
    return r


if __name__ == "__main__":
    sys.exit(main() or 0)
