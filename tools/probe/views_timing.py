"""`pvrl_frames_u8_patchify_views` against `pvrl_frames_u8_patchify` on physically replicated frames at the EPIC-Kitchens test
shape: S = 2 decoded views of T = 32 frames, 256 x 456 -> 6 clips of 224 x 224 (3 crops per view).  Event-timed like
tools/bench_kernels.py (`timeit`), the two variants alternating over several rounds so that a drift of the clock hits both;
prints every round and the medians.  The outputs are compared bit for bit first.  Usage: python tools/probe/views_timing.py"""
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch  # noqa: E402

from procedurevrl_amd import ops  # noqa: E402
from procedurevrl_amd.config import get_cfg  # noqa: E402
from procedurevrl_amd.transform import DecodedClips, decoded_test_views  # noqa: E402

DEV = "cuda:0"


def timeit(fn, reps=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3   # us


def main():
    cfg = get_cfg()
    cfg.merge_from_list(["DATA.TEST_CROP_SIZE", "224", "TEST.NUM_SPATIAL_CROPS", "3"])
    S, T, H0, W0 = 2, 32, 256, 456
    frames = torch.randint(0, 256, (S, T, H0, W0, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8).to(DEV)
    views = decoded_test_views(cfg, frames)
    plain = DecodedClips(frames[views.src_host.long().to(DEV)], views.params_host, cfg.DATA.MEAN, cfg.DATA.STD, 224)
    out_v, out_p = ops.frames_u8_patchify(views), ops.frames_u8_patchify(plain)
    assert torch.equal(out_v, out_p)
    print(f"source bytes: shared {views.frames.numel() / 1e6:.1f} MB, replicated {plain.frames.numel() / 1e6:.1f} MB; "
          f"output {out_v.numel() * out_v.element_size() / 1e6:.1f} MB")
    tv, tp = [], []
    for r in range(7):
        tv.append(timeit(lambda: ops.frames_u8_patchify(views, out=out_v)))
        tp.append(timeit(lambda: ops.frames_u8_patchify(plain, out=out_p)))
        print(f"round {r}: views {tv[-1]:.1f} us, replicated {tp[-1]:.1f} us")
    mv, mp = statistics.median(tv), statistics.median(tp)
    print(f"median: views {mv:.1f} us (min {min(tv):.1f}, max {max(tv):.1f}), replicated {mp:.1f} us (min {min(tp):.1f}, max {max(tp):.1f}), "
          f"views / replicated = {mv / mp:.3f}")


if __name__ == "__main__":
    main()
