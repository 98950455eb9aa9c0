"""Micro-benchmark of individual kernels at the BASELINE config-2 shapes (32 clips): event-timed, L2-flushed between
reps by cycling through several operand sets.  Usage: python tools/bench_kernels.py [filter ...]"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from procedurevrl_amd import ops  # noqa: E402
from procedurevrl_amd._lib import lib  # noqa: E402
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "probe"))
import probe_lib as pl  # noqa: E402   (measured-and-rejected variants: tools/probe/libpvrl_probe.so)

DEV = "cuda:0"
BF = torch.bfloat16


def timeit(fn, reps=20, warm=3):
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
    L = lib()
    flt = sys.argv[1:]
    want = lambda n: not flt or any(f in n for f in flt)
    B, N, T, C = 32, 196, 8, 768
    R = B * N * T
    M = R + B
    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)
    rows = []

    sel = {"tile": 0, "gm": 0}     # 0 = the product library; otherwise the probe library's explicit selectors

    def gemm_case(name, M_, N_, K_, epi, **kw):
        if not want(name):
            return
        A = rnd(M_, K_).to(BF); W = (rnd(N_, K_) * 0.02).to(BF)
        bias = rnd(N_)
        args = dict(bias=bias)
        if epi == L.PVRL_EPI_RESID_F32:
            args["aux"] = rnd(M_, N_)
        if epi in (L.PVRL_EPI_DGELU,):
            args["aux"] = rnd(M_, N_).to(BF); args.pop("bias")
        if sel["tile"] or sel["gm"]:
            us = timeit(lambda: pl.gemm_nt(sel["tile"], A, W, epi, gm=sel["gm"], **args))
        else:
            us = timeit(lambda: ops.gemm_nt(A, W, epi, **args))
        rows.append((name, us, 2.0 * M_ * N_ * K_ / us / 1e6))

    for tile in (1, 2, 3):
        sel["tile"] = tile
        tg = {1: "128x128", 2: "256x128", 3: "256x256"}[tile]
        gemm_case(f"nt[{tg}] qkv   bf16  M x2304x768", M, 2304, 768, L.PVRL_EPI_BF16)
        gemm_case(f"nt[{tg}] proj  bf16  M x768x768", R, 768, 768, L.PVRL_EPI_BF16)
        gemm_case(f"nt[{tg}] fc    resid M x768x768", R, 768, 768, L.PVRL_EPI_RESID_F32)
        gemm_case(f"nt[{tg}] fc1   gelu  M x3072x768", M, 3072, 768, L.PVRL_EPI_GELU)
        gemm_case(f"nt[{tg}] fc2   resid M x768x3072", M, 768, 3072, L.PVRL_EPI_RESID_F32)
        gemm_case(f"nt[{tg}] dfc2  dgelu M x3072x768", M, 3072, 768, L.PVRL_EPI_DGELU)
        gemm_case(f"nt[{tg}] dfc1  bf16  M x768x3072", M, 768, 3072, L.PVRL_EPI_BF16)
        gemm_case(f"nt[{tg}] dqkv  bf16  M x768x2304", M, 768, 2304, L.PVRL_EPI_BF16)
    for rep in range(2):
        for tile, tg in ((3, "256 16 waves"), (13, "4 waves, register-staged, 32x32x16")):
            sel["tile"] = tile
            gemm_case(f"ab[{tg}] qkv   bf16  M x2304x768", M, 2304, 768, L.PVRL_EPI_BF16)
            gemm_case(f"ab[{tg}] fc1   gelu  M x3072x768", M, 3072, 768, L.PVRL_EPI_GELU)
            gemm_case(f"ab[{tg}] proj  bf16  M x768x768", R, 768, 768, L.PVRL_EPI_BF16)
            gemm_case(f"ab[{tg}] fc    resid M x768x768", R, 768, 768, L.PVRL_EPI_RESID_F32)
            gemm_case(f"ab[{tg}] fc2   resid M x768x3072", M, 768, 3072, L.PVRL_EPI_RESID_F32)
            gemm_case(f"ab[{tg}] dfc1  bf16  M x768x3072", M, 768, 3072, L.PVRL_EPI_BF16)
            gemm_case(f"ab[{tg}] dqkv  bf16  M x768x2304", M, 768, 2304, L.PVRL_EPI_BF16)
            gemm_case(f"ab[{tg}] dfc2  dgelu M x3072x768", M, 3072, 768, L.PVRL_EPI_DGELU)
    sel["tile"] = 0
    for rep in range(2):
        for gm in (1, 2, 3, 4):
            sel["gm"] = gm
            gemm_case(f"gm[{gm}] qkv   bf16  M x2304x768", M, 2304, 768, L.PVRL_EPI_BF16)
            gemm_case(f"gm[{gm}] dfc1  bf16  M x768x3072", M, 768, 3072, L.PVRL_EPI_BF16)
            gemm_case(f"gm[{gm}] fc1   gelu  M x3072x768", M, 3072, 768, L.PVRL_EPI_GELU)
            gemm_case(f"gm[{gm}] proj  bf16  M x768x768", R, 768, 768, L.PVRL_EPI_BF16)
    sel["gm"] = 0
    gemm_case("nt-auto qkv      bf16  M x2304x768", M, 2304, 768, L.PVRL_EPI_BF16)
    gemm_case("nt proj     bf16  M x768x768", R, 768, 768, L.PVRL_EPI_BF16)
    gemm_case("nt fc/projs resid M x768x768", R, 768, 768, L.PVRL_EPI_RESID_F32)
    gemm_case("nt fc1      gelu  M x3072x768", M, 3072, 768, L.PVRL_EPI_GELU)
    gemm_case("nt fc2      resid M x768x3072", M, 768, 3072, L.PVRL_EPI_RESID_F32)
    gemm_case("nt dfc2     dgelu M x3072x768", M, 3072, 768, L.PVRL_EPI_DGELU)
    gemm_case("nt dfc1     bf16  M x768x3072", M, 768, 3072, L.PVRL_EPI_BF16)
    gemm_case("nt dqkv     bf16  M x768x2304", M, 768, 2304, L.PVRL_EPI_BF16)

    tn_sel = {"tile": 0}

    def tn_case(name, M_, N_, K_, splits=None):
        if not want(name):
            return
        P = rnd(M_, N_).to(BF); Q = rnd(M_, K_).to(BF)
        dW = torch.zeros(N_, K_, device=DEV); db = torch.zeros(N_, device=DEV)
        if tn_sel["tile"]:
            if splits is None:
                splits = pl.tn_splits(tn_sel["tile"], M_, N_, K_)
            us = timeit(lambda: pl.gemm_tn(tn_sel["tile"], P, Q, dW, db, splits=splits))
        else:
            if splits is None:
                splits = ops.tn_splits(M_, N_, K_)
            us = timeit(lambda: ops.gemm_tn(P, Q, dW, db, splits=splits))
        name = name + f" s={splits}"
        rows.append((name, us, 2.0 * M_ * N_ * K_ / us / 1e6))

    for tile in (7, 8, 7, 8):
        tn_sel["tile"] = tile
        tg = {1: "128x128 tr-read", 0: "default", 6: "rt 16x16x32", 7: "rt 32x32x16", 8: "rt 8 waves"}[tile]
        tn_case(f"tn[{tg}] wqkv  2304x768", M, 2304, 768)
        tn_case(f"tn[{tg}] wproj 768x768", R, 768, 768)
        tn_case(f"tn[{tg}] wfc1  3072x768", M, 3072, 768)
        tn_case(f"tn[{tg}] wfc2  768x3072", M, 768, 3072)
    tn_sel["tile"] = 0

    if want("f32"):
        a = rnd(32, 512); lab = rnd(9871, 512); labt = lab.t().contiguous(); dyl = rnd(32, 9871)
        us = timeit(lambda: ops.gemm_nt_f32(a, lab, alpha=50.0)); rows.append(("f32 logits fwd 32x9871x512", us, 2.0 * 32 * 9871 * 512 / us / 1e6))
        us = timeit(lambda: ops.gemm_nt_f32(dyl, labt, alpha=50.0)); rows.append(("f32 logits bwd 32x512x9871", us, 2.0 * 32 * 9871 * 512 / us / 1e6))
        f = rnd(32, 768); wh = rnd(512, 768)
        us = timeit(lambda: ops.gemm_nt_f32(f, wh)); rows.append(("f32 head 32x512x768", us, 2.0 * 32 * 512 * 768 / us / 1e6))
    if want("attn"):
        H = 12
        qkv = rnd(M, 3 * C).to(BF)
        o = torch.empty(R + B * T, C, device=DEV, dtype=BF)
        lse = torch.empty(B * T, H, N + 1, device=DEV)
        f = lambda: ops.attn_fwd(qkv, B * T, N + 1, H, 0.125, mode=1, T=T, cls_base=R, o=o[:R], o_cls=o[R:], lse=lse)
        us = timeit(f)
        fl = 4.0 * B * T * H * (N + 1) ** 2 * 64
        rows.append(("attn spatial fwd", us, fl / us / 1e6))
        do = rnd(R + B * T, C).to(BF)
        dq = torch.empty(M + B * T, 3 * C, device=DEV, dtype=BF)
        fb = lambda: ops.attn_bwd(qkv, o[:R], o[R:], do[:R], do[R:], lse, B * T, N + 1, H, 0.125, mode=1, T=T, cls_base=R,
                                  dqkv=dq[:M], dqkv_cls=dq[M:])
        us = timeit(fb)
        rows.append(("attn spatial bwd (q + kv kernels)", us, 2.5 * fl / us / 1e6))
        qt = rnd(R, 3 * C).to(BF)
        us = timeit(lambda: ops.attn_t8_fwd(qt, B * N, H, 0.125))
        rows.append(("attn t8 fwd [GB/s]", us, (R * 4 * C * 2) / us / 1e3))
        dot = rnd(R, C).to(BF)
        us = timeit(lambda: ops.attn_t8_bwd(qt, dot, B * N, H, 0.125))
        rows.append(("attn t8 bwd [GB/s]", us, (R * 8 * C * 2) / us / 1e3))

    if want("ln"):
        x = rnd(M, C); gam = rnd(C); bet = rnd(C)
        us = timeit(lambda: ops.layernorm_fwd(x, gam, bet, 1e-6))
        rows.append(("ln fwd [GB/s]", us, M * C * 6 / us / 1e3))
        y, mean, rstd = ops.layernorm_fwd(x, gam, bet, 1e-6)
        dy = rnd(M, C).to(BF); dg = torch.zeros(C, device=DEV); db = torch.zeros(C, device=DEV); dx = rnd(M, C)
        us = timeit(lambda: ops.layernorm_bwd(dy, x, mean, rstd, gam, dg, db, dx_in=dx, dx_out=dx))
        rows.append(("ln bwd (+reduce) [GB/s]", us, M * C * 14 / us / 1e3))
        us = timeit(lambda: ops.cast_scale(x, None))
        rows.append(("cast_scale [GB/s]", us, M * C * 6 / us / 1e3))

    if want("randaug"):
        # RandAugment at the EPIC-Kitchens per-GPU shape (4 clips x 32 frames x 256 x 456), every frame with two applied ops
        # cycling through the 15 increasing transforms at magnitude 10, both signs and resample modes.  The rate counts one read
        # and one write of the clip per layer (the histogram pass and the gathers' neighbours come on top).
        from procedurevrl_amd import randaugment as ra
        Bc, Tc, Hc, Wc = 4, 32, 256, 456
        arg = {"Rotate": 30.0, "ShearX": 0.3, "ShearY": 0.3, "TranslateXRel": 0.45, "TranslateYRel": 0.45, "PosterizeIncreasing": 0,
               "SolarizeIncreasing": 0, "SolarizeAdd": 110, "ColorIncreasing": 1.9, "ContrastIncreasing": 1.9,
               "BrightnessIncreasing": 1.9, "SharpnessIncreasing": 1.9}

        def op(i):
            name = ra.RAND_INCREASING_TRANSFORMS[i % 15]
            a = arg.get(name)
            if name in ra.GEOMETRIC and (i // 15) % 2:
                a = -a
            elif name.endswith("Increasing") and isinstance(a, float) and (i // 15) % 2:
                a = 2.0 - a
            return ra.resolve_op(name, () if a is None else (a,), (ra.BILINEAR, ra.BICUBIC)[(i // 30) % 2], Wc, Hc)
        clips = [ra.ClipPlan(None, [[op(b * Tc + t), op(7 * (b * Tc + t) + 3)] for t in range(Tc)], (115, 115, 115), Wc, Hc)
                 for b in range(Bc)]
        plan = ra.RandAugPlan(clips)
        fr = torch.randint(0, 256, (Bc, Tc, Hc, Wc, 3), device=DEV, dtype=torch.uint8, generator=g)
        us = timeit(lambda: ops.rand_augment_u8(fr, plan))
        rows.append(("randaug u8 4x32x256x456, 2 layers [GB/s]", us, 4.0 * fr.numel() / us / 1e3))

    if want("attn_long"):
        # The streamed long-sequence attention (csrc/attn_long.hip) at joint space-time attention's shapes -- 32 clips x 12 heads x 1,569
        # tokens (8 x 224^2) and 4 x 12 x 6,273 (32 x 224^2) -- and at the divided scheme's TimeSformer-HR shape: 32 clips x 16 frames =
        # 512 sequences of 785 tokens (448^2), the 16 sequences of a clip sharing its cls row (mode 1, T = 16) -- in alternating rounds
        # with torch's scaled_dot_product_attention on the same values in the same process; the median round counts.  FLOPs: 4 S^2 64
        # per (sequence, head) forward; the backward's EXECUTED products: seven here (S and dP are formed in both backward kernels),
        # five assumed for the baseline.
        import statistics
        import torch.nn.functional as F
        OP = ops.OP16
        for Bl, Tl, Hl, Sl in ((32, 1, 12, 1569), (4, 1, 12, 6273), (32, 16, 12, 785)):
            nl, Nl = Bl * Tl, Sl - 1
            Rl = Bl * Nl * Tl
            qkv = rnd(Rl + Bl, 3 * Hl * 64).to(OP)
            do = rnd(Rl + nl, Hl * 64).to(OP)
            o = torch.empty(Rl + nl, Hl * 64, device=DEV, dtype=OP)
            dq = torch.empty(Rl + Bl + nl, 3 * Hl * 64, device=DEV, dtype=OP)      # (T = 1: the cls partial rows ARE the cls rows)
            dq_cls = dq[Rl:Rl + Bl] if Tl == 1 else dq[Rl + Bl:]
            kw = dict(mode=1, T=Tl, cls_base=Rl)
            ff = lambda: ops.attn_long_fwd(qkv, nl, Sl, Hl, 0.125, o=o[:Rl], o_cls=o[Rl:], **kw)
            lse = ff()[2]
            fb = lambda: ops.attn_long_bwd(qkv, o[:Rl], o[Rl:], do[:Rl], do[Rl:], lse, nl, Sl, Hl, 0.125, dqkv=dq[:Rl + Bl], dqkv_cls=dq_cls, **kw)
            # the same sequences as [nseq, H, S, 64] tensors: the clip's cls row first, then the patch rows (b, n, t) of frame t
            def seqs(x, cls):
                W = x.shape[1]
                pat = x[:Rl].view(Bl, Nl, Tl, W).permute(0, 2, 1, 3)
                return torch.cat([cls.view(Bl, Tl, 1, W), pat], 2).reshape(nl, Sl, W)
            seq = seqs(qkv, qkv[Rl:].view(Bl, 1, -1).expand(Bl, Tl, -1)).view(nl, Sl, 3, Hl, 64).permute(2, 0, 3, 1, 4)
            q, k, v = (t.contiguous().requires_grad_(True) for t in seq)
            dos = seqs(do, do[Rl:]).view(nl, Sl, Hl, 64).permute(0, 2, 1, 3).contiguous()
            sf = lambda: F.scaled_dot_product_attention(q, k, v, scale=0.125)
            os_ = sf()
            sb = lambda: torch.autograd.grad(os_, (q, k, v), dos, retain_graph=True)
            t = {n: [] for n in ("ff", "sf", "fb", "sb")}
            for _ in range(5):
                for n, fn in (("ff", ff), ("sf", sf), ("fb", fb), ("sb", sb)):
                    t[n].append(timeit(fn, reps=5, warm=1))
            med = {n: statistics.median(v) for n, v in t.items()}
            fl = 4.0 * nl * Hl * Sl * Sl * 64
            tag = f"{Bl}x{Hl}xS{Sl}" if Tl == 1 else f"{Bl}x{Tl}x{Hl}xS{Sl} T={Tl}"
            rows.append((f"attn_long fwd {tag}", med["ff"], fl / med["ff"] / 1e6))
            rows.append((f"torch sdpa fwd {tag}", med["sf"], fl / med["sf"] / 1e6))
            rows.append((f"attn_long bwd {tag} (7 products)", med["fb"], 3.5 * fl / med["fb"] / 1e6))
            rows.append((f"torch sdpa bwd {tag} (5 products)", med["sb"], 2.5 * fl / med["sb"] / 1e6))
            del q, k, v, os_, dos, seq

    for name, us, rate in rows:
        print(f"{name:42s} {us:9.1f} us   {rate:9.1f} {'TFLOP/s' if 'GB/s' not in name else 'GB/s'}")


if __name__ == "__main__":
    main()
