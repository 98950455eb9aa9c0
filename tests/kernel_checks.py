"""Per-kernel parity checks: HIP kernel (through the C ABI) vs a CPU fp32 restatement.

Each check returns a list of (label, error, tolerance) triples; `error` is the relative L2 error
||hip - ref|| / ||ref|| unless stated.  bf16 operands carry 2^-9 relative rounding, so kernels
that round operands / outputs to bf16 are held to 1e-2 (typically 2-4e-3 is observed); fp32
kernels to 1e-5.  Used by tests/test_kernels_gpu.py (pytest -m gpu) and tools/gpu_check.py.
"""
import math

import torch
import torch.nn.functional as F

from procedurevrl_amd._lib import OPERAND

BF = torch.bfloat16 if OPERAND == "bf16" else torch.float16     # the library flavour's 16-bit operand type
# a kernel that rounds its output to the operand type sits at ~1.7e-3 (bf16) / 2.1e-4 (fp16) against fp32 math on the
# rounded inputs; backward kernels chain two or three such roundings
TOL_BF16 = 1e-2 if OPERAND == "bf16" else 1.5e-3
TOL_F32 = 2e-5


def rel(a, b):
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    d = (a - b).norm().item()
    n = b.norm().item()
    if not math.isfinite(d):
        return float("inf")
    return d / max(n, 1e-30)


def bf(x):
    """round to bf16 and back (what the kernels see)"""
    return x.to(BF).float()


def dev():
    return torch.device("cuda:0")


def check_gemm_nt():
    from procedurevrl_amd import ops
    from procedurevrl_amd._lib import lib
    L = lib()
    out = []
    g = torch.Generator().manual_seed(1)
    # the last three: the 128 x 384 / 128 x 320 tiles of MViTv2-S's N = 384 / 1152 / 640 layers (M >= 4096), ragged last tile
    # (M <= 192 with K % 256 == 0 -- (130, 768, 3072) and the three after it, the order / diffusion stack's shapes -- run the few-row kernel
    # of csrc/gemm_nt_skinny.h: ragged last 16-row tile, one to three 48-row passes)
    for (M, N, K) in [(300, 128, 64), (1000, 768, 768), (257, 2304, 768), (130, 768, 3072), (36, 512, 2048), (144, 1536, 512),
                      (37, 2048, 512), (100100, 384, 128), (4230, 768, 128), (4500, 640, 256)]:
        A = torch.randn(M, K, generator=g)
        W = torch.randn(N, K, generator=g) * 0.05
        bias = torch.randn(N, generator=g)
        rs = torch.rand(M, generator=g) + 0.5
        resid = torch.randn(M, N, generator=g)
        Ab, Wb = bf(A), bf(W)
        ref = Ab @ Wb.t()
        Ad, Wd = A.to(dev(), BF), W.to(dev(), BF)
        bd, rsd = bias.to(dev()), rs.to(dev())
        o = ops.gemm_nt(Ad, Wd, L.PVRL_EPI_BF16, bias=bd, rowscale=rsd)
        out.append((f"gemm_nt bf16 {M}x{N}x{K}", rel(o, rs[:, None] * (ref + bias)), TOL_BF16))
        o = ops.gemm_nt(Ad, Wd, L.PVRL_EPI_F32, bias=bd)
        out.append((f"gemm_nt f32 {M}x{N}x{K}", rel(o, ref + bias), 1e-4))
        o = ops.gemm_nt(Ad, Wd, L.PVRL_EPI_RESID_F32, bias=bd, rowscale=rsd, aux=resid.to(dev()))
        out.append((f"gemm_nt resid {M}x{N}x{K}", rel(o, resid + rs[:, None] * (ref + bias)), 1e-4))
        b2 = torch.randn(N, generator=g)
        o = ops.gemm_nt(Ad, Wd, L.PVRL_EPI_RESID_F32, bias=bd, rowscale=rsd, aux=resid.to(dev()), bias2=b2.to(dev()))
        out.append((f"gemm_nt resid + unscaled bias2 {M}x{N}x{K}", rel(o, resid + rs[:, None] * (ref + bias) + b2), 1e-4))
        rm = 7
        o = ops.gemm_nt(Ad, Wd, L.PVRL_EPI_RESID_F32, bias=bd, aux=resid[:rm].contiguous().to(dev()), aux_rowmod=rm)
        out.append((f"gemm_nt resid-mod {M}x{N}x{K}", rel(o, resid[torch.arange(M) % rm] + ref + bias), 1e-4))
        u, gl = ops.gemm_nt(Ad, Wd, L.PVRL_EPI_GELU, bias=bd)
        out.append((f"gemm_nt gelu(u) {M}x{N}x{K}", rel(u, ref + bias), TOL_BF16))
        out.append((f"gemm_nt gelu(g) {M}x{N}x{K}", rel(gl, F.gelu(ref + bias)), TOL_BF16))
        u2, g2 = ops.gemm_nt(Ad, Wd, L.PVRL_EPI_QGELU, bias=bd)
        z = ref + bias
        out.append((f"gemm_nt qgelu {M}x{N}x{K}", rel(g2, z * torch.sigmoid(1.702 * z)), TOL_BF16))
        upre = torch.randn(M, N, generator=g)
        ub = bf(upre)
        o = ops.gemm_nt(Ad, Wd, L.PVRL_EPI_DGELU, aux=upre.to(dev(), BF))
        ur = ub.clone().requires_grad_(True)
        F.gelu(ur).sum().backward()
        out.append((f"gemm_nt dgelu {M}x{N}x{K}", rel(o, ref * ur.grad), TOL_BF16))
        o = ops.gemm_nt(Ad, Wd, L.PVRL_EPI_DQGELU, aux=upre.to(dev(), BF))
        ur = ub.clone().requires_grad_(True)
        (ur * torch.sigmoid(1.702 * ur)).sum().backward()
        out.append((f"gemm_nt dqgelu {M}x{N}x{K}", rel(o, ref * ur.grad), TOL_BF16))
    # large-M path: 256x256 tiles, ragged last M-tile (50208 = 196 * 256 + 32), row-modulo residual table
    M, N, K = 50208, 768, 128
    A = torch.randn(M, K, generator=g); W = torch.randn(N, K, generator=g) * 0.1
    bias = torch.randn(N, generator=g); rs = torch.rand(M, generator=g) + 0.5
    E = torch.randn(1568, N, generator=g)
    ref = bf(A) @ bf(W).t()
    Ad, Wd = A.to(dev(), BF), W.to(dev(), BF)
    o = ops.gemm_nt(Ad, Wd, L.PVRL_EPI_RESID_F32, bias=bias.to(dev()), rowscale=rs.to(dev()), aux=E.to(dev()), aux_rowmod=1568)
    out.append(("gemm_nt large-M resid-mod 50208x768", rel(o, E[torch.arange(M) % 1568] + rs[:, None] * (ref + bias)), 1e-4))
    u, gl = ops.gemm_nt(Ad, Wd, L.PVRL_EPI_GELU, bias=bias.to(dev()))
    out.append(("gemm_nt large-M gelu 50208x768", rel(gl, F.gelu(ref + bias)), TOL_BF16))
    upre = torch.randn(M, N, generator=g)
    o = ops.gemm_nt(Ad, Wd, L.PVRL_EPI_DGELU, rowscale=rs.to(dev()), aux=upre.to(dev(), BF))
    ur = bf(upre).clone().requires_grad_(True)
    F.gelu(ur).sum().backward()
    out.append(("gemm_nt large-M dgelu 50208x768", rel(o, rs[:, None] * ref * ur.grad), TOL_BF16))
    # strided A (a column slice of a wider buffer) and row-sliced output
    M, N, K = 200, 128, 128
    big = torch.randn(M, 3 * K, generator=g)
    W = torch.randn(N, K, generator=g) * 0.1
    Ad = big.to(dev(), BF)[:, K:2 * K]
    o = ops.gemm_nt(Ad, W.to(dev(), BF), L.PVRL_EPI_F32)
    out.append(("gemm_nt strided-A", rel(o, bf(big[:, K:2 * K]) @ bf(W).t()), 1e-4))
    return out


def check_gemm_nt_batched():
    """pvrl_gemm_nt_batched_bf16: several small NT problems in one launch (the 768^3 products of the fused temporal branch) vs fp32 math
    on the rounded operands; differing shapes, ragged M, row scale, residual, more problems than one launch carries."""
    from procedurevrl_amd import ops
    from procedurevrl_amd._lib import lib
    L = lib()
    g = torch.Generator().manual_seed(21)
    out = []
    shapes = [(768, 768, 768)] * 13 + [(300, 256, 128), (130, 128, 64), (1000, 384, 256)]
    probs, refs = [], []
    for (M, N, K) in shapes:
        A = torch.randn(M, K, generator=g); W = torch.randn(N, K, generator=g) * 0.05
        rs = torch.rand(M, generator=g) + 0.5
        aux = torch.randn(M, N, generator=g)
        probs.append(dict(A=A.to(dev(), BF), W=W.to(dev(), BF), rowscale=rs.to(dev()), aux=aux.to(dev())))
        refs.append((bf(A) @ bf(W).t(), rs, aux))
    o = ops.gemm_nt_batched([dict(A=p["A"], W=p["W"]) for p in probs], L.PVRL_EPI_F32)
    out.append(("gemm_nt_batched f32 (16 problems, worst)", max(rel(x, r[0]) for x, r in zip(o, refs)), 1e-5))
    o = ops.gemm_nt_batched(probs, L.PVRL_EPI_RESID_F32)
    out.append(("gemm_nt_batched residual + row scale (worst)", max(rel(x, r[2] + r[1][:, None] * r[0]) for x, r in zip(o, refs)), 1e-5))
    o = ops.gemm_nt_batched([dict(A=p["A"], W=p["W"]) for p in probs[:3]], L.PVRL_EPI_BF16)
    out.append(("gemm_nt_batched 16-bit out (worst)", max(rel(x, r[0]) for x, r in zip(o, refs)), TOL_BF16))
    one = ops.gemm_nt(probs[0]["A"], probs[0]["W"], L.PVRL_EPI_F32)
    out.append(("gemm_nt_batched == gemm_nt bit for bit", float((one != ops.gemm_nt_batched([dict(A=probs[0]["A"], W=probs[0]["W"])], L.PVRL_EPI_F32)[0]).sum()), 0.0))
    return out


def check_grad_scale_begin():
    """pvrl_grad_scale_begin (grads.GradStore.begin_scaled in one launch) vs the torch formula it replaces: S = the power of two that brings
    max|g| to the target, g * S exactly, 1 / S in every slot; zeros, inf and nan leave S a finite power of two."""
    from procedurevrl_amd import ops
    from procedurevrl_amd._lib import lib
    g0 = torch.Generator().manual_seed(4)
    out = []
    for name, t in (("normal", torch.randn(32, 768, generator=g0) * 3e-6), ("large", torch.randn(5, 777, generator=g0) * 1e9),
                    ("zeros", torch.zeros(4, 100)), ("inf", torch.tensor([1.0, float("inf"), -2.0])),
                    ("nan", torch.tensor([1e-3, float("nan"), 5e-4]))):
        t = t.contiguous()
        amax = torch.nan_to_num(t.abs().max(), nan=1.0, posinf=3e38).clamp(1e-30, 3e38)
        S = torch.exp2(torch.floor(torch.log2(256.0 / amax)).clamp(-100.0, 100.0))
        if name == "nan":       # the kernel treats nan like inf (S from 3e38): torch's nan_to_num(nan=1) differs only in this don't-care case
            S = torch.exp2(torch.floor(torch.log2(torch.tensor(256.0 / 3e38))).clamp(-100.0, 100.0))
        d = t.to(dev())
        o = torch.empty_like(d); sc = torch.empty(1, device=dev()); inv = torch.empty(64, device=dev())
        lib().call("pvrl_grad_scale_begin", ops._ptr(d), d.numel(), 256.0, ops._ptr(o), ops._ptr(sc), ops._ptr(inv), 64, ops._stream())
        out.append((f"grad_scale_begin S ({name})", abs(float(sc) - float(S)) / float(S), 0.0))
        out.append((f"grad_scale_begin 1/S in every slot ({name})", float((inv.cpu() != 1.0 / S).sum()), 0.0))
        ref = t * S
        ok = torch.equal(torch.nan_to_num(o.cpu(), nan=7.0), torch.nan_to_num(ref, nan=7.0))
        out.append((f"grad_scale_begin g * S exact ({name})", 0.0 if ok else 1.0, 0.0))
    return out


def check_small_batched():
    """pvrl_gemv_rows_batched_f32 / pvrl_rank1_add_batched_f32: many problems per launch, bit-equal to the one-problem entry points"""
    from procedurevrl_amd import ops
    g = torch.Generator().manual_seed(31)
    n, R, C = 19, 768, 768
    out = []
    for wdt in (torch.float32, BF):
        Ws = [(torch.randn(R, C, generator=g) * 0.05).to(dev(), wdt) for _ in range(n)]
        xs = [torch.randn(C, generator=g).to(dev()) for _ in range(n)]
        y0 = [torch.randn(R, generator=g).to(dev()) for _ in range(n)]
        betas = [float(i % 2) for i in range(n)]
        half = torch.full((1,), 0.5, device=dev())
        ya = [y.clone() for y in y0]
        yb = [y.clone() for y in y0]
        ops.gemv_rows_batched(Ws, xs, ya, betas, gscale=half)
        for W, x, y, b in zip(Ws, xs, yb, betas):
            ops.gemv_rows(W, x, out=y, beta=b, gscale=half)
        out.append((f"gemv_rows_batched == gemv_rows ({wdt})", float(sum((a != b).sum() for a, b in zip(ya, yb))), 0.0))
    outs = [torch.randn(R, C, generator=g).to(dev()) for _ in range(n)]
    As = [torch.randn(R, generator=g).to(dev()) for _ in range(n)]
    Bs = [torch.randn(C, generator=g).to(dev()) for _ in range(n)]
    oa = [o.clone() for o in outs]
    ob = [o.clone() for o in outs]
    ops.rank1_add_batched(oa, As, Bs)
    for o, a, b in zip(ob, As, Bs):
        ops.rank1_add(o, a, b)
    out.append(("rank1_add_batched == rank1_add", float(sum((a != b).sum() for a, b in zip(oa, ob))), 0.0))
    out.append(("rank1_add_batched vs torch", rel(oa[3], outs[3].cpu() + torch.outer(As[3].cpu(), Bs[3].cpu())), TOL_F32))
    return out


def check_gemm_f32_small():
    from procedurevrl_amd import ops
    g = torch.Generator().manual_seed(2)
    out = []
    for (M, N, K) in [(32, 9871, 512), (104, 1000, 512), (5, 512, 768), (512, 40, 32), (32, 512, 9871), (26, 768, 3000)]:
        A = torch.randn(M, K, generator=g)
        B = torch.randn(N, K, generator=g)
        bias = torch.randn(N, generator=g)
        o = ops.gemm_nt_f32(A.to(dev()), B.to(dev()), bias.to(dev()), alpha=50.0)
        out.append((f"gemm_f32_small {M}x{N}x{K}", rel(o, 50.0 * (A @ B.t()) + bias), TOL_F32))
    return out


def check_cls_linear():
    """pvrl_cls_linear_f32: the cls rows' fp32 projection / MLP (vit.py:147-157) vs fp64 math on the same fp32 inputs."""
    from procedurevrl_amd import ops
    g = torch.Generator().manual_seed(12)
    out = []
    for (M, N, K) in [(32, 768, 768), (36, 3072, 768), (32, 768, 3072), (2, 768, 768), (50, 3072, 768), (7, 768, 3072), (3, 512, 512),
                      (5, 256, 128), (100, 256, 2048)]:      # one to three 16-row tiles, several row passes; K >= 2048 with few columns: four K slices
        X = torch.randn(M, K, generator=g)
        W = torch.randn(N, K, generator=g) * 0.05
        bias = torch.randn(N, generator=g)
        rs = torch.rand(M, generator=g) + 0.5
        bs = torch.rand(M, generator=g) + 0.5
        aux = torch.randn(M, N, generator=g)
        Xd, Wd, bd = X.to(dev()), W.to(dev()), bias.to(dev())
        acc = X.double() @ W.double().t()
        o = ops.cls_linear(Xd, Wd, bd)
        out.append((f"cls_linear {M}x{N}x{K}", rel(o, acc + bias), TOL_F32))
        o = ops.cls_linear(Xd, Wd, bd, rowscale=rs.to(dev()), biasscale=bs.to(dev()), aux=aux.to(dev()))
        out.append((f"cls_linear residual {M}x{N}x{K}", rel(o, aux + rs[:, None] * acc + bs[:, None] * bias), TOL_F32))
        o = ops.cls_linear(Xd, Wd, bd, gelu=True)
        out.append((f"cls_linear gelu {M}x{N}x{K}", rel(o, F.gelu((acc + bias).float())), TOL_F32))
        # a strided view as the engine passes it (rows of a larger buffer)
        big = torch.zeros(M + 5, N + 64, device=dev())
        ops.cls_linear(Xd, Wd, None, out=big[5:, :N])
        out.append((f"cls_linear strided out {M}x{N}x{K}", rel(big[5:, :N], acc), TOL_F32))
        again = ops.cls_linear(Xd, Wd, bd)          # (K slices are summed by a second kernel in slice order)
        out.append((f"cls_linear repeatable {M}x{N}x{K}", float((again != ops.cls_linear(Xd, Wd, bd)).sum()), 0.0))
    return out


def check_gemm_tn():
    from procedurevrl_amd import ops
    g = torch.Generator().manual_seed(3)
    out = []
    for (M, N, K, splits) in [(96, 128, 128, 8), (1000, 768, 768, 16), (5000, 256, 384, None), (333, 128, 256, 24),
                              (1569, 384, 1152, None), (700, 640, 128, None), (2000, 1152, 384, 5)]:   # half tiles (N or K = 128 mod 256)
        P = torch.randn(M, N, generator=g)
        Q = torch.randn(M, K, generator=g)
        ref = bf(P).t() @ bf(Q)
        dW = torch.zeros(N, K, device=dev())
        db = torch.zeros(N, device=dev())
        ops.gemm_tn(P.to(dev(), BF), Q.to(dev(), BF), dW, db, beta=0.0, splits=splits)
        out.append((f"gemm_tn dW {M}x{N}x{K} s={splits}", rel(dW, ref), 1e-4))
        out.append((f"gemm_tn dbias {M}x{N}x{K}", rel(db, bf(P).sum(0)), 1e-4))
        ops.gemm_tn(P.to(dev(), BF), Q.to(dev(), BF), dW, db, beta=1.0, splits=splits)
        out.append((f"gemm_tn accumulate {M}x{N}x{K}", rel(dW, 2 * ref), 1e-4))
    return out


def check_gemm_tn_rows_behind_the_end():
    """the operands are the first M rows of larger buffers whose following rows hold large values: a staging path that reads past
    the last slice's end (M not a multiple of the 64-row stage) shows as a gross error.  Whole-256 shapes (LDS-DMA kernel) and a
    half-tile shape (register-transposed kernel), single and grouped launches."""
    from procedurevrl_amd import ops
    g = torch.Generator().manual_seed(35)
    out = []
    probs, refs = [], []
    for (M, N, K, splits) in [(1569, 768, 256, None), (1000, 256, 512, 3), (333, 256, 256, 1), (1569, 384, 256, None)]:
        Pb = torch.full((M + 300, N), 1000.0); Qb = torch.full((M + 300, K), -1000.0)
        Pb[:M] = torch.randn(M, N, generator=g); Qb[:M] = torch.randn(M, K, generator=g)
        Pd, Qd = Pb.to(dev(), BF), Qb.to(dev(), BF)
        ref = bf(Pb[:M]).t() @ bf(Qb[:M])
        dW = torch.zeros(N, K, device=dev()); db = torch.zeros(N, device=dev())
        ops.gemm_tn(Pd[:M], Qd[:M], dW, db, beta=0.0, splits=splits)
        out.append((f"gemm_tn rows behind the end dW {M}x{N}x{K} s={splits}", rel(dW, ref), 1e-4))
        out.append((f"gemm_tn rows behind the end dbias {M}x{N}x{K}", rel(db, bf(Pb[:M]).sum(0)), 1e-4))
        if N % 256 == 0 and K % 256 == 0:
            probs.append((Pd[:M], Qd[:M], torch.zeros(N, K, device=dev()), torch.zeros(N, device=dev()), 0.0))
            refs.append((ref, bf(Pb[:M]).sum(0)))
    ops.gemm_tn_grouped(probs)
    for (_, _, dW, db, _), (rw, rb) in zip(probs, refs):
        out.append((f"gemm_tn_grouped rows behind the end dW {tuple(dW.shape)}", rel(dW, rw), 1e-4))
        out.append((f"gemm_tn_grouped rows behind the end dbias {tuple(dW.shape)}", rel(db, rb), 1e-4))
    return out


def check_gemm_tn_repeatable():
    """The weight-gradient kernel for whole-256 shapes keeps its LDS-DMA copies in flight across barriers with counted waits: launched
    repeatedly next to an uneven load on a second stream, every result must be BIT-identical to the first (a wait that is one short or a
    slot re-staged too early shows as a run-to-run difference), and identical to the register-transposed kernel's order of summation
    (checked against fp32 matmul within rounding)."""
    from procedurevrl_amd import ops
    g = torch.Generator().manual_seed(36)
    out = []
    burn = torch.randn(4096, 4096, device=dev())
    side = torch.cuda.Stream()
    shapes = [(6273, 768, 768), (6273, 2304, 768), (6272, 768, 3072), (6273, 3072, 768)]       # a block's gradients at 4 clips (ragged last stage)
    P = [(torch.randn(m, N, generator=g) * 0.05).to(dev(), BF) for m, N, K in shapes]
    Q = [torch.randn(m, K, generator=g).to(dev(), BF) for m, N, K in shapes]

    def run():
        dW = [torch.empty(N, K, device=dev()) for m, N, K in shapes]
        db = [torch.empty(N, device=dev()) for m, N, K in shapes]
        ops.gemm_tn_grouped([(P[i], Q[i], dW[i], db[i], 0.0) for i in range(len(shapes))])
        return dW + db
    ref = [x.clone() for x in run()]
    diff = 0
    for it in range(8):
        if it % 3 != 0:
            with torch.cuda.stream(side):
                burn @ burn
        diff += sum(int(not torch.equal(a.view(torch.int32), b.view(torch.int32))) for a, b in zip(ref, run()))
    torch.cuda.synchronize()
    out.append(("gemm_tn_grouped (LDS-DMA kernel): results that differ from the first launch (8 launches x 8 tensors)", float(diff), 0.0))
    out.append(("gemm_tn_grouped (LDS-DMA kernel) dW vs fp32 matmul", rel(ref[1], P[1].float().cpu().t() @ Q[1].float().cpu()), 1e-4))
    return out


def check_gemm_tn_into():
    """zero-padded operands reduced straight into an un-padded, odd-width destination (pvrl_gemm_tn_into_bf16): the MViT
    engine's weight gradients (96 -> 128, 441 -> 512 columns); separate betas for weight and bias"""
    from procedurevrl_amd import ops
    g = torch.Generator().manual_seed(31)
    out = []
    for (M, Nv, Kv, Np, Kp, bw, bb) in [(700, 96, 441, 128, 512, 0.0, 0.0), (333, 288, 96, 384, 128, 1.0, 1.0),
                                        (5000, 192, 192, 256, 256, 0.0, 1.0), (64, 768, 384, 768, 384, 1.0, 0.0)]:
        P = torch.zeros(M, Np); P[:, :Nv] = torch.randn(M, Nv, generator=g)
        Q = torch.zeros(M, Kp); Q[:, :Kv] = torch.randn(M, Kv, generator=g)
        w0 = torch.randn(Nv, Kv, generator=g); b0 = torch.randn(Nv, generator=g)
        ref_w = bw * w0 + (bf(P).t() @ bf(Q))[:Nv, :Kv]
        ref_b = bb * b0 + bf(P).sum(0)[:Nv]
        dW = w0.to(dev()).clone(); db = b0.to(dev()).clone()
        ops.gemm_tn_into(P.to(dev(), BF), Q.to(dev(), BF), dW, Nv, Kv, dbias=db, beta=bw, beta_bias=bb)
        out.append((f"gemm_tn_into dW {M}x{Nv}({Np})x{Kv}({Kp}) beta={bw}", rel(dW, ref_w), 1e-4))
        out.append((f"gemm_tn_into dbias {M}x{Nv} beta={bb}", rel(db, ref_b), 1e-4))
    return out


def check_gemm_tn_grouped():
    """several weight gradients in one launch (pvrl_gemm_tn_grouped_bf16): ragged and differing M, bias / no bias,
    accumulate, bit-identical across repeats, and the per-problem fallback for shapes the grouped kernel refuses"""
    from procedurevrl_amd import ops
    g = torch.Generator().manual_seed(33)
    out = []
    shapes = [(1569, 768, 256, True, 0.0), (1569, 256, 768, True, 1.0), (1568, 256, 256, False, 0.0),
              (1569, 512, 256, True, 0.0), (1000, 256, 512, True, 1.0)]
    def make():
        probs, refs = [], []
        gg = torch.Generator().manual_seed(34)
        for (M, N, K, hb, beta) in shapes:
            P = torch.randn(M, N, generator=gg); Q = torch.randn(M, K, generator=gg)
            w0 = torch.randn(N, K, generator=gg); b0 = torch.randn(N, generator=gg)
            dW = w0.to(dev()).clone(); db = b0.to(dev()).clone() if hb else None
            probs.append((P.to(dev(), BF), Q.to(dev(), BF), dW, db, beta))
            refs.append((beta * w0 + bf(P).t() @ bf(Q), beta * b0 + bf(P).sum(0)))
        return probs, refs
    probs, refs = make()
    ops.gemm_tn_grouped(probs)
    for (M, N, K, hb, beta), (_, _, dW, db, _), (rw, rb) in zip(shapes, probs, refs):
        out.append((f"gemm_tn_grouped dW {M}x{N}x{K} beta={beta}", rel(dW, rw), 1e-4))
        if hb:
            out.append((f"gemm_tn_grouped dbias {M}x{N}x{K}", rel(db, rb), 1e-4))
    probs2, _ = make()
    ops.gemm_tn_grouped(probs2)
    same = all(torch.equal(a[2], b[2]) and (a[3] is None or torch.equal(a[3], b[3])) for a, b in zip(probs, probs2))
    out.append(("gemm_tn_grouped bit-identical across repeats", 0.0 if same else 1.0, 0.5))
    # a 128-multiple shape in the list -> one plain launch per problem, same results
    P = torch.randn(500, 128, generator=g); Q = torch.randn(500, 384, generator=g)
    dW = torch.zeros(128, 384, device=dev())
    probs3, refs3 = make()
    ops.gemm_tn_grouped(probs3[:2] + [(P.to(dev(), BF), Q.to(dev(), BF), dW, None, 0.0)])
    out.append(("gemm_tn_grouped fallback dW", rel(dW, bf(P).t() @ bf(Q)), 1e-4))
    out.append(("gemm_tn_grouped fallback dW[0]", rel(probs3[0][2], refs3[0][0]), 1e-4))
    return out


def check_gemm_tn_grouped_block_size():
    """the benchmark's dominant launch at ITS size: the seven weight gradients of one TimeSformer block at 32 clips
    (M = 50,208 / 50,176 rows; the (N, K) of tests/test_cabi.py) in one grouped launch vs fp32 CPU matmuls."""
    from procedurevrl_amd import ops
    gg = torch.Generator().manual_seed(77)
    R, M, BT = 50176, 50208, 256
    shapes = [(M, 768, 3072, "fc2"), (M, 3072, 768, "fc1"), (R + BT, 768, 768, "attn.proj"), (M, 2304, 768, "attn.qkv"),
              (R, 768, 768, "fused temporal map"), (R, 2304, 768, "temporal_attn.qkv"), (R, 768, 768, "patch_embed")]
    probs, refs = [], []
    for (m, N, K, _) in shapes:
        P = (torch.randn(m, N, generator=gg) * 0.05).to(BF); Q = torch.randn(m, K, generator=gg).to(BF)
        refs.append((P.float().t() @ Q.float(), P.float().sum(0)))
        probs.append((P.to(dev()), Q.to(dev()), torch.empty(N, K, device=dev()), torch.empty(N, device=dev()), 0.0))
    ops.gemm_tn_grouped(probs)
    out = []
    for (m, N, K, name), (_, _, dW, db, _), (rw, rb) in zip(shapes, probs, refs):
        out.append((f"grouped dW {name} {m}x{N}x{K}", rel(dW, rw), 1e-4))
        out.append((f"grouped dbias {name}", rel(db, rb), 1e-4))
    return out


def check_cast_weights_multi():
    """pvrl_cast_weights_multi_bf16: many fp32 weight matrices -> bf16 copy + transposed copy in one launch (ragged
    shapes, with and without the transposed copy, more than one launch worth of items)"""
    from procedurevrl_amd import ops
    g = torch.Generator().manual_seed(41)
    shapes = [(768, 768), (2304, 768), (768, 588), (33, 65), (512, 2048), (1, 7)] * 17 + [(100, 31)]
    items, refs = [], []
    for k, (R, C) in enumerate(shapes):
        w = torch.randn(R, C, generator=g)
        out = torch.zeros(R, C, device=dev(), dtype=BF)
        out_t = torch.zeros(C, R, device=dev(), dtype=BF) if k % 3 else None
        items.append((w.to(dev()), out, out_t))
        refs.append(w.to(BF))
    ops.cast_weights_multi(items)
    bad = 0
    for (w, out, out_t), r in zip(items, refs):
        bad += int(not torch.equal(out.cpu(), r))
        if out_t is not None:
            bad += int(not torch.equal(out_t.cpu(), r.t().contiguous()))
    res = [(f"cast_weights_multi: {len(shapes)} matrices, mismatching copies", float(bad), 0.0)]
    # every side a multiple of 64 (the encoder's Linears): the 64 x 64-tile kernel, 16-byte loads / 8-byte stores
    shapes = [(768, 768), (2304, 768), (64, 64), (768, 3072), (3072, 768), (128, 192)] * 9
    items, refs = [], []
    for k, (R, C) in enumerate(shapes):
        w = torch.randn(R, C, generator=g)
        out = torch.zeros(R, C, device=dev(), dtype=BF)
        out_t = torch.zeros(C, R, device=dev(), dtype=BF) if k % 4 else None
        items.append((w.to(dev()), out, out_t))
        refs.append(w.to(BF))
    ops.cast_weights_multi(items)
    bad = 0
    for (w, out, out_t), r in zip(items, refs):
        bad += int(not torch.equal(out.cpu(), r))
        if out_t is not None:
            bad += int(not torch.equal(out_t.cpu(), r.t().contiguous()))
    res.append((f"cast_weights_multi (64-tile kernel): {len(shapes)} matrices, mismatching copies", float(bad), 0.0))
    return res


def check_gemv_rows():
    """pvrl_gemv_rows_f32: y = beta*y + W x for fp32 and bf16 matrices (ragged sizes, leading dimension > C)"""
    from procedurevrl_amd import ops
    g = torch.Generator().manual_seed(43)
    out = []
    for (R, C) in [(768, 768), (5, 70), (513, 129)]:
        Wf = torch.randn(R, C + 8, generator=g)[:, :C]
        x = torch.randn(C, generator=g)
        y0 = torch.randn(R, generator=g)
        y = ops.gemv_rows(Wf.to(dev()), x.to(dev()))
        out.append((f"gemv_rows fp32 {R}x{C}", rel(y, Wf @ x), 1e-5))
        yb = y0.to(dev()).clone()
        ops.gemv_rows(Wf.to(dev(), BF), x.to(dev()), out=yb, beta=1.0)
        out.append((f"gemv_rows bf16 accumulate {R}x{C}", rel(yb, y0 + bf(Wf) @ x), 1e-5))
    return out


def check_layernorm():
    from procedurevrl_amd import ops
    g = torch.Generator().manual_seed(4)
    out = []
    for (M, C, eps) in [(1001, 768, 1e-6), (77, 512, 1e-5), (5000, 768, 1e-6)]:
        x = torch.randn(M, C, generator=g) * 2 + 0.3
        gam = torch.randn(C, generator=g)
        bet = torch.randn(C, generator=g)
        ref = F.layer_norm(x, (C,), gam, bet, eps)
        y, mean, rstd = ops.layernorm_fwd(x.to(dev()), gam.to(dev()), bet.to(dev()), eps, out_dtype=torch.float32)
        out.append((f"ln_fwd f32 {M}x{C}", rel(y, ref), TOL_F32))
        yb, _, _ = ops.layernorm_fwd(x.to(dev()), gam.to(dev()), bet.to(dev()), eps, out_dtype=BF)
        out.append((f"ln_fwd bf16 {M}x{C}", rel(yb, ref), TOL_BF16))
        out.append((f"ln_fwd mean {M}x{C}", rel(mean, x.mean(1)), TOL_F32))
        dy = torch.randn(M, C, generator=g)
        dxin = torch.randn(M, C, generator=g)
        xr = x.clone().requires_grad_(True)
        gr = gam.clone().requires_grad_(True)
        br = bet.clone().requires_grad_(True)
        F.layer_norm(xr, (C,), gr, br, eps).backward(dy)
        dg = torch.zeros(C, device=dev())
        db = torch.zeros(C, device=dev())
        dx = ops.layernorm_bwd(dy.to(dev()), x.to(dev()), mean, rstd, gam.to(dev()), dg, db, dx_in=dxin.to(dev()))
        out.append((f"ln_bwd dx {M}x{C}", rel(dx, xr.grad + dxin), TOL_F32))
        out.append((f"ln_bwd dgamma {M}x{C}", rel(dg, gr.grad), 1e-4))
        out.append((f"ln_bwd dbeta {M}x{C}", rel(db, br.grad), 1e-4))
        dyb = bf(dy)
        xr.grad = None
        F.layer_norm(xr, (C,), gam, bet, eps).backward(dyb)
        dx = ops.layernorm_bwd(dy.to(dev(), BF), x.to(dev()), mean, rstd, gam.to(dev()), dg, db)
        out.append((f"ln_bwd dx (bf16 dy) {M}x{C}", rel(dx, xr.grad), TOL_F32))
        rows = M - 5
        sc = torch.rand(M, generator=g) + 0.5
        dxs = torch.zeros(rows, C, device=dev(), dtype=BF)
        dx2 = ops.layernorm_bwd(dy.to(dev(), BF), x.to(dev()), mean, rstd, gam.to(dev()), dg, db, dxs=dxs, dxs_scale=sc.to(dev()))
        out.append((f"ln_bwd fused bf16 scaled copy {M}x{C}", rel(dxs, (sc[:, None] * dx2.cpu())[:rows]), 5e-3))
        # deferred reduces: the partials of several LayerNorms summed by ONE launch -- bit-equal to the immediate form, accumulate + scale incl.
        items = []
        want = []
        for rep, (beta, bsum) in enumerate(((0.0, 0.0), (1.0, 1.0), (0.0, 1.0))):
            a_g, a_b, a_s = (torch.full((C,), 0.5 + rep, device=dev()) for _ in range(3))
            d_g, d_b, d_s = a_g.clone(), a_b.clone(), a_s.clone()
            ops.layernorm_bwd(dy.to(dev(), BF), x.to(dev()), mean, rstd, gam.to(dev()), a_g, a_b, dxs=dxs, dxs_scale=sc.to(dev()),
                              beta_acc=beta, dxsum=a_s, dxsum_beta=bsum)
            ops.layernorm_bwd(dy.to(dev(), BF), x.to(dev()), mean, rstd, gam.to(dev()), d_g, d_b, dxs=dxs, dxs_scale=sc.to(dev()),
                              beta_acc=beta, dxsum=d_s, dxsum_beta=bsum, defer=items)
            want.append(((a_g, a_b, a_s), (d_g, d_b, d_s)))
        ops.layernorm_bwd_reduce_batched(items)
        diff = sum(float((a != d).sum()) for imm, dfr in want for a, d in zip(imm, dfr))
        out.append((f"ln_bwd deferred + batched reduce == immediate {M}x{C}", diff, 0.0))
        cs = torch.full((C,), 2.0, device=dev())
        dg2, db2 = torch.ones(C, device=dev()), torch.ones(C, device=dev())
        dx3 = ops.layernorm_bwd(dy.to(dev(), BF), x.to(dev()), mean, rstd, gam.to(dev()), dg2, db2, dxs=dxs, dxs_scale=sc.to(dev()),
                                beta_acc=1.0, dxsum=cs)
        out.append((f"ln_bwd unscaled column sums of the emitted rows (accumulating) {M}x{C}",
                    rel(cs, 2.0 + dx3.cpu()[:rows].sum(0)), 1e-5))
        out.append((f"ln_bwd dgamma with the column-sum output on {M}x{C}", rel(dg2, 1.0 + dg.cpu()), 1e-5))
    return out


def check_layernorm_bwd_refuses_before_launch():
    """dxsum_beta = 0 with beta_acc = 1 and no `defer`: the kernel has one beta for its three sums, and the host side can only split
    them for beta_acc = 0.  ops.layernorm_bwd raises PvrlError BEFORE anything is launched, for a plain x and for a SplitRows x:
    every output, pre-filled with a sentinel, is bit-for-bit untouched (label value = elements changed, + 1 if nothing was raised)."""
    from procedurevrl_amd import ops
    from procedurevrl_amd._lib import PvrlError
    g = torch.Generator().manual_seed(41)
    M, C, rows16 = 4, 768, 3
    x, dy = torch.randn(M, C, generator=g).to(dev()), torch.randn(M, C, generator=g).to(dev(), BF)
    gam = torch.randn(C, generator=g).to(dev())
    _, mean, rstd = ops.layernorm_fwd(x, gam, gam, 1e-6)
    out = []
    for kind in ("plain", "split"):
        sent = lambda *shape, dtype=torch.float32: torch.full(shape, 3.25, device=dev(), dtype=dtype)
        dg, db, dsum, dxs = sent(C), sent(C), sent(C), sent(M, C, dtype=BF)
        if kind == "plain":
            xin, dxo = x, sent(M, C)
            outs = [dxo]
        else:
            xin = ops.SplitRows(x[:rows16].to(BF), x[rows16:].contiguous())
            dxo = ops.SplitRows(sent(rows16, C, dtype=BF), sent(M - rows16, C))
            outs = [dxo.lo, dxo.hi]
        outs += [dg, db, dsum, dxs]
        raised = 0
        try:
            ops.layernorm_bwd(dy, xin, mean, rstd, gam, dg, db, dx_out=dxo, beta_acc=1.0, dxs=dxs, dxsum=dsum, dxsum_beta=0.0)
        except PvrlError:
            raised = 1
        torch.cuda.synchronize()
        changed = sum(int((t != 3.25).sum()) for t in outs)
        out.append((f"ln_bwd {kind}: dxsum_beta=0 with beta_acc=1 refused, outputs untouched", float(changed + 1 - raised), 0.0))
    return out


def check_split_residual_stream():
    """Round 6: the patch rows of the residual stream (and of its gradient) in the 16-bit operand type, the cls rows fp32 (pvrl_rows).
    PVRL_EPI_RESID_16 (16-bit residual in / out; the fp32 pos / time table form), pvrl_layernorm_fwd_split / _bwd_split and
    pvrl_batch_sum_bf16 vs fp32 math on the rounded inputs: they differ from it by the one rounding of a 16-bit output."""
    from procedurevrl_amd import ops
    from procedurevrl_amd._lib import lib
    L = lib()
    out = []
    g = torch.Generator().manual_seed(61)
    # every tile family: few rows (skinny kernel), 128 x 128, 256 x 128, the persistent 256 x 256 kernel with a ragged last panel
    for (M, N, K) in [(130, 768, 768), (300, 128, 64), (2500, 768, 256), (50208 - 32, 768, 128), (4230, 768, 3072)]:
        A = torch.randn(M, K, generator=g); W = torch.randn(N, K, generator=g) * 0.05
        bias = torch.randn(N, generator=g); b2 = torch.randn(N, generator=g)
        rs = torch.rand(M, generator=g) + 0.5
        resid = torch.randn(M, N, generator=g) * 3
        ref = bf(A) @ bf(W).t()
        Ad, Wd, rd = A.to(dev(), BF), W.to(dev(), BF), resid.to(dev(), BF)
        o = ops.gemm_nt(Ad, Wd, L.PVRL_EPI_RESID_16, bias=bias.to(dev()), rowscale=rs.to(dev()), aux=rd)
        want = bf(resid) + rs[:, None] * (ref + bias)
        out.append((f"gemm_nt resid_16 {M}x{N}x{K}", rel(o, want), TOL_BF16))
        out.append((f"gemm_nt resid_16 {M}x{N}x{K}: the rounding of the fp32 result, elementwise (max |diff| / |ref|)",
                    float((o.float().cpu() - bf(want)).abs().max() / want.abs().max()), 5e-3 if OPERAND == "bf16" else 6e-4))
        o = ops.gemm_nt(Ad, Wd, L.PVRL_EPI_RESID_16, bias=bias.to(dev()), rowscale=rs.to(dev()), aux=rd, bias2=b2.to(dev()))
        out.append((f"gemm_nt resid_16 + unscaled bias2 {M}x{N}x{K}", rel(o, bf(resid) + rs[:, None] * (ref + bias) + b2), TOL_BF16))
        o = ops.gemm_nt(Ad, Wd, L.PVRL_EPI_RESID_16, bias=bias.to(dev()), aux=rd, bias2=b2.to(dev()))
        out.append((f"gemm_nt resid_16 bias + bias2, no row scale {M}x{N}x{K}", rel(o, bf(resid) + ref + bias + b2), TOL_BF16))
        rm = 1568 if M > 4000 else 7
        E = torch.randn(rm, N, generator=g)
        o = ops.gemm_nt(Ad, Wd, L.PVRL_EPI_RESID_16, bias=bias.to(dev()), aux=E.to(dev()), aux_rowmod=rm)
        out.append((f"gemm_nt resid_16 fp32 table (rows mod {rm}) {M}x{N}x{K}", rel(o, E[torch.arange(M) % rm] + ref + bias), TOL_BF16))
    # LayerNorm over a split matrix: M = R + B rows, the first R 16-bit
    for (R, B, C, eps) in [(1000, 3, 768, 1e-6), (5008, 32, 768, 1e-6), (64, 2, 512, 1e-5), (12, 1, 768, 1e-6), (1, 1, 768, 1e-6)]:
        M = R + B
        x = torch.randn(M, C, generator=g) * 2 + 0.3
        xq = torch.cat([bf(x[:R]), x[R:]], 0)                     # what the split matrix holds
        gam = torch.randn(C, generator=g); bet = torch.randn(C, generator=g)
        xs = ops.SplitRows(x[:R].to(dev(), BF), x[R:].to(dev()))
        ref = F.layer_norm(xq, (C,), gam, bet, eps)
        y, mean, rstd = ops.layernorm_fwd(xs, gam.to(dev()), bet.to(dev()), eps, out_dtype=torch.float32)
        out.append((f"ln_fwd split {R}+{B}x{C}", rel(y, ref), TOL_F32))
        out.append((f"ln_fwd split mean {R}+{B}x{C}", rel(mean, xq.mean(1)), TOL_F32))
        y2, _, _ = ops.layernorm_fwd(ops.SplitRows(x[:R].to(dev(), BF), None), gam.to(dev()), bet.to(dev()), eps, out_dtype=torch.float32)
        out.append((f"ln_fwd split, 16-bit rows only {R}x{C}", rel(y2, ref[:R]), TOL_F32))
        dy = bf(torch.randn(M, C, generator=g))
        dxin = torch.randn(M, C, generator=g)
        dq = torch.cat([bf(dxin[:R]), dxin[R:]], 0)
        xr = xq.clone().requires_grad_(True)
        gr = gam.clone().requires_grad_(True); br = bet.clone().requires_grad_(True)
        F.layer_norm(xr, (C,), gr, br, eps).backward(dy)
        want = xr.grad + dq
        dg = torch.zeros(C, device=dev()); db = torch.zeros(C, device=dev())
        dsum = torch.zeros(C, device=dev())
        rows = max(1, R - 5)
        sc = torch.rand(M, generator=g) + 0.5
        dxs = torch.zeros(rows, C, device=dev(), dtype=BF)
        dxo = ops.SplitRows(torch.zeros(R, C, device=dev(), dtype=BF), torch.zeros(B, C, device=dev()))
        ops.layernorm_bwd(dy.to(dev(), BF), xs, mean, rstd, gam.to(dev()), dg, db,
                          dx_in=ops.SplitRows(dxin[:R].to(dev(), BF), dxin[R:].to(dev())), dx_out=dxo, dxs=dxs, dxs_scale=sc.to(dev()),
                          dxsum=dsum)
        out.append((f"ln_bwd split dx, 16-bit rows {R}+{B}x{C}", rel(dxo.lo, want[:R]), TOL_BF16))
        out.append((f"ln_bwd split dx, fp32 rows {R}+{B}x{C}", rel(dxo.hi, want[R:]), TOL_F32))
        out.append((f"ln_bwd split dgamma {R}+{B}x{C}", rel(dg, gr.grad), 1e-4))
        out.append((f"ln_bwd split dbeta {R}+{B}x{C}", rel(db, br.grad), 1e-4))
        out.append((f"ln_bwd split scaled 16-bit copy {R}+{B}x{C}", rel(dxs, (sc[:, None] * want)[:rows]), TOL_BF16))
        out.append((f"ln_bwd split column sums of the emitted rows {R}+{B}x{C}", rel(dsum, want[:rows].sum(0)), 1e-4))
        # a dx_in part that is known to be zero is not read (the pruned last block: no gradient has reached the patch rows yet)
        dxo2 = ops.SplitRows(torch.zeros(R, C, device=dev(), dtype=BF), torch.zeros(B, C, device=dev()))
        ops.layernorm_bwd(dy.to(dev(), BF), xs, mean, rstd, gam.to(dev()), dg, db, dx_in=ops.SplitRows(None, dxin[R:].to(dev()), n_lo=R),
                          dx_out=dxo2)
        out.append((f"ln_bwd split, zero patch part of dx_in: 16-bit rows {R}+{B}x{C}", rel(dxo2.lo, xr.grad[:R]), TOL_BF16))
        out.append((f"ln_bwd split, zero patch part of dx_in: fp32 rows {R}+{B}x{C}", rel(dxo2.hi, want[R:]), TOL_F32))
        # deferred partial sums + the batched reduce, as the engine runs it
        items = []
        d_g, d_b = torch.zeros(C, device=dev()), torch.zeros(C, device=dev())
        ops.layernorm_bwd(dy.to(dev(), BF), xs, mean, rstd, gam.to(dev()), d_g, d_b,
                          dx_in=ops.SplitRows(dxin[:R].to(dev(), BF), dxin[R:].to(dev())), dx_out=dxo, defer=items)
        ops.layernorm_bwd_reduce_batched(items)
        out.append((f"ln_bwd split deferred reduce == immediate {R}+{B}x{C}", float((d_g != dg).sum() + (d_b != db).sum()), 0.0))
    Bc, rows_, C = 5, 24, 768
    dx = torch.randn(Bc * rows_, C, generator=g)
    G = ops.batch_sum(dx.to(dev(), BF), Bc, rows_)
    out.append(("batch_sum over 16-bit rows", rel(G, bf(dx).view(Bc, rows_, C).sum(0)), TOL_F32))
    return out


def _ref_attn(q, k, v, scale, mask=None):
    s = (q @ k.transpose(-1, -2)) * scale
    if mask is not None:
        s = s.masked_fill(mask, float("-inf"))
    return torch.softmax(s, -1) @ v


def check_attn_t8():
    from procedurevrl_amd import ops
    g = torch.Generator().manual_seed(5)
    out = []
    nseq, H = 37, 12
    qkv = torch.randn(nseq * 8, 3 * H * 64, generator=g)
    qb = bf(qkv).view(nseq, 8, 3, H, 64).permute(2, 0, 3, 1, 4).clone().requires_grad_(True)
    o_ref = _ref_attn(qb[0], qb[1], qb[2], 0.125)  # [nseq,H,8,64]
    o_ref2 = o_ref.permute(0, 2, 1, 3).reshape(nseq * 8, H * 64)
    o = ops.attn_t8_fwd(qkv.to(dev(), BF), nseq, H, 0.125)
    out.append(("attn_t8 fwd", rel(o, o_ref2), TOL_BF16))
    do = torch.randn(nseq * 8, H * 64, generator=g)
    dob = bf(do)
    o_ref2.backward(dob)
    dref = qb.grad.permute(1, 3, 0, 2, 4).reshape(nseq * 8, 3 * H * 64)
    dq = ops.attn_t8_bwd(qkv.to(dev(), BF), do.to(dev(), BF), nseq, H, 0.125)
    HD = H * 64
    out.append(("attn_t8 bwd dq", rel(dq[:, :HD], dref[:, :HD]), TOL_BF16))
    out.append(("attn_t8 bwd dk", rel(dq[:, HD:2 * HD], dref[:, HD:2 * HD]), TOL_BF16))
    out.append(("attn_t8 bwd dv", rel(dq[:, 2 * HD:], dref[:, 2 * HD:]), TOL_BF16))
    return out


def check_attn_mfma_contig():
    """mode 0: contiguous sequences, with causal / key-padding masks (CLIP text, order transformer)."""
    from procedurevrl_amd import ops
    g = torch.Generator().manual_seed(6)
    out = []
    for (nseq, S, H, causal, pad) in [(5, 77, 8, True, False), (6, 9, 8, False, True), (3, 197, 12, False, False),
                                      (4, 32, 12, False, False), (2, 208, 2, False, False), (3, 16, 2, True, True),
                                      # longer crops: 224 (fused backward's last size), 257 = 256^2 / 16^2 + cls, 401 = 320^2
                                      (2, 224, 2, False, False), (2, 257, 2, False, False), (1, 401, 2, False, False),
                                      (3, 100, 2, False, False), (2, 150, 3, False, False),
                                      # one-wave-per-item backward (16 < S <= 32): ragged sequence lengths, more items than one workgroup's four
                                      (7, 24, 3, False, False), (5, 17, 2, False, False), (130, 32, 12, False, False)]:
        HD = H * 64
        qkv = torch.randn(nseq * S, 3 * HD, generator=g)
        qb = bf(qkv).view(nseq, S, 3, H, 64).permute(2, 0, 3, 1, 4).clone().requires_grad_(True)
        mask = torch.zeros(nseq, 1, S, S, dtype=torch.bool)
        kpm = None
        if causal:
            mask |= torch.triu(torch.ones(S, S, dtype=torch.bool), 1)
        if pad:
            kpm = torch.zeros(nseq, S, dtype=torch.bool)
            for i in range(nseq):
                start = 1 + int(torch.randint(0, S - 1, (1,), generator=g))
                kpm[i, start:] = True
            kpm[0, :] = False
            mask = mask | kpm[:, None, None, :]
        o_ref = _ref_attn(qb[0], qb[1], qb[2], 0.125, mask)
        o_ref2 = o_ref.permute(0, 2, 1, 3).reshape(nseq * S, HD)
        kd = kpm.to(torch.uint8).to(dev()) if kpm is not None else None
        qd = qkv.to(dev(), BF)
        o, _, lse = ops.attn_fwd(qd, nseq, S, H, 0.125, mode=0, causal=causal, kpm=kd)
        tag = f"attn S={S} H={H} c={int(causal)} p={int(pad)}"
        out.append((tag + " fwd", rel(o, o_ref2), TOL_BF16))
        do = torch.randn(nseq * S, HD, generator=g)
        o_ref2.backward(bf(do))
        dref = qb.grad.permute(1, 3, 0, 2, 4).reshape(nseq * S, 3 * HD)
        dq, _ = ops.attn_bwd(qd, o, None, do.to(dev(), BF), None, lse, nseq, S, H, 0.125, mode=0, causal=causal, kpm=kd)
        out.append((tag + " dq", rel(dq[:, :HD], dref[:, :HD]), 1.5e-2))
        out.append((tag + " dk", rel(dq[:, HD:2 * HD], dref[:, HD:2 * HD]), 1.5e-2))
        out.append((tag + " dv", rel(dq[:, 2 * HD:], dref[:, 2 * HD:]), 1.5e-2))
    return out


def check_attn_mfma_spatial():
    """mode 1: TimeSformer spatial gather (cls + every T-th row) addressed in place."""
    from procedurevrl_amd import ops
    g = torch.Generator().manual_seed(7)
    out = []
    # (11, 8, 196, 12): 88 sequences x 12 heads = 1,056 (sequence, head) items -> more than the persistent fused backward's 256
    # workgroups, ragged over them (some walk 5 items, some 4) and over the XCDs (11 sequences each); the forward is one workgroup per item
    # (1, 2, 256, 2): a 256^2 crop's 257-token spatial sequences (long-sequence instantiation of the two-pass kernels);
    # (3, 4, 120, 2): 121 tokens -> four query blocks in the fused backward's run-time-loop form, 12 sequences x 2 heads
    for (B, T, N, H) in [(2, 4, 16, 2), (2, 8, 196, 12), (11, 8, 196, 12), (1, 2, 256, 2), (3, 4, 120, 2)]:
        HD = H * 64
        S = N + 1
        R = B * N * T
        nseq = B * T
        qkv = torch.randn(R + B, 3 * HD, generator=g)
        qkvb = bf(qkv).clone().requires_grad_(True)
        # gather to [B*T, S, 3HD] exactly like vit.py:139-143
        tok = qkvb[:R].view(B, N, T, 3 * HD).permute(0, 2, 1, 3)              # b t n c
        cls = qkvb[R:].view(B, 1, 1, 3 * HD).expand(B, T, 1, 3 * HD)
        seqs = torch.cat([cls, tok], 2).reshape(nseq, S, 3, H, 64).permute(2, 0, 3, 1, 4)
        o_ref = _ref_attn(seqs[0], seqs[1], seqs[2], 0.125).permute(0, 2, 1, 3).reshape(B, T, S, HD)
        o_tok_ref = o_ref[:, :, 1:].permute(0, 2, 1, 3).reshape(R, HD)
        o_cls_ref = o_ref[:, :, 0].reshape(nseq, HD)
        qd = qkv.to(dev(), BF)
        obuf = torch.zeros(R + nseq, HD, device=dev(), dtype=BF)
        o, o_cls, lse = ops.attn_fwd(qd, nseq, S, H, 0.125, mode=1, T=T, cls_base=R, o=obuf[:R], o_cls=obuf[R:])
        tag = f"attn spatial B={B} T={T} N={N}"
        out.append((tag + " fwd tok", rel(o, o_tok_ref), TOL_BF16))
        out.append((tag + " fwd cls", rel(o_cls, o_cls_ref), TOL_BF16))
        do = torch.randn(R + nseq, HD, generator=g)
        dob = bf(do)
        (o_tok_ref * dob[:R]).sum().backward(retain_graph=True)
        (o_cls_ref * dob[R:]).sum().backward()
        dref = qkvb.grad
        dod = do.to(dev(), BF)
        dbuf = torch.zeros(R + B + nseq, 3 * HD, device=dev(), dtype=BF)
        dqkv, dcls = ops.attn_bwd(qd, obuf[:R], obuf[R:], dod[:R], dod[R:], lse, nseq, S, H, 0.125, mode=1, T=T,
                                  cls_base=R, dqkv=dbuf[:R + B], dqkv_cls=dbuf[R + B:])
        out.append((tag + " bwd tok", rel(dqkv[:R], dref[:R]), 1.5e-2))
        dcls_sum = dcls.float().view(B, T, 3 * HD).sum(1)
        out.append((tag + " bwd cls", rel(dcls_sum, dref[R:]), 1.5e-2))
    return out


def check_attn_cls():
    """pvrl_attn_cls_fwd / _bwd (the last block's spatial attention: the cls query only, csrc/attn_cls.hip) against fp32 autograd of
    vit.py:75-92 on the gathered sequences with the gradient fed to the cls queries' outputs only."""
    from procedurevrl_amd import ops
    g = torch.Generator().manual_seed(31)
    out = []
    for (B, T, N, H) in [(2, 4, 16, 2), (3, 8, 196, 12), (1, 2, 255, 3)]:
        HD = H * 64
        S = N + 1
        R = B * N * T
        nseq = B * T
        qkv = torch.randn(R + B, 3 * HD, generator=g)
        qkvb = bf(qkv).clone().requires_grad_(True)
        tok = qkvb[:R].view(B, N, T, 3 * HD).permute(0, 2, 1, 3)
        cls = qkvb[R:].view(B, 1, 1, 3 * HD).expand(B, T, 1, 3 * HD)
        seqs = torch.cat([cls, tok], 2).reshape(nseq, S, 3, H, 64).permute(2, 0, 3, 1, 4)
        o_ref = _ref_attn(seqs[0], seqs[1], seqs[2], 0.125).permute(0, 2, 1, 3).reshape(B, T, S, HD)
        o_cls_ref = o_ref[:, :, 0].reshape(nseq, HD)
        qd = qkv.to(dev(), BF)
        o_cls, lse = ops.attn_cls_fwd(qd, nseq, S, H, 0.125, T, R)
        tag = f"attn cls-query B={B} T={T} N={N}"
        out.append((tag + " fwd", rel(o_cls, o_cls_ref), TOL_BF16))
        do = torch.randn(nseq, HD, generator=g)
        dob = bf(do)
        (o_cls_ref * dob).sum().backward()
        dref = qkvb.grad
        dbuf = torch.full((R + B + nseq, 3 * HD), float("nan"), device=dev(), dtype=BF)      # every row must be written
        ops.attn_cls_bwd(qd, o_cls, do.to(dev(), BF), lse, nseq, S, H, 0.125, T, R, dbuf[:R + B], dbuf[R + B:])
        out.append((tag + " bwd tok", rel(dbuf[:R], dref[:R]), 1.5e-2))
        out.append((tag + " bwd tok: dQ of the patch tokens (max abs)", float(dbuf[:R, :HD].float().abs().max()), 0.0))
        dcls_sum = dbuf[R + B:].float().view(B, T, 3 * HD).sum(1)
        out.append((tag + " bwd cls", rel(dcls_sum, dref[R:]), 1.5e-2))
    return out


def check_attn_bwd_repeatable():
    """The persistent (S = 197, mode 1) and the one-wave (S = 32, mode 0) backward kernels stream their operands with counted waits
    and no workgroup-wide drains: launched repeatedly next to an uneven load on a second stream, every result must be BIT-identical
    to the first (a race on an LDS image or a wait that is one short shows as a run-to-run difference)."""
    from procedurevrl_amd import ops
    g = torch.Generator().manual_seed(21)
    out = []
    burn = torch.randn(4096, 4096, device=dev())
    side = torch.cuda.Stream()
    for (B, T, N, H, mode) in [(8, 8, 196, 12, 1), (392, 1, 31, 12, 0)]:
        HD = H * 64
        if mode == 1:
            S = N + 1; R = B * N * T; nseq = B * T
            qd = torch.randn(R + B, 3 * HD, generator=g).to(dev(), BF)
            obuf = torch.zeros(R + nseq, HD, device=dev(), dtype=BF)
            dod = torch.randn(R + nseq, HD, generator=g).to(dev(), BF)
            _, _, lse = ops.attn_fwd(qd, nseq, S, H, 0.125, mode=1, T=T, cls_base=R, o=obuf[:R], o_cls=obuf[R:])
            # (explicit zeroed outputs: the kernel leaves the cls rows of dqkv untouched -- token 0's gradients go to dqkv_cls)
            run = lambda: ops.attn_bwd(qd, obuf[:R], obuf[R:], dod[:R], dod[R:], lse, nseq, S, H, 0.125, mode=1, T=T, cls_base=R,
                                       dqkv=torch.zeros(R + B, 3 * HD, device=dev(), dtype=BF),
                                       dqkv_cls=torch.zeros(nseq, 3 * HD, device=dev(), dtype=BF))
        else:
            nseq, S = B, N + 1
            qd = torch.randn(nseq * S, 3 * HD, generator=g).to(dev(), BF)
            dod = torch.randn(nseq * S, HD, generator=g).to(dev(), BF)
            o, _, lse = ops.attn_fwd(qd, nseq, S, H, 0.125, mode=0)
            run = lambda: ops.attn_bwd(qd, o, None, dod, None, lse, nseq, S, H, 0.125, mode=0, dqkv=torch.zeros_like(qd))
        ref = [x.clone() for x in run() if x is not None]
        diff = 0
        for it in range(8):
            if it % 3 != 0:
                with torch.cuda.stream(side):
                    burn @ burn
            res = [x for x in run() if x is not None]
            diff += sum(int(not torch.equal(a.view(torch.int16), b.view(torch.int16))) for a, b in zip(ref, res))
        torch.cuda.synchronize()
        out.append((f"attn bwd S={S} mode {mode}: launches that differ from the first (of 8)", float(diff), 0.0))
    return out


def check_elementwise():
    from procedurevrl_amd import ops
    g = torch.Generator().manual_seed(8)
    out = []
    B, T, HI = 2, 4, 64
    frames = torch.randn(B, 3, T, HI, HI, generator=g)
    P = HI // 16
    # reference im2col in (b, n, t) order with (c, py, px) columns
    x = frames.permute(0, 2, 1, 3, 4).reshape(B, T, 3, P, 16, P, 16).permute(0, 3, 5, 1, 2, 4, 6)
    ref = x.reshape(B * P * P * T, 768)
    o = ops.patchify(frames.to(dev()))
    out.append(("patchify", rel(o, ref), 5e-3))
    N, C = 9, 768
    pos = torch.randn(1 + N, C, generator=g); tim = torch.randn(T, C, generator=g); bias = torch.randn(C, generator=g)
    E = ops.embed_table(pos.to(dev()), tim.to(dev()), bias.to(dev()), N, T)
    refE = (pos[1:, None, :] + tim[None, :, :] + bias).reshape(N * T, C)
    out.append(("embed_table", rel(E, refE), TOL_F32))
    dx = torch.randn(B * N * T, C, generator=g)
    G = ops.batch_sum(dx.to(dev()), B, N * T)
    out.append(("batch_sum", rel(G, dx.view(B, N * T, C).sum(0)), TOL_F32))
    rs = torch.rand(B * N * T, generator=g)
    cs = ops.cast_scale(dx.to(dev()), rs.to(dev()))
    out.append(("cast_scale", rel(cs, dx * rs[:, None]), 5e-3))
    w = torch.randn(300, 130, generator=g)
    wt = ops.cast_transpose(w.to(dev()))
    out.append(("cast_transpose", rel(wt, w.t()), 5e-3))
    wb, wtt = ops.cast_weight(w.to(dev()))
    out.append(("cast_weight bf16", rel(wb, w), 5e-3))
    out.append(("cast_weight transposed", rel(wtt, w.t()), 5e-3))
    o1 = torch.randn(768, 772, generator=g); av = torch.randn(768, generator=g); bv = torch.randn(768, generator=g)
    o1d = o1.to(dev())
    ops.rank1_add(o1d[:, :768], av.to(dev()), bv.to(dev()))            # a strided view: ld 772
    ref1 = o1.clone(); ref1[:, :768] += av[:, None] * bv[None, :]
    out.append(("rank1_add (addr_)", rel(o1d, ref1), TOL_F32))
    groups, Gs = 5, 8
    xin = torch.randn(groups * Gs, C, generator=g)
    sc = torch.rand(groups * Gs, generator=g)
    resid = torch.randn(groups, C, generator=g)
    r = ops.group_reduce(xin.to(dev()), groups, Gs, scale=sc.to(dev()), alpha=0.125, resid=resid.to(dev()))
    refr = resid + 0.125 * (xin * sc[:, None]).view(groups, Gs, C).sum(1)
    out.append(("group_reduce f32", rel(r, refr), TOL_F32))
    r = ops.group_reduce(xin.to(dev(), BF), groups, Gs, out_dtype=BF)
    out.append(("group_reduce bf16", rel(r, bf(xin).view(groups, Gs, C).sum(1)), 5e-3))
    gin = torch.randn(groups, C, generator=g)
    bc = ops.group_bcast(gin.to(dev()), groups, Gs, scale=sc.to(dev()), alpha=0.125)
    out.append(("group_bcast", rel(bc, 0.125 * sc[:, None] * gin.repeat_interleave(Gs, 0)), 5e-3))
    return out


def ref_kl_topk(pred, teacher, topk):
    """tools/train_net.py:152-160 verbatim semantics."""
    with torch.no_grad():
        t = F.softmax(teacher, 1)
        if topk != 0:
            t = (t.unsqueeze(1) * (t.unsqueeze(1) == t.topk(k=topk, dim=1)[0].unsqueeze(2)).float()).sum(1)
            t = t / t.sum(1, keepdim=True)
    loss = torch.nn.KLDivLoss(reduction="batchmean")(F.log_softmax(pred, dim=1), t)
    return loss, t


def check_loss():
    from procedurevrl_amd import ops
    g = torch.Generator().manual_seed(9)
    out = []
    x = torch.randn(26, 512, generator=g)
    y, inv = ops.l2norm_fwd(x.to(dev()))
    xr = x.clone().requires_grad_(True)
    yr = xr / xr.norm(dim=1, keepdim=True)
    out.append(("l2norm fwd", rel(y, yr), TOL_F32))
    dy = torch.randn(26, 512, generator=g)
    yr.backward(dy)
    dx = ops.l2norm_bwd(dy.to(dev()), y, inv)
    out.append(("l2norm bwd", rel(dx, xr.grad), TOL_F32))
    for (rows, K, topk) in [(26, 9871, 5), (7, 778, 5), (4, 300, 0), (3, 13001, 5)]:     # (K > 12288: the form that does not keep the row in LDS)
        pred = torch.randn(rows, K, generator=g) * 3
        teacher = torch.randn(rows, K, generator=g) * 4
        teacher[0, 5] = teacher[0, 9] = teacher[0].max() + 1.0  # exact tie inside the top-k (double counted by the reference)
        pr = pred.clone().requires_grad_(True)
        loss_ref, t_ref = ref_kl_topk(pr, teacher, topk)
        loss_ref.backward()
        rl, dp, tg = ops.kl_topk(pred.to(dev()), teacher.to(dev()), topk, grad_scale=1.0 / rows, want_target=True)
        out.append((f"kl_topk loss rows={rows} K={K} k={topk}", abs(rl.sum().item() / rows - loss_ref.item()) / abs(loss_ref.item()), 1e-4))
        out.append((f"kl_topk target rows={rows} K={K}", rel(tg, t_ref), 1e-4))
        out.append((f"kl_topk dpred rows={rows} K={K}", rel(dp, pr.grad), 1e-4))
    from oracle import timesformer_oracle as orc
    from procedurevrl_amd.functional import milnce_loss
    for (n, C, D) in [(4, 3, 16), (32, 1, 512), (24, 5, 64)]:
        v = torch.randn(n, D, generator=g) * 0.3
        t = torch.randn(n * C, D, generator=g) * 0.3
        vr = v.clone().requires_grad_(True); tr = t.clone().requires_grad_(True)
        lref = orc.milnce(vr, tr); lref.backward()
        vd = v.to(dev()).requires_grad_(True); td = t.to(dev()).requires_grad_(True)
        l = milnce_loss(vd, td); l.backward()
        out.append((f"milnce loss n={n} C={C}", abs(l.item() - lref.item()) / abs(lref.item()), 1e-5))
        out.append((f"milnce dV n={n} C={C}", rel(vd.grad, vr.grad), 1e-4))
        out.append((f"milnce dT n={n} C={C}", rel(td.grad, tr.grad), 1e-4))
    lg = torch.randn(7, 9871, generator=g) * 6
    out.append(("softmax rows (eval probabilities)", rel(ops.softmax_rows(lg.to(dev())), torch.softmax(lg, 1)), 1e-5))
    xg = (torch.randn(4, 512, generator=g) * 2).requires_grad_(True)
    dyg = torch.randn(4, 512, generator=g)
    F.gelu(xg).backward(dyg)
    out.append(("gelu f32", rel(ops.gelu_f32(xg.detach().to(dev())), F.gelu(xg.detach())), 1e-5))
    out.append(("gelu f32 backward", rel(ops.gelu_f32(xg.detach().to(dev()), dyg.to(dev())), xg.grad), 1e-5))
    a = torch.randn(8, 512, generator=g); b = torch.randn(8, 512, generator=g)
    ar = a.clone().requires_grad_(True); br = b.clone().requires_grad_(True)
    lref = F.mse_loss(ar, br); lref.backward()
    l, da, db = ops.mse(a.to(dev()), b.to(dev()), grad_scale=1.0)
    out.append(("mse loss", abs(l.item() - lref.item()) / lref.item(), TOL_F32))
    out.append(("mse da", rel(da, ar.grad), TOL_F32))
    out.append(("mse db", rel(db, br.grad), TOL_F32))
    return out


def check_input_pipeline():
    """pvrl_frames_u8_patchify (normalise + bilinear rescale + crop + flip + im2col on decoded uint8 clips) against
    (a) the REFERENCE's own CPU chain (tests/golden/input_pipeline.pt) and (b) the oracle on a ragged random batch.
    Output is bf16: 1 bf16 ulp (2^-8 relative) on the few values whose fp32 result sits on a rounding boundary.
    These are aggregate bounds against the reference's order of operations.  The per-pixel contract -- every element bit-equal to the
    kernel-order fp32 model, on every clamp, scale, crop, `_views` arrangement and past the workgroup cap -- is held by
    tests/input_checks.py (tests/test_input_kernels_gpu.py), which also measures how far that model lies from this reference."""
    import os
    import numpy as np
    from procedurevrl_amd import ops
    from procedurevrl_amd.transform import DecodedClips, spatial_sampling_params
    from oracle import timesformer_oracle as orc
    out = []
    gold = torch.load(os.path.join(os.path.dirname(__file__), "golden", "input_pipeline.pt"), weights_only=False)

    def cmp(name, got, ref):
        ref_b = ref.to(BF).float()
        d = (got.float().cpu() - ref_b).abs()
        ulp = ref_b.abs().clamp_min(2.0 ** -10) * 2.0 ** -7
        out.append((name + " max err / bf16 ulp", float((d / ulp).max()), 1.01))
        # twice the worst fraction by which the kernel-order model differs from these references on these very inputs (1.45e-3, fp16
        # operands; tests/test_input_harness_host.py measures and asserts it); was 2e-2
        out.append((name + " fraction not bit-equal", float((d > 0).float().mean()), 3e-3))

    for i, c in enumerate(gold["cases"]):
        np.random.seed(c["seed"])
        prm = spatial_sampling_params(c["H0"], c["W0"], c["spatial_idx"], c["min_scale"], c["max_scale"], c["crop"],
                                      c["flip"], c["inv"])
        clips = DecodedClips(c["frames"].unsqueeze(0).to(dev()), [prm], gold["mean"], gold["std"], c["crop"])
        got = ops.frames_u8_patchify(clips)
        cmp(f"u8 pipeline vs reference case {i}", got, orc.patch_rows(c["out"].unsqueeze(0)))
    g = torch.Generator().manual_seed(5)
    B, T, H0, W0, crop = 5, 3, 72, 100, 64
    fr = torch.randint(0, 256, (B, T, H0, W0, 3), generator=g, dtype=torch.uint8)
    np.random.seed(11)
    prms = [spatial_sampling_params(H0, W0, -1, 64, 96, crop) for _ in range(B)]
    ref = torch.stack([orc.input_pipeline(fr[b], prms[b], [0.45, 0.40, 0.5], [0.225, 0.25, 0.2], crop) for b in range(B)])
    got = ops.frames_u8_patchify(DecodedClips(fr.to(dev()), prms, [0.45, 0.40, 0.5], [0.225, 0.25, 0.2], crop))
    cmp("u8 pipeline vs oracle, batch of 5", got, orc.patch_rows(ref))
    f32 = ops.frames_u8_to_f32(DecodedClips(fr.to(dev()), prms, [0.45, 0.40, 0.5], [0.225, 0.25, 0.2], crop))
    out.append(("u8 pipeline -> fp32 clip tensor vs oracle", rel(f32, ref), 1e-6))
    return out


ALL_CHECKS = [check_input_pipeline, check_gemm_nt, check_gemm_nt_batched, check_small_batched, check_grad_scale_begin, check_gemm_f32_small, check_cls_linear, check_gemm_tn, check_gemm_tn_rows_behind_the_end, check_gemm_tn_repeatable, check_gemm_tn_into, check_gemm_tn_grouped, check_gemm_tn_grouped_block_size, check_cast_weights_multi, check_gemv_rows, check_layernorm, check_layernorm_bwd_refuses_before_launch, check_split_residual_stream, check_attn_t8, check_attn_cls,
              check_attn_mfma_contig, check_attn_mfma_spatial, check_attn_bwd_repeatable, check_elementwise, check_loss]
