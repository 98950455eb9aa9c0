"""The kernels at ViT-L's sizes (embed_dim 1024, 16 heads, MLP 4096), through the existing harnesses and under their rules -- no bound of
this file's own (pytest -m gpu):

  * LayerNorm forward / backward / split / batched reduce at C = 1024 (the NV = 4 instantiations of csrc/norm.hip) against fp64 with the
    bounds of kernel_checks.check_layernorm / check_split_residual_stream, M = 66 and 4,612 rows, and a `dxs_scale` vector of dxs_rows < M
    entries (nothing behind dxs_rows may be read: include/pvrl.h).  At M = 4,612 (dxs_rows = 4,608 = 36 x 128 floats) its last entry is
    the last float of its allocation; at M = 66 (dxs_rows = 64) it is an ordinary allocation, only shorter than M.  A read behind it would
    land in the allocator's pool and neither fault nor show in the numbers: what keeps the kernel from it is the `row < dxs_rows` select
    of ln_bwd_rows (csrc/norm.hip); these cases pin the interface the engine uses (an R-long vector under an M = R + B-row launch);
  * pvrl_cls_linear_f32 at (N, K) = (1024, 1024), (4096, 1024), (1024, 4096) -- the last one the four-slice path -- for M = 2, 17, 33, both
    epilogues, under kernel_checks.check_cls_linear's rule;
  * the NT / TN / grouped-TN GEMMs at the seven ViT-L operand shapes for M = 4,612 and the 1024^3 batched small problems through
    tests/gemm_checks.py (exact and per-segment);
  * attention with H = 16 through tests/attn_checks.py's per-row rule: attn_t8, the in-LDS kernel at S = 145 (mode 1, T = 8) and the
    cls-query kernel.  The harness pads every input's leading dimension by 8 columns behind the 3 * H * 64 = 3,072 owned ones (its guard
    band); test_attention_with_a_qkv_leading_dimension_of_exactly_3072 runs the three kernels on the engine's own operand, a contiguous
    [rows, 3072] qkv with 4,612 rows (577 sequences = 4,616 rows for attn_t8): no multiple of any tile.

On the commit before this one the LayerNorm tests fail with `pvrl_layernorm_fwd failed with status -1` (C = 1024 is refused) and the
N = 2048 / 1536 cases of test_gemm_nt_at_the_vit_l_shapes leave 128-row halves of their output unwritten (launch_nt8's grid); the other
GEMM, cls-chain and attention cases already passed at these sizes, which these tests now pin."""
import pytest
import torch
import torch.nn.functional as F

import attn_checks as ac
import gemm_checks as gc
import kernel_checks as kc

C = 1024
BF = kc.BF
M_ROWS = (66, 4612)


def dev():
    return kc.dev()


def _show(name, out):
    for label, e, tol in out:
        print(f"[{name}] {label}: err={e:.3e} tol={tol:g}")
    bad = [(label, e, tol) for label, e, tol in out if not e <= tol]
    assert not bad, bad


def _verdict(name, findings, mod):
    print(f"\n== {name}\n{mod.report(findings)}")
    bad = [f for f in findings if not f.ok]
    assert not bad, name + "\n" + mod.report(bad)


def _ln64(x, gam, bet, eps, dy=None):
    """fp64 LayerNorm of fp32-valued inputs -> y (and dx, dgamma, dbeta for `dy`)"""
    xr = x.double().requires_grad_(True)
    gr, br = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    y = F.layer_norm(xr, (x.shape[1],), gr, br, eps)
    if dy is None:
        return y.detach()
    y.backward(dy.double())
    return y.detach(), xr.grad, gr.grad, br.grad


def _tail_of_an_allocation(n):
    """fp32 [n] whose last element is the last float of its allocation (n a multiple of 128: 512-byte blocks leave no slack)"""
    assert n % 128 == 0
    t = torch.empty(n, device=dev(), dtype=torch.float32)
    assert t.untyped_storage().nbytes() == 4 * n
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("M", M_ROWS)
def test_layernorm_c1024_plain_rows(M):
    """kernel_checks.check_layernorm's quantities and bounds at C = 1024, references in fp64"""
    from procedurevrl_amd import ops
    g = torch.Generator().manual_seed(400 + M)
    eps = 1e-6
    x = torch.randn(M, C, generator=g) * 2 + 0.3
    gam, bet = torch.randn(C, generator=g), torch.randn(C, generator=g)
    dy, dxin = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    xd, gd, bd = x.to(dev()), gam.to(dev()), bet.to(dev())
    ref, dx64, dg64, db64 = _ln64(x, gam, bet, eps, dy)
    out = []
    y, mean, rstd = ops.layernorm_fwd(xd, gd, bd, eps, out_dtype=torch.float32)
    out.append((f"ln_fwd f32 {M}x{C}", kc.rel(y, ref), kc.TOL_F32))
    yb, _, _ = ops.layernorm_fwd(xd, gd, bd, eps, out_dtype=BF)
    out.append((f"ln_fwd 16-bit {M}x{C}", kc.rel(yb, ref), kc.TOL_BF16))
    out.append((f"ln_fwd mean {M}x{C}", kc.rel(mean, x.double().mean(1)), kc.TOL_F32))
    out.append((f"ln_fwd rstd {M}x{C}", kc.rel(rstd, (x.double().var(1, unbiased=False) + eps).rsqrt()), kc.TOL_F32))
    dg, db = torch.zeros(C, device=dev()), torch.zeros(C, device=dev())
    dx = ops.layernorm_bwd(dy.to(dev()), xd, mean, rstd, gd, dg, db, dx_in=dxin.to(dev()))
    out.append((f"ln_bwd dx {M}x{C}", kc.rel(dx, dx64 + dxin.double()), kc.TOL_F32))
    out.append((f"ln_bwd dgamma {M}x{C}", kc.rel(dg, dg64), 1e-4))
    out.append((f"ln_bwd dbeta {M}x{C}", kc.rel(db, db64), 1e-4))
    dyb = kc.bf(dy)
    _, dxb64, dgb64, _ = _ln64(x, gam, bet, eps, dyb)
    dx = ops.layernorm_bwd(dy.to(dev(), BF), xd, mean, rstd, gd, dg, db)
    out.append((f"ln_bwd dx (16-bit dy) {M}x{C}", kc.rel(dx, dxb64), kc.TOL_F32))
    # the emitted 16-bit copy of the first dxs_rows rows, its DropPath vector dxs_rows long and flush with the end of its allocation
    rows = 128 * ((M - 2) // 128) if M > 130 else M - 2
    if rows % 128 == 0:
        sc = _tail_of_an_allocation(rows)
        sc.copy_(torch.rand(rows, generator=g) + 0.5)
    else:
        sc = (torch.rand(rows, generator=g) + 0.5).to(dev())
    dxs = torch.zeros(rows, C, device=dev(), dtype=BF)
    cs = torch.full((C,), 2.0, device=dev())
    dg2, db2 = torch.ones(C, device=dev()), torch.ones(C, device=dev())
    dx2 = ops.layernorm_bwd(dy.to(dev(), BF), xd, mean, rstd, gd, dg2, db2, dxs=dxs, dxs_scale=sc, beta_acc=1.0, dxsum=cs)
    out.append((f"ln_bwd 16-bit scaled copy, dxs_scale of dxs_rows = {rows} < M entries {M}x{C}",
                kc.rel(dxs, sc.cpu().double()[:, None] * dxb64[:rows]), 5e-3))
    out.append((f"ln_bwd dx with the copy on {M}x{C}", kc.rel(dx2, dxb64), kc.TOL_F32))
    out.append((f"ln_bwd unscaled column sums of the emitted rows (accumulating) {M}x{C}", kc.rel(cs, 2.0 + dxb64[:rows].sum(0)), 1e-5))
    out.append((f"ln_bwd dgamma with the column-sum output on (accumulating) {M}x{C}", kc.rel(dg2, 1.0 + dgb64), 1e-4))
    # deferred partials + ONE batched reduce == the immediate form, bit for bit, accumulate and scale included
    items, want = [], []
    for rep, (beta, bsum) in enumerate(((0.0, 0.0), (1.0, 1.0), (0.0, 1.0))):
        a_g, a_b, a_s = (torch.full((C,), 0.5 + rep, device=dev()) for _ in range(3))
        d_g, d_b, d_s = a_g.clone(), a_b.clone(), a_s.clone()
        ops.layernorm_bwd(dy.to(dev(), BF), xd, mean, rstd, gd, a_g, a_b, dxs=dxs, dxs_scale=sc, beta_acc=beta, dxsum=a_s, dxsum_beta=bsum)
        ops.layernorm_bwd(dy.to(dev(), BF), xd, mean, rstd, gd, d_g, d_b, dxs=dxs, dxs_scale=sc, beta_acc=beta, dxsum=d_s, dxsum_beta=bsum,
                          defer=items)
        want.append(((a_g, a_b, a_s), (d_g, d_b, d_s)))
    ops.layernorm_bwd_reduce_batched(items)
    diff = sum(float((a != d).sum()) for imm, dfr in want for a, d in zip(imm, dfr))
    out.append((f"ln_bwd deferred + batched reduce == immediate {M}x{C}", diff, 0.0))
    _show(f"layernorm C={C} M={M}", out)


@pytest.mark.gpu
@pytest.mark.parametrize("M,B", [(66, 2), (4612, 4)])
def test_layernorm_c1024_split_residual_stream(M, B):
    """kernel_checks.check_split_residual_stream's LayerNorm quantities and bounds at C = 1024: R = M - B patch rows 16-bit, B cls rows fp32,
    the emitted copy's DropPath vector R entries long (as the engine passes s1_tok / s2_tok to an M-row launch) and flush with the end of
    its allocation where R allows it"""
    from procedurevrl_amd import ops
    g = torch.Generator().manual_seed(600 + M)
    eps, R = 1e-6, M - B
    x = torch.randn(M, C, generator=g) * 2 + 0.3
    xq = torch.cat([kc.bf(x[:R]), x[R:]], 0)                     # what the split matrix holds
    gam, bet = torch.randn(C, generator=g), torch.randn(C, generator=g)
    gd, bd = gam.to(dev()), bet.to(dev())
    xs = ops.SplitRows(x[:R].to(dev(), BF), x[R:].to(dev()))
    dy = kc.bf(torch.randn(M, C, generator=g))
    dxin = torch.randn(M, C, generator=g)
    dq = torch.cat([kc.bf(dxin[:R]), dxin[R:]], 0).double()
    ref, dx64, dg64, db64 = _ln64(xq, gam, bet, eps, dy)
    want = dx64 + dq
    out = []
    y, mean, rstd = ops.layernorm_fwd(xs, gd, bd, eps, out_dtype=torch.float32)
    out.append((f"ln_fwd split {R}+{B}x{C}", kc.rel(y, ref), kc.TOL_F32))
    out.append((f"ln_fwd split mean {R}+{B}x{C}", kc.rel(mean, xq.double().mean(1)), kc.TOL_F32))
    y16, _, _ = ops.layernorm_fwd(xs, gd, bd, eps)
    out.append((f"ln_fwd split, 16-bit output {R}+{B}x{C}", kc.rel(y16, ref), kc.TOL_BF16))
    y2, _, _ = ops.layernorm_fwd(ops.SplitRows(x[:R].to(dev(), BF), None), gd, bd, eps, out_dtype=torch.float32)
    out.append((f"ln_fwd split, 16-bit rows only {R}x{C}", kc.rel(y2, ref[:R]), kc.TOL_F32))
    rows = R                                                        # 64 and 4,608 = 36 * 128
    if rows % 128 == 0:
        sc = _tail_of_an_allocation(rows)
        sc.copy_(torch.rand(rows, generator=g) + 0.5)
    else:
        sc = (torch.rand(rows, generator=g) + 0.5).to(dev())
    sc64 = sc.cpu().double()
    dg, db, dsum = (torch.zeros(C, device=dev()) for _ in range(3))
    dxs = torch.zeros(rows, C, device=dev(), dtype=BF)
    dxo = ops.SplitRows(torch.zeros(R, C, device=dev(), dtype=BF), torch.zeros(B, C, device=dev()))
    din = lambda: ops.SplitRows(dxin[:R].to(dev(), BF), dxin[R:].to(dev()))
    ops.layernorm_bwd(dy.to(dev(), BF), xs, mean, rstd, gd, dg, db, dx_in=din(), dx_out=dxo, dxs=dxs, dxs_scale=sc, dxsum=dsum)
    out.append((f"ln_bwd split dx, 16-bit rows {R}+{B}x{C}", kc.rel(dxo.lo, want[:R]), kc.TOL_BF16))
    out.append((f"ln_bwd split dx, fp32 rows {R}+{B}x{C}", kc.rel(dxo.hi, want[R:]), kc.TOL_F32))
    out.append((f"ln_bwd split dgamma {R}+{B}x{C}", kc.rel(dg, dg64), 1e-4))
    out.append((f"ln_bwd split dbeta {R}+{B}x{C}", kc.rel(db, db64), 1e-4))
    out.append((f"ln_bwd split scaled 16-bit copy, dxs_scale of {rows} < M entries {R}+{B}x{C}",
                kc.rel(dxs, (sc64[:, None] * want[:rows])), kc.TOL_BF16))
    out.append((f"ln_bwd split column sums of the emitted rows {R}+{B}x{C}", kc.rel(dsum, want[:rows].sum(0)), 1e-4))
    # a dx_in part that is known to be zero is not read (the pruned last block)
    dxo2 = ops.SplitRows(torch.zeros(R, C, device=dev(), dtype=BF), torch.zeros(B, C, device=dev()))
    ops.layernorm_bwd(dy.to(dev(), BF), xs, mean, rstd, gd, dg, db, dx_in=ops.SplitRows(None, dxin[R:].to(dev()), n_lo=R), dx_out=dxo2)
    out.append((f"ln_bwd split, zero patch part of dx_in: 16-bit rows {R}+{B}x{C}", kc.rel(dxo2.lo, dx64[:R]), kc.TOL_BF16))
    out.append((f"ln_bwd split, zero patch part of dx_in: fp32 rows {R}+{B}x{C}", kc.rel(dxo2.hi, want[R:]), kc.TOL_F32))
    # deferred partial sums + the batched reduce, as the engine runs it
    items = []
    d_g, d_b, d_s = (torch.zeros(C, device=dev()) for _ in range(3))
    ops.layernorm_bwd(dy.to(dev(), BF), xs, mean, rstd, gd, d_g, d_b, dx_in=din(), dx_out=dxo, dxs=dxs, dxs_scale=sc, dxsum=d_s, defer=items)
    ops.layernorm_bwd_reduce_batched(items)
    out.append((f"ln_bwd split deferred reduce == immediate {R}+{B}x{C}",
                float((d_g != dg).sum() + (d_b != db).sum() + (d_s != dsum).sum()), 0.0))
    _show(f"layernorm split C={C} {R}+{B}", out)


@pytest.mark.gpu
def test_layernorm_refuses_a_width_without_an_instantiation():
    from procedurevrl_amd import ops
    from procedurevrl_amd._lib import PvrlError
    x = torch.zeros(4, 384, device=dev())
    w = torch.ones(384, device=dev())
    with pytest.raises(PvrlError):
        ops.layernorm_fwd(x, w, w, 1e-6)


CLS_SHAPES = [(M, N, K) for (N, K) in ((1024, 1024), (4096, 1024), (1024, 4096)) for M in (2, 17, 33)]


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", CLS_SHAPES, ids=[f"{m}x{n}x{k}" for m, n, k in CLS_SHAPES])
def test_cls_linear_at_the_vit_l_shapes(M, N, K):
    """kernel_checks.check_cls_linear's rule: fp64 math on the same fp32 inputs, kc.TOL_F32; K / 8 = 128 per wave takes launch_cls's KU = 2
    branch, (1024, 4096) four K slices of 1024 (gemm_checks.cls_names restates the dispatch)"""
    from procedurevrl_amd import ops
    assert gc.cls_ksplit(N, K) == (4 if K == 4096 else 1) and "KU2" in gc.cls_kernel(M, K, gc.cls_ksplit(N, K))
    g = torch.Generator().manual_seed(12 + M + N + K)
    X = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) * 0.05
    bias = torch.randn(N, generator=g)
    rs, bs = torch.rand(M, generator=g) + 0.5, torch.rand(M, generator=g) + 0.5
    aux = torch.randn(M, N, generator=g)
    Xd, Wd, bd = X.to(dev()), W.to(dev()), bias.to(dev())
    acc = X.double() @ W.double().t()
    out = []
    o = ops.cls_linear(Xd, Wd, bd)
    out.append((f"cls_linear {M}x{N}x{K}", kc.rel(o, acc + bias), kc.TOL_F32))
    o = ops.cls_linear(Xd, Wd, bd, rowscale=rs.to(dev()), biasscale=bs.to(dev()), aux=aux.to(dev()))
    out.append((f"cls_linear residual {M}x{N}x{K}", kc.rel(o, aux + rs[:, None] * acc + bs[:, None] * bias), kc.TOL_F32))
    o = ops.cls_linear(Xd, Wd, bd, gelu=True)
    out.append((f"cls_linear gelu {M}x{N}x{K}", kc.rel(o, F.gelu(acc + bias)), kc.TOL_F32))
    big = torch.zeros(M + 5, N + 64, device=dev())
    ops.cls_linear(Xd, Wd, None, out=big[5:, :N])
    out.append((f"cls_linear strided out {M}x{N}x{K}", kc.rel(big[5:, :N], acc), kc.TOL_F32))
    out.append((f"cls_linear repeatable {M}x{N}x{K}", float((ops.cls_linear(Xd, Wd, bd) != ops.cls_linear(Xd, Wd, bd)).sum()), 0.0))
    _show(f"cls_linear {M}x{N}x{K}", out)


# the seven linear maps of a ViT-L step at M = 4,612 rows (l_nt8's M), with the epilogue the engine gives each:
#   forward: qkv (temporal and spatial), the fused temporal map / proj, fc1, fc2, the patch embedding; data gradients: through qkv, through fc2
M_NT8 = 4612
NT_CASES = [gc._nt(M_NT8, 3072, 1024, "bf16"), gc._nt(M_NT8, 1024, 1024, "resid_16"), gc._nt(M_NT8, 4096, 1024, "gelu"),
            gc._nt(M_NT8, 1024, 4096, "resid_16"), gc._nt(M_NT8, 1024, 768, "resid_16.tab"), gc._nt(M_NT8, 1024, 3072, "bf16"),
            gc._nt(M_NT8, 4096, 1024, "dgelu")]
# the pruned last block's key / value GEMM (N = 2 C: the query third is the cls rows' alone) at ViT-L's and ViT-B's width.  With 19 row
# panels, five XCDs own two of them: 2 x 8 = 16 (2 x 6 = 12) tiles go out as 32 (24) half items next to the 24 (18) whole tiles of the
# XCDs that own three -- the longer list must size the persistent grid (launch_nt8)
NT_CASES += [gc._nt(M_NT8, 2048, 1024, "bf16"), gc._nt(M_NT8, 1536, 768, "bf16")]
NT_TESTS = [(c, r) for c in NT_CASES for r in ("exact", "randn")]


@pytest.mark.gpu
@pytest.mark.parametrize("case,regime", NT_TESTS, ids=[f"{gc.nt_case_id(c)}-{r}" for c, r in NT_TESTS])
def test_gemm_nt_at_the_vit_l_shapes(case, regime):
    # launch_nt as it stands (no new dispatch rule): the persistent kernel from M >= 4,096 for these N; the patch embedding's fp32-table
    # epilogue lives in the one-tile kernel
    assert ("nt8" in case.kernel) == (case.epi != "resid_16.tab"), case.kernel
    _verdict(f"{gc.nt_case_id(case)}-{regime}", gc.check_nt_case(case, regime), gc)


# the weight gradients of the same maps: dW [N, K] = dy^T x over the 4,612 rows
TN_CASES = [gc._tn(M_NT8, 3072, 1024), gc._tn(M_NT8, 1024, 1024, beta=1.0, gexp=-3), gc._tn(M_NT8, 4096, 1024), gc._tn(M_NT8, 1024, 4096, beta=0.5),
            gc._tn(M_NT8, 1024, 768, gexp=2)]
TN_TESTS = [(c, "exact") for c in TN_CASES] + [(TN_CASES[0], "randn"), (TN_CASES[3], "randn")]


@pytest.mark.gpu
@pytest.mark.parametrize("case,regime", TN_TESTS, ids=[f"{gc.tn_case_id(c)}-{r}" for c, r in TN_TESTS])
def test_gemm_tn_at_the_vit_l_shapes(case, regime):
    _verdict(f"{gc.tn_case_id(case)}-{regime}", gc.check_tn_case(case, regime), gc)


# a divided block's seven weight gradients as the engine's ONE grouped launch (temporal qkv, W_e, qkv, proj, fc1, fc2) + the patch embedding's
GROUP_L = gc._group([(M_NT8, 3072, 1024, True, 0.0, 0), (M_NT8, 1024, 1024, True, 0.0, 0), (M_NT8, 3072, 1024, True, 1.0, -3),
                     (M_NT8, 1024, 1024, True, 0.5, 0), (M_NT8, 4096, 1024, True, 0.0, 2), (M_NT8, 1024, 4096, True, 1.0, 0),
                     (M_NT8, 1024, 768, True, 0.0, 0)])


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["exact", "randn"])
def test_gemm_tn_grouped_seven_vit_l_problems(regime):
    _verdict(f"{gc.group_case_id(GROUP_L)}-{regime}", gc.check_group_case(GROUP_L, regime), gc)


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["exact", "randn"])
@pytest.mark.parametrize("epi", ["f32", "resid_f32"])
def test_gemm_nt_batched_1024_cubed(epi, regime, monkeypatch):
    """W_e = W_fc W_proj of every block and the gradient recovery of _temporal_chain_all: 1024^3 problems, thirteen = two launches"""
    monkeypatch.setattr(gc, "BATCH_SHAPES", [(1024, 1024, 1024)] * 13)
    _verdict(f"batched-1024^3-{epi}-{regime}", gc.check_nt_batched(epi, regime), gc)


def _cls_case(B, T, S, H, z):
    return ac.Case("cls", 1, B * T, S, H, T, ac.POW2, False, False, 8, z, "cls_fwd+cls_bwd" + ("" if z else "_nodq"))


# H = 16: 3 * 16 * 64 = 3,072 columns of qkv.  t8 with nseq = 577 (4 x 144 + 1: no multiple of anything); the in-LDS kernel at S = 145 with
# B * T = 8 and 24 sequences (24 x 16 = 384 items exceed the persistent backward's grid of 256); the cls-query kernel at S = 145 and 442
ATTN_CASES = [ac.Case("t8", 0, 37, 8, 16, 1, ac.POW2, False, False, 8, True, "t8_fwd+t8_bwd"),
              ac.Case("t8", 0, 577, 8, 16, 1, ac.POW2, False, False, 8, True, "t8_fwd+t8_bwd"),
              ac._attn(1, 8, 145, 16, T=8), ac._attn(1, 24, 145, 16, T=8),
              _cls_case(2, 8, 145, 16, True), _cls_case(2, 8, 145, 16, False), _cls_case(2, 2, 442, 16, True), _cls_case(2, 2, 442, 16, False)]
ATTN_TESTS = [(c, r) for c in ATTN_CASES for r in ("randn", "peaked")]


@pytest.mark.gpu
@pytest.mark.parametrize("case,regime", ATTN_TESTS, ids=[f"{ac.case_id(c)}-{r}" for c, r in ATTN_TESTS])
def test_attention_with_sixteen_heads(case, regime):
    assert case.H == 16
    _verdict(f"{ac.case_id(case)}-{regime}", ac.check_case(case, regime), ac)


# the engine's own operand: qkv with a leading dimension of EXACTLY 3,072 (no padding columns behind the 16 heads; the harness's guard rows
# stay behind the last row, so a read past the end still shows in the numbers) and row counts that are no multiple of a tile -- l_nt8's
# geometry, 4 clips of 8 x 144 patches: 4,612 rows for the spatial kernels (32 sequences of 145 tokens sharing 4 cls rows), 577 sequences
# = 4,616 rows for attn_t8
LD3072_CASES = [ac.Case("t8", 0, 577, 8, 16, 1, ac.POW2, False, False, 8, True, "t8_fwd+t8_bwd"), ac._attn(1, 32, 145, 16, T=8),
                _cls_case(4, 8, 145, 16, True), _cls_case(4, 8, 145, 16, False)]
LD3072_TESTS = [(c, r) for c in LD3072_CASES for r in ("randn", "peaked")]


@pytest.mark.gpu
@pytest.mark.parametrize("case,regime", LD3072_TESTS, ids=[f"ld3072-{ac.case_id(c)}-{r}" for c, r in LD3072_TESTS])
def test_attention_with_a_qkv_leading_dimension_of_exactly_3072(case, regime, monkeypatch):
    padded = ac.guarded_input
    seen = []

    def unpadded(x, dtype, device, extra_cols=8):
        if x.shape[1] != 3072:            # dO keeps the harness's padding: the entry points take ONE leading dimension for o and dO, and
            return padded(x, dtype, device, extra_cols)       # the guarded output buffers carry 8 columns of guard band
        t = padded(x, dtype, device, extra_cols=0)
        seen.append((tuple(t.shape), t.stride(0)))
        return t
    monkeypatch.setattr(ac, "guarded_input", unpadded)
    findings = ac.check_case(case, regime)
    rows = 577 * 8 if case.entry == "t8" else 4612
    assert seen and all(q == ((rows, 3072), 3072) for q in seen), seen[:2]           # the qkv operand: [rows, 3072], contiguous
    _verdict(f"ld3072-{ac.case_id(case)}-{regime}", findings, ac)
