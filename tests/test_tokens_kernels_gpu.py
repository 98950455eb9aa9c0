"""pvrl_layernorm_fwd_tokens / pvrl_layernorm_bwd_tokens (csrc/norm.hip): the encoder's final norm over every token, whose fp32 side --
y in the forward, dy in the backward -- lies in the reference's token order [B, 1 + P, C] while x, the statistics, dx and the emitted
16-bit copy keep the engine's rows (B * P patch rows, then the B cls rows).  Against fp64 LayerNorm on the CPU, EVERY row on its own
(the worst row's relative L2 error), under kernel_checks.TOL_F32 / TOL_BF16 as the LayerNorm checks of kernel_checks use them (fp32
rows and statistics: TOL_F32; rows stored in the 16-bit operand type: TOL_BF16; dgamma / dbeta: 1e-4).  (pytest -m gpu)

Shapes (B clips of P patch rows): 3 x 32 -- clip seams inside a workgroup's group of rows (4 waves x 2 rows on the 16-bit part, 4 rows
on the fp32 part; 33 is a multiple of neither); 16 x 4 -- `space_only`'s pseudo-clip shape, a seam in every group; 2 x 882 -- many row
groups per clip.  Each at C = 768 and 1024, as a split stream (rows16 = R) and as a plain fp32 one (rows16 = 0)."""
import pytest
import torch
import torch.nn.functional as F

import kernel_checks as kc
from kernel_checks import BF, TOL_BF16, TOL_F32, bf

TOL_SUMS = 1e-4         # dgamma / dbeta, as kernel_checks.check_layernorm / check_split_residual_stream hold them
EPS = 1e-6
CANARY = 12345.5
SHAPES = [(3, 32), (16, 4), (2, 882)]


def _worst_row(a, b):
    """the largest relative L2 error of a row of `a` against the fp64 rows `b`"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    if not torch.isfinite(a).all():
        return float("inf")
    return float(((a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-30)).max())


def _to_tokens(rows, B):
    """engine rows [B * P + B, C] -> token rows [B * (P + 1), C]: clip b's cls row, then its P patch rows"""
    M, C = rows.shape
    R = M - B
    return torch.cat([rows[R:].view(B, 1, C), rows[:R].view(B, R // B, C)], 1).reshape(M, C)


def _case(B, P, C, split, seed):
    from procedurevrl_amd import ops
    d = kc.dev()
    g = torch.Generator().manual_seed(seed)
    R, M = B * P, B * P + B
    x = torch.randn(M, C, generator=g) * 2 + 0.3
    xq = torch.cat([bf(x[:R]), x[R:]], 0) if split else x          # what the stream holds
    gam, bet = torch.randn(C, generator=g), torch.randn(C, generator=g)
    mk = (lambda t: ops.SplitRows(t[:R].to(d, BF), t[R:].to(d))) if split else (lambda t: t.to(d))
    return dict(B=B, P=P, C=C, R=R, M=M, g=g, split=split, xq=xq, gam=gam, bet=bet, xs=mk(x), mk=mk, d=d)


def _rows_out(c):
    """a zeroed dx_out for the case, and a function that reads it back as fp32 engine rows"""
    from procedurevrl_amd import ops
    if c["split"]:
        o = ops.SplitRows(torch.zeros(c["R"], c["C"], device=c["d"], dtype=BF), torch.zeros(c["B"], c["C"], device=c["d"]))
        return o, lambda: torch.cat([o.lo.float(), o.hi], 0)
    o = torch.zeros(c["M"], c["C"], device=c["d"])
    return o, lambda: o


@pytest.mark.gpu
@pytest.mark.parametrize("split", [True, False], ids=["split", "plain"])
@pytest.mark.parametrize("C", [768, 1024])
@pytest.mark.parametrize("B,P", SHAPES)
def test_forward_every_row_and_the_guard_rows(B, P, C, split):
    from procedurevrl_amd import ops
    c = _case(B, P, C, split, 7)
    M = c["M"]
    big = torch.full((M + 2, C), CANARY, device=c["d"])          # a guard row in front of the tokens and one behind them
    y, mean, rstd = ops.layernorm_fwd_tokens(c["xs"], c["gam"].to(c["d"]), c["bet"].to(c["d"]), EPS, P, out=big[1:M + 1])
    torch.cuda.synchronize()
    assert bool((big[0] == CANARY).all()) and bool((big[M + 1] == CANARY).all()), "a guard row was written"
    x64 = c["xq"].double()
    ref = F.layer_norm(x64, (C,), c["gam"].double(), c["bet"].double(), EPS)
    res = [("tokens, every row", _worst_row(y, _to_tokens(ref, B)), TOL_F32),
           ("mean (engine rows)", kc.rel(mean, x64.mean(1)), TOL_F32),
           ("rstd (engine rows)", kc.rel(rstd, (x64.var(1, unbiased=False) + EPS).rsqrt()), TOL_F32)]
    for label, e, tol in res:
        print(f"[fwd {B}x{P} C={C} {'split' if split else 'plain'}] {label}: err={e:.3e} tol={tol:g}")
    assert not [r for r in res if not r[1] <= r[2]], res


@pytest.mark.gpu
@pytest.mark.parametrize("split", [True, False], ids=["split", "plain"])
@pytest.mark.parametrize("C", [768, 1024])
@pytest.mark.parametrize("B,P", SHAPES)
def test_backward_every_row_sums_and_the_emitted_copy(B, P, C, split):
    from procedurevrl_amd import ops
    c = _case(B, P, C, split, 11)
    d, g, R, M = c["d"], c["g"], c["R"], c["M"]
    gam_d = c["gam"].to(d)
    _, mean, rstd = ops.layernorm_fwd_tokens(c["xs"], gam_d, c["bet"].to(d), EPS, P)
    dtok = torch.randn(M, C, generator=g)                        # token order
    dy_rows = torch.cat([dtok.view(B, P + 1, C)[:, 1:].reshape(R, C), dtok.view(B, P + 1, C)[:, 0]], 0)     # the same in engine rows
    dxin = torch.randn(M, C, generator=g)
    dq = torch.cat([bf(dxin[:R]), dxin[R:]], 0) if split else dxin
    xr = c["xq"].double().requires_grad_(True)
    gr, br = c["gam"].double().requires_grad_(True), c["bet"].double().requires_grad_(True)
    F.layer_norm(xr, (C,), gr, br, EPS).backward(dy_rows.double())
    tol_p = TOL_BF16 if split else TOL_F32                       # the patch rows of dx are 16-bit in a split stream
    res = []

    def rows_err(tag, got, want):
        res.append((f"{tag}: dx patch rows", _worst_row(got[:R], want[:R]), tol_p))
        res.append((f"{tag}: dx cls rows", _worst_row(got[R:], want[R:]), TOL_F32))

    # ---- no dx_in, beta_acc = 0; the emitted 16-bit copy SHORTER than M, it and its scale vector flush with their allocations
    rows = max(1, R - 5)
    sc = torch.rand(rows, generator=g) + 0.5
    dxs = torch.zeros(rows, C, device=d, dtype=BF)
    dg, db = torch.full((C,), 7.0, device=d), torch.full((C,), 7.0, device=d)
    dxo, read = _rows_out(c)
    ops.layernorm_bwd(dtok.to(d), c["xs"], mean, rstd, gam_d, dg, db, dx_out=dxo, dxs=dxs, dxs_scale=sc.to(d), rows_per_clip=P)
    rows_err("no dx_in", read(), xr.grad)
    res.append(("no dx_in: dgamma (beta_acc 0 overwrites)", kc.rel(dg, gr.grad), TOL_SUMS))
    res.append(("no dx_in: dbeta", kc.rel(db, br.grad), TOL_SUMS))
    res.append((f"emitted 16-bit copy, {rows} of {M} rows", _worst_row(dxs, sc[:, None].double() * xr.grad[:rows]), TOL_BF16))

    # ---- dx_in, beta_acc = 1, gscale; the copy over all M rows (what the engine asks for: the last block's first operand)
    want = xr.grad + dq.double()
    gsc = torch.tensor([0.125], device=d)
    old_g, old_b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    dg1, db1 = old_g.to(d), old_b.to(d)
    sc_all = torch.rand(M, generator=g) + 0.5
    dxs_all = torch.zeros(M, C, device=d, dtype=BF)
    dxo, read = _rows_out(c)
    ops.layernorm_bwd(dtok.to(d), c["xs"], mean, rstd, gam_d, dg1, db1, dx_in=c["mk"](dxin), dx_out=dxo, beta_acc=1.0, gscale=gsc,
                      dxs=dxs_all, dxs_scale=sc_all.to(d), rows_per_clip=P)
    rows_err("dx_in", read(), want)
    res.append(("dx_in: dgamma = old + gscale * sums", kc.rel(dg1, old_g.double() + 0.125 * gr.grad), TOL_SUMS))
    res.append(("dx_in: dbeta = old + gscale * sums", kc.rel(db1, old_b.double() + 0.125 * br.grad), TOL_SUMS))
    res.append((f"emitted 16-bit copy, all {M} rows", _worst_row(dxs_all, sc_all[:, None].double() * want), TOL_BF16))

    # ---- the deferred reduce, as the engine runs it, against the immediate one: the same bits
    items = []
    dg2, db2 = old_g.to(d), old_b.to(d)
    dxo2, read2 = _rows_out(c)
    ops.layernorm_bwd(dtok.to(d), c["xs"], mean, rstd, gam_d, dg2, db2, dx_in=c["mk"](dxin), dx_out=dxo2, beta_acc=1.0, defer=items,
                      rows_per_clip=P)
    assert len(items) == 1
    ops.layernorm_bwd_reduce_batched(items, gscale=gsc)
    torch.cuda.synchronize()
    assert torch.equal(dg2, dg1) and torch.equal(db2, db1), "deferred reduce differs from the immediate one"
    assert torch.equal(read2(), read())
    for label, e, tol in res:
        print(f"[bwd {B}x{P} C={C} {'split' if split else 'plain'}] {label}: err={e:.3e} tol={tol:g}")
    assert not [r for r in res if not r[1] <= r[2]], [r for r in res if not r[1] <= r[2]]


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_a_launch():
    from procedurevrl_amd import ops
    from procedurevrl_amd._lib import PvrlError
    d = kc.dev()

    def fwd(M, C, P):
        x = torch.zeros(M, C, device=d)
        return ops.layernorm_fwd_tokens(x, torch.ones(C, device=d), torch.zeros(C, device=d), EPS, P)

    def bwd(M, C, P):
        x = torch.zeros(M, C, device=d)
        st = torch.ones(M, device=d)
        return ops.layernorm_bwd(torch.zeros(M, C, device=d), x, st, st, torch.ones(C, device=d), torch.zeros(C, device=d),
                                 torch.zeros(C, device=d), dx_out=torch.zeros(M, C, device=d), rows_per_clip=P)

    for call in (fwd, bwd):
        for M, C, P in [(10, 512, 4), (10, 640, 4), (10, 768, 0), (10, 1024, -1), (11, 768, 4)]:     # width; rows_per_clip; M % (P + 1)
            with pytest.raises(PvrlError):
                call(M, C, P)
        call(10, 768, 4)
    x = ops.SplitRows(torch.zeros(7, 768, device=d, dtype=BF), torch.zeros(3, 768, device=d))           # split at 7, not at R = 8
    with pytest.raises(PvrlError):
        ops.layernorm_fwd_tokens(x, torch.ones(768, device=d), torch.zeros(768, device=d), EPS, 4)
    torch.cuda.synchronize()
