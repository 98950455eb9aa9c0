"""The long-sequence attention kernels (pvrl_attn_long_fwd / _bwd, csrc/attn_long.hip) under the rules of tests/attn_checks.py: its fp64
reference by query chunks, its rounding model (oracle/rounded_oracle.AttnMFMA), its per-row metric, guard bands and tolerance rule --
rowerr(kernel) <= ROW_FACTOR * rowerr(model), the lse rule as written there.  No new constants.

Used by tests/test_attn_long_gpu.py (pytest -m gpu) and tests/test_attn_long_harness_host.py (no GPU: `model_online`, the streamed
kernel's own rounding model, stands in for the kernel, and planted defects show that the inherited rule bites on an online softmax).

What is new here is aimed at the online rescale: a streamed kernel carries a running maximum m and a running sum l over key tiles
of KT keys and multiplies l and its accumulators by exp(m - m') whenever a tile raises the maximum.  Three regimes make that happen
where it can go wrong (each on top of N(0, 1) v and dO; q and k at a quarter / half of that so the planted term decides):
    ramp / ramp_rev   every query's score rises (falls) linearly with the key index over RAMP_SPREAD: every full key tile raises the
                      running maximum (ramp), or only the first one does and every later P is tiny against l (ramp_rev)
    late_peak         the LAST key -- in the ragged last tile wherever S is no multiple of KT -- beats every other by PEAK: the last
                      tile rescales everything accumulated before it by <= exp(-30)
    early_peak        the same at key 0: every later tile is rounded against a maximum far above it
The score spread each regime reaches is recorded as a finding (always ok) so the run shows it.
"""
import torch

import attn_checks as ac
from procedurevrl_amd import ops

KT, QT, MAX_S = ops.ATTN_LONG_KT, ops.ATTN_LONG_QT, ops.ATTN_LONG_MAX_S
BF = ac.BF
OLD_REGIMES = ("randn", "hot", "peaked", "offset", "equal")
NEW_REGIMES = ("ramp", "ramp_rev", "late_peak", "early_peak")
REGIMES = OLD_REGIMES + NEW_REGIMES
RAMP_SPREAD = 24.0       # scaled-score units from the first key to the last
PEAK = 40.0              # the planted key's scaled score above the rest's mean; the rest spread over a few units: margin >= 30
Q0 = 8.0                 # the constant first feature of every query that the planted key feature multiplies


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def _long(mode, nseq, S, H, T=1, scale=ac.POW2, ldd_extra=8):
    return ac.Case("long", mode, nseq, S, H, T, scale, False, False, ldd_extra, True, "long_fwd+long_bwd")


def _build_tests():
    tests = []
    # mode 0: one key tile and its edges, two tiles and a ragged third, a second query block, the first length the short kernels
    # refuse, and a ragged 9th tile; (QT + 1 = 2 KT + 1 with today's tiles: the set removes the double)
    for S in sorted({1, KT - 1, KT, KT + 1, 2 * KT + 1, QT + 1, 417, 513}):
        tests += [(_long(0, 3, S, 2), r) for r in REGIMES]
    heavy = ("randn", "peaked") + NEW_REGIMES
    tests += [(_long(0, 2, 785, 12), r) for r in heavy]                 # TimeSformer-HR's tokens per frame, every head column
    tests += [(_long(1, 2, 1569, 2), r) for r in heavy]                 # joint attention at 8 x 224^2
    tests += [(_long(1, 3, 513, 12), r) for r in heavy]                 # joint attention at 32 x 64^2: the engine test's shape
    tests += [(_long(1, 4, 450, 2, T=2), r) for r in REGIMES]           # general T: two sequences share a cls row
    tests += [(_long(0, 1, 6273, 1), "randn")]                          # EPIC-Kitchens' 32 x 224^2
    # the scale that is no power of two; a dqkv leading dimension of 3 * H * 64 + 4
    tests += [(_long(0, 3, 2 * KT + 1, 2, scale=ac.ODD_SCALE), r) for r in REGIMES]
    tests += [(_long(1, 4, 450, 2, T=2, scale=ac.ODD_SCALE), r) for r in REGIMES]
    tests += [(_long(0, 3, 2 * KT + 1, 2, ldd_extra=4), r) for r in ("randn", "late_peak")]
    tests += [(_long(1, 3, 513, 12, ldd_extra=4), r) for r in ("randn", "late_peak")]
    return tests


TESTS = _build_tests()
SHORT_TOO = [(c, r) for c, r in TESTS if c.S <= ops.ATTN_MAX_S and c.scale == ac.POW2 and c.ldd_extra == 8 and r in ("randn", "late_peak")]


def case_id(c):
    return ac.case_id(c)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def token_index(c):
    """token index j of every packed qkv row (mode 1: patch rows (b, n, t) hold token n + 1, then the B cls rows hold token 0)"""
    if c.mode == 0:
        return torch.arange(c.nseq * c.S) % c.S
    B, N = c.nseq // c.T, c.S - 1
    return torch.cat([(torch.arange(B * N * c.T) // c.T) % N + 1, torch.zeros(B, dtype=torch.long)])


def make_problem(c, regime, operand=None, seed=None):
    """attn_checks.make_problem for its regimes; the new ones plant feature 0 of q (a constant) and k (a function of the token index)"""
    if regime in OLD_REGIMES:
        return ac.make_problem(c, regime, operand, seed)
    operand = BF if operand is None else operand
    base = ac.make_problem(c, "randn", torch.float32, seed=(777 + 31 * REGIMES.index(regime) + 7 * c.S + c.nseq) if seed is None else seed)
    HD = c.H * 64
    qkv = base["qkv"].reshape(-1, 3, c.H, 64).clone()
    qkv[:, 0] *= 0.25
    qkv[:, 1] *= 0.5
    j = token_index(c).double()
    unit = 1.0 / (c.scale * Q0)                     # key feature that adds 1 to the scaled score
    if regime in ("ramp", "ramp_rev"):
        frac = j / max(c.S - 1, 1)
        k0 = RAMP_SPREAD * (frac if regime == "ramp" else 1.0 - frac) * unit
    else:
        k0 = torch.where(j == (c.S - 1 if regime == "late_peak" else 0), PEAK * unit, 0.0)
    qkv[:, 0, :, 0] = Q0
    qkv[:, 1, :, 0] = k0.float()[:, None]
    base["qkv"] = ac._rnd(qkv.reshape(-1, 3 * HD), operand)
    base["do"] = ac._rnd(base["do"], operand)
    return base


def score_spread(q, k, scale):
    """largest over (item, query) of max_j - min_j of the scaled scores, and the smallest margin of the row maximum over the runner-up"""
    s = (q[:2].double() @ k[:2].double().transpose(-1, -2)) * scale
    top = s.topk(min(2, s.shape[-1]), -1).values
    margin = (top[..., 0] - top[..., -1]).min().item()
    return (s.amax(-1) - s.amin(-1)).max().item(), margin


# ---------------------------------------------------------------------------------------------------------------------
# the streamed kernel's rounding model (host)
# ---------------------------------------------------------------------------------------------------------------------
def model_online(q, k, v, do, scale, operand, kt=None, defect=None):
    """csrc/attn_long.hip in fp32 on the CPU, rounding where it rounds: key tiles of `kt` in order, the tile's scores against the running
    maximum m', l and the accumulator times exp(m - m') in fp32, P rounded to the operand type only for the second product, summed
    unrounded; o = acc / l rounded; backward with P from lse, D from the stored o, dS and P rounded as operands.
    defect (what a broken kernel would do; for tests/test_attn_long_harness_host.py):
      "stale_l"      l is not rescaled when a tile raises the maximum
      "unmasked"     the zero-filled keys of the ragged last tile take part with score 0
      "unscaled_pv"  the accumulator is not rescaled in front of the last tile's P.V"""
    kt = KT if kt is None else kt
    rnd = lambda x: ac._rnd(x, operand)
    n, S, _ = q.shape
    m = torch.full((n, S, 1), float("-inf"))
    l = torch.zeros(n, S, 1)
    acc = torch.zeros(n, S, 64)
    for ti, j0 in enumerate(range(0, S, kt)):
        kj, vj = k[:, j0:j0 + kt], v[:, j0:j0 + kt]
        if defect == "unmasked" and kj.shape[1] < kt:
            pad = kt - kj.shape[1]
            kj = torch.cat([kj, torch.zeros(n, pad, 64)], 1)
            vj = torch.cat([vj, torch.zeros(n, pad, 64)], 1)
        t = (q @ kj.transpose(-1, -2)) * scale
        mn = torch.maximum(m, t.amax(-1, keepdim=True))
        alpha = torch.exp(m - mn)
        p = torch.exp(t - mn)
        l = (l if defect == "stale_l" else l * alpha) + p.sum(-1, keepdim=True)
        acc = (acc if (defect == "unscaled_pv" and j0 + kt >= S) else acc * alpha) + rnd(p) @ vj
        m = mn
    o = rnd(acc / l)
    lse = m + torch.log(l)
    s = (q @ k.transpose(-1, -2)) * scale
    p = torch.exp(s - lse)
    dp = do @ v.transpose(-1, -2)
    d = (do * o).sum(-1, keepdim=True)
    ds = rnd(p * (dp - d) * scale)
    return dict(o=o, lse=lse[..., 0], dq=rnd(ds @ k), dk=rnd(ds.transpose(-1, -2) @ q), dv=rnd(rnd(p).transpose(-1, -2) @ do))


def judge_host(c, regime, operand, defect=None):
    """`model_online` in the kernel's place under attn_checks.judge -> findings"""
    prob = make_problem(c, regime, operand)
    items = ac.choose_items(c)
    q, k, v, do, _ = ac.gathered_inputs(c, prob, items)
    ref = ac.reference(q, k, v, do, c.scale, None)
    mod = ac.model(q, k, v, do, c.scale, None, operand)
    got = model_online(q, k, v, do, c.scale, operand, defect=defect)
    return ac.judge(c, regime, got, ref, mod, items, (q, k, v, do), operand)


# ---------------------------------------------------------------------------------------------------------------------
# the kernels (GPU)
# ---------------------------------------------------------------------------------------------------------------------
def run_kernels(c, prob, items, short=False, keep=None):
    """the case through ops.attn_long_fwd / _bwd (short: ops.attn_fwd / _bwd, the second yardstick) on cuda:0 -> (got, guard findings);
    `keep` (a dict) receives the raw device buffers of the backward for the run-to-run comparison"""
    dev = torch.device("cuda:0")
    HD, R, B, S, nseq, H = c.H * 64, prob["R"], prob["B"], c.S, c.nseq, c.H
    qd = ac.guarded_input(prob["qkv"], BF, dev)
    dod = ac.guarded_input(prob["do"], BF, dev)
    cpu = lambda t: t.float().cpu()
    m1 = c.mode == 1
    ntok = R if m1 else nseq * S
    fwd, bwd = (ops.attn_fwd, ops.attn_bwd) if short else (ops.attn_long_fwd, ops.attn_long_bwd)
    ob = ac.Guarded("o / o_cls", [ntok] + ([nseq] if m1 else []), HD, BF, 8, device=dev)
    lb = ac.Guarded("lse", [nseq * H], S, torch.float32, 0, device=dev)
    lse = lb.seg(0).view(nseq, H, S)
    fwd(qd, nseq, S, H, c.scale, mode=c.mode, T=c.T, cls_base=R, o=ob.seg(0), o_cls=ob.seg(1) if m1 else None, lse=lse)
    db = ac.Guarded("dqkv / dqkv_cls", [ntok + B] + ([nseq] if m1 else []), 3 * HD, BF, c.ldd_extra,
                    unowned=[(0, R, R + B, 0, 3 * HD)] if m1 else (), device=dev)
    args = (qd, ob.seg(0), ob.seg(1) if m1 else None, dod[:ntok], dod[ntok:] if m1 else None, lse, nseq, S, H, c.scale)
    kw = dict(mode=c.mode, T=c.T, cls_base=R)
    bwd(*args, **kw, dqkv=db.seg(0), dqkv_cls=db.seg(1) if m1 else None)
    torch.cuda.synchronize()
    if keep is not None:
        keep.update(args=args, kw=kw, db=db, m1=m1)
    f = ob.check() + lb.check() + db.check()
    og = ac.gather(c, cpu(ob.seg(0)), cpu(ob.seg(1)) if m1 else None, 1, False)[0, items]
    dg = ac.gather(c, cpu(db.seg(0))[:ntok], cpu(db.seg(1)) if m1 else None, 3, False)[:, items]
    return dict(o=og, lse=cpu(lb.seg(0))[items], dq=dg[0], dk=dg[1], dv=dg[2]), f


def _collect(c, regime, with_short=False):
    items = ac.choose_items(c)
    findings, parts = [], []
    for d in range(ac.n_draws(c)):
        prob = make_problem(c, regime, seed=None if d == 0 else d)
        got, guards = run_kernels(c, prob, items)
        findings += [f for f in guards if d == 0 or not f.ok]
        q, k, v, do, _ = ac.gathered_inputs(c, prob, items)
        ref = ac.reference(q, k, v, do, c.scale, None)
        mod = ac.model(q, k, v, do, c.scale, None, BF)
        part = [got, ref, mod, dict(q=q, k=k, v=v, do=do), items + d * c.nseq * c.H]
        if with_short:
            part.append(run_kernels(c, prob, items, short=True)[0])
        parts.append(part)
    cat = lambda j: {key: torch.cat([p[j][key] for p in parts]) for key in parts[0][j]}
    return findings, parts, cat


def check_case(c, regime):
    """one case x regime on the GPU -> list of Finding (score spread, guard bands, then attn_checks' tolerance rule per tensor)"""
    findings, parts, cat = _collect(c, regime)
    got, ref, mod, inp = (cat(j) for j in range(4))
    spread, margin = score_spread(inp["q"], inp["k"], c.scale)
    head = [ac.Finding(f"score spread [{regime}]", True, spread, 0.0, f"smallest margin of a row's maximum over its runner-up {margin:.2f}")]
    return head + findings + ac.judge(c, regime, got, ref, mod, torch.cat([p[4] for p in parts]), (inp["q"], inp["k"], inp["v"], inp["do"]))


def check_against_short(c, regime):
    """S <= 416: pvrl_attn_fwd / _bwd on the same inputs as a second yardstick.  Each kernel is held to ROW_FACTOR * rowerr(model)
    against fp64 and typically sits near 1 x; the two then differ by about twice the model's error, so the distance between them is
    held to the same ROW_FACTOR * rowerr(model) (in the units of the fp64 reference's row norm), lse to twice attn_checks' lse bound."""
    findings, parts, cat = _collect(c, regime, with_short=True)
    got, ref, mod, inp, short = cat(0), cat(1), cat(2), cat(3), cat(5)
    out = []
    for name in ("o", "dq", "dk", "dv"):
        n = ac.row_rms(ref[name])
        if ref[name].abs().max().item() < 1e-10:      # zero reference: each kernel is within ROW_FACTOR * max|model| + floor of zero
            n = 1.0
            floor = ac.fp32_zero_floor(inp["q"], inp["k"], inp["v"], inp["do"], c.scale).get(name, 0.0)
            bound = 2 * (ac.ROW_FACTOR * mod[name].abs().max().item() + floor)
        else:
            bound = ac.ROW_FACTOR * ac.rowerr(mod[name], ref[name])[0]
        e = (got[name].double() - short[name].double()).pow(2).sum(-1).sqrt().max().item() / n
        out.append(ac.Finding(f"{name}: long vs short kernel, worst row", e <= bound, e, bound, "in units of the reference's rms row norm"))
    y = (ref["lse32"].double() - ref["lse"]).abs().max().item()
    ulp = 2.0 ** -23 * max(1.0, ref["lse"].abs().max().item())
    e = (got["lse"].double() - short["lse"].double()).abs().max().item()
    out.append(ac.Finding("lse: long vs short kernel", e <= 2 * (ac.LSE_FACTOR * y + ac.LSE_ULPS * ulp), e, 2 * (ac.LSE_FACTOR * y + ac.LSE_ULPS * ulp), ""))
    return [f for f in findings if not f.ok] + out


def check_backward_twice(c, regime="randn"):
    """the backward run twice on the same inputs and forward outputs: every byte of dqkv / dqkv_cls equal"""
    prob = make_problem(c, regime)
    keep = {}
    run_kernels(c, prob, ac.choose_items(c), keep=keep)
    db = keep["db"]
    first = db.buf.view(db.idt).clone()
    db.buf.view(db.idt).zero_()
    ops.attn_long_bwd(*keep["args"], **keep["kw"], dqkv=db.seg(0), dqkv_cls=db.seg(1) if keep["m1"] else None)
    torch.cuda.synchronize()
    second = db.buf.view(db.idt)
    same = torch.equal(first.cpu()[db.owned], second.cpu()[db.owned])
    return [ac.Finding("dqkv / dqkv_cls: second run bit-equal to the first", same, 0.0 if same else 1.0, 0.0, case_id(c))]


def check_refusals():
    """S = 0 and S = MAX_S + 1: PVRL_EINVAL from both entry points and not one byte of the guarded outputs changes"""
    from procedurevrl_amd._lib import PvrlError
    dev = torch.device("cuda:0")
    nseq, H = 1, 1
    out = []
    for S in (0, MAX_S + 1):
        rows = max(S, 1)
        qd = torch.zeros(rows, 3 * H * 64, device=dev, dtype=BF)
        ob = ac.Guarded("o", [rows], H * 64, BF, 8, device=dev)
        lb = ac.Guarded("lse", [nseq * H], rows, torch.float32, 0, device=dev)
        db = ac.Guarded("dqkv", [rows], 3 * H * 64, BF, 8, device=dev)
        lse = lb.seg(0).view(nseq, H, rows)
        calls = (("fwd", lambda: ops.attn_long_fwd(qd, nseq, S, H, ac.POW2, o=ob.seg(0), lse=lse)),
                 ("bwd", lambda: ops.attn_long_bwd(qd, ob.seg(0), None, ob.seg(0), None, lse, nseq, S, H, ac.POW2, dqkv=db.seg(0))))
        for what, call in calls:
            try:
                call()
                msg = "returned 0"
            except PvrlError as e:
                msg = str(e)
            out.append(ac.Finding(f"pvrl_attn_long_{what} S={S}: status", msg.endswith("status -1"), 0.0, 0.0, msg))
        torch.cuda.synchronize()
        for g in (ob, lb, db):
            same = torch.equal(g.buf.view(g.idt).cpu(), g.before)
            out.append(ac.Finding(f"S={S}: {g.name} untouched", same, 0.0 if same else 1.0, 0.0, ""))
    return out
