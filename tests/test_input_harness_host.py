"""The input-kernel harness (tests/input_checks.py) without a GPU: the CPU models stand in for the kernels.  The kernel-order model is
close to the reference's order of operations (measured, printed with -s, asserted at twice the recorded value), the bit-equality rule
bites (every planted defect fails a named case, and the finding names the element), and the case table holds what it claims."""
import fractions

import numpy as np
import pytest
import torch

import input_checks as ic
from oracle import timesformer_oracle as orc

SMALL = [c for c in ic.DEC_CASES if "below_cap" in c.path and c.B <= 8]
PAST = [c for c in ic.DEC_CASES if "past_the_8192_workgroup_cap" in c.path]


def _failed(findings):
    return [f for f in findings if not f.ok]


# ---------------------------------------------------------------------------------------------------------------------
# the tools
# ---------------------------------------------------------------------------------------------------------------------
def test_torch_fp32_elementwise_arithmetic_rounds_once_like_numpy():
    g = ic._gen("arith")
    a, b = torch.rand(4096, generator=g) * 255, torch.rand(4096, generator=g)
    an, bn = a.numpy(), b.numpy()
    assert np.array_equal((a / 255.0).numpy(), an / np.float32(255))
    assert np.array_equal((a * b - 0.5).numpy(), an * bn - np.float32(0.5))
    assert np.array_equal((a * b + b * a).numpy(), an * bn + bn * an)
    assert np.array_equal((torch.tensor(37.0) / a.clamp_min(1)).numpy(), np.float32(37) / np.maximum(an, np.float32(1)))


def test_model_equals_a_scalar_restatement_of_the_kernel():
    """model_f32 (vectorised) against the kernel's lines written out pixel by pixel on numpy float32 scalars"""
    f32 = np.float32
    for c in (ic._dec("f32", 2, 1, 16, "up_bottomright", 1, "randint"), ic._dec("f32", 2, 2, 16, "down_interior", 0, "ramp"),
              ic._dec("f32", 2, 1, 16, "up_topleft", 0, "checker")):
        p = ic.make_dec_problem(c)
        fr, prm = p["frames"].numpy(), p["params"].tolist()
        H0, W0 = ic.geom_frame(c.geom, c.crop)
        want = np.zeros((c.B, 3, c.T, c.crop, c.crop), dtype=f32)

        def coord(scale, d, size):
            f = scale * (f32(d) + f32(0.5)) - f32(0.5)
            f = f32(0) if f < 0 else f
            i0 = int(f)
            l1 = f - f32(i0)
            return i0, i0 + (1 if i0 < size - 1 else 0), f32(1) - l1, l1
        for b, (nh, nw, yo, xo, flip) in enumerate(prm):
            sy, sx = f32(H0) / f32(nh), f32(W0) / f32(nw)
            for y in range(c.crop):
                y0, y1, ly0, ly1 = coord(sy, y + yo, H0)
                for x in range(c.crop):
                    x0, x1, lx0, lx1 = coord(sx, (c.crop - 1 - x if flip else x) + xo, W0)
                    for t in range(c.T):
                        for ch in range(3):
                            a = [f32(fr[b, t, yy, xx, ch]) for yy in (y0, y1) for xx in (x0, x1)]
                            v = ly0 * (lx0 * a[0] + lx1 * a[1]) + ly1 * (lx0 * a[2] + lx1 * a[3])
                            want[b, ch, t, y, x] = (v / f32(255) - f32(ic.MEAN[ch])) * (f32(1) / f32(ic.STD[ch]))
        bad = _failed(ic.bits_equal("model", ic.model_f32(p["frames"], p["params"], c.crop), torch.from_numpy(want)))
        assert not bad, ic.dec_case_id(c) + "\n" + ic.report(bad)


def test_row_layouts_agree():
    g = ic._gen("layout")
    for shape in ((2, 3, 3, 32, 32), (2, 3, 2, 32, 48), (1, 3, 3, 48, 16)):
        x = torch.randn(*shape, generator=g)
        B, _, T, H, W = shape
        assert torch.equal(ic.patchify_rows(x), orc.patch_rows(x))
        assert torch.equal(ic.unpatch_rows(orc.patch_rows(x), B, T, H // 16, W // 16), x)


def test_fma32_is_the_exactly_rounded_fma():
    g = ic._gen("fma")
    a, b = torch.randn(2000, generator=g), torch.randn(2000, generator=g)
    c = -(a * b) + torch.randn(2000, generator=g) * 1e-7            # heavy cancellation: the sum needs more than 53 bits
    got = ic.fma32(a, b, c)
    Fr = fractions.Fraction
    for i in range(0, 2000, 7):
        exact = Fr(float(a[i])) * Fr(float(b[i])) + Fr(float(c[i]))
        lo = np.float32(float(exact))           # float(Fraction) rounds once to fp64; settle the fp32 neighbour exactly
        cand = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        dist = [abs(Fr(float(v)) - exact) for v in cand]
        best = [v for v, d in zip(cand, dist) if d == min(dist)]
        if len(best) == 2:                      # a tie goes to the even mantissa
            best = [v for v in best if int(np.float32(v).view(np.int32)) % 2 == 0]
        assert float(got[i]) == float(best[0]), (i, float(got[i]), float(best[0]))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the model is close to the reference's order of operations
# ---------------------------------------------------------------------------------------------------------------------
def test_model_against_the_reference_order_in_fp64():
    worst, n16, ndiff, where = 0.0, 0, {torch.float16: 0, torch.bfloat16: 0}, ""
    seen = set()
    for c in SMALL:
        for regime in ic.REGIMES:
            key = (c.geom, c.crop, c.B, c.T, c.flip, c.src, regime)
            if key in seen:
                continue
            seen.add(key)
            p = ic.make_dec_problem(c._replace(regime=regime))
            mod = ic.model_f32(p["frames"], p["params"], c.crop, p["src"])
            ref = ic.reference_f64(p["frames"], p["params"], c.crop, p["src"])
            mean = torch.tensor(ic.MEAN, dtype=torch.float32).double()
            unit = 2.0 ** -24 * float((p["frames"].double() / 255.0 - mean).abs().max()) / min(ic.STD)
            e = float((mod.double() - ref).abs().max()) / unit
            if e > worst:
                worst, where = e, f"{ic.dec_case_id(c)} / {regime}"
            n16 += mod.numel()
            for dt in ndiff:
                ndiff[dt] += int((mod.to(dt) != ref.to(dt)).sum())
    frac = {dt: ndiff[dt] / n16 for dt in ndiff}
    print(f"\nkernel-order model against the fp64 reference order, {len(seen)} geometry x regime problems, {n16} values:")
    print(f"  worst per-pixel error {worst:.3f} x 2^-24 max|x / 255 - mean| / min(std)   ({where})   [recorded {ic.MODEL_ERR_UNITS}]")
    for dt, v in frac.items():
        print(f"  fraction of R16(model) != R16(reference), {dt}: {v:.3e}   [recorded {ic.MODEL_FRAC16[dt]:.3e}]")
    assert worst <= 2 * ic.MODEL_ERR_UNITS
    for dt, v in frac.items():
        assert v <= 2 * ic.MODEL_FRAC16[dt], dt


def test_fraction_bound_of_check_input_pipeline_is_twice_what_the_model_needs():
    """kernel_checks.check_input_pipeline allows 3e-3 of the 16-bit values to differ from its references (the recorded fixture, the oracle on
    a batch of 5): on those very inputs the kernel-order model, to which the kernels are bit-equal, differs on at most 1.45e-3 of them"""
    import os
    from procedurevrl_amd.transform import spatial_sampling_params
    gold = torch.load(os.path.join(os.path.dirname(__file__), "golden", "input_pipeline.pt"), weights_only=False)
    probs = []
    for c in gold["cases"]:
        np.random.seed(c["seed"])
        prm = spatial_sampling_params(c["H0"], c["W0"], c["spatial_idx"], c["min_scale"], c["max_scale"], c["crop"], c["flip"], c["inv"])
        probs.append((c["frames"].unsqueeze(0), [prm], c["crop"], gold["mean"], gold["std"], c["out"].unsqueeze(0)))
    g = torch.Generator().manual_seed(5)
    B, T, H0, W0, crop = 5, 3, 72, 100, 64
    fr = torch.randint(0, 256, (B, T, H0, W0, 3), generator=g, dtype=torch.uint8)
    np.random.seed(11)
    prms = [spatial_sampling_params(H0, W0, -1, 64, 96, crop) for _ in range(B)]
    probs.append((fr, prms, crop, ic.MEAN, ic.STD, torch.stack([orc.input_pipeline(fr[b], prms[b], list(ic.MEAN), list(ic.STD), crop) for b in range(B)])))
    worst = 0.0
    for frames, prm, crop, mean, std, ref in probs:
        mod = ic.model_f32(frames, torch.tensor(prm, dtype=torch.int32), crop, mean=tuple(mean), std=tuple(std))
        assert float((mod - ref).norm() / ref.norm()) <= 1e-6 / 1.5           # the fp32 clip's aggregate bound there, with room to spare
        for dt in (torch.float16, torch.bfloat16):
            worst = max(worst, float((mod.to(dt) != ref.to(dt)).float().mean()))
    print(f"\ncheck_input_pipeline's inputs: worst fraction of R16(model) != R16(reference) {worst:.3e}   [recorded 1.45e-3, bound there 3e-3]")
    assert 2 * worst <= 3e-3


def test_the_model_passes_its_own_rule_on_every_small_case():
    for c in SMALL:
        bad = _failed(ic.check_dec_case(c, run=ic.model_decoded()))
        assert not bad, ic.dec_case_id(c) + "\n" + ic.report(bad)
    for c in ic.PAT_CASES:
        if "below_cap" in c.path:
            bad = _failed(ic.check_pat_case(c, run=lambda c, x: (ic.patchify_rows(x.to(ic.BF)), [])))
            assert not bad, ic.pat_case_id(c) + "\n" + ic.report(bad)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the rule bites
# ---------------------------------------------------------------------------------------------------------------------
def _first_catch(defect):
    if defect == "grid_stride_one_pass":
        table = PAST
    elif defect == "views_read_slab_b":
        table = [c for c in SMALL if c.src is not None]
    else:
        table = SMALL
    for c in table:
        bad = _failed(ic.check_dec_case(c, run=ic.model_decoded(defect)))
        if bad:
            return c, bad
    return None, []


@pytest.mark.parametrize("defect", ic.DECODED_DEFECTS)
def test_planted_defect_in_the_pipeline_is_caught(defect):
    c, bad = _first_catch(defect)
    assert c is not None, f"{defect}: no case of the table fails"
    print(f"\n{defect}: caught by {ic.dec_case_id(c)}\n{ic.report(bad)}")
    assert any("first at (" in f.detail and "clips [" in f.detail for f in bad), "the finding does not name the clip, row and column"
    if defect == "grid_stride_one_pass":        # both entry points, each in its own thread order
        for c in PAST:
            assert _failed(ic.check_dec_case(c, run=ic.model_decoded(defect))), ic.dec_case_id(c)


def test_planted_defect_reaches_no_case_it_should_not():
    """the clamp defects change nothing where no clamp is taken: the labels mean what they say"""
    for defect, label in (("x1_unclamped", "x1_clamped"), ("y1_unclamped", "y1_clamped"), ("negative_clamp_dropped", "negative_coordinate_clamped")):
        for c in SMALL:
            caught = bool(_failed(ic.check_dec_case(c, run=ic.model_decoded(defect))))
            assert not caught or label in c.path.split("."), f"{defect} caught by {ic.dec_case_id(c)}, which does not claim {label}"


@pytest.mark.parametrize("defect", ("patchify_PH_PW_swapped", "grid_stride_one_pass"))
def test_planted_defect_in_patchify_is_caught(defect):
    caught = []
    for c in ic.PAT_CASES:
        if (defect == "grid_stride_one_pass") != ("past_the_8192_workgroup_cap" in c.path):
            continue
        bad = _failed(ic.check_pat_case(c, run=lambda c, x: (ic.patchify_rows(x.to(ic.BF), defect), [])))
        if bad:
            caught.append((c, bad))
        elif defect == "patchify_PH_PW_swapped":
            assert c.HI == c.WI, f"PH / PW swapped passes {ic.pat_case_id(c)}"
    assert caught, f"{defect}: no case fails"
    print(f"\n{defect}: caught by {', '.join(ic.pat_case_id(c) for c, _ in caught[:3])}{' ..' if len(caught) > 3 else ''}\n{ic.report(caught[0][1])}")
    assert all("first at (" in f.detail for _, bad in caught for f in bad)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the table holds what it claims
# ---------------------------------------------------------------------------------------------------------------------
def test_case_table():
    ids = ([ic.dec_case_id(c) for c in ic.DEC_CASES] + [ic.pat_case_id(c) for c in ic.PAT_CASES] + [ic.ct_case_id(c) for c in ic.CT_CASES]
           + [ic.r1_case_id(c) for c in ic.R1_CASES] + [ic.bat_case_id(c) for c in ic.BAT_CASES] + [ic.cwm_case_id(c) for c in ic.CWM_CASES])
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    for entry in ("patchify", "f32"):
        mine = [c for c in ic.DEC_CASES if c.entry == entry]
        have = set().union(*(c.path.split(".") for c in mine))
        want = set(ic.DEC_LABELS) - ({"crop_x4_not_x16"} if entry == "patchify" else {"pad_columns"})
        assert want <= have, (entry, sorted(want - have))
        for c in mine:
            assert c.path == ic.dec_path(c)             # derived, not written by hand
            H0, W0 = ic.geom_frame(c.geom, c.crop)
            for (nh, nw, yo, xo, fl) in ic.dec_params(c).tolist():
                assert 0 <= yo and yo + c.crop <= nh and 0 <= xo and xo + c.crop <= nw and fl in (0, 1)
        for geom in ic.GEOMS:                           # every geometry with flip 0 / 1 and T 1 / 3
            assert {(c.flip, c.T) for c in mine if c.geom == geom and c.src is None} >= {(0, 1), (0, 3), (1, 1), (1, 3)}, geom
        assert {c.B for c in mine} >= {1, 5} and {c.crop for c in mine} >= {16, 32, 48} | ({20} if entry == "f32" else set())
        assert {c.regime for c in mine} == set(ic.REGIMES)
        if entry == "patchify":
            assert {c.ldo for c in mine} == {768, 776}
        past = [c for c in mine if "past_the_8192_workgroup_cap" in c.path]
        assert len(past) == 1 and 0 < ic.dec_threads(past[0]) - 8192 * 256 <= ic.dec_threads(past[0]) // past[0].B
        assert any(c.B == past[0].B - 1 and "below_cap" in c.path and c._replace(B=past[0].B, path="") == past[0]._replace(path="") for c in mine)
    have = set().union(*(c.path.split(".") for c in ic.PAT_CASES))
    assert set(ic.PAT_LABELS) <= have
    assert {(c.HI, c.WI, c.T, c.B, c.ldo) for c in ic.PAT_CASES} >= {(h, w, t, b, l) for (h, w) in ((32, 48), (48, 16)) for t in (1, 3) for b in (1, 2) for l in (768, 776)}
    past = [c for c in ic.PAT_CASES if "past_the_8192_workgroup_cap" in c.path]
    assert len(past) == 1 and 0 < past[0].B * 3 * past[0].T * past[0].HI * (past[0].WI // 8) - 8192 * 256 <= 3 * past[0].T * past[0].HI * (past[0].WI // 8)
    assert set(ic.R1_LABELS) <= set().union(*(c.path.split(".") for c in ic.R1_CASES))
    assert {c.n for c in ic.BAT_CASES if c.entry == "gemv"} == {1, 16, 17, 33} == {c.n for c in ic.BAT_CASES if c.entry == "rank1"}
    assert all(c.R % 4 for c in ic.BAT_CASES if c.entry == "gemv") and {c.opt for c in ic.BAT_CASES if c.entry == "gemv"} == {"32", "16"}
    assert ic.cwm_path("seam_96_then_ragged") == "tile64+tile32" and ic.cwm_path("out_offset_4_bytes") == "tile32"
    assert set(ic.CT_CASES) == {(1, 1), (31, 33), (32, 32), (33, 65), (300, 130)}


def test_check_decoded_raises_from_the_host_copies():
    bad = _failed(ic.check_decoded_validation("cpu"))
    assert not bad, ic.report(bad)
