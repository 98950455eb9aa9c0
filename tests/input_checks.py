"""The input pipeline and the layout kernels of csrc/elementwise.hip -- pvrl_frames_u8_patchify / _to_f32 and their _views forms,
pvrl_patchify, pvrl_cast_transpose_bf16, pvrl_rank1_add_f32, and the chunk seams of the batched gemv / rank-1 / weight-cast entry
points -- PER PIXEL, bit for bit, on every path, inside guard bands.

Used by tests/test_input_kernels_gpu.py (pytest -m gpu: the HIP kernels through the C ABI / procedurevrl_amd.ops) and by
tests/test_input_harness_host.py (no GPU: the CPU models stand in for the kernels, planted defects show that the rule bites).
Guard bands, findings and the bit comparisons are those of tests/attn_checks.py and tests/row_checks.py.

No tolerance anywhere.  The contracts:
  frames_u8_to_f32      every element bit-equal to `model_f32`, the kernel-order fp32 model: one rounding per operation in the order of
                        u8_src_coord / u8_pixel (scale = f32(H0) / f32(new); f = scale * (f32(d) + 0.5) - 0.5; clamp at 0; i0 = trunc(f);
                        i1 = i0 + (i0 < size - 1); l1 = f - i0; l0 = 1 - l1; v = ly0 * (lx0 a00 + lx1 a01) + ly1 * (lx0 a10 + lx1 a11);
                        (v / 255 - mean) * (1 / std)), flip x -> (crop - 1 - x) + x_off, interleaved RGB
  frames_u8_patchify    bit-equal to R16(model) laid out by oracle.patch_rows, ldo 768 and 776, pads and guards untouched
  _views                bit-equal to the plain form on frames[src] (repeats, descending, S > B, S < B, S == 1)
  identity scale        additionally (u8 / 255 - mean) * istd gathered directly (l1 is exactly 0)
  patchify              bit-equal to R16(frames) permuted into (b, n, t) x (c, py, px) (`patchify_rows`, index arithmetic of its own)
  cast_transpose        bit-equal to R16(w).t()
  rank1_add (_batched)  every element one of fl(out + fl(a' b)) and fma(a', b, out), a' = fl(a gscale); outside [:R, :C] untouched
  batched forms         gemv_rows_batched / rank1_add_batched bit-equal per item to the one-item entry point, n = 1, 16, 17, 33
  cast_weights_multi    bit-equal to R16(w) and R16(w).t() across the 96-item seam and on the 32-tile fall-back of an offset `out`
  refusals              PVRL_EINVAL and nothing written; B == 0 returns OK and writes nothing (tests/test_cabi.py asserts none of these)

Bit equality with the kernel-order model on the GPU holds on every case of the table, in both operand flavours.  The compiled kernels (hipcc -S, both operand flavours) hold
no contracted multiply-add in the pipeline's arithmetic: every v_fma_f32 / v_fmac_f32 of the two kernels belongs to one of the 29 (8
pixels x 3 channels of v / 255, 3 of 1 / std, 2 scales; 9 in the fp32 form) v_div_scale / v_rcp / v_div_fmas / v_div_fixup sequences,
the correctly rounded fp32 division, or to the integer divisions of the index decode; the 16-bit store is v_cvt_pk_*_f32 of the fp32
result.  The model was written from the source and has not been changed to reproduce the kernel; no kernel needed a fix.

The model against the reference's order of operations (normalise, bilinear with align_corners=False, crop, flip, in fp64:
`reference_f64`), measured on the CPU over the whole geometry table x every content regime (pytest tests/test_input_harness_host.py -s
prints these; they are asserted at twice the value):
  195 geometry x regime problems, 3.9e6 values
  worst per-pixel error      333.7 x 2^-24 max|x / 255 - mean| / min(std)   (`checker`, 101x149 -> crop 48 down-scale: the fp32 source
                             coordinate near 140 carries an error of 2^-17, and a 0 / 255 neighbour pair turns all of it into the value)
  R16(model) != R16(reference)   fp16 7.34e-3, bf16 2.03e-3 of the values   (MODEL_ERR_UNITS, MODEL_FRAC16 below)

Planted defects (the model with the defect stands in for the kernel) and the first case of the table that caught each:
  source coordinate computed with an fma        frames_u8_patchify-B5-T3-69x101-crop32-down_interior-flip0-checker (17 pixels of 3 clips)
  x1 not clamped at W0 - 1, y1 at H0 - 1        frames_u8_patchify-B1-T1-27x30-crop48-up_bottomright-flip0-ramp (column 47 / row 47); caught by
                                                no case without the label x1_clamped / y1_clamped
  negative-coordinate clamp dropped             frames_u8_patchify-B5-T1-19x22-crop32-up_topleft-flip0-checker; by no case without its label
  flip about the rescaled frame's width         frames_u8_patchify-B5-T3-69x101-crop32-down_interior-flip0-checker (the flipped clips 1 and 3)
  x_off and y_off swapped                       frames_u8_patchify-B1-T1-37x53-crop16-down_interior-flip0-randint
  mean / std channel order reversed             the same case (channels 0 and 2)
  _views form reads slab b instead of src[b]    frames_u8_patchify_views-B5-T3-19x22-crop32-up_bottomright-flip0-randint-S3-src00221 (clips 1, 3)
  clip b takes the params of clip b - 1         frames_u8_patchify-B5-T3-69x101-crop32-down_interior-flip0-checker
  grid-stride loop makes one pass only          frames_u8_patchify-B16385 and frames_u8_to_f32-B2731 (..-past_the_8192_workgroup_cap), patchify-B3641
  normalise-then-interpolate (the oracle)       frames_u8_patchify-B1-T1-37x53-crop16-down_interior-flip0-randint: the contract is sharper than
                                                the aggregate tolerances of kernel_checks.check_input_pipeline, which the oracle passes by definition
  PH and PW swapped in patchify's row index     every patchify case with HI != WI (first: patchify-B1-T1-32x48-ldo768); the square case passes
"""
import collections
import ctypes
import itertools

import numpy as np
import torch
import torch.nn.functional as F

from attn_checks import Finding, report, Guarded, guarded_input, PATTERN  # noqa: F401
from row_checks import bits_equal, bits_among, untouched, _gen, _abi, BF, F32, OPERAND, GRID_CAP  # noqa: F401
from oracle import timesformer_oracle as orc

MEAN, STD = (0.45, 0.40, 0.5), (0.225, 0.25, 0.2)          # differ per channel: a channel swap shows
REGIMES = ("randint", "checker", "ramp")
SMALL_BATCH_MAX, CAST_MULTI_MAX = 16, 96                   # elementwise.hip
I64 = torch.int64

# recorded by tests/test_input_harness_host.py -s (asserted there at twice these values)
MODEL_ERR_UNITS = 334.0            # worst |model - reference|, in units of 2^-24 * max|x / 255 - mean| / min(std)
MODEL_FRAC16 = {torch.float16: 7.34e-3, torch.bfloat16: 2.04e-3}   # fraction of R16(model) != R16(reference)


def grid_threads(total):
    """grid_for of elementwise.hip: threads of the launched grid for `total` work items"""
    return min(max(-(-total // 256), 1), 8192) * 256


def grid_label(total):
    return "past_the_8192_workgroup_cap" if total > grid_threads(total) else "below_cap"


# =====================================================================================================================
# decoded clips: content, geometry, models
# =====================================================================================================================
def make_frames(regime, S, T, H0, W0, key):
    """uint8 [S, T, H0, W0, 3]; every clip and time step differs"""
    if regime == "randint":
        return torch.randint(0, 256, (S, T, H0, W0, 3), generator=_gen("frames", key), dtype=torch.uint8)
    s, t, y, x, c = torch.meshgrid(*(torch.arange(n) for n in (S, T, H0, W0, 3)), indexing="ij")
    if regime == "checker":             # 0 / 255 alternating per pixel: the worst cancellation in the blend
        return (((x + y + c + t + s) % 2) * 255).to(torch.uint8)
    return ((7 * x + 13 * y + 101 * c + 31 * t + 57 * s) % 256).to(torch.uint8)          # ramp: every neighbour differs


GEOMS = ("down_interior", "up_topleft", "up_bottomright", "identity", "anisotropic", "H0_is_1", "W0_is_1")


def geom_frame(geom, c):
    """(H0, W0) of the source frame for crop c: odd sizes, 3 * W0 no multiple of 4 where the geometry leaves the choice"""
    return {"down_interior": (2 * c + 5, 3 * c + 5), "up_topleft": (c // 2 + 3, c // 2 + 6), "up_bottomright": (c // 2 + 3, c // 2 + 6),
            "identity": (c + 7, c + 9), "anisotropic": (2 * c + 3, c // 2 + 5), "H0_is_1": (1, c + 9), "W0_is_1": (c + 9, 1)}[geom]


def geom_params(geom, c, b, flip):
    """(new_h, new_w, y_off, x_off, flip) of clip b: the draws differ per clip; odd clips take the other flip"""
    H0, W0 = geom_frame(geom, c)
    k = b % 5
    if geom == "down_interior":
        q = (c + 2 + k, c + 8 + 2 * k, 1, 2 + k)
    elif geom == "up_topleft":
        q = (2 * H0 + k, 2 * W0 + 1 + k, 0, 0)
    elif geom == "up_bottomright":
        q = (2 * H0 + k, 2 * W0 + 1 + k, 2 * H0 + k - c, 2 * W0 + 1 + k - c)
    elif geom == "identity":
        q = (H0, W0, 1 + k, 2 + k)
    elif geom == "anisotropic":
        q = (c + 4 + k, 2 * c + k, 2, 3 + k)
    elif geom == "H0_is_1":
        q = (c + 2 + k, W0 + 3 + k, 1, 2)
    else:
        q = (H0 + 3 + k, c + 2 + k, 2, 1)
    return q + ((flip + b) % 2,)


def _coords(scale, d, size, defect=None, axis="x"):
    """u8_src_coord and the neighbour / weight lines of the two kernels: scale fp32 [n], d int64 [n, crop] -> i0, i1 (int64), l0, l1 (fp32)"""
    df = d.to(F32) + 0.5
    if defect == "coord_fma":           # the product of two fp32 values is exact in fp64
        f = (scale.double()[:, None] * df.double() - 0.5).to(F32)
    else:
        f = scale[:, None] * df - 0.5
    if defect != "negative_clamp_dropped":
        f = torch.where(f < 0, torch.zeros_like(f), f)
    i0 = f.to(I64)                      # (int)f: towards zero
    i1 = i0 + (1 if defect == axis + "1_unclamped" else (i0 < size - 1).to(I64))
    l1 = f - i0.to(F32)
    return i0, i1, 1.0 - l1, l1


DECODED_DEFECTS = ("coord_fma", "x1_unclamped", "y1_unclamped", "negative_clamp_dropped", "flip_about_rescaled_width", "offsets_swapped",
                   "mean_std_reversed", "views_read_slab_b", "params_of_previous_clip", "grid_stride_one_pass", "oracle_order")


def model_f32(frames, params, crop, src=None, defect=None, chunk=1024, mean=MEAN, std=STD):
    """the kernel-order fp32 model (module docstring), vectorised over clips.  frames uint8 [S, T, H0, W0, 3], params [B, 5], src [B] or
    None -> fp32 [B, 3, T, crop, crop].  The gather addresses memory as the kernels do (pixel ((slab T + t) H0 + y) W0 + x of the flat
    buffer), so a defect that leaves the row or the slab reads what the kernel would read."""
    S, T, H0, W0, _ = frames.shape
    B = params.shape[0]
    if defect == "oracle_order":
        sb = torch.arange(B) if src is None else src.to(I64)
        return torch.stack([orc.input_pipeline(frames[int(sb[b])], params[b].tolist(), MEAN, STD, crop) for b in range(B)])
    prm = params.to(I64)
    if defect == "params_of_previous_clip":
        prm = prm.roll(1, 0)
    sb_all = torch.arange(B) if src is None else src.to(I64)
    if defect == "views_read_slab_b":
        sb_all = torch.arange(B) % S
    pix = torch.cat([frames.reshape(-1, 3), torch.zeros(W0 + 2, 3, dtype=torch.uint8)])
    mean, istd = torch.tensor(mean, dtype=F32), 1.0 / torch.tensor(std, dtype=F32)
    if defect == "mean_std_reversed":
        mean, istd = mean.flip(0), istd.flip(0)
    out = torch.empty(B, 3, T, crop, crop)
    ar, tt = torch.arange(crop)[None], torch.arange(T)[None]
    for b0 in range(0, B, chunk):
        nh, nw, yo, xo, fl = prm[b0:b0 + chunk].unbind(1)
        if defect == "offsets_swapped":
            yo, xo = xo, yo
        sy, sx = torch.tensor(float(H0)) / nh.to(F32), torch.tensor(float(W0)) / nw.to(F32)
        X = torch.where(fl[:, None] != 0, crop - 1 - ar, ar) + xo[:, None]
        if defect == "flip_about_rescaled_width":
            X = torch.where(fl[:, None] != 0, nw[:, None] - 1 - (ar + xo[:, None]), X)
        y0, y1, ly0, ly1 = _coords(sy, ar + yo[:, None], H0, defect, "y")
        x0, x1, lx0, lx1 = _coords(sx, X, W0, defect, "x")
        rowbase = (sb_all[b0:b0 + chunk, None] * T + tt) * H0                       # [n, T]

        def tap(yy, xx):
            idx = (rowbase[:, :, None] + yy[:, None, :])[..., None] * W0 + xx[:, None, None, :]
            return pix[idx.clamp(0, pix.shape[0] - 1)].to(F32)                       # [n, T, crop, crop, 3]
        LY0, LY1 = ly0[:, None, :, None, None], ly1[:, None, :, None, None]
        LX0, LX1 = lx0[:, None, None, :, None], lx1[:, None, None, :, None]
        v = LY0 * (LX0 * tap(y0, x0) + LX1 * tap(y0, x1)) + LY1 * (LX0 * tap(y1, x0) + LX1 * tap(y1, x1))
        out[b0:b0 + chunk] = ((v / 255.0 - mean) * istd).permute(0, 4, 1, 2, 3)
    if defect == "grid_stride_one_pass":             # thread idx of frames_u8_to_f32_kernel writes elements 4 idx .. 4 idx + 3
        out.view(-1)[grid_threads(out.numel() // 4) * 4:] = float("nan")
    return out


def one_pass_mask_patchify(B, T, crop):
    """[B, 1, T, crop, crop] bool: pixels whose thread of frames_u8_patchify_kernel ((b, t, y, x8), all three channels) lies in the first pass"""
    b, t, y, x = torch.meshgrid(torch.arange(B), torch.arange(T), torch.arange(crop), torch.arange(crop), indexing="ij")
    idx = ((b * T + t) * crop + y) * (crop // 8) + x // 8
    return (idx < grid_threads(B * T * crop * (crop // 8)))[:, None]


def reference_f64(frames, params, crop, src=None):
    """the reference's chain in its own order (oracle.timesformer_oracle.input_pipeline), in fp64, from the fp32 mean / std the kernel is given"""
    B = params.shape[0]
    mean, std = torch.tensor(MEAN, dtype=F32).double(), torch.tensor(STD, dtype=F32).double()
    out = []
    for b in range(B):
        nh, nw, yo, xo, flip = params[b].tolist()
        x = ((frames[b if src is None else int(src[b])].double() / 255.0 - mean) / std).permute(3, 0, 1, 2)
        if (nh, nw) != tuple(x.shape[2:]):
            x = F.interpolate(x, size=(nh, nw), mode="bilinear", align_corners=False)
        x = x[:, :, yo:yo + crop, xo:xo + crop]
        out.append(x.flip(-1) if flip else x)
    return torch.stack(out)


def identity_gather(frames, params, crop, src=None):
    """identity scale: (u8 / 255 - mean) * istd gathered directly, no interpolation"""
    mean, istd = torch.tensor(MEAN, dtype=F32), 1.0 / torch.tensor(STD, dtype=F32)
    out = []
    for b in range(params.shape[0]):
        _, _, yo, xo, flip = params[b].tolist()
        x = ((frames[b if src is None else int(src[b])].to(F32) / 255.0 - mean) * istd)[:, yo:yo + crop, xo:xo + crop].permute(3, 0, 1, 2)
        out.append(x.flip(-1) if flip else x)
    return torch.stack(out)


def unpatch_rows(rows, B, T, PH, PW):
    """inverse of oracle.patch_rows: [(b, n, t), (c, py, px)] -> [B, 3, T, 16 PH, 16 PW]"""
    return rows.reshape(B, PH, PW, T, 3, 16, 16).permute(0, 4, 3, 1, 5, 2, 6).reshape(B, 3, T, 16 * PH, 16 * PW)


def patchify_rows(x, defect=None):
    """pvrl_patchify's layout by index arithmetic of its own (not a reshape): x [B, 3, T, HI, WI] -> [(b, n, t), 768] with
    n = (y >> 4) PW + (x >> 4), row = (b PH PW + n) T + t, column = c 256 + (y & 15) 16 + (x & 15); rows nobody wrote hold NaN"""
    B, _, T, HI, WI = x.shape
    PH, PW = HI // 16, WI // 16
    rows = B * PH * PW * T
    ar = torch.arange
    nmul = PH if defect == "patchify_PH_PW_swapped" else PW
    flat = ((ar(B) * PH * PW * T * 768)[:, None, None, None, None] + (ar(3) * 256)[None, :, None, None, None]
            + (ar(T) * 768)[None, None, :, None, None] + ((ar(HI) >> 4) * nmul * T * 768 + (ar(HI) & 15) * 16)[None, None, None, :, None]
            + ((ar(WI) >> 4) * T * 768 + (ar(WI) & 15))[None, None, None, None, :]).reshape(-1)
    vals = x.reshape(-1)
    if defect == "grid_stride_one_pass":             # thread idx of patchify_kernel reads elements 8 idx .. 8 idx + 7
        n = grid_threads(x.numel() // 8) * 8
        flat, vals = flat[:n], vals[:n]
    keep = flat < rows * 768
    out = torch.full((rows * 768,), float("nan"), dtype=x.dtype)
    out[flat[keep]] = vals[keep]
    return out.reshape(rows, 768)


# ---------------------------------------------------------------------------------------------------------------------
# the case table of the decoded-clip entry points
# ---------------------------------------------------------------------------------------------------------------------
DecCase = collections.namedtuple("DecCase", "entry B T crop geom flip regime ldo src S path")
# entry "patchify" (pvrl_frames_u8_patchify) / "f32" (pvrl_frames_u8_to_f32); src: None or the tuple of slab indices of the _views form, S slabs
VIEWS = {"repeats": ((0, 0, 2, 2, 1), 3), "descending": ((4, 3, 2, 1, 0), 5), "unnamed_slabs": ((6, 1, 3), 7), "fewer_slabs": ((1, 0, 1, 1, 0), 2),
         "one_slab": ((0, 0, 0, 0), 1)}


def dec_params(c):
    return torch.tensor([geom_params(c.geom, c.crop, b, c.flip) for b in range(c.B)], dtype=torch.int32)


def _edge(size, new, off, crop):
    """the clamp conditions restated on scalars: (a negative source coordinate occurs, the last neighbour index is clamped at size - 1)"""
    f32 = np.float32
    s = f32(size) / f32(new)
    first, last = s * (f32(off) + f32(0.5)) - f32(0.5), s * (f32(off + crop - 1) + f32(0.5)) - f32(0.5)
    return bool(first < 0), int(max(last, f32(0))) >= size - 1


def dec_threads(c):
    return c.B * c.T * c.crop * (c.crop // 8) if c.entry == "patchify" else c.B * 3 * c.T * c.crop * (c.crop // 4)


def dec_path(c):
    """the path labels of a case, from its shape alone"""
    H0, W0 = geom_frame(c.geom, c.crop)
    lab = set()
    for (nh, nw, yo, xo, _) in dec_params(c).tolist():
        ny, cy = _edge(H0, nh, yo, c.crop)
        nx, cx = _edge(W0, nw, xo, c.crop)
        lab |= {"negative_coordinate_clamped"} if (ny or nx) else set()
        lab |= {"y1_clamped"} if cy else set()
        lab |= {"x1_clamped"} if cx else set()
        lab.add("identity_scale" if (nh, nw) == (H0, W0) else "anisotropic" if (nh - H0) * (nw - W0) < 0 else
                "down_scale" if nh < H0 else "up_scale")
    lab |= {"H0_is_1"} if H0 == 1 else set()
    lab |= {"W0_is_1"} if W0 == 1 else set()
    lab |= {"row_bytes_not_x4"} if (3 * W0) % 4 else set()
    lab.add({1: "one_patch"}.get(c.crop // 16, "odd_patch_grid" if (c.crop // 16) % 2 else "even_patch_grid") if c.crop % 16 == 0
            else "crop_x4_not_x16")
    lab |= {"pad_columns"} if c.ldo > 768 else set()
    if c.src is not None:
        lab.add("views")
        lab |= {"src_repeats"} if len(set(c.src)) < len(c.src) else set()
        lab |= {"src_descending"} if all(a > b for a, b in zip(c.src, c.src[1:])) else set()
        lab.add("one_slab" if c.S == 1 else "slabs_nobody_names" if c.S > len(set(c.src)) and c.S > c.B else "S_below_B" if c.S < c.B else "S_is_B")
    return ".".join(sorted(lab)) + "." + grid_label(dec_threads(c))


def dec_case_id(c):
    H0, W0 = geom_frame(c.geom, c.crop)
    s = f"frames_u8_{'patchify' if c.entry == 'patchify' else 'to_f32'}{'_views' if c.src is not None else ''}-B{c.B}-T{c.T}-{H0}x{W0}-crop{c.crop}"
    s += f"-{c.geom}-flip{c.flip}-{c.regime}" + (f"-ldo{c.ldo}" if c.entry == "patchify" else "")
    return s + (f"-S{c.S}-src{''.join(str(v) for v in c.src)}" if c.src is not None else "") + "-" + c.path


def _dec(entry, B, T, crop, geom, flip, regime, ldo=768, src=None, S=None):
    c = DecCase(entry, B, T, crop, geom, flip, regime, ldo if entry == "patchify" else 0, src, S, "")
    return c._replace(path=dec_path(c))


def _build_dec_cases():
    cases = []
    for entry, crops in (("patchify", (16, 32, 48)), ("f32", (16, 20, 32, 48))):
        for gi, geom in enumerate(GEOMS):       # every geometry with flip 0 / 1 and T 1 / 3; crop, B, regime and ldo rotate over them
            for k, (flip, T) in enumerate(itertools.product((0, 1), (1, 3))):
                cases.append(_dec(entry, (1, 5)[(gi + k // 2 + k) % 2], T, crops[(gi + k) % len(crops)], geom, flip, REGIMES[(gi + k) % 3], (768, 776)[(gi + k // 2) % 2]))
        for vi, (src, S) in enumerate(VIEWS.values()):
            cases.append(_dec(entry, len(src), (3, 1)[vi % 2], (32, 16, 48)[vi % 3] if entry == "patchify" else (20, 32, 16)[vi % 3],
                              ("up_bottomright", "down_interior", "anisotropic")[vi % 3], vi % 2, REGIMES[vi % 3], (776, 768)[vi % 2], src, S))
        per_clip = dec_threads(_dec(entry, 1, 1, 32, "up_bottomright", 0, "randint"))
        for B in (GRID_CAP // per_clip, GRID_CAP // per_clip + 1):      # the last B of one pass and the first B of a grid-stride second pass
            cases.append(_dec(entry, B, 1, 32, "up_bottomright", 1, "randint"))
    return cases


DEC_CASES = _build_dec_cases()
DEC_LABELS = ("negative_coordinate_clamped", "y1_clamped", "x1_clamped", "identity_scale", "anisotropic", "down_scale", "up_scale", "H0_is_1",
              "W0_is_1", "row_bytes_not_x4", "one_patch", "odd_patch_grid", "even_patch_grid", "crop_x4_not_x16", "pad_columns", "views",
              "src_repeats", "src_descending", "one_slab", "slabs_nobody_names", "S_below_B", "past_the_8192_workgroup_cap", "below_cap")


def make_dec_problem(c):
    H0, W0 = geom_frame(c.geom, c.crop)
    S = c.B if c.src is None else c.S
    return dict(frames=make_frames(c.regime, S, c.T, H0, W0, (c.geom, c.crop, c.B, c.T)), params=dec_params(c),
                src=None if c.src is None else torch.tensor(c.src, dtype=torch.int32))


def _u8_device(frames, dev):
    """the frames followed by 4096 bytes of 255: a read past the end stays inside the allocation and shows in the numbers"""
    buf = torch.full((frames.numel() + 4096,), 255, dtype=torch.uint8)
    buf[:frames.numel()] = frames.reshape(-1)
    return buf.to(dev)[:frames.numel()].view(frames.shape)


def _f3(v):
    a = (ctypes.c_float * 3)(*v)
    return a, ctypes.cast(a, ctypes.c_void_p)


def _dec_call(entry, fr, prm, src, S, B, T, H0, W0, crop, out, ldo, mean=MEAN, std=STD):
    """one call of the C ABI -> None or the refusal's text"""
    from procedurevrl_amd._lib import PvrlError
    L, P, St, _ = _abi()
    (km, mean_p), (ks, std_p) = _f3(mean), _f3(std)
    name = "pvrl_frames_u8_patchify" if entry == "patchify" else "pvrl_frames_u8_to_f32"
    head = (P(fr), P(prm)) if src is None else (P(fr), P(prm), (P(src) if torch.is_tensor(src) else None), S)
    tail = (P(out), ldo, St()) if entry == "patchify" else (P(out), St())
    try:
        L.call(name + ("" if src is None else "_views"), *head, B, T, H0, W0, crop, mean_p, std_p, *tail)
    except PvrlError as e:
        return str(e)
    return None


def _dec_out(entry, name, B, T, crop, ldo, dev):
    if entry == "patchify":
        return Guarded(name, [B * (crop // 16) ** 2 * T], 768, BF, ldo - 768, device=dev)
    return Guarded(name, [B * 3 * T * crop], crop, F32, device=dev)


def gpu_decoded(c, p, dev):
    """the entry point of the case (and, for a _views case, the plain form on frames[src]) -> (dict(out, plain), findings)"""
    H0, W0 = geom_frame(c.geom, c.crop)
    fr, prm = _u8_device(p["frames"], dev), p["params"].to(dev)
    src = None if p["src"] is None else p["src"].to(dev)
    ob = _dec_out(c.entry, "out", c.B, c.T, c.crop, c.ldo, dev)
    msg = _dec_call(c.entry, fr, prm, src, c.S, c.B, c.T, H0, W0, c.crop, ob.seg(0), c.ldo)
    f = [Finding("status", msg is None, 0.0, 0.0, msg or "OK")]
    got = dict(out=ob, plain=None)
    if src is not None:
        pb = _dec_out(c.entry, "plain form on frames[src]", c.B, c.T, c.crop, c.ldo, dev)
        msg = _dec_call(c.entry, _u8_device(p["frames"][p["src"].to(I64)], dev), prm, None, 0, c.B, c.T, H0, W0, c.crop, pb.seg(0), c.ldo)
        f.append(Finding("status of the plain form", msg is None, 0.0, 0.0, msg or "OK"))
        got["plain"] = pb
    torch.cuda.synchronize()
    for k, g in list(got.items()):
        if g is not None:
            f += g.check()
            got[k] = g.seg(0).cpu()
    return got, f


def model_decoded(defect=None):
    """the model (with a planted defect) in the place of the kernels, for the host test"""
    def run(c, p):
        def form(x):
            if c.entry == "f32":
                return x.reshape(-1, c.crop)
            if defect == "grid_stride_one_pass":
                x = torch.where(one_pass_mask_patchify(c.B, c.T, c.crop), x, torch.full_like(x, float("nan")))
            return orc.patch_rows(x).to(BF)
        d = defect if not (defect == "grid_stride_one_pass" and c.entry == "patchify") else None
        out = form(model_f32(p["frames"], p["params"], c.crop, p["src"], d))
        plain = None if p["src"] is None else form(model_f32(p["frames"][p["src"].to(I64)], p["params"], c.crop))
        return dict(out=out, plain=plain), []
    return run


def localise(got, want):
    """where two [B, 3, T, crop, crop] tensors differ: clips, rows, columns -- whole rows / columns point at a coordinate, scattered pixels at a value"""
    idt = {2: torch.int16, 4: torch.int32}[got.element_size()]
    d = got.contiguous().view(idt) != want.contiguous().view(idt)
    if not bool(d.any()):
        return ""
    clips, rows, cols = (d.any(dim=tuple(a for a in range(5) if a != k)).nonzero().flatten().tolist() for k in (0, 3, 4))
    full_rows = int(d.all(dim=4).sum())
    full_cols = int(d.all(dim=3).sum())
    return (f"index = (clip, channel, time, row, column); clips {clips[:8]}, rows {rows[:8]} ({len(rows)}), columns {cols[:8]} ({len(cols)}); "
            f"{full_rows} whole rows and {full_cols} whole columns differ")


def check_dec_case(c, run=None):
    """one decoded-clip case -> [Finding]; run(c, p) -> (dict(out, plain), findings): the GPU by default"""
    if run is None:
        dev = torch.device("cuda:0")
        run = lambda c, p: gpu_decoded(c, p, dev)
    p = make_dec_problem(c)
    got, f = run(c, p)
    B, T, crop = c.B, c.T, c.crop
    as5 = (lambda r: unpatch_rows(r, B, T, crop // 16, crop // 16)) if c.entry == "patchify" else (lambda r: r.reshape(B, 3, T, crop, crop))
    r16 = (lambda x: x.to(BF)) if c.entry == "patchify" else (lambda x: x)
    want = r16(model_f32(p["frames"], p["params"], crop, p["src"]))
    out = as5(got["out"])
    f += bits_equal("out against the kernel-order model" + (", rounded to the operand type" if c.entry == "patchify" else ""), out, want, localise(out, want))
    if "identity_scale" in c.path:
        direct = r16(identity_gather(p["frames"], p["params"], crop, p["src"]))
        f += bits_equal("out against (u8 / 255 - mean) * istd gathered without interpolation", out, direct, localise(out, direct))
    if got["plain"] is not None:
        f += bits_equal("_views form against the plain form on frames[src]", out, as5(got["plain"]), localise(out, as5(got["plain"])))
    return f


# =====================================================================================================================
# pvrl_patchify
# =====================================================================================================================
PatCase = collections.namedtuple("PatCase", "B T HI WI ldo path")


def _pat(B, T, HI, WI, ldo=768):
    shape = "square" if HI == WI else "PH_above_PW" if HI > WI else "PW_above_PH"
    return PatCase(B, T, HI, WI, ldo, shape + (".pad_columns" if ldo > 768 else "") + "." + grid_label(B * 3 * T * HI * (WI // 8)))


_PAT_CAP_B = GRID_CAP // (3 * 32 * 6)
PAT_CASES = ([_pat(B, T, HI, WI, ldo) for (HI, WI) in ((32, 48), (48, 16)) for T in (1, 3) for B in (1, 2) for ldo in (768, 776)]
             + [_pat(2, 3, 32, 32), _pat(_PAT_CAP_B, 1, 32, 48), _pat(_PAT_CAP_B + 1, 1, 32, 48)])
PAT_LABELS = ("PH_above_PW", "PW_above_PH", "square", "pad_columns", "past_the_8192_workgroup_cap", "below_cap")


def pat_case_id(c):
    return f"patchify-B{c.B}-T{c.T}-{c.HI}x{c.WI}-ldo{c.ldo}-{c.path}"


def gpu_patchify(c, x, dev):
    L, P, St, ops = _abi()
    ob = Guarded("out", [c.B * (c.HI // 16) * (c.WI // 16) * c.T], 768, BF, c.ldo - 768, device=dev)
    buf = torch.full((x.numel() + 64,), 1000.0)
    buf[:x.numel()] = x.reshape(-1)
    ops.patchify(buf.to(dev)[:x.numel()].view(x.shape), out=ob.seg(0))
    torch.cuda.synchronize()
    return ob.seg(0).cpu(), ob.check()


def check_pat_case(c, run=None):
    if run is None:
        dev = torch.device("cuda:0")
        run = lambda c, x: gpu_patchify(c, x, dev)
    x = torch.randn(c.B, 3, c.T, c.HI, c.WI, generator=_gen("patchify", c.B, c.T, c.HI, c.WI)) * 3
    got, f = run(c, x)
    PH, PW = c.HI // 16, c.WI // 16
    got5, want5 = unpatch_rows(got, c.B, c.T, PH, PW), unpatch_rows(patchify_rows(x.to(BF)), c.B, c.T, PH, PW)
    return f + bits_equal("out against R16(frames) in (b, n, t) x (c, py, px) order", got5, want5, localise(got5, want5))


# =====================================================================================================================
# cast_transpose, rank1_add, the batched forms, cast_weights_multi
# =====================================================================================================================
CT_CASES = [(1, 1), (31, 33), (32, 32), (33, 65), (300, 130)]


def ct_case_id(s):
    R, C = s
    return f"cast_transpose-{R}x{C}-tiles{-(-C // 32)}x{-(-R // 32)}" + (".ragged" if R % 32 or C % 32 else ".full_tiles")


def check_ct_case(s):
    _, _, _, ops = _abi()
    dev = torch.device("cuda:0")
    R, C = s
    w = torch.randn(R, C, generator=_gen("ct", s))
    ob = Guarded("out", [C], R, BF, device=dev)
    ops.cast_transpose(guarded_input(w.reshape(1, -1), F32, dev, 64)[0].view(R, C), out=ob.seg(0))
    torch.cuda.synchronize()
    return ob.check() + bits_equal("out against R16(w).t(); index = (column of w, row of w)", ob.seg(0), w.t().to(BF))


def fma32(a, b, c):
    """fp32 fma, exactly: the product is exact in fp64, the fp64 sum is rounded to odd, so the rounding to fp32 is the only one"""
    p, c = a.double() * b.double(), c.double().expand_as(a.double() * b.double())
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                                                  # TwoSum: p + c = s + e exactly
    even = (s.contiguous().view(I64) & 1) == 0
    odd = torch.nextafter(s, torch.where(e > 0, torch.full_like(s, float("inf")), torch.full_like(s, float("-inf"))))
    return torch.where((e != 0) & even, odd, s).to(F32)


def rank1_candidates(out0, a, b, gs):
    a1 = (a * torch.tensor(gs, dtype=F32)) if gs is not None else a
    return [out0 + a1[:, None] * b[None, :], fma32(a1[:, None].expand(-1, b.numel()), b[None, :].expand(a.numel(), -1), out0)]


R1Case = collections.namedtuple("R1Case", "R C extra gs path")


def _r1(R, C, extra, gs):
    n = R * C // 4
    return R1Case(R, C, extra, gs, ("full_workgroups" if n % 256 == 0 else "ragged_last_workgroup") + (".strided" if extra else "")
                  + (".gscale" if gs is not None else "") + (".one_row" if R == 1 else ""))


R1_CASES = [_r1(16, 64, 0, None), _r1(16, 64, 4, 0.37), _r1(5, 12, 0, 0.37), _r1(5, 12, 8, None), _r1(1, 8, 4, None), _r1(1, 1024, 0, 0.37),
            _r1(768, 768, 4, 0.37), _r1(768, 768, 0, None), _r1(33, 100, 12, None)]
R1_LABELS = ("full_workgroups", "ragged_last_workgroup", "strided", "gscale", "one_row")


def r1_case_id(c):
    return f"rank1_add-{c.R}x{c.C}-ld{c.C + c.extra}-{c.path}"


def _r1_problem(R, C, key):
    g = _gen("rank1", R, C, key)
    return torch.randn(R, C, generator=g), torch.randn(R, generator=g), torch.randn(C, generator=g)


def _vec(t, dev):
    return guarded_input(t[None], F32, dev, 0)[0]


def check_r1_case(c):
    _, _, _, ops = _abi()
    dev = torch.device("cuda:0")
    out0, a, b = _r1_problem(c.R, c.C, 0)
    ob = Guarded("out", [c.R], c.C, F32, c.extra, device=dev)
    ob.seg(0).copy_(out0)
    ops.rank1_add(ob.seg(0), _vec(a, dev), _vec(b, dev), gscale=None if c.gs is None else torch.full((1,), c.gs, device=dev))
    torch.cuda.synchronize()
    return ob.check() + bits_among("out: fl(out + fl(a' b)) or fma(a', b, out); index = (row, column)", ob.seg(0), rank1_candidates(out0, a, b, c.gs))


BatCase = collections.namedtuple("BatCase", "entry n R C opt gs path")      # entry "gemv" (opt "32" / "16": the weight type) / "rank1"


def _bat(entry, n, R, C, opt, gs):
    launches = -(-n // SMALL_BATCH_MAX)
    return BatCase(entry, n, R, C, opt, gs, f"launches{launches}.last_launch_{n - SMALL_BATCH_MAX * (launches - 1)}_items" + (".gscale" if gs is not None else ""))


BAT_NS = (1, 16, 17, 33)
BAT_CASES = ([_bat("gemv", n, 5, 65, opt, gs) for n in BAT_NS for opt in ("32", "16") for gs in (None, 0.5)]
             + [_bat("rank1", n, 5, 12, "", gs) for n in BAT_NS for gs in (None, 0.37)])


def bat_case_id(c):
    return f"{'gemv_rows' if c.entry == 'gemv' else 'rank1_add'}_batched-n{c.n}-{c.R}x{c.C}" + (f"-w{c.opt}" if c.opt else "") + "-" + c.path


def check_bat_case(c):
    """the batched entry point against n calls of the one-item entry point on the same inputs: bit-equal per item; betas mixed 0 / 1"""
    _, _, _, ops = _abi()
    dev = torch.device("cuda:0")
    gs = None if c.gs is None else torch.full((1,), c.gs, device=dev)
    f, bad = [], 0
    if c.entry == "gemv":
        g = _gen("gemv_batched", c.n, c.opt)
        W = [guarded_input(torch.randn(c.R, c.C, generator=g), BF if c.opt == "16" else F32, dev, 8 if c.opt == "16" else 4) for _ in range(c.n)]
        x = [_vec(torch.randn(c.C, generator=g), dev) for _ in range(c.n)]
        y0 = [torch.randn(c.R, generator=g) for _ in range(c.n)]
        betas = [float(i % 2) for i in range(c.n)]
        runs = []
        for tag in ("batched", "one by one"):
            ys = [Guarded(f"y[{i}] ({tag})", [c.R], 1, F32, device=dev) for i in range(c.n)]
            for yb, v in zip(ys, y0):
                yb.seg(0).copy_(v[:, None])
            outs = [yb.seg(0)[:, 0] for yb in ys]
            if tag == "batched":
                ops.gemv_rows_batched(W, x, outs, betas, gscale=gs)
            else:
                for i in range(c.n):
                    ops.gemv_rows(W[i], x[i], out=outs[i], beta=betas[i], gscale=gs)
            runs.append(ys)
    else:
        probs = [_r1_problem(c.R, c.C, i) for i in range(c.n)]
        a, b = [_vec(p[1], dev) for p in probs], [_vec(p[2], dev) for p in probs]
        runs = []
        for tag in ("batched", "one by one"):
            ys = [Guarded(f"out[{i}] ({tag})", [c.R], c.C, F32, 4, device=dev) for i in range(c.n)]
            for yb, p in zip(ys, probs):
                yb.seg(0).copy_(p[0])
            outs = [yb.seg(0) for yb in ys]
            if tag == "batched":
                ops.rank1_add_batched(outs, a, b, gscale=gs)
            else:
                for i in range(c.n):
                    ops.rank1_add(outs[i], a[i], b[i], gscale=gs)
            runs.append(ys)
    torch.cuda.synchronize()
    for i, (yb, y1) in enumerate(zip(*runs)):
        r = yb.check() + y1.check() + bits_equal(f"item {i}: batched against the one-item entry point", yb.seg(0), y1.seg(0))
        if c.entry == "rank1":
            r += bits_among(f"item {i}: fl(out + fl(a' b)) or fma(a', b, out)", yb.seg(0), rank1_candidates(*probs[i], c.gs))
        bad += sum(not x.ok for x in r)
        f += [x for x in r if not x.ok]
    f.append(Finding(f"{c.n} items: findings that failed", bad == 0, float(bad), 0.0, c.path))
    return f


def cwm_items(kind):
    """[(R, C, offset of `out` in elements)]: "seam_96_then_ragged" 96 items with sides x64 and a ragged 97th; "out_offset_4_bytes" all x64, one
    `out` 4 bytes into its buffer"""
    if kind == "seam_96_then_ragged":
        return [((64, 128), (128, 64), (64, 64))[i % 3] + (0,) for i in range(CAST_MULTI_MAX)] + [(33, 65, 0)]
    return [(64, 64, 0), (128, 64, 0), (64, 128, 2), (64, 64, 0), (128, 128, 0)]


def cwm_path(kind):
    """the dispatch of pvrl_cast_weights_multi_bf16 restated: per launch of <= 96 items, 64-tiles only when every side is x64 and every `out` 8-byte aligned"""
    items, tiles = cwm_items(kind), []
    for i0 in range(0, len(items), CAST_MULTI_MAX):
        part = items[i0:i0 + CAST_MULTI_MAX]
        tiles.append("tile64" if all(R % 64 == 0 and C % 64 == 0 and (2 * off) % 8 == 0 for R, C, off in part) else "tile32")
    return "+".join(tiles)


CWM_CASES = ("seam_96_then_ragged", "out_offset_4_bytes")


def cwm_case_id(kind):
    return f"cast_weights_multi-{len(cwm_items(kind))}_items-{kind}-{cwm_path(kind)}"


def check_cwm_case(kind):
    _, _, _, ops = _abi()
    dev = torch.device("cuda:0")
    g = _gen("cwm", kind)
    pat = torch.full((1,), PATTERN[2], dtype=torch.int16).view(BF)
    ws, bufs, items = [], [], []
    for (R, C, off) in cwm_items(kind):
        w = torch.randn(R, C, generator=g)
        pair = [pat.repeat(R * C + 64).to(dev) for _ in range(2)]          # off elements in front of and 64 - off behind each copy hold the pattern
        ws.append(w)
        bufs.append(pair)
        items.append((guarded_input(w.reshape(1, -1), F32, dev, 64)[0].view(R, C), pair[0][off:off + R * C].view(R, C), pair[1][off:off + R * C].view(C, R)))
    ops.cast_weights_multi(items)
    torch.cuda.synchronize()
    f, bad = [], 0
    for i, ((R, C, off), w, pair, it) in enumerate(zip(cwm_items(kind), ws, bufs, items)):
        r = bits_equal(f"item {i} ({R}x{C}): out against R16(w)", it[1], w.to(BF)) + bits_equal(f"item {i} ({R}x{C}): out_t against R16(w).t()", it[2], w.t().to(BF))
        for name, b in zip(("out", "out_t"), pair):
            rest = torch.cat([b[:off], b[off + R * C:]]).cpu().view(torch.int16)
            nt = int((rest != PATTERN[2]).sum())
            r.append(Finding(f"item {i}: elements around {name} that changed", nt == 0, float(nt), 0.0, ""))
        bad += sum(not x.ok for x in r)
        f += [x for x in r if not x.ok]
    f.append(Finding(f"{len(items)} items ({cwm_path(kind)}): findings that failed", bad == 0, float(bad), 0.0, ""))
    return f


# =====================================================================================================================
# refusals
# =====================================================================================================================
def check_refusals():
    """PVRL_EINVAL before any launch and nothing written: crop % 16 (patchify), crop % 4 (f32), ldo % 8, ldo < 768, a zero std, null src or
    S <= 0 on a _views call; B == 0 returns OK and writes nothing; pvrl_patchify's own ldo / size refusals"""
    from procedurevrl_amd._lib import PvrlError
    L, P, St, ops = _abi()
    dev = torch.device("cuda:0")
    T, H0, W0, B = 2, 40, 44, 2
    fr = _u8_device(make_frames("randint", B, T, H0, W0, "refusals"), dev)
    prm = torch.tensor([[40, 44, 1, 2, 0], [40, 44, 2, 1, 1]], dtype=torch.int32, device=dev)
    src = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    rows = [("patchify", "crop % 16 != 0", dict(crop=24)), ("f32", "crop % 4 != 0", dict(crop=18)), ("patchify", "ldo % 8 != 0", dict(ldo=772)),
            ("patchify", "ldo < 768", dict(ldo=760)), ("patchify", "zero std", dict(std=(0.225, 0.0, 0.2))), ("f32", "zero std", dict(std=(0.0, 0.25, 0.2))),
            ("patchify", "null src on a _views call", dict(src="null", S=2)), ("f32", "null src on a _views call", dict(src="null", S=2)),
            ("patchify", "S == 0 on a _views call", dict(src=src, S=0)), ("f32", "S == -1 on a _views call", dict(src=src, S=-1)),
            ("patchify", "B == 0", dict(B=0)), ("f32", "B == 0", dict(B=0)), ("patchify", "B == 0 on a _views call", dict(B=0, src=src, S=2))]
    f = []
    for entry, what, kw in rows:
        crop, ldo, nB = kw.get("crop", 16), kw.get("ldo", 768), kw.get("B", B)
        ob = Guarded("out", [B * T * 4], 768, BF, 8, device=dev) if entry == "patchify" else Guarded("out", [B * 3 * T * 24], 24, F32, device=dev)
        msg = _dec_call(entry, fr, prm, kw.get("src"), kw.get("S", 0), nB, T, H0, W0, crop, ob.seg(0), ldo, std=kw.get("std", STD))
        torch.cuda.synchronize()
        ok = (msg is None) if nB == 0 else (msg is not None and msg.endswith("status -1"))
        f.append(Finding(f"frames_u8_{entry} {what}: status", ok, 0.0, 0.0, msg or "returned OK"))
        f += untouched(ob)
    x = torch.randn(1, 3, 1, 32, 48).to(dev)
    for what, (HI, WI, ldo, nB) in (("HI % 16 != 0", (24, 48, 768, 1)), ("WI % 16 != 0", (32, 40, 768, 1)), ("ldo % 8 != 0", (32, 48, 772, 1)),
                                    ("ldo < 768", (32, 48, 760, 1)), ("B == 0", (32, 48, 768, 0))):
        ob = Guarded("out", [6], 768, BF, 8, device=dev)
        try:
            L.call("pvrl_patchify", P(x), nB, 1, HI, WI, P(ob.seg(0)), ldo, St())
            msg = None
        except PvrlError as e:
            msg = str(e)
        torch.cuda.synchronize()
        ok = (msg is None) if nB == 0 else (msg is not None and msg.endswith("status -1"))
        f.append(Finding(f"patchify {what}: status", ok, 0.0, 0.0, msg or "returned OK"))
        f += untouched(ob)
    return f


def check_decoded_validation(dev="cpu"):
    """ops._check_decoded raises, from the host copies alone, for a window that leaves the rescaled frame, a negative offset and a `src`
    outside [0, S)"""
    from procedurevrl_amd import ops
    from procedurevrl_amd.transform import DecodedClips, DecodedViews
    fr = torch.zeros(2, 1, 40, 44, 3, dtype=torch.uint8, device=dev)
    ok_p = [40, 44, 3, 4, 0]
    rows = [("window below the rescaled frame", DecodedClips(fr, [ok_p, [40, 44, 9, 4, 0]], MEAN, STD, 32)),
            ("window right of the rescaled frame", DecodedClips(fr, [[40, 44, 3, 13, 1], ok_p], MEAN, STD, 32)),
            ("rescaled frame smaller than the crop", DecodedClips(fr, [ok_p, [31, 44, 0, 0, 0]], MEAN, STD, 32)),
            ("negative y_off", DecodedClips(fr, [ok_p, [40, 44, -1, 4, 0]], MEAN, STD, 32)),
            ("negative x_off", DecodedClips(fr, [[40, 44, 3, -2, 0], ok_p], MEAN, STD, 32)),
            ("src == S", DecodedViews(fr, [ok_p] * 3, [0, 2, 1], MEAN, STD, 32)), ("src == -1", DecodedViews(fr, [ok_p] * 3, [0, -1, 1], MEAN, STD, 32))]
    f = []
    for what, clips in rows:
        try:
            ops._check_decoded(clips)
            msg = None
        except ValueError as e:
            msg = str(e)
        f.append(Finding(f"_check_decoded, {what}: raises ValueError", msg is not None, 0.0, 0.0, msg or "accepted"))
    return f
