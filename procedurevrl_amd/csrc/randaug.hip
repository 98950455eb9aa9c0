// RandAugment of decoded uint8 clips (lib/datasets/autoaugment.py through PIL, per frame: lib/datasets/epickitchens.py:149-162),
// bit-equal to Pillow.  The host draws the plan (procedurevrl_amd/randaugment.py): one pvrl_ra_desc per frame and layer, in
// device memory, so the launch sequence is the same whatever was drawn.  Per layer, from the previous layer's output:
//   ra_stats_kernel   the three channel histograms and the luma histogram of the frames whose op reads them (AutoContrast,
//                     Equalize, Contrast): LDS atomics per workgroup, then one vector atomic per non-empty bin into an int32
//                     workspace that a memset node cleared; other frames' workgroups leave at once
//   ra_apply_kernel   per frame, by descriptor: copy / 3 x 256 table in LDS (built from the argument or the histogram) /
//                     Image.blend against a degenerate (black, mean luma, luma, 3x3 smooth) / affine gather
// Arithmetic, as Pillow's C does it and one rounding per operation (fp contraction is off for the whole file):
//   affine   source position a (x + 1/2) + b (y + 1/2) + c in double, fill colour outside [0, W) x [0, H); then - 1/2, clamped
//            neighbours; bilinear: two lerps p + (q - p) d, truncated; bicubic: Geometry.c's cubic in Horner form over 4 x 4, clamped
//            to [0, 255], truncated
//   blend    (float) deg + (float) factor * (float) (img - deg): Blend.c takes its alpha as a C float; clamped, truncated
//   smooth   (sum of the 3 x 3 neighbourhood + 4 centre) / 13 rounded = (2 s + 13) / 26 in integers; the border is copied
//   tables   AutoContrast int(i * (255.0 / (hi - lo)) + (-lo * scale)) in double; Equalize in integers, clipped to 255 as
//            Image.point clips its table
// Work item: 4 pixels of a row (12 bytes = 3 dwords, loaded and stored as dwords) when W % 4 == 0 and the buffers are dword-aligned;
// else 1 pixel (byte loads and stores).  One workgroup takes up to 1024 items of one frame.
#include "common.h"
#include "../../include/pvrl.h"

#pragma clang fp contract(off)

namespace {

constexpr int ITEMS_PER_BLOCK = 1024;
constexpr int STAT_PIXELS_PER_BLOCK = 8192;

__device__ __forceinline__ int luma24(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

__device__ __forceinline__ bool needs_stats(int kind) {
  return kind == PVRL_RA_AUTOCONTRAST || kind == PVRL_RA_EQUALIZE || kind == PVRL_RA_CONTRAST;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// 4 pixels <-> 3 dwords
__device__ __forceinline__ void unpack12(const uint32_t w[3], uint8_t px[12]) {
#pragma unroll
  for (int i = 0; i < 12; ++i) px[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}
__device__ __forceinline__ void pack12(const uint8_t px[12], uint32_t w[3]) {
#pragma unroll
  for (int j = 0; j < 3; ++j)
    w[j] = (uint32_t)px[4 * j] | ((uint32_t)px[4 * j + 1] << 8) | ((uint32_t)px[4 * j + 2] << 16) | ((uint32_t)px[4 * j + 3] << 24);
}

template <bool VEC>
__global__ __launch_bounds__(256) void ra_stats_kernel(const uint8_t* __restrict__ src, const pvrl_ra_desc* __restrict__ desc,
                                                       int32_t* __restrict__ hist, int64_t npix, int bpf) {
  const int64_t f = blockIdx.x / bpf;
  const int part = blockIdx.x % bpf;
  const int kind = desc[f].kind;
  if (!needs_stats(kind)) return;
  __shared__ int h[4 * 256];
  for (int i = threadIdx.x; i < 4 * 256; i += 256) h[i] = 0;
  __syncthreads();
  const bool want_luma = kind == PVRL_RA_CONTRAST;
  const uint8_t* p = src + f * npix * 3;
  constexpr int V = VEC ? 4 : 1;
  const int64_t nitems = npix / V;
  const int64_t per = (nitems + bpf - 1) / bpf;
  const int64_t lo = part * per, hi = lo + per < nitems ? lo + per : nitems;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
    uint8_t px[3 * V];
    if constexpr (VEC) {
      const uint32_t* q = reinterpret_cast<const uint32_t*>(p) + i * 3;
      const uint32_t w[3] = {q[0], q[1], q[2]};
      unpack12(w, px);
    } else {
      px[0] = p[i * 3], px[1] = p[i * 3 + 1], px[2] = p[i * 3 + 2];
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int r = px[3 * k], g = px[3 * k + 1], b = px[3 * k + 2];
      if (want_luma) {
        atomicAdd(&h[768 + luma24(r, g, b)], 1);
      } else {
        atomicAdd(&h[r], 1);
        atomicAdd(&h[256 + g], 1);
        atomicAdd(&h[512 + b], 1);
      }
    }
  }
  __syncthreads();
  int32_t* out = hist + f * 1024;
  for (int i = threadIdx.x; i < 4 * 256; i += 256)
    if (h[i]) atomicAdd(&out[i], h[i]);
}

struct frame_ctx {
  const uint8_t* src;       // the frame this layer reads
  const uint8_t* lut;       // 3 x 256 table in LDS (table kinds)
  int W, H;
  int kind, resample;
  int mean;                 // Contrast's degenerate
  float factor;             // Image.blend's alpha
  double c[6];
  uint8_t fill[3];
};

__device__ __forceinline__ uint8_t blend8(int deg, int img, float alpha) {
  const float diff = (float)(img - deg);
  const float prod = alpha * diff;
  const float t = (float)deg + prod;
  if (t <= 0.0f) return 0;
  if (t >= 255.0f) return 255;
  return (uint8_t)(int)t;
}

__device__ __forceinline__ double cubic(double v1, double v2, double v3, double v4, double d) {
  const double p1 = v2;
  const double p2 = -v1 + v3;
  const double p3 = 2 * (v1 - v2) + v3 - v4;
  const double p4 = -v1 + v2 - v3 + v4;
  return p1 + d * (p2 + d * (p3 + d * p4));
}

__device__ __forceinline__ void affine_pixel(const frame_ctx& c, int x, int y, uint8_t out[3]) {
  const double xin = (double)x + 0.5, yin = (double)y + 0.5;
  double sx = c.c[0] * xin + c.c[1] * yin + c.c[2];
  double sy = c.c[3] * xin + c.c[4] * yin + c.c[5];
  if (!(sx >= 0.0 && sx < (double)c.W && sy >= 0.0 && sy < (double)c.H)) {
    out[0] = c.fill[0], out[1] = c.fill[1], out[2] = c.fill[2];
    return;
  }
  sx -= 0.5;
  sy -= 0.5;
  const double fx = floor(sx), fy = floor(sy);
  const int x0 = (int)fx, y0 = (int)fy;
  const double dx = sx - fx, dy = sy - fy;
  const int64_t row = (int64_t)c.W * 3;
  if (c.resample == PVRL_RA_BILINEAR) {
    const uint8_t* r0 = c.src + clampi(y0, 0, c.H - 1) * row;
    const uint8_t* r1 = c.src + clampi(y0 + 1, 0, c.H - 1) * row;
    const int xa = clampi(x0, 0, c.W - 1) * 3, xb = clampi(x0 + 1, 0, c.W - 1) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int p00 = r0[xa + ch], p01 = r0[xb + ch], p10 = r1[xa + ch], p11 = r1[xb + ch];
      const double v1 = (double)p00 + (double)(p01 - p00) * dx;
      const double v2 = (double)p10 + (double)(p11 - p10) * dx;
      const double v = v1 + (v2 - v1) * dy;
      out[ch] = (uint8_t)(int)v;
    }
  } else {
    int xs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) xs[i] = clampi(x0 - 1 + i, 0, c.W - 1) * 3;
    double acc[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint8_t* r = c.src + clampi(y0 - 1 + j, 0, c.H - 1) * row;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        acc[ch][j] = cubic((double)r[xs[0] + ch], (double)r[xs[1] + ch], (double)r[xs[2] + ch], (double)r[xs[3] + ch], dx);
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const double v = cubic(acc[ch][0], acc[ch][1], acc[ch][2], acc[ch][3], dy);
      out[ch] = v <= 0.0 ? 0 : (v >= 255.0 ? 255 : (uint8_t)(int)v);
    }
  }
}

// one output pixel of every kind but AFFINE; `in` is the pixel at (x, y)
__device__ __forceinline__ void point_pixel(const frame_ctx& c, int x, int y, const uint8_t in[3], uint8_t out[3]) {
  switch (c.kind) {
    case PVRL_RA_AUTOCONTRAST:
    case PVRL_RA_EQUALIZE:
    case PVRL_RA_INVERT:
    case PVRL_RA_POSTERIZE:
    case PVRL_RA_SOLARIZE:
    case PVRL_RA_SOLARIZE_ADD:
      out[0] = c.lut[in[0]], out[1] = c.lut[256 + in[1]], out[2] = c.lut[512 + in[2]];
      break;
    case PVRL_RA_COLOR: {
      const int l = luma24(in[0], in[1], in[2]);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) out[ch] = blend8(l, in[ch], c.factor);
      break;
    }
    case PVRL_RA_CONTRAST:
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) out[ch] = blend8(c.mean, in[ch], c.factor);
      break;
    case PVRL_RA_BRIGHTNESS:
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) out[ch] = blend8(0, in[ch], c.factor);
      break;
    case PVRL_RA_SHARPNESS: {
      if (x == 0 || y == 0 || x == c.W - 1 || y == c.H - 1) {   // the filter copies the border: blend(img, img) = img
        out[0] = in[0], out[1] = in[1], out[2] = in[2];
        break;
      }
      int s[3] = {4 * in[0], 4 * in[1], 4 * in[2]};
      const uint8_t* p = c.src + ((int64_t)(y - 1) * c.W + (x - 1)) * 3;
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 9; ++i) s[i % 3] += p[(int64_t)j * c.W * 3 + i];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) out[ch] = blend8((2 * s[ch] + 13) / 26, in[ch], c.factor);
      break;
    }
    default:   // PVRL_RA_NONE and anything unknown: the frame as it is
      out[0] = in[0], out[1] = in[1], out[2] = in[2];
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void ra_apply_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                       const pvrl_ra_desc* __restrict__ desc, const int32_t* __restrict__ hist,
                                                       int H, int W, int bpf, int fill_r, int fill_g, int fill_b) {
  const int64_t f = blockIdx.x / bpf;
  const int part = blockIdx.x % bpf;
  const int64_t npix = (int64_t)H * W;
  const pvrl_ra_desc d = desc[f];
  __shared__ uint8_t lut[3 * 256];
  __shared__ int sh[3 * 256];
  __shared__ int s_lo[3], s_hi[3], s_step[3], s_mean;
  const int tid = threadIdx.x;
  const int32_t* hf = hist + f * 1024;

  frame_ctx c;
  c.src = src + f * npix * 3;
  c.lut = lut;
  c.W = W, c.H = H;
  c.kind = d.kind, c.resample = d.resample;
  c.mean = 0;
  c.factor = (float)d.c[0];
#pragma unroll
  for (int i = 0; i < 6; ++i) c.c[i] = d.c[i];
  c.fill[0] = (uint8_t)fill_r, c.fill[1] = (uint8_t)fill_g, c.fill[2] = (uint8_t)fill_b;

  // ---- per-frame table / statistic, rebuilt by every workgroup of the frame ----
  if (d.kind == PVRL_RA_INVERT || d.kind == PVRL_RA_POSTERIZE || d.kind == PVRL_RA_SOLARIZE || d.kind == PVRL_RA_SOLARIZE_ADD) {
    const int i = tid, a0 = d.iarg[0], a1 = d.iarg[1];
    int v;
    if (d.kind == PVRL_RA_INVERT) v = 255 - i;
    else if (d.kind == PVRL_RA_POSTERIZE) v = a0 <= 0 ? 0 : (a0 >= 8 ? i : (i & ~((1 << (8 - a0)) - 1)));
    else if (d.kind == PVRL_RA_SOLARIZE) v = i < a0 ? i : 255 - i;
    else v = i < a1 ? (i + a0 > 255 ? 255 : i + a0) : i;
    lut[i] = lut[256 + i] = lut[512 + i] = (uint8_t)clampi(v, 0, 255);
    __syncthreads();
  } else if (d.kind == PVRL_RA_AUTOCONTRAST || d.kind == PVRL_RA_EQUALIZE) {
    for (int i = tid; i < 768; i += 256) sh[i] = hf[i];
    __syncthreads();
    if (tid < 3) {
      const int* h = sh + tid * 256;
      if (d.kind == PVRL_RA_AUTOCONTRAST) {
        int lo = 0, hi = 255;
        while (lo < 255 && !h[lo]) ++lo;
        while (hi > 0 && !h[hi]) --hi;
        s_lo[tid] = lo, s_hi[tid] = hi;
      } else {
        // ImageOps.equalize: step = (pixels - count of the last occupied bin) // 255; the table is the running count
        int nnz = 0, last = 0;
        long sum = 0;
        for (int i = 0; i < 256; ++i)
          if (h[i]) ++nnz, last = h[i], sum += h[i];
        const int step = nnz <= 1 ? 0 : (int)((sum - last) / 255);
        s_step[tid] = step;
        if (step) {
          long n = step / 2;
          for (int i = 0; i < 256; ++i) {
            const long v = n / step;
            lut[tid * 256 + i] = (uint8_t)(v > 255 ? 255 : v);
            n += h[i];
          }
        }
      }
    }
    __syncthreads();
    for (int ch = 0; ch < 3; ++ch) {
      const int i = tid;
      if (d.kind == PVRL_RA_AUTOCONTRAST) {
        const int lo = s_lo[ch], hi = s_hi[ch];
        int v = i;
        if (hi > lo) {
          const double scale = 255.0 / (double)(hi - lo);
          const double offset = (double)(-lo) * scale;
          const double t = (double)i * scale + offset;
          v = clampi((int)t, 0, 255);
        }
        lut[ch * 256 + i] = (uint8_t)v;
      } else if (!s_step[ch]) {
        lut[ch * 256 + i] = (uint8_t)i;
      }
    }
    __syncthreads();
  } else if (d.kind == PVRL_RA_CONTRAST) {
    // ImageEnhance.Contrast: int(mean of the luma image + 0.5), the mean a double quotient of two exact integers
    if (tid == 0) {
      long sum = 0, n = 0;
      for (int i = 0; i < 256; ++i) sum += (long)i * hf[768 + i], n += hf[768 + i];
      const double m = (double)sum / (double)(n > 0 ? n : 1);
      s_mean = (int)(m + 0.5);
    }
    __syncthreads();
    c.mean = s_mean;
  }

  constexpr int V = VEC ? 4 : 1;
  const int wv = W / V;                                  // items per row
  const int64_t nitems = npix / V;
  const int64_t per = (nitems + bpf - 1) / bpf;
  const int64_t lo = part * per, hi = lo + per < nitems ? lo + per : nitems;
  uint8_t* out_frame = dst + f * npix * 3;
  for (int64_t it = lo + tid; it < hi; it += 256) {
    const int y = (int)(it / wv), x = (int)(it % wv) * V;
    uint8_t in[3 * V], out[3 * V];
    if (c.kind != PVRL_RA_AFFINE) {
      if constexpr (VEC) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(c.src) + it * 3;
        const uint32_t w[3] = {q[0], q[1], q[2]};
        unpack12(w, in);
      } else {
        in[0] = c.src[it * 3], in[1] = c.src[it * 3 + 1], in[2] = c.src[it * 3 + 2];
      }
#pragma unroll
      for (int k = 0; k < V; ++k) point_pixel(c, x + k, y, in + 3 * k, out + 3 * k);
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) affine_pixel(c, x + k, y, out + 3 * k);
    }
    if constexpr (VEC) {
      uint32_t w[3];
      pack12(out, w);
      uint32_t* q = reinterpret_cast<uint32_t*>(out_frame) + it * 3;
      q[0] = w[0], q[1] = w[1], q[2] = w[2];
    } else {
      out_frame[it * 3] = out[0], out_frame[it * 3 + 1] = out[1], out_frame[it * 3 + 2] = out[2];
    }
  }
}

}  // namespace

extern "C" int pvrl_rand_augment_u8(const void* in, void* out, void* tmp, const pvrl_ra_desc* desc, int64_t frames, int64_t layers,
                                    int64_t H, int64_t W, int fill_r, int fill_g, int fill_b, int32_t* hist, void* stream) {
  if (frames <= 0) return PVRL_OK;
  if (!in || !out || in == out || layers < 0 || H <= 0 || W <= 0 || H >= (int64_t(1) << 31) || W >= (int64_t(1) << 31) || H * W >= (int64_t(1) << 31)) return PVRL_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int64_t npix = H * W;
  if (layers == 0) {
    if (hipMemcpyAsync(out, in, (size_t)(frames * npix * 3), hipMemcpyDeviceToDevice, st) != hipSuccess) return PVRL_EHIP;
    return PVRL_OK;
  }
  if (!desc || !hist || (layers > 1 && (!tmp || tmp == in || tmp == out))) return PVRL_EINVAL;
  const bool vec = W % 4 == 0 && (((uintptr_t)in | (uintptr_t)out | (uintptr_t)tmp) & 3) == 0;
  const int64_t nitems = vec ? npix / 4 : npix;
  int64_t bpf = (nitems + ITEMS_PER_BLOCK - 1) / ITEMS_PER_BLOCK;
  if (bpf > 64) bpf = 64;
  int64_t sbpf = (npix + STAT_PIXELS_PER_BLOCK - 1) / STAT_PIXELS_PER_BLOCK;
  if (sbpf > 32) sbpf = 32;
  if (frames * bpf >= (int64_t(1) << 31) || frames * sbpf >= (int64_t(1) << 31)) return PVRL_EINVAL;
  const uint8_t* src = static_cast<const uint8_t*>(in);
  for (int64_t l = 0; l < layers; ++l) {
    uint8_t* dst = static_cast<uint8_t*>((layers - 1 - l) % 2 == 0 ? out : tmp);     // the last layer writes `out`
    const pvrl_ra_desc* dl = desc + l * frames;
    if (hipMemsetAsync(hist, 0, (size_t)(frames * 1024 * sizeof(int32_t)), st) != hipSuccess) return PVRL_EHIP;
    const dim3 sgrid((unsigned)(frames * sbpf)), agrid((unsigned)(frames * bpf));
    if (vec) {
      hipLaunchKernelGGL(ra_stats_kernel<true>, sgrid, dim3(256), 0, st, src, dl, hist, npix, (int)sbpf);
      hipLaunchKernelGGL(ra_apply_kernel<true>, agrid, dim3(256), 0, st, src, dst, dl, hist, (int)H, (int)W, (int)bpf, fill_r, fill_g,
                         fill_b);
    } else {
      hipLaunchKernelGGL(ra_stats_kernel<false>, sgrid, dim3(256), 0, st, src, dl, hist, npix, (int)sbpf);
      hipLaunchKernelGGL(ra_apply_kernel<false>, agrid, dim3(256), 0, st, src, dst, dl, hist, (int)H, (int)W, (int)bpf, fill_r, fill_g,
                         fill_b);
    }
    PVRL_LAUNCH_CHECK();
    src = dst;
  }
  return PVRL_OK;
}
