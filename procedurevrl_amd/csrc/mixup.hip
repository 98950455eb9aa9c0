// Mixup / CutMix of a fine-tuning batch (lib/datasets/mixup.py `Mixup._mix_batch / _mix_pair / _mix_elem`), in place.
// The host draws the plan (procedurevrl_amd/mixup.py); this kernel does the per-element work.  Clip b is mixed with clip
// p = B-1-b in every mode, so the batch splits into B/2 independent pairs: one thread owns element e of BOTH clips of a pair,
// loads both before storing either, and every output is therefore a function of the unmixed batch (the reference's
// `x.flip(0)` / `x_orig` copies), with no second buffer.
//   blend  x[b] = x[b] * lam + x[p] * lam_partner   two fp32 products and an fp32 sum, each rounded (no FMA contraction):
//                                                   the bits of torch's CPU `x.mul_(lam).add_(x.flip(0).mul_(1 - lam))`
//   cut    x[b][:, t0:t1, h0:h1, :] = x[p][...]     the box is drawn on (H, W) but sliced on (T, H), all columns (reference quirk)
// Grid: x over the vectors of one clip (grid-stride), y over the pairs.  A box covers whole W rows, so a float4 along W is
// entirely inside or outside it; W % 4 != 0 (or an unaligned batch) takes the scalar form.
#include "common.h"
#include "../../include/pvrl.h"

namespace {

__device__ __forceinline__ float blend(float a, float wa, float b, float wb) {
#pragma clang fp contract(off)   // hipcc contracts a*b + c into an FMA by default (and so would __fmul_rn / __fadd_rn, once inlined)
  const float u = a * wa, v = b * wb;
  return u + v;
}

__device__ __forceinline__ bool touches(const pvrl_mix_desc& d, int t, int h) {
  return d.kind == PVRL_MIX_BLEND || (d.kind == PVRL_MIX_CUT && t >= d.t0 && t < d.t1 && h >= d.h0 && h < d.h1);
}

template <int V>
struct vec_t { typedef float type; };
template <>
struct vec_t<4> { typedef float4 type; };

template <int V>
__device__ __forceinline__ typename vec_t<V>::type mix_vec(typename vec_t<V>::type a, float wa, typename vec_t<V>::type b, float wb) {
  if constexpr (V == 4) {
    return make_float4(blend(a.x, wa, b.x, wb), blend(a.y, wa, b.y, wb), blend(a.z, wa, b.z, wb), blend(a.w, wa, b.w, wb));
  } else {
    return blend(a, wa, b, wb);
  }
}

template <int V>
__global__ __launch_bounds__(256) void mix_clips_kernel(float* __restrict__ x, const pvrl_mix_desc* __restrict__ desc, int B,
                                                        unsigned T, unsigned H, unsigned WV, unsigned nvec) {
  typedef typename vec_t<V>::type vt;
  const int b = blockIdx.y, p = B - 1 - b;
  const pvrl_mix_desc db = desc[b], dp = desc[p];
  if (db.kind == PVRL_MIX_NONE && dp.kind == PVRL_MIX_NONE) return;
  vt* xb = reinterpret_cast<vt*>(x) + (long)b * nvec;
  vt* xp = reinterpret_cast<vt*>(x) + (long)p * nvec;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < nvec; i += gridDim.x * 256) {
    const unsigned row = i / WV;                 // (c, t, h) row of W / V vectors (32-bit: the host caps a clip at 2^31 elements)
    const int h = (int)(row % H), t = (int)((row / H) % T);
    const bool ib = touches(db, t, h), ip = touches(dp, t, h);
    if (!ib && !ip) continue;
    // load only what an output needs: a cut reads the partner alone, a blend both clips
    vt vb{}, vp{};
    if (ip || db.kind == PVRL_MIX_BLEND) vb = xb[i];
    if (ib || dp.kind == PVRL_MIX_BLEND) vp = xp[i];
    if (ib) xb[i] = db.kind == PVRL_MIX_BLEND ? mix_vec<V>(vb, db.lam, vp, db.lam_partner) : vp;
    if (ip) xp[i] = dp.kind == PVRL_MIX_BLEND ? mix_vec<V>(vp, dp.lam, vb, dp.lam_partner) : vb;
  }
}

}  // namespace

extern "C" int pvrl_mix_clips(float* x, const pvrl_mix_desc* desc, int64_t B, int64_t C, int64_t T, int64_t H, int64_t W,
                              void* stream) {
  if (B <= 0) return PVRL_OK;
  if (!x || !desc || B % 2 != 0 || B / 2 > 65535 || C <= 0 || T <= 0 || H <= 0 || W <= 0) return PVRL_EINVAL;
  if (C * T * H * W >= (int64_t(1) << 31)) return PVRL_EINVAL;
  const bool v4 = W % 4 == 0 && ((uintptr_t)x & 15) == 0;
  const int V = v4 ? 4 : 1;
  const long nvec = C * T * H * W / V;
  long blocks = (nvec + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  const dim3 grid((unsigned)blocks, (unsigned)(B / 2));
  if (v4)
    hipLaunchKernelGGL(mix_clips_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, x, desc, (int)B, (unsigned)T, (unsigned)H,
                       (unsigned)(W / 4), (unsigned)nvec);
  else
    hipLaunchKernelGGL(mix_clips_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, desc, (int)B, (unsigned)T, (unsigned)H,
                       (unsigned)W, (unsigned)nvec);
  PVRL_LAUNCH_CHECK();
  return PVRL_OK;
}
