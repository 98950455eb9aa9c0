// Multi-head self-attention (head_dim 64) on MFMA, forward + backward, S <= 416 tokens (tuned for S <= 208; the reference takes any
// crop through its pos-embed resize, lib/models/vit.py:374-386 -- 256^2 gives 257 tokens, 320^2 gives 401).
//
// Reference semantics: Attention.forward, lib/models/vit.py:75-92
//     attn = softmax((q @ k^T) * scale);  x = attn @ v
// used for the spatial branch of Block.forward (vit.py:137-151; 197 tokens per (clip, frame)),
// and nn.MultiheadAttention inside ResidualAttentionBlock (lib/models/tfm_model.py:32-53; key padding
// mask) / the CLIP text tower (causal mask).  Backward = autograd of the same expression.
//
// One workgroup (4 waves) per (sequence, head); every kernel keeps <= 57 KiB of LDS so two workgroups share a CU and
// one's tile loads overlap the other's MFMA work.  The whole K and V head slices of a sequence fit in LDS
// (197 x 64 bf16 = 25 KiB each), so softmax is exact single-pass (no online rescale) and the S x S
// score matrix never exists in memory (the reference materialises 477 MB of it).
// MFMA operands are arranged "swapped" (a = keys, b = queries) so that a lane owns ONE query and
// 4 keys per 16-key tile: the softmax row reduction is register-local plus two cross-lane
// steps, and P feeds the second MFMA straight from registers as its b-operand.  V (and, in the
// backward, K / Q / dO) is read through ds_read_b64_tr_b16 from a [4][16]-blocked LDS image, so
// no transposed copies are ever built.
// Round 2 measured a PERSISTENT form of the forward kernel (one workgroup per CU walking its (sequence, head) items, K / V in two
// LDS slots filled by LDS-DMA one item ahead, counted vmcnt so output stores are not waited for; 8 waves sharing each K / V
// fragment between two query tiles, or 16 waves): 121-127 us and 157 us against 100 us for this kernel at 3,072 items.  The
// kernel is not latency-bound: an item costs ~8 us of CU time whatever hides its loads -- 700 MFMAs (1.4 us), 43 k exp2
// (1.3 us at quarter rate), ~6 VALU operations per score (2 us) and 650 KB of LDS fragment reads (3-5 us) that 8-16 waves
// do not overlap with each other -- 12 items per CU = the 96 us measured (3.3 TB/s is a consequence, not the limit).
// The number of 16-key tiles NKT is a template parameter (1, 2, 3, 5, 13): every loop over keys is
// straight-line code the compiler can software-pipeline (a run-time tile count cost 5x in branches).
#include "attn_common.h"
#include "../../include/pvrl.h"

// attn_bwd_fused.hip: the persistent, LDS-DMA-streamed one-kernel backward for 96 < S <= 224 without masks
bool pvrl_attn_bwd_fused_ok(const AttnArgs& p);
int pvrl_attn_bwd_fused_launch(const AttnArgs& p, hipStream_t s);
// attn_bwd_s32.hip: one wave per (sequence, head) for 16 < S <= 32 contiguous tokens without masks (temporal attention at 32 frames)
bool pvrl_attn_bwd_s32_ok(const AttnArgs& p);
int pvrl_attn_bwd_s32_launch(const AttnArgs& p, hipStream_t s);

namespace {

// key-padding bits of the 4*NKT keys a lane owns in the "lane = query" layout (key = 16 kt + 4 q4 + r)
template <int NKT, bool GEN>
__device__ __forceinline__ unsigned long long pad_bits_q(const AttnArgs& p, int seq, int q4) {
  unsigned long long bits = 0ull;
  if constexpr (GEN) {
    if (p.kpm) {
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kt * 16 + 4 * q4 + r;
          if (key < p.mp.S && p.kpm[(long)seq * p.mp.S + key]) bits |= 1ull << (kt * 4 + r);
        }
    }
  }
  return bits;
}

// Cooperative load of one head slice [S rows][64] of a packed activation into the blocked LDS image, in two halves so a
// kernel can put EVERY global load it needs (both tiles + its waves' own fragments) in flight before the first wait.
// The image has ROWS rows (a multiple of 32, for the K = 32 MFMA steps), the workgroup NT threads; chunk_load (attn_common.h) is
// branch-free, so an issue is nothing but loads.
template <int NT, int ROWS>
struct TileRegs { u32x4 v[(ROWS * 8 + NT - 1) / NT]; };

template <int NT, int ROWS>
__device__ __forceinline__ void tile_issue(TileRegs<NT, ROWS>& t, const op_t* base, long ld, int col0, const SeqRows& sr, int S,
                                           const op_t* src0, int tid) {
  constexpr int ITERS = (ROWS * 8 + NT - 1) / NT;
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int idx = tid + NT * it;
    t.v[it] = chunk_load(base, ld, col0, sr, S, src0, idx >> 3, idx & 7);
  }
}
template <int NT, int ROWS>
__device__ __forceinline__ void tile_commit(const TileRegs<NT, ROWS>& t, char* bl, int tid) {
  constexpr int ITERS = (ROWS * 8 + NT - 1) / NT;
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int idx = tid + NT * it;
    const int row = idx >> 3, c = idx & 7;
    if (row < ROWS) *reinterpret_cast<u32x4*>(bl + bl_off(row, c * 8)) = t.v[it];
  }
}

// What every kernel of this file knows about its workgroup and lane before it touches data: tid / lane / wave (wave-uniform),
// the workgroup's (seq, h), S (SC: the sequence length as a compile-time constant, 0 = run time), HD = H * 64 (the column
// distance q -> k -> v), the sequence's rows sr, and the lane's place in a 16 x 16 tile (q4, i).  A workgroup past the last
// sequence (the grid is rounded up to 8 sequences) returns.
// Workgroups are dealt round-robin to the 8 XCDs: keep the H heads of a sequence on ONE XCD, back to back, so the
// 128-byte head slices of a token row are fetched together (same DRAM pages, same L2).
// A macro: the same lines as a struct filled by an inline function changed the register counts of 39 of the 48 instantiations
// (the compiler's early passes run before the inliner and see the struct in memory).
#define ATTN_WG_PROLOGUE(p, SC)                                            \
  const int tid = threadIdx.x, lane = tid & 63;                            \
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);               \
  const int xj = blockIdx.x >> 3;                                          \
  const int seq = (xj / p.H) * 8 + (blockIdx.x & 7), h = xj % p.H;         \
  if (seq >= p.nseq) return;                                               \
  const int S = SC ? SC : p.mp.S;                                          \
  const int HD = p.H * PVRL_HEAD_DIM;                                      \
  const SeqRows sr = seq_rows(p.mp, seq);                                  \
  const int q4 = lane >> 4, i = lane & 15

// ------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------
template <int NKT, bool GEN, int NW, int SC = 0>
__global__ __launch_bounds__(64 * NW, NKT > 13 ? 2 : (NW + 1) / 2) void attn_fwd_kernel(AttnArgs p) {
  constexpr int NKS2 = (NKT + 1) / 2;
  constexpr int BL = NKS2 * 32 * 128;
  __shared__ __attribute__((aligned(16))) char smem[2 * BL];
  char* Kb = smem;
  char* Vb = smem + BL;
  ATTN_WG_PROLOGUE(p, SC);
  constexpr int MAXT = (NKT + NW - 1) / NW;   // query tiles per wave
  const int nqt = (S + 15) >> 4;
  // every global load of the workgroup goes out before the first wait: this wave's query fragments, then K and V
  opx8 qf[MAXT][2];
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    const int query = (wave + t * NW) * 16 + i;
    const int qrow = query < S ? query : S - 1;
    const op_t* qp = p.qkv + row_of(sr, qrow) * p.ld + h * 64 + q4 * 8;
    row_frags(qp, qf[t][0], qf[t][1]);
  }
  {
    TileRegs<64 * NW, NKS2 * 32> kr, vr;
    tile_issue<64 * NW, NKS2 * 32>(kr, p.qkv, p.ld, HD + h * 64, sr, S, nullptr, tid);
    tile_issue<64 * NW, NKS2 * 32>(vr, p.qkv, p.ld, 2 * HD + h * 64, sr, S, nullptr, tid);
    tile_commit<64 * NW, NKS2 * 32>(kr, Kb, tid);
    tile_commit<64 * NW, NKS2 * 32>(vr, Vb, tid);
  }
  __syncthreads();

  const unsigned long long pbits = pad_bits_q<NKT, GEN>(p, seq, q4);
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    const int qt = wave + t * NW;
    if (qt >= nqt) break;
    const int query = qt * 16 + i;
    const opx8 qf0 = qf[t][0], qf1 = qf[t][1];

    f32x4 sc[NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      const int krow = kt * 16 + i;
      const opx8 k0 = bl_row_frag(Kb, krow, q4);
      const opx8 k1 = bl_row_frag(Kb, krow, 4 + q4);
      f32x4 a = (f32x4){0.f, 0.f, 0.f, 0.f};
      a = MFMA_16x16x32(k0, qf0, a, 0, 0, 0);
      sc[kt] = MFMA_16x16x32(k1, qf1, a, 0, 0, 0);
      if (NKT > 5 && (kt & 1)) __builtin_amdgcn_sched_barrier(0);   // keep the fragment look-ahead (and VGPRs) bounded
    }
    // softmax over the lane's 4*NKT keys.  exp(scale*s - max) is evaluated as exp2(fma(s, c, -max*c)) with
    // c = scale*log2(e) (one FMA + one v_exp per element); P stays un-normalised (<= 1) and the 16 output values are
    // scaled by 1/sum instead of the 4*NKT probabilities.  Only tiles that can hold masked keys pay for the select.
    const float c = p.scale * LOG2E;
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kt * 16 + 4 * q4 + r;
        if (GEN || kt * 16 + 15 >= S) {
          bool msk = key >= S;
          if constexpr (GEN) msk = msk || ((pbits >> (kt * 4 + r)) & 1ull) || (p.causal && key > query);
          if (msk) sc[kt][r] = -INFINITY;
        }
        mx = fmaxf(mx, sc[kt][r]);
      }
    mx = q4_max(mx);
    const float mref = (mx == -INFINITY) ? 0.f : mx;      // raw-score maximum (scale > 0)
    const float mc = mref * c;
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __builtin_amdgcn_exp2f(fmaf(sc[kt][r], c, -mc));
        sc[kt][r] = e;
        sum += e;
      }
    sum = q4_sum(sum);
    const float inv = sum > 0.f ? 1.0f / sum : 0.f;

    f32x4 oacc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oacc[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks2 = 0; ks2 < NKS2; ++ks2) {
      opx8 pf;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pf[r] = (op_t)sc[2 * ks2][r];
        if (2 * ks2 + 1 < NKT) pf[4 + r] = (op_t)sc[(2 * ks2 + 1 < NKT) ? 2 * ks2 + 1 : 0][r];
        else pf[4 + r] = (op_t)0.f;
      }
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const opx8 vf = bl_frag(Vb, ks2, dt, lane);
        oacc[dt] = MFMA_16x16x32(vf, pf, oacc[dt], 0, 0, 0);
      }
      if (NKT > 5) __builtin_amdgcn_sched_barrier(0);
    }
    if (query < S) {
      op_t* op = tok_ptr(p.o, p.o_cls, p.ldo, p.mp, sr, seq, query) + h * 64 + 4 * q4;
      store_acc(op, oacc, inv);
      if (q4 == 0 && p.lse) p.lse[((long)seq * p.H + h) * S + query] = mref * p.scale + __logf(sum);
    }
  }
}

// ------------------------------------------------------------------------------------------
// backward, pass 1: dQ (and D = rowsum(dO * O)); waves own query tiles exactly as in the forward.
// ------------------------------------------------------------------------------------------
template <int NKT, bool GEN, int NW, int SC = 0>
__global__ __launch_bounds__(64 * NW, NKT > 13 ? 2 : (NW + 1) / 2) void attn_bwd_q_kernel(AttnArgs p) {
  constexpr int NKS2 = (NKT + 1) / 2;
  constexpr int BL = NKS2 * 32 * 128;
  __shared__ __attribute__((aligned(16))) char smem[2 * BL];
  char* Kb = smem;
  char* Vb = smem + BL;
  ATTN_WG_PROLOGUE(p, SC);
  constexpr int MAXT = (NKT + NW - 1) / NW;   // query tiles per wave
  const int nqt = (S + 15) >> 4;
  const float c = p.scale * LOG2E;
  // every global load of the workgroup goes out before the first wait: q / dO / O / lse of this wave's query tiles,
  // then the K and V head slices
  opx8 qf[MAXT][2], df[MAXT][2];
  float lse2[MAXT], dss[MAXT];
  {
    opx8 of[MAXT][2];
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      const int query = (wave + t * NW) * 16 + i;
      const int qj = query < S ? query : S - 1;
      const op_t* qp = p.qkv + row_of(sr, qj) * p.ld + h * 64 + q4 * 8;
      row_frags(qp, qf[t][0], qf[t][1]);
      const op_t* dop = tok_ptr(p.d_o, p.d_o_cls, p.ldo, p.mp, sr, seq, qj) + h * 64 + q4 * 8;
      row_frags(dop, df[t][0], df[t][1]);
      const op_t* ofp = tok_ptr(p.ofw, p.ofw_cls, p.ldo, p.mp, sr, seq, qj) + h * 64 + q4 * 8;
      row_frags(ofp, of[t][0], of[t][1]);
      lse2[t] = p.lse[((long)seq * p.H + h) * S + qj] * LOG2E;
    }
    TileRegs<64 * NW, NKS2 * 32> kr, vr;
    tile_issue<64 * NW, NKS2 * 32>(kr, p.qkv, p.ld, HD + h * 64, sr, S, nullptr, tid);
    tile_issue<64 * NW, NKS2 * 32>(vr, p.qkv, p.ld, 2 * HD + h * 64, sr, S, nullptr, tid);
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      float dsum = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) dsum += (float)df[t][0][e] * (float)of[t][0][e] + (float)df[t][1][e] * (float)of[t][1][e];
      dsum = q4_sum(dsum);
      dss[t] = dsum * p.scale;
      const int query = (wave + t * NW) * 16 + i;
      if (q4 == 0 && query < S) p.dvec[((long)seq * p.H + h) * S + query] = dsum;
    }
    tile_commit<64 * NW, NKS2 * 32>(kr, Kb, tid);
    tile_commit<64 * NW, NKS2 * 32>(vr, Vb, tid);
  }
  __syncthreads();

  const unsigned long long pbits = pad_bits_q<NKT, GEN>(p, seq, q4);
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    const int qt = wave + t * NW;
    if (qt >= nqt) break;
    const int query = qt * 16 + i;
    const opx8 qf0 = qf[t][0], qf1 = qf[t][1], df0 = df[t][0], df1 = df[t][1];
    const float lse2_t = lse2[t], dss_t = dss[t];

    // dS for two 16-key tiles at a time, consumed at once by the dQ MFMAs: nothing but dq[] lives across iterations
    f32x4 dq[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks2 = 0; ks2 < NKS2; ++ks2) {
      opx8 sf;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int kt = 2 * ks2 + half;
        if (kt >= NKT) {
#pragma unroll
          for (int r = 0; r < 4; ++r) sf[4 * half + r] = (op_t)0.f;
          continue;
        }
        f32x4 s, dp;
        s_dp_tile(Kb, Vb, kt * 16 + i, q4, qf0, qf1, df0, df1, s, dp);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kt * 16 + 4 * q4 + r;
          float pr = p_from_lse(s[r], c, lse2_t);
          // (a padded query, query >= S, needs no mask: its lane's dS only feeds that lane's own dq, which is never stored)
          if (GEN || kt * 16 + 15 >= S) {
            bool msk = key >= S || (GEN && query >= S);
            if constexpr (GEN) msk = msk || ((pbits >> (kt * 4 + r)) & 1ull) || (p.causal && key > query);
            if (msk) pr = 0.f;
          }
          sf[4 * half + r] = (op_t)ds_of(pr, dp[r], p.scale, dss_t);
        }
      }
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const opx8 kf = bl_frag(Kb, ks2, dt, lane);
        dq[dt] = MFMA_16x16x32(kf, sf, dq[dt], 0, 0, 0);
      }
      if (NKT > 5) __builtin_amdgcn_sched_barrier(0);
    }
    if (query < S) {
      op_t* op = tok_ptr(p.dqkv, p.dqkv_cls, p.ldd, p.mp, sr, seq, query) + h * 64 + 4 * q4;
      store_acc(op, dq);
    }
  }
}

// ------------------------------------------------------------------------------------------
// backward, pass 2: dK and dV.  Waves own KEY tiles; the query dimension is the MFMA reduction.
// Needs lse and dvec from the forward / pass 1.
// ------------------------------------------------------------------------------------------
template <int NKT, bool GEN, int NW, int SC = 0>
__global__ __launch_bounds__(64 * NW, NKT > 13 ? 2 : (NW + 1) / 2) void attn_bwd_kv_kernel(AttnArgs p) {
  constexpr int NKS2 = (NKT + 1) / 2;
  constexpr int ROWS = NKS2 * 32;
  constexpr int T = ROWS * 128;
  __shared__ __attribute__((aligned(16))) char smem[2 * T + 2 * ROWS * 4];
  char* Qb = smem;
  char* Db = smem + T;
  float* lse_s = reinterpret_cast<float*>(smem + 2 * T);
  float* dv_s = lse_s + ROWS;
  ATTN_WG_PROLOGUE(p, SC);
  constexpr int MAXT = (NKT + NW - 1) / NW;   // key tiles per wave
  const float c = p.scale * LOG2E;
  const int nkt_rt = (S + 15) >> 4;
  // every global load of the workgroup goes out before the first wait: this wave's K / V fragments, then Q and dO
  opx8 kf[MAXT][2], vf[MAXT][2];
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    const int key = (wave + t * NW) * 16 + i;
    const int kj = key < S ? key : S - 1;
    const op_t* kp = p.qkv + row_of(sr, kj) * p.ld + HD + h * 64 + q4 * 8;
    row_frags(kp, kf[t][0], kf[t][1]);
    row_frags(kp + HD, vf[t][0], vf[t][1]);
  }
  {
    const op_t* src0 = p.mp.mode == 1 ? p.d_o_cls + (long)seq * p.ldo : nullptr;   // dO of token 0 lives in the side buffer
    TileRegs<64 * NW, ROWS> qr, dr;
    tile_issue<64 * NW, ROWS>(qr, p.qkv, p.ld, h * 64, sr, S, nullptr, tid);
    tile_issue<64 * NW, ROWS>(dr, p.d_o, p.ldo, h * 64, sr, S, src0, tid);
    for (int idx = tid; idx < ROWS; idx += 64 * NW) {
      const long stat = ((long)seq * p.H + h) * S + idx;
      lse_s[idx] = idx < S ? p.lse[stat] * LOG2E : 0.f;
      dv_s[idx] = idx < S ? p.dvec[stat] * p.scale : 0.f;
    }
    tile_commit<64 * NW, ROWS>(qr, Qb, tid);
    tile_commit<64 * NW, ROWS>(dr, Db, tid);
  }
  __syncthreads();

#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    const int kt = wave + t * NW;
    if (kt >= nkt_rt) break;
    const int key = kt * 16 + i;
    const int kj = key < S ? key : S - 1;
    const opx8 kf0 = kf[t][0], kf1 = kf[t][1], vf0 = vf[t][0], vf1 = vf[t][1];
    bool kbad = key >= S;
    if constexpr (GEN) kbad = kbad || (p.kpm ? (p.kpm[(long)seq * S + kj] != 0) : false);

    f32x4 dk[4], dv[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) { dk[dt] = (f32x4){0.f, 0.f, 0.f, 0.f}; dv[dt] = (f32x4){0.f, 0.f, 0.f, 0.f}; }

#pragma unroll 1
    for (int u = 0; u < NKS2; ++u) {
      opx8 pf, sf;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        // (spelt out, not s_dp_tile: through the helper the NKT = 3 instantiations lose one s_movk_i32 and one s_waitcnt)
        const int qrow = (2 * u + half) * 16 + i;   // a-operand row: query
        const opx8 a0 = bl_row_frag(Qb, qrow, q4);
        const opx8 a1 = bl_row_frag(Qb, qrow, 4 + q4);
        const opx8 d0 = bl_row_frag(Db, qrow, q4);
        const opx8 d1 = bl_row_frag(Db, qrow, 4 + q4);
        f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f};
        s = MFMA_16x16x32(a0, kf0, s, 0, 0, 0);
        s = MFMA_16x16x32(a1, kf1, s, 0, 0, 0);
        f32x4 dp = (f32x4){0.f, 0.f, 0.f, 0.f};
        dp = MFMA_16x16x32(d0, vf0, dp, 0, 0, 0);
        dp = MFMA_16x16x32(d1, vf1, dp, 0, 0, 0);
        // s[r] = S[query = (2u+half)*16 + 4*q4 + r][key]
        const int qb = (2 * u + half) * 16 + 4 * q4;
        const f32x4 l4 = *reinterpret_cast<const f32x4*>(lse_s + qb);   // lse * log2(e)
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(dv_s + qb);    // D * scale
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int query = qb + r;
          bool msk = query >= S || kbad;
          if constexpr (GEN) msk = msk || (p.causal && key > query);
          const float pr = msk ? 0.f : p_from_lse(s[r], c, l4[r]);
          pf[half * 4 + r] = (op_t)pr;
          sf[half * 4 + r] = (op_t)ds_of(pr, dp[r], p.scale, d4[r]);
        }
      }
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const opx8 qtf = bl_frag(Qb, u, dt, lane);
        const opx8 dtf = bl_frag(Db, u, dt, lane);
        dk[dt] = MFMA_16x16x32(qtf, sf, dk[dt], 0, 0, 0);
        dv[dt] = MFMA_16x16x32(dtf, pf, dv[dt], 0, 0, 0);
      }
    }
    if (key < S) {
      op_t* op = tok_ptr(p.dqkv, p.dqkv_cls, p.ldd, p.mp, sr, seq, key) + HD + h * 64 + 4 * q4;
      store_acc2(op, dk, op + HD, dv);
    }
  }
}

int check_common(const AttnArgs& p) {
  if (!p.qkv || p.H <= 0 || p.nseq < 0 || p.mp.S <= 0 || p.mp.S > ATT_ROWS_LONG) return PVRL_EINVAL;
  if ((p.ld % 8)) return PVRL_EINVAL;
  if (p.mp.mode == 1 && (p.mp.T <= 0 || (p.nseq % p.mp.T))) return PVRL_EINVAL;
  if ((p.causal || p.kpm) && p.mp.S > ATT_ROWS) return PVRL_EINVAL;      // the masked forms keep their key bits in one 64-bit word per 16 tiles
  return PVRL_OK;
}

// run-time (S, masks) -> the instantiation of the three kernels that serves them: with_inst calls f(Inst<NKT, GEN, NW, SC>{})
template <int NKT, bool GEN, int NW, int SC>
struct Inst {};

// The two sequence lengths of the TimeSformer path at its benchmark geometry -- 197 (196 patches + cls, spatial) and 32 (temporal,
// long clips) -- are instantiated with S as a compile-time constant: `key >= S` is then false for every key tile but the last
// (none at S = 32), so 12 of 13 tiles lose their per-score compare + select, and the 52 64-bit lane masks that spilled the
// kernels' scalar registers into v_writelane / v_readlane pairs (SGPR spills 66 / 58 -> 0) disappear with them.
template <int NKT, int NW, typename F>
int with_form(const AttnArgs& p, F&& f) {
  constexpr int SFIX = NKT == 13 ? 197 : NKT == 2 ? 32 : 0;
  if (p.causal || p.kpm) return f(Inst<NKT, true, NW, 0>{});
  if (SFIX && p.mp.S == SFIX) return f(Inst<NKT, false, NW, SFIX>{});
  return f(Inst<NKT, false, NW, 0>{});
}
template <typename F>
int with_inst(int64_t S, const AttnArgs& p, F&& f) {
  if (S <= 16) return with_form<1, 4>(p, f);
  if (S <= 32) return with_form<2, 4>(p, f);
  if (S <= 48) return with_form<3, 4>(p, f);
  if (S <= 80) return with_form<5, 4>(p, f);
  if (S <= 208) return with_form<13, 8>(p, f);
  // longer crops (256^2 -> 257 tokens, 320^2 -> 401): the same kernels with more key tiles, one 8-wave workgroup per CU
  if (S <= 272) return with_form<17, 8>(p, f);
  return with_form<26, 8>(p, f);
}

template <int NKT, bool GEN, int NW, int SC>
int launch_fwd(Inst<NKT, GEN, NW, SC>, const AttnArgs& p, hipStream_t s) {
  const dim3 grid((unsigned)(8 * ((p.nseq + 7) / 8) * p.H)), blk(64 * NW);
  hipLaunchKernelGGL((attn_fwd_kernel<NKT, GEN, NW, SC>), grid, blk, 0, s, p);
  PVRL_LAUNCH_CHECK();
  return PVRL_OK;
}

template <int NKT, bool GEN, int NW, int SC>
int launch_bwd(Inst<NKT, GEN, NW, SC>, const AttnArgs& p, hipStream_t s) {
  const dim3 grid((unsigned)(8 * ((p.nseq + 7) / 8) * p.H)), blk(64 * NW);
  hipLaunchKernelGGL((attn_bwd_q_kernel<NKT, GEN, NW, SC>), grid, blk, 0, s, p);
  PVRL_LAUNCH_CHECK();
  hipLaunchKernelGGL((attn_bwd_kv_kernel<NKT, GEN, NW, SC>), grid, blk, 0, s, p);
  PVRL_LAUNCH_CHECK();
  return PVRL_OK;
}

}  // namespace

extern "C" int pvrl_attn_fwd(const void* qkv, int64_t ld, int64_t nseq, int64_t S, int64_t H, int mode, int64_t T,
                             int64_t cls_base, float scale, int causal, const void* key_padding_mask, void* o,
                             void* o_cls, int64_t ldo, float* lse, void* stream) {
  const AttnArgs p = attn_args(qkv, ld, nseq, S, H, mode, T, cls_base, scale, causal, key_padding_mask, o, o_cls, ldo, lse);
  if (nseq == 0) return PVRL_OK;
  if (int e = check_common(p)) return e;
  if (!o || (ldo % 4) || (mode == 1 && !o_cls)) return PVRL_EINVAL;
  return with_inst(S, p, [&](auto inst) { return launch_fwd(inst, p, (hipStream_t)stream); });
}

extern "C" int pvrl_attn_bwd(const void* qkv, int64_t ld, int64_t nseq, int64_t S, int64_t H, int mode, int64_t T,
                             int64_t cls_base, float scale, int causal, const void* key_padding_mask, const void* o,
                             const void* o_cls, const void* d_o, const void* d_o_cls, int64_t ldo, const float* lse,
                             float* dvec, void* dqkv, void* dqkv_cls, int64_t ldd, void* stream) {
  const AttnArgs p = attn_args_bwd(qkv, ld, nseq, S, H, mode, T, cls_base, scale, causal, key_padding_mask, o, o_cls, d_o, d_o_cls,
                                   ldo, lse, dvec, dqkv, dqkv_cls, ldd);
  if (nseq == 0) return PVRL_OK;
  if (int e = check_common(p)) return e;
  if (!o || !d_o || !lse || !dvec || !dqkv || (ldo % 8) || (ldd % 4)) return PVRL_EINVAL;
  if (mode == 1 && (!o_cls || !d_o_cls || !dqkv_cls)) return PVRL_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (pvrl_attn_bwd_fused_ok(p)) return pvrl_attn_bwd_fused_launch(p, s);
  if (pvrl_attn_bwd_s32_ok(p)) return pvrl_attn_bwd_s32_launch(p, s);
  return with_inst(S, p, [&](auto inst) { return launch_bwd(inst, p, s); });
}
