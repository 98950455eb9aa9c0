// Long-sequence multi-head self-attention (head_dim 64, no masks) on MFMA, forward + backward, 1 <= S <= 8192 tokens.
//
// Reference semantics: Attention.forward, lib/models/vit.py:75-92, as the `joint_space_time` and `space_only` schemes of
// Block.forward use it (vit.py:124-127): ONE sequence of 1 + N*T tokens per clip (8 x 224^2: 1,569; 32 x 224^2: 6,273).
// attn_mfma.hip keeps a sequence's whole K and V in LDS and stops at 416 tokens; here K / V (forward, dQ) or Q / dO (dK / dV) are
// STREAMED through LDS in tiles of KT = 64 rows, double-buffered: the loads of tile t + 1 are issued before the math of tile t and
// committed to the other buffer after it, one barrier per tile.  A workgroup of 8 waves owns QT = 128 rows of one (sequence, head),
// a wave 16 of them.  MFMA operands are "swapped" exactly as in attn_mfma.hip (a = streamed rows, b = the wave's own rows), so a lane
// owns ONE query (forward, dQ) or ONE key (dK / dV) and the same blocked LDS image serves row-wise and transposed fragment reads.
//
// Forward: online softmax.  Scores are kept in log2 units (t = s * scale * log2(e)); per key tile m' = max(m, max t), the running sum
// l and the 16 accumulators of the lane are multiplied by 2^(m - m') (always, right before the tile's P.V products: nothing is pending
// across the decision, so there is no stale factor), P = 2^(t - m') is rounded to the operand type only as the b-operand of the second
// product and summed unrounded.  Keys past S in the ragged last tile are set to -inf BEFORE the maximum; every tile holds at least
// one real key, so m' is finite from the first tile on and 2^(-inf - m') = 0 starts the recurrence.  Queries past S are computed on
// a clamped row and not stored.  lse = m ln 2 + log l.
// Backward: deterministic, two kernels, P recomputed from lse.  attn_long_bwd_q_kernel owns a query block, sweeps the key tiles for dQ and
// writes D = rowsum(dO * O) to the workspace; attn_long_bwd_kv_kernel owns a key block and sweeps the query tiles for dK and dV.  S and dP
// are formed in both: seven MFMA products against the five of a fused backward, and no atomics or hand-off between workgroups.
#include "attn_common.h"
#include "../../include/pvrl.h"

namespace {

constexpr int KT = PVRL_ATTN_LONG_KT;    // rows of a streamed tile
constexpr int QT = PVRL_ATTN_LONG_QT;    // rows a workgroup owns
constexpr int NW = QT / 16;              // waves per workgroup
constexpr int NT = 64 * NW;
constexpr int TILE = KT * 128;           // bytes of one blocked [KT][64] tile
static_assert(KT == 64 && KT * 8 == NT, "one 16-byte chunk per thread and tile; the tile loops below are written for 4 sub-tiles of 16 rows");

// A streamed tile is one 16-byte chunk per thread: chunk_load (attn_common.h) of row r0 + (tid >> 3), chunk tid & 7, put into the
// blocked image by chunk_store.
__device__ __forceinline__ void chunk_store(char* tile, const u32x4& v, int tid) {
  *reinterpret_cast<u32x4*>(tile + bl_off(tid >> 3, (tid & 7) * 8)) = v;
}

struct Item { int seq, h, blk; };
__device__ __forceinline__ Item item_of(const AttnArgs& p, int nblk) {
  // consecutive workgroups walk the row blocks of one (sequence, head), then its other heads: the streamed K / V (Q / dO) slices
  // of a token row are fetched together
  const unsigned b = blockIdx.x;
  Item it;
  it.blk = (int)(b % (unsigned)nblk);
  const unsigned sh = b / (unsigned)nblk;
  it.h = (int)(sh % (unsigned)p.H);
  it.seq = (int)(sh / (unsigned)p.H);
  return it;
}

// What the three kernels know before they touch data: tid / lane / wave (wave-uniform), S, HD = H * 64 (the column distance
// q -> k -> v), the workgroup's (seq, h) and the sequence's rows sr, the lane's place in a 16 x 16 tile (q4, i), its own row ROW
// (a query in the forward and dQ, a key in dK / dV), the number NTILES of streamed tiles, c = scale * log2(e), and this thread's
// chunk of a streamed tile (row crow, 16-byte chunk cc).  `live` is wave-uniform: a wave past the sequence still loads and meets
// the barriers.  (A macro for the reason given in attn_mfma.hip, ATTN_WG_PROLOGUE.)
#define ATTN_LONG_PROLOGUE(p, ROW, NTILES)                          \
  const int tid = threadIdx.x, lane = tid & 63;                     \
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);        \
  const int S = p.mp.S, HD = p.H * PVRL_HEAD_DIM;                   \
  const Item it = item_of(p, (S + QT - 1) / QT);                    \
  const int seq = it.seq, h = it.h;                                 \
  const SeqRows sr = seq_rows(p.mp, seq);                           \
  const int q4 = lane >> 4, i = lane & 15;                          \
  const int row0 = it.blk * QT + wave * 16;                         \
  const int ROW = row0 + i;                                         \
  const bool live = row0 < S;                                       \
  const int NTILES = (S + KT - 1) / KT;                             \
  const float c = p.scale * LOG2E;                                  \
  const int crow = tid >> 3, cc = tid & 7

// ------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT, 2) void attn_long_fwd_kernel(AttnArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE];   // [buffer][K | V]
  ATTN_LONG_PROLOGUE(p, query, nkt);

  const op_t* qp = p.qkv + row_of(sr, min(query, S - 1)) * p.ld + h * 64 + q4 * 8;
  opx8 qf0, qf1;
  row_frags(qp, qf0, qf1);
  u32x4 kr = chunk_load(p.qkv, p.ld, HD + h * 64, sr, S, nullptr, crow, cc);
  u32x4 vr = chunk_load(p.qkv, p.ld, 2 * HD + h * 64, sr, S, nullptr, crow, cc);
  chunk_store(smem, kr, tid);
  chunk_store(smem + TILE, vr, tid);
  __syncthreads();

  float m = -INFINITY, l = 0.f;
  f32x4 oacc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) oacc[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int kt = 0; kt < nkt; ++kt) {
    const char* Kb = smem + (kt & 1) * 2 * TILE;
    const char* Vb = Kb + TILE;
    char* nxt = smem + ((kt + 1) & 1) * 2 * TILE;
    // the next tile's loads fly under this tile's math (past the last tile: clamped rows, zeros, never read)
    kr = chunk_load(p.qkv, p.ld, HD + h * 64, sr, S, nullptr, (kt + 1) * KT + crow, cc);
    vr = chunk_load(p.qkv, p.ld, 2 * HD + h * 64, sr, S, nullptr, (kt + 1) * KT + crow, cc);
    if (live) {
      f32x4 sc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const opx8 k0 = bl_row_frag(Kb, j * 16 + i, q4);
        const opx8 k1 = bl_row_frag(Kb, j * 16 + i, 4 + q4);
        f32x4 a = (f32x4){0.f, 0.f, 0.f, 0.f};
        a = MFMA_16x16x32(k0, qf0, a, 0, 0, 0);
        sc[j] = MFMA_16x16x32(k1, qf1, a, 0, 0, 0);
      }
      const int kbase = kt * KT;
      const bool ragged = kbase + KT > S;
      float tmax = -INFINITY;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float t = sc[j][r] * c;
          if (ragged && kbase + j * 16 + 4 * q4 + r >= S) t = -INFINITY;
          sc[j][r] = t;
          tmax = fmaxf(tmax, t);
        }
      tmax = q4_max(tmax);
      const float mn = fmaxf(m, tmax);
      const float alpha = __builtin_amdgcn_exp2f(m - mn);
      float psum = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = __builtin_amdgcn_exp2f(sc[j][r] - mn);
          sc[j][r] = e;
          psum += e;
        }
      psum = q4_sum(psum);
      l = fmaf(l, alpha, psum);
      m = mn;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) oacc[dt] *= alpha;
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2) {
        opx8 pf;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          pf[r] = (op_t)sc[2 * ks2][r];
          pf[4 + r] = (op_t)sc[2 * ks2 + 1][r];
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const opx8 vf = bl_frag(Vb, ks2, dt, lane);
          oacc[dt] = MFMA_16x16x32(vf, pf, oacc[dt], 0, 0, 0);
        }
      }
    }
    chunk_store(nxt, kr, tid);
    chunk_store(nxt + TILE, vr, tid);
    __syncthreads();
  }

  if (query < S) {
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    op_t* op = tok_ptr(p.o, p.o_cls, p.ldo, p.mp, sr, seq, query) + h * 64 + 4 * q4;
    // (spelt out, not store_acc: through the helper the compiler orders this kernel's instructions differently)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      opx4 ov;
#pragma unroll
      for (int r = 0; r < 4; ++r) ov[r] = (op_t)(oacc[dt][r] * inv);
      *reinterpret_cast<opx4*>(op + 16 * dt) = ov;
    }
    if (q4 == 0 && p.lse) p.lse[((long)seq * p.H + h) * S + query] = fmaf(m, 0.6931471805599453f, __logf(l));
  }
}

// ------------------------------------------------------------------------------------------
// backward, query blocks: dQ and D = rowsum(dO * O); K and V streamed
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT, 2) void attn_long_bwd_q_kernel(AttnArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE];   // [buffer][K | V]
  ATTN_LONG_PROLOGUE(p, query, nkt);
  const int qj = min(query, S - 1);

  const op_t* qp = p.qkv + row_of(sr, qj) * p.ld + h * 64 + q4 * 8;
  opx8 qf0, qf1;
  row_frags(qp, qf0, qf1);
  const op_t* dop = tok_ptr(p.d_o, p.d_o_cls, p.ldo, p.mp, sr, seq, qj) + h * 64 + q4 * 8;
  opx8 df0, df1;
  row_frags(dop, df0, df1);
  const op_t* ofp = tok_ptr(p.ofw, p.ofw_cls, p.ldo, p.mp, sr, seq, qj) + h * 64 + q4 * 8;
  opx8 of0, of1;
  row_frags(ofp, of0, of1);
  const long stat = ((long)seq * p.H + h) * S;
  const float lse2 = p.lse[stat + qj] * LOG2E;
  u32x4 kr = chunk_load(p.qkv, p.ld, HD + h * 64, sr, S, nullptr, crow, cc);
  u32x4 vr = chunk_load(p.qkv, p.ld, 2 * HD + h * 64, sr, S, nullptr, crow, cc);
  float dsum = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) dsum += (float)df0[e] * (float)of0[e] + (float)df1[e] * (float)of1[e];
  dsum = q4_sum(dsum);
  const float dss = dsum * p.scale;
  if (q4 == 0 && query < S) p.dvec[stat + query] = dsum;
  chunk_store(smem, kr, tid);
  chunk_store(smem + TILE, vr, tid);
  __syncthreads();

  f32x4 dq[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dq[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int kt = 0; kt < nkt; ++kt) {
    const char* Kb = smem + (kt & 1) * 2 * TILE;
    const char* Vb = Kb + TILE;
    char* nxt = smem + ((kt + 1) & 1) * 2 * TILE;
    kr = chunk_load(p.qkv, p.ld, HD + h * 64, sr, S, nullptr, (kt + 1) * KT + crow, cc);
    vr = chunk_load(p.qkv, p.ld, 2 * HD + h * 64, sr, S, nullptr, (kt + 1) * KT + crow, cc);
    if (live) {
      const int kbase = kt * KT;
      const bool ragged = kbase + KT > S;
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2) {
        opx8 sf;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          f32x4 s, dp;
          s_dp_tile(Kb, Vb, (2 * ks2 + half) * 16 + i, q4, qf0, qf1, df0, df1, s, dp);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float pr = p_from_lse(s[r], c, lse2);
            if (ragged && kbase + (2 * ks2 + half) * 16 + 4 * q4 + r >= S) pr = 0.f;
            sf[4 * half + r] = (op_t)ds_of(pr, dp[r], p.scale, dss);
          }
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const opx8 kf = bl_frag(Kb, ks2, dt, lane);
          dq[dt] = MFMA_16x16x32(kf, sf, dq[dt], 0, 0, 0);
        }
      }
    }
    chunk_store(nxt, kr, tid);
    chunk_store(nxt + TILE, vr, tid);
    __syncthreads();
  }

  if (query < S) {
    op_t* op = tok_ptr(p.dqkv, p.dqkv_cls, p.ldd, p.mp, sr, seq, query) + h * 64 + 4 * q4;
    store_acc(op, dq);
  }
}

// ------------------------------------------------------------------------------------------
// backward, key blocks: dK and dV; Q, dO, lse and D streamed.  Runs after attn_long_bwd_q_kernel on the same stream (D).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT, 2) void attn_long_bwd_kv_kernel(AttnArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE + 4 * KT * 4];   // [buffer][Q | dO], then [buffer][lse | D]
  float* stats = reinterpret_cast<float*>(smem + 4 * TILE);
  ATTN_LONG_PROLOGUE(p, key, nqt);
  const long stat = ((long)seq * p.H + h) * S;
  const op_t* src0 = p.mp.mode == 1 ? p.d_o_cls + (long)seq * p.ldo : nullptr;   // dO of token 0 lives in the side buffer

  const op_t* kp = p.qkv + row_of(sr, min(key, S - 1)) * p.ld + HD + h * 64 + q4 * 8;
  opx8 kf0, kf1, vf0, vf1;
  row_frags(kp, kf0, kf1);
  row_frags(kp + HD, vf0, vf1);

  // threads 0..63 carry lse * log2(e), threads 64..127 D * scale of the tile's 64 queries (zeros past the sequence)
  const int srow = tid & 63;
  const bool is_lse = tid < 64, has_stat = tid < 128;
  auto stat_load = [&](int r0) -> float {
    const int q = r0 + srow;
    const long idx = stat + min(q, S - 1);
    const float v = is_lse ? p.lse[idx] * LOG2E : p.dvec[idx] * p.scale;
    return q < S ? v : 0.f;
  };
  u32x4 qr = chunk_load(p.qkv, p.ld, h * 64, sr, S, nullptr, crow, cc);
  u32x4 dr = chunk_load(p.d_o, p.ldo, h * 64, sr, S, src0, crow, cc);
  float st = has_stat ? stat_load(0) : 0.f;
  chunk_store(smem, qr, tid);
  chunk_store(smem + TILE, dr, tid);
  if (has_stat) stats[tid] = st;
  __syncthreads();

  f32x4 dk[4], dv[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) { dk[dt] = (f32x4){0.f, 0.f, 0.f, 0.f}; dv[dt] = (f32x4){0.f, 0.f, 0.f, 0.f}; }

  for (int qt = 0; qt < nqt; ++qt) {
    const char* Qb = smem + (qt & 1) * 2 * TILE;
    const char* Db = Qb + TILE;
    const float* lse_s = stats + (qt & 1) * 2 * KT;
    const float* dv_s = lse_s + KT;
    char* nxt = smem + ((qt + 1) & 1) * 2 * TILE;
    qr = chunk_load(p.qkv, p.ld, h * 64, sr, S, nullptr, (qt + 1) * KT + crow, cc);
    dr = chunk_load(p.d_o, p.ldo, h * 64, sr, S, src0, (qt + 1) * KT + crow, cc);
    st = has_stat ? stat_load((qt + 1) * KT) : 0.f;
    if (live) {
      const int qbase = qt * KT;
      const bool ragged = qbase + KT > S;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        opx8 pf, sf;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          f32x4 s, dp;
          s_dp_tile(Qb, Db, (2 * u + half) * 16 + i, q4, kf0, kf1, vf0, vf1, s, dp);   // a-operand rows: queries
          // s[r] = S[query = qbase + (2u + half) * 16 + 4 * q4 + r][key]
          const int qb = (2 * u + half) * 16 + 4 * q4;
          const f32x4 l4 = *reinterpret_cast<const f32x4*>(lse_s + qb);   // lse * log2(e)
          const f32x4 d4 = *reinterpret_cast<const f32x4*>(dv_s + qb);    // D * scale
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float pr = p_from_lse(s[r], c, l4[r]);
            if (ragged && qbase + qb + r >= S) pr = 0.f;
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
    }
    chunk_store(nxt, qr, tid);
    chunk_store(nxt + TILE, dr, tid);
    if (has_stat) stats[((qt + 1) & 1) * 2 * KT + tid] = st;
    __syncthreads();
  }

  if (key < S) {
    op_t* op = tok_ptr(p.dqkv, p.dqkv_cls, p.ldd, p.mp, sr, seq, key) + HD + h * 64 + 4 * q4;
    store_acc2(op, dk, op + HD, dv);
  }
}

int check_long(const AttnArgs& p, long* grid) {
  if (!p.qkv || p.H <= 0 || p.nseq < 0 || p.mp.S <= 0 || p.mp.S > PVRL_ATTN_LONG_MAX_S) return PVRL_EINVAL;
  if (p.ld % 8) return PVRL_EINVAL;
  if (p.mp.mode != 0 && p.mp.mode != 1) return PVRL_EINVAL;
  if (p.mp.mode == 1 && (p.mp.T <= 0 || (p.nseq % p.mp.T))) return PVRL_EINVAL;
  *grid = (long)p.nseq * p.H * ((p.mp.S + QT - 1) / QT);
  if (*grid > 0x7fffffffL) return PVRL_EINVAL;
  return PVRL_OK;
}

}  // namespace

extern "C" int pvrl_attn_long_fwd(const void* qkv, int64_t ld, int64_t nseq, int64_t S, int64_t H, int mode, int64_t T,
                                  int64_t cls_base, float scale, void* o, void* o_cls, int64_t ldo, float* lse, void* stream) {
  if (nseq < 0 || nseq > 0x7fffffffL || S < 1 || S > PVRL_ATTN_LONG_MAX_S || H <= 0 || H > 0x7fffffffL || T > 0x7fffffffL)
    return PVRL_EINVAL;
  const AttnArgs p = attn_args(qkv, ld, nseq, S, H, mode, T, cls_base, scale, 0, nullptr, o, o_cls, ldo, lse);
  if (nseq == 0) return PVRL_OK;
  long grid = 0;
  if (int e = check_long(p, &grid)) return e;
  if (!o || (ldo % 4) || (mode == 1 && !o_cls)) return PVRL_EINVAL;
  hipLaunchKernelGGL(attn_long_fwd_kernel, dim3((unsigned)grid), dim3(NT), 0, (hipStream_t)stream, p);
  PVRL_LAUNCH_CHECK();
  return PVRL_OK;
}

extern "C" int64_t pvrl_attn_long_bwd_workspace_bytes(int64_t nseq, int64_t S, int64_t H) {
  if (nseq <= 0 || S <= 0 || H <= 0) return 0;
  return nseq * S * H * (int64_t)sizeof(float);      // D = rowsum(dO * O), [nseq][H][S]
}

extern "C" int pvrl_attn_long_bwd(const void* qkv, int64_t ld, int64_t nseq, int64_t S, int64_t H, int mode, int64_t T,
                                  int64_t cls_base, float scale, const void* o, const void* o_cls, const void* d_o,
                                  const void* d_o_cls, int64_t ldo, const float* lse, void* dqkv, void* dqkv_cls, int64_t ldd,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  if (nseq < 0 || nseq > 0x7fffffffL || S < 1 || S > PVRL_ATTN_LONG_MAX_S || H <= 0 || H > 0x7fffffffL || T > 0x7fffffffL)
    return PVRL_EINVAL;
  const AttnArgs p = attn_args_bwd(qkv, ld, nseq, S, H, mode, T, cls_base, scale, 0, nullptr, o, o_cls, d_o, d_o_cls, ldo, lse,
                                   (float*)workspace, dqkv, dqkv_cls, ldd);
  if (nseq == 0) return PVRL_OK;
  long grid = 0;
  if (int e = check_long(p, &grid)) return e;
  if (!o || !d_o || !lse || !dqkv || (ldo % 8) || (ldd % 4)) return PVRL_EINVAL;
  if (mode == 1 && (!o_cls || !d_o_cls || !dqkv_cls)) return PVRL_EINVAL;
  if (!workspace || workspace_bytes < pvrl_attn_long_bwd_workspace_bytes(nseq, S, H)) return PVRL_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(attn_long_bwd_q_kernel, dim3((unsigned)grid), dim3(NT), 0, s, p);
  PVRL_LAUNCH_CHECK();
  hipLaunchKernelGGL(attn_long_bwd_kv_kernel, dim3((unsigned)grid), dim3(NT), 0, s, p);
  PVRL_LAUNCH_CHECK();
  return PVRL_OK;
}
