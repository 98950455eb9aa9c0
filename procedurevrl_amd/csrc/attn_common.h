// Shared pieces of the MFMA attention kernels (forward, dQ, dK/dV).
//
// Sequence addressing.  The divided space-time attention of the reference
// (lib/models/vit.py:129-151) gathers its sequences with einops rearranges + torch.cat, each a
// full copy of the token tensor.  Here the packed QKV activations stay where the QKV GEMM wrote
// them and the kernels address rows in place:
//   mode 0 (contiguous): row(seq, j) = seq*S + j           -- temporal attention (b h w) t m,
//                                                              order transformer, CLIP text
//   mode 1 (TimeSformer spatial): seq = b*T + t, token 0 is the clip's cls row,
//                                  token j>=1 is patch n=j-1 of frame t:
//            row(seq, 0) = cls_base + b ; row(seq, j) = b*(S-1)*T + (j-1)*T + t
//          outputs for token 0 go to a separate per-(b,t) buffer (the T cls copies of
//          vit.py:139-141 differ after attention and are averaged later, vit.py:147-149).
#pragma once
#include "common.h"
#include "../../include/pvrl.h"

struct SeqMap {
  int mode, S, T;
  long cls_base;
};

constexpr int ATT_MAX_TILES = 13;               // S <= 208
constexpr int ATT_ROWS = ATT_MAX_TILES * 16;    // 208
constexpr int ATT_ROWS_LONG = 26 * 16;          // 416: the long-sequence instantiations of the same kernels (NKT = 17, 26)
static_assert(ATT_ROWS_LONG == PVRL_ATTN_MAX_S, "include/pvrl.h states the limit the callers read");

// row-major [rows][64] bf16 tile with 16-byte chunk swizzle (conflict-free ds_read_b128 fragments)
__device__ __forceinline__ int rm_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
// blocked tile for ds_read_b64_tr_b16: contiguous [4 rows][16 cols] 128-byte blocks
__device__ __forceinline__ int bl_off(int row, int col) {
  const int rb = row >> 2;
  return (rb * 4 + ((col >> 4) ^ (rb & 1))) * 128 + (row & 3) * 32 + (col & 15) * 2;
}

// 8 consecutive columns (16-byte chunk `chunk` of 8) of one row, from the SAME blocked image: with the (cb ^ (rb & 1))
// block swizzle the 16 lanes of every ds_read_b128 group hit 16 distinct 16-byte slots, so one LDS copy of a tile
// serves both the row-wise (a-operand) and the transposed (ds_read_b64_tr_b16) fragment reads.
__device__ __forceinline__ opx8 bl_row_frag(const char* tile, int row, int chunk) {
  return *reinterpret_cast<const opx8*>(tile + bl_off(row, chunk * 8));
}

__device__ __forceinline__ opx8 tr_frag8(const char* tile, int off0, int off1) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(tile + off0));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(tile + off1));
  union { struct { s16x4 a, b; } s; opx8 v; } u;
  u.s.a = lo; u.s.b = hi;
  return u.v;
}

// Transposed fragment for a K=32 MFMA step `ks2` (rows 32*ks2 .. 32*ks2+31 of a blocked tile):
// lane (i = lane&15, q = lane>>4) receives column 16*ct + i at rows {32ks2+4q+0..3, 32ks2+16+4q+0..3}.
__device__ __forceinline__ opx8 bl_frag(const char* tile, int ks2, int ct, int lane) {
  const int q = lane >> 4, i = lane & 15;
  const int rb0 = 8 * ks2 + q, rb1 = rb0 + 4;
  const int o0 = (rb0 * 4 + (ct ^ (rb0 & 1))) * 128 + i * 8;
  const int o1 = (rb1 * 4 + (ct ^ (rb1 & 1))) * 128 + i * 8;
  return tr_frag8(tile, o0, o1);
}

// Per-workgroup view of one sequence: row(j) without per-element integer division.
struct SeqRows {
  long base0;   // row of token 0
  long base1;   // row of token 1
  long stride;  // row distance between tokens j and j+1 (j >= 1)
};
__device__ __forceinline__ SeqRows seq_rows(const SeqMap& mp, int seq) {
  SeqRows r;
  if (mp.mode == 0) {
    r.base0 = (long)seq * mp.S; r.base1 = r.base0 + 1; r.stride = 1;
  } else {
    const int b = seq / mp.T, t = seq - b * mp.T;
    r.base0 = mp.cls_base + b; r.base1 = (long)b * (mp.S - 1) * mp.T + t; r.stride = mp.T;
  }
  return r;
}
__device__ __forceinline__ long row_of(const SeqRows& r, int j) { return j == 0 ? r.base0 : r.base1 + (long)(j - 1) * r.stride; }

// 16-byte chunk `c` (of 8) of row `row` of one head slice [S rows][64] of a packed activation, zeros for rows >= S.  `src0` (optional)
// overrides the source row of token 0 (side buffer of the per-(b,t) cls rows).
// BRANCH-FREE: every lane loads (rows past the sequence re-read its last row) and the padding is zeroed by a select.  A load
// inside `if (row < S)` is followed by s_waitcnt vmcnt(0) at the join: the two guarded iterations of
// a whole-slice load cost the workgroup two extra serial memory round trips in front of its first barrier.
__device__ __forceinline__ u32x4 chunk_load(const op_t* base, long ld, int col0, const SeqRows& sr, int S, const op_t* src0, int row,
                                            int c) {
  const int rc = min(row, S - 1);
  const op_t* src = (rc == 0 && src0) ? src0 : base + row_of(sr, rc) * ld;
  const u32x4 v = *reinterpret_cast<const u32x4*>(src + col0 + c * 8);
  const unsigned keep = row < S ? 0xffffffffu : 0u;
  return v & (u32x4){keep, keep, keep, keep};
}

// kernel arguments shared by attn_mfma.hip (forward, two-pass backward) and attn_bwd_fused.hip
struct AttnArgs {
  const op_t* qkv; long ld;   // packed [rows][3*H*64]: q | k | v, head h at columns h*64
  int H, nseq;
  SeqMap mp;
  float scale;
  int causal;
  const unsigned char* kpm;   // [nseq][S], 1 = key masked, or null
  // forward
  op_t* o; op_t* o_cls; long ldo;
  float* lse;                 // [nseq][H][S]
  // backward
  const op_t* d_o; const op_t* d_o_cls; const op_t* ofw; const op_t* ofw_cls;
  float* dvec;                // [nseq][H][S]  rowsum(dO * O)
  op_t* dqkv; op_t* dqkv_cls; long ldd;   // dqkv_cls: [nseq][3*H*64] partial rows for token 0 (mode 1)
};

// host: AttnArgs from the C arguments of an entry point (include/pvrl.h).  attn_args takes a forward's arguments and leaves the
// backward fields zero; attn_args_bwd takes a backward's (`o` is then the forward's output, `dvec` the D buffer or workspace).
inline AttnArgs attn_args(const void* qkv, int64_t ld, int64_t nseq, int64_t S, int64_t H, int mode, int64_t T, int64_t cls_base,
                          float scale, int causal, const void* key_padding_mask, void* o, void* o_cls, int64_t ldo, float* lse) {
  AttnArgs p = {};
  p.qkv = (const op_t*)qkv; p.ld = ld; p.H = (int)H; p.nseq = (int)nseq;
  p.mp.mode = mode; p.mp.S = (int)S; p.mp.T = (int)T; p.mp.cls_base = cls_base;
  p.scale = scale; p.causal = causal; p.kpm = (const unsigned char*)key_padding_mask;
  p.o = (op_t*)o; p.o_cls = (op_t*)o_cls; p.ldo = ldo; p.lse = lse;
  return p;
}
inline AttnArgs attn_args_bwd(const void* qkv, int64_t ld, int64_t nseq, int64_t S, int64_t H, int mode, int64_t T, int64_t cls_base,
                              float scale, int causal, const void* key_padding_mask, const void* o, const void* o_cls,
                              const void* d_o, const void* d_o_cls, int64_t ldo, const float* lse, float* dvec, void* dqkv,
                              void* dqkv_cls, int64_t ldd) {
  AttnArgs p = attn_args(qkv, ld, nseq, S, H, mode, T, cls_base, scale, causal, key_padding_mask, nullptr, nullptr, ldo,
                         const_cast<float*>(lse));
  p.ofw = (const op_t*)o; p.ofw_cls = (const op_t*)o_cls; p.d_o = (const op_t*)d_o; p.d_o_cls = (const op_t*)d_o_cls;
  p.dvec = dvec; p.dqkv = (op_t*)dqkv; p.dqkv_cls = (op_t*)dqkv_cls; p.ldd = ldd;
  return p;
}

// row pointer helpers for per-token outputs / inputs that keep token 0 in a side buffer (mode 1)
template <typename T>
__device__ __forceinline__ T* tok_ptr(T* tok, T* cls, long ld, const SeqMap& mp, const SeqRows& sr, int seq, int j) {
  if (mp.mode == 1 && j == 0) return cls + (long)seq * ld;
  return tok + row_of(sr, j) * ld;
}

__device__ __forceinline__ unsigned pack_opx2(float a, float b) {
  union { opx2 v; unsigned u; } x;
  x.v[0] = (op_t)a; x.v[1] = (op_t)b;
  return x.u;
}

// ---- lane-level pieces of the head_dim-64 kernels (attn_mfma.hip, attn_long.hip).  MFMA operands are "swapped" (a = rows read from a
// blocked LDS image, b = the wave's own rows), so lane (i = lane & 15, q4 = lane >> 4) owns ONE row of the wave's tile -- a query in
// the forward and dQ, a key in dK / dV -- and elements 4 q4 .. 4 q4 + 3 of each 16 along the other dimension.
constexpr float LOG2E = 1.4426950408889634f;

// the wave's own fragments of a row: 8 columns at p (= row + 8 q4) and 8 at p + 32, the b-operands of the two K = 32 steps over head_dim
__device__ __forceinline__ void row_frags(const op_t* p, opx8& f0, opx8& f1) {
  f0 = *reinterpret_cast<const opx8*>(p);
  f1 = *reinterpret_cast<const opx8*>(p + 32);
}

// maximum / sum over the four lanes (q4 = 0..3) that share a row
__device__ __forceinline__ float q4_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float q4_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// S and dP of one 16-row tile of the blocked images A and B (a-operands; `row` = the tile's first row + i) against the wave's own
// fragments x and y (b-operands): s[r] = A[tile row 4 q4 + r] . x[the lane's row], dp[r] = B[same row] . y[the lane's row].
// Statement order as it stood in the kernels: four fragment reads, then the four products.
__device__ __forceinline__ void s_dp_tile(const char* A, const char* B, int row, int q4, opx8 x0, opx8 x1, opx8 y0, opx8 y1, f32x4& s,
                                          f32x4& dp) {
  const opx8 a0 = bl_row_frag(A, row, q4);
  const opx8 a1 = bl_row_frag(A, row, 4 + q4);
  const opx8 b0 = bl_row_frag(B, row, q4);
  const opx8 b1 = bl_row_frag(B, row, 4 + q4);
  s = (f32x4){0.f, 0.f, 0.f, 0.f};
  s = MFMA_16x16x32(a0, x0, s, 0, 0, 0);
  s = MFMA_16x16x32(a1, x1, s, 0, 0, 0);
  dp = (f32x4){0.f, 0.f, 0.f, 0.f};
  dp = MFMA_16x16x32(b0, y0, dp, 0, 0, 0);
  dp = MFMA_16x16x32(b1, y1, dp, 0, 0, 0);
}

// P recomputed from the saved statistics, and dS = P * (dP - D) * scale: c = scale * log2(e), lse2 = lse * log2(e), dss = D * scale
__device__ __forceinline__ float p_from_lse(float s, float c, float lse2) { return __builtin_amdgcn_exp2f(fmaf(s, c, -lse2)); }
__device__ __forceinline__ float ds_of(float pr, float dp, float scale, float dss) { return pr * fmaf(dp, scale, -dss); }

// the lane's 16 accumulator values of an output row (columns 16 dt + 4 q4 + r), times `mul`, as four 8-byte stores; op = row + 4 q4
__device__ __forceinline__ void store_acc(op_t* op, const f32x4 (&acc)[4], float mul = 1.f) {
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    opx4 ov;
#pragma unroll
    for (int r = 0; r < 4; ++r) ov[r] = (op_t)(acc[dt][r] * mul);
    *reinterpret_cast<opx4*>(op + 16 * dt) = ov;
  }
}
// two accumulators (dK and dV), their stores interleaved
__device__ __forceinline__ void store_acc2(op_t* op0, const f32x4 (&acc0)[4], op_t* op1, const f32x4 (&acc1)[4]) {
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    opx4 o0, o1;
#pragma unroll
    for (int r = 0; r < 4; ++r) { o0[r] = (op_t)acc0[dt][r]; o1[r] = (op_t)acc1[dt][r]; }
    *reinterpret_cast<opx4*>(op0 + 16 * dt) = o0;
    *reinterpret_cast<opx4*>(op1 + 16 * dt) = o1;
  }
}

// ---- head_dim 96 (MViTv2): 32-row tiles of 6 sixteen-column blocks, shared by attn_pool.hip and mvit_rel.hip
constexpr int PB_D = 96, NCB = 6;
static_assert(PB_D == PVRL_MVIT_HEAD_DIM, "include/pvrl.h states the head_dim the callers read");
// blocked [rows][96] bf16 tile: contiguous [4 rows][16 cols] 128-byte blocks, pairwise block swizzle
__device__ __forceinline__ int pb_off(int row, int col) {
  const int rb = row >> 2;
  return (rb * NCB + ((col >> 4) ^ (rb & 1))) * 128 + (row & 3) * 32 + (col & 15) * 2;
}
__device__ __forceinline__ opx8 pb_row_frag(const char* tile, int row, int chunk) {
  return *reinterpret_cast<const opx8*>(tile + pb_off(row, chunk * 8));
}
// transposed fragment over the tile's 32 rows: lane (i, q) receives column 16*ct + i at rows {4q..4q+3, 16+4q..16+4q+3}
__device__ __forceinline__ opx8 pb_tr_frag(const char* tile, int ct, int lane) {
  const int q = lane >> 4, i = lane & 15;
  const int rb0 = q, rb1 = q + 4;
  return tr_frag8(tile, (rb0 * NCB + (ct ^ (rb0 & 1))) * 128 + i * 8, (rb1 * NCB + (ct ^ (rb1 & 1))) * 128 + i * 8);
}
