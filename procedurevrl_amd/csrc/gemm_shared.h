// What the NT and the TN GEMM families share: the buffer descriptor, the raw LDS-DMA copy, the segment ends of the 8-wave ping-pong
// schedule (gemm_nt8_core.h, gemm_tn8_core.h) and the slot lookup of the launches that carry several problems.
#pragma once
#include "common.h"

namespace {

typedef __amdgpu_buffer_rsrc_t rsrc_t;

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
// One 1 KiB LDS-DMA copy through a buffer descriptor: lane l's 16 bytes at r.base + soff + voff land at LDS byte lds + 16 l.
// Offsets past the descriptor's size read as zero (the rows behind M of the ragged last panel, behind a slice's end).  Raw ISA: the
// compiler neither counts it nor waits for it.  (s_nop 4: a descriptor / offset register produced by v_readfirstlane needs five wait
// states before a vector-memory instruction reads it; s_nop 0: M0 write -> LDS-DMA.  Nothing inside an asm string is padded by hipcc.)
__device__ __forceinline__ void bdma16(rsrc_t r, unsigned voff, unsigned soff, unsigned lds) {
  asm volatile("s_nop 4\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds"
               :: "v"(voff), "s"(r), "s"(soff), "s"(lds) : "memory", "m0");
}
#pragma clang diagnostic pop

// ---- the 8-wave ping-pong schedule: wave groups G0 = waves 0-3 (one per SIMD) and G1 = waves 4-7, G1 one barrier interval behind
// G0.  A phase is a MEMORY segment (fragment reads into registers, LDS-DMA for a later stage, the counted wait) and a COMPUTE segment
// (MFMAs on registers only, s_setprio 1), each closed by a workgroup barrier: while one wave of a SIMD computes, its partner is in its
// memory segment.  Hazards:
//   RAW  a half-tile is read in the phase AFTER the one whose memory segment waited for it (vmcnt) -- by then both groups have
//        passed a barrier behind their wait;
//   WAR  a half-tile is re-staged in the phase AFTER its last read, and every memory segment ends with lgkmcnt(0) BEFORE its
//        barrier: when G0 issues the DMA, G1's reads of the previous phase have completed behind that barrier.
#define PP_BARRIER()                        \
  do {                                      \
    __builtin_amdgcn_sched_barrier(0);      \
    __builtin_amdgcn_s_barrier();           \
    __builtin_amdgcn_sched_barrier(0);      \
  } while (0)
// end of a memory segment: this wave's fragment reads have completed BEFORE the barrier (WAR rule: the slot they came from may be
// re-staged by the other group right behind it)
#define PP_MEM_END()                                      \
  do {                                                    \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    \
    PP_BARRIER();                                         \
    __builtin_amdgcn_s_setprio(1);                        \
  } while (0)
#define PP_CMP_END()                  \
  do {                                \
    __builtin_amdgcn_s_setprio(0);    \
    PP_BARRIER();                     \
  } while (0)

// A launch that carries n problems laid end to end: first[t] is the first work item of problem t; the problem that owns item `idx`
template <int NP1>
__device__ __forceinline__ int group_slot(const int (&first)[NP1], int n, int idx) {
  int q = 0;
#pragma unroll
  for (int t = 1; t < NP1 - 1; ++t)
    if (t < n && idx >= first[t]) q = t;
  return q;
}

}  // namespace
