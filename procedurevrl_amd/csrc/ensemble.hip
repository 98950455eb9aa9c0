// Multi-view test ensemble on the device (reference: lib/utils/meters.py `EPICTestMeter.update_stats` :1040-1047 and
// `TestMeter.update_stats` :103-128 -- a Python loop over the clips of a batch, one row added into a CPU tensor per iteration,
// after a `.cpu()` of the batch's predictions).  Here the batch stays on the GPU and nothing waits for it.
//
// The fp32 order of additions into one element must be the loop's (increasing ind), so there are no atomics: one workgroup per
// batch clip; the workgroup of the FIRST clip of a video within the batch is that video's leader, every other one leaves.  The
// leader folds the video's rows ind, ..., N-1 in order into the value it read from video_preds and writes each element once.
// Leaders of different videos touch different rows, so no two workgroups write the same address.  N is a batch (tens to low
// hundreds of clips): the id scans are wave-uniform loads of a few hundred bytes that stay in the scalar cache.
#include "common.h"
#include "../../include/pvrl.h"

namespace {

template <int MODE>
__global__ __launch_bounds__(256) void view_ensemble_kernel(const float* __restrict__ preds, long ldp,
                                                            const long* __restrict__ clip_ids,
                                                            const long* __restrict__ labels, int N, int C, long num_clips,
                                                            float* __restrict__ video_preds, long ldv, long V,
                                                            long* __restrict__ video_labels, long* __restrict__ clip_count,
                                                            int* __restrict__ bad) {
  const int ind = blockIdx.x;
  const long limit = V * num_clips;
  const long id = clip_ids[ind];
  if (id < 0 || id >= limit) {      // (uniform over the workgroup)
    if (threadIdx.x == 0) *bad = 1;
    return;
  }
  const long vid = id / num_clips;
  for (int j = 0; j < ind; ++j) {   // an earlier clip of the same video leads
    const long o = clip_ids[j];
    if (o >= 0 && o < limit && o / num_clips == vid) return;
  }
  int count = 0, last = ind;        // how many rows of this batch the video has, and the last of them (its label stays)
  for (int j = ind; j < N; ++j) {
    const long o = clip_ids[j];
    if (o >= 0 && o < limit && o / num_clips == vid) { ++count; last = j; }
  }
  for (int c = threadIdx.x; c < C; c += 256) {
    float acc = video_preds[vid * ldv + c];
    for (int j = ind; j < N; ++j) {
      const long o = clip_ids[j];
      if (!(o >= 0 && o < limit && o / num_clips == vid)) continue;
      const float p = preds[(long)j * ldp + c];
      if (MODE == 0)
        acc = acc + p;
      else
        acc = (p != p || p > acc) ? p : acc;    // torch.max: a NaN on either side stays
    }
    video_preds[vid * ldv + c] = acc;
  }
  if (threadIdx.x == 0) {
    video_labels[vid] = labels[last];
    if (clip_count) clip_count[vid] += count;
  }
}

}  // namespace

extern "C" int pvrl_view_ensemble(const float* preds, int64_t ldp, const int64_t* clip_ids, const int64_t* labels, int64_t N,
                                  int64_t C, int64_t num_clips, int mode, float* video_preds, int64_t ldv, int64_t V,
                                  int64_t* video_labels, int64_t* clip_count, int32_t* bad, void* stream) {
  if (N < 0 || C < 0 || V < 0 || num_clips <= 0 || (mode != 0 && mode != 1) || ldp < C || ldv < C || N > 0x7fffffff ||
      C > 0x7fffffff || V > 0x7fffffffffffffffLL / num_clips)
    return PVRL_EINVAL;
  if (N == 0) return PVRL_OK;
  if (!preds || !clip_ids || !labels || !video_preds || !video_labels || !bad) return PVRL_EINVAL;
  if (mode == 0)
    hipLaunchKernelGGL(view_ensemble_kernel<0>, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, preds, (long)ldp,
                       (const long*)clip_ids, (const long*)labels, (int)N, (int)C, (long)num_clips, video_preds, (long)ldv,
                       (long)V, (long*)video_labels, (long*)clip_count, (int*)bad);
  else
    hipLaunchKernelGGL(view_ensemble_kernel<1>, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, preds, (long)ldp,
                       (const long*)clip_ids, (const long*)labels, (int)N, (int)C, (long)num_clips, video_preds, (long)ldv,
                       (long)V, (long*)video_labels, (long*)clip_count, (int*)bad);
  PVRL_LAUNCH_CHECK();
  return PVRL_OK;
}
