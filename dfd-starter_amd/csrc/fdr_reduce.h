// Workgroup-wide f64 sums of the learner kernels: wave_sum, one LDS slot per wave, every thread adds the slots in
// wave order -- the same value in every thread, independent of which wave arrives first.
#pragma once
#include "fdr_common.h"

namespace fdr {

// 256 threads, red[4]: every wave's sum in its slot, visible to all threads on return
inline __device__ void wave_sums_256(double v, double* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
}

// 256 threads, red[4].  The trailing barrier lets the caller reuse red at once; fd_grad_fused_kernel is tuned
// around this barrier placement.
inline __device__ double block_sum_256(double v, double* red) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6, j = threadIdx.x & 63;
  if (j == 0) red[w] = v;
  __syncthreads();
  const double s = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return s;
}

// 1024 threads (every caller launches exactly that many), red[16].  The leading barrier guards a red still being
// read from the call before.
inline __device__ double block_sum_1024(double v, double* red) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6, j = threadIdx.x & 63;
  __syncthreads();
  if (j == 0) red[w] = v;
  __syncthreads();
  double s = 0.0;
  for (int i = 0; i < 16; ++i) s += red[i];
  return s;
}

}  // namespace fdr
