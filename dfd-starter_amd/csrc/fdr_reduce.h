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

// ---- in-launch hand-off between workgroups (the ticket of fd_grad_fused_kernel, dsgd_apply_cb_kernel and
// opt_apply_cb_kernel) ----
// handed-off payload is stored write-through (sc1: an agent-scope relaxed atomic store), so the ticket needs
// no release fence (cdna_hip_programming.md Guideline 16 R1)
__device__ __forceinline__ void store_wt(double* p, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), __builtin_bit_cast(unsigned long long, v),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void publish_and_ticket(unsigned* cnt, unsigned need, int* s_flag) {
  // every storing wave drains its sc1 stores, the workgroup meets, ONE lane takes the ticket
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned prev = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = prev == need - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    *s_flag = last;
  }
  __syncthreads();
}

}  // namespace fdr
