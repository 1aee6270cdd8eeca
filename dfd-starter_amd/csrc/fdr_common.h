// Shared device helpers for the FD engine kernels (gfx950 / CDNA4, wave64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fdr.h"

namespace fdr {

constexpr int kWave = 64;
constexpr int kHidden = 64;  // policies/discrete.py:35-36, policies/mujoco.py:33-34

// ---------------------------------------------------------------------------------------------
// Counter random stream (oracle/rng.py restates it for the checker; DESIGN.md "Random streams")
// ---------------------------------------------------------------------------------------------
// mix64 in its three rounds and hash_ctr's counter word, separately callable: the pair rollout kernel spreads one
// draw batch over the steps of the batch before it (mix64 = c(b(a(z))), hash_ctr = mix64(hash_ctr_word))
__host__ __device__ __forceinline__ uint64_t mix64_a(uint64_t z) { return (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; }
__host__ __device__ __forceinline__ uint64_t mix64_b(uint64_t z) { return (z ^ (z >> 27)) * 0x94D049BB133111EBull; }
__host__ __device__ __forceinline__ uint64_t mix64_c(uint64_t z) { return z ^ (z >> 31); }
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) { return mix64_c(mix64_b(mix64_a(z))); }
constexpr uint64_t kCtrMul = 0x9E3779B97F4A7C15ull;
__device__ __forceinline__ uint64_t hash_ctr_word(uint64_t key, uint64_t lane, uint64_t t, uint64_t k) {
  const uint64_t c = (lane << 32) | (t << 4) | k;
  return key + c * kCtrMul;
}
// The word is linear in t modulo 2^64 while (t << 4) | k stays below 2^32 (t < 2^28, k < 16; kJiggleT is the last such
// t): hash_ctr_word(key, lane, t + n, k) = hash_ctr_word(key, lane, t, k) + n * kCtrStepInc.  A loop over steps forms
// its per-thread base word (hash_ctr_base) once and adds (tests/test_ctr_recurrence.py).
constexpr uint64_t kCtrStepInc = 16ull * kCtrMul;
// low = (t0 << 4) | k, the word's low 32 counter bits
__device__ __forceinline__ uint64_t hash_ctr_base(uint64_t key, uint64_t lane, uint32_t low) {
  return key + ((lane << 32) | (uint64_t)low) * kCtrMul;
}
__device__ __forceinline__ uint64_t hash_ctr(uint64_t key, uint64_t lane, uint64_t t, uint64_t k) {
  return mix64(hash_ctr_word(key, lane, t, k));
}
constexpr uint64_t kJiggleT = (1ull << 28) - 1;

__device__ __forceinline__ float uniform24(uint64_t h) {
  return (float)(uint32_t)(h >> 40) * 0x1p-24f;
}
// Box-Muller on the hardware transcendental units: v_log_f32 is log2, v_cos_f32 takes revolutions,
// so cos(2*pi*u2) needs no range reduction.  Agrees with oracle/rng.py to a few ulp.
__device__ __forceinline__ float bm_u1(uint64_t h) { return (float)((uint32_t)(h >> 40) + 1u) * 0x1p-24f; }
__device__ __forceinline__ float bm_u2(uint64_t h) { return (float)((uint32_t)(h >> 16) & 0xFFFFFFu) * 0x1p-24f; }
__device__ __forceinline__ float bm_radius(float u1) {
  return __builtin_sqrtf(-1.38629436111989061f * __builtin_amdgcn_logf(u1));  // -2 ln u1
}
__device__ __forceinline__ float bm_normal(float r, float u2) { return r * __builtin_amdgcn_cosf(u2); }
__device__ __forceinline__ float normal_bm(uint64_t h) { return bm_normal(bm_radius(bm_u1(h)), bm_u2(h)); }

// tanh(x) = 1 - 2 / (1 + e^{2x}) on v_exp_f32 / v_rcp_f32 (abs error ~3e-7; saturates to +-1)
constexpr float kTanhScale = 2.88539008177792681f;  // 2 * log2(e)
__device__ __forceinline__ float tanh_pre(float t) {  // tanh(x) for t = kTanhScale * x
  const float e = __builtin_amdgcn_exp2f(t);
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + e);
}
__device__ __forceinline__ float tanh_fast(float x) { return tanh_pre(x * kTanhScale); }
template <bool kPre>  // kPre: the argument is already x kTanhScale
__device__ __forceinline__ float tanh_act(float z) {
  if constexpr (kPre) return tanh_pre(z);
  else return tanh_fast(z);
}

// ---------------------------------------------------------------------------------------------
// Wave-scope LDS ordering: LDS ops of one wave complete in order, so a wave that only talks to
// itself through LDS needs a compiler fence, not an s_barrier (no cross-wave hand-off here).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
  return v;
}

// theta'[p] = fl32(base[p] +/- fl32(sigma * eps[p]))  -- no contraction (bit-exact with numpy).
// Branch-free: eps is always a readable address (the lane's base when it is not perturbed -- its value is then
// discarded by the select), so every element's two loads are unconditional and the compiler batches them.  (r12: a
// per-element `if (sgn != 0)` around the eps load put each load behind its own exec branch and wait -- ~200 serialised
// HBM round trips per thread in the MLP rollouts' prologue.)
//
// The sign rides on sigma (ss = sgn < 0 ? -sigma : sigma, set once in LanesArgs::src), so an element costs one
// product, one 32-bit select, one add and one f64 FMA instead of two sums, four selects and an f64 multiply and add
// (the MLP rollouts' prologue is VALU-issue-bound: DESIGN.md 3.0).  With st = fl32(ss * eps[p]) and
// z = sgn != 0 ? st : -0.0f the result is base[p] + z and the norm term fma(z, z, n2) in f64.  Same bits as the
// two-sided form (tests/test_theta_prime_identities.py checks each identity in numpy):
//   - fl32((-sigma) * eps) = -fl32(sigma * eps): round-to-nearest-even is symmetric about zero;
//   - t - x and t + (-x) are the same IEEE operation, signed zeros included, so base[p] + z is t +/- st;
//   - t + (-0.0f) = t for every t, -0.0f included (t + (+0.0f) would turn a -0.0f into +0.0f): an unperturbed lane
//     gets t itself;
//   - d = (double)z has a 24-bit significand, so d * d is exact in f64 and fma(d, d, n2) = fl64(n2 + d * d) is the
//     rounded sum n2 + fl64(d * d) of the two-step form;
//   - an unperturbed lane has d = -0.0, d * d = +0.0: the two-step form's n2 += 0.0;
//   - a lane whose n2 starts as NaN (out-of-range offset) keeps it.
// (A second form without the select, taken by waves that hold no unperturbed lane, was measured and not kept:
// DESIGN.md 3.0 p14.)
struct ParamSrc {
  const float* base;
  const float* eps;  // table + idx, or base (unperturbed lane: loaded, not used)
  float ss;          // sigma with the lane's sign: -sigma when sgn < 0
  int sgn;           // +1 / -1 / 0
  double n2;         // running sum of fl32(sigma*eps)^2 over the elements this thread loaded

  __device__ __forceinline__ float step(int64_t p) const {  // z: the signed step, -0.0f on an unperturbed lane
#pragma clang fp contract(off)
    const float st = ss * eps[p];
    return sgn != 0 ? st : -0.0f;
  }
  __device__ __forceinline__ float get(int64_t p) {
#pragma clang fp contract(off)
    const float t = base[p];
    const float z = step(p);
    const double d = (double)z;
    n2 = __builtin_fma(d, d, n2);
    return t + z;
  }
  // get(p) counted in n2 only when `use` (an element read unconditionally from a clamped index whose value the caller
  // discards otherwise: no load behind a branch)
  __device__ __forceinline__ float get_if(int64_t p, bool use) {
#pragma clang fp contract(off)
    const float t = base[p];
    const float z = step(p);
    const double d = (double)(use ? z : -0.0f);
    n2 = __builtin_fma(d, d, n2);
    return t + z;
  }
  // same value, but not counted in n2 (an element several threads replicate)
  __device__ __forceinline__ float get_nocount(int64_t p) const {
#pragma clang fp contract(off)
    const float t = base[p];
    return t + step(p);
  }
};

// Diagnostics (fdr_diag_theta_prime): a ParamSrc that also records what the loaders ask of it.  Every accessor returns
// ParamSrc's own value and stores it at out[p], adds 1 to reads[p], and to counted[p] when the call is one that
// contributes to n2 (get, and get_if with `use`).  The three rows are this lane's; rec = false records nothing (the
// idle half of a pair wave, which shadows its partner).  Plain vector stores and int atomics.
struct RecordSrc : ParamSrc {
  float* out;
  int32_t* reads;
  int32_t* counted;
  bool rec;

  __device__ __forceinline__ void note(int64_t p, float v, bool cnt) const {
    if (!rec) return;
    out[p] = v;
    atomicAdd(&reads[p], 1);
    if (cnt) atomicAdd(&counted[p], 1);
  }
  __device__ __forceinline__ float get(int64_t p) {
    const float v = ParamSrc::get(p);
    note(p, v, true);
    return v;
  }
  __device__ __forceinline__ float get_if(int64_t p, bool use) {
    const float v = ParamSrc::get_if(p, use);
    note(p, v, use);
    return v;
  }
  __device__ __forceinline__ float get_nocount(int64_t p) const {
    const float v = ParamSrc::get_nocount(p);
    note(p, v, false);
    return v;
  }
};

}  // namespace fdr
