// fdr_learner_fused.hip -- the fused learner step: weighting, noise-weighted gradient and chunk combine in one launch
// (fd_grad_fused_kernel; fd_grad_fused_mix_kernel for the reward / novelty / entropy objective), the DSGD that can
// follow it in the same call (dsgd_apply_cb_kernel; fdr_optim.hip's opt_apply_cb_kernel for Adam / AdamW / SGD),
// centred-rank weights.  Top-b direction weights: fdr_top_dirs.hip, in front of the centred-rank instance.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "fdr_learner.h"
#include "fdr_reduce.h"

namespace fdr {

// ------------------------------------------------------------------------------------------
// Fused learner step (fdr_fd_grad_fused / fdr_fd_step): the weighting, the noise-weighted gradient and
// its chunk combine in ONE launch -- and, single-process with P <= 65536, DSGD in the same launch.
//
// fd_grad_fused_kernel, grid (column blocks of 256, row chunks), 256 threads:
//   1. the chunk's first 64 table rows are requested up front (they do not depend on the weights);
//   2. meanwhile the workgroup forms the weights of ITS directions: the z-score statistics over all
//      rewards (f64, the same fixed-order tree in every workgroup, so all agree bit for bit), or
//      precomputed centred-rank weights, or the raw moments form; coefficients in LDS (NaN for a row
//      whose table offset is out of range: the gradient is poisoned, the table never over-read);
//   3. f64 column sums over the chunk's rows;
//   4. chunk partials are combined in the same launch: slab store -> agent-scope release -> ticket on
//      the column block's counter; the last arriver acquires and sums the slabs in chunk order
//      (deterministic and placement-independent: cdna_hip_programming.md Guideline 16, counter form)
//      and resets the counter;
//   5. (fdr_fd_step) each column block's owner publishes sum fl32(-g)^2 of its columns and takes a
//      ticket on the DSGD counter; the last owner forms ||fl32(-g)|| in column-block order and applies
//      the update to all of theta (dynamic_sgd.py:19-39), then ||d theta||.
// Counters must be zero before the first launch on a workspace (the caller zeroes the leading counter
// block once); every launch leaves them zero.
// ------------------------------------------------------------------------------------------
constexpr int kFusedRows = 64;       // table rows per pass: loads in flight per thread
constexpr int kFusedMaxRows = 1024;  // directions per chunk (LDS coefficient arrays)

// store_wt / publish_and_ticket: fdr_reduce.h (shared with opt_apply_cb_kernel, fdr_optim.hip)

// sum over k < n of base[k * stride] in k order, 16 loads in flight
__device__ __forceinline__ double sum_slabs(const double* base, int64_t stride, int n) {
  double s = 0.0;
  int k = 0;
  for (; k + 16 <= n; k += 16) {
    double v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = base[(int64_t)(k + e) * stride];
#pragma unroll
    for (int e = 0; e < 16; ++e) s += v[e];
  }
  for (; k < n; ++k) s += base[(int64_t)k * stride];
  return s;
}

template <int MODE>
__global__ __launch_bounds__(256) void fd_grad_fused_kernel(FdArgs a) {
  __shared__ double cA[kFusedMaxRows];
  __shared__ double cB[MODE == FDR_WEIGHT_MOMENTS ? kFusedMaxRows : 1];
  __shared__ double red[4];
  __shared__ int s_flag;
  const int tid = threadIdx.x;
  const int chunk = blockIdx.y, cb = blockIdx.x;
  const int d0 = chunk * a.rows_per_chunk, d1 = min(a.n_dirs, d0 + a.rows_per_chunk);
  const int64_t P = a.P;
  const int64_t col = (int64_t)cb * 256 + tid;
  const bool ok = col < P;
  const int64_t cc = ok ? col : 0;
  auto row_off = [&](int d) {
    const int64_t off = a.idx[(int64_t)d * a.lpd];
    return (off < 0 || off > a.max_idx) ? (int64_t)-1 : off;
  };
  float v[kFusedRows];
  // Row offsets: lane l of every wave loads row r0 + l's offset (one vector load; clamped into the chunk,
  // an invalid offset reads row 0 -- its coefficient is NaN) and the pass takes row r's through
  // v_readlane, so the table address is scalar base + column.  (Per-row scalar loads were each followed
  // by an lgkmcnt(0) wait: 64 dependent round trips before the last row was even requested.)
  auto row_offsets = [&](int r0) {
    int64_t off = a.idx[(int64_t)min(r0 + (tid & 63), d1 - 1) * a.lpd];
    return (off < 0 || off > a.max_idx) ? (int64_t)0 : off;
  };
  auto load_pass = [&](int r0, int64_t offl) {
    const unsigned lo = (unsigned)offl, hi = (unsigned)((uint64_t)offl >> 32);
#pragma unroll
    for (int r = 0; r < kFusedRows; ++r) {
      const int64_t o = (int64_t)(((uint64_t)(unsigned)__builtin_amdgcn_readlane((int)hi, r) << 32) |
                                  (unsigned)__builtin_amdgcn_readlane((int)lo, r));
      const float x = a.table[o + cc];  // unconditional (rows past the chunk repeat its last row): no branch
      v[r] = r0 + r < d1 ? x : 0.f;
    }
  };
  const int64_t off0 = row_offsets(d0);  // first in the vmcnt order: the table loads wait only for it
  // Load order matters: vmcnt retires loads in issue order, so the statistics' inputs are requested
  // BEFORE the chunk's 64 table rows -- consuming them then waits only for themselves, and the table
  // rows stay in flight through the statistics (issued after the rows, they would wait for all 64).
  // this thread's first direction's per-lane inputs
  constexpr int kMaxLpd = 4;
  const int dmine = d0 + tid;
  // Branch-free (clamped indices, selects): a load under a condition ends its basic block with a full
  // vmcnt(0) wait, which serialised these ~30 loads into as many L2 round trips (measured: the kernel's
  // 24 us vs 10.5 us for the bare 50 MB stream, tools/learner_bench.py).
  double xin[kMaxLpd], vin[kMaxLpd];
  const int roff = MODE == FDR_WEIGHT_MOMENTS ? 0 : a.lo;  // MOMENTS: r_all holds the local lanes only
  {
    const int nloc = max(1, (d1 - d0) * a.lpd);  // this chunk's local lanes: [d0 * lpd, d1 * lpd)
    int sg[kMaxLpd];
    double n2v[kMaxLpd], xv[kMaxLpd];
#pragma unroll
    for (int k = 0; k < kMaxLpd; ++k) {
      const int i = d0 * a.lpd + min((dmine - d0) * a.lpd + k, nloc - 1);
      sg[k] = a.sign[i];
      n2v[k] = a.n2[i];
      if constexpr (MODE == FDR_WEIGHT_CENTERED_RANK) xv[k] = a.w[i];
      else xv[k] = a.r_all[roff + i];
    }
#pragma unroll
    for (int k = 0; k < kMaxLpd; ++k) {
      // computed unconditionally (an unused lane's 0/0 is selected away): a division under the condition
      // lets the compiler sink the n2 load into the branch, behind a vmcnt(0)
      const double q = (double)sg[k] * (double)a.sigma / n2v[k];
      const bool use = dmine < d1 && k < a.lpd && sg[k] != 0;
      vin[k] = use ? q : 0.0;
      xin[k] = use ? (MODE == FDR_WEIGHT_CENTERED_RANK ? xv[k] : xv[k] - a.pr) : 0.0;
    }
  }
  double mean = 0.0, sd = 0.0;
  // one load pass, the values kept in registers for the second (same per-thread order as a reload)
  constexpr int kR = MODE == FDR_WEIGHT_ZSCORE ? 16 : 1;
  double xr[kR];
  if constexpr (MODE == FDR_WEIGHT_ZSCORE) {
#pragma unroll
    for (int k = 0; k < kR; ++k) xr[k] = a.r_all[min(tid + 256 * k, a.n_all - 1)];  // clamped: no branches
#pragma unroll
    for (int k = 0; k < kR; ++k) xr[k] = tid + 256 * k < a.n_all ? xr[k] - a.pr : 0.0;
  }
  load_pass(d0, off0);  // the table rows: in flight from here through the statistics and the coefficients
  if constexpr (MODE == FDR_WEIGHT_ZSCORE) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kR; ++k)
      if (tid + 256 * k < a.n_all) s += xr[k];
    for (int i = tid + 256 * kR; i < a.n_all; i += 256) s += a.r_all[i] - a.pr;
    mean = block_sum_256(s, red) / (double)a.n_all;
    double q = 0.0;
#pragma unroll
    for (int k = 0; k < kR; ++k)
      if (tid + 256 * k < a.n_all) {
        const double d = xr[k] - mean;
        q += d * d;
      }
    for (int i = tid + 256 * kR; i < a.n_all; i += 256) {
      const double d = (a.r_all[i] - a.pr) - mean;
      q += d * d;
    }
    sd = sqrt(block_sum_256(q, red) / (double)a.n_all);
  }
  auto weight = [&](double x) {
    if constexpr (MODE == FDR_WEIGHT_ZSCORE) return sd == 0.0 ? x : (x - mean) / sd;  // math_helpers.py:127-134
    else return x;
  };
  // MOMENTS: c = sum_k (r'_k - r'_0) v_k + r'_0 b, b = sum_k v_k -- the same value in real arithmetic, but an
  // antithetic pair (v_1 = -v_0, so b = 0 exactly) gives c = (r'_1 - r'_0) v_1 with the difference exact
  // (Sterbenz) instead of r'_0 v_0 + r'_1 v_1, whose products cancel when the returns are near-constant
  if (dmine < d1 && a.lpd <= kMaxLpd) {
    double c = 0.0, b = 0.0;
    const double x0 = MODE == FDR_WEIGHT_MOMENTS ? xin[0] : 0.0;
#pragma unroll
    for (int k = 0; k < kMaxLpd; ++k)
      if (k < a.lpd && vin[k] != 0.0) {
        c += weight(xin[k] - x0) * vin[k];
        b += vin[k];
      }
    if constexpr (MODE == FDR_WEIGHT_MOMENTS) c = fma(x0, b, c);
    if (row_off(dmine) < 0) c = b = __builtin_nan("");
    cA[dmine - d0] = c;
    if constexpr (MODE == FDR_WEIGHT_MOMENTS) cB[dmine - d0] = b;
  }
  for (int d = d0 + tid + (a.lpd <= kMaxLpd ? 256 : 0); d < d1; d += 256) {  // further directions of this thread
    double c = 0.0, b = 0.0, x0 = 0.0;
    for (int k = 0; k < a.lpd; ++k) {
      const int i = d * a.lpd + k;
      const int sg = a.sign[i];
      if (sg == 0) continue;
      const double vi = (double)sg * (double)a.sigma / a.n2[i];
      double x;
      if constexpr (MODE == FDR_WEIGHT_CENTERED_RANK) x = a.w[i];
      else x = a.r_all[roff + i] - a.pr;
      if (MODE == FDR_WEIGHT_MOMENTS && k == 0) x0 = x;  // as above
      c += weight(x - x0) * vi;
      b += vi;
    }
    if constexpr (MODE == FDR_WEIGHT_MOMENTS) c = fma(x0, b, c);
    if (row_off(d) < 0) c = b = __builtin_nan("");
    cA[d - d0] = c;
    if constexpr (MODE == FDR_WEIGHT_MOMENTS) cB[d - d0] = b;
  }
  __syncthreads();

  double acc0 = 0.0, acc1 = 0.0, bcc0 = 0.0, bcc1 = 0.0;
  for (int r0 = d0; r0 < d1; r0 += kFusedRows) {
    if (r0 != d0) load_pass(r0, row_offsets(r0));
#pragma unroll
    for (int r = 0; r < kFusedRows; r += 2) {
      if (r0 + r < d1) {
        acc0 = fma(cA[r0 + r - d0], (double)v[r], acc0);
        if constexpr (MODE == FDR_WEIGHT_MOMENTS) bcc0 = fma(cB[r0 + r - d0], (double)v[r], bcc0);
      }
      if (r0 + r + 1 < d1) {
        acc1 = fma(cA[r0 + r + 1 - d0], (double)v[r + 1], acc1);
        if constexpr (MODE == FDR_WEIGHT_MOMENTS) bcc1 = fma(cB[r0 + r + 1 - d0], (double)v[r + 1], bcc1);
      }
    }
  }
  const double ga = acc0 + acc1, gb = bcc0 + bcc1;

  bool owner = true;  // this workgroup holds the final g of its column block
  double gfin = ga;
  if (a.n_chunks == 1) {
    if (ok) {
      store_wt(a.out + col, ga);
      if constexpr (MODE == FDR_WEIGHT_MOMENTS) a.out[P + col] = gb;
    }
  } else {
    if (ok) {
      store_wt(a.partial + (int64_t)chunk * P + col, ga);
      if constexpr (MODE == FDR_WEIGHT_MOMENTS) store_wt(a.partial + ((int64_t)a.n_chunks + chunk) * P + col, gb);
    }
    publish_and_ticket(a.cnt + cb, (unsigned)a.n_chunks, &s_flag);
    owner = s_flag != 0;
    if (owner) {
      double sa = 0.0, sb = 0.0;
      if (ok) {
        sa = sum_slabs(a.partial + col, P, a.n_chunks);
        store_wt(a.out + col, sa);  // read by the DSGD workgroup of fdr_fd_step
        if constexpr (MODE == FDR_WEIGHT_MOMENTS) {
          sb = sum_slabs(a.partial + (int64_t)a.n_chunks * P + col, P, a.n_chunks);
          a.out[P + col] = sb;
        }
      }
      gfin = sa;
      if (tid == 0) __hip_atomic_store(a.cnt + cb, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if constexpr (MODE == FDR_WEIGHT_MOMENTS) {
    if (cb == 0 && chunk == 0) {
      // [n_local | r' slots]: this rank's r' at its global lanes, 0 elsewhere -- the all-reduce's sum is then
      // every rank's r' (x + 0 = x exactly) and the lane count, from which the DSGD launch forms the z-score
      // statistics in two passes as standardize_arr does (a one-pass sum r'^2 / n - m^2 cancels when the
      // returns are near-constant)
      const int n_local = a.n_dirs * a.lpd;
      double* slots = a.out + 2 * P + 1;
      for (int i = tid; i < a.n_all; i += 256) {
        const int k = i - a.lo;
        slots[i] = (k >= 0 && k < n_local) ? a.r_all[k] - a.pr : 0.0;
      }
      if (tid == 0) a.out[2 * P] = (double)n_local;
    }
  } else {
    if (a.gsq && owner) {  // fdr_fd_step: this column block's sum fl32(-g)^2 for the DSGD launch
      const float gr = ok ? (float)(-gfin) : 0.f;  // set_grad_from_flat casts to f32 (policy.py:68)
      const double part = block_sum_256((double)gr * (double)gr, red);
      if (tid == 0) a.gsq[cb] = part;
    }
  }
}

// ------------------------------------------------------------------------------------------
// The mixed objective (fdr_fd_grad_fused_mix / fdr_fd_step_mix, FDR_WEIGHT_ZSCORE_MIX): the z-score instance with
// three channels, w_i = a_r z_r[i] + a_n z_n[i] + a_e z_e[i] over the active ones (MixChannels, fdr_learner.h).  A
// kernel of its own, so that fd_grad_fused_kernel's three instances and FdArgs stay what they are, instruction for
// instruction; the tiling, the load order (statistics inputs, then the chunk's first 64 rows), the NaN coefficient,
// the chunk combine and the sum fl32(-g)^2 partials are that kernel's, restated.
//
// Registers: the z-score instance holds 16 x values per thread (32 VGPRs) beside v[64] at 153 VGPRs, 3 waves per
// SIMD -- what keeps config 3's 768 workgroups resident at once.  Three channels at 16 would take 96: kMixR = 4 per
// channel (24 VGPRs; n_all <= 1024 entirely in registers) and the per-lane inputs of directions of up to kMixLpd = 2
// lanes (antithetic pairs) stay under that line; lanes beyond either are read again from memory (L2-hot: every
// workgroup reads the same 3 n_all doubles), kMixTail per channel in flight, after the table rows: 152 VGPRs, no
// scratch, 3 waves per SIMD.  (kMixTail = 6: 166 VGPRs and no faster at config 3, 27.9 against 27.4 us -- the three
// statistics chains cost what the r11 probe put on one, ~2.2 us each, not the tail's round trips.)  Per thread the
// sums run over i = tid, tid + 256, .. in this order whatever kMixR is, and the workgroup tree is block_sum_256's:
// with coefficients (1, 0, 0) the statistics, the weights and g are the z-score instance's bits.
// ------------------------------------------------------------------------------------------
constexpr int kMixR = 4;     // x values per channel held in registers
constexpr int kMixLpd = 2;   // lanes of a thread's first direction whose inputs are held in registers
constexpr int kMixTail = 4;  // lanes per channel in flight in the tail loops

// a workgroup-uniform f64 into scalar registers (same bits)
__device__ __forceinline__ double uniform_f64(double v) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)u);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(u >> 32));
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// block_sum_256 of three values at once: the same wave_sum and the same slot order per value, one barrier pair
__device__ __forceinline__ void block_sum3_256(double (&s)[3], double (*red3)[4]) {
  const int w = threadIdx.x >> 6, j = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double t = wave_sum(s[c]);
    if (j == 0) red3[c][w] = t;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 3; ++c) s[c] = uniform_f64(red3[c][0] + red3[c][1] + red3[c][2] + red3[c][3]);
  __syncthreads();
}

__global__ __launch_bounds__(256) void fd_grad_fused_mix_kernel(FdMixArgs m) {
  const FdArgs& a = m.fd;
  __shared__ double cA[kFusedMaxRows];
  __shared__ double red[4];
  __shared__ double red3[3][4];
  __shared__ int s_flag;
  const int tid = threadIdx.x;
  const int chunk = blockIdx.y, cb = blockIdx.x;
  const int d0 = chunk * a.rows_per_chunk, d1 = min(a.n_dirs, d0 + a.rows_per_chunk);
  const int64_t P = a.P;
  const int64_t col = (int64_t)cb * 256 + tid;
  const bool ok = col < P;
  const int64_t cc = ok ? col : 0;
  const bool act0 = m.mix.a[0] != 0.0, act1 = m.mix.a[1] != 0.0, act2 = m.mix.a[2] != 0.0;
  auto row_off = [&](int d) {
    const int64_t off = a.idx[(int64_t)d * a.lpd];
    return (off < 0 || off > a.max_idx) ? (int64_t)-1 : off;
  };
  float v[kFusedRows];
  // as fd_grad_fused_kernel: one vector load of the pass's 64 offsets (clamped into the chunk, an invalid offset
  // reads row 0 under a NaN coefficient), each row's taken by v_readlane
  auto row_offsets = [&](int r0) {
    int64_t off = a.idx[(int64_t)min(r0 + (tid & 63), d1 - 1) * a.lpd];
    return (off < 0 || off > a.max_idx) ? (int64_t)0 : off;
  };
  auto load_pass = [&](int r0, int64_t offl) {
    const unsigned lo = (unsigned)offl, hi = (unsigned)((uint64_t)offl >> 32);
#pragma unroll
    for (int r = 0; r < kFusedRows; ++r) {
      const int64_t o = (int64_t)(((uint64_t)(unsigned)__builtin_amdgcn_readlane((int)hi, r) << 32) |
                                  (unsigned)__builtin_amdgcn_readlane((int)lo, r));
      const float x = a.table[o + cc];
      v[r] = r0 + r < d1 ? x : 0.f;
    }
  };
  const int64_t off0 = row_offsets(d0);
  // the statistics' inputs before the table rows, branch-free with clamped indices (fd_grad_fused_kernel says why)
  const int dmine = d0 + tid;
  double xin[3][kMixLpd], vin[kMixLpd];
  {
    const int nloc = max(1, (d1 - d0) * a.lpd);
    int sg[kMixLpd];
    double n2v[kMixLpd], xv[3][kMixLpd];
#pragma unroll
    for (int k = 0; k < kMixLpd; ++k) {
      const int i = d0 * a.lpd + min((dmine - d0) * a.lpd + k, nloc - 1);
      sg[k] = a.sign[i];
      n2v[k] = a.n2[i];
#pragma unroll
      for (int c = 0; c < 3; ++c) xv[c][k] = m.mix.v[c][a.lo + i];
    }
#pragma unroll
    for (int k = 0; k < kMixLpd; ++k) {
      const double q = (double)sg[k] * (double)a.sigma / n2v[k];
      const bool use = dmine < d1 && k < a.lpd && sg[k] != 0;
      vin[k] = use ? q : 0.0;
#pragma unroll
      for (int c = 0; c < 3; ++c) xin[c][k] = use ? xv[c][k] - m.mix.p[c] : 0.0;
    }
  }
  double xr[3][kMixR];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int k = 0; k < kMixR; ++k) xr[c][k] = m.mix.v[c][min(tid + 256 * k, a.n_all - 1)];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int k = 0; k < kMixR; ++k) xr[c][k] = tid + 256 * k < a.n_all ? xr[c][k] - m.mix.p[c] : 0.0;
  load_pass(d0, off0);  // the table rows: in flight through the statistics and the coefficients
  double mean[3], sd[3];
  {
    double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int k = 0; k < kMixR; ++k)
        if (tid + 256 * k < a.n_all) s[c] += xr[c][k];
    for (int b = 256 * kMixR; b < a.n_all; b += 256 * kMixTail) {  // the tail: kMixTail x 3 loads in flight
      double t[3][kMixTail];
#pragma unroll
      for (int e = 0; e < kMixTail; ++e)
#pragma unroll
        for (int c = 0; c < 3; ++c) t[c][e] = m.mix.v[c][min(b + 256 * e + tid, a.n_all - 1)];
#pragma unroll
      for (int e = 0; e < kMixTail; ++e)
#pragma unroll
        for (int c = 0; c < 3; ++c)
          if (b + 256 * e + tid < a.n_all) s[c] += t[c][e] - m.mix.p[c];
    }
    block_sum3_256(s, red3);
#pragma unroll
    for (int c = 0; c < 3; ++c) mean[c] = s[c] / (double)a.n_all;
    double q[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int k = 0; k < kMixR; ++k)
        if (tid + 256 * k < a.n_all) {
          const double d = xr[c][k] - mean[c];
          q[c] += d * d;
        }
    for (int b = 256 * kMixR; b < a.n_all; b += 256 * kMixTail) {
      double t[3][kMixTail];
#pragma unroll
      for (int e = 0; e < kMixTail; ++e)
#pragma unroll
        for (int c = 0; c < 3; ++c) t[c][e] = m.mix.v[c][min(b + 256 * e + tid, a.n_all - 1)];
#pragma unroll
      for (int e = 0; e < kMixTail; ++e)
#pragma unroll
        for (int c = 0; c < 3; ++c)
          if (b + 256 * e + tid < a.n_all) {
            const double d = (t[c][e] - m.mix.p[c]) - mean[c];
            q[c] += d * d;
          }
    }
    block_sum3_256(q, red3);
#pragma unroll
    for (int c = 0; c < 3; ++c) sd[c] = sqrt(q[c] / (double)a.n_all);
  }
  auto zs = [&](int c, double x) { return sd[c] == 0.0 ? x : (x - mean[c]) / sd[c]; };  // math_helpers.py:127-134
  auto weight = [&](double x0, double x1, double x2) {  // the active channels' terms, in channel order
    double w = 0.0;
    if (act0) w = m.mix.a[0] * zs(0, x0);
    if (act1) {
      const double t = m.mix.a[1] * zs(1, x1);
      w = act0 ? w + t : t;
    }
    if (act2) {
      const double t = m.mix.a[2] * zs(2, x2);
      w = (act0 || act1) ? w + t : t;
    }
    return w;
  };
  if (dmine < d1 && a.lpd <= kMixLpd) {
    double c = 0.0;
#pragma unroll
    for (int k = 0; k < kMixLpd; ++k)
      if (k < a.lpd && vin[k] != 0.0) c += weight(xin[0][k], xin[1][k], xin[2][k]) * vin[k];
    if (row_off(dmine) < 0) c = __builtin_nan("");
    cA[dmine - d0] = c;
  }
  for (int d = d0 + tid + (a.lpd <= kMixLpd ? 256 : 0); d < d1; d += 256) {  // further directions of this thread
    double c = 0.0;
    for (int k = 0; k < a.lpd; ++k) {
      const int i = d * a.lpd + k;
      const int sg = a.sign[i];
      if (sg == 0) continue;
      const double vi = (double)sg * (double)a.sigma / a.n2[i];
      c += weight(m.mix.v[0][a.lo + i] - m.mix.p[0], m.mix.v[1][a.lo + i] - m.mix.p[1],
                  m.mix.v[2][a.lo + i] - m.mix.p[2]) * vi;
    }
    if (row_off(d) < 0) c = __builtin_nan("");
    cA[d - d0] = c;
  }
  __syncthreads();

  double acc0 = 0.0, acc1 = 0.0;
  for (int r0 = d0; r0 < d1; r0 += kFusedRows) {
    if (r0 != d0) load_pass(r0, row_offsets(r0));
#pragma unroll
    for (int r = 0; r < kFusedRows; r += 2) {
      if (r0 + r < d1) acc0 = fma(cA[r0 + r - d0], (double)v[r], acc0);
      if (r0 + r + 1 < d1) acc1 = fma(cA[r0 + r + 1 - d0], (double)v[r + 1], acc1);
    }
  }
  const double ga = acc0 + acc1;

  bool owner = true;  // this workgroup holds the final g of its column block
  double gfin = ga;
  if (a.n_chunks == 1) {
    if (ok) store_wt(a.out + col, ga);
  } else {
    if (ok) store_wt(a.partial + (int64_t)chunk * P + col, ga);
    publish_and_ticket(a.cnt + cb, (unsigned)a.n_chunks, &s_flag);
    owner = s_flag != 0;
    if (owner) {
      double sa = 0.0;
      if (ok) {
        sa = sum_slabs(a.partial + col, P, a.n_chunks);
        store_wt(a.out + col, sa);  // read by the DSGD workgroup of fdr_fd_step_mix
      }
      gfin = sa;
      if (tid == 0) __hip_atomic_store(a.cnt + cb, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (a.gsq && owner) {  // fdr_fd_step_mix: this column block's sum fl32(-g)^2 for the DSGD launch
    const float gr = ok ? (float)(-gfin) : 0.f;
    const double part = block_sum_256((double)gr * (double)gr, red);
    if (tid == 0) a.gsq[cb] = part;
  }
}

// DSGD after fd_grad_fused (fdr_fd_step): one 256-column block per workgroup.  Every workgroup forms
// ||fl32(-g)|| from the per-column-block partials in the same order, updates its columns
// (dynamic_sgd.py:19-39), writes theta_new to the history slot (the learner's policy_history,
// finite_differences.py:75-78) and its sum of squared updates; the last workgroup (ticket) forms ||d theta||.
__global__ __launch_bounds__(256) void dsgd_apply_cb_kernel(float* __restrict__ theta, const double* __restrict__ g,
                                                            int64_t P, const double* __restrict__ gsq, int col_blocks,
                                                            double lr, double lr_scale, float* __restrict__ hist,
                                                            double* __restrict__ upart, unsigned* __restrict__ cnt,
                                                            double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  __shared__ double gs[256];
  __shared__ int s_flag;
  const int tid = threadIdx.x, cb = blockIdx.x;
  const int64_t p = (int64_t)cb * 256 + tid;
  const double gv = p < P ? g[p] : 0.0;
  const float old = p < P ? theta[p] : 0.f;
  double ss = 0.0;
  for (int k0 = 0; k0 < col_blocks; k0 += 256) {
    __syncthreads();
    if (k0 + tid < col_blocks) gs[tid] = gsq[k0 + tid];
    __syncthreads();
    for (int k = 0; k < min(256, col_blocks - k0); ++k) ss += gs[k];
  }
  const float norm = (float)sqrt(ss);  // flat_grad.norm().item() (dynamic_sgd.py:27)
  double u = 0.0;
  float nw = old;
  if (norm > 0.f) {
    const double coef = lr * sqrt((double)P) * lr_scale / (double)norm;  // dynamic_sgd.py:30,51
    const float c32 = (float)coef;
    const float g32 = (float)(-gv);
    nw = old - c32 * g32;  // p.sub_(coef * grad_slice) (dynamic_sgd.py:36)
    const float dd = old - nw;
    u = p < P ? (double)dd * (double)dd : 0.0;
  }
  if (p < P) {
    theta[p] = nw;
    if (hist) hist[p] = nw;
  }
  u = block_sum_256(u, red);
  if (tid == 0) store_wt(upart + cb, u);
  publish_and_ticket(cnt, (unsigned)col_blocks, &s_flag);
  if (s_flag) {
    double t = 0.0;
    for (int k0 = 0; k0 < col_blocks; k0 += 256) {
      __syncthreads();
      if (k0 + tid < col_blocks) gs[tid] = upart[k0 + tid];
      __syncthreads();
      for (int k = 0; k < min(256, col_blocks - k0); ++k) t += gs[k];
    }
    if (tid == 0) {
      out[0] = sqrt(t);
      out[1] = (double)norm;
      __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// centred rank (build extension; the standard ES transform): rank of r_i among all n_all returns,
// ties broken by lane index; w_i = rank_i / (n_all - 1) - 0.5.  Each thread counts over LDS tiles.
__global__ __launch_bounds__(256) void rank_weights_kernel(const double* __restrict__ r_all, int n_all, int lo,
                                                           int n_local, double* __restrict__ w) {
  __shared__ double tile[2048];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int gi = lo + (i < n_local ? i : 0);
  const double ri = r_all[gi];
  int rank = 0;
  for (int t0 = 0; t0 < n_all; t0 += 2048) {
    const int tn = min(2048, n_all - t0);
    __syncthreads();
    for (int k = threadIdx.x; k < tn; k += 256) tile[k] = r_all[t0 + k];
    __syncthreads();
    for (int k = 0; k < tn; ++k) {
      const double rk = tile[k];
      rank += (rk < ri || (rk == ri && t0 + k < gi)) ? 1 : 0;
    }
  }
  if (i < n_local) w[i] = n_all > 1 ? (double)rank / (double)(n_all - 1) - 0.5 : 0.0;
}

static GradPlan fused_plan(int n_dirs, int64_t P) {
  GradPlan f;
  f.col_blocks = (int)((P + 255) / 256);
  const int target_chunks = std::max(1, 1024 / std::max(1, f.col_blocks));
  const int rows = std::max(kFusedRows, (n_dirs + target_chunks - 1) / target_chunks);
  f.rows_per_chunk = std::min(kFusedMaxRows, (rows + kFusedRows - 1) / kFusedRows * kFusedRows);
  f.n_chunks = std::max(1, (n_dirs + f.rows_per_chunk - 1) / f.rows_per_chunk);
  return f;
}

// workspace: [counters: col_blocks + 1 u32, padded to 256 B][gsq][update partials][rank weights][partial slabs]
// (FDR_WEIGHT_TOP_DIRS: [lane mask, n_all bytes] behind them)
static int64_t pad256(int64_t b) { return (b + 255) / 256 * 256; }
int64_t fused_counter_bytes(int n_dirs, int64_t P) {
  const GradPlan f = fused_plan(std::max(1, n_dirs), P);
  return pad256((int64_t)(f.col_blocks + 1) * 4);
}
int64_t fused_workspace_bytes(int n_dirs, int n_local, int64_t P, int mode) {
  if (n_dirs < 0 || P <= 0) return -1;
  const GradPlan f = fused_plan(std::max(1, n_dirs), P);
  const int64_t slabs = f.n_chunks > 1 ? (int64_t)f.n_chunks * P * 8 * (mode == FDR_WEIGHT_MOMENTS ? 2 : 1) : 0;
  return fused_counter_bytes(n_dirs, P) + 2 * pad256((int64_t)f.col_blocks * 8) +
         pad256((int64_t)std::max(0, n_local) * 8) + slabs;
}

// FDR_WEIGHT_TOP_DIRS: the centred-rank layout (its weight region holds the top-b weights), then the lane mask
int64_t fused_top_workspace_bytes(int n_dirs, int n_local, int64_t P, int n_all) {
  const int64_t base = fused_workspace_bytes(n_dirs, n_local, P, FDR_WEIGHT_CENTERED_RANK);
  const int64_t mask = top_dirs_workspace_bytes(n_all);
  return base < 0 || mask < 0 ? -1 : base + mask;
}

int launch_fd_grad_fused(const FusedCall& c, void* ws, int64_t ws_bytes, hipStream_t stream) {
  FdArgs a = c.fd;
  const int64_t P = a.P;
  const int n_local = a.n_dirs * a.lpd;
  const bool top = c.mode == FDR_WEIGHT_TOP_DIRS;
  const int64_t need = top ? fused_top_workspace_bytes(a.n_dirs, n_local, P, a.n_all)
                           : fused_workspace_bytes(a.n_dirs, n_local, P, c.mode);
  if (!ws || ws_bytes < need) return set_error(FDR_ERR_WORKSPACE, "fd_grad_fused workspace too small");
  const GradPlan f = fused_plan(a.n_dirs, P);
  char* w = static_cast<char*>(ws);
  const int64_t cnt_b = fused_counter_bytes(a.n_dirs, P);
  const int64_t cb_b = pad256((int64_t)f.col_blocks * 8);
  const int64_t w_b = pad256((int64_t)n_local * 8);
  a.rows_per_chunk = f.rows_per_chunk;
  a.n_chunks = f.n_chunks;
  a.col_blocks = f.col_blocks;
  a.cnt = reinterpret_cast<unsigned*>(w);
  double* gsq = reinterpret_cast<double*>(w + cnt_b);
  double* upart = reinterpret_cast<double*>(w + cnt_b + cb_b);
  a.gsq = c.theta && !c.opt_kind ? gsq : nullptr;  // opt_apply_cb_kernel sums its own fl32(-g)^2
  a.w = reinterpret_cast<double*>(w + cnt_b + 2 * cb_b);
  a.partial = reinterpret_cast<double*>(w + cnt_b + 2 * cb_b + w_b);
  const dim3 grid(f.col_blocks, f.n_chunks);
  switch (c.mode) {
    case FDR_WEIGHT_ZSCORE:
      hipLaunchKernelGGL(fd_grad_fused_kernel<FDR_WEIGHT_ZSCORE>, grid, dim3(256), 0, stream, a);
      break;
    case FDR_WEIGHT_CENTERED_RANK:
      hipLaunchKernelGGL(rank_weights_kernel, dim3((n_local + 255) / 256), dim3(256), 0, stream, a.r_all, a.n_all, a.lo,
                         n_local, const_cast<double*>(a.w));
      hipLaunchKernelGGL(fd_grad_fused_kernel<FDR_WEIGHT_CENTERED_RANK>, grid, dim3(256), 0, stream, a);
      break;
    case FDR_WEIGHT_MOMENTS:
      if (c.theta) return set_error(FDR_ERR_INVALID, "the moments form is reduced across ranks before DSGD");
      hipLaunchKernelGGL(fd_grad_fused_kernel<FDR_WEIGHT_MOMENTS>, grid, dim3(256), 0, stream, a);
      break;
    case FDR_WEIGHT_ZSCORE_MIX:
      hipLaunchKernelGGL(fd_grad_fused_mix_kernel, grid, dim3(256), 0, stream, FdMixArgs{a, c.mix});
      break;
    case FDR_WEIGHT_TOP_DIRS: {  // the top-b weights into the weight region, then the instance that takes weights
      const int64_t mask_off = fused_workspace_bytes(a.n_dirs, n_local, P, FDR_WEIGHT_CENTERED_RANK);
      const int rc = launch_top_dir_weights(a.r_all, a.n_all, a.pr, a.lpd, c.top_dirs, a.lo, n_local,
                                            const_cast<double*>(a.w), nullptr, w + mask_off, ws_bytes - mask_off, stream);
      if (rc) return rc;
      hipLaunchKernelGGL(fd_grad_fused_kernel<FDR_WEIGHT_CENTERED_RANK>, grid, dim3(256), 0, stream, a);
      break;
    }
    default:
      return set_error(FDR_ERR_INVALID, "unknown weighting mode");
  }
  int rc = check_launch("fd_grad_fused_kernel");
  if (rc || !c.theta) return rc;
  if (c.opt_kind)  // fdr_fd_step_opt: the same regions and counter, the optimizer's apply in DSGD's place
    return launch_opt_apply(c.opt_kind, c.theta, a.out, P, c.opt, c.opt_step, c.state0, c.state1, c.hist, gsq, upart,
                            a.cnt + f.col_blocks, c.dsgd_out, stream);
  hipLaunchKernelGGL(dsgd_apply_cb_kernel, dim3(f.col_blocks), dim3(256), 0, stream, c.theta, a.out, P, gsq,
                     f.col_blocks, c.lr, c.lr_scale, c.hist, upart, a.cnt + f.col_blocks, c.dsgd_out);
  return check_launch("dsgd_apply_cb_kernel");
}

int launch_rank_weights(const double* r_all, int n_all, int lo, int n_local, double* w, hipStream_t stream) {
  if (n_local == 0) return FDR_OK;
  hipLaunchKernelGGL(rank_weights_kernel, dim3((n_local + 255) / 256), dim3(256), 0, stream, r_all, n_all, lo, n_local,
                     w);
  return check_launch("rank_weights_kernel");
}

}  // namespace fdr
