// fdr_top_dirs.hip -- top-b direction selection (the weighting of Augmented Random Search; build extension, the
// reference has no counterpart): the b best directions by max over their lanes' returns keep their lanes, z-scored
// over the kept lanes alone; every other lane weighs 0.  Two small kernels in front of
// fd_grad_fused_kernel<FDR_WEIGHT_CENTERED_RANK>, which consumes per-lane weights as they are (fdr_learner_fused.hip).
#include <hip/hip_runtime.h>

#include "fdr_learner.h"
#include "fdr_reduce.h"

namespace fdr {

constexpr int kTopTile = 2048;  // scores per LDS tile (rank_weights_kernel's tile)
constexpr int kTopMaxLpd = 4;   // lanes of a direction loaded at once (longer directions: further rounds)

// s = max over the direction's lanes, -inf when one of them is NaN.  Branch-free (fdr_learner_fused.hip says why):
// every round loads kTopMaxLpd lanes at indices clamped into the direction and selects the live ones.
__device__ __forceinline__ double dir_score(const double* __restrict__ r_all, int d, int lpd) {
  const double ninf = -__builtin_inf();
  double s = ninf;
  bool nan = false;
  const int64_t base = (int64_t)d * lpd;
  for (int k0 = 0; k0 < lpd; k0 += kTopMaxLpd) {
    double v[kTopMaxLpd];
#pragma unroll
    for (int k = 0; k < kTopMaxLpd; ++k) v[k] = r_all[base + min(k0 + k, lpd - 1)];
#pragma unroll
    for (int k = 0; k < kTopMaxLpd; ++k) {
      const bool live = k0 + k < lpd;
      nan = nan || (live && v[k] != v[k]);
      s = (live && v[k] > s) ? v[k] : s;
    }
  }
  return nan ? ninf : s;
}

// One thread per GLOBAL direction d < D: rank_d = #{e : s_e > s_d, or s_e == s_d and e < d} counted over LDS tiles
// of scores (each formed from its lanes while the tile is filled); lane_mask[i] = rank_d < b for the lanes of d.
// A stable descending order: exactly b directions are kept, ties go to the lower index.  Every rank runs this over
// all directions, so every rank holds the same mask.
__global__ __launch_bounds__(256) void top_dirs_select_kernel(const double* __restrict__ r_all, int D, int lpd, int b,
                                                              int8_t* __restrict__ lane_mask) {
  __shared__ double tile[kTopTile];
  const int d = blockIdx.x * 256 + threadIdx.x;
  const int dc = min(d, D - 1);
  const double sd = dir_score(r_all, dc, lpd);
  int rank = 0;
  for (int t0 = 0; t0 < D; t0 += kTopTile) {
    const int tn = min(kTopTile, D - t0);
    __syncthreads();
    for (int k = threadIdx.x; k < tn; k += 256) tile[k] = dir_score(r_all, t0 + k, lpd);
    __syncthreads();
    // 8 scores per round (four ds_read_b128 issued together) and a bitwise count that compiles without a branch.
    // Measured against rank_weights_kernel's form of this loop (one read and one `||` per compare, a branch per
    // compare in the ISA): both kernels of this file 61 us instead of 152 us at D = 2048, 457 us instead of 1180 us at
    // D = 16384 (tools/learner_bench.py n_dirs P top); the two changes were not timed apart.
    int k = 0;
    for (; k + 8 <= tn; k += 8) {
      double se[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) se[e] = tile[k + e];
#pragma unroll
      for (int e = 0; e < 8; ++e)
        rank += (int)(se[e] > sd) | ((int)(se[e] == sd) & (int)(t0 + k + e < dc));
    }
    for (; k < tn; ++k) {
      const double se = tile[k];
      rank += (se > sd || (se == sd && t0 + k < dc)) ? 1 : 0;
    }
  }
  if (d < D) {
    const int8_t m = rank < b ? 1 : 0;
    for (int k = 0; k < lpd; ++k) lane_mask[(int64_t)d * lpd + k] = m;
  }
}

// Every workgroup forms m and sd of x = r - pr over the kept lanes in ONE fixed order -- thread t takes lanes t,
// t + 256, .. in lane order, a lane that is not kept adds nothing, block_sum_256's tree, two passes -- so the
// statistics do not depend on the grid and agree bit for bit in every workgroup and on every rank; then it writes
// the weights of its 256 local lanes.  The per-thread order and the expressions are the z-score instance's
// (fd_grad_fused_kernel<FDR_WEIGHT_ZSCORE>): with every direction kept these are its statistics and its weights.
// n_sel = b * lpd, the kept lanes.  A kept NaN makes m, sd and with them every weight NaN, as in the z-score.
// The bit equality at b == D depends on the compiler: `q + dv * dv` here and `q += d * d` there must both contract to
// one fma (two units, no fp-contract pragma on either side).  tests/test_gpu_top_dirs.py
// (test_all_kept_is_bitwise_the_zscore_instance) holds it; touch either side and run that test.
constexpr int kTopFlight = 8;  // lanes per thread in flight in the statistics passes

__global__ __launch_bounds__(256) void top_dirs_weights_kernel(const double* __restrict__ r_all, int n_all, double pr,
                                                               const int8_t* __restrict__ lane_mask, int n_sel, int lpd,
                                                               int lo, int n_local, double* __restrict__ w,
                                                               int8_t* __restrict__ selected) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * 256 + tid;
  const int gi = lo + min(i, n_local - 1);
  const double xi = r_all[gi] - pr;
  const bool mi = lane_mask[gi] != 0;
  double s = 0.0;
  for (int b0 = 0; b0 < n_all; b0 += 256 * kTopFlight) {
    double x[kTopFlight];
    int8_t m[kTopFlight];
#pragma unroll
    for (int e = 0; e < kTopFlight; ++e) {
      const int j = min(b0 + 256 * e + tid, n_all - 1);
      x[e] = r_all[j];
      m[e] = lane_mask[j];
    }
#pragma unroll
    for (int e = 0; e < kTopFlight; ++e) {
      const double t = s + (x[e] - pr);
      s = (b0 + 256 * e + tid < n_all && m[e] != 0) ? t : s;
    }
  }
  const double mean = block_sum_256(s, red) / (double)n_sel;
  double q = 0.0;
  for (int b0 = 0; b0 < n_all; b0 += 256 * kTopFlight) {
    double x[kTopFlight];
    int8_t m[kTopFlight];
#pragma unroll
    for (int e = 0; e < kTopFlight; ++e) {
      const int j = min(b0 + 256 * e + tid, n_all - 1);
      x[e] = r_all[j];
      m[e] = lane_mask[j];
    }
#pragma unroll
    for (int e = 0; e < kTopFlight; ++e) {
      const double dv = (x[e] - pr) - mean;
      const double t = q + dv * dv;
      q = (b0 + 256 * e + tid < n_all && m[e] != 0) ? t : q;
    }
  }
  const double sd = sqrt(block_sum_256(q, red) / (double)n_sel);
  if (i < n_local) {
    const double z = sd == 0.0 ? xi : (xi - mean) / sd;  // math_helpers.py:127-134, as FDR_WEIGHT_ZSCORE
    w[i] = mi ? z : (sd != sd ? sd : 0.0);
    if (selected && gi % lpd == 0) selected[i / lpd] = mi ? 1 : 0;
  }
}

int64_t top_dirs_workspace_bytes(int n_all) { return n_all > 0 ? ((int64_t)n_all + 255) / 256 * 256 : -1; }

int launch_top_dir_weights(const double* r_all, int n_all, double pr, int lpd, int top_dirs, int lo, int n_local,
                           double* w, int8_t* selected, void* ws, int64_t ws_bytes, hipStream_t stream) {
  if (n_local == 0) return FDR_OK;
  if (!ws || ws_bytes < top_dirs_workspace_bytes(n_all))
    return set_error(FDR_ERR_WORKSPACE, "top_dir_weights workspace too small");
  int8_t* mask = static_cast<int8_t*>(ws);
  const int D = n_all / lpd;
  hipLaunchKernelGGL(top_dirs_select_kernel, dim3((D + 255) / 256), dim3(256), 0, stream, r_all, D, lpd, top_dirs, mask);
  int rc = check_launch("top_dirs_select_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(top_dirs_weights_kernel, dim3((n_local + 255) / 256), dim3(256), 0, stream, r_all, n_all, pr, mask,
                     top_dirs * lpd, lpd, lo, n_local, w, selected);
  return check_launch("top_dirs_weights_kernel");
}

}  // namespace fdr
