// fdr_learner_runs.hip -- the whole FD step of R independent runs in ONE launch (fdr_fd_step_runs): one 256-thread
// workgroup per run does the top-b selection (or the z-score over all lanes), the coefficients, the gradient of the
// run's P <= kRunsMaxP parameters and the DSGD update of the run's theta.  The formulas are include/fdr.h's
// (FDR_WEIGHT_TOP_DIRS / FDR_WEIGHT_ZSCORE, fdr_dsgd_step); at these sizes the fused gradient of fdr_learner_fused.hip,
// tiled for P in the thousands, is all fixed cost, and it steps one theta per call.  Every summation order below is a
// function of the run's own (n_dirs, lanes_per_dir, P) alone, so a run's bits depend neither on R nor on its place in
// the grid.  No workspace, no counters, no hand-off between workgroups.  DESIGN.md 3.2.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "fdr_learner.h"
#include "fdr_reduce.h"

namespace fdr {

constexpr int kRunsTile = 2048;       // scores per LDS tile (top_dirs_select_kernel's tile)
constexpr int kRunsDirsPerPass = 4;   // directions a thread ranks in one pass over the tiles

// max over the direction's lanes of the run's returns (LDS), -inf when one of them is NaN
__device__ __forceinline__ double runs_dir_score(const double* ret, int d, int lpd) {
  const double ninf = -__builtin_inf();
  double s = ninf;
  bool nan = false;
  for (int k = 0; k < lpd; ++k) {
    const double v = ret[d * lpd + k];
    nan = nan || v != v;
    s = v > s ? v : s;
  }
  return nan ? ninf : s;
}

// DSGD of fdr_dsgd.hip on the P <= PMAX values of g every thread holds: the same arithmetic in every thread (sums in
// ascending p), thread 0 stores.  A zero or NaN norm leaves theta untouched, out = [0, norm].
template <int PMAX>
__device__ __forceinline__ void runs_dsgd(const double* g, int P, float* theta, double lr, double lr_scale,
                                          double* out) {
#pragma clang fp contract(off)
  double s = 0.0;
#pragma unroll
  for (int p = 0; p < PMAX; ++p) {
    const float gr = (float)(-g[p]);  // set_grad_from_flat casts to f32 (policy.py:68)
    const double sq = (double)gr * (double)gr;
    s = p < P ? s + sq : s;
  }
  const float norm = (float)sqrt(s);  // flat_grad.norm().item() (dynamic_sgd.py:27)
  double u = 0.0;
  if (norm > 0.f) {
    const double coef = lr * sqrt((double)P) * lr_scale / (double)norm;  // dynamic_sgd.py:30,51
    const float c32 = (float)coef;
#pragma unroll
    for (int p = 0; p < PMAX; ++p) {
      if (p < P) {
        const float gr = (float)(-g[p]);
        const float old = theta[p];
        const float nw = old - c32 * gr;  // p.sub_(coef * grad_slice) (dynamic_sgd.py:36)
        if (threadIdx.x == 0) theta[p] = nw;
        const float dd = old - nw;
        u += (double)dd * (double)dd;
      }
    }
  }
  if (threadIdx.x == 0) {
    out[0] = sqrt(u);
    out[1] = (double)norm;
  }
}

// Workgroup r steps run r.  ret: the run's training returns; tile: one tile of direction scores; keep: rank_d < b.
template <int PMAX>
__global__ __launch_bounds__(256) void fd_step_runs_kernel(FdRunsArgs a) {
  __shared__ double ret[kRunsMaxTrain];
  __shared__ double tile[kRunsTile];
  __shared__ int8_t keep[kRunsMaxTrain];
  __shared__ double red[4];
  const int tid = threadIdx.x, r = blockIdx.x;
  const int D = a.n_dirs, lpd = a.lpd, n = D * lpd, P = a.P;
  const int64_t lane0 = (int64_t)r * a.run_stride;
  const double pr = a.policy_reward ? a.policy_reward[r] : 0.0;
  const int b = a.top_dirs ? a.top_dirs[r] : D;  // NULL: every direction kept, the z-score over all lanes
  const bool bad_b = b < 1 || b > D;

  for (int i = tid; i < n; i += 256) ret[i] = a.rewards[lane0 + i];
  __syncthreads();

  // rank_d = #{e : s_e > s_d, or s_e == s_d and e < d}, counted over LDS tiles of scores without a branch
  // (top_dirs_select_kernel's count); kRunsDirsPerPass directions per thread and pass
  for (int q0 = 0; q0 < D; q0 += 256 * kRunsDirsPerPass) {
    double sd[kRunsDirsPerPass];
    int dc[kRunsDirsPerPass], rank[kRunsDirsPerPass];
#pragma unroll
    for (int e = 0; e < kRunsDirsPerPass; ++e) {
      dc[e] = min(q0 + 256 * e + tid, D - 1);
      sd[e] = runs_dir_score(ret, dc[e], lpd);
      rank[e] = 0;
    }
    for (int t0 = 0; t0 < D; t0 += kRunsTile) {
      const int tn = min(kRunsTile, D - t0);
      __syncthreads();
      for (int k = tid; k < tn; k += 256) tile[k] = runs_dir_score(ret, t0 + k, lpd);
      __syncthreads();
      for (int k = 0; k < tn; ++k) {
        const double se = tile[k];
#pragma unroll
        for (int e = 0; e < kRunsDirsPerPass; ++e)
          rank[e] += (int)(se > sd[e]) | ((int)(se == sd[e]) & (int)(t0 + k < dc[e]));
      }
    }
#pragma unroll
    for (int e = 0; e < kRunsDirsPerPass; ++e) {
      const int d = q0 + 256 * e + tid;
      if (d < D) keep[d] = rank[e] < b ? 1 : 0;
    }
  }
  __syncthreads();

  // two-pass mean / population std of x = r - pr over the kept lanes: thread t takes lanes t, t + 256, .. in lane
  // order, a lane that is not kept adds nothing, block_sum_256's tree (top_dirs_weights_kernel's order)
  const int n_sel = b * lpd;
  double s = 0.0;
  for (int i = tid; i < n; i += 256) {
    const double t = s + (ret[i] - pr);
    s = keep[i / lpd] != 0 ? t : s;
  }
  double mean = block_sum_256(s, red) / (double)n_sel;
  double q = 0.0;
  for (int i = tid; i < n; i += 256) {
    const double dv = (ret[i] - pr) - mean;
    const double t = q + dv * dv;
    q = keep[i / lpd] != 0 ? t : q;
  }
  double sdev = sqrt(block_sum_256(q, red) / (double)n_sel);
  if (bad_b) mean = sdev = __builtin_nan("");  // top_dirs outside 1 .. D: every weight NaN

  // thread t: directions t, t + 256, .. -- the coefficient, then the row into all P columns (f64 registers).  Columns
  // from P to PMAX read the row's last element again and are never summed.
  const double sigma = (double)a.sigma_runs[r];
  double acc[PMAX];
#pragma unroll
  for (int p = 0; p < PMAX; ++p) acc[p] = 0.0;
  for (int d = tid; d < D; d += 256) {
    const bool kept = keep[d] != 0;
    double c = 0.0;
    for (int k = 0; k < lpd; ++k) {
      const int i = d * lpd + k;
      const int sg = a.sign[lane0 + i];
      if (sg == 0) continue;
      const double vi = (double)sg * sigma / a.norm2[lane0 + i];
      const double x = ret[i] - pr;
      const double z = sdev == 0.0 ? x : (x - mean) / sdev;  // math_helpers.py:127-134
      const double w = kept ? z : (sdev != sdev ? sdev : 0.0);
      c += w * vi;
    }
    int64_t off = a.idx[lane0 + (int64_t)d * lpd];
    if (off < 0 || off > a.max_idx) {  // never dereferenced: the row poisons g
      off = 0;
      c = __builtin_nan("");
    }
    const float* row = a.table + off;
#pragma unroll
    for (int p = 0; p < PMAX; ++p) acc[p] = fma(c, (double)row[min(p, P - 1)], acc[p]);
  }
  double g[PMAX];
#pragma unroll
  for (int p = 0; p < PMAX; ++p) {
    g[p] = 0.0;
    if (p < P) g[p] = block_sum_256(acc[p], red);  // P is uniform: every thread meets the barriers
  }
  if (a.g_out && tid == 0) {
#pragma unroll
    for (int p = 0; p < PMAX; ++p)
      if (p < P) a.g_out[(int64_t)r * P + p] = g[p];
  }
  runs_dsgd<PMAX>(g, P, a.theta_runs + (int64_t)r * P, a.lr[r], a.lr_scale, a.out + 2 * (int64_t)r);
}

int launch_fd_step_runs(const FdRunsArgs& a, int n_runs, hipStream_t stream) {
  char msg[160];
  if (a.P > kRunsMaxP) {
    snprintf(msg, sizeof(msg), "fdr_fd_step_runs: n_params %lld above the limit of %d", (long long)a.P, kRunsMaxP);
    return set_error(FDR_ERR_UNSUPPORTED, msg);
  }
  if ((int64_t)a.n_dirs * a.lpd > kRunsMaxTrain) {
    snprintf(msg, sizeof(msg), "fdr_fd_step_runs: %lld training lanes per run above the limit of %d",
             (long long)a.n_dirs * a.lpd, kRunsMaxTrain);
    return set_error(FDR_ERR_UNSUPPORTED, msg);
  }
  if (a.P <= 8)
    hipLaunchKernelGGL(fd_step_runs_kernel<8>, dim3(n_runs), dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL(fd_step_runs_kernel<kRunsMaxP>, dim3(n_runs), dim3(256), 0, stream, a);
  return check_launch("fd_step_runs_kernel");
}

}  // namespace fdr
