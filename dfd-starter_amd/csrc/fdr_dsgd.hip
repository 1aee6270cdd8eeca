// fdr_dsgd.hip -- DSGD (dsgd/dynamic_sgd.py:19-39) from a gradient g or from the all-reduced moments form.
//
//   P <= 65536   dsgd_fused_kernel: ONE 1024-thread workgroup, barriers only
//   larger P     (moments: moment_stats_kernel + moments_to_grad_kernel, then) dsgd_norm_kernel, dsgd_apply_kernel,
//                dsgd_final_kernel over up to 256 blocks, partials combined in block order
// Same per-element arithmetic and the same f32 norm either way.  The DSGD that follows the fused gradient in one
// call (fdr_fd_step) is dsgd_apply_cb_kernel in fdr_learner_fused.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "fdr_learner.h"
#include "fdr_reduce.h"

namespace fdr {

constexpr int kDsgdBlocks = 256;

// The workspace of the large-P path, in doubles.  Its three kernels run nb <= kDsgdBlocks blocks and pack their
// regions by that grid, indexing them themselves (gridDim.x, dsgd_final_kernel's nb); the statistics of the moments
// form sit past the widest such packing.
struct DsgdWs {
  static constexpr int kPartMax = 2 * kDsgdBlocks + 1;  // the widest packing of `part`
  static constexpr int kStats = 2 * kDsgdBlocks + 2;
  static constexpr int kDoubles = 2 * kDsgdBlocks + 8;
  double* part;   // [nb] sum fl32(-g)^2 per block | [nb] sum (d theta)^2 per block | [1] ||fl32(-g)||
  double* stats;  // [2] mean, sd of all ranks' r'
  explicit DsgdWs(void* ws) : part(static_cast<double*>(ws)), stats(part + kStats) {}
};
static_assert(DsgdWs::kPartMax <= DsgdWs::kStats && DsgdWs::kStats + 2 <= DsgdWs::kDoubles,
              "dsgd workspace regions overlap");

int64_t dsgd_workspace_bytes(int64_t) { return (int64_t)DsgdWs::kDoubles * sizeof(double); }

__global__ __launch_bounds__(256) void dsgd_norm_kernel(const double* __restrict__ g, int64_t P,
                                                         double* __restrict__ part) {
  __shared__ double red[4];
  double s = 0.0;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P;
       p += (int64_t)gridDim.x * blockDim.x) {
    const float gr = (float)(-g[p]);  // set_grad_from_flat casts to f32 (policy.py:68)
    s += (double)gr * (double)gr;
  }
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void dsgd_apply_kernel(float* __restrict__ theta,
                                                          const double* __restrict__ g, int64_t P,
                                                          double lr, double lr_scale,
                                                          double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  // every block re-reduces the norm partials in the same fixed order -> identical coef
  double ss = 0.0;
  for (int i = 0; i < (int)gridDim.x; ++i) ss += part[i];
  const float norm = (float)sqrt(ss);  // flat_grad.norm().item() (dynamic_sgd.py:27)
  double s = 0.0;
  if (norm > 0.f) {
    const double coef = lr * sqrt((double)P) * lr_scale / (double)norm;  // dynamic_sgd.py:30,51
    const float c32 = (float)coef;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P;
         p += (int64_t)gridDim.x * blockDim.x) {
      const float gr = (float)(-g[p]);
      const float old = theta[p];
      const float nw = old - c32 * gr;  // p.sub_(coef * grad_slice) (dynamic_sgd.py:36)
      theta[p] = nw;
      const float dd = old - nw;
      s += (double)dd * (double)dd;
    }
  }
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) part[gridDim.x + blockIdx.x] = s;
  if (blockIdx.x == 0 && threadIdx.x == 0) part[2 * gridDim.x] = (double)norm;
}

__global__ void dsgd_final_kernel(const double* __restrict__ part, int nb, double* __restrict__ out) {
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < nb; ++i) s += part[nb + i];
    out[0] = sqrt(s);
    out[1] = part[2 * nb];
  }
}

static int launch_dsgd(float* theta, const double* g, int64_t P, double lr, double lr_scale, double* out,
                       void* ws, int64_t ws_bytes, hipStream_t stream) {
  if (ws == nullptr || ws_bytes < dsgd_workspace_bytes(P))
    return set_error(FDR_ERR_WORKSPACE, "dsgd workspace too small");
  double* part = DsgdWs(ws).part;
  const int nb = (int)std::min<int64_t>(kDsgdBlocks, (P + 255) / 256);
  hipLaunchKernelGGL(dsgd_norm_kernel, dim3(nb), dim3(256), 0, stream, g, P, part);
  int rc = check_launch("dsgd_norm_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(dsgd_apply_kernel, dim3(nb), dim3(256), 0, stream, theta, g, P, lr, lr_scale, part);
  rc = check_launch("dsgd_apply_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(dsgd_final_kernel, dim3(1), dim3(64), 0, stream, part, nb, out);
  return check_launch("dsgd_final_kernel");
}

// ------------------------------------------------------------------------------------------
// Fused DSGD (P <= kDsgdFusedMaxP): ONE 1024-thread workgroup does the norm of fl32(-g), the update
// and ||d theta|| (dynamic_sgd.py:19-39) with barriers only.  src = g, or (moments form) the summed
// [A | B | sum r' | sum r'^2 | n] from which g = (A - m B) / sd (z-score identity), also
// written to g_out.  Same per-element arithmetic and the same f32 norm as the 3-kernel path.
// ------------------------------------------------------------------------------------------
constexpr int64_t kDsgdFusedMaxP = 1 << 16;

__device__ __forceinline__ double grad_elem(const double* src, int64_t P, int64_t p, bool mom, double m, double sd) {
  if (!mom) return src[p];
  const double A = src[p], B = src[P + p];
  return sd == 0.0 ? A : (A - m * B) / sd;  // standardize_arr returns its input unchanged when std == 0
}

// z-score statistics of the summed moments [A | B | n | r'_0 .. r'_{n-1}]: mean and population std of all
// ranks' r' in two f64 passes (utils/math_helpers.py:127-134), by a 1024-thread workgroup in a fixed order
__device__ void moment_stats_1024(const double* src, int64_t P, double* red, double& m, double& sd) {
  const int n = (int)src[2 * P];
  const double* r = src + 2 * P + 1;
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) s += r[i];
  m = block_sum_1024(s, red) / (double)n;
  double q = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) {
    const double d = r[i] - m;
    q += d * d;
  }
  sd = sqrt(block_sum_1024(q, red) / (double)n);
}

__global__ __launch_bounds__(1024) void dsgd_fused_kernel(float* __restrict__ theta, const double* __restrict__ src,
                                                          int64_t P, int mom, double lr, double lr_scale,
                                                          double* __restrict__ g_out, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double red[16];
  double m = 0.0, sd = 0.0;
  if (mom) moment_stats_1024(src, P, red, m, sd);
  double s = 0.0;
  for (int64_t p = threadIdx.x; p < P; p += 1024) {
    const double g = grad_elem(src, P, p, mom, m, sd);
    if (mom && g_out) g_out[p] = g;
    const float gr = (float)(-g);
    s += (double)gr * (double)gr;
  }
  const float norm = (float)sqrt(block_sum_1024(s, red));
  double u = 0.0;
  if (norm > 0.f) {
    const double coef = lr * sqrt((double)P) * lr_scale / (double)norm;
    const float c32 = (float)coef;
    for (int64_t p = threadIdx.x; p < P; p += 1024) {
      const float gr = (float)(-grad_elem(src, P, p, mom, m, sd));
      const float old = theta[p];
      const float nw = old - c32 * gr;
      theta[p] = nw;
      const float dd = old - nw;
      u += (double)dd * (double)dd;
    }
  }
  u = block_sum_1024(u, red);
  if (threadIdx.x == 0) {
    out[0] = sqrt(u);
    out[1] = (double)norm;
  }
}

// multi-block path for large P (ImpalaPolicy): the statistics once, then g = (A - m B) / sd
__global__ __launch_bounds__(1024) void moment_stats_kernel(const double* __restrict__ src, int64_t P,
                                                            double* __restrict__ stats) {
  __shared__ double red[16];
  double m, sd;
  moment_stats_1024(src, P, red, m, sd);
  if (threadIdx.x == 0) {
    stats[0] = m;
    stats[1] = sd;
  }
}

__global__ __launch_bounds__(256) void moments_to_grad_kernel(const double* __restrict__ src, int64_t P,
                                                              const double* __restrict__ stats,
                                                              double* __restrict__ g) {
  const double m = stats[0], sd = stats[1];
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (int64_t)gridDim.x * blockDim.x)
    g[p] = grad_elem(src, P, p, true, m, sd);
}

// the moments form's g at any P: the statistics into stats [2], then g = (A - m B) / sd into g_out (also the first
// half of fdr_optim.hip's launch_opt_step)
int launch_moments_to_grad(const double* src, int64_t P, double* stats, double* g_out, hipStream_t stream) {
  hipLaunchKernelGGL(moment_stats_kernel, dim3(1), dim3(1024), 0, stream, src, P, stats);
  int rc = check_launch("moment_stats_kernel");
  if (rc) return rc;
  const int rb = (int)std::min<int64_t>((P + 255) / 256, 2048);
  hipLaunchKernelGGL(moments_to_grad_kernel, dim3(rb), dim3(256), 0, stream, src, P, stats, g_out);
  return check_launch("moments_to_grad_kernel");
}

int launch_dsgd_ex(float* theta, const double* src, int mom, int64_t P, double lr, double lr_scale, double* g_out,
                   double* out, void* ws, int64_t ws_bytes, hipStream_t stream) {
  if (P <= kDsgdFusedMaxP) {
    hipLaunchKernelGGL(dsgd_fused_kernel, dim3(1), dim3(1024), 0, stream, theta, src, P, mom, lr, lr_scale, g_out, out);
    return check_launch("dsgd_fused_kernel");
  }
  const double* g = src;
  if (mom) {
    if (!g_out) return set_error(FDR_ERR_INVALID, "moments form needs g_out for large P");
    if (ws == nullptr || ws_bytes < dsgd_workspace_bytes(P))
      return set_error(FDR_ERR_WORKSPACE, "dsgd workspace too small");
    const int rc = launch_moments_to_grad(src, P, DsgdWs(ws).stats, g_out, stream);
    if (rc) return rc;
    g = g_out;
  }
  return launch_dsgd(theta, g, P, lr, lr_scale, out, ws, ws_bytes, stream);
}

}  // namespace fdr
