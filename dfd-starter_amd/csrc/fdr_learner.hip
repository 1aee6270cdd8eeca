// fdr_learner.hip -- perturbation batch, FD weighting, the staged noise-weighted gradient, delayed returns.
//
// All of these are HBM-bound integer/byte-indexed streams (DESIGN.md "Learner kernels"):
//   perturb       reads P floats of theta (L2-resident) + n*P table floats, writes n*P
//   fd_weights    one workgroup, N rewards (a few KB)
//   fd_grad       reads n_dirs * P table floats once (dword loads: table offsets are arbitrary,
//                 so rows are only 4-B aligned), f64 column partial sums per row-chunk, then a
//                 fixed-order chunk reduce -> deterministic result independent of launch shape
//   lambda_*      the same tiling over delayed returns' rows sign sigma eps + drift
// The fused step is fdr_learner_fused.hip, DSGD fdr_dsgd.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "fdr_learner.h"
#include "fdr_reduce.h"

namespace fdr {

// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void perturb_kernel(const float* __restrict__ theta, int64_t P,
                                                       const float* __restrict__ table, int64_t max_idx,
                                                       const int64_t* __restrict__ idx,
                                                       const int8_t* __restrict__ sign, float sigma,
                                                       float* __restrict__ out) {
#pragma clang fp contract(off)
  const int l = blockIdx.y;
  const int s = sign ? sign[l] : 1;
  const int64_t off = idx[l];
  const bool bad = off < 0 || off > max_idx;  // never dereference an out-of-range offset
  const float* eps = table + (bad ? 0 : off);
  float* o = out + (int64_t)l * P;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P;
       p += (int64_t)gridDim.x * blockDim.x) {
    const float t = theta[p];
    if (bad) {
      o[p] = __builtin_nanf("");
      continue;
    }
    const float st = sigma * eps[p];
    o[p] = s > 0 ? t + st : (s < 0 ? t - st : t);
  }
}

int launch_perturb(const float* theta, int64_t P, const float* table, int64_t table_size,
                   const int64_t* idx, const int8_t* sign, int n, float sigma, float* out,
                   hipStream_t stream) {
  const int bx = (int)std::min<int64_t>((P + 255) / 256, 64);
  hipLaunchKernelGGL(perturb_kernel, dim3(bx, n), dim3(256), 0, stream, theta, P, table,
                     table_size - P, idx, sign, sigma, out);
  return check_launch("perturb_kernel");
}

// ------------------------------------------------------------------------------------------
// FD weighting: one 1024-thread workgroup.  Deterministic tree sums in f64.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void fd_weights_kernel(const double* __restrict__ r_all, int n_all,
                                                           double pr, int lo, int n_local,
                                                           const int8_t* __restrict__ sign,
                                                           const double* __restrict__ n2, int lpd,
                                                           float sigma, double* __restrict__ coef) {
  __shared__ double red[16];
  double s = 0.0;
  for (int i = threadIdx.x; i < n_all; i += blockDim.x) s += r_all[i] - pr;
  const double mean = block_sum_1024(s, red) / (double)n_all;
  double q = 0.0;
  for (int i = threadIdx.x; i < n_all; i += blockDim.x) {
    const double d = (r_all[i] - pr) - mean;
    q += d * d;
  }
  const double var = block_sum_1024(q, red) / (double)n_all;
  const double sd = sqrt(var);
  const int n_dirs = n_local / lpd;
  for (int d = threadIdx.x; d < n_dirs; d += blockDim.x) {
    double c = 0.0;
    for (int k = 0; k < lpd; ++k) {
      const int i = d * lpd + k;
      const int sg = sign[i];
      if (sg == 0) continue;
      const double x = r_all[lo + i] - pr;
      const double z = sd == 0.0 ? x : (x - mean) / sd;  // utils/math_helpers.py:127-134
      c += z * (double)sg * (double)sigma / n2[i];
    }
    coef[d] = c;
  }
}

int launch_fd_weights(const double* r_all, int n_all, double pr, int lo, int n_local,
                      const int8_t* sign, const double* n2, int lpd, float sigma, double* coef,
                      hipStream_t stream) {
  hipLaunchKernelGGL(fd_weights_kernel, dim3(1), dim3(1024), 0, stream, r_all, n_all, pr, lo,
                     n_local, sign, n2, lpd, sigma, coef);
  return check_launch("fd_weights_kernel");
}

// The mixed objective's staged weighting (fdr_fd_weights_mix; the delayed-return route): fd_weights_kernel with a
// z-score per active channel (MixChannels), each over the same per-thread order and workgroup tree; an inactive
// channel's array is not read.  With coefficients (1, 0, 0) the coefficients are fd_weights_kernel's bits.
__global__ __launch_bounds__(1024) void fd_weights_mix_kernel(MixChannels mx, int n_all, int lo, int n_local,
                                                               const int8_t* __restrict__ sign,
                                                               const double* __restrict__ n2, int lpd, float sigma,
                                                               double* __restrict__ coef) {
  __shared__ double red[16];
  double mean[3] = {0.0, 0.0, 0.0}, sd[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (mx.a[c] == 0.0) continue;  // uniform
    const double* __restrict__ v = mx.v[c];
    const double p = mx.p[c];
    double s = 0.0;
    for (int i = threadIdx.x; i < n_all; i += blockDim.x) s += v[i] - p;
    mean[c] = block_sum_1024(s, red) / (double)n_all;
    double q = 0.0;
    for (int i = threadIdx.x; i < n_all; i += blockDim.x) {
      const double d = (v[i] - p) - mean[c];
      q += d * d;
    }
    sd[c] = sqrt(block_sum_1024(q, red) / (double)n_all);
  }
  const int n_dirs = n_local / lpd;
  for (int d = threadIdx.x; d < n_dirs; d += blockDim.x) {
    double cf = 0.0;
    for (int k = 0; k < lpd; ++k) {
      const int i = d * lpd + k;
      const int sg = sign[i];
      if (sg == 0) continue;
      double w = 0.0;
      bool any = false;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (mx.a[c] == 0.0) continue;
        const double x = mx.v[c][lo + i] - mx.p[c];
        const double t = mx.a[c] * (sd[c] == 0.0 ? x : (x - mean[c]) / sd[c]);  // utils/math_helpers.py:127-134
        w = any ? w + t : t;
        any = true;
      }
      cf += w * (double)sg * (double)sigma / n2[i];
    }
    coef[d] = cf;
  }
}

int launch_fd_weights_mix(const MixChannels& mx, int n_all, int lo, int n_local, const int8_t* sign, const double* n2,
                          int lpd, float sigma, double* coef, hipStream_t stream) {
  hipLaunchKernelGGL(fd_weights_mix_kernel, dim3(1), dim3(1024), 0, stream, mx, n_all, lo, n_local, sign, n2, lpd,
                     sigma, coef);
  return check_launch("fd_weights_mix_kernel");
}

// ------------------------------------------------------------------------------------------
// Noise-weighted gradient: g[p] = sum_d coef[d] * table[idx[d] + p]
// ------------------------------------------------------------------------------------------
constexpr int kGradThreads = 256;  // one column per thread: a wave reads 256 contiguous bytes per row
constexpr int kGradMinRows = 64;   // rows per chunk: bounds the partial slabs to n_dirs/64 * P * 8 B

static GradPlan grad_plan(int n_dirs, int64_t P) {
  GradPlan g;
  g.col_blocks = (int)((P + kGradThreads - 1) / kGradThreads);
  // aim for ~1024 workgroups (4 per CU) without letting the slab count explode
  const int target_chunks = std::max(1, 1024 / std::max(1, g.col_blocks));
  g.rows_per_chunk = std::max(kGradMinRows, (n_dirs + target_chunks - 1) / target_chunks);
  g.n_chunks = (n_dirs + g.rows_per_chunk - 1) / g.rows_per_chunk;
  return g;
}

int64_t grad_workspace_bytes(int n_dirs, int64_t P) {
  if (n_dirs <= 0 || P <= 0) return 0;
  const GradPlan g = grad_plan(n_dirs, P);
  return (int64_t)g.n_chunks * P * (int64_t)sizeof(double);
}

__global__ __launch_bounds__(kGradThreads) void fd_grad_partial_kernel(
    const float* __restrict__ table, int64_t max_idx, const int64_t* __restrict__ idx,
    const double* __restrict__ coef, int n_dirs, int64_t P, int rows_per_chunk,
    double* __restrict__ partial) {
  const int64_t c = (int64_t)blockIdx.x * kGradThreads + threadIdx.x;
  const int chunk = blockIdx.y;
  const int d0 = chunk * rows_per_chunk;
  const int d1 = min(n_dirs, d0 + rows_per_chunk);
  const bool ok = c < P;
  const int64_t cc = ok ? c : 0;
  // an out-of-range offset reads row 0 with a NaN weight: the gradient is poisoned, never a fault
  auto row = [&](int dd, double& w) {
    const int64_t off = idx[dd];
    const bool bad = off < 0 || off > max_idx;
    w = bad ? __builtin_nan("") : coef[dd];
    return table + (bad ? 0 : off);
  };
  double acc0 = 0.0, acc1 = 0.0;
  int d = d0;
  for (; d + 4 <= d1; d += 4) {  // four rows in flight
    double w0, w1, w2, w3;
    const float v0 = row(d, w0)[cc], v1 = row(d + 1, w1)[cc];
    const float v2 = row(d + 2, w2)[cc], v3 = row(d + 3, w3)[cc];
    acc0 = fma(w0, (double)v0, acc0);
    acc1 = fma(w1, (double)v1, acc1);
    acc0 = fma(w2, (double)v2, acc0);
    acc1 = fma(w3, (double)v3, acc1);
  }
  for (; d < d1; ++d) {
    double w;
    const float v = row(d, w)[cc];
    acc0 = fma(w, (double)v, acc0);
  }
  if (ok) partial[(int64_t)chunk * P + c] = acc0 + acc1;
}

__global__ __launch_bounds__(256) void fd_grad_reduce_kernel(const double* __restrict__ partial,
                                                              int n_chunks, int64_t P,
                                                              double* __restrict__ g) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P;
       p += (int64_t)gridDim.x * blockDim.x) {
    double s = 0.0;
    for (int c = 0; c < n_chunks; ++c) s += partial[(int64_t)c * P + p];
    g[p] = s;
  }
}

// What launch_fd_grad and launch_lambda_grad share: the workspace check, then `partial_pass` (the caller's launch
// of its partial kernel into the slabs, named `what`), then the chunk reduce in chunk order.
template <class PartialPass>
static int grad_in_chunks(int n, int64_t P, double* g, void* ws, int64_t ws_bytes, hipStream_t stream,
                          const char* what, PartialPass partial_pass) {
  const GradPlan pl = grad_plan(n, P);
  if (ws_bytes < grad_workspace_bytes(n, P) || ws == nullptr)
    return set_error(FDR_ERR_WORKSPACE, "fd_grad workspace too small");
  double* partial = static_cast<double*>(ws);
  partial_pass(pl, partial);
  int rc = check_launch(what);
  if (rc) return rc;
  const int rb = (int)std::min<int64_t>((P + 255) / 256, 2048);
  hipLaunchKernelGGL(fd_grad_reduce_kernel, dim3(rb), dim3(256), 0, stream, partial, pl.n_chunks, P, g);
  return check_launch("fd_grad_reduce_kernel");
}

int launch_fd_grad(const float* table, int64_t table_size, const int64_t* idx, const double* coef,
                   int n_dirs, int64_t P, double* g, void* ws, int64_t ws_bytes, hipStream_t stream) {
  return grad_in_chunks(n_dirs, P, g, ws, ws_bytes, stream, "fd_grad_partial_kernel",
                        [&](const GradPlan& pl, double* partial) {
    hipLaunchKernelGGL(fd_grad_partial_kernel, dim3(pl.col_blocks, pl.n_chunks), dim3(kGradThreads), 0,
                       stream, table, table_size - P, idx, coef, n_dirs, P, pl.rows_per_chunk, partial);
  });
}

// ------------------------------------------------------------------------------------------
// Delayed returns (learner/finite_differences.py:66-73, 80-114): the perturbation of return i is
//   lambda_i[p] = fl32( sign_i * fl32(sigma * eps_i[p]) + D_{slot_i}[p] ),  D = dist_map[epoch_i]
// (theta of that epoch minus the current theta; slot < 0: current epoch, D = 0).  Norms and the
// gradient g = sum_i coef_i * lambda_i run over returns, in the fd_grad tiling, f64 accumulation.
// ------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void lambda_norm_kernel(LambdaRow R, double* __restrict__ n2) {
  const int i = blockIdx.x;
  bool bad;
  const float* e = R.eps(i, bad);
  const float* d = R.dr(i);
  const int sg = R.sign ? (int)R.sign[i] : 1;
  double acc = 0.0;
  for (int64_t p = threadIdx.x; p < R.P; p += 256) {
    const double v = R.value(e, d, sg, p);
    acc = fma(v, v, acc);
  }
  __shared__ double red[256 / kWave];
  wave_sums_256(acc, red);
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < 256 / kWave; ++w) t += red[w];
    n2[i] = bad ? __builtin_nan("") : t;
  }
}

__global__ __launch_bounds__(kGradThreads) void lambda_grad_partial_kernel(LambdaRow R, const double* __restrict__ coef,
                                                                          int n, int rows_per_chunk,
                                                                          double* __restrict__ partial) {
  const int64_t c = (int64_t)blockIdx.x * kGradThreads + threadIdx.x;
  const int chunk = blockIdx.y;
  const int d0 = chunk * rows_per_chunk, d1 = min(n, d0 + rows_per_chunk);
  const bool ok = c < R.P;
  const int64_t cc = ok ? c : 0;
  double acc0 = 0.0, acc1 = 0.0;
  int i = d0;
  for (; i + 2 <= d1; i += 2) {
    bool b0, b1;
    const float* e0 = R.eps(i, b0);
    const float* e1 = R.eps(i + 1, b1);
    const float v0 = R.value(e0, R.dr(i), R.sign ? (int)R.sign[i] : 1, cc);
    const float v1 = R.value(e1, R.dr(i + 1), R.sign ? (int)R.sign[i + 1] : 1, cc);
    acc0 = fma(b0 ? __builtin_nan("") : coef[i], (double)v0, acc0);
    acc1 = fma(b1 ? __builtin_nan("") : coef[i + 1], (double)v1, acc1);
  }
  for (; i < d1; ++i) {
    bool b;
    const float* e = R.eps(i, b);
    const float v = R.value(e, R.dr(i), R.sign ? (int)R.sign[i] : 1, cc);
    acc0 = fma(b ? __builtin_nan("") : coef[i], (double)v, acc0);
  }
  if (ok) partial[(int64_t)chunk * R.P + c] = acc0 + acc1;
}

int launch_lambda_norms(const LambdaRow& R, int n, double* n2, hipStream_t stream) {
  if (n == 0) return FDR_OK;
  hipLaunchKernelGGL(lambda_norm_kernel, dim3(n), dim3(256), 0, stream, R, n2);
  return check_launch("lambda_norm_kernel");
}

int launch_lambda_grad(const LambdaRow& R, const double* coef, int n, double* g, void* ws, int64_t ws_bytes,
                       hipStream_t stream) {
  return grad_in_chunks(n, R.P, g, ws, ws_bytes, stream, "lambda_grad_partial_kernel",
                        [&](const GradPlan& pl, double* partial) {
    hipLaunchKernelGGL(lambda_grad_partial_kernel, dim3(pl.col_blocks, pl.n_chunks), dim3(kGradThreads), 0, stream,
                       R, coef, n, pl.rows_per_chunk, partial);
  });
}

}  // namespace fdr
