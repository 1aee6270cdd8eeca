// fdr_mlp_vbn.hip -- DiscretePolicy.compute_vbn on the device (fdr_bn_refresh).
#include <hip/hip_runtime.h>

#include <cmath>

#include "fdr_learner.h"
#include "fdr_reduce.h"

namespace fdr {

// ------------------------------------------------------------------------------------------
// BatchNorm running-stat refresh of the DiscretePolicy (policies/policy.py:31-34 compute_vbn,
// policies/discrete.py:34-48): one train-mode pass of the buffer; each BN normalises with its batch
// statistics (biased variance) and folds mean / unbiased variance into its running stats.
// ------------------------------------------------------------------------------------------
constexpr float kVbnEps = 1e-5f;

__global__ __launch_bounds__(256) void col_stats_kernel(const float* __restrict__ X, int n, int C,
                                                        double* __restrict__ mean, double* __restrict__ var) {
  const int c = blockIdx.x;
  __shared__ double red[256 / kWave];
  __shared__ double mu;
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += X[(int64_t)i * C + c];
  wave_sums_256(s, red);
  if (threadIdx.x == 0) mu = (red[0] + red[1] + red[2] + red[3]) / n;
  __syncthreads();
  double q = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double d = X[(int64_t)i * C + c] - mu;
    q = fma(d, d, q);
  }
  __syncthreads();
  wave_sums_256(q, red);
  if (threadIdx.x == 0) {
    mean[c] = mu;
    var[c] = (red[0] + red[1] + red[2] + red[3]) / n;  // biased: what train-mode BN normalises with
  }
}

// Y[i][j] = relu(b_j + sum_k W[j][k] * BN_batch(X[i][k]))
__global__ __launch_bounds__(256) void bn_linear_relu_kernel(const float* __restrict__ X, int n, int Cin,
                                                             const double* __restrict__ mean, const double* __restrict__ var,
                                                             const float* __restrict__ bw, const float* __restrict__ bb,
                                                             const float* __restrict__ W, const float* __restrict__ b,
                                                             int Cout, float* __restrict__ Y) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)n * Cout) return;
  const int i = (int)(t / Cout), j = (int)(t % Cout);
  float acc = b[j];
  for (int k = 0; k < Cin; ++k) {
    const float inv = 1.f / sqrtf((float)var[k] + kVbnEps);
    const float xn = ((X[(int64_t)i * Cin + k] - (float)mean[k]) * inv) * bw[k] + bb[k];
    acc = fmaf(W[j * Cin + k], xn, acc);
  }
  Y[t] = acc > 0.f ? acc : 0.f;
}

__global__ void bn_running_update_kernel(int C, int n, float momentum, const double* __restrict__ mean,
                                         const double* __restrict__ var, float* __restrict__ rm,
                                         float* __restrict__ rv) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float unb = (float)(var[c] * (double)n / (double)(n - 1));
  rm[c] = momentum * (float)mean[c] + (1.f - momentum) * rm[c];
  rv[c] = momentum * unb + (1.f - momentum) * rv[c];
}

int64_t bn_refresh_workspace_bytes(int n) { return (int64_t)n * 64 * 4 * 2 + 6 * 64 * 8 + 256; }

int launch_bn_refresh(int n_in, const float* theta, const float* x, int n, float momentum, float* rm, float* rv,
                      void* ws, int64_t ws_bytes, hipStream_t stream) {
  if (ws_bytes < bn_refresh_workspace_bytes(n) || !ws) return set_error(FDR_ERR_WORKSPACE, "bn refresh workspace too small");
  constexpr int H = kHidden;
  float* h1 = static_cast<float*>(ws);
  float* h2 = h1 + (int64_t)n * H;
  double* st = reinterpret_cast<double*>(h2 + (int64_t)n * H);  // [3 layers][mean 64 | var 64]
  // theta layout (policies/discrete.py:34-48, parameters() order)
  const float* bn0w = theta;
  const float* bn0b = bn0w + n_in;
  const float* l1w = bn0b + n_in;
  const float* l1b = l1w + H * n_in;
  const float* bn1w = l1b + H;
  const float* bn1b = bn1w + H;
  const float* l2w = bn1b + H;
  const float* l2b = l2w + H * H;
  const float* bn2w = l2b + H;
  (void)bn2w;
  const int nb = (int)(((int64_t)n * H + 255) / 256);
  hipLaunchKernelGGL(col_stats_kernel, dim3(n_in), dim3(256), 0, stream, x, n, n_in, st, st + 64);
  hipLaunchKernelGGL(bn_linear_relu_kernel, dim3(nb), dim3(256), 0, stream, x, n, n_in, st, st + 64, bn0w, bn0b, l1w,
                     l1b, H, h1);
  hipLaunchKernelGGL(col_stats_kernel, dim3(H), dim3(256), 0, stream, h1, n, H, st + 128, st + 192);
  hipLaunchKernelGGL(bn_linear_relu_kernel, dim3(nb), dim3(256), 0, stream, h1, n, H, st + 128, st + 192, bn1w, bn1b,
                     l2w, l2b, H, h2);
  hipLaunchKernelGGL(col_stats_kernel, dim3(H), dim3(256), 0, stream, h2, n, H, st + 256, st + 320);
  hipLaunchKernelGGL(bn_running_update_kernel, dim3(1), dim3(64), 0, stream, n_in, n, momentum, st, st + 64, rm, rv);
  hipLaunchKernelGGL(bn_running_update_kernel, dim3(1), dim3(64), 0, stream, H, n, momentum, st + 128, st + 192,
                     rm + n_in, rv + n_in);
  hipLaunchKernelGGL(bn_running_update_kernel, dim3(1), dim3(64), 0, stream, H, n, momentum, st + 256, st + 320,
                     rm + n_in + H, rv + n_in + H);
  return check_launch("bn refresh kernels");
}

}  // namespace fdr
