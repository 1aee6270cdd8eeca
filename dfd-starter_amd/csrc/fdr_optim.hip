// fdr_optim.hip -- the torch.optim steps the learner honours besides DSGD: Adam, AdamW and SGD (momentum, dampening,
// nesterov, weight decay) applied to theta on the device from the f64 gradient g, or from the summed moments form.
//
//   opt_apply_cb_kernel<KIND>   dsgd_apply_cb_kernel's map: one 256-column block per workgroup.  Per element
//                               grad = fl32(-g) (set_grad_from_flat, policy.py:68), the optimizer's single-tensor
//                               formula of torch/optim/{adam,adamw,sgd}.py (non-capturable, maximize = False) in f32
//                               with contraction off, theta / state / theta_hist written, and the block's
//                               sum (theta_old - theta_new)^2 and sum grad^2 handed off; the last workgroup (ticket)
//                               forms out = [||d theta||, ||fl32(-g)||] in column-block order and zeroes the counter.
// None of these optimizers needs a global norm before the update, so there is no first pass over g.  The scalars that
// torch forms from Python floats (step_size, bias_correction2_sqrt, 1 - lr * wd, ..) are formed here on the host in
// double from `step` and the hyperparameters, and reach the kernel rounded to f32 once, as a Python float reaches an
// f32 tensor operation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "fdr_learner.h"
#include "fdr_reduce.h"

namespace fdr {

// the kernel's scalars, by value
struct OptScalars {
  float lr;         // SGD: alpha of param.add_(grad, alpha=-lr)
  float w1;         // 1 - beta1: exp_avg.lerp_(grad, 1 - beta1)
  float b2, c2;     // beta2, 1 - beta2
  float eps;
  float step_size;  // lr / (1 - beta1^t)
  float bc2_sqrt;   // sqrt(1 - beta2^t)
  float wd;         // weight_decay (L2 term)
  float decay;      // 1 - lr * weight_decay (AdamW)
  float momentum;
  float d1;         // 1 - dampening
  int has_wd, nesterov, first;  // first: step == 1, the momentum buffer is the gradient itself
};

template <int KIND>
__global__ __launch_bounds__(256) void opt_apply_cb_kernel(float* __restrict__ theta, const double* __restrict__ g,
                                                           int64_t P, OptScalars h, float* __restrict__ s0,
                                                           float* __restrict__ s1, float* __restrict__ hist,
                                                           double* __restrict__ gpart, double* __restrict__ upart,
                                                           int col_blocks, unsigned* __restrict__ cnt,
                                                           double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  __shared__ double gs[256], gq[256];
  __shared__ int s_flag;
  const int tid = threadIdx.x, cb = blockIdx.x;
  const int64_t p = (int64_t)cb * 256 + tid;
  const bool ok = p < P;
  const float g32 = ok ? (float)(-g[p]) : 0.f;  // set_grad_from_flat casts to f32 (policy.py:68)
  const float old = ok ? theta[p] : 0.f;
  float grad = g32, nw = old;
  if constexpr (KIND == FDR_OPT_ADAM || KIND == FDR_OPT_ADAMW) {
    float m = ok ? s0[p] : 0.f, v = ok ? s1[p] : 0.f;
    if constexpr (KIND == FDR_OPT_ADAMW) {
      if (h.has_wd) nw = old * h.decay;  // param.mul_(1 - lr * weight_decay)
    } else {
      if (h.has_wd) grad = grad + h.wd * old;  // grad.add(param, alpha=weight_decay)
    }
    // exp_avg.lerp_(grad, w): torch's lerp takes the form that is exact at its nearer end
    const float diff = grad - m;
    m = h.w1 < 0.5f ? m + h.w1 * diff : grad - diff * (1.f - h.w1);
    v = v * h.b2;  // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    v = v + h.c2 * grad * grad;
    const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
    nw = nw - h.step_size * (m / denom);  // param.addcdiv_(exp_avg, denom, value=-step_size)
    if (ok) {
      s0[p] = m;
      s1[p] = v;
    }
  } else {
    if (h.has_wd) grad = grad + h.wd * old;
    if (h.momentum != 0.f) {  // uniform: momentum == 0 reads and writes no state
      float buf = grad;       // first step: buf = grad.clone()
      if (!h.first) {
        buf = ok ? s0[p] : 0.f;
        buf = buf * h.momentum + h.d1 * grad;  // buf.mul_(momentum).add_(grad, alpha=1 - dampening)
      }
      if (ok) s0[p] = buf;
      grad = h.nesterov ? grad + h.momentum * buf : buf;
    }
    nw = old - h.lr * grad;  // param.add_(grad, alpha=-lr)
  }
  if (ok) {
    theta[p] = nw;
    if (hist) hist[p] = nw;
  }
  const float dd = old - nw;
  const double u = block_sum_256(ok ? (double)dd * (double)dd : 0.0, red);
  const double q = block_sum_256((double)g32 * (double)g32, red);
  if (tid == 0) {
    store_wt(upart + cb, u);
    store_wt(gpart + cb, q);
  }
  publish_and_ticket(cnt, (unsigned)col_blocks, &s_flag);
  if (s_flag) {
    // both sums in column-block order, their two dependent add chains side by side
    double t = 0.0, n = 0.0;
    for (int k0 = 0; k0 < col_blocks; k0 += 256) {
      __syncthreads();
      if (k0 + tid < col_blocks) {
        gs[tid] = upart[k0 + tid];
        gq[tid] = gpart[k0 + tid];
      }
      __syncthreads();
      const int kn = min(256, col_blocks - k0);
#pragma unroll 8
      for (int k = 0; k < kn; ++k) {
        t += gs[k];
        n += gq[k];
      }
    }
    if (tid == 0) {
      out[0] = sqrt(t);
      out[1] = sqrt(n);
      __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------
static bool finite_nonneg(double x) { return std::isfinite(x) && x >= 0.0; }

int opt_validate(int kind, const OptHyper& h, int64_t step, const float* state0, const float* state1) {
  if (kind != FDR_OPT_ADAM && kind != FDR_OPT_ADAMW && kind != FDR_OPT_SGD)
    return set_error(FDR_ERR_INVALID, "kind: not one of FDR_OPT_ADAM / FDR_OPT_ADAMW / FDR_OPT_SGD");
  if (step < 1) return set_error(FDR_ERR_INVALID, "step: must be >= 1 (the count including this step)");
  if (!finite_nonneg(h.lr)) return set_error(FDR_ERR_INVALID, "lr: must be finite and >= 0");
  if (!finite_nonneg(h.weight_decay)) return set_error(FDR_ERR_INVALID, "weight_decay: must be finite and >= 0");
  if (kind == FDR_OPT_SGD) {
    if (!finite_nonneg(h.momentum)) return set_error(FDR_ERR_INVALID, "momentum: must be finite and >= 0");
    if (!std::isfinite(h.dampening)) return set_error(FDR_ERR_INVALID, "dampening: must be finite");
    if (h.nesterov && (h.momentum == 0.0 || h.dampening != 0.0))
      return set_error(FDR_ERR_INVALID, "nesterov: needs momentum > 0 and dampening == 0");
    if (h.momentum != 0.0 && !state0) return set_error(FDR_ERR_INVALID, "state0: momentum_buffer is NULL");
    return FDR_OK;
  }
  if (!finite_nonneg(h.eps)) return set_error(FDR_ERR_INVALID, "eps: must be finite and >= 0");
  if (!(h.beta1 >= 0.0 && h.beta1 < 1.0)) return set_error(FDR_ERR_INVALID, "beta1: must be in [0, 1)");
  if (!(h.beta2 >= 0.0 && h.beta2 < 1.0)) return set_error(FDR_ERR_INVALID, "beta2: must be in [0, 1)");
  if (!state0) return set_error(FDR_ERR_INVALID, "state0: exp_avg is NULL");
  if (!state1) return set_error(FDR_ERR_INVALID, "state1: exp_avg_sq is NULL");
  return FDR_OK;
}

// torch's scalars (adam.py _single_tensor_adam, sgd.py _single_tensor_sgd) in double, rounded to f32 once
static OptScalars opt_scalars(int kind, const OptHyper& h, int64_t step) {
  OptScalars s{};
  s.lr = (float)h.lr;
  s.wd = (float)h.weight_decay;
  s.has_wd = h.weight_decay != 0.0;
  s.first = step == 1;
  if (kind == FDR_OPT_SGD) {
    s.momentum = (float)h.momentum;
    s.d1 = (float)(1.0 - h.dampening);
    s.nesterov = h.nesterov;
    return s;
  }
  const double bc1 = 1.0 - std::pow(h.beta1, (double)step);
  const double bc2 = 1.0 - std::pow(h.beta2, (double)step);
  s.w1 = (float)(1.0 - h.beta1);
  s.b2 = (float)h.beta2;
  s.c2 = (float)(1.0 - h.beta2);
  s.eps = (float)h.eps;
  s.step_size = (float)(h.lr / bc1);
  s.bc2_sqrt = (float)std::sqrt(bc2);
  s.decay = (float)(1.0 - h.lr * h.weight_decay);
  return s;
}

int launch_opt_apply(int kind, float* theta, const double* g, int64_t P, const OptHyper& h, int64_t step,
                     float* state0, float* state1, float* hist, double* gpart, double* upart, unsigned* cnt,
                     double* out, hipStream_t stream) {
  const int rc = opt_validate(kind, h, step, state0, state1);
  if (rc) return rc;
  const int64_t cb64 = (P + 255) / 256;
  if (cb64 > 0x7fffffff) return set_error(FDR_ERR_UNSUPPORTED, "n_params: more than 2^31 - 1 column blocks");
  const int col_blocks = (int)cb64;
  const OptScalars s = opt_scalars(kind, h, step);
  const dim3 grid(col_blocks), block(256);
  switch (kind) {
    case FDR_OPT_ADAM:
      hipLaunchKernelGGL(opt_apply_cb_kernel<FDR_OPT_ADAM>, grid, block, 0, stream, theta, g, P, s, state0, state1, hist,
                         gpart, upart, col_blocks, cnt, out);
      break;
    case FDR_OPT_ADAMW:
      hipLaunchKernelGGL(opt_apply_cb_kernel<FDR_OPT_ADAMW>, grid, block, 0, stream, theta, g, P, s, state0, state1,
                         hist, gpart, upart, col_blocks, cnt, out);
      break;
    default:
      hipLaunchKernelGGL(opt_apply_cb_kernel<FDR_OPT_SGD>, grid, block, 0, stream, theta, g, P, s, state0, state1, hist,
                         gpart, upart, col_blocks, cnt, out);
      break;
  }
  return check_launch("opt_apply_cb_kernel");
}

// workspace of the standalone step: [ticket counter, 256 B][sum grad^2 per column block][sum (d theta)^2 per column
// block][mean, sd of the moments form]
static int64_t pad256(int64_t b) { return (b + 255) / 256 * 256; }
int64_t opt_workspace_bytes(int64_t P) {
  if (P <= 0) return -1;
  return kOptCounterBytes + 2 * pad256((P + 255) / 256 * 8) + 256;
}

int launch_opt_step(int kind, float* theta, const double* src, int src_is_moments, int64_t P, const OptHyper& h,
                    int64_t step, float* state0, float* state1, double* g_out, float* hist, double* out, void* ws,
                    int64_t ws_bytes, hipStream_t stream) {
  int rc = opt_validate(kind, h, step, state0, state1);
  if (rc) return rc;
  if (src_is_moments && !g_out) return set_error(FDR_ERR_INVALID, "g_out: the moments form writes g there");
  if (!ws || ws_bytes < opt_workspace_bytes(P)) return set_error(FDR_ERR_WORKSPACE, "opt workspace too small");
  char* w = static_cast<char*>(ws);
  const int64_t cb_b = pad256((P + 255) / 256 * 8);
  unsigned* cnt = reinterpret_cast<unsigned*>(w);
  double* gpart = reinterpret_cast<double*>(w + kOptCounterBytes);
  double* upart = reinterpret_cast<double*>(w + kOptCounterBytes + cb_b);
  double* stats = reinterpret_cast<double*>(w + kOptCounterBytes + 2 * cb_b);
  const double* g = src;
  if (src_is_moments) {  // the statistics once, then g = (A - m B) / sd: fdr_dsgd.hip's kernels, at every P
    rc = launch_moments_to_grad(src, P, stats, g_out, stream);
    if (rc) return rc;
    g = g_out;
  }
  return launch_opt_apply(kind, theta, g, P, h, step, state0, state1, hist, gpart, upart, cnt, out, stream);
}

}  // namespace fdr
