// Internal (non-ABI) host interface of the learner-side units behind the C ABI (fdr_api.hip): the launchers and
// workspace queries of fdr_learner.hip, fdr_learner_fused.hip, fdr_top_dirs.hip, fdr_learner_runs.hip, fdr_dsgd.hip, fdr_optim.hip, fdr_novelty.hip and
// fdr_mlp_vbn.hip, and the two structs that cross to their kernels by value (LambdaRow, FdArgs).
#pragma once
#include "fdr_internal.h"

namespace fdr {

// ---- fdr_learner.hip ----
int launch_perturb(const float* theta, int64_t P, const float* table, int64_t table_size,
                   const int64_t* idx, const int8_t* sign, int n, float sigma, float* out,
                   hipStream_t stream);
int launch_fd_weights(const double* r_all, int n_all, double pr, int lo, int n_local,
                      const int8_t* sign, const double* n2, int lpd, float sigma, double* coef,
                      hipStream_t stream);
// The mixed objective's channels (reward, novelty, entropy), by value to kernels: w_i = sum over the channels with
// a != 0, in this order, of a_c z_c[i], z_c the z-score of v_c - p_c over all lanes (input unchanged when its std is
// 0).  A channel with a == 0 is inactive: the C boundary points its v at an active channel's array (so every load
// stays branch-free and in bounds) and the kernels add no term for it.
struct MixChannels {
  const double* v[3];  // [n_all] each
  double p[3];         // the policy's own value
  double a[3];         // 1 - omega, omega, ent_coef
};
int launch_fd_weights_mix(const MixChannels& mx, int n_all, int lo, int n_local, const int8_t* sign, const double* n2,
                          int lpd, float sigma, double* coef, hipStream_t stream);

// The tiling of a noise-weighted gradient: 256-column blocks x row chunks, one f64 partial slab per chunk.  The
// staged pair (grad_plan) and the fused kernel (fused_plan) choose rows_per_chunk by formulas of their own; each
// fixes its summation order and with it the result bits.
struct GradPlan {
  int col_blocks, rows_per_chunk, n_chunks;
};
int64_t grad_workspace_bytes(int n_dirs, int64_t P);
int launch_fd_grad(const float* table, int64_t table_size, const int64_t* idx, const double* coef,
                   int n_dirs, int64_t P, double* g, void* ws, int64_t ws_bytes, hipStream_t stream);

// Delayed-return perturbation rows (fdr_fd_lambda_norms / fdr_fd_grad_lambda), by value to kernels.
struct LambdaRow {
  const float* table;
  int64_t max_idx;
  const int64_t* idx;
  const int8_t* sign;
  const int32_t* slot;
  const float* drift;
  int n_slots;
  int64_t P;
  float sigma;

  // pointer to eps_i (row 0 if the offset is out of range: the caller poisons that row with NaN)
  __device__ __forceinline__ const float* eps(int i, bool& bad) const {
    const int64_t off = idx[i];
    bad = off < 0 || off > max_idx;
    return table + (bad ? 0 : off);
  }
  __device__ __forceinline__ const float* dr(int i) const {
    const int s = slot ? slot[i] : -1;
    return (s >= 0 && s < n_slots) ? drift + (int64_t)s * P : nullptr;
  }
  __device__ __forceinline__ float value(const float* e, const float* d, int sg, int64_t p) const {
#pragma clang fp contract(off)
    float v = sigma * e[p];
    v = sg < 0 ? -v : v;
    return d ? v + d[p] : v;
  }
};
int launch_lambda_norms(const LambdaRow& R, int n, double* n2, hipStream_t stream);
int launch_lambda_grad(const LambdaRow& R, const double* coef, int n, double* g, void* ws, int64_t ws_bytes,
                       hipStream_t stream);

// ---- fdr_learner_fused.hip ----
// fd_grad_fused_kernel's argument.  The caller fills the first block; launch_fd_grad_fused adds the plan and the
// workspace regions.
struct FdArgs {
  const float* table;
  int64_t max_idx;       // table_size - P: largest legal offset
  const int64_t* idx;    // per LOCAL lane [n_dirs * lpd]; direction d's row starts at idx[d * lpd]
  int n_dirs;
  int64_t P;
  const double* r_all;   // [n_all]; MOMENTS: the local lanes' rewards only
  int n_all;             // lanes over all ranks
  double pr;
  int lo;                // this rank's first global lane
  const int8_t* sign;    // [n_dirs * lpd] (local lanes)
  const double* n2;      // [n_dirs * lpd]
  const double* w;       // centred-rank weights of the local lanes
  int lpd;
  float sigma;
  int rows_per_chunk, n_chunks, col_blocks;
  double* partial;       // [n_chunks][P] (x2 in MOMENTS mode)
  unsigned* cnt;         // [col_blocks] chunk tickets, [col_blocks] the DSGD ticket
  double* out;           // g [P]; MOMENTS: [A | B | n_local | r' slots [n_all]]
  double* gsq;           // [col_blocks] sum fl32(-g)^2 per column block (fdr_fd_step), or NULL
};
// fd_grad_fused_mix_kernel's argument: FdArgs as it is (the existing instances' kernarg layout does not move) and
// the channels; fd.r_all / fd.pr are not read, the reward channel is mix.v[0] / mix.p[0].
struct FdMixArgs {
  FdArgs fd;
  MixChannels mix;
};
// A torch.optim step's hyperparameters as torch holds them (Python floats); fdr_optim.hip forms the kernel's f32
// scalars from them and the step count.
struct OptHyper {
  double lr, beta1, beta2, eps, weight_decay, momentum, dampening;
  int nesterov;
};
struct FusedCall {
  FdArgs fd;             // table .. sigma and out
  int mode;              // FDR_WEIGHT_*
  MixChannels mix;       // FDR_WEIGHT_ZSCORE_MIX only
  int top_dirs;          // FDR_WEIGHT_TOP_DIRS only: b, the directions kept (1 <= b <= n_all / lpd)
  // fdr_fd_step: DSGD in the same call (theta NULL: the gradient only)
  float* theta;
  double lr, lr_scale;
  float* hist;           // theta_new also goes here (the learner's policy_history), or NULL
  double* dsgd_out;      // [||d theta||, ||fl32(-g)||]
  // fdr_fd_step_opt: opt_kind != 0 applies that optimizer (FDR_OPT_*) in place of DSGD; lr / lr_scale are not read
  int opt_kind;
  OptHyper opt;
  int64_t opt_step;      // the step count including this step (torch's state["step"] after it)
  float *state0, *state1;
};
int64_t fused_workspace_bytes(int n_dirs, int n_local, int64_t P, int mode);
int64_t fused_counter_bytes(int n_dirs, int64_t P);
int launch_fd_grad_fused(const FusedCall& c, void* ws, int64_t ws_bytes, hipStream_t stream);
int launch_rank_weights(const double* r_all, int n_all, int lo, int n_local, double* w, hipStream_t stream);
// FDR_WEIGHT_TOP_DIRS: fused_workspace_bytes(.., FDR_WEIGHT_CENTERED_RANK) and, behind it, the lane mask over all ranks
int64_t fused_top_workspace_bytes(int n_dirs, int n_local, int64_t P, int n_all);

// ---- fdr_top_dirs.hip ----
// top-b direction selection: top_dirs_select_kernel (lane mask over ALL n_all lanes -> ws) + top_dirs_weights_kernel
// (w [n_local], selected int8 [n_local / lpd] or NULL).  ws: top_dirs_workspace_bytes(n_all).  The caller has
// validated n_all % lpd == 0, 1 <= top_dirs <= n_all / lpd, lo and n_local multiples of lpd inside [0, n_all].
int64_t top_dirs_workspace_bytes(int n_all);
int launch_top_dir_weights(const double* r_all, int n_all, double pr, int lpd, int top_dirs, int lo, int n_local,
                           double* w, int8_t* selected, void* ws, int64_t ws_bytes, hipStream_t stream);

// ---- fdr_learner_runs.hip ----
// fdr_fd_step_runs: R runs, one workgroup each (fd_step_runs_kernel).  Per-lane arrays hold run_stride entries per run,
// the first n_dirs * lpd of them the run's training lanes.  launch_fd_step_runs refuses P > kRunsMaxP and
// n_dirs * lpd > kRunsMaxTrain (FDR_ERR_UNSUPPORTED, the limit in the message) before any launch.
constexpr int kRunsMaxP = 32;         // parameters per run (f64 registers per thread); the physics shapes reach 18
constexpr int kRunsMaxTrain = 4096;   // training lanes per run (the returns in LDS)
struct FdRunsArgs {
  const float* table;
  int64_t max_idx;               // table_size - P: largest legal offset
  const int64_t* idx;            // per lane; direction d of run r: idx[r * run_stride + d * lpd]
  const int8_t* sign;            // per lane
  const double* norm2;           // per lane
  const double* rewards;         // per lane
  int64_t run_stride;
  const double* policy_reward;   // [R], or NULL: 0
  const float* sigma_runs;       // [R]
  const int32_t* top_dirs;       // [R], or NULL: the z-score over all lanes
  float* theta_runs;             // [R, P], in/out
  const double* lr;              // [R]
  double lr_scale;
  double* g_out;                 // [R, P], or NULL
  double* out;                   // [R, 2]: ||d theta||, ||fl32(-g)||
  int n_dirs, lpd, P;
};
int launch_fd_step_runs(const FdRunsArgs& a, int n_runs, hipStream_t stream);

// ---- fdr_dsgd.hip ----
int64_t dsgd_workspace_bytes(int64_t P);
int launch_dsgd_ex(float* theta, const double* src, int mom, int64_t P, double lr, double lr_scale, double* g_out,
                   double* out, void* ws, int64_t ws_bytes, hipStream_t stream);
// moment_stats_kernel + moments_to_grad_kernel: stats [2] <- mean, sd of the summed r' slots, g_out <- (A - m B) / sd
int launch_moments_to_grad(const double* src, int64_t P, double* stats, double* g_out, hipStream_t stream);

// ---- fdr_optim.hip ----
constexpr int64_t kOptCounterBytes = 256;  // the ticket counter at the head of the standalone step's workspace
int64_t opt_workspace_bytes(int64_t P);
// FDR_ERR_INVALID naming the offending field, or FDR_OK; no device work
int opt_validate(int kind, const OptHyper& h, int64_t step, const float* state0, const float* state1);
// opt_apply_cb_kernel<kind> alone: gpart / upart [col_blocks] each, cnt one zeroed counter (left zero)
int launch_opt_apply(int kind, float* theta, const double* g, int64_t P, const OptHyper& h, int64_t step,
                     float* state0, float* state1, float* hist, double* gpart, double* upart, unsigned* cnt,
                     double* out, hipStream_t stream);
// from g or (src_is_moments) the summed moments, any P
int launch_opt_step(int kind, float* theta, const double* src, int src_is_moments, int64_t P, const OptHyper& h,
                    int64_t step, float* state0, float* state1, double* g_out, float* hist, double* out, void* ws,
                    int64_t ws_bytes, hipStream_t stream);

// ---- fdr_novelty.hip ----
int launch_strategy_dist(const float* S, int n, const float* B, int H, int Z, int D, int kind, double* dists,
                         double* min_d, int32_t* arg, hipStream_t stream);

// ---- fdr_mlp_vbn.hip ----
int64_t bn_refresh_workspace_bytes(int n);
int launch_bn_refresh(int n_in, const float* theta, const float* x, int n, float momentum, float* rm, float* rv,
                      void* ws, int64_t ws_bytes, hipStream_t stream);

}  // namespace fdr
