// Internal (non-ABI) host interface of the ImpalaPolicy path: the model's shape constants, the parameter layout and
// the launchers behind the C ABI (fdr_api.hip).  No kernel is declared here -- those are in fdr_impala_kernels.h --
// so a kernel-only change does not rebuild fdr_api.hip.
#pragma once
#include "fdr_pack.h"

namespace fdr {
namespace impala {

constexpr int kFeat = 2048;  // 32 x 8 x 8 (policies/impala.py:113)
constexpr int kGates = 1024;
constexpr int kCoreIn = 257; // fc output + clipped reward (policies/impala.py:116, 163-164)
// fp16 pair-form core step on MFMA (core_kernel_hpm2): fc W^T and [W_ih | W_hh]^T as v_mfma_f32_16x16x32_f16
// A-fragment images [k-step][16-column tile][64 lanes][8 halves] (lane l: W[16 nt + (l & 15)][32 ks + 8 (l >> 4) ..
// + 7]), one for theta and one per pair for sigma-eps; K of the gates (513) zero-padded to 17 k-steps.
constexpr int kFcKS = kFeat / 32, kFcNT = kHid / 16;
constexpr int kGateK = kCoreIn + kHid, kGateKS = (kGateK + 31) / 32, kGateNT = kGates / 16;
constexpr int64_t kFcImg = (int64_t)kFcKS * kFcNT * 512;      // halves
constexpr int64_t kGateImg = (int64_t)kGateKS * kGateNT * 512;
constexpr int64_t kMImg = kFcImg + kGateImg;                    // halves per image (2.2 MB)
constexpr int kReplayChunk = 64;  // entropy replay: steps per batched input-projection GEMM
constexpr int kFramePix = 3 * 64 * 64;
constexpr int kBnTab = 15 * 32;

// ---- fdr_impala.hip ----
bool make_layout(int n_act, Layout* out);

// Workspace of the pair form's operands (byte offsets; what a call does not build is empty): a zero base, theta's
// (half) pack, one sigma-eps (half) pack per pair, the pairs' table offsets, fp16: theta's + the pairs' MFMA images,
// f32: the n2 partials of those packs (not the lanes' norms)
struct PairOperands {
  int64_t zeros, thpack, epack, idxe, n2x, mimg;
};
struct Plan {  // workspace carve-up (byte offsets)
  int64_t pack, hpack, feat, h, c, rprev, ci, gx, n2, bntab, total;
  PairOperands pair;
  int nblk;    // prep blocks per lane
};
Plan plan(const Layout& L, int n_lanes, int envs, int T, bool entropy, bool fp16 = false, bool pairs = false);
bool pair_core_supported(int envs);

struct RolloutCall {
  const Context* ctx;
  const Layout* layout;
  LanesArgs lanes;
  int n_lanes, envs, T, entropy, jiggle, fp16, pairs;
  uint64_t seed, env_seed;
  const float* bn_mean;
  const float* bn_var;
  double* ret;
  double* ent;
  int32_t* steps;
  double* norm2;
  int32_t* actions;
  float* probs;
};
int launch_rollout(const RolloutCall& c, void* ws, int64_t ws_bytes, hipStream_t stream);

struct ForwardCall {
  const Layout* layout;
  int fp16;
  const float* theta;
  int n_envs;
  const float* frames;
  const float* reward;
  const float* notdone;
  float* h;
  float* c;
  float* probs;
  float* feat_out;
  const float* bn_mean;
  const float* bn_var;
};
int64_t forward_workspace_bytes(const Layout& L, int n_envs, bool fp16 = false);

// get_strategy over a probe set (policies/impala.py:24-27): Z shared frames, one LSTM sequence per lane
struct StrategiesCall {
  const Layout* layout;
  LanesArgs lanes;
  int n_lanes, n_states, fp16;
  int pairs;             // fdr_impala_desc.pairs: fp16 + n_lanes % 4 == 0 -> the pair form on MFMA
  const float* frames;   // [Z][3][64][64] f32 0..255
  const float* reward;   // [Z] or NULL
  float* h;              // [n_lanes][256] in/out initial state, or NULL (zero state)
  float* c;
  float* probs;          // [n_lanes][Z][A]
  const float* bn_mean;
  const float* bn_var;
};
int64_t strategies_workspace_bytes(const Layout& L, int n_lanes, int n_states, bool fp16, bool pairs = false);
int launch_strategies(const StrategiesCall& c, void* ws, int64_t ws_bytes, hipStream_t stream);
int launch_env_frames(uint64_t env_seed, int n_act, uint64_t env_id, int t0, int n, const int32_t* actions,
                      float* frames, float* reward, hipStream_t stream);
int set_profile(Context& ctx, int on);
int read_profile(Context& ctx, double* out3);
void destroy_profile(Profile* p);
int launch_forward(const ForwardCall& c, void* ws, int64_t ws_bytes, hipStream_t stream);

// ---- fdr_impala_vbn.hip ----
// ImpalaPolicy.compute_vbn (policies/impala.py:12-16): train-mode pass of an n-obs buffer (fdr_impala_vbn.hip)
struct VbnCall {
  const Layout* layout;
  const float* theta;
  int n;
  const float* frames;   // [n][3][64][64] f32 0..255
  const float* reward;   // [n] or NULL
  int first_done;        // the first obs' done flag: zero the carried state
  float* h;              // [256] in/out carried LSTM state, or NULL (zero, not written)
  float* c;
  float momentum;
  float* bn_mean;        // [fdr_impala_num_bn_stats] running stats, updated in place
  float* bn_var;
};
int64_t vbn_workspace_bytes(int n);
int launch_vbn(const VbnCall& c, void* ws, int64_t ws_bytes, hipStream_t stream);

}  // namespace impala
}  // namespace fdr
