// Internal (non-ABI) host interface of the AtariPolicy path behind the C ABI (fdr_api.hip): the parameter count, the
// workspace queries and the launchers of fdr_atari.hip and of the Atari half of fdr_impala_vbn.hip, one call struct
// each as on the Impala path (fdr_impala.h).  No kernel is declared here.
#pragma once
#include "fdr_internal.h"

namespace fdr {
namespace atari {

// ---- fdr_atari.hip ----
int64_t num_params(int n_act);  // -1: n_act outside 1..32

struct RolloutCall {
  int n_act, envs, T;
  uint64_t env_seed;
  LanesArgs lanes;
  int n_lanes;
  uint64_t seed;
  int jiggle;
  const float* bn_mean;  // running stats [16 | 32 | 256], or NULL (0 / 1)
  const float* bn_var;
  double* ret;
  double* ent;
  int32_t* steps;
  double* norm2;
  int32_t* actions;
  float* probs;
};
int64_t workspace_bytes(int n_act, int n_lanes, int envs);
int launch_rollout(const RolloutCall& c, void* ws, int64_t ws_bytes, hipStream_t stream);

struct ForwardCall {
  int n_act;
  const float* theta;
  int n;
  const float* frames;   // [n][4][84][84] f32 0..255
  const float* bn_mean;
  const float* bn_var;
  float* probs;          // [n][A]
  float* feat;           // [n][2592], or NULL
};
int64_t forward_workspace_bytes(int n_act, int n);
int launch_forward(const ForwardCall& c, void* ws, int64_t ws_bytes, hipStream_t stream);

// get_strategy of every lane's theta' over Z shared probe frames (policies/atari.py:30-31)
struct StrategiesCall {
  int n_act;
  LanesArgs lanes;
  int n_lanes, n_states;
  const float* frames;   // [Z][4][84][84] f32 0..255
  const float* bn_mean;
  const float* bn_var;
  float* probs;          // [n_lanes][Z][A]
};
int64_t strategies_workspace_bytes(int n_act, int n_lanes, int Z);
int launch_strategies(const StrategiesCall& c, void* ws, int64_t ws_bytes, hipStream_t stream);

int launch_env_frames(uint64_t env_seed, uint64_t env_id, int t0, int n, float* frames, hipStream_t stream);

// ---- fdr_impala_vbn.hip ----
// AtariPolicy.compute_vbn: train-mode pass of an n-frame buffer
struct VbnCall {
  const float* theta;
  int n;
  const float* frames;   // [n][4][84][84] f32 0..255
  float momentum;
  float* bn_mean;        // [16 | 32 | 256] running stats, updated in place
  float* bn_var;
};
int64_t vbn_workspace_bytes(int n);
int launch_vbn(const VbnCall& c, void* ws, int64_t ws_bytes, hipStream_t stream);

}  // namespace atari
}  // namespace fdr
