// Internal (non-ABI) declarations shared by the fdr translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <array>

#include "fdr_common.h"

namespace fdr {

int set_error(int code, const char* msg);
int check_launch(const char* what);

// Per-device engine state behind an fdr_ctx (include/fdr.h): the settings that were process-wide
// globals before (rollout kernel selection, Impala phase profiling, replay GEMM switch, debug clocks).
// A NULL ctx at the ABI means default_context(), the process-wide one (FDR_ROLLOUT read at first use).
namespace impala {
struct Profile;
}
struct Context {
  int device = -1;      // -1: any (the default context follows the current device)
  int cus = 0;          // compute units of `device` (0: query the current device)
  int rollout_impl = 2; // FDR_ROLLOUT_AUTO
  int replay_gemm = 1;
  uint64_t* debug_clock = nullptr;
  impala::Profile* prof = nullptr;  // owned, created on first enable
};
Context& default_context();
int context_cus(const Context& c);
// The context of a call for an entry point outside fdr_api.hip: ctx's own, or the default one for NULL; FDR_ERR_INVALID
// when ctx belongs to another device than the current one (what FDR_CTX does inside fdr_api.hip).
int resolve_context(::fdr_ctx* ctx, Context** out);

struct PolicyKey {
  int n_in, n_act;
  bool discrete;
  int64_t n_params;
  bool linear = false;  // FDR_POLICY_LINEAR: W [n_act, n_in] alone (discrete is then unused: the env decides)
};

// Device-side view of fdr_lanes_desc (passed by value as a kernel argument).
struct LanesArgs {
  const float* base;
  int64_t base_stride;
  const float* table;
  int64_t max_idx;  // table_size - n_params: largest legal offset
  const int64_t* idx;
  const int8_t* sign;
  float sigma;
  const int8_t* deterministic;
  int64_t lane_offset;

  // A lane whose table offset is out of range is never dereferenced: it runs unperturbed and
  // reports norm2 = NaN, which poisons the FD step visibly instead of faulting the GPU.
  __device__ __forceinline__ ParamSrc src(int lane) const {
    ParamSrc s;
    s.base = base + (int64_t)lane * base_stride;
    s.ss = sigma;
    s.n2 = 0.0;
    s.sgn = 0;
    s.eps = s.base;  // unperturbed: a readable address whose value ParamSrc discards
    if (table != nullptr) {
      const int64_t off = idx[lane];
      const int sg = sign ? (int)sign[lane] : 1;
      if (off < 0 || off > max_idx) {
        s.n2 = __builtin_nan("");
      } else if (sg != 0) {
        s.sgn = sg > 0 ? 1 : -1;
        s.ss = sg > 0 ? sigma : -sigma;  // the sign rides on sigma (ParamSrc)
        s.eps = table + off;
      }
    }
    return s;
  }
};

struct RolloutArgs {
  LanesArgs lanes;
  int n_lanes;
  int lane_base;  // first lane of this launch (rollout_pair_kernel launches lanes in rounds, launch_pair)
  int T;
  uint64_t key;
  int jiggle;
  const float* bn_mean;
  const float* bn_var;
  const float* obs_mean;
  const float* obs_std;
  // synthetic env
  const float* M;
  const float* K;
  const float* s0;
  float done_thr;  // > 0: terminating env, done when |s'[done_dim]| > done_thr (fdr_env_desc.done_threshold)
  int done_dim;
  // trap env
  const uint8_t* walkable;
  int map_w, map_h, trap_start_col, trap_start_row;
  // outputs
  double* ret;
  double* ent;
  int32_t* steps;
  double* norm2;
  float* states;  // NULL, or [n_lanes, T, n_in] visited raw observations (fdr_rollout_states)
  // NULL, or per-lane Welford obs statistics (fdr_rollout_obs_stats)
  float* os_mean;
  float* os_m2;
  int32_t* os_count;
  float os_chance;
  // NULL, or [n_lanes, T, k] host-injected draws replacing the counter stream (fdr_rollout_extras.u_inject)
  const float* u_inject;
};
// fdr_rollout_episodes' kernel argument: the rollout's own (synthetic / trap members, states and u_inject unused) and
// the episode loop's.  A struct of its own: a member added to RolloutArgs moves the hidden kernel arguments behind it,
// which changes an s_load offset in every kernel that takes RolloutArgs (tools/isa_diff.py).
struct EpisodesArgs {
  RolloutArgs r;
  int n_episodes;              // K: episodes per lane
  const int64_t* episode_ids;  // NULL, or [n_lanes, K] stream ids
  double* ret_sq;              // NULL, or [n_lanes] sum of squared episode returns
};

int launch_policy_forward(const Context& ctx, const PolicyKey& k, const LanesArgs& lanes, int n_lanes,
                          const float* bn_mean, const float* bn_var, const float* x, float* out0,
                          float* out1, hipStream_t stream);
int launch_rollout(const Context& ctx, const PolicyKey& k, int env_kind, const RolloutArgs& args, hipStream_t stream);
// The rollout kernel families launch_rollout chooses from, one translation unit and one launcher each
// (fdr_rollout_lane / _wide / _env / _pair.hip); each matches the policy shape and the feature set itself.
// synthetic env, one lane per wave: the 128-VGPR kernel / the 256-VGPR one
int launch_rollout_lane(const PolicyKey& k, const RolloutArgs& args, hipStream_t stream);
int launch_rollout_wide(const PolicyKey& k, const RolloutArgs& args, hipStream_t stream);
// The classic-control physics envs, the one table of them: each kind with its observation / action sizes, the one
// policy it runs under, the refusal of any other and its kernels' display names.  The kernels' shape checks, the
// shapes compiled for them (fdr_mlp.h: PhysicsShapes), the runtime table and both launchers derive from it.
template <int KIND>
struct PhysicsSpec;
#define FDR_PHYSICS_SPEC(KIND, NIN_, NA_, DISC_, TAG, POLICY_MSG)                                                  \
  template <>                                                                                                      \
  struct PhysicsSpec<KIND> {                                                                                       \
    static constexpr int ENV = KIND, NIN = NIN_, NA = NA_;                                                         \
    static constexpr bool DISC = DISC_;                                                                            \
    static constexpr const char *policy_msg = POLICY_MSG, *rollout_name = "rollout_kernel<" TAG ">",               \
                                *episodes_name = "rollout_episodes_kernel<" TAG ">";                               \
    template <int I, int A, bool D>                                                                                \
    static constexpr bool is_shape() { return I == NIN_ && A == NA_ && D == DISC_; }                               \
  }
FDR_PHYSICS_SPEC(FDR_ENV_CARTPOLE, 4, 2, true, "cartpole", "CartPole needs a DiscretePolicy(4, 2)");
FDR_PHYSICS_SPEC(FDR_ENV_PENDULUM, 3, 1, false, "pendulum", "Pendulum needs a MujocoPolicy(3, 1)");
FDR_PHYSICS_SPEC(FDR_ENV_ACROBOT, 6, 3, true, "acrobot", "Acrobot needs a DiscretePolicy(6, 3)");
FDR_PHYSICS_SPEC(FDR_ENV_MOUNTAINCAR, 2, 3, true, "mountaincar", "MountainCar needs a DiscretePolicy(2, 3)");
FDR_PHYSICS_SPEC(FDR_ENV_MOUNTAINCAR_CONT, 2, 1, false, "mountaincar_cont",
                 "MountainCarContinuous needs a MujocoPolicy(2, 1)");
#undef FDR_PHYSICS_SPEC
template <int... KIND>
struct PhysicsKinds {};
using PhysicsEnvKinds = PhysicsKinds<FDR_ENV_CARTPOLE, FDR_ENV_PENDULUM, FDR_ENV_ACROBOT, FDR_ENV_MOUNTAINCAR,
                                     FDR_ENV_MOUNTAINCAR_CONT>;
// f(PhysicsSpec<kind>{}) for the physics env `kind`; false (f not called): not a physics env
template <class F, int... KIND>
bool with_physics_env(int kind, F&& f, PhysicsKinds<KIND...>) {
  return ((kind == KIND && (f(PhysicsSpec<KIND>{}), true)) || ...);
}
template <class F>
bool with_physics_env(int kind, F&& f) {
  return with_physics_env(kind, f, PhysicsEnvKinds{});
}
// The spec as runtime values: fdr_rollout_ex validates the descriptor against it, the launchers the policy.
struct PhysicsEnv {
  int kind, obs, act;
  bool discrete;
  const char* policy_msg;
};
template <int... KIND>
constexpr std::array<PhysicsEnv, sizeof...(KIND)> physics_table(PhysicsKinds<KIND...>) {
  return {{{KIND, PhysicsSpec<KIND>::NIN, PhysicsSpec<KIND>::NA, PhysicsSpec<KIND>::DISC,
            PhysicsSpec<KIND>::policy_msg}...}};
}
inline constexpr auto kPhysicsEnvs = physics_table(PhysicsEnvKinds{});
inline const PhysicsEnv* physics_env(int kind) {  // NULL: not a physics env
  for (const PhysicsEnv& e : kPhysicsEnvs)
    if (e.kind == kind) return &e;
  return nullptr;
}
inline bool physics_policy_ok(const PhysicsEnv& e, const PolicyKey& k) {
  return k.discrete == e.discrete && k.n_in == e.obs && k.n_act == e.act;
}
// trap gridworld and the physics envs
int launch_rollout_env(const PolicyKey& k, int env_kind, const RolloutArgs& args, hipStream_t stream);
// the physics envs, args.n_episodes episodes per lane in one launch (fdr_rollout_episodes.hip); any other env kind or
// a policy that is not the env's own: FDR_ERR_UNSUPPORTED, nothing launched
int launch_rollout_episodes(const PolicyKey& k, int env_kind, const EpisodesArgs& args, hipStream_t stream);
// two lanes per wave; round_lanes: lanes of one resident round (more go out as consecutive launches)
int launch_rollout_pair(const PolicyKey& k, const RolloutArgs& args, int round_lanes, hipStream_t stream);
// fdr_diag_theta_prime: what MlpLane::load / MlpPair::load / DynLane::load read through a RecordSrc (out / reads /
// counted [n_lanes, P])
int launch_theta_prime(const PolicyKey& k, const LanesArgs& lanes, int n_lanes, int loader, const float* bn_mean,
                       const float* bn_var, float* out, int32_t* reads, int32_t* counted, double* n2,
                       hipStream_t stream);
// The runtime-shaped family (fdr_rollout_dyn.hip): n_in / n_act are kernel arguments.  It runs every shape within
// dyn_shape_check's limits that is no compiled instance, and every synthetic-env rollout and policy forward of a
// FDR_ROLLOUT_GENERIC context.  dyn_shape_check: FDR_OK, or FDR_ERR_UNSUPPORTED with the limit in the message.
int dyn_shape_check(const PolicyKey& k);
int launch_rollout_dyn(const PolicyKey& k, const RolloutArgs& args, hipStream_t stream);
int launch_policy_forward_dyn(const PolicyKey& k, const LanesArgs& lanes, int n_lanes, const float* bn_mean,
                              const float* bn_var, const float* x, float* out0, float* out1, hipStream_t stream);
int launch_theta_prime_dyn(const PolicyKey& k, const LanesArgs& lanes, int n_lanes, const float* bn_mean,
                           const float* bn_var, float* out, int32_t* reads, int32_t* counted, double* n2,
                           hipStream_t stream);

// FDR_POLICY_LINEAR (fdr_rollout_linear.hip): one lane per thread.  The rollout serves fdr_rollout* (n_episodes 1) and
// fdr_rollout_episodes alike, on the physics envs at their own shapes; anything else: FDR_ERR_UNSUPPORTED, nothing
// launched.  The forward takes any shape within linear_shape_check's limits.
int linear_shape_check(const PolicyKey& k);
int launch_rollout_linear(const PolicyKey& k, int env_kind, const EpisodesArgs& args, hipStream_t stream);
int launch_policy_forward_linear(const PolicyKey& k, const LanesArgs& lanes, int n_lanes, const float* x, float* out,
                                 hipStream_t stream);

// fdr_rollout_runs' kernel argument (fdr_rollout_linear.hip, rollout_runs_kernel): R runs x lanes_per_run lanes in one
// launch, global lane g = r * lanes_per_run + l.  e holds what every lane shares (table, idx, sign, the outputs, T, key,
// K, episode_ids; e.r.n_lanes = R * lanes_per_run); e.r.lanes.base / sigma / lane_offset and e.r.obs_mean / obs_std are
// not read: run r's come from the arrays here.
struct RunsArgs {
  EpisodesArgs e;
  const float* theta_runs;         // [R, P]
  const float* sigma_runs;         // [R]
  const float* obs_mean_runs;      // [R, n_in], or NULL
  const float* obs_std_runs;       // [R, n_in], or NULL
  const int64_t* run_lane_offset;  // [R] global id of the run's lane 0
  int lanes_per_run;
};
int launch_rollout_runs(const PolicyKey& k, int env_kind, const RunsArgs& args, hipStream_t stream);

// fdr_rollout.hip: per-lane Welford obs statistics folded into the accumulated ones (fdr_obs_stats_merge)
int launch_obs_stats_merge(const float* mean, const float* m2, const int32_t* count, int n, int d, float* acc_mean,
                           float* acc_m2, int64_t* acc_count, hipStream_t stream);
// fdr_rollout_linear.hip: run r folds its lanes_per_run partials into accumulator r (fdr_obs_stats_merge_runs)
int launch_obs_stats_merge_runs(const float* mean, const float* m2, const int32_t* count, int n_runs, int lanes_per_run,
                                int d, float* acc_mean, float* acc_m2, int64_t* acc_count, hipStream_t stream);

}  // namespace fdr
