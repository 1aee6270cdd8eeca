// fdr_rollout_env.hip -- the rollout_kernel instances of the envs that are not the synthetic one: the trap
// gridworld at DiscretePolicy(2, 9), CartPole-v1 at DiscretePolicy(4, 2), Pendulum-v1 at MujocoPolicy(3, 1),
// Acrobot-v1 at DiscretePolicy(6, 3), MountainCar-v0 at DiscretePolicy(2, 3), MountainCarContinuous-v0 at
// MujocoPolicy(2, 1).  Always the one-lane kernel, whatever the context's rollout_impl says.
#include "fdr_rollout_kernel.h"

namespace fdr {

// The physics env ENV at its one shape (NIN, NA, DISC): launched when S is that shape and env_kind that env.
template <class S, int ENV, int NIN, int NA, bool DISC>
bool launch_physics(int env_kind, const RolloutArgs& args, int feat, hipStream_t stream, const char* what, int& rc) {
  if constexpr (S::NIN == NIN && S::NA == NA && S::DISC == DISC) {
    if (env_kind == ENV) {
      rc = launch_rollout_kernel<S, ENV, false, kPhysicsFeatBits>(args, feat, stream, what,
                                                                  "u_inject is not combined with the obs statistics");
      return true;
    }
  }
  return false;
}

int launch_rollout_env(const PolicyKey& k, int env_kind, const RolloutArgs& args, hipStream_t stream) {
  // physics envs: one policy shape each
  const PhysicsEnv* const pe = physics_env(env_kind);
  if (pe && !physics_policy_ok(*pe, k)) return set_error(FDR_ERR_UNSUPPORTED, pe->policy_msg);
  const char* const no_shape = "no compiled rollout for this (kind, n_in, n_act)";
  auto launch = [&](auto shape) {
    using S = decltype(shape);
    // no kFeatTerm: a physics env's termination lives under its ENV branch.  u_inject never comes with the Welford
    // statistics (fdr_rollout_ex refuses it).
    const int feat = rollout_feat(args, false);
    int rc = FDR_OK;
    if (launch_physics<S, FDR_ENV_CARTPOLE, 4, 2, true>(env_kind, args, feat, stream, "rollout_kernel<cartpole>", rc) ||
        launch_physics<S, FDR_ENV_PENDULUM, 3, 1, false>(env_kind, args, feat, stream, "rollout_kernel<pendulum>", rc) ||
        launch_physics<S, FDR_ENV_ACROBOT, 6, 3, true>(env_kind, args, feat, stream, "rollout_kernel<acrobot>", rc) ||
        launch_physics<S, FDR_ENV_MOUNTAINCAR, 2, 3, true>(env_kind, args, feat, stream,
                                                           "rollout_kernel<mountaincar>", rc) ||
        launch_physics<S, FDR_ENV_MOUNTAINCAR_CONT, 2, 1, false>(env_kind, args, feat, stream,
                                                                 "rollout_kernel<mountaincar_cont>", rc))
      return rc;
    if constexpr (S::NIN == 2 && S::NA == 9 && S::DISC) {
      if (env_kind == FDR_ENV_TRAP)
        return launch_rollout_kernel<S, FDR_ENV_TRAP, false, kLaneFeatBits>(
            args, feat, stream, "rollout_kernel<trap>", "no compiled rollout_kernel for this feature set");
    }
    return set_error(FDR_ERR_UNSUPPORTED, "env kind not compiled for this policy shape");
  };
  return pe ? with_shape<true>(k, no_shape, launch) : with_shape<false>(k, no_shape, launch);
}

}  // namespace fdr
