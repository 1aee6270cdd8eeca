// fdr_rollout_env.hip -- the rollout_kernel instances of the envs that are not the synthetic one: the trap
// gridworld at DiscretePolicy(2, 9), CartPole-v1 at DiscretePolicy(4, 2), Pendulum-v1 at MujocoPolicy(3, 1).
// Always the one-lane kernel, whatever the context's rollout_impl says.
#include "fdr_rollout_kernel.h"

namespace fdr {

int launch_rollout_env(const PolicyKey& k, int env_kind, const RolloutArgs& args, hipStream_t stream) {
  // physics envs: one policy shape each
  if (env_kind == FDR_ENV_CARTPOLE && (k.n_in != 4 || k.n_act != 2 || !k.discrete))
    return set_error(FDR_ERR_UNSUPPORTED, "CartPole needs a DiscretePolicy(4, 2)");
  if (env_kind == FDR_ENV_PENDULUM && (k.n_in != 3 || k.n_act != 1 || k.discrete))
    return set_error(FDR_ERR_UNSUPPORTED, "Pendulum needs a MujocoPolicy(3, 1)");
  const bool physics = env_kind == FDR_ENV_CARTPOLE || env_kind == FDR_ENV_PENDULUM;
  const char* const no_shape = "no compiled rollout for this (kind, n_in, n_act)";
  auto launch = [&](auto shape) {
    using S = decltype(shape);
    // no kFeatTerm: CartPole's termination lives under its ENV branch.  u_inject never comes with the Welford
    // statistics (fdr_rollout_ex refuses it).
    const int feat = rollout_feat(args, false);
    const char* const no_feat = "u_inject is not combined with the obs statistics";
    if constexpr (S::NIN == 4 && S::NA == 2 && S::DISC) {
      if (env_kind == FDR_ENV_CARTPOLE)
        return launch_rollout_kernel<S, FDR_ENV_CARTPOLE, false, kPhysicsFeatBits>(args, feat, stream,
                                                                                   "rollout_kernel<cartpole>", no_feat);
    }
    if constexpr (S::NIN == 3 && S::NA == 1 && !S::DISC) {
      if (env_kind == FDR_ENV_PENDULUM)
        return launch_rollout_kernel<S, FDR_ENV_PENDULUM, false, kPhysicsFeatBits>(args, feat, stream,
                                                                                   "rollout_kernel<pendulum>", no_feat);
    }
    if constexpr (S::NIN == 2 && S::NA == 9 && S::DISC) {
      if (env_kind == FDR_ENV_TRAP)
        return launch_rollout_kernel<S, FDR_ENV_TRAP, false, kLaneFeatBits>(
            args, feat, stream, "rollout_kernel<trap>", "no compiled rollout_kernel for this feature set");
    }
    return set_error(FDR_ERR_UNSUPPORTED, "env kind not compiled for this policy shape");
  };
  return physics ? with_shape<true>(k, no_shape, launch) : with_shape<false>(k, no_shape, launch);
}

}  // namespace fdr
