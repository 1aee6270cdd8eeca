// fdr_rollout_env.hip -- the rollout_kernel instances of the envs that are not the synthetic one: the trap
// gridworld at DiscretePolicy(2, 9) and the five classic-control physics envs, each at its PhysicsSpec shape
// (fdr_internal.h).  Always the one-lane kernel, whatever the context's rollout_impl says.
#include "fdr_rollout_kernel.h"

namespace fdr {

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
    const char* const no_env = "env kind not compiled for this policy shape";
    int rc = FDR_OK;
    // a physics env at its one shape: launched when S is that shape
    if (with_physics_env(env_kind, [&](auto spec) {
          using E = decltype(spec);
          if constexpr (E::template is_shape<S::NIN, S::NA, S::DISC>())
            rc = launch_rollout_kernel<S, E::ENV, false, kPhysicsFeatBits>(
                args, feat, stream, E::rollout_name, "u_inject is not combined with the obs statistics");
          else
            rc = set_error(FDR_ERR_UNSUPPORTED, no_env);
        }))
      return rc;
    if constexpr (S::NIN == 2 && S::NA == 9 && S::DISC) {
      if (env_kind == FDR_ENV_TRAP)
        return launch_rollout_kernel<S, FDR_ENV_TRAP, false, kLaneFeatBits>(
            args, feat, stream, "rollout_kernel<trap>", "no compiled rollout_kernel for this feature set");
    }
    return set_error(FDR_ERR_UNSUPPORTED, no_env);
  };
  return pe ? with_shape<true>(k, no_shape, launch) : with_shape<false>(k, no_shape, launch);
}

}  // namespace fdr
