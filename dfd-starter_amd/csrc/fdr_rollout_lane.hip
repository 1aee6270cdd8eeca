// fdr_rollout_lane.hip -- the synthetic-env rollout_kernel instances, one lane per wave (128-VGPR budget).
#include "fdr_rollout_kernel.h"

namespace fdr {

// terminating env instances (kFeatTerm) only for the synthetic env, so the fixed-length kernels stay as they are
int launch_rollout_lane(const PolicyKey& k, const RolloutArgs& args, hipStream_t stream) {
  return with_shape<false>(k, "no compiled rollout for this (kind, n_in, n_act)", [&](auto shape) {
    return launch_rollout_kernel<decltype(shape), FDR_ENV_SYNTH, false, kLaneFeatBits>(
        args, rollout_feat(args, args.done_thr > 0.f), stream, "rollout_kernel<synth>",
        "no compiled rollout_kernel for this feature set");
  });
}

}  // namespace fdr
