// fdr_rollout_wide.hip -- the synthetic-env rollout_kernel<WIDE> instances: one lane per wave with a 256-VGPR
// budget, for launches of few lanes (launch_rollout, use_wide_kernel).  No injected draws.
#include "fdr_rollout_kernel.h"

namespace fdr {

int launch_rollout_wide(const PolicyKey& k, const RolloutArgs& args, hipStream_t stream) {
  return with_shape<false>(k, "no compiled rollout for this (kind, n_in, n_act)", [&](auto shape) {
    return launch_rollout_kernel<decltype(shape), FDR_ENV_SYNTH, true, kWideFeatBits>(
        args, rollout_feat(args, args.done_thr > 0.f), stream, "rollout_kernel<synth, wide>",
        "no compiled rollout_kernel<wide> for this feature set");
  });
}

}  // namespace fdr
