// fdr_rollout_episodes.hip -- rollout_episodes_kernel: K episodes per lane in one launch, for the five physics envs
// at their one policy shape (fdr_rollout_episodes).  theta' is formed once per lane (MlpLane::load) and held in
// registers / LDS over all K episodes; episode e of lane l is the episode rollout_kernel runs for global lane id
// id(l, e) = episode_ids[l * K + e], or (lane_offset + l) * K + e without the array: every draw -- the reset slots,
// the action draws, the obs-stat coins -- is keyed by that id, so lanes given equal ids play under common random
// numbers.  The jiggle alone stays keyed by the physical global lane lane_offset + l: lanes that share streams still
// get distinct tie-breakers.  The env (PhysicsSim), the obs statistics and the lane frame are the shared pieces of
// fdr_rollout_parts.h; this file holds the episode loop and the fold into the lane's totals.
#include "fdr_rollout_kernel.h"

namespace fdr {

// A wave-uniform double held in SGPRs (lane 0's value: every lane of a physics wave holds the same sums).
__device__ __forceinline__ double uniform_f64(double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b >> 32));
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// FEAT: a subset of kFeatObsNorm | kFeatObsStats (no state recording, no injected draws on this route).
template <int NIN, int NA, bool DISC, int ENV, int FEAT>
__global__ __launch_bounds__(64 * kLanesPerBlock, 4) void rollout_episodes_kernel(EpisodesArgs ea) {
  const RolloutArgs& a = ea.r;
  static_assert((FEAT & ~(kFeatObsNorm | kFeatObsStats)) == 0, "episodes: obs-norm and obs-stats only");
  static_assert(PhysicsSpec<ENV>::template is_shape<NIN, NA, DISC>(), "a physics env runs under its own policy shape");
  using Lane = MlpLane<NIN, NA, DISC>;
  constexpr int NX = Lane::NX;
  __shared__ float4 wtile[kLanesPerBlock * Lane::kTileF4];
  __shared__ typename Lane::Scratch scratch[kLanesPerBlock];

  const int j = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = blockIdx.x * kLanesPerBlock + wv;
  if (lane >= a.n_lanes) return;

  Lane pl;  // once per lane, before the first episode
  const bool det = lane_prologue(a, lane, j, wtile + wv * Lane::kTileF4, pl);
  const ObsInput<(FEAT & kFeatObsNorm) != 0> obs_input(a, j < NIN ? j : NIN - 1);

  const int T = a.T;
  const int K = ea.n_episodes;
  const uint64_t key = a.key;
  const uint64_t glane = (uint64_t)(a.lanes.lane_offset + lane);  // physical global lane: the jiggle's key
  using Draws = DrawBatch<NA, DISC>;
  auto mark = [](int, float) {};

  // lane totals over the K episodes (wave-uniform, SGPRs) and the Welford stat that runs on across them
  double rsum = 0.0, rsq = 0.0, esum = 0.0;
  int nsum = 0;
  [[maybe_unused]] ObsWelford os;

  for (int ep = 0; ep < K; ++ep) {
    // the episode's stream id (wave-uniform: a scalar load or scalar arithmetic)
    uint64_t ulane = ea.episode_ids ? (uint64_t)ea.episode_ids[(int64_t)lane * K + ep]
                                    : glane * (uint64_t)K + (uint64_t)ep;
    ulane = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(ulane >> 32)) << 32) |
            (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)ulane);
    PhysicsSim<ENV> sim;
    sim.reset(key, ulane);
    float s = sim.obs(j);

    int nsteps = T;
    double racc = 0.0;
    float eacc = 0.f;
    Draws draws;
    // One episode, to its termination (the lambda returns: the wave goes on to the next episode) or to T.
    auto episode = [&](auto det_tag) {
      constexpr bool kDet = decltype(det_tag)::value;
      for (int t0 = 0; t0 < T; t0 += Draws::kStepsPerBatch) {
        if constexpr (!kDet) draws.draw(key, ulane, t0, j);
        const int nb = T - t0 < Draws::kStepsPerBatch ? T - t0 : Draws::kStepsPerBatch;
        for (int tb = 0; tb < nb; ++tb) {
          const int t = t0 + tb;
          // W1 rows stay per-step LDS reads (rollout_kernel: hoisting them would spill W2)
          asm volatile("" ::: "memory");
          const float zt = draws.z(t, j);
          if constexpr (FEAT & kFeatObsStats) os.visit(a, ulane, t, j, s);
          auto* sc = &scratch[wv];
          sc->x[j] = j < NIN ? obs_input(pl, s) : (j == NIN ? 1.f : 0.f);
          wave_lds_sync();
          float xb[NX];
          lds_bcast<NX>(sc->x, xb);
          const float h1 = pl.layer1(xb);
          const float y = pl.layers23(h1, sc, j, mark, nullptr);
          int act_d = 0;
          float act_c = 0.f;
          if constexpr (DISC)
            act_d = select_action<NA, kDet>(pl.template softmax<false, !kDet>(y, j), draws, tb, j, eacc);
          else
            act_c = gauss_head_action<NA, kDet>(y, zt, eacc);
          if (sim.step(j, act_d, act_c, racc, s)) {
            nsteps = t + 1;
            return;
          }
        }
      }
    };
    if (det)
      episode(std::true_type{});
    else
      episode(std::false_type{});

    // ---- fold the episode into the lane totals (sequential f64, episode order) ----
    const double es = entropy_sum(eacc, j, NA);
    const double r = uniform_f64(racc);
    rsum = uniform_f64(rsum + r);
    rsq = uniform_f64(rsq + r * r);
    esum = uniform_f64(esum + es);
    nsum += __builtin_amdgcn_readfirstlane(nsteps);
  }

  // ---- epilogue ----
  store_results<DISC>(a, lane, j, glane, rsum / (double)K, esum, nsum, NA);
  if (j == 0 && ea.ret_sq) ea.ret_sq[lane] = rsq;
  if constexpr (FEAT & kFeatObsStats) os.store(a, lane, NIN, j);
}

constexpr int kEpisodesFeatBits = kFeatObsStats | kFeatObsNorm;  // 4 sets per env

int launch_rollout_episodes(const PolicyKey& k, int env_kind, const EpisodesArgs& args, hipStream_t stream) {
  const PhysicsEnv* const pe = physics_env(env_kind);
  if (!pe) return set_error(FDR_ERR_UNSUPPORTED, "fdr_rollout_episodes runs the physics envs only");
  if (!physics_policy_ok(*pe, k)) return set_error(FDR_ERR_UNSUPPORTED, pe->policy_msg);
  return with_shape<true>(k, "no compiled rollout for this (kind, n_in, n_act)", [&](auto shape) {
    using S = decltype(shape);
    const int feat = rollout_feat(args.r, false);
    const dim3 grid((args.r.n_lanes + kLanesPerBlock - 1) / kLanesPerBlock), block(64 * kLanesPerBlock);
    int rc = FDR_OK;
    with_physics_env(env_kind, [&](auto spec) {  // pe: env_kind is one of them
      using E = decltype(spec);
      if constexpr (E::template is_shape<S::NIN, S::NA, S::DISC>()) {
        const bool hit = launch_feat_set<kEpisodesFeatBits>(feat, [&](auto f) {
          hipLaunchKernelGGL((rollout_episodes_kernel<S::NIN, S::NA, S::DISC, E::ENV, decltype(f)::value>), grid,
                             block, 0, stream, args);
        });
        rc = hit ? check_launch(E::episodes_name)
                 : set_error(FDR_ERR_UNSUPPORTED, "fdr_rollout_episodes takes no state recording or injected draws");
      } else {
        rc = set_error(FDR_ERR_UNSUPPORTED, "env kind not compiled for this policy shape");
      }
    });
    return rc;
  });
}

}  // namespace fdr
