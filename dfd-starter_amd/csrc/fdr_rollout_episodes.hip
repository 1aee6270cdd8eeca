// fdr_rollout_episodes.hip -- rollout_episodes_kernel: K episodes per lane in one launch, for the five physics envs
// at their one policy shape (fdr_rollout_episodes).  theta' is formed once per lane (MlpLane::load) and held in
// registers / LDS over all K episodes; episode e of lane l is the episode rollout_kernel runs for global lane id
// id(l, e) = episode_ids[l * K + e], or (lane_offset + l) * K + e without the array: every draw -- the reset slots,
// the action draws, the obs-stat coins -- is keyed by that id, so lanes given equal ids play under common random
// numbers.  The jiggle alone stays keyed by the physical global lane lane_offset + l: lanes that share streams still
// get distinct tie-breakers.  The env steps, the policy and the draw batching are rollout_kernel's
// (fdr_rollout_kernel.h), statement for statement; rollout_kernel itself is not touched.
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
  using Lane = MlpLane<NIN, NA, DISC>;
  constexpr int NX = Lane::NX;
  __shared__ float4 wtile[kLanesPerBlock * Lane::kTileF4];
  __shared__ typename Lane::Scratch scratch[kLanesPerBlock];

  const int j = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = blockIdx.x * kLanesPerBlock + wv;
  if (lane >= a.n_lanes) return;

  ParamSrc src = a.lanes.src(lane);
  const bool det = a.lanes.deterministic ? a.lanes.deterministic[lane] != 0 : false;
  Lane pl;
  pl.load(src, j, a.bn_mean, a.bn_var, wtile + wv * Lane::kTileF4);
  {  // once per lane, before the first episode (rollout_kernel: a double live across the step loop would be spilled)
    double n2 = wave_sum(src.n2);
    asm volatile("" : "+v"(n2));
    if (j == 0 && a.norm2) a.norm2[lane] = n2;
  }

  const int ji = j < NIN ? j : NIN - 1;
  constexpr bool norm_obs = (FEAT & kFeatObsNorm) != 0;
  const float om = norm_obs ? a.obs_mean[ji] : 0.f;
  const float osd = norm_obs ? a.obs_std[ji] : 1.f;
  auto policy_input = [&](float s) {
    float x = s;
    if (norm_obs) x = fminf(fmaxf((s - om) / osd, -10.f), 10.f);  // agent.py:40-41
    return pl.input_transform(x);
  };

  const int T = a.T;
  const int K = ea.n_episodes;
  const uint64_t key = a.key;
  const uint64_t glane = (uint64_t)(a.lanes.lane_offset + lane);  // physical global lane: the jiggle's key
  const int o = j & 15;
  constexpr int kDrawsPerStep = DISC ? 1 : NA;
  constexpr int kStepsPerBatch = 64 / kDrawsPerStep;
  const int zbase = 4 * (o < NA ? o : 0);
  auto mark = [](int, float) {};

  // lane totals over the K episodes (wave-uniform, SGPRs) and the Welford stat that runs on across them
  double rsum = 0.0, rsq = 0.0, esum = 0.0;
  int nsum = 0;
  int os_n = 0;
  float os_mean = 0.f, os_m2 = 0.f;

  for (int ep = 0; ep < K; ++ep) {
    // the episode's stream id (wave-uniform: a scalar load or scalar arithmetic)
    uint64_t ulane = ea.episode_ids ? (uint64_t)ea.episode_ids[(int64_t)lane * K + ep]
                                    : glane * (uint64_t)K + (uint64_t)ep;
    ulane = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(ulane >> 32)) << 32) |
            (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)ulane);
    float px0 = 0.f, px1 = 0.f, px2 = 0.f, px3 = 0.f;
    auto physics_obs = [&]() {
      if constexpr (ENV == FDR_ENV_CARTPOLE) return j == 0 ? px0 : (j == 1 ? px1 : (j == 2 ? px2 : px3));
      else if constexpr (ENV == FDR_ENV_ACROBOT) return acrobot_obs(j, px0, px1, px2, px3);
      else if constexpr (ENV == FDR_ENV_MOUNTAINCAR || ENV == FDR_ENV_MOUNTAINCAR_CONT) return j == 0 ? px0 : px1;
      else return j == 0 ? px2 : (j == 1 ? px3 : px1);
    };
    float s = 0.f;
    if constexpr (ENV == FDR_ENV_CARTPOLE) {
      static_assert(NIN == 4 && NA == 2 && DISC, "CartPole: DiscretePolicy(4, 2)");
      px0 = physics_reset(key, ulane, 0, 0.1f, 0.05f);
      px1 = physics_reset(key, ulane, 1, 0.1f, 0.05f);
      px2 = physics_reset(key, ulane, 2, 0.1f, 0.05f);
      px3 = physics_reset(key, ulane, 3, 0.1f, 0.05f);
    } else if constexpr (ENV == FDR_ENV_PENDULUM) {
      static_assert(NIN == 3 && NA == 1 && !DISC, "Pendulum: MujocoPolicy(3, 1)");
      px0 = physics_reset(key, ulane, 0, kTwoPiF, kPiF);
      px1 = physics_reset(key, ulane, 1, 2.f, 1.f);
      px2 = cosf(px0);
      px3 = sinf(px0);
    } else if constexpr (ENV == FDR_ENV_ACROBOT) {
      static_assert(NIN == 6 && NA == 3 && DISC, "Acrobot: DiscretePolicy(6, 3)");
      px0 = physics_reset(key, ulane, 0, 0.2f, 0.1f);
      px1 = physics_reset(key, ulane, 1, 0.2f, 0.1f);
      px2 = physics_reset(key, ulane, 2, 0.2f, 0.1f);
      px3 = physics_reset(key, ulane, 3, 0.2f, 0.1f);
    } else if constexpr (ENV == FDR_ENV_MOUNTAINCAR) {
      static_assert(NIN == 2 && NA == 3 && DISC, "MountainCar: DiscretePolicy(2, 3)");
      px0 = physics_reset(key, ulane, 0, 0.2f, 0.6f);
    } else {
      static_assert(ENV == FDR_ENV_MOUNTAINCAR_CONT && NIN == 2 && NA == 1 && !DISC,
                    "MountainCarContinuous: MujocoPolicy(2, 1)");
      px0 = physics_reset(key, ulane, 0, 0.2f, 0.6f);
    }
    s = physics_obs();

    int nsteps = T;
    double racc = 0.0;
    float eacc = 0.f;
    float rbuf = 0.f;
    uint64_t os_mask = 0;
    auto draw = [&](int t) {
      const int ds = j / kDrawsPerStep, dk = j % kDrawsPerStep;
      const uint64_t h = hash_ctr(key, ulane, (uint64_t)(t + ds), (uint64_t)dk);
      rbuf = DISC ? uniform24(h) : normal_bm(h);
    };
    auto fetch_z = [&](int t) {
      if constexpr (DISC) return 0.f;
      const int addr = zbase + 4 * NA * (t % kStepsPerBatch);
      return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addr, __builtin_bit_cast(int, rbuf)));
    };
    // One episode, to its termination (the lambda returns: the wave goes on to the next episode) or to T.
    auto episode = [&](auto det_tag) {
      constexpr bool kDet = decltype(det_tag)::value;
      for (int t0 = 0; t0 < T; t0 += kStepsPerBatch) {
        if constexpr (!kDet) draw(t0);
        const int nb = T - t0 < kStepsPerBatch ? T - t0 : kStepsPerBatch;
        for (int tb = 0; tb < nb; ++tb) {
          const int t = t0 + tb;
          // W1 rows stay per-step LDS reads (rollout_kernel: hoisting them would spill W2)
          asm volatile("" ::: "memory");
          const float zt = fetch_z(t);
          if constexpr (FEAT & kFeatObsStats) {
            if ((t & 63) == 0) {
              const float u = uniform24(hash_ctr(key, ulane, (uint64_t)(t + j), 14));
              os_mask = __ballot(u < a.os_chance);
            }
            if ((os_mask >> (t & 63)) & 1ull) {
    #pragma clang fp contract(off)
              const int cc = os_n;
              os_n += 1;
              const float delta = s - os_mean;
              const float delta_n = delta / (float)os_n;
              os_mean += delta_n;
              os_m2 += (delta * delta_n) * (float)cc;
            }
          }
          auto* sc = &scratch[wv];
          sc->x[j] = j < NIN ? policy_input(s) : (j == NIN ? 1.f : 0.f);
          wave_lds_sync();
          float xb[NX];
          lds_bcast<NX>(sc->x, xb);
          const float h1 = pl.layer1(xb);
          const float y = pl.layers23(h1, sc, j, mark, nullptr);
          int act_d = 0;
          float act_c = 0.f;
          if constexpr (DISC) {
            const float p = pl.template softmax<false, !kDet>(y, j);
            float pv[NA];
    #pragma unroll
            for (int i = 0; i < NA; ++i) pv[i] = readlane_f(p, i);
            float tot = pv[0];
    #pragma unroll
            for (int i = 1; i < NA; ++i) tot += pv[i];
            if constexpr (kDet) {
              float best = pv[0];
    #pragma unroll
              for (int i = 1; i < NA; ++i) {
                act_d = pv[i] > best ? i : act_d;
                best = fmaxf(best, pv[i]);
              }
            } else {
              const float target = readlane_f(rbuf, tb) * tot;
              float c = 0.f;
    #pragma unroll
              for (int i = 0; i < NA - 1; ++i) {
                c += pv[i];
                act_d += c <= target ? 1 : 0;
              }
            }
            eacc -= (j < NA) ? disc_entropy_term(p, tot) : 0.f;
          } else {
            const float th = tanh_fast(y);
            const float sd = std_from_tanh(dpp_mov<kDppRowShl + NA>(th));
            eacc += __builtin_amdgcn_logf(sd);
            act_c = kDet ? th : gauss_action(th, sd, zt);
          }
          // ---- env step ----
          if constexpr (ENV == FDR_ENV_CARTPOLE) {
            const bool fail = cartpole_step(px0, px1, px2, px3, act_d);
            racc += 1.0;
            s = physics_obs();
            if (__builtin_amdgcn_readfirstlane(fail ? 1 : 0)) {
              nsteps = t + 1;
              return;
            }
          } else if constexpr (ENV == FDR_ENV_PENDULUM) {
            racc += (double)pendulum_step(px0, px1, px2, px3, readlane_f(act_c, 0));
            s = physics_obs();
          } else if constexpr (ENV == FDR_ENV_ACROBOT) {
            const bool done = acrobot_step(px0, px1, px2, px3, act_d);
            s = physics_obs();
            if (__builtin_amdgcn_readfirstlane(done ? 1 : 0)) {
              nsteps = t + 1;
              return;
            }
            racc -= 1.0;
          } else if constexpr (ENV == FDR_ENV_MOUNTAINCAR) {
            const bool done = mountaincar_step(px0, px1, (float)(act_d - 1) * 0.001f, 0.5f);
            racc -= 1.0;
            s = physics_obs();
            if (__builtin_amdgcn_readfirstlane(done ? 1 : 0)) {
              nsteps = t + 1;
              return;
            }
          } else {
            const float ac = readlane_f(act_c, 0);
            const bool done = mountaincar_step(px0, px1, fminf(fmaxf(ac, -1.f), 1.f) * 0.0015f, 0.45f);
            racc += (double)((done ? 100.f : 0.f) - 0.1f * ac * ac);
            s = physics_obs();
            if (__builtin_amdgcn_readfirstlane(done ? 1 : 0)) {
              nsteps = t + 1;
              return;
            }
          }
        }
      }
    };
    if (det)
      episode(std::true_type{});
    else
      episode(std::false_type{});

    // ---- fold the episode into the lane totals (sequential f64, episode order) ----
    eacc *= 0.693147180559945309f;  // log2 -> ln
    const double es = wave_sum((j < NA) ? (double)eacc : 0.0);
    const double r = uniform_f64(racc);
    rsum = uniform_f64(rsum + r);
    rsq = uniform_f64(rsq + r * r);
    esum = uniform_f64(esum + es);
    nsum += __builtin_amdgcn_readfirstlane(nsteps);
  }

  // ---- epilogue ----
  if (j == 0) {
    double r = rsum / (double)K;
    if (a.jiggle) r += (hash_ctr(key, glane, kJiggleT, 15) & 1ull) ? 1e-12 : -1e-12;
    a.ret[lane] = r;
    if (ea.ret_sq) ea.ret_sq[lane] = rsq;
    double e = esum / (double)nsum;
    if constexpr (!DISC) e += (double)NA * 1.4189385332046727;
    a.ent[lane] = e;
    a.steps[lane] = nsum;
  }
  if constexpr (FEAT & kFeatObsStats) {
    if (j < NIN) {
      a.os_mean[(int64_t)lane * NIN + j] = os_mean;
      a.os_m2[(int64_t)lane * NIN + j] = os_m2;
    }
    if (j == 0) a.os_count[lane] = os_n;
  }
}

constexpr int kEpisodesFeatBits = kFeatObsStats | kFeatObsNorm;  // 4 sets per env

template <class S, int ENV, int NIN, int NA, bool DISC>
bool launch_episodes(int env_kind, const EpisodesArgs& args, int feat, hipStream_t stream, const char* what, int& rc) {
  if constexpr (S::NIN == NIN && S::NA == NA && S::DISC == DISC) {
    if (env_kind == ENV) {
      const dim3 grid((args.r.n_lanes + kLanesPerBlock - 1) / kLanesPerBlock), block(64 * kLanesPerBlock);
      const bool hit = launch_feat_set<kEpisodesFeatBits>(feat, [&](auto f) {
        hipLaunchKernelGGL((rollout_episodes_kernel<NIN, NA, DISC, ENV, decltype(f)::value>), grid, block, 0, stream,
                           args);
      });
      rc = hit ? check_launch(what)
               : set_error(FDR_ERR_UNSUPPORTED, "fdr_rollout_episodes takes no state recording or injected draws");
      return true;
    }
  }
  return false;
}

int launch_rollout_episodes(const PolicyKey& k, int env_kind, const EpisodesArgs& args, hipStream_t stream) {
  const PhysicsEnv* const pe = physics_env(env_kind);
  if (!pe) return set_error(FDR_ERR_UNSUPPORTED, "fdr_rollout_episodes runs the physics envs only");
  if (!physics_policy_ok(*pe, k)) return set_error(FDR_ERR_UNSUPPORTED, pe->policy_msg);
  return with_shape<true>(k, "no compiled rollout for this (kind, n_in, n_act)", [&](auto shape) {
    using S = decltype(shape);
    const int feat = rollout_feat(args.r, false);
    int rc = FDR_OK;
    if (launch_episodes<S, FDR_ENV_CARTPOLE, 4, 2, true>(env_kind, args, feat, stream,
                                                        "rollout_episodes_kernel<cartpole>", rc) ||
        launch_episodes<S, FDR_ENV_PENDULUM, 3, 1, false>(env_kind, args, feat, stream,
                                                          "rollout_episodes_kernel<pendulum>", rc) ||
        launch_episodes<S, FDR_ENV_ACROBOT, 6, 3, true>(env_kind, args, feat, stream,
                                                        "rollout_episodes_kernel<acrobot>", rc) ||
        launch_episodes<S, FDR_ENV_MOUNTAINCAR, 2, 3, true>(env_kind, args, feat, stream,
                                                            "rollout_episodes_kernel<mountaincar>", rc) ||
        launch_episodes<S, FDR_ENV_MOUNTAINCAR_CONT, 2, 1, false>(env_kind, args, feat, stream,
                                                                  "rollout_episodes_kernel<mountaincar_cont>", rc))
      return rc;
    return set_error(FDR_ERR_UNSUPPORTED, "env kind not compiled for this policy shape");
  });
}

}  // namespace fdr
