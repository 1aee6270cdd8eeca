// fdr_rollout_kernel.h -- the one-lane-per-wave rollout_kernel template with the envs it steps (the synthetic
// linear-tanh system, the trap gridworld, gym's five classic-control systems).  Instantiated by fdr_rollout_lane.hip
// (synthetic env), fdr_rollout_wide.hip (WIDE) and fdr_rollout_env.hip (trap, CartPole, Pendulum, Acrobot, MountainCar,
// MountainCarContinuous).
#pragma once
#include "fdr_rollout_parts.h"

namespace fdr {

// trap-env observation (environment.py:59-61): python f64 division, cast to f32 by the policy
__device__ __forceinline__ float trap_obs(int j, int col, int row) {
  return j == 0 ? (float)((double)(col * 7) / 1918.0) : (float)((double)(row * 7) / 1071.0);
}

// ---------------------------------------------------------------------------------------------
// Whole-episode rollout: fdr_rollout
// ---------------------------------------------------------------------------------------------
// FEAT (fdr_mlp.h): kFeatStates: record visited observations (fdr_rollout_states); kFeatObsStats: Welford obs
// statistics; kFeatObsNorm: observation normalisation (obs_mean / obs_std given); kFeatInject: host-injected draws
// (u_inject); kFeatTerm: terminating synthetic env (fdr_env_desc.done_threshold): the lane's episode ends after the
// step whose next state has |s'[done_dim]| > done_threshold (worker/agent.py:50-52: done -> break), or at T
// (one lane per wave: the wave leaves its loop -- only these instances carry the test)
// ENV: FDR_ENV_SYNTH, FDR_ENV_TRAP, or a physics env at its PhysicsSpec shape (fdr_internal.h; !WIDE only) -- per-lane
// reset states from the counter stream, each env's termination test in PhysicsSim::step (not kFeatTerm).
// Of the pieces shared with rollout_episodes_kernel (fdr_rollout_parts.h) the prologue, the draw batch, the discrete
// selection and the Welford update keep their own text here: the synth / trap instances stay as is.
// WIDE (synthetic env, few lanes: <= 2 waves per SIMD): a 256-VGPR budget instead of 128, so the
// step's loop invariants (M / K rows, the head's W3 slice) stay in registers; the policy input and env
// state cross lanes by v_readlane instead of an LDS round trip (NIN <= 8); a discrete env's candidate
// next states tanh(M s + K[:, a]) are formed for every action while the policy runs, so the action
// only selects one.
template <int NIN, int NA, bool DISC, int ENV, int FEAT, bool WIDE>
__global__ __launch_bounds__(64 * kLanesPerBlock, WIDE ? 2 : 4) void rollout_kernel(RolloutArgs a) {
  using Lane = MlpLane<NIN, NA, DISC>;
  constexpr int NX = Lane::NX;
  constexpr bool kRegIn = WIDE && ENV == FDR_ENV_SYNTH && !Lane::kW1Lds;
  constexpr bool kCand = kRegIn && DISC && NA <= 4;
  constexpr bool kHead2 = WIDE && DISC && NA == 2;
  // env rows [M[i] (NX) | K[i] (one column per action)], stride MKS (b128 rows)
  constexpr int NMK = NX + round4(NA);
  constexpr int MKS = NMK % 8 == 0 ? NMK + 4 : NMK;
  __shared__ float4 env4[(ENV == FDR_ENV_SYNTH) ? NIN * MKS / 4 : 1];
  __shared__ float4 wtile[kLanesPerBlock * Lane::kTileF4];
  __shared__ typename Lane::Scratch scratch[kLanesPerBlock];
  float* envMK = reinterpret_cast<float*>(env4);

  // wv through readfirstlane: the compiler then treats the lane index (and det) as wave-uniform (SGPRs,
  // scalar branches) instead of masking EXEC around the sampled / deterministic action paths
  const int j = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = blockIdx.x * kLanesPerBlock + wv;
  if constexpr (ENV == FDR_ENV_SYNTH) {
    for (int e = threadIdx.x; e < NIN * MKS; e += blockDim.x) {  // padding columns zero (b128 row reads)
      const int i = e / MKS, k = e % MKS;
      envMK[e] = (k < NIN ? a.M[i * NIN + k] : (k >= NX && k < NX + NA ? a.K[i * NA + k - NX] : 0.f));
    }
    __syncthreads();  // the only cross-wave hand-off: shared env matrices
  }
  if (lane >= a.n_lanes) return;

  ParamSrc src = a.lanes.src(lane);
  const bool det = a.lanes.deterministic ? a.lanes.deterministic[lane] != 0 : false;
  Lane pl;
  pl.load(src, j, a.bn_mean, a.bn_var, wtile + wv * Lane::kTileF4);
  {  // written now: a double live across the T-step loop would be spilled (and the asm keeps the compiler from
     // sinking the norm past the loop with every element's sigma * eps in scratch)
    double n2 = wave_sum(src.n2);
    asm volatile("" : "+v"(n2));
    if (j == 0 && a.norm2) a.norm2[lane] = n2;
  }

  const int ji = j < NIN ? j : NIN - 1;
  constexpr bool norm_obs = (FEAT & kFeatObsNorm) != 0;
  const ObsInput<norm_obs> obs_input(a, ji);
  auto policy_input = [&](float s) { return obs_input(pl, s); };

  int col = 0, row = 0;  // trap env state (wave-uniform)
  float s = 0.f;         // synthetic env state element j (j < NIN)
  if constexpr (ENV == FDR_ENV_SYNTH) {
    s = a.s0[ji];
  } else if constexpr (ENV == FDR_ENV_TRAP) {
    col = a.trap_start_col;
    row = a.trap_start_row;
    s = trap_obs(j, col, row);
  }
  const int T = a.T;
  const uint64_t key = a.key;
  const uint64_t ulane = (uint64_t)(a.lanes.lane_offset + lane);  // global lane id
  constexpr bool kPhysics = ENV != FDR_ENV_SYNTH && ENV != FDR_ENV_TRAP;
  [[maybe_unused]] PhysicsSim<ENV> sim;  // physics env state (wave-uniform)
  if constexpr (kPhysics) {
    static_assert(PhysicsSpec<ENV>::template is_shape<NIN, NA, DISC>() && !WIDE,
                  "a physics env runs under its own policy shape, one-lane kernel");
    sim.reset(key, ulane);
    s = sim.obs(j);
  }
  constexpr bool kTerm = (FEAT & kFeatTerm) != 0;
  int nsteps = T;  // env.step calls of the episode (agent.py:47)
  double racc = 0.0;
  float eacc = 0.f;  // per-lane entropy sum (f32: T terms of O(1), rel. error ~1e-7 * sqrt(T))
  const int o = j & 15;
  // Random draws are made in batches: one counter hash per lane covers up to 64 future draws
  // (discrete: lane i holds the uniform of step t0 + i; continuous: lane i holds the normal of
  // step t0 + i / NA, dim i % NA).  Same (lane, t, k) counters as drawing them one at a time.
  constexpr int kDrawsPerStep = DISC ? 1 : NA;
  constexpr int kStepsPerBatch = 64 / kDrawsPerStep;
  float rbuf = 0.f;
  uint64_t os_mask = 0;  // obs-stat coins of the current 64-step batch (wave-uniform)
  int os_n = 0;
  float os_mean = 0.f, os_m2 = 0.f;

#ifdef FDR_PHASE_STAMPS
  uint64_t ph_acc[5] = {0, 0, 0, 0, 0};
  uint64_t ph_last = 0;
  auto mark = [&](int k, float dep) {
    uint64_t now;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now) : "v"(dep));
    if (k >= 0) ph_acc[k] += now - ph_last;
    ph_last = now;
  };
#else
  auto mark = [](int, float) {};
#endif
  // Draw batch starting at step t (lane-parallel), and the normal of step t for action dim o.
  auto draw = [&](int t) {
    const int ds = j / kDrawsPerStep, dk = j % kDrawsPerStep;
    if constexpr ((FEAT & kFeatInject) != 0) {  // host-injected draws (u_inject), same batch layout
      const int tt = t + ds;
      rbuf = tt < T ? a.u_inject[((int64_t)lane * T + tt) * kDrawsPerStep + dk] : 0.f;
    } else {
      const uint64_t h = hash_ctr(key, ulane, (uint64_t)(t + ds), (uint64_t)dk);
      rbuf = DISC ? uniform24(h) : normal_bm(h);
    }
  };
  // WIDE: loop invariants in registers (M row ji, K row ji, the head's W3 slice)
  float mreg[kRegIn ? NX : 1], kreg[WIDE ? NA : 1], w3reg[WIDE ? 16 : 1];
  if constexpr (WIDE) {
    if constexpr (ENV == FDR_ENV_SYNTH) {
      const float* mr = envMK + ji * MKS;
#pragma unroll
      for (int k = 0; k < NA; ++k) kreg[k] = mr[NX + k];
      if constexpr (kRegIn) {
#pragma unroll
        for (int k = 0; k < NX; ++k) mreg[k] = mr[k];
      }
    }
    pl.head_weights(w3reg);
  }
  f2 w3c = {0.f, 0.f};  // head2: (W3[0][j], W3[1][j]) from lane (j >> 4, o) of the tile
  float b3p = 0.f;
  if constexpr (kHead2) {
    const float* t0 = reinterpret_cast<const float*>(pl.tile - j + (Lane::kW1Chunks + ((j & 15) >> 2)) * kWave +
                                                     (j >> 4) * 16);
    w3c = f2{t0[j & 3], t0[4 + (j & 3)]};
    if (WIDE && (j & 1)) w3c = f2{w3c.y, w3c.x};  // output j & 1 first (head2<true>)
    const float b30 = readlane_f(pl.b3, 0), b31 = readlane_f(pl.b3, 1);
    b3p = (j & 1) ? b31 : b30;
  }
  const int zbase = 4 * (o < NA ? o : 0);  // ds_bpermute byte address of dim o in step 0 of a batch
  auto fetch_z = [&](int t) {
    if constexpr (DISC) return 0.f;
    const int addr = zbase + 4 * NA * (t % kStepsPerBatch);
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addr, __builtin_bit_cast(int, rbuf)));
  };
  // The deterministic / sampled choice is fixed for the episode (wave-uniform): one specialised loop each, and the
  // draw batches as an outer loop, so the per-step body carries neither branch.
  auto episode = [&](auto det_tag) {
    constexpr bool kDet = decltype(det_tag)::value;
    for (int t0 = 0; t0 < T; t0 += kStepsPerBatch) {
      if constexpr (!kDet) draw(t0);
      const int nb = T - t0 < kStepsPerBatch ? T - t0 : kStepsPerBatch;
      for (int tb = 0; tb < nb; ++tb) {
        const int t = t0 + tb;
        // The W1 / M / K rows are loop-invariant LDS data; hoisting their loads out of the loop would
        // pin ~46 more VGPRs (and spill W2).  Keep them per-step reads.
        asm volatile("" ::: "memory");
        mark(-1, s);
        const float zt = fetch_z(t);  // this step's normal for action dim o (continuous)
        if constexpr (FEAT & kFeatStates) {  // visited (raw) observations, worker/agent.py:36 / 58-59 (save_states)
          if (j < NIN) a.states[((int64_t)lane * T + t) * NIN + j] = s;
        }
        if constexpr (FEAT & kFeatObsStats) {
          // worker/agent.py:37-39: with probability obs_stats_update_chance the raw obs enters the lane's
          // WelfordRunningStat (utils/math_helpers.py:29-38, f32, same operation order, no contraction).
          // Coins come 64 steps at a time: lane i draws step t + i (counter k = 14), one ballot.
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
        constexpr bool kSame = !DISC && !norm_obs;  // mujoco: policy input == env state
        const float* mrow = envMK + ji * MKS;
        float pre = 0.f;
        float h1;
        float cand[kCand ? NA : 1];  // discrete WIDE: next state for each action
        if constexpr (kRegIn) {
          // policy input and env state of lanes 0 .. NIN-1, wave-uniform through v_readlane
          const float xin = j < NIN ? policy_input(s) : 0.f;
          float xv[NX], sv[NX];
    #pragma unroll
          for (int k = 0; k < NX; ++k) {
            xv[k] = k < NIN ? readlane_f(xin, k) : (k == NIN ? 1.f : 0.f);
            sv[k] = k < NIN ? (kSame ? xv[k] : readlane_f(s, k)) : 0.f;
          }
          h1 = pl.layer1_env_reg(xv, sv, mreg, pre);
          if constexpr (kCand) {
    #pragma unroll
            for (int i = 0; i < NA; ++i) cand[i] = tanh_fast(pre + kreg[i]);
          }
        } else {
        // policy input (and env state) broadcast through the wave's LDS scratch, then packed FMAs
        // against the lane's W1 row and M row (two MACs per instruction instead of one DPP FMA)
        sc->x[j] = j < NIN ? policy_input(s) : (j == NIN ? 1.f : 0.f);
        if constexpr (ENV == FDR_ENV_SYNTH && !kSame) sc->h1[j] = j < NIN ? s : 0.f;
        wave_lds_sync();
        if constexpr (ENV == FDR_ENV_SYNTH) {
          // one pass over the input chunks: W1 row j against x, M row j against s (M's padding
          // columns are 0, so the bias column's 1 drops out of M s)
          h1 = pl.template layer1_env_pk<kSame>(sc->x, sc->h1, mrow, pre);
        } else {
          float xb[NX];
          lds_bcast<NX>(sc->x, xb);
          h1 = pl.layer1(xb);
        }
        }
        mark(0, h1);
        float y;
        if constexpr (kHead2) {
          const float h2 = pl.template layer2<WIDE>(h1, sc, j);
          mark(1, h2);
          y = pl.template head2<WIDE>(h2, w3c, b3p, j);
          mark(2, y);
        } else {
          y = pl.layers23(h1, sc, j, mark, WIDE ? w3reg : nullptr);
        }
        int act_d = 0;
        float act_c = 0.f;
        if constexpr (DISC) {
          float p;
          p = pl.template softmax<kHead2, !kDet>(y, j);
          if constexpr (kHead2 && !kDet) {
            // two outputs, sampled: everything in VALU, no readlane round trip -- lane parity o holds p_o;
            // tot = p0 + p1 (the oracle's 0 + p0 + p1, exactly), p0 to every lane by one DPP move, and the
            // inverse CDF of two outputs is (p0 <= u tot); no contraction of p's product into the sum
    #pragma clang fp contract(off)
            const float tot = p + dpp_mov<kDppQuadXor1>(p);
            const float p0 = dpp_mov<0xA0>(p);  // quad_perm [0,0,2,2]
            act_d = p0 <= readlane_f(rbuf, tb) * tot ? 1 : 0;
            eacc -= (j < NA) ? disc_entropy_term(p, tot) : 0.f;
          } else {
          float pv[NA];
    #pragma unroll
          for (int i = 0; i < NA; ++i) pv[i] = readlane_f(p, i);
          float tot = pv[0];  // sequential f32 cumsum, the oracle's order (0 + p0 == p0)
    #pragma unroll
          for (int i = 1; i < NA; ++i) tot += pv[i];
          // Branch-free selection (selects, no data-dependent control flow):
          //   argmax = first maximal index; inverse CDF = first i with cumsum_i > target, i.e. the
          //   number of (monotone) partial sums <= target, capped at NA - 1.
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
          // Categorical(probs) entropy: probs normalised, log clamped (torch semantics)
          eacc -= (j < NA) ? disc_entropy_term(p, tot) : 0.f;
          }
        } else {
          act_c = gauss_head_action<NA, kDet>(y, zt, eacc);
        }

        mark(3, DISC ? (float)act_d : act_c);
        // ---- env step ----
        if constexpr (ENV == FDR_ENV_SYNTH) {
          if constexpr (kCand) {
            s = cand[0];
    #pragma unroll
            for (int i = 1; i < NA; ++i) s = act_d == i ? cand[i] : s;
          } else {
            if constexpr (DISC) {
              pre += mrow[NX + act_d];
            } else {
              float kr[NA];
    #pragma unroll
              for (int m = 0; m < NA; ++m) kr[m] = WIDE ? kreg[m] : mrow[NX + m];
              dpp_tail<NA>(pre, act_c, kr);  // a[m] sits in lane m of every row
            }
            s = tanh_fast(pre);
          }
          racc += (double)s;  // lane 0 holds the reward s'[0]; other lanes' sums are discarded
          if constexpr (kTerm) {  // done after this step: the reward and entropy of step t count (agent.py:46-52)
            if (fabsf(readlane_f(s, a.done_dim)) > a.done_thr) {
              nsteps = t + 1;
              return;
            }
          }
        } else if constexpr (kPhysics) {
          if (sim.step(j, act_d, act_c, racc, s)) {
            nsteps = t + 1;
            return;
          }
        } else {
          static_assert(ENV == FDR_ENV_TRAP, "unknown env kind");
          // custom_envs/simple_trap_env: node.py:9-14, tile_map.py:11-23, environment.py:33-48
          const int prev_x = col * 7;
          const int tc = col + act_d / 3 - 1, tr = row + act_d % 3 - 1;
          if (tc >= 0 && tc < a.map_w && tr >= 0 && tr < a.map_h && a.walkable[tr * a.map_w + tc]) {
            col = tc;
            row = tr;
          }
          racc += (double)(col * 7 - prev_x);
          s = trap_obs(j, col, row);
        }
        mark(4, s);
      }
    }
  };
  if (det)
    episode(std::true_type{});
  else
    episode(std::false_type{});
#ifdef FDR_PHASE_STAMPS
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int k = 0; k < 5; ++k) g_phase_stamps[k] = ph_acc[k];
#endif

  // ---- epilogue ----
  store_results<DISC>(a, lane, j, ulane, racc, entropy_sum(eacc, j, NA), nsteps, NA);
  if constexpr (FEAT & kFeatObsStats) {
    if (j < NIN) {
      a.os_mean[(int64_t)lane * NIN + j] = os_mean;
      a.os_m2[(int64_t)lane * NIN + j] = os_m2;
    }
    if (j == 0) a.os_count[lane] = os_n;
  }
}

// Launch the rollout_kernel<S, ENV, feat, WIDE> instance of a family (BITS: its legal feature sets) over all lanes.
// feat outside the family: nothing is launched, FDR_ERR_UNSUPPORTED with none_msg.
template <class S, int ENV, bool WIDE, int BITS>
int launch_rollout_kernel(const RolloutArgs& args, int feat, hipStream_t stream, const char* what,
                          const char* none_msg) {
  const dim3 grid((args.n_lanes + kLanesPerBlock - 1) / kLanesPerBlock), block(64 * kLanesPerBlock);
  FDR_PHASE_UNIT();
  const bool hit = launch_feat_set<BITS>(feat, [&](auto f) {
    hipLaunchKernelGGL((rollout_kernel<S::NIN, S::NA, S::DISC, ENV, decltype(f)::value, WIDE>), grid, block, 0, stream,
                       args);
  });
  return hit ? check_launch(what) : set_error(FDR_ERR_UNSUPPORTED, none_msg);
}

}  // namespace fdr
