// fdr_rollout_kernel.h -- the one-lane-per-wave rollout_kernel template with the envs it steps (the synthetic
// linear-tanh system, the trap gridworld, gym's five classic-control systems).  Instantiated by fdr_rollout_lane.hip
// (synthetic env), fdr_rollout_wide.hip (WIDE) and fdr_rollout_env.hip (trap, CartPole, Pendulum, Acrobot, MountainCar,
// MountainCarContinuous).
#pragma once
#include "fdr_mlp_lane.h"

namespace fdr {

// trap-env observation (environment.py:59-61): python f64 division, cast to f32 by the policy
__device__ __forceinline__ float trap_obs(int j, int col, int row) {
  return j == 0 ? (float)((double)(col * 7) / 1918.0) : (float)((double)(row * 7) / 1071.0);
}

// ---- classic-control physics envs (gym classic_control cartpole.py / pendulum.py / acrobot.py / mountain_car.py /
// continuous_mountain_car.py in f32) ----
// The state is a few scalars every thread of the wave holds identically (as the trap env's col / row).
constexpr float kPiF = 3.14159274101257324f;     // fl32(pi)
constexpr float kTwoPiF = 6.28318548202514648f;  // fl32(2 pi)
// Reset draw i of a lane: the reserved counter slot t = kJiggleT, k = i (k = 15 there is the jiggle's; action draws
// have t < 10000), scaled to gym's uniform range as fl32(fl32(scale * u) - shift) -- no contraction: compared bitwise.
__device__ __forceinline__ float physics_reset(uint64_t key, uint64_t ulane, int i, float scale, float shift) {
#pragma clang fp contract(off)
  const float v = scale * uniform24(hash_ctr(key, ulane, kJiggleT, (uint64_t)i));
  return v - shift;
}
// ((th + pi) mod 2 pi) - pi, floor-mod
__device__ __forceinline__ float wrap_pi(float th) {
  const float y = th + kPiF;
  return (y - kTwoPiF * floorf(y * (1.0f / kTwoPiF))) - kPiF;
}
// CartPole-v1, explicit Euler (positions advance with the old velocities); returns the failure test of the new state
__device__ __forceinline__ bool cartpole_step(float& x, float& xd, float& th, float& thd, int act) {
  const float force = act == 1 ? 10.f : -10.f;
  const float sn = sinf(th), cs = cosf(th);
  const float temp = (force + 0.05f * thd * thd * sn) / 1.1f;
  const float thacc = (9.8f * sn - cs * temp) / (0.5f * (4.0f / 3.0f - 0.1f * cs * cs / 1.1f));
  const float xacc = temp - 0.05f * thacc * cs / 1.1f;
  x += 0.02f * xd;
  xd += 0.02f * xacc;
  th += 0.02f * thd;
  thd += 0.02f * thacc;
  constexpr float kThetaThr = 0.20943951023931953f;  // 12 * 2 pi / 360
  return x < -2.4f || x > 2.4f || th < -kThetaThr || th > kThetaThr;
}
// Pendulum-v1 (g = 10, m = l = 1, dt = 0.05): sn = sin(th) on entry; th is kept wrapped, (cs, sn) follow it.
// Returns the reward -cost of the pre-step state.
__device__ __forceinline__ float pendulum_step(float& th, float& thd, float& cs, float& sn, float a) {
  const float u = fminf(fmaxf(a, -2.f), 2.f);
  const float w = wrap_pi(th);
  const float cost = w * w + 0.1f * thd * thd + 0.001f * u * u;
  thd = fminf(fmaxf(thd + (15.f * sn + 3.f * u) * 0.05f, -8.f), 8.f);
  th = wrap_pi(th + thd * 0.05f);
  cs = cosf(th);
  sn = sinf(th);
  return -cost;
}
// Acrobot-v1 ("book" dynamics: m1 = m2 = l1 = I1 = I2 = 1, lc1 = lc2 = 0.5, g = 9.8, no torque noise): the
// accelerations of (th1, th2) at velocities (d1, d2) under torque tq.  gym's cos(. - pi / 2) is taken as the sine.
__device__ __forceinline__ void acrobot_dsdt(float th1, float th2, float d1, float d2, float tq, float& a1, float& a2) {
  float sn2, cs2;
  sincosf(th2, &sn2, &cs2);
  const float dd1 = 0.25f + (1.25f + cs2) + 2.f;  // m1 lc1^2 + m2 (l1^2 + lc2^2 + 2 l1 lc2 cos th2) + I1 + I2
  const float dd2 = (0.25f + 0.5f * cs2) + 1.f;   // m2 (lc2^2 + l1 lc2 cos th2) + I2
  const float phi2 = 4.9f * sinf(th1 + th2);
  const float phi1 = -0.5f * d2 * d2 * sn2 - d2 * d1 * sn2 + 14.7f * sinf(th1) + phi2;
  a2 = (tq + dd2 / dd1 * phi1 - 0.5f * d1 * d1 * sn2 - phi2) / (1.25f - dd2 * dd2 / dd1);
  a1 = -(dd2 * a2 + phi1) / dd1;
}
// one classical RK4 step over [0, 0.2], then gym's wrap of the angles (one conditional 2 pi: |thd| dt < 2 pi) and
// clamp of the velocities; returns the success test of the new state (the free end above the bar by one link)
__device__ __forceinline__ bool acrobot_step(float& th1, float& th2, float& d1, float& d2, int act) {
  const float tq = (float)(act - 1);
  constexpr float h = 0.2f, h2 = 0.1f, h6 = 0.2f / 6.0f;
  float k1a, k1b, k2a, k2b, k3a, k3b, k4a, k4b;
  acrobot_dsdt(th1, th2, d1, d2, tq, k1a, k1b);
  const float u1 = d1 + h2 * k1a, u2 = d2 + h2 * k1b;  // the stages' velocities: the angles' derivatives
  acrobot_dsdt(th1 + h2 * d1, th2 + h2 * d2, u1, u2, tq, k2a, k2b);
  const float v1 = d1 + h2 * k2a, v2 = d2 + h2 * k2b;
  acrobot_dsdt(th1 + h2 * u1, th2 + h2 * u2, v1, v2, tq, k3a, k3b);
  const float w1 = d1 + h * k3a, w2 = d2 + h * k3b;
  acrobot_dsdt(th1 + h * v1, th2 + h * v2, w1, w2, tq, k4a, k4b);
  th1 += h6 * (d1 + 2.f * u1 + 2.f * v1 + w1);
  th2 += h6 * (d2 + 2.f * u2 + 2.f * v2 + w2);
  d1 += h6 * (k1a + 2.f * k2a + 2.f * k3a + k4a);
  d2 += h6 * (k1b + 2.f * k2b + 2.f * k3b + k4b);
  th1 = th1 > kPiF ? th1 - kTwoPiF : (th1 < -kPiF ? th1 + kTwoPiF : th1);
  th2 = th2 > kPiF ? th2 - kTwoPiF : (th2 < -kPiF ? th2 + kTwoPiF : th2);
  d1 = fminf(fmaxf(d1, -4.f * kPiF), 4.f * kPiF);
  d2 = fminf(fmaxf(d2, -9.f * kPiF), 9.f * kPiF);
  return -cosf(th1) - cosf(th1 + th2) > 1.f;
}
// observation element j of (cos th1, sin th1, cos th2, sin th2, thd1, thd2)
__device__ __forceinline__ float acrobot_obs(int j, float th1, float th2, float d1, float d2) {
  float sn, cs;
  sincosf(j < 2 ? th1 : th2, &sn, &cs);
  return j < 4 ? ((j & 1) ? sn : cs) : (j == 4 ? d1 : d2);
}
// MountainCar-v0 / MountainCarContinuous-v0: force * power already formed (discrete (a - 1) 0.001, continuous
// clamp(a, +-1) 0.0015), goal 0.5 / 0.45; the car stops at the left wall.  Returns the success test of the new state.
__device__ __forceinline__ bool mountaincar_step(float& pos, float& vel, float push, float goal) {
  vel = fminf(fmaxf(vel + push - 0.0025f * cosf(3.f * pos), -0.07f), 0.07f);
  pos = fminf(fmaxf(pos + vel, -1.2f), 0.6f);
  if (pos == -1.2f && vel < 0.f) vel = 0.f;
  return pos >= goal && vel >= 0.f;
}

// ---------------------------------------------------------------------------------------------
// Whole-episode rollout: fdr_rollout
// ---------------------------------------------------------------------------------------------
// FEAT (fdr_mlp.h): kFeatStates: record visited observations (fdr_rollout_states); kFeatObsStats: Welford obs
// statistics; kFeatObsNorm: observation normalisation (obs_mean / obs_std given); kFeatInject: host-injected draws
// (u_inject); kFeatTerm: terminating synthetic env (fdr_env_desc.done_threshold): the lane's episode ends after the
// step whose next state has |s'[done_dim]| > done_threshold (worker/agent.py:50-52: done -> break), or at T
// (one lane per wave: the wave leaves its loop -- only these instances carry the test)
// ENV: FDR_ENV_SYNTH, FDR_ENV_TRAP, or a physics env (FDR_ENV_CARTPOLE at (4, 2, discrete), FDR_ENV_PENDULUM at
// (3, 1, continuous), FDR_ENV_ACROBOT at (6, 3, discrete), FDR_ENV_MOUNTAINCAR at (2, 3, discrete),
// FDR_ENV_MOUNTAINCAR_CONT at (2, 1, continuous); !WIDE only) -- per-lane reset states from the counter stream, each
// env's termination test in its own branch (not kFeatTerm).
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
  const float om = norm_obs ? a.obs_mean[ji] : 0.f;
  const float osd = norm_obs ? a.obs_std[ji] : 1.f;
  auto policy_input = [&](float s) {
    float x = s;
    if (norm_obs) x = fminf(fmaxf((s - om) / osd, -10.f), 10.f);  // agent.py:40-41
    return pl.input_transform(x);
  };

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
  // physics env state (wave-uniform): CartPole (x, xdot, theta, thetadot); Pendulum (theta, thetadot, cos, sin);
  // Acrobot (theta1, theta2, thetadot1, thetadot2); both MountainCars (position, velocity).
  // Thread j < NIN selects observation element j into s, so everything downstream of s runs unchanged.
  float px0 = 0.f, px1 = 0.f, px2 = 0.f, px3 = 0.f;
  auto physics_obs = [&]() {
    if constexpr (ENV == FDR_ENV_CARTPOLE) return j == 0 ? px0 : (j == 1 ? px1 : (j == 2 ? px2 : px3));
    else if constexpr (ENV == FDR_ENV_ACROBOT) return acrobot_obs(j, px0, px1, px2, px3);
    else if constexpr (ENV == FDR_ENV_MOUNTAINCAR || ENV == FDR_ENV_MOUNTAINCAR_CONT) return j == 0 ? px0 : px1;
    else return j == 0 ? px2 : (j == 1 ? px3 : px1);
  };
  (void)physics_obs;
  if constexpr (ENV == FDR_ENV_CARTPOLE) {  // gym: U(-0.05, 0.05) on all four
    static_assert(NIN == 4 && NA == 2 && DISC && !WIDE, "CartPole: DiscretePolicy(4, 2), one-lane kernel");
    px0 = physics_reset(key, ulane, 0, 0.1f, 0.05f);
    px1 = physics_reset(key, ulane, 1, 0.1f, 0.05f);
    px2 = physics_reset(key, ulane, 2, 0.1f, 0.05f);
    px3 = physics_reset(key, ulane, 3, 0.1f, 0.05f);
    s = physics_obs();
  } else if constexpr (ENV == FDR_ENV_PENDULUM) {  // gym: theta ~ U(-pi, pi), thetadot ~ U(-1, 1)
    static_assert(NIN == 3 && NA == 1 && !DISC && !WIDE, "Pendulum: MujocoPolicy(3, 1), one-lane kernel");
    px0 = physics_reset(key, ulane, 0, kTwoPiF, kPiF);
    px1 = physics_reset(key, ulane, 1, 2.f, 1.f);
    px2 = cosf(px0);
    px3 = sinf(px0);
    s = physics_obs();
  } else if constexpr (ENV == FDR_ENV_ACROBOT) {  // gym: U(-0.1, 0.1) on all four
    static_assert(NIN == 6 && NA == 3 && DISC && !WIDE, "Acrobot: DiscretePolicy(6, 3), one-lane kernel");
    px0 = physics_reset(key, ulane, 0, 0.2f, 0.1f);
    px1 = physics_reset(key, ulane, 1, 0.2f, 0.1f);
    px2 = physics_reset(key, ulane, 2, 0.2f, 0.1f);
    px3 = physics_reset(key, ulane, 3, 0.2f, 0.1f);
    s = physics_obs();
  } else if constexpr (ENV == FDR_ENV_MOUNTAINCAR) {  // gym: position ~ U(-0.6, -0.4), at rest
    static_assert(NIN == 2 && NA == 3 && DISC && !WIDE, "MountainCar: DiscretePolicy(2, 3), one-lane kernel");
    px0 = physics_reset(key, ulane, 0, 0.2f, 0.6f);
    s = physics_obs();
  } else if constexpr (ENV == FDR_ENV_MOUNTAINCAR_CONT) {
    static_assert(NIN == 2 && NA == 1 && !DISC && !WIDE, "MountainCarContinuous: MujocoPolicy(2, 1), one-lane kernel");
    px0 = physics_reset(key, ulane, 0, 0.2f, 0.6f);
    s = physics_obs();
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
          const float th = tanh_fast(y);
          const float sd = std_from_tanh(dpp_mov<kDppRowShl + NA>(th));
          eacc += __builtin_amdgcn_logf(sd);  // log2; lanes >= NA and the ln 2 scale: epilogue
          act_c = kDet ? th : gauss_action(th, sd, zt);
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
        } else if constexpr (ENV == FDR_ENV_CARTPOLE) {
          // reward 1 for every step taken, the failing one included; done after it (agent.py:46-52), or at T
          const bool fail = cartpole_step(px0, px1, px2, px3, act_d);
          racc += 1.0;
          s = physics_obs();
          if (__builtin_amdgcn_readfirstlane(fail ? 1 : 0)) {  // wave-uniform: the whole wave leaves its loop
            nsteps = t + 1;
            return;
          }
        } else if constexpr (ENV == FDR_ENV_PENDULUM) {
          // the action (mean, or mean + std z, unscaled) sits in lane 0 of every row
          racc += (double)pendulum_step(px0, px1, px2, px3, readlane_f(act_c, 0));
          s = physics_obs();
        } else if constexpr (ENV == FDR_ENV_ACROBOT) {
          // reward -1 per step, 0 on the step that reaches the goal; done after it, or at T
          const bool done = acrobot_step(px0, px1, px2, px3, act_d);
          s = physics_obs();
          if (__builtin_amdgcn_readfirstlane(done ? 1 : 0)) {
            nsteps = t + 1;
            return;
          }
          racc -= 1.0;
        } else if constexpr (ENV == FDR_ENV_MOUNTAINCAR) {
          // reward -1 for every step taken, the one that reaches the goal included
          const bool done = mountaincar_step(px0, px1, (float)(act_d - 1) * 0.001f, 0.5f);
          racc -= 1.0;
          s = physics_obs();
          if (__builtin_amdgcn_readfirstlane(done ? 1 : 0)) {
            nsteps = t + 1;
            return;
          }
        } else if constexpr (ENV == FDR_ENV_MOUNTAINCAR_CONT) {
          // the force is the clamped action; the cost is the unclipped one's (gym), +100 on reaching the goal
          const float ac = readlane_f(act_c, 0);
          const bool done = mountaincar_step(px0, px1, fminf(fmaxf(ac, -1.f), 1.f) * 0.0015f, 0.45f);
          racc += (double)((done ? 100.f : 0.f) - 0.1f * ac * ac);
          s = physics_obs();
          if (__builtin_amdgcn_readfirstlane(done ? 1 : 0)) {
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
  eacc *= 0.693147180559945309f;  // log2 -> ln (both kinds)
  const double esum = wave_sum((j < NA) ? (double)eacc : 0.0);
  if (j == 0) {
    double r = racc;
    if (a.jiggle) r += (hash_ctr(key, ulane, kJiggleT, 15) & 1ull) ? 1e-12 : -1e-12;
    a.ret[lane] = r;
    double e = esum / (double)nsteps;  // mean over the visited states (agent.py:60-65)
    if constexpr (!DISC) e += (double)NA * 1.4189385332046727;  // 0.5 + 0.5*ln(2*pi) per dim
    a.ent[lane] = e;
    a.steps[lane] = nsteps;
  }
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
