// fdr_rollout_parts.h -- the device pieces rollout_kernel (fdr_rollout_kernel.h) and rollout_episodes_kernel share:
// the five classic-control systems (PhysicsSim<ENV>: reset draws, observation, step with its reward and termination
// order) and the lane frame; rollout_dyn_kernel (fdr_rollout_dyn.hip) takes the pieces without a compile-time shape.
// Every helper is force-inlined, takes no flag that names its caller and adds no runtime branch.
#pragma once
#include "fdr_mlp_lane.h"

namespace fdr {

// ---- classic-control physics envs (gym classic_control cartpole.py / pendulum.py / acrobot.py / mountain_car.py /
// continuous_mountain_car.py in f32) ----
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

// One lane's physics env (a PhysicsSpec kind, fdr_internal.h), wave-uniform: CartPole (x, xdot, theta, thetadot);
// Pendulum (theta, thetadot, cos, sin); Acrobot (theta1, theta2, thetadot1, thetadot2); MountainCars (pos, velocity).
template <int ENV>
struct PhysicsSim {
  float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
  __device__ __forceinline__ void reset(uint64_t key, uint64_t ulane) {
    if constexpr (ENV == FDR_ENV_CARTPOLE) {  // gym: U(-0.05, 0.05) on all four
      p0 = physics_reset(key, ulane, 0, 0.1f, 0.05f);
      p1 = physics_reset(key, ulane, 1, 0.1f, 0.05f);
      p2 = physics_reset(key, ulane, 2, 0.1f, 0.05f);
      p3 = physics_reset(key, ulane, 3, 0.1f, 0.05f);
    } else if constexpr (ENV == FDR_ENV_PENDULUM) {  // gym: theta ~ U(-pi, pi), thetadot ~ U(-1, 1)
      p0 = physics_reset(key, ulane, 0, kTwoPiF, kPiF);
      p1 = physics_reset(key, ulane, 1, 2.f, 1.f);
      p2 = cosf(p0);
      p3 = sinf(p0);
    } else if constexpr (ENV == FDR_ENV_ACROBOT) {  // gym: U(-0.1, 0.1) on all four
      p0 = physics_reset(key, ulane, 0, 0.2f, 0.1f);
      p1 = physics_reset(key, ulane, 1, 0.2f, 0.1f);
      p2 = physics_reset(key, ulane, 2, 0.2f, 0.1f);
      p3 = physics_reset(key, ulane, 3, 0.2f, 0.1f);
    } else {  // both MountainCars, gym: position ~ U(-0.6, -0.4), at rest
      static_assert(ENV == FDR_ENV_MOUNTAINCAR || ENV == FDR_ENV_MOUNTAINCAR_CONT, "not a physics env");
      p0 = physics_reset(key, ulane, 0, 0.2f, 0.6f);
      p1 = p2 = p3 = 0.f;
    }
  }
  // observation element j: thread j < NIN selects it into the kernel's s; everything downstream of s runs unchanged
  __device__ __forceinline__ float obs(int j) const {
    if constexpr (ENV == FDR_ENV_CARTPOLE) return j == 0 ? p0 : (j == 1 ? p1 : (j == 2 ? p2 : p3));
    else if constexpr (ENV == FDR_ENV_ACROBOT) return acrobot_obs(j, p0, p1, p2, p3);
    else if constexpr (ENV == FDR_ENV_MOUNTAINCAR || ENV == FDR_ENV_MOUNTAINCAR_CONT) return j == 0 ? p0 : p1;
    else return j == 0 ? p2 : (j == 1 ? p3 : p1);
  }

  // One env.step under act_d, or act_c (unscaled, in lane 0 of every row): the reward joins racc, s becomes the new
  // observation.  True (wave-uniform: the whole wave leaves its loop): done after this step (agent.py:46-52).
  __device__ __forceinline__ bool step(int j, int act_d, float act_c, double& racc, float& s) {
    bool done = false;
    if constexpr (ENV == FDR_ENV_CARTPOLE) {
      // reward 1 for every step taken, the failing one included
      done = cartpole_step(p0, p1, p2, p3, act_d);
      racc += 1.0;
      s = obs(j);
    } else if constexpr (ENV == FDR_ENV_PENDULUM) {  // never done
      racc += (double)pendulum_step(p0, p1, p2, p3, readlane_f(act_c, 0));
      s = obs(j);
      return false;
    } else if constexpr (ENV == FDR_ENV_ACROBOT) {
      // reward -1 per step, 0 on the step that reaches the goal
      done = acrobot_step(p0, p1, p2, p3, act_d);
      s = obs(j);
      if (__builtin_amdgcn_readfirstlane(done ? 1 : 0)) return true;
      racc -= 1.0;
      return false;
    } else if constexpr (ENV == FDR_ENV_MOUNTAINCAR) {
      // reward -1 for every step taken, the one that reaches the goal included
      done = mountaincar_step(p0, p1, (float)(act_d - 1) * 0.001f, 0.5f);
      racc -= 1.0;
      s = obs(j);
    } else {
      // the force is the clamped action; the cost is the unclipped one's (gym), +100 on reaching the goal
      const float ac = readlane_f(act_c, 0);
      done = mountaincar_step(p0, p1, fminf(fmaxf(ac, -1.f), 1.f) * 0.0015f, 0.45f);
      racc += (double)((done ? 100.f : 0.f) - 0.1f * ac * ac);
      s = obs(j);
    }
    return __builtin_amdgcn_readfirstlane(done ? 1 : 0) != 0;
  }
};

// ---- pieces that depend on no compile-time shape ----
// The lane's squared perturbation norm, written before the step loop: a double live across it would be spilled (and
// the asm keeps the compiler from sinking the norm past the loop with every element's sigma * eps in scratch).
__device__ __forceinline__ void write_norm2(const RolloutArgs& a, int lane, int j, double src_n2) {
  double n2 = wave_sum(src_n2);
  asm volatile("" : "+v"(n2));
  if (j == 0 && a.norm2) a.norm2[lane] = n2;
}

// worker/agent.py:37-39: with probability obs_stats_update_chance the raw obs enters the lane's WelfordRunningStat
// (utils/math_helpers.py:29-38, f32, same operation order, no contraction).  Thread j holds observation element j.
struct ObsWelford {
  uint64_t mask = 0;  // coins of the current 64-step batch (wave-uniform)
  int n = 0;
  float mean = 0.f, m2 = 0.f;

  // step t of stream ulane sees s; coins come 64 steps at a time: lane i draws step t + i (counter k = 14), one ballot
  __device__ __forceinline__ void visit(const RolloutArgs& a, uint64_t ulane, int t, int j, float s) {
    if ((t & 63) == 0) {
      const float u = uniform24(hash_ctr(a.key, ulane, (uint64_t)(t + j), 14));
      mask = __ballot(u < a.os_chance);
    }
    if ((mask >> (t & 63)) & 1ull) {
#pragma clang fp contract(off)
      const int cc = n;
      n += 1;
      const float delta = s - mean;
      const float delta_n = delta / (float)n;
      mean += delta_n;
      m2 += (delta * delta_n) * (float)cc;
    }
  }
  __device__ __forceinline__ void store(const RolloutArgs& a, int lane, int n_in, int j) const {
    if (j < n_in) {
      a.os_mean[(int64_t)lane * n_in + j] = mean;
      a.os_m2[(int64_t)lane * n_in + j] = m2;
    }
    if (j == 0) a.os_count[lane] = n;
  }
};

// The lane's entropy sum in nats from the threads' log2 sums (threads j >= n_act hold no term)
__device__ __forceinline__ double entropy_sum(float eacc, int j, int n_act) {
  eacc *= 0.693147180559945309f;  // log2 -> ln (both kinds)
  return wave_sum((j < n_act) ? (double)eacc : 0.0);
}

// Thread 0's stores: r with its jiggle (keyed by jlane), esum as the mean over nsteps states (agent.py:60-65), nsteps
template <bool DISC>
__device__ __forceinline__ void store_results(const RolloutArgs& a, int lane, int j, uint64_t jlane, double r,
                                              double esum, int nsteps, int n_act) {
  if (j == 0) {
    if (a.jiggle) r += (hash_ctr(a.key, jlane, kJiggleT, 15) & 1ull) ? 1e-12 : -1e-12;
    a.ret[lane] = r;
    double e = esum / (double)nsteps;
    if constexpr (!DISC) e += (double)n_act * 1.4189385332046727;  // 0.5 + 0.5*ln(2*pi) per dim
    a.ent[lane] = e;
    a.steps[lane] = nsteps;
  }
}

// ---- the lane frame of rollout_kernel and rollout_episodes_kernel (compile-time shape) ----
// rollout_kernel keeps its own text of lane_prologue, DrawBatch, select_action and (as rollout_dyn_kernel) ObsWelford:
// called there they change instances that are to stay instruction for instruction what they were.
// Lane `lane`'s theta' into pl and its norm2 out; returns the lane's deterministic flag.
template <class Lane>
__device__ __forceinline__ bool lane_prologue(const RolloutArgs& a, int lane, int j, float4* tile, Lane& pl) {
  ParamSrc src = a.lanes.src(lane);
  const bool det = a.lanes.deterministic ? a.lanes.deterministic[lane] != 0 : false;
  pl.load(src, j, a.bn_mean, a.bn_var, tile);
  write_norm2(a, lane, j, src.n2);
  return det;
}

// The policy's input from a raw observation element: normalised and clipped when NORM (agent.py:40-41), then the
// policy's own input transform.
template <bool NORM>
struct ObsInput {
  float om = 0.f, osd = 1.f;
  __device__ __forceinline__ ObsInput(const RolloutArgs& a, int ji) {
    if constexpr (NORM) {
      om = a.obs_mean[ji];
      osd = a.obs_std[ji];
    }
  }
  template <class Lane>
  __device__ __forceinline__ float operator()(const Lane& pl, float s) const {
    float x = s;
    if constexpr (NORM) x = fminf(fmaxf((s - om) / osd, -10.f), 10.f);
    return pl.input_transform(x);
  }
};

// rollout_kernel's draw batches: one counter hash per thread covers up to 64 future draws.
template <int NA, bool DISC>
struct DrawBatch {
  static constexpr int kDrawsPerStep = DISC ? 1 : NA;
  static constexpr int kStepsPerBatch = 64 / kDrawsPerStep;
  float rbuf = 0.f;

  // the batch that starts at step t (thread-parallel)
  __device__ __forceinline__ void draw(uint64_t key, uint64_t ulane, int t, int j) {
    const int ds = j / kDrawsPerStep, dk = j % kDrawsPerStep;
    const uint64_t h = hash_ctr(key, ulane, (uint64_t)(t + ds), (uint64_t)dk);
    rbuf = DISC ? uniform24(h) : normal_bm(h);
  }
  // continuous: the normal of step t for the thread's action dim j & 15
  __device__ __forceinline__ float z(int t, int j) const {
    if constexpr (DISC) return 0.f;
    const int o = j & 15;
    const int zbase = 4 * (o < NA ? o : 0);  // ds_bpermute byte address of dim o in step 0 of a batch
    const int addr = zbase + 4 * NA * (t % kStepsPerBatch);
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addr, __builtin_bit_cast(int, rbuf)));
  }
  // discrete: the uniform of step tb of the batch (wave-uniform)
  __device__ __forceinline__ float u(int tb) const { return readlane_f(rbuf, tb); }
};

// rollout_kernel's generic discrete selection from the softmax p (p_i in thread i of every row), branch-free: argmax
// when kDet, else the inverse CDF at the batch's uniform of step tb.  The step's entropy term leaves eacc.
template <int NA, bool kDet, class Draws>
__device__ __forceinline__ int select_action(float p, const Draws& draws, int tb, int j, float& eacc) {
  int act_d = 0;
  float pv[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) pv[i] = readlane_f(p, i);
  float tot = pv[0];  // sequential f32 cumsum, the oracle's order (0 + p0 == p0)
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
    const float target = draws.u(tb) * tot;
    float c = 0.f;
#pragma unroll
    for (int i = 0; i < NA - 1; ++i) {
      c += pv[i];
      act_d += c <= target ? 1 : 0;
    }
  }
  eacc -= (j < NA) ? disc_entropy_term(p, tot) : 0.f;
  return act_d;
}

// Continuous action from the head's y (mean in thread o, std's in thread o + NA): mean, or mean + std zt; log2 std
// joins eacc (threads >= NA and the ln 2 scale: entropy_sum).
template <int NA, bool kDet>
__device__ __forceinline__ float gauss_head_action(float y, float zt, float& eacc) {
  const float th = tanh_fast(y);
  const float sd = std_from_tanh(dpp_mov<kDppRowShl + NA>(th));
  eacc += __builtin_amdgcn_logf(sd);
  return kDet ? th : gauss_action(th, sd, zt);
}

}  // namespace fdr
