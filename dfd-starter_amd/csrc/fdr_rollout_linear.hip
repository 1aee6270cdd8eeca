// fdr_rollout_linear.hip -- FDR_POLICY_LINEAR: y = W' x, W' [n_act, n_in] row-major, no bias (the policy of Augmented
// Random Search).  A lane's theta' is at most 18 floats on the five physics envs, so one THREAD runs one lane:
// rollout_linear_kernel holds theta' in registers, loops over the lane's K episodes and their steps and calls the free
// per-thread step functions of fdr_rollout_parts.h.  No LDS, no barrier, no cross-lane traffic but the ballot that lets
// a wave leave the step loop once all its threads are done.  policy_forward_linear_kernel is the runtime-shaped forward
// (fdr_policy_forward), one lane per thread too.  DESIGN.md 3.1.3.
#include "fdr_rollout_parts.h"

namespace fdr {

constexpr int kLinearBlock = 256;  // threads = lanes per workgroup
constexpr int kLinearMaxIn = 64, kLinearMaxAct = 16;  // policy_forward_linear_kernel's limits

// Row i of W' against x in ascending j, every product and sum rounded to f32: (((w0 x0) + w1 x1) + ...)
template <int NIN>
__device__ __forceinline__ float linear_row(const float* w, const float* x) {
#pragma clang fp contract(off)
  float acc = w[0] * x[0];
#pragma unroll
  for (int j = 1; j < NIN; ++j) {
    const float p = w[j] * x[j];
    acc = acc + p;
  }
  return acc;
}

// One thread's physics env: PhysicsSim's reset draws and state, the observation as NIN registers and the step with its
// reward and termination order under a per-thread action (PhysicsSim::step is wave-uniform).
template <int ENV>
struct LinearSim {
  PhysicsSim<ENV> sim;
  static constexpr int NIN = PhysicsSpec<ENV>::NIN;

  __device__ __forceinline__ void obs(float* s) const {
    if constexpr (ENV == FDR_ENV_ACROBOT) {  // acrobot_obs's values, one sincosf per angle
      sincosf(sim.p0, &s[1], &s[0]);
      sincosf(sim.p1, &s[3], &s[2]);
      s[4] = sim.p2;
      s[5] = sim.p3;
    } else {
#pragma unroll
      for (int j = 0; j < NIN; ++j) s[j] = sim.obs(j);
    }
  }
  // true: done after this step
  __device__ __forceinline__ bool step(const float* y, double& racc) {
    float &p0 = sim.p0, &p1 = sim.p1, &p2 = sim.p2, &p3 = sim.p3;
    int act = 0;
    if constexpr (PhysicsSpec<ENV>::DISC) {  // the smallest index attaining the maximum (select_action<kDet>'s scan)
      float best = y[0];
#pragma unroll
      for (int i = 1; i < PhysicsSpec<ENV>::NA; ++i) {
        act = y[i] > best ? i : act;
        best = fmaxf(best, y[i]);
      }
    }
    if constexpr (ENV == FDR_ENV_CARTPOLE) {
      const bool done = cartpole_step(p0, p1, p2, p3, act);
      racc += 1.0;
      return done;
    } else if constexpr (ENV == FDR_ENV_PENDULUM) {
      racc += (double)pendulum_step(p0, p1, p2, p3, y[0]);
      return false;
    } else if constexpr (ENV == FDR_ENV_ACROBOT) {
      const bool done = acrobot_step(p0, p1, p2, p3, act);
      if (!done) racc -= 1.0;
      return done;
    } else if constexpr (ENV == FDR_ENV_MOUNTAINCAR) {
      const bool done = mountaincar_step(p0, p1, (float)(act - 1) * 0.001f, 0.5f);
      racc -= 1.0;
      return done;
    } else {
      const float ac = y[0];
      const bool done = mountaincar_step(p0, p1, fminf(fmaxf(ac, -1.f), 1.f) * 0.0015f, 0.45f);
      racc += (double)((done ? 100.f : 0.f) - 0.1f * ac * ac);
      return done;
    }
  }
};

// FEAT: a subset of kFeatStates | kFeatObsStats | kFeatObsNorm; kFeatStates with one episode per lane only.
template <int ENV, int FEAT>
__global__ __launch_bounds__(kLinearBlock) void rollout_linear_kernel(EpisodesArgs ea) {
  using E = PhysicsSpec<ENV>;
  constexpr int NIN = E::NIN, NA = E::NA, P = NIN * NA;
  const RolloutArgs& a = ea.r;
  const int lane = blockIdx.x * kLinearBlock + threadIdx.x;
  if (lane >= a.n_lanes) return;

  // theta' and the lane's norm2 (f64, ascending p); an out-of-range offset never reaches the table (LanesArgs::src)
  ParamSrc src = a.lanes.src(lane);
  float w[P];
#pragma unroll
  for (int p = 0; p < P; ++p) w[p] = src.get(p);
  if (a.norm2) a.norm2[lane] = src.n2;

  [[maybe_unused]] float om[NIN], osd[NIN];
  if constexpr (FEAT & kFeatObsNorm) {
#pragma unroll
    for (int j = 0; j < NIN; ++j) {
      om[j] = a.obs_mean[j];
      osd[j] = a.obs_std[j];
    }
  }

  const int T = a.T, K = ea.n_episodes;
  const uint64_t key = a.key;
  const uint64_t glane = (uint64_t)(a.lanes.lane_offset + lane);  // physical global lane: the jiggle's key
  double rsum = 0.0, rsq = 0.0;
  int nsum = 0;
  // the lane's Welford statistic, running on across its episodes (ObsWelford's arithmetic per element)
  [[maybe_unused]] int os_n = 0;
  [[maybe_unused]] float os_mean[NIN], os_m2[NIN];
#pragma unroll
  for (int j = 0; j < NIN; ++j) os_mean[j] = os_m2[j] = 0.f;

  for (int ep = 0; ep < K; ++ep) {
    const uint64_t ulane =
        ea.episode_ids ? (uint64_t)ea.episode_ids[(int64_t)lane * K + ep] : glane * (uint64_t)K + (uint64_t)ep;
    LinearSim<ENV> env;
    env.sim.reset(key, ulane);
    double racc = 0.0;
    int nsteps = T;
    bool done = false;
    for (int t = 0; t < T; ++t) {
      if (!done) {  // a finished thread adds nothing and stores nothing more
        float s[NIN];
        env.obs(s);
        if constexpr (FEAT & kFeatStates) {
#pragma unroll
          for (int j = 0; j < NIN; ++j) a.states[((int64_t)lane * T + t) * NIN + j] = s[j];
        }
        if constexpr (FEAT & kFeatObsStats) {
          // the coin of step t of stream ulane: the one the wave-per-lane kernels draw 64 steps at a time
          if (uniform24(hash_ctr(key, ulane, (uint64_t)t, 14)) < a.os_chance) {
#pragma clang fp contract(off)
            const int cc = os_n;
            os_n += 1;
#pragma unroll
            for (int j = 0; j < NIN; ++j) {
              const float delta = s[j] - os_mean[j];
              const float delta_n = delta / (float)os_n;
              os_mean[j] += delta_n;
              os_m2[j] += (delta * delta_n) * (float)cc;
            }
          }
        }
        if constexpr (FEAT & kFeatObsNorm) {
#pragma unroll
          for (int j = 0; j < NIN; ++j) s[j] = fminf(fmaxf((s[j] - om[j]) / osd[j], -10.f), 10.f);
        }
        float y[NA];
#pragma unroll
        for (int i = 0; i < NA; ++i) y[i] = linear_row<NIN>(w + i * NIN, s);
        if (env.step(y, racc)) {
          done = true;
          nsteps = t + 1;
        }
      }
      if (__ballot(!done) == 0) break;  // the wave leaves when all its threads are done
    }
    // fold the episode into the lane totals (sequential f64, episode order)
    rsum += racc;
    rsq += racc * racc;
    nsum += nsteps;
  }

  double r = rsum / (double)K;
  if (a.jiggle) r += (hash_ctr(key, glane, kJiggleT, 15) & 1ull) ? 1e-12 : -1e-12;
  a.ret[lane] = r;
  a.ent[lane] = 0.0;  // a deterministic policy
  a.steps[lane] = nsum;
  if (ea.ret_sq) ea.ret_sq[lane] = rsq;
  if constexpr (FEAT & kFeatObsStats) {
#pragma unroll
    for (int j = 0; j < NIN; ++j) {
      a.os_mean[(int64_t)lane * NIN + j] = os_mean[j];
      a.os_m2[(int64_t)lane * NIN + j] = os_m2[j];
    }
    a.os_count[lane] = os_n;
  }
}

// ---- run batches (fdr_rollout_runs): R runs x L lanes in one launch ---------------------------------------------
// rollout_runs_kernel is rollout_linear_kernel with the lane's theta, sigma, observation statistics and global id
// taken from the lane's RUN: thread g of the grid is lane g % L of run g / L, whatever the wave and workgroup
// boundaries; idx, sign, episode_ids and every output stay indexed by g.  The episode loop below repeats
// rollout_linear_kernel's text: moved into one shared __forceinline__ body, the 40 solo instances kept their
// instruction counts but not their register allocation (tools/isa_diff.py; DESIGN.md 3.1.4 has the diff), so the solo
// kernel stays as it was and this one holds a copy.  A change to one episode loop belongs in both:
// tests/test_gpu_runs.py holds the two bit-equal.
template <int P, int NIN>
struct RunLane {
  const RunsArgs& ra;
  int run;
  __device__ __forceinline__ ParamSrc src(int lane) const {
    LanesArgs l = ra.e.r.lanes;
    l.base = ra.theta_runs + (int64_t)run * P;
    l.base_stride = 0;
    l.sigma = ra.sigma_runs[run];
    return l.src(lane);
  }
  __device__ __forceinline__ const float* obs_mean() const { return ra.obs_mean_runs + (int64_t)run * NIN; }
  __device__ __forceinline__ const float* obs_std() const { return ra.obs_std_runs + (int64_t)run * NIN; }
  __device__ __forceinline__ uint64_t glane(int lane) const {
    return (uint64_t)(ra.run_lane_offset[run] + (int64_t)(lane - run * ra.lanes_per_run));
  }
};

// FEAT: a subset of kFeatObsStats | kFeatObsNorm (no state recording).
template <int ENV, int FEAT>
__global__ __launch_bounds__(kLinearBlock) void rollout_runs_kernel(RunsArgs ra) {
  static_assert((FEAT & ~(kFeatObsNorm | kFeatObsStats)) == 0, "runs: obs-norm and obs-stats only");
  using E = PhysicsSpec<ENV>;
  constexpr int NIN = E::NIN, NA = E::NA, P = NIN * NA;
  const EpisodesArgs& ea = ra.e;
  const RolloutArgs& a = ea.r;
  const int lane = blockIdx.x * kLinearBlock + threadIdx.x;
  if (lane >= a.n_lanes) return;
  const RunLane<P, NIN> from{ra, lane / ra.lanes_per_run};

  // theta' and the lane's norm2 (f64, ascending p); an out-of-range offset never reaches the table (LanesArgs::src)
  ParamSrc src = from.src(lane);
  float w[P];
#pragma unroll
  for (int p = 0; p < P; ++p) w[p] = src.get(p);
  if (a.norm2) a.norm2[lane] = src.n2;

  [[maybe_unused]] float om[NIN], osd[NIN];
  if constexpr (FEAT & kFeatObsNorm) {
#pragma unroll
    for (int j = 0; j < NIN; ++j) {
      om[j] = from.obs_mean()[j];
      osd[j] = from.obs_std()[j];
    }
  }

  const int T = a.T, K = ea.n_episodes;
  const uint64_t key = a.key;
  const uint64_t glane = from.glane(lane);  // physical global lane: the jiggle's key
  double rsum = 0.0, rsq = 0.0;
  int nsum = 0;
  // the lane's Welford statistic, running on across its episodes (ObsWelford's arithmetic per element)
  [[maybe_unused]] int os_n = 0;
  [[maybe_unused]] float os_mean[NIN], os_m2[NIN];
#pragma unroll
  for (int j = 0; j < NIN; ++j) os_mean[j] = os_m2[j] = 0.f;

  for (int ep = 0; ep < K; ++ep) {
    const uint64_t ulane =
        ea.episode_ids ? (uint64_t)ea.episode_ids[(int64_t)lane * K + ep] : glane * (uint64_t)K + (uint64_t)ep;
    LinearSim<ENV> env;
    env.sim.reset(key, ulane);
    double racc = 0.0;
    int nsteps = T;
    bool done = false;
    for (int t = 0; t < T; ++t) {
      if (!done) {  // a finished thread adds nothing and stores nothing more
        float s[NIN];
        env.obs(s);
        if constexpr (FEAT & kFeatObsStats) {
          // the coin of step t of stream ulane: the one the wave-per-lane kernels draw 64 steps at a time
          if (uniform24(hash_ctr(key, ulane, (uint64_t)t, 14)) < a.os_chance) {
#pragma clang fp contract(off)
            const int cc = os_n;
            os_n += 1;
#pragma unroll
            for (int j = 0; j < NIN; ++j) {
              const float delta = s[j] - os_mean[j];
              const float delta_n = delta / (float)os_n;
              os_mean[j] += delta_n;
              os_m2[j] += (delta * delta_n) * (float)cc;
            }
          }
        }
        if constexpr (FEAT & kFeatObsNorm) {
#pragma unroll
          for (int j = 0; j < NIN; ++j) s[j] = fminf(fmaxf((s[j] - om[j]) / osd[j], -10.f), 10.f);
        }
        float y[NA];
#pragma unroll
        for (int i = 0; i < NA; ++i) y[i] = linear_row<NIN>(w + i * NIN, s);
        if (env.step(y, racc)) {
          done = true;
          nsteps = t + 1;
        }
      }
      if (__ballot(!done) == 0) break;  // the wave leaves when all its threads are done
    }
    // fold the episode into the lane totals (sequential f64, episode order)
    rsum += racc;
    rsq += racc * racc;
    nsum += nsteps;
  }

  double r = rsum / (double)K;
  if (a.jiggle) r += (hash_ctr(key, glane, kJiggleT, 15) & 1ull) ? 1e-12 : -1e-12;
  a.ret[lane] = r;
  if (a.ent) a.ent[lane] = 0.0;  // a deterministic policy
  a.steps[lane] = nsum;
  if (ea.ret_sq) ea.ret_sq[lane] = rsq;
  if constexpr (FEAT & kFeatObsStats) {
#pragma unroll
    for (int j = 0; j < NIN; ++j) {
      a.os_mean[(int64_t)lane * NIN + j] = os_mean[j];
      a.os_m2[(int64_t)lane * NIN + j] = os_m2[j];
    }
    a.os_count[lane] = os_n;
  }
}

// obs_stats_merge_kernel (fdr_rollout.hip) per run: workgroup r folds run r's L partials into accumulator r in lane
// order, one thread per observation dimension, the same f32 expressions.
__global__ void obs_stats_merge_runs_kernel(const float* __restrict__ mean, const float* __restrict__ m2,
                                            const int32_t* __restrict__ count, int L, int d, float* acc_mean,
                                            float* acc_m2, int64_t* acc_count) {
#pragma clang fp contract(off)
  const int j = threadIdx.x, r = blockIdx.x;
  const int64_t l0 = (int64_t)r * L;
  int64_t c = acc_count[r];
  float m = j < d ? acc_mean[(int64_t)r * d + j] : 0.f, v = j < d ? acc_m2[(int64_t)r * d + j] : 0.f;
  for (int i = 0; i < L; ++i) {
    const int64_t oc = count[l0 + i];
    if (oc == 0) continue;
    const int64_t cnt = c + oc;
    if (j < d) {
      const float om = mean[(l0 + i) * d + j], ov = m2[(l0 + i) * d + j];
      const float md = om - m;
      const float mds = md * md;
      const float cm = ((float)c * m + (float)oc * om) / (float)cnt;
      v = (v + ov) + ((mds * (float)c) * (float)oc) / (float)cnt;
      m = cm;
    }
    c = cnt;
  }
  if (j < d) {
    acc_mean[(int64_t)r * d + j] = m;
    acc_m2[(int64_t)r * d + j] = v;
  }
  __syncthreads();  // every thread has read acc_count[r]
  if (j == 0) acc_count[r] = c;
}

// out[l, i] = row i of theta'_l against x[l, :], any n_in <= 64 / n_act <= 16
__global__ __launch_bounds__(kLinearBlock) void policy_forward_linear_kernel(LanesArgs lanes, int n_lanes, int n_in,
                                                                            int n_act, const float* x, float* out) {
#pragma clang fp contract(off)
  const int lane = blockIdx.x * kLinearBlock + threadIdx.x;
  if (lane >= n_lanes) return;
  const ParamSrc src = lanes.src(lane);
  const float* xl = x + (int64_t)lane * n_in;
  for (int i = 0; i < n_act; ++i) {
    float acc = src.get_nocount((int64_t)i * n_in) * xl[0];
    for (int j = 1; j < n_in; ++j) {
      const float p = src.get_nocount((int64_t)i * n_in + j) * xl[j];
      acc = acc + p;
    }
    out[(int64_t)lane * n_act + i] = acc;
  }
}

int linear_shape_check(const PolicyKey& k) {
  if (k.n_in < 1 || k.n_in > kLinearMaxIn) return set_error(FDR_ERR_UNSUPPORTED, "linear n_in must be in 1..64");
  if (k.n_act < 1 || k.n_act > kLinearMaxAct) return set_error(FDR_ERR_UNSUPPORTED, "linear n_act must be in 1..16");
  return FDR_OK;
}

int launch_policy_forward_linear(const PolicyKey& k, const LanesArgs& lanes, int n_lanes, const float* x, float* out,
                                 hipStream_t stream) {
  const int rc = linear_shape_check(k);
  if (rc) return rc;
  const dim3 grid((n_lanes + kLinearBlock - 1) / kLinearBlock), block(kLinearBlock);
  hipLaunchKernelGGL(policy_forward_linear_kernel, grid, block, 0, stream, lanes, n_lanes, k.n_in, k.n_act, x, out);
  return check_launch("policy_forward_linear_kernel");
}

constexpr int kLinearFeatBits = kFeatStates | kFeatObsStats | kFeatObsNorm;  // 8 sets per env

int launch_rollout_linear(const PolicyKey& k, int env_kind, const EpisodesArgs& args, hipStream_t stream) {
  const PhysicsEnv* const pe = physics_env(env_kind);
  if (!pe) return set_error(FDR_ERR_UNSUPPORTED, "a linear policy runs the physics envs only");
  if (k.n_in != pe->obs || k.n_act != pe->act)
    return set_error(FDR_ERR_UNSUPPORTED, "a linear policy runs a physics env at the env's own (obs, act) shape");
  const int feat = rollout_feat(args.r, false);
  if ((feat & kFeatStates) && args.n_episodes != 1)
    return set_error(FDR_ERR_UNSUPPORTED, "state recording takes one episode per lane");
  const dim3 grid((args.r.n_lanes + kLinearBlock - 1) / kLinearBlock), block(kLinearBlock);
  int rc = FDR_OK;
  with_physics_env(env_kind, [&](auto spec) {  // pe: env_kind is one of them
    using E = decltype(spec);
    const bool hit = launch_feat_set<kLinearFeatBits>(feat, [&](auto f) {
      hipLaunchKernelGGL((rollout_linear_kernel<E::ENV, decltype(f)::value>), grid, block, 0, stream, args);
    });
    rc = hit ? check_launch("rollout_linear_kernel")
             : set_error(FDR_ERR_UNSUPPORTED, "a linear policy takes no injected draws");
  });
  return rc;
}

constexpr int kRunsFeatBits = kFeatObsStats | kFeatObsNorm;  // 4 sets per env

int launch_rollout_runs(const PolicyKey& k, int env_kind, const RunsArgs& args, hipStream_t stream) {
  const PhysicsEnv* const pe = physics_env(env_kind);
  if (!pe) return set_error(FDR_ERR_UNSUPPORTED, "a linear policy runs the physics envs only");
  if (!k.linear) return set_error(FDR_ERR_UNSUPPORTED, "fdr_rollout_runs takes a linear policy");
  if (k.n_in != pe->obs || k.n_act != pe->act)
    return set_error(FDR_ERR_UNSUPPORTED, "a linear policy runs a physics env at the env's own (obs, act) shape");
  const int feat = rollout_feat(args.e.r, false);
  const dim3 grid((args.e.r.n_lanes + kLinearBlock - 1) / kLinearBlock), block(kLinearBlock);
  int rc = FDR_OK;
  with_physics_env(env_kind, [&](auto spec) {  // pe: env_kind is one of them
    using E = decltype(spec);
    const bool hit = launch_feat_set<kRunsFeatBits>(feat, [&](auto f) {
      hipLaunchKernelGGL((rollout_runs_kernel<E::ENV, decltype(f)::value>), grid, block, 0, stream, args);
    });
    rc = hit ? check_launch("rollout_runs_kernel")
             : set_error(FDR_ERR_UNSUPPORTED, "fdr_rollout_runs takes no state recording or injected draws");
  });
  return rc;
}

int launch_obs_stats_merge_runs(const float* mean, const float* m2, const int32_t* count, int n_runs, int lanes_per_run,
                                int d, float* acc_mean, float* acc_m2, int64_t* acc_count, hipStream_t stream) {
  if (d > 1024) return set_error(FDR_ERR_UNSUPPORTED, "obs_dim > 1024");
  const int threads = (d + 63) / 64 * 64;
  hipLaunchKernelGGL(obs_stats_merge_runs_kernel, dim3(n_runs), dim3(threads), 0, stream, mean, m2, count,
                     lanes_per_run, d, acc_mean, acc_m2, acc_count);
  return check_launch("obs_stats_merge_runs_kernel");
}

}  // namespace fdr
