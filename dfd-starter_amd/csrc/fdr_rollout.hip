// fdr_rollout.hip -- whole-episode batched rollouts and batched policy forwards for the FD engine.
//
// Design (DESIGN.md "Rollout kernel"):
//   * ONE WAVE PER LANE (lane = one perturbation x env).  Hidden width 64 == wave width: wave lane
//     j owns hidden unit j of both layers and keeps its weight rows in VGPRs for the whole episode
//     (W1 row j, W2 row j, a 16-input slice of W3) -- theta' is read from HBM once per episode,
//     never per step.  The kernel is fp32-VALU-bound, not HBM-bound.
//   * theta'_l is built on the fly from theta + sign_l * fl32(sigma * table[idx_l + p])
//     (bit-exact with worker/worker.py:28) while loading those registers; the same pass
//     accumulates ||lambda_l||^2 for the learner (learner/finite_differences.py:107).
//   * Activations cross lanes through a 1 KiB per-wave LDS scratch (one ds_write_b32 per lane,
//     broadcast ds_read_b128 back) feeding packed f32 FMAs, or through DPP row_newbcast where the
//     input already sits in the caller's 16-lane row (the head, K a).
//   * The env (synthetic linear-tanh system, the trap gridworld, or one of gym's five classic-control systems) runs
//     inside the same loop.
//   * 4 lanes (waves) per 256-thread workgroup, <= 128 VGPRs -> 16 waves/CU: 4096 lanes fill
//     all 256 CUs in one wave of workgroups.
//
// This unit: launch_rollout (which kernel family runs a rollout), policy_forward_kernel, the theta' read-back
// kernels and the Welford merge.  The rollout kernels are compiled in units of their own, one family each:
//   fdr_rollout_lane.hip   rollout_kernel, synthetic env          (fdr_rollout_kernel.h, fdr_mlp_lane.h)
//   fdr_rollout_wide.hip   rollout_kernel<WIDE>, synthetic env
//   fdr_rollout_env.hip    rollout_kernel, trap / CartPole / Pendulum / Acrobot / MountainCar (both)
//   fdr_rollout_pair.hip   rollout_pair_kernel                    (fdr_mlp_pair.h)
//   fdr_rollout_dyn.hip    the runtime-shaped family: rollout, forward and loader read-back at any (n_in, n_act)
//                          within Layout's limits                 (fdr_mlp_dyn.h)
// fdr_mlp.h holds what they share: Layout, the compiled shapes (with_shape) and the feature bits.
#include "fdr_mlp_lane.h"
#include "fdr_mlp_pair.h"

namespace fdr {

// ---------------------------------------------------------------------------------------------
// Batched single-step forward: fdr_policy_forward
// ---------------------------------------------------------------------------------------------
template <int NIN, int NA, bool DISC>
__global__ __launch_bounds__(64 * kLanesPerBlock) void policy_forward_kernel(
    LanesArgs lanes, int n_lanes, const float* __restrict__ bn_mean,
    const float* __restrict__ bn_var, const float* __restrict__ x, float* __restrict__ out0,
    float* __restrict__ out1) {
  using Lane = MlpLane<NIN, NA, DISC>;
  __shared__ float4 wtile[kLanesPerBlock * Lane::kTileF4];
  __shared__ typename Lane::Scratch scratch[kLanesPerBlock];
  const int j = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int lane = blockIdx.x * kLanesPerBlock + wv;
  if (lane >= n_lanes) return;
  ParamSrc src = lanes.src(lane);
  Lane pl;
  pl.load(src, j, bn_mean, bn_var, wtile + wv * Lane::kTileF4);
  auto* sc = &scratch[wv];
  sc->x[j] = j < NIN ? pl.input_transform(x[(int64_t)lane * NIN + j]) : (j == NIN ? 1.f : 0.f);
  wave_lds_sync();
  float xb[Lane::NX];
  lds_bcast<Lane::NX>(sc->x, xb);
  const float y = pl.layers23(pl.layer1(xb), sc, j, [](int, float) {});
  if constexpr (DISC) {
    const float p = pl.softmax(y, j);
    if (j < NA) out0[(int64_t)lane * NA + j] = p;
  } else {
    const float t = tanh_fast(y);
    const float ts = dpp_mov<kDppRowShl + NA>(t);  // lane o <- lane o + NA: the std half
    if (j < NA) {
      out0[(int64_t)lane * NA + j] = t;
      out1[(int64_t)lane * NA + j] = std_from_tanh(ts);
    }
  }
}

// Is k's (n_in, n_act, discrete) one of the list's compiled shapes?
template <class... S>
static bool key_in(ShapeList<S...>, const PolicyKey& k) {
  return ((k.n_in == S::NIN && k.n_act == S::NA && k.discrete == S::DISC) || ...);
}
// The runtime-shaped family (fdr_rollout_dyn.hip) takes every shape that is no compiled instance, and every shape
// of a FDR_ROLLOUT_GENERIC context.
static bool use_dyn_family(int rollout_impl, const PolicyKey& k) {
  return rollout_impl == FDR_ROLLOUT_GENERIC || !(key_in(MlpShapes{}, k) || key_in(PhysicsShapes{}, k));
}

int launch_policy_forward(const Context& ctx, const PolicyKey& k, const LanesArgs& lanes, int n_lanes,
                          const float* bn_mean, const float* bn_var, const float* x, float* out0,
                          float* out1, hipStream_t stream) {
  if (use_dyn_family(ctx.rollout_impl, k))
    return launch_policy_forward_dyn(k, lanes, n_lanes, bn_mean, bn_var, x, out0, out1, stream);
  const dim3 grid((n_lanes + kLanesPerBlock - 1) / kLanesPerBlock), block(64 * kLanesPerBlock);
  return with_shape<true>(k, "no compiled policy_forward for this (kind, n_in, n_act)", [&](auto shape) {
    using S = decltype(shape);
    hipLaunchKernelGGL((policy_forward_kernel<S::NIN, S::NA, S::DISC>), grid, block, 0, stream, lanes, n_lanes, bn_mean,
                       bn_var, x, out0, out1);
    return check_launch("policy_forward_kernel");
  });
}

static int pair_round_lanes(const Context& ctx) { return 16 * context_cus(ctx); }

// Synthetic-env rollouts: rollout_pair_kernel (two lanes per wave) or rollout_kernel (one lane per
// wave), by the context's rollout_impl: FDR_ROLLOUT_AUTO (default) takes the pair kernel once it puts
// >= 2 waves on every SIMD (n_lanes >= 4 x SIMDs; measured DESIGN.md 3.0: below that the one-lane kernel's
// extra waves win).  The Welford obs statistics and the trap env always use rollout_kernel.
static bool use_pair_kernel(const Context& ctx, int n_lanes) {
  if (ctx.rollout_impl != FDR_ROLLOUT_AUTO) return ctx.rollout_impl == FDR_ROLLOUT_PAIR;
  return n_lanes >= 4 * 4 * context_cus(ctx);  // 4 SIMDs per CU, 2 lanes x 2 waves per SIMD
}

// The register-rich one-lane kernel (rollout_kernel<WIDE>) when its 2-waves-per-SIMD occupancy holds
// every lane in one pass (n_lanes <= 8 x CUs): below that the step is a latency chain, and VGPR room
// buys a shorter one.
static bool use_wide_kernel(const Context& ctx, int n_lanes) {
  if (ctx.rollout_impl != FDR_ROLLOUT_AUTO) return ctx.rollout_impl == FDR_ROLLOUT_WIDE;
  return n_lanes <= 2 * 4 * context_cus(ctx);
}

int launch_rollout(const Context& ctx, const PolicyKey& k, int env_kind, const RolloutArgs& args, hipStream_t stream) {
  if (env_kind != FDR_ENV_SYNTH) return launch_rollout_env(k, env_kind, args, stream);
  // (a PhysicsShapes shape under any other impl has no synthetic-env kernel: launch_rollout_lane refuses it)
  if (use_dyn_family(ctx.rollout_impl, k)) return launch_rollout_dyn(k, args, stream);
  if (use_pair_kernel(ctx, args.n_lanes) && !args.os_mean && !args.u_inject)
    return launch_rollout_pair(k, args, pair_round_lanes(ctx), stream);
  if (use_wide_kernel(ctx, args.n_lanes) && !args.u_inject) return launch_rollout_wide(k, args, stream);
  return launch_rollout_lane(k, args, stream);
}

// ---------------------------------------------------------------------------------------------
// Diagnostics: read-back of the theta' the two loaders form (fdr_diag_theta_prime, include/fdr_diag.h)
// ---------------------------------------------------------------------------------------------
// Only lanes.src(lane) and the loader's load, under the thread mapping of the kernel that owns the loader
// (rollout_kernel / rollout_pair_kernel with lane_base 0), over a RecordSrc: out / reads / counted [n_lanes, P] receive
// every value the loader asked for, n2 [n_lanes] the norm as the rollouts sum it.  No rollout kernel runs this code.
struct ThetaPrimeArgs {
  LanesArgs lanes;
  int n_lanes;
  int64_t P;
  const float* bn_mean;
  const float* bn_var;
  float* out;
  int32_t* reads;
  int32_t* counted;
  double* n2;

  __device__ __forceinline__ RecordSrc src(int lane, bool rec) const {
    RecordSrc s;
    static_cast<ParamSrc&>(s) = lanes.src(lane);
    s.out = out + (int64_t)lane * P;
    s.reads = reads + (int64_t)lane * P;
    s.counted = counted + (int64_t)lane * P;
    s.rec = rec;
    return s;
  }
};

template <int NIN, int NA, bool DISC>
__global__ __launch_bounds__(64 * kLanesPerBlock) void theta_prime_lane_kernel(ThetaPrimeArgs a) {
  using Lane = MlpLane<NIN, NA, DISC>;
  __shared__ float4 wtile[kLanesPerBlock * Lane::kTileF4];
  const int j = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = blockIdx.x * kLanesPerBlock + wv;
  if (lane >= a.n_lanes) return;
  RecordSrc src = a.src(lane, true);
  Lane pl;
  pl.load(src, j, a.bn_mean, a.bn_var, wtile + wv * Lane::kTileF4);
  const double n2 = wave_sum(src.n2);
  if (j == 0) a.n2[lane] = n2;
}

template <int NIN, int NA, bool DISC>
__global__ __launch_bounds__(64 * kPairWaves) void theta_prime_pair_kernel(ThetaPrimeArgs a) {
  using Lane = MlpPair<NIN, NA, DISC>;
  __shared__ float4 wtile[kPairWaves * Lane::kTileF4];
  const int tid = threadIdx.x & 63, wv = threadIdx.x >> 6, hh = tid >> 5, t = tid & 31;
  const int lane0 = (blockIdx.x * kPairWaves + wv) * 2;
  if (lane0 >= a.n_lanes) return;
  const bool active = lane0 + hh < a.n_lanes;
  const int lane = active ? lane0 + hh : lane0;  // an idle half shadows its partner, records nothing
  RecordSrc src = a.src(lane, active);
  Lane pl;
  pl.load(src, t, tid, a.bn_mean, a.bn_var, wtile + wv * Lane::kTileF4);
  double n2 = src.n2;
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) n2 += __shfl_xor(n2, m, kWave);
  if (t == 0 && active) a.n2[lane] = n2;
}

int launch_theta_prime(const PolicyKey& k, const LanesArgs& lanes, int n_lanes, int loader, const float* bn_mean,
                       const float* bn_var, float* out, int32_t* reads, int32_t* counted, double* n2,
                       hipStream_t stream) {
  // the dyn loader where it is asked for, and at every shape that has no compiled loader
  if (loader == FDR_LOADER_DYN || use_dyn_family(FDR_ROLLOUT_AUTO, k))
    return launch_theta_prime_dyn(k, lanes, n_lanes, bn_mean, bn_var, out, reads, counted, n2, stream);
  const ThetaPrimeArgs a{lanes, n_lanes, k.n_params, bn_mean, bn_var, out, reads, counted, n2};
  return with_shape<true>(k, "no compiled loader for this (kind, n_in, n_act)", [&](auto shape) {
    using S = decltype(shape);
    if constexpr (!shape_in<S>(MlpShapes{})) {  // the physics-only shapes have a lane loader and no pair loader
      if (loader != FDR_LOADER_LANE)
        return set_error(FDR_ERR_UNSUPPORTED, "no pair loader compiled for this (kind, n_in, n_act)");
    } else if (loader == FDR_LOADER_PAIR) {
      const int quantum = 2 * kPairWaves;
      hipLaunchKernelGGL((theta_prime_pair_kernel<S::NIN, S::NA, S::DISC>), dim3((n_lanes + quantum - 1) / quantum),
                         dim3(64 * kPairWaves), 0, stream, a);
      return check_launch("theta_prime_pair_kernel");
    }
    hipLaunchKernelGGL((theta_prime_lane_kernel<S::NIN, S::NA, S::DISC>),
                       dim3((n_lanes + kLanesPerBlock - 1) / kLanesPerBlock), dim3(64 * kLanesPerBlock), 0, stream, a);
    return check_launch("theta_prime_lane_kernel");
  });
}

// ---------------------------------------------------------------------------------------------
// Welford merge (utils/math_helpers.py:68-87, increment_from_obs_stats_update): the lanes' partial
// statistics folded into the accumulator in lane order, f32, the reference's operation order.
// One thread per observation dimension; lanes with count 0 are skipped, as the reference.
// ---------------------------------------------------------------------------------------------
__global__ void obs_stats_merge_kernel(const float* __restrict__ mean, const float* __restrict__ m2,
                                       const int32_t* __restrict__ count, int n, int d, float* acc_mean,
                                       float* acc_m2, int64_t* acc_count) {
#pragma clang fp contract(off)
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  int64_t c = *acc_count;
  float m = j < d ? acc_mean[j] : 0.f, v = j < d ? acc_m2[j] : 0.f;
  for (int i = 0; i < n; ++i) {
    const int64_t oc = count[i];
    if (oc == 0) continue;
    const int64_t cnt = c + oc;
    if (j < d) {
      const float om = mean[(int64_t)i * d + j], ov = m2[(int64_t)i * d + j];
      const float md = om - m;
      const float mds = md * md;
      const float cm = ((float)c * m + (float)oc * om) / (float)cnt;
      v = (v + ov) + ((mds * (float)c) * (float)oc) / (float)cnt;
      m = cm;
    }
    c = cnt;
  }
  if (j < d) {
    acc_mean[j] = m;
    acc_m2[j] = v;
  }
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0) *acc_count = c;
}

int launch_obs_stats_merge(const float* mean, const float* m2, const int32_t* count, int n, int d, float* acc_mean,
                           float* acc_m2, int64_t* acc_count, hipStream_t stream) {
  if (d > 1024) return set_error(FDR_ERR_UNSUPPORTED, "obs_dim > 1024");
  hipLaunchKernelGGL(obs_stats_merge_kernel, dim3(1), dim3(1024), 0, stream, mean, m2, count, n, d, acc_mean, acc_m2,
                     acc_count);
  return check_launch("obs_stats_merge_kernel");
}

}  // namespace fdr

#ifdef FDR_PHASE_STAMPS
namespace fdr {
PhaseReader g_phase_reader = nullptr;
}
extern "C" int fdr_debug_phase_read(unsigned long long* out5) {
  return fdr::g_phase_reader ? fdr::g_phase_reader(out5) : -1;
}
#endif
