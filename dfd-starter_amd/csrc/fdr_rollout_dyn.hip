// fdr_rollout_dyn.hip -- the runtime-shaped kernel family: one wave per lane, the policy's n_in / n_act kernel
// arguments instead of template parameters (DESIGN.md 3.1 "Runtime-shaped kernels").
//
//   rollout_dyn_kernel<DISC>         the synthetic env, every feature of rollout_kernel (fdr_rollout_kernel.h)
//   policy_forward_dyn_kernel<DISC>  policy_forward_kernel's contract
//   theta_prime_dyn_kernel<DISC>     DynLane::load over a RecordSrc (fdr_diag_theta_prime, FDR_LOADER_DYN)
//
// The fallback for every (n_in, n_act) that is no compiled instance (fdr_mlp.h: MlpShapes, PhysicsShapes), and the
// whole of FDR_ROLLOUT_GENERIC.  Limits, Layout's own: 1 <= n_in <= 64; discrete 1 <= n_act <= 16; continuous
// 1 <= n_act <= 8.  Two instances per kernel (discrete / continuous): the feature bits are wave-uniform runtime
// branches, only the deterministic / sampled choice is compiled twice (as rollout_kernel: one loop each).
//
// LDS is dynamic, sized from the shape: the env's [M | K] rows (shared by the block), a per-wave weight tile
// (W1 row j, the W3 slice) and the per-wave hand-off scratch.  (64, 16): 21.0 + 80.0 + 2.0 KiB per 4-lane block.
// The draws use the compiled kernels' counters -- hash_ctr(key, global lane, t, k) -- so a lane's stream does not
// depend on the kernel that runs it.
#include "fdr_mlp_dyn.h"
#include "fdr_rollout_parts.h"

namespace fdr {

extern __shared__ __attribute__((aligned(16))) char dyn_smem[];

// env rows [M[i] (nx) | K[i] (one column per action)], stride in floats (b128 rows; rollout_kernel's padding rule)
__host__ __device__ inline int dyn_env_stride(int nx, int n_act) {
  const int nmk = nx + round4(n_act);
  return nmk % 8 == 0 ? nmk + 4 : nmk;
}
template <bool DISC>
static size_t dyn_lane_lds_bytes(const DynLayout<DISC>& l) {  // tiles + scratch of a block
  return (size_t)kLanesPerBlock * (l.tile_f4() * sizeof(float4) + sizeof(WaveScratch));
}

template <bool DISC>
__global__ __launch_bounds__(64 * kLanesPerBlock, 4) void rollout_dyn_kernel(RolloutArgs a, int n_in, int n_act,
                                                                             int feat) {
  using Lane = DynLane<DISC>;
  const DynLayout<DISC> lay(n_in, n_act);
  const int NX = lay.nx, MKS = dyn_env_stride(NX, n_act);
  float* envMK = reinterpret_cast<float*>(dyn_smem);
  float4* wtile = reinterpret_cast<float4*>(dyn_smem + (size_t)n_in * MKS * sizeof(float));
  WaveScratch* scratch = reinterpret_cast<WaveScratch*>(wtile + kLanesPerBlock * lay.tile_f4());

  const int j = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = blockIdx.x * kLanesPerBlock + wv;
  for (int e = threadIdx.x; e < n_in * MKS; e += blockDim.x) {  // padding columns zero (b128 row reads)
    const int i = e / MKS, k = e % MKS;
    envMK[e] = (k < n_in ? a.M[i * n_in + k] : (k >= NX && k < NX + n_act ? a.K[i * n_act + k - NX] : 0.f));
  }
  __syncthreads();  // the only cross-wave hand-off: shared env matrices
  if (lane >= a.n_lanes) return;

  ParamSrc src = a.lanes.src(lane);
  const bool det = a.lanes.deterministic ? a.lanes.deterministic[lane] != 0 : false;
  Lane pl;
  pl.load(lay, src, j, a.bn_mean, a.bn_var, wtile + wv * lay.tile_f4());
  write_norm2(a, lane, j, src.n2);

  const bool f_states = (feat & kFeatStates) != 0, f_stats = (feat & kFeatObsStats) != 0,
             f_norm = (feat & kFeatObsNorm) != 0, f_inject = (feat & kFeatInject) != 0,
             f_term = (feat & kFeatTerm) != 0;
  const int ji = j < n_in ? j : n_in - 1;
  const float om = f_norm ? a.obs_mean[ji] : 0.f;
  const float osd = f_norm ? a.obs_std[ji] : 1.f;
  auto policy_input = [&](float s) {
    float x = s;
    if (f_norm) x = fminf(fmaxf((s - om) / osd, -10.f), 10.f);  // agent.py:40-41
    return pl.input_transform(x);
  };

  float s = a.s0[ji];  // env state element j (j < n_in)
  const int T = a.T;
  const uint64_t key = a.key;
  const uint64_t ulane = (uint64_t)(a.lanes.lane_offset + lane);  // global lane id
  int nsteps = T;
  double racc = 0.0;
  float eacc = 0.f;
  const int o = j & 15;
  // Draw batches as rollout_kernel: one counter hash per thread covers up to 64 future draws (discrete: thread i
  // holds the uniform of step t0 + i; continuous: thread i the normal of step t0 + i / n_act, dim i % n_act).
  const int draws_per_step = DISC ? 1 : n_act;
  const int steps_per_batch = 64 / draws_per_step;
  const int ds = j / draws_per_step, dk = j - ds * draws_per_step;
  float rbuf = 0.f;
  uint64_t os_mask = 0;
  int os_n = 0;
  float os_mean = 0.f, os_m2 = 0.f;
  auto draw = [&](int t) {
    if (f_inject) {  // host-injected draws (u_inject), same batch layout
      const int tt = t + ds;
      rbuf = tt < T && ds < steps_per_batch ? a.u_inject[((int64_t)lane * T + tt) * draws_per_step + dk] : 0.f;
    } else {
      const uint64_t h = hash_ctr(key, ulane, (uint64_t)(t + ds), (uint64_t)dk);
      rbuf = DISC ? uniform24(h) : normal_bm(h);
    }
  };
  const int zbase = 4 * (o < n_act ? o : 0);  // ds_bpermute byte address of dim o in step 0 of a batch
  WaveScratch* const sc = &scratch[wv];
  const float* const mrow = envMK + ji * MKS;

  auto episode = [&](auto det_tag) {
    constexpr bool kDet = decltype(det_tag)::value;
    for (int t0 = 0; t0 < T; t0 += steps_per_batch) {
      if constexpr (!kDet) draw(t0);
      const int nb = T - t0 < steps_per_batch ? T - t0 : steps_per_batch;
      for (int tb = 0; tb < nb; ++tb) {
        const int t = t0 + tb;
        asm volatile("" ::: "memory");  // the W1 / M / K rows stay per-step LDS reads
        float zt = 0.f;  // this step's normal for action dim o (continuous)
        if constexpr (!DISC && !kDet)
          zt = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(zbase + 4 * n_act * tb,
                                                                      __builtin_bit_cast(int, rbuf)));
        if (f_states) {
          if (j < n_in) a.states[((int64_t)lane * T + t) * n_in + j] = s;
        }
        if (f_stats) {  // rollout_kernel's Welford update: coins 64 steps at a time (counter k = 14), one ballot
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
        // policy input and env state broadcast through the wave's LDS scratch
        sc->x[j] = pl.input_slot(j, policy_input(s));
        sc->h1[j] = j < n_in ? s : 0.f;
        wave_lds_sync();
        float pre = 0.f;
        const float h1 = pl.layer1_env(sc->x, sc->h1, mrow, pre);
        const float y = pl.layers23(h1, sc, j);
        if constexpr (DISC) {
          const float p = pl.template softmax<!kDet>(y, j);
          // sequential f32 cumsum, the oracle's order; argmax = first maximal index; inverse CDF = the number of
          // partial sums <= target, capped at n_act - 1 (rollout_kernel, with a runtime trip count)
          const float p0 = readlane_f(p, 0);
          float tot = p0;
          int act_d = 0;
          if constexpr (kDet) {
            float best = p0;
            for (int i = 1; i < n_act; ++i) {
              const float pi = readlane_f(p, i);
              tot += pi;
              act_d = pi > best ? i : act_d;
              best = fmaxf(best, pi);
            }
          } else {
            for (int i = 1; i < n_act; ++i) tot += readlane_f(p, i);
            const float target = readlane_f(rbuf, tb) * tot;
            float c = 0.f;
            for (int i = 0; i < n_act - 1; ++i) {
              c += readlane_f(p, i);
              act_d += c <= target ? 1 : 0;
            }
          }
          eacc -= (j < n_act) ? disc_entropy_term(p, tot) : 0.f;
          pre += mrow[NX + act_d];
        } else {
          const float th = tanh_fast(y);
          const float sd = std_from_tanh(row_shl_dyn(th, j, n_act));  // lane o <- lane o + n_act: the std half
          eacc += __builtin_amdgcn_logf(sd);  // log2; lanes >= n_act and the ln 2 scale: epilogue
          const float act_c = kDet ? th : gauss_action(th, sd, zt);
          // K a: a[m] sits in lane m; the FMA chain of dpp_tail, in its order
          for (int m = 0; m < n_act; ++m) pre = fmaf(readlane_f(act_c, m), mrow[NX + m], pre);
        }
        s = tanh_fast(pre);
        racc += (double)s;  // lane 0 holds the reward s'[0]
        if (f_term) {       // done after this step: its reward and entropy count (agent.py:46-52)
          if (fabsf(readlane_f(s, a.done_dim)) > a.done_thr) {
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

  // ---- epilogue ----
  store_results<DISC>(a, lane, j, ulane, racc, entropy_sum(eacc, j, n_act), nsteps, n_act);
  if (f_stats) {
    if (j < n_in) {
      a.os_mean[(int64_t)lane * n_in + j] = os_mean;
      a.os_m2[(int64_t)lane * n_in + j] = os_m2;
    }
    if (j == 0) a.os_count[lane] = os_n;
  }
}

template <bool DISC>
__global__ __launch_bounds__(64 * kLanesPerBlock) void policy_forward_dyn_kernel(
    LanesArgs lanes, int n_lanes, int n_in, int n_act, const float* __restrict__ bn_mean,
    const float* __restrict__ bn_var, const float* __restrict__ x, float* __restrict__ out0,
    float* __restrict__ out1) {
  using Lane = DynLane<DISC>;
  const DynLayout<DISC> lay(n_in, n_act);
  float4* wtile = reinterpret_cast<float4*>(dyn_smem);
  WaveScratch* scratch = reinterpret_cast<WaveScratch*>(wtile + kLanesPerBlock * lay.tile_f4());
  const int j = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int lane = blockIdx.x * kLanesPerBlock + wv;
  if (lane >= n_lanes) return;
  ParamSrc src = lanes.src(lane);
  Lane pl;
  pl.load(lay, src, j, bn_mean, bn_var, wtile + wv * lay.tile_f4());
  WaveScratch* sc = &scratch[wv];
  const int ji = j < n_in ? j : n_in - 1;
  sc->x[j] = pl.input_slot(j, pl.input_transform(x[(int64_t)lane * n_in + ji]));
  wave_lds_sync();
  const float y = pl.layers23(pl.layer1(sc->x), sc, j);
  if constexpr (DISC) {
    const float p = pl.template softmax<false>(y, j);
    if (j < n_act) out0[(int64_t)lane * n_act + j] = p;
  } else {
    const float t = tanh_fast(y);
    const float ts = row_shl_dyn(t, j, n_act);
    if (j < n_act) {
      out0[(int64_t)lane * n_act + j] = t;
      out1[(int64_t)lane * n_act + j] = std_from_tanh(ts);
    }
  }
}

// The read-back of what DynLane::load asks of its source (fdr_rollout.hip: ThetaPrimeArgs' contract)
struct ThetaPrimeDynArgs {
  LanesArgs lanes;
  int n_lanes, n_in, n_act;
  int64_t P;
  const float* bn_mean;
  const float* bn_var;
  float* out;
  int32_t* reads;
  int32_t* counted;
  double* n2;
};

template <bool DISC>
__global__ __launch_bounds__(64 * kLanesPerBlock) void theta_prime_dyn_kernel(ThetaPrimeDynArgs a) {
  const DynLayout<DISC> lay(a.n_in, a.n_act);
  float4* wtile = reinterpret_cast<float4*>(dyn_smem);
  const int j = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = blockIdx.x * kLanesPerBlock + wv;
  if (lane >= a.n_lanes) return;
  RecordSrc src;
  static_cast<ParamSrc&>(src) = a.lanes.src(lane);
  src.out = a.out + (int64_t)lane * a.P;
  src.reads = a.reads + (int64_t)lane * a.P;
  src.counted = a.counted + (int64_t)lane * a.P;
  src.rec = true;
  DynLane<DISC> pl;
  pl.load(lay, src, j, a.bn_mean, a.bn_var, wtile + wv * lay.tile_f4());
  const double n2 = wave_sum(src.n2);
  if (j == 0) a.n2[lane] = n2;
}

// ---------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------
int dyn_shape_check(const PolicyKey& k) {
  if (k.n_in < 1 || k.n_in > kDynMaxIn) return set_error(FDR_ERR_UNSUPPORTED, "n_in must be in 1..64");
  if (k.discrete && (k.n_act < 1 || k.n_act > kDynMaxActDisc))
    return set_error(FDR_ERR_UNSUPPORTED, "discrete n_act must be in 1..16");
  if (!k.discrete && (k.n_act < 1 || k.n_act > kDynMaxActCont))
    return set_error(FDR_ERR_UNSUPPORTED, "continuous n_act must be in 1..8 (a head of 2 n_act <= 16 outputs)");
  return FDR_OK;
}

// the shape against the limits and n_params against the layout, then f(DynLayout<DISC>)
template <class F>
static int with_dyn_layout(const PolicyKey& k, F&& f) {
  const int rc = dyn_shape_check(k);
  if (rc) return rc;
  auto one = [&](auto lay) {
    if (lay.P != k.n_params) return set_error(FDR_ERR_INVALID, "n_params does not match the policy layout");
    return f(lay);
  };
  return k.discrete ? one(DynLayout<true>(k.n_in, k.n_act)) : one(DynLayout<false>(k.n_in, k.n_act));
}

// A block's dynamic LDS above the 64 KiB every kernel may take needs the kernel's opt-in (up to the CU's 160 KiB)
template <class Kernel>
static int dyn_lds_opt_in(Kernel kernel, size_t bytes, const char* what) {
  if (bytes <= 64 * 1024) return FDR_OK;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)bytes) != hipSuccess) {
    (void)hipGetLastError();
    return set_error(FDR_ERR_HIP, what);
  }
  return FDR_OK;
}

int launch_rollout_dyn(const PolicyKey& k, const RolloutArgs& args, hipStream_t stream) {
  const int feat = rollout_feat(args, args.done_thr > 0.f);
  if (!feat_legal(kLaneFeatBits, feat))
    return set_error(FDR_ERR_UNSUPPORTED, "u_inject is not combined with the obs statistics");
  const dim3 grid((args.n_lanes + kLanesPerBlock - 1) / kLanesPerBlock), block(64 * kLanesPerBlock);
  return with_dyn_layout(k, [&](auto lay) {
    constexpr bool DISC = std::is_same_v<decltype(lay), DynLayout<true>>;
    const size_t lds = (size_t)k.n_in * dyn_env_stride(lay.nx, k.n_act) * sizeof(float) + dyn_lane_lds_bytes(lay);
    const int rc = dyn_lds_opt_in(rollout_dyn_kernel<DISC>, lds, "rollout_dyn_kernel (LDS opt-in)");
    if (rc) return rc;
    hipLaunchKernelGGL((rollout_dyn_kernel<DISC>), grid, block, lds, stream, args, k.n_in, k.n_act, feat);
    return check_launch("rollout_dyn_kernel");
  });
}

int launch_policy_forward_dyn(const PolicyKey& k, const LanesArgs& lanes, int n_lanes, const float* bn_mean,
                              const float* bn_var, const float* x, float* out0, float* out1, hipStream_t stream) {
  const dim3 grid((n_lanes + kLanesPerBlock - 1) / kLanesPerBlock), block(64 * kLanesPerBlock);
  return with_dyn_layout(k, [&](auto lay) {
    constexpr bool DISC = std::is_same_v<decltype(lay), DynLayout<true>>;
    const size_t lds = dyn_lane_lds_bytes(lay);
    const int rc = dyn_lds_opt_in(policy_forward_dyn_kernel<DISC>, lds, "policy_forward_dyn_kernel (LDS opt-in)");
    if (rc) return rc;
    hipLaunchKernelGGL((policy_forward_dyn_kernel<DISC>), grid, block, lds, stream, lanes, n_lanes, k.n_in, k.n_act,
                       bn_mean, bn_var, x, out0, out1);
    return check_launch("policy_forward_dyn_kernel");
  });
}

int launch_theta_prime_dyn(const PolicyKey& k, const LanesArgs& lanes, int n_lanes, const float* bn_mean,
                           const float* bn_var, float* out, int32_t* reads, int32_t* counted, double* n2,
                           hipStream_t stream) {
  const ThetaPrimeDynArgs a{lanes, n_lanes, k.n_in, k.n_act, k.n_params, bn_mean, bn_var, out, reads, counted, n2};
  const dim3 grid((n_lanes + kLanesPerBlock - 1) / kLanesPerBlock), block(64 * kLanesPerBlock);
  return with_dyn_layout(k, [&](auto lay) {
    constexpr bool DISC = std::is_same_v<decltype(lay), DynLayout<true>>;
    const size_t lds = dyn_lane_lds_bytes(lay);
    const int rc = dyn_lds_opt_in(theta_prime_dyn_kernel<DISC>, lds, "theta_prime_dyn_kernel (LDS opt-in)");
    if (rc) return rc;
    hipLaunchKernelGGL((theta_prime_dyn_kernel<DISC>), grid, block, lds, stream, a);
    return check_launch("theta_prime_dyn_kernel");
  });
}

}  // namespace fdr
