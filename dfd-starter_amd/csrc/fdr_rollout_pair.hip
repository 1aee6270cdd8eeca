// fdr_rollout_pair.hip -- rollout_pair_kernel (two lanes per wave, synthetic env) and its launcher.
// The default source of `make resource` / `make asm`: the headline (HalfCheetah-shaped) rollout runs this kernel.
#include <algorithm>

#include "fdr_mlp_pair.h"

namespace fdr {

// The draw batch's counter word by addition.  hash_ctr_word is linear in the step modulo 2^64, so
// the word of the batch drawn ahead is the previous batch's plus kStepsPerBatch * 16 * kCtrMul: one 64-bit add per batch
// in place of the shift, or, two 32-bit products, 64-bit multiply-add and add3 that form it from (lane, step, dim).  Every
// draw keeps its bits (tests/test_ctr_recurrence.py).  Off by default: measured -0.55 % per FD step on its own, but
// +0.15 to +0.25 % on top of FDR_PAIR_X_DUMP on two machines (profiles/p26_pair_ctr_xdump.txt) -- the integer multiplies
// issue at the rate of the 64-bit add (tools/probes/mix_probe.hip).  -DFDR_PAIR_CTR_ADD=1: the variant build.
#ifndef FDR_PAIR_CTR_ADD
#define FDR_PAIR_CTR_ADD 0
#endif
// The x hand-off write without its select (continuous instances without observation normalisation, where the policy
// input is the env state itself).  The columns >= NIN of a half's x row (the 1 of the folded bias column, zeros) never
// change: they are written once ahead of the loop, and in the loop thread t >= NIN stores to its own dump slot of the
// wave's scratch, which nobody reads -- the address is a per-thread value fixed before the loop, the store's data is s'
// itself.  -DFDR_PAIR_X_DUMP=0: the select in front of every step's write.
#ifndef FDR_PAIR_X_DUMP
#define FDR_PAIR_X_DUMP 1
#endif

// Where the continuous step loop sits in memory.  The code ahead of the loop is padded to a 64-byte boundary plus a
// count of one-dword nops (executed once per wave); with the loop set-up the compiler puts behind them the loop's first
// instruction then lies 8 bytes past a 64-byte boundary.  Measured: the same 1,203 instructions run
// ~0.9 % faster when the loop starts on an 8-byte boundary than 4 bytes off one, which is where it fell before;
// tools/prologue_mix.py prints the address.  The set-up's size follows what the loop carries in, so the count depends
// on the two macros above: FDR_STEP_LOOP_PAD_DUMP for the instances with the select-free x write, FDR_STEP_LOOP_PAD_SEL
// for those that keep the select (tuned, like the parent's 15, on <17,6,false,0>).  -DFDR_STEP_LOOP_PAD=n sets both,
// n = -1: no padding (make variant).
#ifdef FDR_STEP_LOOP_PAD
#define FDR_STEP_LOOP_PAD_SEL FDR_STEP_LOOP_PAD
#define FDR_STEP_LOOP_PAD_DUMP FDR_STEP_LOOP_PAD
#elif FDR_PAIR_CTR_ADD
#define FDR_STEP_LOOP_PAD_SEL 13
#define FDR_STEP_LOOP_PAD_DUMP 2
#else
#define FDR_STEP_LOOP_PAD_SEL 15
#define FDR_STEP_LOOP_PAD_DUMP 4
#endif
#define FDR_STR2(x) #x
#define FDR_STR(x) FDR_STR2(x)
#define FDR_STEP_LOOP_PLACED(n) \
  if constexpr ((n) >= 0) asm volatile(".p2align 6\n\t.rept " FDR_STR(n) "\n\ts_nop 0\n\t.endr");

// FEAT (fdr_mlp.h): kFeatStates: record visited observations; kFeatObsNorm: observation normalisation (kFeatObsStats,
// the Welford statistics, runs on rollout_kernel); kFeatTerm: terminating synthetic env -- each half keeps a done flag
// (wave-uniform scalars alive0 / alive1): a finished half's steps still execute in lockstep with its partner but add
// nothing to its reward, entropy or step count, and the wave leaves the loop when both halves are done
template <int NIN, int NA, bool DISC, int FEAT>
__global__ __launch_bounds__(64 * kPairWaves, 2) void rollout_pair_kernel(RolloutArgs a) {
  using Lane = MlpPair<NIN, NA, DISC>;
  constexpr int NX = Lane::NX;
  constexpr int NMK = NX + round4(NA);
  constexpr int MKS = NMK % 8 == 0 ? NMK + 4 : NMK;
  __shared__ float4 env4[NIN * MKS / 4];
  __shared__ float4 wtile[kPairWaves * Lane::kTileF4];
  constexpr bool kXDump = FDR_PAIR_X_DUMP && !DISC && !(FEAT & kFeatObsNorm);
  __shared__ PairScratch<kXDump> scratch[kPairWaves];
  float* envMK = reinterpret_cast<float*>(env4);
  for (int e = threadIdx.x; e < NIN * MKS; e += blockDim.x) {
    const int i = e / MKS, k = e % MKS;
    envMK[e] = kPreScale * (k < NIN ? a.M[i * NIN + k] : (k >= NX && k < NX + NA ? a.K[i * NA + k - NX] : 0.f));
  }
  __syncthreads();

  const int tid = threadIdx.x & 63, wv = threadIdx.x >> 6, hh = tid >> 5, t = tid & 31;
  const int lane0 = a.lane_base + (blockIdx.x * kPairWaves + wv) * 2;
  if (lane0 >= a.n_lanes) return;  // whole wave idle
  const bool active = lane0 + hh < a.n_lanes;
  const int lane = active ? lane0 + hh : lane0;  // an idle half shadows its partner, writes nothing

  ParamSrc src = a.lanes.src(lane);
  const bool det = a.lanes.deterministic ? a.lanes.deterministic[lane] != 0 : false;
  Lane pl;
  pl.load(src, t, tid, a.bn_mean, a.bn_var, wtile + wv * Lane::kTileF4);
  {
    double n2 = src.n2;
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) n2 += __shfl_xor(n2, m, kWave);
    // formed here: otherwise the compiler sinks the norm (and its store) past the step loop and keeps every
    // element's sigma * eps in scratch across it
    asm volatile("" : "+v"(n2));
    if (t == 0 && active && a.norm2) a.norm2[lane] = n2;
  }

  const int ji = t < NIN ? t : NIN - 1;
  constexpr bool norm_obs = (FEAT & kFeatObsNorm) != 0;
  const float om = norm_obs ? a.obs_mean[ji] : 0.f;
  const float osd = norm_obs ? a.obs_std[ji] : 1.f;
  auto policy_input = [&](float s) {
    float x = s;
    if (norm_obs) x = fminf(fmaxf((s - om) / osd, -10.f), 10.f);  // agent.py:40-41
    return pl.input_transform(x);
  };
  float s = a.s0[ji];
  const int T = a.T;
  const uint64_t key = a.key;
  const uint64_t ulane = (uint64_t)(a.lanes.lane_offset + lane);
  double racc = 0.0;
  float eacc = 0.f;
  const int o = t & 15;
  constexpr int kDrawsPerStep = DISC ? 1 : NA;
  constexpr int kStepsPerBatch = 32 / kDrawsPerStep;
  constexpr bool kTerm = (FEAT & kFeatTerm) != 0;
  bool alive0 = true, alive1 = true;  // wave-uniform: half 0 / half 1 still stepping (kTerm)
  int n0 = T, n1 = T;                 // their env.step counts
  auto alive_me = [&]() { return hh ? alive1 : alive0; };
  float rbuf = 0.f;
  // continuous: action dim d's mean sits in row thread d -- or, behind the reduce-scatter head (Lane::kHeadRS), in row
  // thread d + d / 3 (0, 1, 2, 4, 5, 6), its std pre-activation kStdShl threads above
  constexpr bool kRS = Lane::kHeadRS;
  constexpr int kStdShl = kRS ? 8 : NA;
  int zbase;
  if constexpr (kRS) zbase = 4 * (32 * hh + ((o < 8 && (o & 3) != 3) ? o - (o >> 2) : 0));
  else zbase = 4 * (32 * hh + (DISC ? 0 : (o < NA ? o : 0)));
  auto* sc = &scratch[wv];
  [[maybe_unused]] float* xs = sc->x[hh];
  float* h1s = sc->h1[hh];
  const float* mrow = envMK + ji * MKS;
  constexpr bool kSame = !DISC && !norm_obs;
  static_assert(!kXDump || kSame, "the select-free x write stores s itself");
  [[maybe_unused]] float* xw = xs + t;  // kXDump: where this thread's x write goes
  if constexpr (kXDump) {
    xs[t] = t < NIN ? s : (t == NIN ? 1.f : 0.f);  // the constant columns, once
    xw = t < NIN ? xs + t : sc->dump_slot(hh, t);
  }
  typename Lane::L1Rows l1rows;
  pl.l1_prefetch(l1rows, mrow);
  float kr[DISC ? 1 : NA];  // K row t: loop-invariant, kept in VGPRs
#pragma unroll
  for (int m = 0; m < (DISC ? 1 : NA); ++m) kr[m] = mrow[NX + m];
  int tb = 0;
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
  // draw batch starting at step st: thread t holds the draw of (step st + t / k, dim t % k)
  auto draw = [&](int st) {
    const int ds = t / kDrawsPerStep, dk = t % kDrawsPerStep;
    const uint64_t hsh = hash_ctr(key, ulane, (uint64_t)(st + ds), (uint64_t)dk);
    rbuf = DISC ? uniform24(hsh) : normal_bm(hsh);
  };
  // continuous: the batch after the running one is drawn in five parts, each in the x hand-off of one step of the
  // running batch -- its first four and its last (draw(st) = parts 0 .. 4 in order; the state between parts is dz,
  // then du1 / du2)
  int dctr = ((t / kDrawsPerStep) << 4) | (t % kDrawsPerStep);  // counter word bits of (step offset, dim)
  // FDR_PAIR_CTR_ADD: the counter word of batch 0's draw (step t / k, dim t % k); each draw_part(0) moves it on a batch
  [[maybe_unused]] uint64_t dword = 0;
  if constexpr (FDR_PAIR_CTR_ADD && !DISC) dword = hash_ctr_base(key, ulane, (uint32_t)dctr);
  [[maybe_unused]] constexpr uint64_t kBatchInc = (uint64_t)kStepsPerBatch * kCtrStepInc;
  uint64_t dz = 0;
  float du1 = 0.f, du2 = 0.f;
  auto draw_part = [&](int k, int st) {
    if (k == 0) {
#if FDR_PAIR_CTR_ADD
      // batches come in order from kStepsPerBatch on: st is the step the running word reaches here
      asm volatile("" : "+v"(dword)::"memory");
      dword += kBatchInc;
      dz = mix64_a(dword);
#else
      asm volatile("" : "+v"(dctr)::"memory");
      dz = mix64_a(key + (((uint64_t)ulane << 32) | (uint64_t)((st << 4) + dctr)) * kCtrMul);
#endif
    } else if (k == 1) {
      asm volatile("" : "+v"(dz)::"memory");
      dz = mix64_b(dz);
    } else if (k == 2) {
      asm volatile("" : "+v"(dz)::"memory");
      const uint64_t hsh = mix64_c(dz);
      du1 = bm_u1(hsh);
      du2 = bm_u2(hsh);
    } else if (k == 3) {
      asm volatile("" : "+v"(du1)::"memory");
      du1 = bm_radius(du1);
    } else if (k == 4) {
      asm volatile("" : "+v"(du1), "+v"(du2)::"memory");
      rbuf = bm_normal(du1, du2);
    }
  };
  auto step = [&](int st, int tb, auto&& fill) {
    // this step's draw: the uniform (discrete) or the normal of action dim o (continuous)
    const float zt = __builtin_bit_cast(
        float, __builtin_amdgcn_ds_bpermute(zbase + 4 * kDrawsPerStep * tb, __builtin_bit_cast(int, rbuf)));
    if constexpr (FEAT & kFeatStates) {
      if (t < NIN && active && (!kTerm || alive_me())) a.states[((int64_t)lane * T + st) * NIN + t] = s;
    }
    float pre = 0.f;
    if constexpr (kXDump) *xw = s;
    else xs[t] = t < NIN ? policy_input(s) : (t == NIN ? 1.f : 0.f);
    if constexpr (!kSame) h1s[t] = t < NIN ? s : 0.f;
    wave_lds_sync();
    typename Lane::SIn sin;
    const f2 h1 = pl.template layer1_env<kSame>(xs, h1s, l1rows, sin, fill);
    pre = pl.env_ms(sin, l1rows);

    mark(0, h1.x);
    const float y = pl.layers23(h1, h1s, t, mark);
    pl.l1_prefetch(l1rows, mrow);  // next step's rows, in flight during the action and env phases
    if constexpr (DISC) {
      const float p = det ? pl.softmax(y, t) : pl.template softmax<false, true>(y, t);
      float pv[NA];
      row_bcast_all(p, pv, std::make_integer_sequence<int, NA>{});  // pv[i] = p of output i
      float tot = 0.f;
#pragma unroll
      for (int i = 0; i < NA; ++i) tot += pv[i];
      int act_d = 0;
      if (det) {
        float best = pv[0];
#pragma unroll
        for (int i = 1; i < NA; ++i) {
          act_d = pv[i] > best ? i : act_d;
          best = fmaxf(best, pv[i]);
        }
      } else {
        const float target = zt * tot;
        float cs = 0.f;
#pragma unroll
        for (int i = 0; i < NA - 1; ++i) {
          cs += pv[i];
          act_d += cs <= target ? 1 : 0;
        }
      }
      eacc -= (o < NA && (!kTerm || alive_me())) ? disc_entropy_term(p, tot) : 0.f;
      pre += mrow[NX + act_d];
    } else {
      const float th = tanh_act<Lane::kPre>(y);
      const float sd = std_from_tanh(dpp_mov<kDppRowShl + kStdShl>(th));
      if constexpr (kTerm)
        eacc += alive_me() ? __builtin_amdgcn_logf(sd) : 0.f;
      else
        eacc += __builtin_amdgcn_logf(sd);
      const float act_c = det ? th : gauss_action(th, sd, zt);
      mark(3, act_c);
      // a[m] sits in thread m (kRS: m + m / 3) of both rows of the half
      if constexpr (kRS) dpp_tail_q3<NA>(pre, act_c, kr);
      else dpp_tail<NA>(pre, act_c, kr);
    }
    s = tanh_pre(pre);  // M, K stored x kPreScale
    mark(4, s);
    if constexpr (kTerm) {
      racc += alive_me() ? (double)s : 0.0;  // thread 0 of the half holds the reward s'[0]
      // done after this step (agent.py:50-52): the half's state element done_dim sits in its thread done_dim
      const bool d0 = fabsf(readlane_f(s, a.done_dim)) > a.done_thr;
      const bool d1 = fabsf(readlane_f(s, 32 + a.done_dim)) > a.done_thr;
      if (alive0 && d0) {
        alive0 = false;
        n0 = st + 1;
      }
      if (alive1 && d1) {
        alive1 = false;
        n1 = st + 1;
      }
      return !alive0 && !alive1;
    } else {
      racc += (double)s;  // thread 0 of the half holds the reward s'[0]
      return false;
    }
  };
  if constexpr (!DISC) {
    [&] {
      // continuous: the loop unrolled by the draw batch (5 steps for 6 dims); batch 0 is drawn here, every later
      // batch unconditionally during the batch before it (det lanes ignore the draws; the one drawn for steps >= T
      // is never used)
      int st = 0;
      draw(0);
      if constexpr (kXDump) {
        FDR_STEP_LOOP_PLACED(FDR_STEP_LOOP_PAD_DUMP)
      } else {
        FDR_STEP_LOOP_PLACED(FDR_STEP_LOOP_PAD_SEL)
      }
      for (; st + kStepsPerBatch <= T; st += kStepsPerBatch) {
        asm volatile("" ::: "memory");
        mark(-1, s);
#pragma unroll
        for (int k = 0; k < kStepsPerBatch; ++k) {
          if (k) {
            asm volatile("" ::: "memory");
            mark(-1, s);
          }
          // parts 0 - 3 in the batch's first four steps; part 4 writes rbuf, so it goes into the batch's last step,
          // after that step's zt -- rbuf's last read -- is taken
          constexpr int kLast = kStepsPerBatch - 1;
          static_assert(kLast >= 4, "draw_part: five parts need a batch of five steps");
          const int part = k == kLast ? 4 : (k < 4 ? k : -1);
          if (step(st + k, k, [&] { draw_part(part, st + kStepsPerBatch); })) return;  // kTerm: both halves done
        }
      }
      if (st < T) {  // the remainder's draws are the batch drawn ahead
        for (int k = 0; st + k < T; ++k) {
          asm volatile("" ::: "memory");
          mark(-1, s);
          if (step(st + k, k, [] {})) return;
        }
      }
    }();
  } else {
    for (int st = 0; st < T; ++st) {
      asm volatile("" ::: "memory");
      mark(-1, s);
      if (!det && tb == 0) draw(st);
      if (step(st, tb, [] {})) break;
      tb = tb + 1 == kStepsPerBatch ? 0 : tb + 1;
    }
  }

#ifdef FDR_PHASE_STAMPS
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int k = 0; k < 5; ++k) g_phase_stamps[k] = ph_acc[k];
#endif
  eacc *= 0.693147180559945309f;  // log2 -> ln (both kinds)
  double esum;  // row 0 of the half: one copy of each output
  if constexpr (kRS) esum = (t < 8 && (t & 3) != 3) ? (double)eacc : 0.0;
  else esum = (t < NA) ? (double)eacc : 0.0;
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) esum += __shfl_xor(esum, m, kWave);
  if (t == 0 && active) {
    double r = racc;
    if (a.jiggle) r += (hash_ctr(key, ulane, kJiggleT, 15) & 1ull) ? 1e-12 : -1e-12;
    a.ret[lane] = r;
    const int nsteps = hh ? n1 : n0;
    double e = esum / (double)nsteps;
    if constexpr (!DISC) e += (double)NA * 1.4189385332046727;
    a.ent[lane] = e;
    a.steps[lane] = nsteps;
  }
}

// More lanes than one resident round (2 waves per SIMD = 16 lanes per CU) go out as consecutive launches of
// equal rounds: one launch of two rounds lets early-finishing CUs start second-round workgroups while slow
// ones still run their first, and the last CUs' second round then runs alone at the end.
int launch_rollout_pair(const PolicyKey& k, const RolloutArgs& args, int round_lanes, hipStream_t stream) {
  return with_shape<false>(k, "no compiled rollout for this (kind, n_in, n_act)", [&](auto shape) {
    using S = decltype(shape);
    FDR_PHASE_UNIT();
    const int quantum = 2 * kPairWaves;
    const int n_rounds = round_lanes > 0 ? (args.n_lanes + round_lanes - 1) / round_lanes : 1;
    const int per = ((args.n_lanes + n_rounds - 1) / n_rounds + quantum - 1) / quantum * quantum;
    const int feat = rollout_feat(args, args.done_thr > 0.f);
    RolloutArgs r = args;
    for (int base = 0; base < args.n_lanes; base += per) {
      r.lane_base = base;
      const dim3 grid((std::min(per, args.n_lanes - base) + quantum - 1) / quantum), block(64 * kPairWaves);
      const bool hit = launch_feat_set<kPairFeatBits>(feat, [&](auto f) {
        hipLaunchKernelGGL((rollout_pair_kernel<S::NIN, S::NA, S::DISC, decltype(f)::value>), grid, block, 0, stream,
                           r);
      });
      if (!hit) return set_error(FDR_ERR_UNSUPPORTED, "no compiled rollout_pair_kernel for this feature set");
    }
    return check_launch("rollout_pair_kernel<synth>");
  });
}

}  // namespace fdr
