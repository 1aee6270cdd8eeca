// fdr_impala.hip -- ImpalaPolicy rollouts (policies/impala.py:8-186) on gfx950: the host side (parameter layout,
// workspace plans, pair-operand builder, step plan, launchers, profiler).  Kernels: fdr_impala_f32.hip (f32),
// fdr_impala_h.hip (fp16), fdr_pack.hip (the theta' pack, init, finish -- shared with AtariPolicy).
//
// Per rollout:   prep    theta'_l = fl32(theta + fl32(sigma * s_l * eps_l)) gathered once into a
//                        per-lane pack laid out for the kernels (+ |lambda_l|^2 partials)
// Per step t:    conv    one workgroup per (lane, env): synthetic frame -> 15 convs on f32 MFMA
//                        (v_mfma_f32_16x16x4_f32), activations LDS-resident, -> relu'd 2048 feature
//                core    one workgroup per lane (E envs): BN1d + fc + ReLU, LSTM cell, BN1d + head,
//                        softmax, action, synthetic reward, return
// After T steps: replay  the reference's entropy pass (worker/agent.py:60-66): the visited obs
//                        replayed through the LSTM from the end-of-episode state
//                finish  jiggle, mean entropy, steps, |lambda|^2
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "fdr_impala_kernels.h"

namespace fdr {
namespace impala {

constexpr int kCh[3] = {16, 32, 32};
constexpr uint64_t kFrameSalt = 0x4652414D45533031ull;  // oracle/impala.py FRAME_SALT
constexpr uint64_t kRewardSalt = 0x5245574152443031ull; // oracle/impala.py REWARD_SALT

// ------------------------------------------------------------------------------------------
// Host: pack layout.  Walks the reference's parameters() order (feat_convs, resnet1, resnet2,
// fc, core, policy -- policies/impala.py:60-119) and assigns every tensor a pack section.
// Conv / BN index = stage * 5 + part, part 0 = stage entry, 1/2 = resnet1 bn0+conv0 / bn1+conv1,
// 3/4 = resnet2; BN 15 = fc BN1d, 16 = head BN1d.  Running stats follow modules() order, which
// is the same walk.
// ------------------------------------------------------------------------------------------
static int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

bool make_layout(int n_act, Layout* L) {
  if (n_act < 1 || n_act > kMaxAct) return false;
  *L = Layout{};
  L->n_act = n_act;
  int32_t dst = 0, src = 0, stat = 0;
  auto add = [&](int32_t kind, int32_t len, int32_t a, int32_t b, int32_t src_len) {
    dst = (int32_t)round_up(dst, 16);  // 64-byte aligned sections: float4 streaming in the core kernel
    Section& s = L->sec[L->n_sections++];
    s = Section{dst, len, src, kind, a, b};
    const int32_t at = dst;
    dst += len;
    src += src_len;
    return at;
  };
  auto bn = [&](int idx, int ch) {
    L->bn_w[idx] = add(kCopy, 2 * ch, 0, 0, 2 * ch);  // weight then bias, contiguous in theta
    L->bn_b[idx] = L->bn_w[idx] + ch;
    L->bn_stat[idx] = stat;
    stat += ch;
  };
  auto conv = [&](int idx, int cin, int cout) {
    const int kpad = (int)round_up(9 * cin, 4);
    L->conv_w[idx] = add(kConvFrag, kpad * cout, cin, cout, 9 * cin * cout);
    L->conv_b[idx] = add(kCopy, cout, 0, 0, cout);
  };
  int cin = 3;
  for (int s = 0; s < 3; ++s) {  // feat_convs[s]: BN2d(cin), Conv2d(cin -> c)
    bn(s * 5, cin);
    conv(s * 5, cin, kCh[s]);
    cin = kCh[s];
  }
  for (int r = 0; r < 2; ++r)    // resnet1[s], resnet2[s]: (BN, ReLU, Conv) x 2
    for (int s = 0; s < 3; ++s)
      for (int j = 0; j < 2; ++j) {
        const int idx = s * 5 + 1 + 2 * r + j;
        bn(idx, kCh[s]);
        conv(idx, kCh[s], kCh[s]);
      }
  bn(15, kFeat);                                                   // fc[0] BatchNorm1d(2048)
  L->fc_wt = add(kTranspose, kFeat * kHid, kHid, kFeat, kFeat * kHid);  // fc[1].weight -> W^T
  L->fc_b = add(kCopy, kHid, 0, 0, kHid);
  L->lstm_wt = add(kTranspose, kCoreIn * kGates, kGates, kCoreIn, kCoreIn * kGates);  // W_ih^T
  add(kTranspose, kHid * kGates, kGates, kHid, kHid * kGates);                        // W_hh^T
  L->lstm_bih = add(kCopy, 2 * kGates, 0, 0, 2 * kGates);  // b_ih, b_hh
  L->lstm_bhh = L->lstm_bih + kGates;
  bn(16, kHid);                                                    // policy[0] BatchNorm1d(256)
  L->head_w = add(kCopy, n_act * kHid + n_act, 0, 0, n_act * kHid + n_act);  // weight, bias
  L->head_b = L->head_w + n_act * kHid;
  L->P = src;
  L->pack = round_up(dst, 64);
  L->n_bn_stats = stat;

  // half pack: walk the same source offsets again
  int32_t hdst = 0;
  auto hadd = [&](int32_t kind, int32_t len, int32_t a, int32_t b, int32_t s0) {
    hdst = (int32_t)round_up(hdst, 64);
    Section& h = L->hsec[L->n_hsections++];
    h = Section{hdst, len, s0, kind, a, b};
    const int32_t at = hdst;
    hdst += len;
    return at;
  };
  for (int i = 0; i < L->n_sections; ++i) {
    const Section& q = L->sec[i];
    if (q.kind == kConvFrag) {
      const int cin = q.a, cout = q.b;
      const int ks = cin == 3 ? 2 : (9 * cin + 31) / 32;      // k-steps of 32
      const int idx = [&] { for (int c = 0; c < kConvs; ++c) if (L->conv_w[c] == q.dst) return c; return -1; }();
      L->conv_h[idx] = hadd(kConvFragH, ks * (cout / 16) * 64 * 8, cin, cout, q.src);
    } else if (q.kind == kTranspose) {
      const int32_t at = hadd(kTranspose, q.len, q.a, q.b, q.src);
      if (q.dst == L->fc_wt) L->fc_wt_h = at;
      if (q.dst == L->lstm_wt) L->lstm_wt_h = at;
    }
  }
  L->hpack = round_up(hdst, 64);
  return true;
}

bool pair_core_supported(int envs) { return envs == 1 || envs == 2 || envs == 4; }

// The pair form's operand regions of n_lanes / 2 pairs (on = false: all empty), for the rollout's and the strategies'
// workspace alike
static PairOperands carve_pair_operands(Carver& ws, const Layout& L, int n_lanes, bool fp16, bool on) {
  PairOperands o{};
  const int64_t np = n_lanes / 2;
  const int64_t plen = fp16 ? L.hpack * 2 : L.pack * 4;  // one (half) pack in bytes
  o.zeros = ws.take(on ? L.P * 4 : 0);
  o.thpack = ws.take(on ? plen : 0);
  o.epack = ws.take(on ? np * plen : 0);
  o.idxe = ws.take(on ? np * 8 : 0);
  o.n2x = ws.take(on && !fp16 ? (np + 1) * prep_blocks(L) * 8 : 0);
  o.mimg = ws.take(on && fp16 ? (np + 1) * kMImg * 2 : 0);
  return o;
}

Plan plan(const Layout& L, int n_lanes, int envs, int T, bool entropy, bool fp16, bool pairs) {
  Plan p{};
  const int64_t ne = (int64_t)n_lanes * envs;
  Carver ws;
  p.nblk = prep_blocks(L);
  p.pack = ws.take((int64_t)n_lanes * L.pack * 4);
  p.hpack = ws.take(fp16 ? (int64_t)n_lanes * L.hpack * 2 : 0);
  p.feat = ws.take(ne * kFeat * 4);
  p.h = ws.take(ne * kHid * 4);
  p.c = ws.take(ne * kHid * 4);
  p.rprev = ws.take(ne * 4);
  p.ci = ws.take(entropy ? (int64_t)T * ne * kCoreIn * 4 : 0);
  p.gx = ws.take(entropy ? (int64_t)std::min(T, kReplayChunk) * ne * kGates * 4 : 0);
  p.n2 = ws.take((int64_t)n_lanes * p.nblk * 8);
  p.pair = carve_pair_operands(ws, L, n_lanes, fp16, pairs && pair_core_supported(envs));
  p.bntab = ws.take(fp16 ? (int64_t)n_lanes * 3 * kBnTab * 4 : 0);       // the conv stack's folded BN / bias tables
  p.total = ws.used;
  return p;
}

// Opt-in phase timing (fdr_ctx_impala_profile): HIP events between the launches of the step loop, so
// a caller (bench.py) can attribute the rollout's time to conv / core / replay kernels live.  One
// Profile per context.
struct Profile {
  bool on = false;
  std::vector<hipEvent_t> ev;
  int used = 0, T = 0, entropy = 0;
  hipEvent_t next() {
    if (used == (int)ev.size()) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) return nullptr;
      ev.push_back(e);
    }
    return ev[used++];
  }
};

void destroy_profile(Profile* p) {
  if (!p) return;
  for (hipEvent_t e : p->ev) (void)hipEventDestroy(e);
  delete p;
}

static void mark(Profile* p, hipStream_t s) {
  if (p && p->on) {
    hipEvent_t e = p->next();
    if (e) (void)hipEventRecord(e, s);
  }
}

int set_profile(Context& ctx, int on) {
  if (!ctx.prof) ctx.prof = new Profile();
  ctx.prof->on = on != 0;
  ctx.prof->used = 0;
  return FDR_OK;
}

int read_profile(Context& ctx, double* out) {
  out[0] = out[1] = out[2] = 0.0;
  Profile* p = ctx.prof;
  if (!p) return set_error(FDR_ERR_INVALID, "no profiled impala rollout");
  const int need = 2 * p->T + 1 + (p->entropy ? p->T : 0);
  if (!p->on || p->used < need) return set_error(FDR_ERR_INVALID, "no profiled impala rollout");
  if (hipEventSynchronize(p->ev[need - 1]) != hipSuccess) return set_error(FDR_ERR_HIP, "event sync failed");
  auto ms = [](hipEvent_t a, hipEvent_t b) { float v = 0.f; (void)hipEventElapsedTime(&v, a, b); return (double)v; };
  for (int t = 0; t < p->T; ++t) {
    out[0] += ms(p->ev[2 * t], p->ev[2 * t + 1]);
    out[1] += ms(p->ev[2 * t + 1], p->ev[2 * t + 2]);
  }
  for (int t = 0; p->entropy && t < p->T; ++t)
    out[2] += ms(p->ev[2 * p->T + t], p->ev[2 * p->T + t + 1]);
  return FDR_OK;
}

// the pairs' table offsets idx[2p] (fdr_impala_desc.pairs: idx[2p] == idx[2p+1] by contract)
// idxe[p] = the pair's shared offset.  A pair whose lanes disagree (fdr_impala_desc.pairs violated) would run lane
// 2p + 1 on lane 2p's noise: both lanes' norms are poisoned with NaN instead (slot 0 of their n2 partials, written by
// the lanes' pack kernels before this launch), as for an out-of-range offset.
__global__ void pair_offsets_kernel(const int64_t* __restrict__ idx, int n_pairs, int64_t* __restrict__ idxe,
                                    double* __restrict__ n2, int nblk) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  const int64_t o0 = idx[2 * p], o1 = idx[2 * p + 1];
  idxe[p] = o0;
  if (o0 != o1) {
    n2[(int64_t)(2 * p) * nblk] = __builtin_nan("");
    n2[(int64_t)(2 * p + 1) * nblk] = __builtin_nan("");
  }
}

// The pair form's operands, built by the pack kernels themselves: theta's pack (no table: theta' = theta) and per pair
// fl32(sigma eps) (a zero base, sign +1: fl32(0 + fl32(sigma eps))).  f32: w = fl32(theta +- fl32(sigma eps)) formed in
// registers is the per-lane pack's value bit for bit.  fp16: half packs, and from them the MFMA-fragment images of
// theta's and the pairs' fc / LSTM weights -- only the images read the pairs' packs (their transposed sections).
// n2: the lanes' norm partials (a pair whose offsets differ is poisoned there).
static void build_pair_operands(const Layout& L, const LanesArgs& lanes, int n_lanes, bool fp16, const PairOperands& po,
                                char* w, double* n2, hipStream_t stream, StepArgs& a) {
  const int np = n_lanes / 2, nblk = prep_blocks(L);
  float* zeros = reinterpret_cast<float*>(w + po.zeros);
  int64_t* idxe = reinterpret_cast<int64_t*>(w + po.idxe);
  (void)hipMemsetAsync(zeros, 0, (size_t)L.P * 4, stream);
  hipLaunchKernelGGL(pair_offsets_kernel, dim3((np + 255) / 256), dim3(256), 0, stream, lanes.idx, np, idxe, n2, nblk);
  LanesArgs lt = lanes;
  lt.table = nullptr;
  LanesArgs le = lanes;
  le.base = zeros;
  le.base_stride = 0;
  le.idx = idxe;
  le.sign = nullptr;
  if (fp16) {
    _Float16* th = reinterpret_cast<_Float16*>(w + po.thpack);
    _Float16* ep = reinterpret_cast<_Float16*>(w + po.epack);
    _Float16* im = reinterpret_cast<_Float16*>(w + po.mimg);
    launch_pack<_Float16>(L, lt, th, n2, 1, 1, stream);
    launch_pack<_Float16>(L, le, ep, n2, np, 1, stream, kTrFull, false);
    const unsigned nb = kFcKS + 4 * kGateKS;
    hipLaunchKernelGGL(mfma_image_kernel, dim3(nb, 1), dim3(256), 0, stream, L, th, (int64_t)0, im);
    hipLaunchKernelGGL(mfma_image_kernel, dim3(nb, np), dim3(256), 0, stream, L, ep, (int64_t)L.hpack, im + kMImg);
    a.th = th;
    a.ep = ep;
    a.ep_stride = L.hpack;
    a.thm = im;
    a.epm = im + kMImg;
  } else {
    float* th = reinterpret_cast<float*>(w + po.thpack);
    float* ep = reinterpret_cast<float*>(w + po.epack);
    double* n2x = reinterpret_cast<double*>(w + po.n2x);  // these packs' norms are not the lanes'
    launch_pack<float>(L, lt, th, n2x, 1, 0, stream);
    launch_pack<float>(L, le, ep, n2x + nblk, np, 0, stream);
    a.th32 = th;
    a.ep32 = ep;
    a.ep_stride = L.pack;
  }
  a.sign = lanes.sign;
}

// the fp16 conv stack over grid workgroups (one per env, XCD-interleaved lanes)
static void launch_conv_h(int grid, const Layout& L, const StepArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL((conv_kernel_h2<kHThreads>), dim3(grid), dim3(kHThreads), 0, stream, L, a);
}

// ------------------------------------------------------------------------------------------
// Step plan: which form of the LSTM core a call runs, decided once before its loops.
//
//   pair = the call built the pair operands (build_pair_operands): fdr_impala_desc.pairs, lanes on a shared base with a
//          noise table, E in {1, 2, 4} (the pair kernels have no E = 8 instance), fp16: n_lanes % 4 == 0
//   gemm = entropy && replay_gemm (fdr_ctx_set_replay_gemm, default on) && the gx workspace exists
//
//   core (every rollout step)      fp16  pair   kernel                          grid
//     kLane                         no    no    core_kernel<E, kRollout>        n_lanes
//     kPairF32                      no    yes   core_kernel_p<E>                n_lanes / 2
//     kLaneH                        yes   no    core_kernel_h<E, kRollout>      n_lanes
//     kPairMfma                     yes   yes   core_kernel_hpm2<E, kRollout>   n_lanes / 4
//   proj (entropy replay, per chunk of kReplayChunk steps: x W_ih^T as one GEMM)
//     kNone      !gemm                          (each replay step streams W_ih itself)
//     kF32       gemm, f32                      lstm_xproj_kernel<false>
//     kHalf      gemm, fp16, !pair              lstm_xproj_kernel<true>
//     kPairMfma  gemm, fp16, pair               xproj_pair_kernel<E, true>  (core inputs from a.ci16)
//   replay (entropy replay, per step -- kPairMfma: per chunk)
//     kLane      f32,  !(gemm && pair)          core_kernel<E, kReplay>         (with or without gx)
//     kPairF32   f32,  gemm && pair             core_kernel_pr<E>               (needs gx)
//     kLaneH     fp16, !(gemm && pair)          core_kernel_h<E, kReplay>       (with or without gx)
//     kPairMfma  fp16, gemm && pair             replay_chunk_hpm2<E, kReplay>   (needs gx)
//
// Without entropy, proj = kNone and replay is not run.  launch_strategies runs the replay half over its probe sequence
// (E = 1, always with the GEMM, kStrategy kernels): (kF32, kLane), (kHalf, kLaneH) or (kPairMfma, kPairMfma) with
// xproj_pair_kernel<1, false> (core inputs from the f32 rows a.ci).
// ------------------------------------------------------------------------------------------
enum class CoreForm { kLane, kPairF32, kLaneH, kPairMfma };
enum class ReplayProj { kNone, kF32, kHalf, kPairMfma };
struct StepPlan {
  CoreForm core;
  ReplayProj proj;
  CoreForm replay;
};
static StepPlan step_plan(bool fp16, bool pair, int E, bool entropy, bool replay_gemm, bool has_gx) {
  pair = pair && pair_core_supported(E);
  const bool gemm = entropy && replay_gemm && has_gx;
  StepPlan sp;
  sp.core = fp16 ? (pair ? CoreForm::kPairMfma : CoreForm::kLaneH) : (pair ? CoreForm::kPairF32 : CoreForm::kLane);
  sp.proj = !gemm ? ReplayProj::kNone : !fp16 ? ReplayProj::kF32 : pair ? ReplayProj::kPairMfma : ReplayProj::kHalf;
  sp.replay = gemm ? sp.core : (fp16 ? CoreForm::kLaneH : CoreForm::kLane);
  return sp;
}

// one rollout (MODE = kRollout) or replay (kReplay) step of every lane in form f; the pair forms exist for E <= 4 only
// (step_plan never chooses them otherwise); replay's kPairMfma runs a chunk at a time (launch_steps)
template <int E, int MODE>
static void launch_core(CoreForm f, const Layout& L, const StepArgs& a, hipStream_t stream) {
  const dim3 wg(kCoreThreads);
  switch (f) {
    case CoreForm::kLane:
      hipLaunchKernelGGL((core_kernel<E, MODE>), dim3(a.n_lanes), wg, 0, stream, L, a);
      break;
    case CoreForm::kLaneH:
      hipLaunchKernelGGL((core_kernel_h<E, MODE>), dim3(a.n_lanes), wg, 0, stream, L, a);
      break;
    case CoreForm::kPairF32:
      if constexpr (E <= 4 && MODE == kRollout)
        hipLaunchKernelGGL((core_kernel_p<E>), dim3(a.n_lanes / 2), wg, 0, stream, L, a);
      else if constexpr (E <= 4 && MODE == kReplay)
        hipLaunchKernelGGL((core_kernel_pr<E>), dim3(a.n_lanes / 2), wg, 0, stream, L, a);
      break;
    case CoreForm::kPairMfma:
      if constexpr (E <= 4 && MODE == kRollout)
        hipLaunchKernelGGL((core_kernel_hpm2<E, kRollout>), dim3(a.n_lanes / 4), dim3(2 * kCoreThreads), 0, stream, L,
                           a);
      break;
  }
}

template <int E>
static int launch_steps(const Context& ctx, const Layout& L, StepArgs a, const StepPlan& sp, int entropy,
                        hipStream_t stream) {
  const int conv_grid = (a.n_lanes + 7) / 8 * 8 * a.envs;
  Profile* prof = ctx.prof;
  if (prof) {
    prof->used = 0;
    prof->T = a.T;
    prof->entropy = entropy;
  }
  mark(prof, stream);
  for (int t = 0; t < a.T; ++t) {
    a.t = t;
    if (a.hpack)
      launch_conv_h(conv_grid, L, a, stream);
    else
      hipLaunchKernelGGL(conv_kernel, dim3(conv_grid), dim3(kConvThreads), 0, stream, L, a);
    mark(prof, stream);
    launch_core<E, kRollout>(sp.core, L, a, stream);
    mark(prof, stream);
  }
  float* gx = const_cast<float*>(a.gx);
  a.gx = nullptr;
  if (entropy)
    for (int t0 = 0; t0 < a.T; t0 += kReplayChunk) {
      const int tc = std::min(kReplayChunk, a.T - t0);
      const dim3 grid(a.n_lanes, (tc * E + 63) / 64, kGates / 256);
      switch (sp.proj) {
        case ReplayProj::kNone:
          break;
        case ReplayProj::kF32:
          hipLaunchKernelGGL(lstm_xproj_kernel<false>, grid, dim3(256), 0, stream, L, a, t0, tc, gx);
          break;
        case ReplayProj::kHalf:
          hipLaunchKernelGGL(lstm_xproj_kernel<true>, grid, dim3(256), 0, stream, L, a, t0, tc, gx);
          break;
        case ReplayProj::kPairMfma:  // theta X + s (E X) from the gate images
          if constexpr (E <= 4)
            hipLaunchKernelGGL((xproj_pair_kernel<E, true>), xproj_grid(a.n_lanes), dim3(256), 0, stream, L, a, t0, tc,
                               gx);
          break;
      }
      if (sp.proj != ReplayProj::kNone) {
        a.gx = gx;
        a.gx_t0 = t0;
      }
      if (sp.replay == CoreForm::kPairMfma) {  // the whole chunk in one launch
        if constexpr (E <= 4)
          hipLaunchKernelGGL((replay_chunk_hpm2<E, kReplay>), dim3(a.n_lanes / 4), dim3(2 * kCoreThreads), 0, stream, L,
                             a, t0, tc);
        for (int t = t0; t < t0 + tc; ++t) mark(prof, stream);  // the profiler's per-step marks
        continue;
      }
      for (int t = t0; t < t0 + tc; ++t) {
        a.t = t;
        launch_core<E, kReplay>(sp.replay, L, a, stream);
        mark(prof, stream);
      }
    }
  return check_launch("impala step kernels");
}

int launch_rollout(const RolloutCall& c, void* ws, int64_t ws_bytes, hipStream_t stream) {
  const Layout& L = *c.layout;
  const Plan p = plan(L, c.n_lanes, c.envs, c.T, c.entropy != 0, c.fp16 != 0, c.pairs != 0);
  if (!ws || ws_bytes < p.total) return set_error(FDR_ERR_WORKSPACE, "impala workspace too small");
  if (c.n_lanes == 0) return FDR_OK;
  char* w = static_cast<char*>(ws);
  StepArgs a{};
  a.pack = reinterpret_cast<float*>(w + p.pack);
  a.pack_stride = L.pack;
  a.bn_mean = c.bn_mean;
  a.bn_var = c.bn_var;
  a.n_lanes = c.n_lanes;
  a.envs = c.envs;
  a.n_act = L.n_act;
  a.T = c.T;
  a.lane_offset = c.lanes.lane_offset;
  a.fkey = mix64(c.env_seed ^ kFrameSalt);
  a.rkey = mix64(c.env_seed ^ kRewardSalt);
  a.akey = mix64(c.seed);
  a.feat = reinterpret_cast<float*>(w + p.feat);
  a.h = reinterpret_cast<float*>(w + p.h);
  a.c = reinterpret_cast<float*>(w + p.c);
  a.rprev = reinterpret_cast<float*>(w + p.rprev);
  a.ci = c.entropy ? reinterpret_cast<float*>(w + p.ci) : nullptr;
  a.gx = c.entropy ? reinterpret_cast<float*>(w + p.gx) : nullptr;  // launch_steps hands it to the replay
  a.ret = c.ret;
  a.ent = c.ent;
  a.actions = c.actions;
  a.probs = c.probs;
  a.deterministic = c.lanes.deterministic;
  a.dbg = c.ctx->debug_clock;
  double* n2 = reinterpret_cast<double*>(w + p.n2);

  // fp16: the MFMA pair core takes two pairs per workgroup (n_lanes % 4 == 0); other lane counts run per lane
  const bool pair_core = c.pairs && pair_core_supported(c.envs) && c.lanes.table && c.lanes.base_stride == 0 &&
                         c.n_lanes >= 2 && (!c.fp16 || c.n_lanes % 4 == 0);
  const StepPlan sp =
      step_plan(c.fp16 != 0, pair_core, c.envs, c.entropy != 0, c.ctx->replay_gemm != 0, a.gx != nullptr);
  launch_pack<float>(L, c.lanes, const_cast<float*>(a.pack), n2, c.n_lanes, 0, stream, c.fp16 ? kTrNorm : kTrFull);
  if (c.fp16) {
    a.hpack = reinterpret_cast<_Float16*>(w + p.hpack);
    a.hpack_stride = L.hpack;
    // the per-lane half pack's fc / LSTM weights are read only off the MFMA pair path: by core_kernel_h (rollout or
    // replay in the kLaneH form) and lstm_xproj_kernel<true> (kHalf)
    const bool pair_images = sp.core == CoreForm::kPairMfma && (!c.entropy || sp.replay == CoreForm::kPairMfma);
    launch_pack<_Float16>(L, c.lanes, a.hpack, n2, c.n_lanes, 1, stream, pair_images ? kTrSkip : kTrFull);
  }
  if (pair_core) build_pair_operands(L, c.lanes, c.n_lanes, c.fp16 != 0, p.pair, w, n2, stream, a);
  if (sp.proj == ReplayProj::kPairMfma) {  // core inputs as f16 rows for xproj_pair_kernel<E, true> (the ci space)
    a.ci16 = reinterpret_cast<_Float16*>(a.ci);
    a.ci = nullptr;
  }
  if (c.fp16) {  // the lanes' BN / bias tables, folded once per rollout (r12: conv launch -1.4 %, same box)
    float* tab = reinterpret_cast<float*>(w + p.bntab);
    hipLaunchKernelGGL(bn_table_kernel, dim3(c.n_lanes), dim3(256), 0, stream, L, a, tab);
    a.bntab = tab;
  }
  const int64_t ne = (int64_t)c.n_lanes * c.envs;
  hipLaunchKernelGGL(init_kernel, dim3((unsigned)((ne * kHid + 255) / 256)), dim3(256), 0, stream, ne, a.h, a.c,
                     a.rprev, a.ret, a.ent);
  int rc = check_launch("impala prep/init");
  if (rc) return rc;
  switch (c.envs) {
    case 1: rc = launch_steps<1>(*c.ctx, L, a, sp, c.entropy, stream); break;
    case 2: rc = launch_steps<2>(*c.ctx, L, a, sp, c.entropy, stream); break;
    case 4: rc = launch_steps<4>(*c.ctx, L, a, sp, c.entropy, stream); break;
    case 8: rc = launch_steps<8>(*c.ctx, L, a, sp, c.entropy, stream); break;
    default: return set_error(FDR_ERR_UNSUPPORTED, "envs_per_lane must be 1, 2, 4 or 8");
  }
  if (rc) return rc;
  const int64_t nmax = std::max<int64_t>(ne, c.n_lanes);
  hipLaunchKernelGGL(finish_kernel, dim3((unsigned)((nmax + 255) / 256)), dim3(256), 0, stream, c.n_lanes, c.envs,
                     c.T, c.entropy, c.jiggle, a.akey, c.lanes.lane_offset, n2, p.nblk, c.ret, c.ent, c.steps,
                     c.norm2);
  return check_launch("impala finish");
}

int64_t forward_workspace_bytes(const Layout& L, int n_envs, bool fp16) {
  const Plan p = plan(L, 1, std::max(n_envs, 0), 0, false, fp16);
  return p.total;
}

int launch_forward(const ForwardCall& c, void* ws, int64_t ws_bytes, hipStream_t stream) {
  const Layout& L = *c.layout;
  const Plan p = plan(L, 1, c.n_envs, 0, false, c.fp16 != 0);
  if (!ws || ws_bytes < p.total) return set_error(FDR_ERR_WORKSPACE, "impala forward workspace too small");
  if (c.n_envs == 0) return FDR_OK;
  char* w = static_cast<char*>(ws);
  LanesArgs lanes{};
  lanes.base = c.theta;
  StepArgs a{};
  a.pack = reinterpret_cast<float*>(w + p.pack);
  a.pack_stride = 0;  // every env shares the one pack
  a.bn_mean = c.bn_mean;
  a.bn_var = c.bn_var;
  a.n_lanes = c.n_envs;
  a.envs = 1;
  a.n_act = L.n_act;
  a.frames = c.frames;
  a.feat = c.feat_out ? c.feat_out : reinterpret_cast<float*>(w + p.feat);
  a.h = c.h;
  a.c = c.c;
  a.probs = c.probs;
  a.reward_in = c.reward;
  a.notdone = c.notdone;
  launch_pack<float>(L, lanes, const_cast<float*>(a.pack), reinterpret_cast<double*>(w + p.n2), 1, 0, stream);
  if (c.fp16) {
    a.hpack = reinterpret_cast<_Float16*>(w + p.hpack);
    a.hpack_stride = 0;
    launch_pack<_Float16>(L, lanes, a.hpack, reinterpret_cast<double*>(w + p.n2), 1, 1, stream);
  }
  if (c.fp16) {
    launch_conv_h((c.n_envs + 7) / 8 * 8, L, a, stream);
    hipLaunchKernelGGL((core_kernel_h<1, kForward>), dim3(c.n_envs), dim3(kCoreThreads), 0, stream, L, a);
  } else {
    hipLaunchKernelGGL(conv_kernel, dim3((c.n_envs + 7) / 8 * 8), dim3(kConvThreads), 0, stream, L, a);
    hipLaunchKernelGGL((core_kernel<1, kForward>), dim3(c.n_envs), dim3(kCoreThreads), 0, stream, L, a);
  }
  return check_launch("impala forward");
}


// ------------------------------------------------------------------------------------------
// get_strategy over a probe set zeta (policies/impala.py:24-27 -> ImpalaCNN.forward :136-186): the Z
// stacked obs are ONE batch_first LSTM sequence per lane (B = 1, T = Z), so per lane the conv stack runs
// on Z shared frames (conv kernel, shared_frames), the fc is one GEMM over the Z feature rows
// (fc_rows_kernel below), the LSTM input projection one GEMM per 64-step chunk (lstm_xproj_kernel) and
// the recurrence + head one core-kernel launch per step (kStrategy: probabilities out).
// ------------------------------------------------------------------------------------------
namespace {
struct StratPlan {
  int64_t pack, hpack, feat, ci, gx, h, c, n2, total;
  PairOperands pair;
  int nblk;
};
// pairs (fp16): the rollout's pair form operands
StratPlan strat_plan(const Layout& L, int n_lanes, int Z, bool fp16, bool pairs = false) {
  StratPlan p{};
  Carver ws;
  const int zc = std::min(Z, kReplayChunk);
  p.nblk = prep_blocks(L);
  p.pack = ws.take((int64_t)n_lanes * L.pack * 4);
  p.hpack = ws.take(fp16 ? (int64_t)n_lanes * L.hpack * 2 : 0);
  p.feat = ws.take((int64_t)n_lanes * zc * kFeat * 4);
  p.ci = ws.take((int64_t)Z * n_lanes * kCoreIn * 4);
  p.gx = ws.take((int64_t)zc * n_lanes * kGates * 4);
  p.h = ws.take((int64_t)n_lanes * kHid * 4);
  p.c = ws.take((int64_t)n_lanes * kHid * 4);
  p.n2 = ws.take((int64_t)n_lanes * p.nblk * 8);
  p.pair = carve_pair_operands(ws, L, n_lanes, fp16, pairs && fp16);
  p.total = ws.used;
  return p;
}
}  // namespace

int64_t strategies_workspace_bytes(const Layout& L, int n_lanes, int n_states, bool fp16, bool pairs) {
  return strat_plan(L, n_lanes, n_states, fp16, pairs).total;
}

// The pair form ran lane 2p + 1 on lane 2p's noise: a pair whose offsets differ has no defined result, so both lanes'
// probabilities become NaN (the rollout's pair form poisons their norms the same way, pair_offsets_kernel)
__global__ void poison_pair_probs_kernel(const int64_t* __restrict__ idx, int64_t per_lane, float* __restrict__ probs) {
  const int p = blockIdx.x;
  if (idx[2 * p] == idx[2 * p + 1]) return;
  float* q = probs + (int64_t)2 * p * per_lane;
  for (int64_t e = threadIdx.x; e < 2 * per_lane; e += blockDim.x) q[e] = __builtin_nanf("");
}

int launch_strategies(const StrategiesCall& c, void* ws, int64_t ws_bytes, hipStream_t stream) {
  const Layout& L = *c.layout;
  const int Z = c.n_states;
  const StratPlan p = strat_plan(L, c.n_lanes, Z, c.fp16 != 0, c.pairs != 0);
  if (!ws || ws_bytes < p.total) return set_error(FDR_ERR_WORKSPACE, "impala strategies workspace too small");
  if (c.n_lanes == 0 || Z == 0) return FDR_OK;
  char* w = static_cast<char*>(ws);
  const bool half = c.fp16 != 0;
  StepArgs a{};
  a.pack = reinterpret_cast<float*>(w + p.pack);
  a.pack_stride = L.pack;
  a.bn_mean = c.bn_mean;
  a.bn_var = c.bn_var;
  a.n_lanes = c.n_lanes;
  a.n_act = L.n_act;
  a.T = Z;
  a.shared_frames = 1;
  a.reward_in = c.reward;
  a.feat = reinterpret_cast<float*>(w + p.feat);
  a.ci = reinterpret_cast<float*>(w + p.ci);
  a.h = c.h ? c.h : reinterpret_cast<float*>(w + p.h);
  a.c = c.c ? c.c : reinterpret_cast<float*>(w + p.c);
  a.probs = c.probs;
  double* n2 = reinterpret_cast<double*>(w + p.n2);
  launch_pack<float>(L, c.lanes, const_cast<float*>(a.pack), n2, c.n_lanes, 0, stream, half ? kTrSkip : kTrFull);
  if (half) {
    a.hpack = reinterpret_cast<_Float16*>(w + p.hpack);
    a.hpack_stride = L.hpack;
    launch_pack<_Float16>(L, c.lanes, a.hpack, n2, c.n_lanes, 1, stream);
  }
  // antithetic pairs (fp16): the recurrence streams each pair's sigma-eps image once (replay_chunk_hpm2<1, kStrategy>,
  // x W_ih^T by xproj_pair_kernel), as the rollout's pair form -- conv and fc stay per lane (per-lane half pack)
  const bool pair_form = half && c.pairs && c.n_lanes % 4 == 0 && c.lanes.table &&
                         c.lanes.base_stride == 0;
  if (pair_form) build_pair_operands(L, c.lanes, c.n_lanes, true, p.pair, w, n2, stream, a);
  // the sequence is the replay half of a step plan, always through the input-projection GEMM
  const StepPlan sp = step_plan(half, pair_form, 1, true, true, true);
  if (!c.h || !c.c) {  // the reset state (worker/agent.py:66 resets the policy before compute_novelty)
    if (hipMemsetAsync(a.h, 0, (size_t)c.n_lanes * kHid * 4, stream) != hipSuccess ||
        hipMemsetAsync(a.c, 0, (size_t)c.n_lanes * kHid * 4, stream) != hipSuccess)
      return set_error(FDR_ERR_HIP, "memset of the initial LSTM state failed");
  }
  for (int z0 = 0; z0 < Z; z0 += kReplayChunk) {
    const int zc = std::min(kReplayChunk, Z - z0);
    a.envs = zc;
    a.frames = c.frames + (int64_t)z0 * kFramePix;
    const int conv_grid = (c.n_lanes + 7) / 8 * 8 * zc;
    if (half)
      launch_conv_h(conv_grid, L, a, stream);
    else
      hipLaunchKernelGGL(conv_kernel, dim3(conv_grid), dim3(kConvThreads), 0, stream, L, a);
    const dim3 grid(c.n_lanes, (zc + 63) / 64);
    if (half)
      hipLaunchKernelGGL(fc_rows_kernel<true>, grid, dim3(256), 0, stream, L, a, z0, zc);
    else
      hipLaunchKernelGGL(fc_rows_kernel<false>, grid, dim3(256), 0, stream, L, a, z0, zc);
  }
  a.envs = 1;
  float* gx = reinterpret_cast<float*>(w + p.gx);
  for (int t0 = 0; t0 < Z; t0 += kReplayChunk) {
    const int tc = std::min(kReplayChunk, Z - t0);
    const dim3 grid(c.n_lanes, (tc + 63) / 64, kGates / 256);
    a.gx = nullptr;
    switch (sp.proj) {
      case ReplayProj::kPairMfma:
        hipLaunchKernelGGL((xproj_pair_kernel<1, false>), xproj_grid(c.n_lanes), dim3(256), 0, stream, L, a, t0, tc,
                           gx);
        break;
      case ReplayProj::kHalf:
        hipLaunchKernelGGL(lstm_xproj_kernel<true>, grid, dim3(256), 0, stream, L, a, t0, tc, gx);
        break;
      default:
        hipLaunchKernelGGL(lstm_xproj_kernel<false>, grid, dim3(256), 0, stream, L, a, t0, tc, gx);
    }
    a.gx = gx;
    a.gx_t0 = t0;
    if (sp.replay == CoreForm::kPairMfma) {  // the chunk's sequence steps in one launch
      hipLaunchKernelGGL((replay_chunk_hpm2<1, kStrategy>), dim3(c.n_lanes / 4), dim3(2 * kCoreThreads), 0, stream, L,
                         a, t0, tc);
      continue;
    }
    for (int t = t0; t < t0 + tc; ++t) {
      a.t = t;
      launch_core<1, kStrategy>(sp.replay, L, a, stream);
    }
  }
  if (pair_form)
    hipLaunchKernelGGL(poison_pair_probs_kernel, dim3(c.n_lanes / 2), dim3(256), 0, stream, c.lanes.idx,
                       (int64_t)Z * L.n_act, c.probs);
  return check_launch("impala strategies");
}

// ------------------------------------------------------------------------------------------
// The synthetic frame env's observations outside a rollout (eval states / the probe set zeta,
// run_sequential.py:142-143, 198-213): frame_t of env `env_id` (the conv kernel's generator) and, given
// the actions taken, the reward each step returns.  One workgroup per step.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void env_frames_kernel(uint64_t fkey, uint64_t rkey, int n_act, uint64_t env_id,
                                                         int t0, const int32_t* actions, float* frames,
                                                         float* reward) {
  const int i = blockIdx.x, t = t0 + i;
  float* fr = frames + (int64_t)i * kFramePix;
  for (int w = threadIdx.x; w < kFramePix / 8; w += blockDim.x) {
    const uint64_t hb = mix64(fkey + ((env_id << 32) | ((uint64_t)t << 11) | (uint64_t)w) * kGolden);
#pragma unroll
    for (int j = 0; j < 8; ++j) fr[8 * w + j] = (float)((uint32_t)(hb >> (8 * j)) & 255u);
  }
  if (threadIdx.x == 0 && reward) {
    float r = 0.f;
    if (actions) {
      const int tgt = (int)((mix64(rkey + ((env_id << 32) | ((uint64_t)t << 11)) * kGolden) >> 40) % (uint64_t)n_act);
      const int act = actions[i];
      r = act == tgt ? 1.f : (act == (tgt + 1) % n_act ? -1.f : 0.f);
    }
    reward[i] = r;
  }
}

int launch_env_frames(uint64_t env_seed, int n_act, uint64_t env_id, int t0, int n, const int32_t* actions,
                      float* frames, float* reward, hipStream_t stream) {
  if (n == 0) return FDR_OK;
  hipLaunchKernelGGL(env_frames_kernel, dim3(n), dim3(256), 0, stream, mix64(env_seed ^ kFrameSalt),
                     mix64(env_seed ^ kRewardSalt), n_act, env_id, t0, actions, frames, reward);
  return check_launch("impala env frames");
}

}  // namespace impala
}  // namespace fdr
