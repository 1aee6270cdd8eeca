// fdr_impala_core.h -- the shared phases of the ImpalaPolicy core step
//   BN1d(features) -> fc -> relu -> [x | clip(r)] -> LSTM gates -> cell -> BN1d(h') -> head -> core_finish
// (policies/impala.py:161-184) for the six core kernels of fdr_impala_f32.hip and fdr_impala_h.hip.  The kernels keep
// their LDS plans, thread roles and weight streams; what every form must compute alike -- the cell, the BN1d fold, the
// head dot product, the pair operands -- is written here once.  Who uses which piece, and how: DESIGN.md.
#pragma once
#include "fdr_impala_kernels.h"

namespace fdr {
namespace impala {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// ---- LSTM cell (torch gate order i, f, g, o) -----------------------------------------------------------------------
// c <- f c + i g, h = o tanh(c) from the four gate pre-activations p0 .. p3, with sigmoid SIG and tanh TANH.  The
// arithmetic exists here once; lstm_cell is its function form, and core_kernel_p / _pr, which read each pre-activation
// from LDS where the cell uses it, expand the macro in place (inside a block: it declares gi, gf, gg, go).
#define FDR_LSTM_CELL(SIG, TANH, p0, p1, p2, p3, c, h)                                       \
  const float gi = SIG(p0);                                                                  \
  const float gf = SIG(p1);                                                                  \
  const float gg = TANH(p2);                                                                 \
  const float go = SIG(p3);                                                                  \
  c = fmaf(gf, c, gi * gg); /* explicit: the same rounding in every core form */             \
  h = go * TANH(c);
__device__ __forceinline__ float sigm_fast(float x) {
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.44269504088896341f * x));
}
// FAST (the fp16 MFMA forms): sigmoid as rcp(1 + exp2(-log2e x)) and tanh_fast; otherwise sigm / tanhf
template <bool FAST>
__device__ __forceinline__ float lstm_cell(const float (&pre)[4], float& c) {
  float h;
  if constexpr (FAST) {
    FDR_LSTM_CELL(sigm_fast, tanh_fast, pre[0], pre[1], pre[2], pre[3], c, h)
  } else {
    FDR_LSTM_CELL(sigm, tanhf, pre[0], pre[1], pre[2], pre[3], c, h)
  }
  return h;
}

// ---- eval-mode BN1d folded per element: y = x sc + sh, sc = w / sqrt(rv + eps), sh = b - rm sc ---------------------
// The running statistics of element k of BN layer i (15: the fc's, 16: the head's) are the same for every lane, the
// affine part (w, b) is each lane's pack: a pair kernel loads the statistics once and folds per lane.  As for the cell,
// the two formulas exist once, as macros that the functions below and the benchmarked kernels both expand.
// FDR_BN1D_STATS declares rm, rv, loaded branch-free: both loads are unconditional -- without running statistics they
// read `valid` (any address that holds k readable floats, e.g. the pack) and the values are replaced by 0 / 1 after.  A
// conditional load ends its basic block with a full vmcnt wait.
#define FDR_BN1D_STATS(i, k, valid, rm, rv)                                                  \
  const float rm##v = (a.bn_mean ? a.bn_mean + L.bn_stat[i] : valid)[k];                     \
  const float rv##v = (a.bn_var ? a.bn_var + L.bn_stat[i] : valid)[k];                       \
  const float rm = a.bn_mean ? rm##v : 0.f, rv = a.bn_var ? rv##v : 1.f;
#define FDR_BN1D_FOLD(w, b, rm, rv, sc, sh)      \
  sc = (w) * (1.f / sqrtf((rv) + kBnEps)); \
  sh = fmaf(-(rm), sc, (b));
struct Bn1dStats { float rm, rv; };
__device__ __forceinline__ Bn1dStats bn1d_stats(const Layout& L, const StepArgs& a, int i, int k, const float* valid) {
  FDR_BN1D_STATS(i, k, valid, rm, rv)
  return Bn1dStats{rm, rv};
}
__device__ __forceinline__ void bn1d_fold(const Layout& L, const float* pk, int i, int k, Bn1dStats s, float& sc,
                                          float& sh) {
  FDR_BN1D_FOLD(pk[L.bn_w[i] + k], pk[L.bn_b[i] + k], s.rm, s.rv, sc, sh)
}

// ---- policy head Linear(256 -> A) (policies/impala.py:122, 184) ---------------------------------------------------
// logit[e][ai] = b[ai] + sum_k W[ai][k] hs[k][e] for the NE envs of a workgroup (hs [k][NE]).
// head_rows: one thread per logit, the 256 FMAs in k order (the VALU kernels).  Env e < E reads lane pack pk0, the
// others pk1 (a per-lane kernel: NE == E, pk0 alone).
template <int E, int NE>
__device__ __forceinline__ void head_rows(const float* pk0, const float* pk1, const Layout& L, int A,
                                          const float* hs, float* logit) {
  const int j = threadIdx.x;
  if (j < A * NE) {
    const int ai = j / NE, e = j - ai * NE;
    const float* pk = e < E ? pk0 : pk1;
    const float* w = pk + L.head_w + ai * kHid;
    float s = 0.f;
    for (int k = 0; k < kHid; ++k) s = fmaf(w[k], hs[k * NE + e], s);
    logit[e * kMaxAct + ai] = s + pk[L.head_b + ai];
  }
}
// head_split: the same logits split over 512 threads -- P parts of 256 / P inputs each, the parts added in part order
// (P = 8 at A * NE <= 64).  (One wave walking the 256 dependent FMAs per logit left the other seven waiting at the next
// barrier.)
template <int E, int NE>
__device__ __forceinline__ void head_split(const float* pack, int64_t pack_stride, int l0, const Layout& L, int A,
                                           const float* hs, float* part, float* logit) {
  const int j = threadIdx.x, nl = A * NE;
  const int parts = nl <= 64 ? 8 : (nl <= 128 ? 4 : (nl <= 256 ? 2 : 1));
  const int kn = kHid / parts;
  if (j < parts * nl) {
    const int pi = j / nl, r = j - pi * nl, ai = r / NE, e = r - ai * NE;
    const float* wh = pack + (int64_t)(l0 + e / E) * pack_stride + L.head_w + ai * kHid + pi * kn;
    const float* hp = hs + (pi * kn) * NE + e;
    float s = 0.f;
    for (int k = 0; k < kn; ++k) s = fmaf(wh[k], hp[k * NE], s);
    part[j] = s;
  }
  __syncthreads();
  if (j < nl) {
    const int ai = j / NE, e = j - ai * NE;
    float s = part[j];
    for (int pi = 1; pi < parts; ++pi) s += part[pi * nl + j];
    logit[e * kMaxAct + ai] = s + pack[(int64_t)(l0 + e / E) * pack_stride + L.head_b + ai];
  }
}

// ---- core-input rows and the carried state (the per-lane kernels; the f32 pair step stores rows too) ---------------
// a.ci holds each step's core inputs as rows [t][env][kCoreIn]; in LDS they are cis [k][NE], transposed.
template <int E>  // E: envs per lane; the row of env e0 at step a.t
__device__ __forceinline__ float* ci_step(const StepArgs& a, int64_t e0) {
  return a.ci + ((int64_t)a.t * a.n_lanes * E + e0) * kCoreIn;
}
template <int NE>
__device__ __forceinline__ void store_ci_rows(float* dst, const float* cis) {
  for (int i = threadIdx.x; i < kCoreIn * NE; i += kCoreThreads) {
    const int e = i / kCoreIn, k = i - e * kCoreIn;
    dst[i] = cis[k * NE + e];
  }
}
template <int NE>
__device__ __forceinline__ void load_ci_rows(const float* src, float* cis) {
  for (int i = threadIdx.x; i < kCoreIn * NE; i += kCoreThreads) {
    const int e = i / kCoreIn, k = i - e * kCoreIn;
    cis[k * NE + e] = src[i];
  }
}
// h of unit j into hs [k][E], c into registers; the forward API's done mask zeroes both (policies/impala.py:170-176)
template <int E, int MODE>
__device__ __forceinline__ void load_state(const StepArgs& a, int64_t e0, int j, float* hs, float (&cj)[E]) {
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const float nd = (MODE == kForward && a.notdone) ? a.notdone[e0 + e] : 1.f;
    hs[j * E + e] = nd * a.h[(e0 + e) * kHid + j];
    cj[e] = nd * a.c[(e0 + e) * kHid + j];
  }
}

// ---- f32 pair operands (core_kernel_p, core_kernel_pr) -------------------------------------------------------------
// Lanes 2p, 2p + 1 of an antithetic pair share theta and their fl32(sigma eps) pack ep; a streamed weight is
// w_l = fmaf(s_l, d, t) per lane -- the per-lane pack's value bit for bit (an fma with s = +-1 rounds theta +- E once),
// so every env sees core_kernel's fma chains.  The pair's 2E envs are contiguous: env e < E is lane 2p's.  Biases, BN
// and head are each lane's own pack (pk0, pk1).
template <int E>
struct PairF32 {
  static constexpr int E2 = 2 * E;
  const float* pk0;
  const float* pk1;
  const float* ep;
  float sg0, sg1;  // the lanes' signs (1 without a.sign); an aggregate: each kernel loads these in its own way
  // one streamed float4 row (t of theta, d of sigma eps): w per lane, then each env's fma chain of core_kernel
  __device__ __forceinline__ void accum(float (&acc)[4][E2], float4 t, float4 d, const float* x) const {
    const float tp[4] = {fmaf(sg0, d.x, t.x), fmaf(sg0, d.y, t.y), fmaf(sg0, d.z, t.z), fmaf(sg0, d.w, t.w)};
    const float tm[4] = {fmaf(sg1, d.x, t.x), fmaf(sg1, d.y, t.y), fmaf(sg1, d.z, t.z), fmaf(sg1, d.w, t.w)};
#pragma unroll
    for (int e = 0; e < E2; ++e) {
      const float xv = x[e];
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c][e] = fmaf(e < E ? tp[c] : tm[c], xv, acc[c][e]);
    }
  }
  // b_ih / b_hh of gate columns 4j .. 4j + 3 for the two lanes, and the gate pre-activation of env e, column c:
  // (x part + b_ih) + (h part + b_hh) with the env's lane's biases
  struct GateBias {
    float bi[2][4], bh[2][4];
  };
  __device__ __forceinline__ GateBias gate_bias(const Layout& L, int j) const {
    const float4 bi0 = reinterpret_cast<const float4*>(pk0 + L.lstm_bih)[j];
    const float4 bh0 = reinterpret_cast<const float4*>(pk0 + L.lstm_bhh)[j];
    const float4 bi1 = reinterpret_cast<const float4*>(pk1 + L.lstm_bih)[j];
    const float4 bh1 = reinterpret_cast<const float4*>(pk1 + L.lstm_bhh)[j];
    return GateBias{{{bi0.x, bi0.y, bi0.z, bi0.w}, {bi1.x, bi1.y, bi1.z, bi1.w}},
                    {{bh0.x, bh0.y, bh0.z, bh0.w}, {bh1.x, bh1.y, bh1.z, bh1.w}}};
  }
  __device__ __forceinline__ static float gate_pre(const GateBias& b, int c, int e, float x, float h) {
    return (x + (e < E ? b.bi[0][c] : b.bi[1][c])) + (h + (e < E ? b.bh[0][c] : b.bh[1][c]));
  }
};

// ---- fp16 pair operands on MFMA, two pairs per workgroup (core_kernel_hpm2, replay_chunk_hpm2) ---------------------
// The pair's lanes share theta and sigma-eps E, so each GEMM of the step is  W_l x = theta x + s_l (E x)  on
// v_mfma_f32_16x16x32_f16: the A operands are fragment images of theta's half pack and of each pair's sigma-eps pack
// (mfma_image_kernel: [k-step][16-column tile][64 lanes][8 halves], HBM order = stream order, 1 KB per wave-load), the
// B operand X holds the activations rounded to f16 (fp16 tolerance), one env per column.  A workgroup of 8 waves takes
// two pairs -- 4 lanes, their NE = 4E envs as the B columns, repeated to 16 -- and issues per 16-column tile and k-step
//   theta x X,   E_0 x (S X masked to pair 0's columns),   E_1 x (S X masked to pair 1's)
// chained into ONE f32 accumulator: theta's fragment, the same for every pair, is read once for both (a past probe
// build of a one-pair-per-workgroup kernel without its per-pair theta loads ran the launch 16 % faster, 0.237 ->
// 0.199 ms at config 5; that experiment is why two pairs share a workgroup).  S X flips the sign bits of the minus
// lanes' columns.  A masked column contributes exact zeros to its accumulator column and an accumulator column only
// ever sees its own B column, so each env's sum is theta x + s_l (E_p x) of its own pair p in k order, whatever the
// other pair holds; a sign-0 (unperturbed) lane's columns are masked in both E operands: it runs theta bitwise.

// The weight stream of one GEMM: the fragments of ring step q (theta's and the two pairs', two column tiles each) are
// loaded D - 1 steps ahead of the MFMAs that consume them.
template <int NQ, class Frag>
struct MfmaRing2 {
  static constexpr int D = 4;
  static_assert(NQ % D == 0, "ring depth divides the step count");
  const _Float16* thm;
  const _Float16* ep0;
  const _Float16* ep1;
  Frag frag;
  h8 rt[D][2], ra[D][2], rb[D][2];
  __device__ __forceinline__ void issue(int q, h8 (&t)[2], h8 (&ea)[2], h8 (&eb)[2]) {
    const int64_t o = frag(q);
#pragma unroll
    for (int jt = 0; jt < 2; ++jt) {
      t[jt] = *reinterpret_cast<const h8*>(thm + o + 512 * jt);
      ea[jt] = ld_stream(reinterpret_cast<const h8*>(ep0 + o + 512 * jt));
      eb[jt] = ld_stream(reinterpret_cast<const h8*>(ep1 + o + 512 * jt));
    }
  }
  __device__ __forceinline__ void prime() {
#pragma unroll
    for (int u = 0; u < D - 1; ++u) issue(u, rt[u], ra[u], rb[u]);
  }
  template <class Mma>
  __device__ __forceinline__ void run(Mma&& mma) {
#pragma unroll 1
    for (int q0 = 0; q0 < NQ; q0 += D) {
#pragma unroll
      for (int u = 0; u < D; ++u) {
        const int q = q0 + u;
        const int v = (u + D - 1) % D;
        issue(min(q + D - 1, NQ - 1), rt[v], ra[v], rb[v]);  // past the end: a re-read
        __builtin_amdgcn_sched_barrier(0);
        mma(q, rt[u], ra[u], rb[u]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
};
template <int NQ, class Frag>
__device__ __forceinline__ MfmaRing2<NQ, Frag> mfma_ring2(const _Float16* thm, const _Float16* ep0, const _Float16* ep1,
                                                          Frag f) {
  return MfmaRing2<NQ, Frag>{thm, ep0, ep1, f};
}

// Fragment offset (halves, in the gate image) of ring step q of wave w's gate GEMM over k-steps KS0 .. kGateKS - 1:
// the wave owns gate column tiles 8w .. 8w + 7, two at a time (g = q / kNks), k-step KS0 + q % kNks.  KS0 = 0: the
// whole [W_ih | W_hh]^T (the rollout step); KS0 = kCoreIn / 32: W_hh^T only (the replay, whose x W_ih^T comes in a.gx).
template <int KS0>
struct GateFrag {
  static constexpr int kNks = kGateKS - KS0;
  int w, l;
  __device__ __forceinline__ int64_t operator()(int q) const {
    const int g = q / kNks, ks = KS0 + q - g * kNks;
    return ((int64_t)(ks * kGateNT + 8 * w + 2 * g) * 64 + l) * 8;
  }
};
template <int KS0>
__device__ __forceinline__ auto gate_ring2(const StepArgs& a, const _Float16* ep0, const _Float16* ep1, int w, int l) {
  return mfma_ring2<4 * GateFrag<KS0>::kNks>(a.thm + kFcImg, ep0 + kFcImg, ep1 + kFcImg, GateFrag<KS0>{w, l});
}

// One k-step of a wave's two column tiles: the three MFMAs per tile, in this order into one accumulator (x for theta,
// xa / xb = S x masked to pair 0's / pair 1's columns for E_0 / E_1).  Every GEMM of the two pair kernels goes through
// here.
__device__ __forceinline__ void pair_mma3(f32x4 (&acc)[2], const h8 (&tf)[2], const h8 (&fa)[2], const h8 (&fb)[2], h8 x,
                                          h8 xa, h8 xb) {
#pragma unroll
  for (int jt = 0; jt < 2; ++jt) {
    acc[jt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(tf[jt], x, acc[jt], 0, 0, 0);
    acc[jt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[jt], xa, acc[jt], 0, 0, 0);
    acc[jt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[jt], xb, acc[jt], 0, 0, 0);
  }
}

// The rest of the two-pairs set-up is shared as text: the three macros below expand inside core_kernel_hpm2 and
// replay_chunk_hpm2 and use those kernels' names -- a, L, E, NE, GP, j, w, l, l0, pkl and the LDS arrays gh, bsum.
// FDR_PAIR2_OPERANDS declares A = a.n_act; this lane's B column -- env benv of the workgroup, lane bl of its 4, pair
// bl / 2; and bfrag(rowp, k0, x, xa, xb), the lane's B fragment of k-step k0 / 32 from its env's row: x for theta, xa /
// xb = S x masked for E_0 / E_1.  S X flips the minus lanes' columns (branch-free sign loads), the two E operands see
// only their own pair's columns, and a sign-0 (unperturbed) lane's columns are zero in both: E adds exact zeros.
#define FDR_PAIR2_OPERANDS                                                                           \
  const int8_t* sgp = a.sign ? a.sign + l0 : reinterpret_cast<const int8_t*>(a.pack);                \
  const int8_t sg0 = sgp[0], sg1 = sgp[1], sg2 = sgp[2], sg3 = sgp[3];                               \
  const int A = a.n_act;                                                                             \
  const int benv = (l & 15) & (NE - 1), bl = benv / E;                                               \
  const int8_t bsg = bl == 0 ? sg0 : (bl == 1 ? sg1 : (bl == 2 ? sg2 : sg3));                        \
  const unsigned smask = (a.sign && bsg < 0) ? 0x80008000u : 0u;                                     \
  const unsigned zmask = (a.sign && bsg == 0) ? 0u : ~0u;                                            \
  const unsigned ma = (bl < 2 ? ~0u : 0u) & zmask, mb = (bl < 2 ? 0u : ~0u) & zmask;                 \
  auto bfrag = [&](const _Float16* rowp, int k0, h8& x, h8& xa, h8& xb) {                            \
    x = *reinterpret_cast<const h8*>(rowp + k0 + 8 * (l >> 4));                                      \
    const u32x4 sx = __builtin_bit_cast(u32x4, x) ^ u32x4{smask, smask, smask, smask};               \
    xa = __builtin_bit_cast(h8, sx & u32x4{ma, ma, ma, ma});                                         \
    xb = __builtin_bit_cast(h8, sx & u32x4{mb, mb, mb, mb});                                         \
  }
// FDR_PAIR2_TABLES zeroes gh's columns beyond kGateK (the last k-step's padding and the pitch) and fills bsum
// [lane][kGates] = b_ih + b_hh of the workgroup's 4 lanes.
#define FDR_PAIR2_TABLES                                                                             \
  for (int i = j; i < NE * (GP - kGateK); i += 2 * kCoreThreads) {                                   \
    const int e = i / (GP - kGateK);                                                                 \
    gh[e * GP + kGateK + i - e * (GP - kGateK)] = (_Float16)0.f;                                     \
  }                                                                                                  \
  _Pragma("unroll") for (int it = 0; it < 4 * kGates / (2 * kCoreThreads); ++it) {                   \
    const int i = j + it * 2 * kCoreThreads, li = i / kGates, col = i & (kGates - 1);                \
    const float* pk = pkl(li);                                                                       \
    bsum[i] = pk[L.lstm_bih + col] + pk[L.lstm_bhh + col];                                           \
  }
// FDR_PAIR2_GATE_GEMM(ring, KS0, gates): gates [col][NE] (f32) = this wave's gate column tiles over the ring's k-steps
// KS0 .. kGateKS - 1 against the B rows gh; the accumulators restart at each tile pair's first k-step and are stored
// at its last.
#define FDR_PAIR2_GATE_GEMM(ring, KS0, gates)                                                        \
  {                                                                                                  \
    f32x4 acc[2];                                                                                    \
    const _Float16* grow = gh + benv * GP;                                                           \
    ring.run([&](int q, const h8 (&tf)[2], const h8 (&fa)[2], const h8 (&fb)[2]) {                   \
      const int g = q / (kGateKS - KS0), ks = KS0 + q - g * (kGateKS - KS0);                         \
      if (ks == KS0)                                                                                 \
        _Pragma("unroll") for (int jt = 0; jt < 2; ++jt) acc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};        \
      h8 x, xa, xb;                                                                                  \
      bfrag(grow, 32 * ks, x, xa, xb);                                                               \
      pair_mma3(acc, tf, fa, fb, x, xa, xb);                                                         \
      if (ks == kGateKS - 1 && (l & 15) < NE) {                                                      \
        _Pragma("unroll") for (int jt = 0; jt < 2; ++jt)                                             \
          _Pragma("unroll") for (int i = 0; i < 4; ++i)                                              \
            gates[(16 * (8 * w + 2 * g + jt) + 4 * (l >> 4) + i) * NE + (l & 15)] = acc[jt][i];      \
      }                                                                                              \
    });                                                                                              \
  }

}  // namespace impala
}  // namespace fdr
