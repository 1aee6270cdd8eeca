// fdr_mlp_pair.h -- MlpPair: two lanes per wave, one per half (rollout_pair_kernel, theta_prime_pair_kernel), with
// the packed tanh forms, the per-wave scratch and the row broadcasts the pair kernel's step uses.
#pragma once
#include "fdr_mlp.h"

namespace fdr {

// ---------------------------------------------------------------------------------------------
// Two lanes per wave: rollout_pair_kernel (synthetic env)
//
// The wave's halves (threads 0-31 / 32-63, two DPP rows each) run one lane each; thread t of a
// half owns hidden units 2t, 2t+1 of layer 1 and units 16r + c, 16r + 8 + c (r = t/8, c = t%8) of
// layer 2.  Per lane the MAC instructions are those of the one-lane-per-wave kernel, but the
// per-lane scalar work (action, sampling, env tail, reward, loop control) is shared by the two
// lanes of a wave, and each wave carries two independent dependency chains:
//   L1 + M s   broadcast input of the half (LDS); W1 rows 2t, 2t+1 (per-wave tile) and M row t.
//   L2         thread (r, c) holds W2[16r + 8e + (c ^ sigma(p))][8c + k] (p < 8, e < 2, k < 8:
//              128 VGPRs) against h1[8c .. 8c + 7] (two b128), 16 partial outputs, then the
//              3-level reduce-scatter of the one-lane kernel over 16 slots (8 + 4 + 2 DPP adds).
//   head       thread (rho = t/16, o = t%16) sums W3[o][.] over the 32 units its own DPP row
//              holds (32 row_newbcast FMAs), then the two rows of the half (one permlane16 swap).
//   head, 12 outputs (kHeadRS: continuous, 6 actions): every thread multiplies its own two units into all 12
//              outputs (12 packed FMAs against 24 W3 values), a 4-level reduce-scatter over the row (12 DPP
//              adds and a select, tools/gen_dpp.py) leaves output 3 (o/4) + min(o%4, 2) in thread o -- means in threads
//              0,1,2,4,5,6, std pre-activations 8 lanes up -- then the two rows as above.
// ---------------------------------------------------------------------------------------------
constexpr int kPairWaves = 2;  // waves per workgroup (4 lanes): 4 workgroups, 8 waves per CU

// tanh_fast on a register pair: packed mul / add / fma around the two exp and two rcp
__device__ __forceinline__ f2 tanh2_pre(f2 t) {  // t = 2 log2(e) x
  const f2 d = f2{__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)} + f2{1.f, 1.f};
  return pk_fma(f2{-2.f, -2.f}, f2{__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)}, f2{1.f, 1.f});
}
__device__ __forceinline__ f2 tanh2_fast(f2 x) {
  return tanh2_pre(x * f2{kTanhScale, kTanhScale});
}
// Every weight and bias feeding a tanh is stored times kTanhScale (after its norm2 count), so the activation
// starts at the exp2 -- one multiply fewer per tanh (L1, L2, head, env: 4 per step)
constexpr float kPreScale = kTanhScale;
template <bool kPre>
__device__ __forceinline__ f2 tanh2_act(f2 z) {
  if constexpr (kPre) return tanh2_pre(z);
  else return tanh2_fast(z);
}

template <int NIN, int NA, bool DISC>
struct MlpPair {
  using L = Layout<NIN, NA, DISC>;
  static constexpr int NOUT = L::NOUT;
  static constexpr int NX = round4(NIN);
  static_assert(NX <= 32, "pair kernel: policy input wider than 32");
  static constexpr bool kBiasCol = NIN < NX;
  static constexpr bool kW1Lds = NIN > 8;
  static constexpr bool kPre = !DISC;  // tanh layers' weights stored x kTanhScale
  static constexpr float kWS = kPre ? kTanhScale : 1.f;
  static constexpr int kW1Chunks = kW1Lds ? NX / 4 : 0;     // per W1 row
  static constexpr bool kHeadRS = !DISC && NOUT == 12;        // the reduce-scatter head (fdr_dpp_gen.h)
  static constexpr int kW3Chunks = kHeadRS ? 6 : 8;           // float4 of W3 per thread
  static constexpr int kTileF4 = (2 * kW1Chunks + kW3Chunks) * kWave;  // float4 per wave: W1 rows, W3 slice
  f2 w1a[kW1Lds ? 1 : NX / 2], w1b[kW1Lds ? 1 : NX / 2];
  float b1a, b1b;
  const float4* tile;  // this thread's column of the wave tile (chunk m at tile[m * kWave])
  f2 w2[64];           // w2[p * 8 + k] = (W2[16r + (c ^ sigma(p))][8c + k], W2[16r + 8 + (c ^ sigma(p))][8c + k])
  float b2a, b2b, b3;
  float a0, c0, a1a, c1a, a1b, c1b, a2a, c2a, a2b, c2b;  // discrete: folded BN

  // unit of layer 2 that row-thread k's value e (0: z.x, 1: z.y) holds, within the row's 32 units
  __host__ __device__ static constexpr int head_unit(int rho, int k, int e) {
    return 32 * rho + 8 * (k >> 2) + 4 * e + (k & 3);  // thread 4q + c holds units 8q + c, 8q + 4 + c
  }

  template <class Src>  // ParamSrc, or RecordSrc (MlpLane::load)
  __device__ __forceinline__ void load(Src& src, int t, int tid, const float* bn_mean, const float* bn_var,
                                       float4* wave_tile) {
    const int rho = t >> 4, o = t & 15;
    const int ua = 2 * t, ub = 2 * t + 1;
    float4* my = wave_tile + tid;
    tile = my;
    auto w1v = [&](int u, int k) {
      return kWS * (k < NIN ? src.get(L::L1W + (int64_t)u * NIN + k) : (k == NIN ? src.get(L::L1B + u) : 0.f));
    };
    if constexpr (kPk) {
#pragma unroll
      for (int j = 0; j < 2 * kW1Chunks; ++j) {
        const float e0 = w1v(ua, 2 * j), f0 = w1v(ub, 2 * j), e1 = w1v(ua, 2 * j + 1), f1 = w1v(ub, 2 * j + 1);
        my[j * kWave] = float4{e0, f0, e1, f1};
      }
    } else if constexpr (kW1Lds) {
#pragma unroll
      for (int m = 0; m < kW1Chunks; ++m) {
        const float e0 = w1v(ua, 4 * m), e1 = w1v(ua, 4 * m + 1), e2 = w1v(ua, 4 * m + 2), e3 = w1v(ua, 4 * m + 3);
        my[m * kWave] = float4{e0, e1, e2, e3};
        const float f0 = w1v(ub, 4 * m), f1 = w1v(ub, 4 * m + 1), f2_ = w1v(ub, 4 * m + 2), f3 = w1v(ub, 4 * m + 3);
        my[(kW1Chunks + m) * kWave] = float4{f0, f1, f2_, f3};
      }
    } else {
#pragma unroll
      for (int p = 0; p < NX / 2; ++p) {
        const float e0 = w1v(ua, 2 * p), e1 = w1v(ua, 2 * p + 1);
        w1a[p] = f2{e0, e1};
        const float f0 = w1v(ub, 2 * p), f1 = w1v(ub, 2 * p + 1);
        w1b[p] = f2{f0, f1};
      }
    }
    b1a = kBiasCol ? 0.f : kWS * src.get(L::L1B + ua);
    b1b = kBiasCol ? 0.f : kWS * src.get(L::L1B + ub);
    // (load groups: each group's loads are issued together, the next group's after it -- hoisting every load of the
    // prologue to its top spilled ~140 values to scratch)
    __builtin_amdgcn_sched_barrier(0);
    // quad q = t / 4 owns units 8q .. 8q + 7; thread c = t % 4 of it takes inputs 16c .. 16c + 15 and pair p the
    // units (8q + (c ^ p), 8q + 4 + (c ^ p)): the quad's reduce-scatter (partners c ^ 2, c ^ 1) leaves pair 0
    const int q4 = t >> 2, c4 = t & 3;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int row0 = 8 * q4 + (c4 ^ p), row1 = row0 + 4;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const float e0 = src.get(L::L2W + (int64_t)row0 * kHidden + 16 * c4 + k);
        const float e1 = src.get(L::L2W + (int64_t)row1 * kHidden + 16 * c4 + k);
        w2[p * 16 + k] = f2{kWS * e0, kWS * e1};
      }
      // the group's weights and its norm terms are final here (else the compiler defers the selects past the other
      // groups' loads and keeps every sigma * eps in scratch meanwhile)
#pragma unroll
      for (int k = 0; k < 16; ++k) asm volatile("" : "+v"(w2[p * 16 + k]));
      asm volatile("" : "+v"(src.n2));
      __builtin_amdgcn_sched_barrier(0);
    }
    const int u2a = 8 * q4 + c4, u2b = 8 * q4 + 4 + c4;  // this thread's layer-2 units
    b2a = kWS * src.get(L::L2B + u2a);
    b2b = kWS * src.get(L::L2B + u2b);
    if constexpr (kHeadRS) {
      // register r of this thread holds output head_rs12_slot(o, r): W3 of the thread's two layer-2 units against all
      // 12 outputs, every element read and counted once per lane.  Chunks 0-2: unit u2a (h2.x), 3-5: unit u2b (h2.y)
#pragma unroll
      for (int m = 0; m < 6; ++m) {
        float e[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          e[i] = src.get(L::L3W + (int64_t)head_rs12_slot(o, 4 * (m % 3) + i) * kHidden + (m < 3 ? u2a : u2b));
        my[(2 * kW1Chunks + m) * kWave] = float4{kWS * e[0], kWS * e[1], kWS * e[2], kWS * e[3]};
      }
      b3 = kWS * src.get_if(L::L3B + head_rs12_out(o), rho == 0 && c4 != 3);  // thread 4q + 3 repeats 4q + 2
    } else {
      const bool has_o = o < NOUT;
      const int oc = has_o ? o : 0;
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        float e[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int w = 4 * m + i;
          // w < 16: value z.x of row-thread w; else z.y of row-thread w - 16
          e[i] = src.get_if(L::L3W + (int64_t)oc * kHidden + head_unit(rho, w & 15, w >> 4), has_o);
        }
        my[(2 * kW1Chunks + m) * kWave] =
            has_o ? float4{kWS * e[0], kWS * e[1], kWS * e[2], kWS * e[3]} : float4{0.f, 0.f, 0.f, 0.f};
      }
      const float b3v = src.get_if(L::L3B + oc, has_o && rho == 0);
      b3 = has_o ? kWS * b3v : 0.f;
    }
    wave_lds_sync();
    a0 = c0 = a1a = c1a = a1b = c1b = a2a = c2a = a2b = c2b = 0.f;
    if constexpr (DISC) {
      const float* bm = bn_mean ? bn_mean : src.base;  // a readable address either way
      const float* bv = bn_var ? bn_var : src.base;
      auto stat = [&](int k, float& rm, float& rv) {
        const float m = bm[k], v = bv[k];
        rm = bn_mean ? m : 0.f;
        rv = bn_var ? v : 1.f;
      };
      {
        const bool in = t < NIN;
        const int tc = in ? t : 0;
        const float w = src.get_if(L::BN0W + tc, in), b = src.get_if(L::BN0B + tc, in);
        float rm, rv, a, c;
        stat(tc, rm, rv);
        bn_fold(w, b, rm, rv, a, c);
        a0 = in ? a : 0.f;
        c0 = in ? c : 0.f;
      }
      auto fold = [&](int64_t wofs, int64_t bofs, int st, int u, float& av, float& cv) {
        const float w = src.get(wofs + u), b = src.get(bofs + u);
        float rm, rv;
        stat(st + u, rm, rv);
        bn_fold(w, b, rm, rv, av, cv);
      };
      fold(L::BN1W, L::BN1B, NIN, ua, a1a, c1a);
      fold(L::BN1W, L::BN1B, NIN, ub, a1b, c1b);
      fold(L::BN2W, L::BN2B, NIN + kHidden, u2a, a2a, c2a);
      fold(L::BN2W, L::BN2B, NIN + kHidden, u2b, a2b, c2b);
    }
  }

  __device__ __forceinline__ float input_transform(float x) const {
    if constexpr (DISC) {
      return fmaf(x, a0, c0);
    } else {
      return x;
    }
  }

  __device__ __forceinline__ float act1(float z, float av, float cv) const {
    if constexpr (DISC) {
      return fmaf(fmaxf(z, 0.f), av, cv);
    } else {
      return tanh_act<kPre>(z);
    }
  }

  // Loop-invariant LDS rows of layer 1 (W1 rows 2t, 2t+1 when kW1Lds) and the env's M row t, loaded
  // a phase ahead of their use (after the head of the previous step), off the step's dependency chain.
  // NIN = 4k + 1 with the folded bias (HalfCheetah's 17): the last input chunk is [x_{NIN-1}, 1, 0, 0] and the
  // W1 / M chunks [w, b, 0, 0] / [m, 0, 0, 0] -- taken as one scalar input (a ds_read_b32 of x, a float2 of
  // W1, a float of M) and 3 FMAs instead of a fifth b128 chunk and 6 packed FMAs
  static constexpr bool kTail = kW1Lds && kBiasCol && NX - NIN == 3;
  static constexpr int NQ = kTail ? NX / 4 - 1 : NX / 4;  // full input chunks
  // W1 rows 2t, 2t+1 interleaved in the tile, [w_a(2j), w_b(2j), w_a(2j+1), w_b(2j+1)] per
  // float4, so each input k is ONE packed FMA over the two units into an (a, b) accumulator -- the layer's
  // output pair needs no horizontal adds / register shuffles before the packed tanh, and the folded bias
  // column is an add, not a multiply by 1
  static constexpr bool kPk = kW1Lds && kBiasCol;
  static constexpr int kPkPairs = (NIN + 2) / 2;  // float4 pairs of inputs 0 .. NIN (the bias column)
  struct L1Rows {
    float4 wa[kW1Lds && !kPk ? NQ : 1], wb[kW1Lds && !kPk ? NQ : 1], m[NQ];
    float2 ta, tb;  // kTail: (w, b) of the last chunk
    float tm;
    float4 wp[kPk ? kPkPairs : 1];
  };
  __device__ __forceinline__ void l1_prefetch(L1Rows& r, const float* mrow) const {
    const float4* m4 = reinterpret_cast<const float4*>(mrow);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if constexpr (kW1Lds && !kPk) {
        r.wa[q] = tile[q * kWave];
        r.wb[q] = tile[(kW1Chunks + q) * kWave];
      }
      r.m[q] = m4[q];
    }
    if constexpr (kPk) {
#pragma unroll
      for (int j = 0; j < kPkPairs; ++j) r.wp[j] = tile[j * kWave];
      if constexpr (kTail) r.tm = mrow[4 * NQ];
    } else if constexpr (kTail) {
      r.ta = *reinterpret_cast<const float2*>(&tile[NQ * kWave]);
      r.tb = *reinterpret_cast<const float2*>(&tile[(kW1Chunks + NQ) * kWave]);
      r.tm = mrow[4 * NQ];
    }
  }

  // The env state chunks layer 1 read (the input itself when kSameInput), kept for env_ms
  struct SIn {
    float4 v[NQ];
    float t;
  };
  // Layer 1 (units 2t, 2t+1) over the broadcast input chunks; the env state chunks go to `sin`.  The chunk reads
  // are issued first and `fill` (work that needs none of them) runs while they are in flight.
  template <bool kSameInput, class Fill>
  __device__ __forceinline__ f2 layer1_env(const float* xs, const float* ss, const L1Rows& rows, SIn& sin,
                                           Fill&& fill) const {
    const float4* x4 = reinterpret_cast<const float4*>(xs);
    const float4* s4 = reinterpret_cast<const float4*>(ss);
    SIn xin;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      xin.v[q] = x4[q];
      sin.v[q] = kSameInput ? xin.v[q] : s4[q];
    }
    xin.t = kTail ? xs[4 * NQ] : 0.f;
    sin.t = kSameInput ? xin.t : (kTail ? ss[4 * NQ] : 0.f);
    fill();
    __builtin_amdgcn_sched_barrier(0);  // layer 1 (asm statements: no class mask holds them) stays behind the fill
    return layer1_q(xin, rows);
  }
  // M[t] . s from the chunks layer 1 read (no part of the policy's chain: the compiler interleaves it with layer 1)
  __device__ __forceinline__ float env_ms(const SIn& sin, const L1Rows& rows) const {
    f2 am0 = {0.f, 0.f}, am1 = {0.f, 0.f};
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const float4 sv = sin.v[q], mv = rows.m[q];
      am0 = pk_fma(f2{mv.x, mv.y}, f2{sv.x, sv.y}, am0);
      am1 = pk_fma(f2{mv.z, mv.w}, f2{sv.z, sv.w}, am1);
    }
    if constexpr (kTail) am1.x = fmaf(rows.tm, sin.t, am1.x);
    const f2 am = am0 + am1;
    return am.x + am.y;
  }
  __device__ __forceinline__ f2 layer1_q(const SIn& xin, const L1Rows& rows) const {
    const float xt = xin.t;
    auto xq = [&](int q) { return xin.v[q]; };
    f2 aa0 = {b1a, 0.f}, aa1 = {0.f, 0.f}, ab0 = {b1b, 0.f}, ab1 = {0.f, 0.f};
    if constexpr (kPk) {
      // units (a, b) packed: acc[k % NC] += (w_a(k), w_b(k)) * x_k; the bias column (k = NIN) is added.
      // NC = 2 chains of ~9 dependent packed FMAs
      constexpr int NC = 2;
      f2 acc[NC];
#pragma unroll
      for (int q = 0; q < NC; ++q) acc[q] = f2{0.f, 0.f};
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const float4 xv = xq(q);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int k = 4 * q + i;
          if (k < NIN) {
            const float4 w = rows.wp[k >> 1];
            const f2 xp = (i < 2) ? f2{xv.x, xv.y} : f2{xv.z, xv.w};
            if (kPre && k == NIN % NC) {  // the chain that takes the bias column starts from it
              const float4 wb = rows.wp[NIN >> 1];
              const f2 bias = (NIN & 1) ? f2{wb.z, wb.w} : f2{wb.x, wb.y};
              acc[k % NC] = (k & 1) ? pk_fma_bhi(f2{w.z, w.w}, xp, bias) : pk_fma_blo(f2{w.x, w.y}, xp, bias);
            } else if (k < NC)
              acc[k % NC] = (k & 1) ? pk_mul_bhi(f2{w.z, w.w}, xp) : pk_mul_blo(f2{w.x, w.y}, xp);
            else
              acc[k % NC] = (k & 1) ? pk_fma_bhi(f2{w.z, w.w}, xp, acc[k % NC]) : pk_fma_blo(f2{w.x, w.y}, xp, acc[k % NC]);
          }
        }
      }
      if constexpr (kTail) {  // input 4 NQ = NIN - 1, then the bias
        const float4 w = rows.wp[(NIN - 1) >> 1];
        acc[(NIN - 1) % NC] = pk_fma(((NIN - 1) & 1) ? f2{w.z, w.w} : f2{w.x, w.y}, f2{xt, xt}, acc[(NIN - 1) % NC]);
      }
      if constexpr (!kPre || NIN % NC >= NIN) {
        const float4 w = rows.wp[NIN >> 1];
        acc[NIN % NC] = acc[NIN % NC] + ((NIN & 1) ? f2{w.z, w.w} : f2{w.x, w.y});
      }
      const f2 h = acc[0] + acc[1];
      if constexpr (DISC) {
        return f2{act1(h.x, a1a, c1a), act1(h.y, a1b, c1b)};
      } else {
        return tanh2_act<kPre>(h);
      }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const float4 xv = xq(q);
      float4 wa, wb;
      if constexpr (kW1Lds) {
        wa = rows.wa[q];
        wb = rows.wb[q];
      } else {
        wa = float4{w1a[2 * q].x, w1a[2 * q].y, w1a[2 * q + 1].x, w1a[2 * q + 1].y};
        wb = float4{w1b[2 * q].x, w1b[2 * q].y, w1b[2 * q + 1].x, w1b[2 * q + 1].y};
      }
      aa0 = pk_fma(f2{wa.x, wa.y}, f2{xv.x, xv.y}, aa0);
      ab0 = pk_fma(f2{wb.x, wb.y}, f2{xv.x, xv.y}, ab0);
      aa1 = pk_fma(f2{wa.z, wa.w}, f2{xv.z, xv.w}, aa1);
      ab1 = pk_fma(f2{wb.z, wb.w}, f2{xv.z, xv.w}, ab1);
    }
    if constexpr (kTail) {  // w x + b of the last chunk
      aa1 = pk_fma(f2{rows.ta.x, rows.ta.y}, f2{xt, 1.f}, aa1);
      ab1 = pk_fma(f2{rows.tb.x, rows.tb.y}, f2{xt, 1.f}, ab1);
    }
    const f2 ha = aa0 + aa1, hb = ab0 + ab1;
    if constexpr (DISC) {
      return f2{act1(ha.x + ha.y, a1a, c1a), act1(hb.x + hb.y, a1b, c1b)};
    } else {
      return tanh2_act<kPre>(f2{ha.x + ha.y, hb.x + hb.y});
    }
  }

  // Layer 2 and the head: h1 = this thread's layer-1 units (2t, 2t+1); h1s = the half's scratch.
  // Returns the head pre-activation for output o = t & 15 (identical in both rows of the half); kHeadRS: for output
  // head_rs12_out(t & 15).
  // Wave priority: low for the 64 independent layer-2 FMAs (from the h1 write on), raised for the serial part of the
  // step -- reduce-scatter, tanh, head, action, env, x hand-off, layer 1 -- so the SIMD's other wave yields to it
  template <class Mark>
  __device__ __forceinline__ float layers23(f2 h1, float* h1s, int t, Mark&& mark) const {
    const int c4 = t & 3;
    float x[16];
    reinterpret_cast<f2*>(h1s)[t] = h1;
    __builtin_amdgcn_s_setprio(0);
    wave_lds_sync();
    lds_bcast<16>(h1s + 16 * c4, x);
    float w3[4 * kW3Chunks];
#pragma unroll
    for (int m = 0; m < kW3Chunks; ++m) {
      const float4 w = tile[(2 * kW1Chunks + m) * kWave];
      w3[4 * m] = w.x;
      w3[4 * m + 1] = w.y;
      w3[4 * m + 2] = w.z;
      w3[4 * m + 3] = w.w;
    }
    f2 acc[4];
#pragma unroll
    for (int p = 0; p < 4; ++p)  // k = 0; kPre: the own pair (p = 0) starts from the biases
      acc[p] = pk_fma(w2[p * 16], f2{x[0], x[0]}, (kPre && p == 0) ? f2{b2a, b2b} : f2{0.f, 0.f});
    {
      // k = 1 .. 15 by op_sel broadcasts of the pairs xp[j] = (x[2j], x[2j + 1]) in one asm statement (operands:
      // %0-%3 acc, %(4 + 4 (k - 1) + p) = w2[16 p + k], %64-%71 the pairs); k = 15 writes acc[3], acc[2] first,
      // the reduce-scatter's first DPP sources
      f2 xp[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) xp[j] = f2{x[2 * j], x[2 * j + 1]};
#define FDR_L2_HI "op_sel:[0,1,0] op_sel_hi:[1,1,1]"
#define FDR_L2_LO "op_sel_hi:[1,0,1]"
      asm(
          "v_pk_fma_f32 %0, %4, %64, %0 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %1, %5, %64, %1 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %2, %6, %64, %2 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %3, %7, %64, %3 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %0, %8, %65, %0 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %1, %9, %65, %1 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %2, %10, %65, %2 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %3, %11, %65, %3 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %0, %12, %65, %0 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %1, %13, %65, %1 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %2, %14, %65, %2 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %3, %15, %65, %3 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %0, %16, %66, %0 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %1, %17, %66, %1 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %2, %18, %66, %2 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %3, %19, %66, %3 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %0, %20, %66, %0 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %1, %21, %66, %1 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %2, %22, %66, %2 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %3, %23, %66, %3 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %0, %24, %67, %0 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %1, %25, %67, %1 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %2, %26, %67, %2 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %3, %27, %67, %3 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %0, %28, %67, %0 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %1, %29, %67, %1 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %2, %30, %67, %2 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %3, %31, %67, %3 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %0, %32, %68, %0 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %1, %33, %68, %1 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %2, %34, %68, %2 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %3, %35, %68, %3 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %0, %36, %68, %0 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %1, %37, %68, %1 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %2, %38, %68, %2 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %3, %39, %68, %3 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %0, %40, %69, %0 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %1, %41, %69, %1 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %2, %42, %69, %2 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %3, %43, %69, %3 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %0, %44, %69, %0 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %1, %45, %69, %1 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %2, %46, %69, %2 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %3, %47, %69, %3 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %0, %48, %70, %0 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %1, %49, %70, %1 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %2, %50, %70, %2 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %3, %51, %70, %3 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %0, %52, %70, %0 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %1, %53, %70, %1 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %2, %54, %70, %2 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %3, %55, %70, %3 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %0, %56, %71, %0 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %1, %57, %71, %1 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %2, %58, %71, %2 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %3, %59, %71, %3 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %3, %63, %71, %3 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %2, %62, %71, %2 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %0, %60, %71, %0 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %1, %61, %71, %1 " FDR_L2_HI "\n"
          : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3])
          : "v"(w2[1]), "v"(w2[17]), "v"(w2[33]), "v"(w2[49]),
            "v"(w2[2]), "v"(w2[18]), "v"(w2[34]), "v"(w2[50]),
            "v"(w2[3]), "v"(w2[19]), "v"(w2[35]), "v"(w2[51]),
            "v"(w2[4]), "v"(w2[20]), "v"(w2[36]), "v"(w2[52]),
            "v"(w2[5]), "v"(w2[21]), "v"(w2[37]), "v"(w2[53]),
            "v"(w2[6]), "v"(w2[22]), "v"(w2[38]), "v"(w2[54]),
            "v"(w2[7]), "v"(w2[23]), "v"(w2[39]), "v"(w2[55]),
            "v"(w2[8]), "v"(w2[24]), "v"(w2[40]), "v"(w2[56]),
            "v"(w2[9]), "v"(w2[25]), "v"(w2[41]), "v"(w2[57]),
            "v"(w2[10]), "v"(w2[26]), "v"(w2[42]), "v"(w2[58]),
            "v"(w2[11]), "v"(w2[27]), "v"(w2[43]), "v"(w2[59]),
            "v"(w2[12]), "v"(w2[28]), "v"(w2[44]), "v"(w2[60]),
            "v"(w2[13]), "v"(w2[29]), "v"(w2[45]), "v"(w2[61]),
            "v"(w2[14]), "v"(w2[30]), "v"(w2[46]), "v"(w2[62]),
            "v"(w2[15]), "v"(w2[31]), "v"(w2[47]), "v"(w2[63]),
            "v"(xp[0]), "v"(xp[1]), "v"(xp[2]), "v"(xp[3]), "v"(xp[4]), "v"(xp[5]), "v"(xp[6]), "v"(xp[7]));
#undef FDR_L2_LO
#undef FDR_L2_HI
    }
    // reduce-scatter over the quad: slot i = acc[i / 2][i % 2]; level 1 o_i = v_i + partner(c ^ 2).v_{i + 4} in
    // the order o2, o3, o0, o1, level 2 o_i += partner(c ^ 1).o_{i + 2} -- every DPP source >= 3 instructions old
    f2 zs;
    __builtin_amdgcn_s_setprio(1);
    {
      float o0, o1, o2, o3;
      asm volatile(
          "v_add_f32_dpp %2, %10, %6 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
          "v_add_f32_dpp %3, %11, %7 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
          "v_add_f32_dpp %0, %8, %4 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
          "v_add_f32_dpp %1, %9, %5 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
          "v_add_f32_dpp %0, %2, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
          "v_add_f32_dpp %1, %3, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
          : "=&v"(o0), "=&v"(o1), "=&v"(o2), "=&v"(o3)
          : "v"(acc[0].x), "v"(acc[0].y), "v"(acc[1].x), "v"(acc[1].y), "v"(acc[2].x), "v"(acc[2].y), "v"(acc[3].x),
            "v"(acc[3].y));
      zs = f2{o0, o1};
    }
    const float za = kPre ? zs.x : zs.x + b2a;  // unit 8q + c
    const float zb = kPre ? zs.y : zs.y + b2b;  // unit 8q + 4 + c
    mark(1, za);
    float h2a, h2b;
    if constexpr (DISC) {
      h2a = fmaf(fmaxf(za, 0.f), a2a, c2a);
      h2b = fmaf(fmaxf(zb, 0.f), a2b, c2b);
    } else {
      const f2 h2 = tanh2_act<kPre>(f2{za, zb});
      h2a = h2.x;
      h2b = h2.y;
    }
    float u, v;  // u = row 2h's partial, v = row 2h+1's, in both rows of half h
    if constexpr (kHeadRS) {
      f2 w3p[12];
#pragma unroll
      for (int j = 0; j < 12; ++j) w3p[j] = f2{w3[2 * j], w3[2 * j + 1]};
      // 12 packed products, 12 DPP adds, a select, the last add again and the row swap: one asm statement
      dpp_head_rs12(u, v, w3p, f2{h2a, h2b});
    } else {
      dpp_dot_32x1(u, h2a, h2b, w3);  // one chain of 32 (the accumulator is no DPP source: no wait states)
      v = u;
      permlane16_swap(u, v);
    }
    const float out = (u + v) + b3;
    mark(2, out);
    return out;
  }

  template <bool kAll = false, bool kFast = false>  // as MlpLane::softmax
  __device__ __forceinline__ float softmax(float logit, int t) const {
    const bool valid = (t & 15) < NOUT;
    const float v = valid ? logit : -FLT_MAX;
    const float mx = row16_max_n<NOUT>(v);
    if constexpr (kFast) {
      const float e = valid ? __builtin_amdgcn_exp2f((v - mx) * 1.44269504088896341f) : 0.f;
      return e * __builtin_amdgcn_rcpf(row16_sum_n<NOUT>(e));
    } else {
      const float e = valid ? expf(v - mx) : 0.f;
      return e / row16_sum_n<NOUT>(e);
    }
  }
};

struct alignas(16) PairScratchBase {
  float h1[2][kHidden];  // per half: layer-1 output; the env state when it differs from the input
  float x[2][32];        // per half: policy input (+ the 1 of the folded bias column)
};
// kDump: a slot per thread that is written and never read, in thread t's own bank (the x write of the threads that hold
// no input column: rollout_pair_kernel, FDR_PAIR_X_DUMP)
template <bool kDump>
struct PairScratch : PairScratchBase {};
template <>
struct alignas(16) PairScratch<true> : PairScratchBase {
  float dump[2][32];
  __device__ __forceinline__ float* dump_slot(int hh, int t) { return &dump[hh][t]; }
};

template <int K>
__device__ __forceinline__ float row_bcast(float v) {  // lane K of the caller's 16-lane row
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x150 + K, 0xF, 0xF, false));
}

template <int N, int... I>
__device__ __forceinline__ void row_bcast_all(float v, float (&out)[N], std::integer_sequence<int, I...>) {
  ((out[I] = row_bcast<I>(v)), ...);
}

}  // namespace fdr
