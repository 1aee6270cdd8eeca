// fdr_mlp_lane.h -- MlpLane: one lane's policy held by one wave (rollout_kernel, policy_forward_kernel,
// theta_prime_lane_kernel), and its per-wave LDS hand-off helpers.
#pragma once
#include "fdr_mlp.h"

namespace fdr {

// ---------------------------------------------------------------------------------------------
// One lane's policy, register resident.
//
// Matvecs run on packed f32 FMAs (v_pk_fma_f32, two MACs per instruction) over operands that sit
// in the lane's own registers -- DPP-operand FMAs issue at ~4.7 cycles per wave-instruction on
// gfx950 (tools/probes/valu_probe.hip) and were the rollout's bottleneck.  Activations cross lanes
// through a 1 KiB per-wave LDS scratch: one ds_write_b32 per lane, broadcast ds_read_b128 back.
//
//   L1 (NIN -> 64)  broadcast input (LDS), lane j: row j of W1 (VGPR pairs, or the per-wave LDS
//                   tile when NIN > 8; bias folded into the padding column); output j in lane j.
//   env (M s + K a) M s in the same pass as L1 over the broadcast input chunks (lane j < NIN: row j
//                   of M from the block's LDS copy); K a by DPP row_newbcast FMAs once the action
//                   (lanes 0 .. NA-1 of every row) is known.
//   L2 (64 -> 64)   8 x 8 lane blocks: lane (r = j/8, c = j%8) holds W2[8r + pi_c(i)][8c + k]
//                   (i, k < 8; 64 VGPRs), reads x[8c .. 8c + 7] (two b128), accumulates 8
//                   partial outputs in 4 packed pairs, then a 3-level reduce-scatter over the 8
//                   lanes of its half-row (DPP half_mirror, quad xor 2, quad xor 1: 7 adds)
//                   leaves output 8r + c = j in lane j.  pi_c(i) = c ^ sigma(i),
//                   sigma = (0 1 2 3 7 6 5 4), is the register order that makes every level send
//                   the partner exactly the outputs it keeps.
//   head (64 -> NOUT <= 16)  lane (q = j/16, o = j%16): W3[o][16q .. 16q + 15] against h2[16q + i],
//                   which sits in lane i of the lane's own row q (DPP row_newbcast FMAs, no LDS round
//                   trip), then the 4-row all-reduce (two permlane swaps).
// ---------------------------------------------------------------------------------------------
__host__ __device__ constexpr int l2_sigma(int i) { return i < 4 ? i : 11 - i; }

// per-wave LDS scratch for the cross-lane hand-offs of one step (16-B aligned slots).  LDS ops of
// one wave complete in order: a slot is rewritten only after the reads of its previous contents.
struct alignas(16) WaveScratch {
  float h1[kHidden];  // layer-1 output (L2 input); the env state when it differs from the policy input
  float x[kWave];     // policy input (+ the 1 of the folded bias column), written by every lane
};

// sum_k w[k] x[k] over a 16-B aligned LDS row (N % 4 == 0), two packed partial sums
template <int N>
__device__ __forceinline__ float dot_lds_row(const float* w, const float (&x)[N], float init) {
  const float4* w4 = reinterpret_cast<const float4*>(w);
  f2 acc = {init, 0.f};
#pragma unroll
  for (int q = 0; q < N / 4; ++q) {
    const float4 t = w4[q];
    acc = pk_fma(f2{t.x, t.y}, f2{x[4 * q], x[4 * q + 1]}, acc);
    acc = pk_fma(f2{t.z, t.w}, f2{x[4 * q + 2], x[4 * q + 3]}, acc);
  }
  return acc.x + acc.y;
}

template <int NIN, int NA, bool DISC>
struct MlpLane {
  using L = Layout<NIN, NA, DISC>;
  using Scratch = WaveScratch;
  static constexpr int NOUT = L::NOUT;
  static constexpr int NX = round4(NIN);
  static constexpr bool kBiasCol = NIN < NX;  // b1 sits in W1 column NIN (input NIN == 1)
  // Per-wave LDS tile of lane-private weights, float4 chunks laid out [chunk][lane] (conflict-free
  // b128): W1 row j when NIN > 8 (bias folded into column NIN), then W3[o][16q .. 16q + 15].
  // Keeping them out of VGPRs leaves room for whole-row loads in flight (<= 128 VGPRs, 4 waves/SIMD);
  // the W3 chunks are read in the same LDS round trip as the head's input.
  static constexpr bool kW1Lds = NIN > 8;
  static constexpr int kW1Chunks = kW1Lds ? NX / 4 : 0;
  static constexpr int kTileF4 = (kW1Chunks + 4) * kWave;  // float4 per wave
  f2 w1[kW1Lds ? 1 : NX / 2];
  float b1;
  const float4* tile;  // this lane's column of the tile (chunk m at tile[m * kWave])
  f2 w2[32];           // w2[p * 8 + k] = (W2[8r + pi_c(2p)][8c + k], W2[8r + pi_c(2p + 1)][8c + k])
  float b2;
  float b3;
  float a0, c0, a1, c1, a2, c2;  // discrete: folded BN for input j / hidden unit j

  // Src: ParamSrc (every rollout / forward kernel), or RecordSrc (the theta' read-back, fdr_diag_theta_prime)
  template <class Src>
  __device__ __forceinline__ void load(Src& src, int j, const float* bn_mean,
                                       const float* bn_var, float4* lds_tile) {
    const int r = j >> 3, c = j & 7, o = j & 15, q = j >> 4;
    tile = lds_tile + j;
    float4* my = lds_tile + j;
    auto w1v = [&](int k) {
      return k < NIN ? src.get(L::L1W + (int64_t)j * NIN + k) : (k == NIN ? src.get(L::L1B + j) : 0.f);
    };
    if constexpr (kW1Lds) {
#pragma unroll
      for (int m = 0; m < kW1Chunks; ++m) {
        const float e0 = w1v(4 * m), e1 = w1v(4 * m + 1), e2 = w1v(4 * m + 2), e3 = w1v(4 * m + 3);
        my[m * kWave] = float4{e0, e1, e2, e3};
      }
    } else {
#pragma unroll
      for (int p = 0; p < NX / 2; ++p) {
        const float e0 = w1v(2 * p), e1 = w1v(2 * p + 1);
        w1[p] = f2{e0, e1};
      }
    }
    b1 = kBiasCol ? 0.f : src.get(L::L1B + j);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int row0 = 8 * r + (c ^ l2_sigma(2 * p)), row1 = 8 * r + (c ^ l2_sigma(2 * p + 1));
#pragma unroll
      for (int k = 0; k < 8; ++k)
        w2[p * 8 + k] = f2{src.get(L::L2W + (int64_t)row0 * kHidden + 8 * c + k),
                           src.get(L::L2W + (int64_t)row1 * kHidden + 8 * c + k)};
      // the group's weights and norm terms are final here (MlpPair::load: no deferred selects held in scratch)
#pragma unroll
      for (int k = 0; k < 8; ++k) asm volatile("" : "+v"(w2[p * 8 + k]));
      asm volatile("" : "+v"(src.n2));
      __builtin_amdgcn_sched_barrier(0);
    }
    b2 = src.get(L::L2B + j);
    // Branch-free from here (r12): a load behind a condition ends its block with a vmcnt(0) wait.  The head rows
    // and the input BN are read from clamped indices by every lane, counted and kept only where they exist; the
    // running stats from a valid address whether or not they were given.
    {
      const bool has_o = o < NOUT;
      const int oc = has_o ? o : 0;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int64_t base = L::L3W + (int64_t)oc * kHidden + 16 * q + 4 * m;
        const float e0 = src.get_if(base, has_o), e1 = src.get_if(base + 1, has_o), e2 = src.get_if(base + 2, has_o),
                    e3 = src.get_if(base + 3, has_o);
        my[(kW1Chunks + m) * kWave] = has_o ? float4{e0, e1, e2, e3} : float4{0.f, 0.f, 0.f, 0.f};
      }
      const float b3v = src.get_if(L::L3B + oc, has_o && q == 0);
      b3 = has_o ? b3v : 0.f;
    }
    wave_lds_sync();
    a0 = c0 = a1 = c1 = a2 = c2 = 0.f;
    if constexpr (DISC) {
      const float* bm = bn_mean ? bn_mean : src.base;  // a readable address either way
      const float* bv = bn_var ? bn_var : src.base;
      auto stat = [&](int k, float& rm, float& rv) {
        const float m = bm[k], v = bv[k];
        rm = bn_mean ? m : 0.f;
        rv = bn_var ? v : 1.f;
      };
      {
        const bool in = j < NIN;
        const int jc = in ? j : 0;
        const float w = src.get_if(L::BN0W + jc, in), b = src.get_if(L::BN0B + jc, in);
        float rm, rv, a, c;
        stat(jc, rm, rv);
        bn_fold(w, b, rm, rv, a, c);
        a0 = in ? a : 0.f;
        c0 = in ? c : 0.f;
      }
      {
        const float w = src.get(L::BN1W + j), b = src.get(L::BN1B + j);
        float rm, rv;
        stat(NIN + j, rm, rv);
        bn_fold(w, b, rm, rv, a1, c1);
      }
      {
        const float w = src.get(L::BN2W + j), b = src.get(L::BN2B + j);
        float rm, rv;
        stat(NIN + kHidden + j, rm, rv);
        bn_fold(w, b, rm, rv, a2, c2);
      }
    }
  }

  // policy input for lane j < NIN from the (already obs-normalised) observation value
  __device__ __forceinline__ float input_transform(float x) const {
    if constexpr (DISC) {
      return fmaf(x, a0, c0);  // BatchNorm1d(n_in), eval mode
    } else {
      return x;
    }
  }

  // First hidden layer of unit j against the broadcast input xs (xs[NIN] == 1 picks up the folded
  // bias).
  __device__ __forceinline__ float layer1(const float (&xs)[NX]) const {
    f2 acc = {b1, 0.f};
    if constexpr (kW1Lds) {
#pragma unroll
      for (int q = 0; q < NX / 4; ++q) {
        const float4 w = tile[q * kWave];
        acc = pk_fma(f2{w.x, w.y}, f2{xs[4 * q], xs[4 * q + 1]}, acc);
        acc = pk_fma(f2{w.z, w.w}, f2{xs[4 * q + 2], xs[4 * q + 3]}, acc);
      }
    } else {
#pragma unroll
      for (int p = 0; p < NX / 2; ++p) acc = pk_fma(w1[p], f2{xs[2 * p], xs[2 * p + 1]}, acc);
    }
    const float z = acc.x + acc.y;
    if constexpr (DISC) {
      return fmaf(fmaxf(z, 0.f), a1, c1);
    } else {
      return tanh_fast(z);
    }
  }

  // First hidden layer and the env's M s in one pass over the broadcast input chunks (LDS):
  // returns unit j's activation, sets env = M[j] . x.  Chunks are consumed as they arrive so at most
  // two are live (VGPR budget: W2 holds 64 of the 128).
  // ss: the env state's broadcast copy when it differs from the policy input (nullptr: same)
  template <bool kSameInput>
  __device__ __forceinline__ float layer1_env_pk(const float* xs, const float* ss, const float* mrow,
                                                 float& env) const {
    const float4* x4 = reinterpret_cast<const float4*>(xs);
    const float4* s4 = reinterpret_cast<const float4*>(ss);
    const float4* m4 = reinterpret_cast<const float4*>(mrow);
    // four independent chains: back-to-back dependent packed FMAs cost an s_nop each
    f2 acc0 = {b1, 0.f}, acc1 = {0.f, 0.f}, accm0 = {0.f, 0.f}, accm1 = {0.f, 0.f};
#pragma unroll
    for (int q = 0; q < NX / 4; ++q) {
      const float4 xv = x4[q], mv = m4[q];
      const float4 sv = kSameInput ? xv : s4[q];
      float4 w;
      if constexpr (kW1Lds) {
        w = tile[q * kWave];
      } else {
        w = float4{w1[2 * q].x, w1[2 * q].y, w1[2 * q + 1].x, w1[2 * q + 1].y};
      }
      acc0 = pk_fma(f2{w.x, w.y}, f2{xv.x, xv.y}, acc0);
      accm0 = pk_fma(f2{mv.x, mv.y}, f2{sv.x, sv.y}, accm0);
      acc1 = pk_fma(f2{w.z, w.w}, f2{xv.z, xv.w}, acc1);
      accm1 = pk_fma(f2{mv.z, mv.w}, f2{sv.z, sv.w}, accm1);
    }
    const f2 am = accm0 + accm1, ah = acc0 + acc1;
    env = am.x + am.y;
    const float z = ah.x + ah.y;
    if constexpr (DISC) {
      return fmaf(fmaxf(z, 0.f), a1, c1);
    } else {
      return tanh_fast(z);
    }
  }

  // Layer 1 and the env's M s from register-resident operands (rollout_kernel<WIDE>): the broadcast
  // input arrives through v_readlane (wave-uniform values), M row j is loop-invariant in VGPRs.
  __device__ __forceinline__ float layer1_env_reg(const float (&xv)[NX], const float (&sv)[NX],
                                                  const float (&mv)[NX], float& env) const {
    static_assert(!kW1Lds, "register-input layer 1 needs W1 in VGPRs");
    f2 acc0 = {b1, 0.f}, acc1 = {0.f, 0.f}, accm0 = {0.f, 0.f}, accm1 = {0.f, 0.f};
#pragma unroll
    for (int q = 0; q < NX / 4; ++q) {
      acc0 = pk_fma(w1[2 * q], f2{xv[4 * q], xv[4 * q + 1]}, acc0);
      accm0 = pk_fma(f2{mv[4 * q], mv[4 * q + 1]}, f2{sv[4 * q], sv[4 * q + 1]}, accm0);
      acc1 = pk_fma(w1[2 * q + 1], f2{xv[4 * q + 2], xv[4 * q + 3]}, acc1);
      accm1 = pk_fma(f2{mv[4 * q + 2], mv[4 * q + 3]}, f2{sv[4 * q + 2], sv[4 * q + 3]}, accm1);
    }
    const f2 am = accm0 + accm1, ah = acc0 + acc1;
    env = am.x + am.y;
    const float z = ah.x + ah.y;
    if constexpr (DISC) {
      return fmaf(fmaxf(z, 0.f), a1, c1);
    } else {
      return tanh_fast(z);
    }
  }

  // this lane's W3 slice (the head's loop-invariant LDS tile chunks) into registers
  __device__ __forceinline__ void head_weights(float (&w3)[16]) const {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const float4 w = tile[(kW1Chunks + m) * kWave];
      w3[4 * m] = w.x;
      w3[4 * m + 1] = w.y;
      w3[4 * m + 2] = w.z;
      w3[4 * m + 3] = w.w;
    }
  }

  // second hidden layer and the head: h = layer-1 output of unit j; returns the head
  // pre-activation for output o = j & 15 (identical in the 4 rows).  w3r: the head's W3 slice when the
  // caller keeps it in registers (nullptr: read from the LDS tile each step).
  template <class Mark>
  __device__ __forceinline__ float layers23(float h, Scratch* sc, int j, Mark&& mark,
                                            const float* w3r = nullptr) const {
    const float h2 = layer2(h, sc, j);
    mark(1, h2);
    // h2[16q + i] sits in lane i of row q: DPP row_newbcast FMAs, no LDS round trip
    float w3[16];
    if (w3r) {
#pragma unroll
      for (int i = 0; i < 16; ++i) w3[i] = w3r[i];
    } else {
      head_weights(w3);
    }
    const float out = row_allreduce_sum(dot_row16(h2, w3)) + b3;
    mark(2, out);
    return out;
  }

  // Two-output head (discrete NA == 2, rollout_kernel<WIDE>): lane j multiplies its own unit h2[j] by
  // w3c = (W3[0][j], W3[1][j]), keeps the product of output o = j & 1 and hands the other to its quad
  // partner, then sums over the 32 lanes of its parity (row_ror 4, row_ror 8, quad xor 2, the 4-row
  // permlane all-reduce): output o in every lane of parity o, 9 VALU instead of the 16-DPP-FMA dot.
  // kKeepFirst: w3c already holds (W3[o][j], W3[1 - o][j]) (the WIDE kernel), so no selects
  template <bool kKeepFirst = false>
  __device__ __forceinline__ float head2(float h2, f2 w3c, float b3p, int j) const {
    const f2 m = w3c * f2{h2, h2};
    const bool odd = !kKeepFirst && (j & 1) != 0;
    const float keep = odd ? m.y : m.x, give = odd ? m.x : m.y;
    float v = keep + dpp_mov<kDppQuadXor1>(give);
    v += dpp_mov<kDppRowRor + 4>(v);
    v += dpp_mov<kDppRowRor + 8>(v);
    v += dpp_mov<kDppQuadXor2>(v);
    return row_allreduce_sum(v) + b3p;
  }

  // second hidden layer: h = layer-1 output of unit j; returns unit j's activation.  kAsm (the 256-VGPR WIDE
  // kernel only: in the 128-VGPR instances the asm block's live range spills): op_sel block, b2 in the own slot
  template <bool kAsm = false>
  __device__ __forceinline__ float layer2(float h, Scratch* sc, int j) const {
    const int c = j & 7;
    sc->h1[j] = h;
    wave_lds_sync();
    float x[8];
    lds_bcast<8>(sc->h1 + 8 * c, x);
    f2 acc[4];
    float kB2;
    if constexpr (kAsm) {
    // k = 0 starts the lane's own slot (acc[0].x, the reduce-scatter's non-DPP operand all the way down) from b2;
    // k = 1 .. 7 as op_sel broadcasts of the pairs (x[2j], x[2j + 1]) in one asm statement (no moves of odd
    // elements; operands %0-%3 acc, %(4 + 4 (k - 1) + p) = w2[8 p + k], %32-%35 the pairs)
#pragma unroll
    for (int p = 0; p < 4; ++p) acc[p] = pk_fma(w2[p * 8], f2{x[0], x[0]}, f2{p == 0 ? b2 : 0.f, 0.f});
    {
      const f2 x01 = {x[0], x[1]}, x23 = {x[2], x[3]}, x45 = {x[4], x[5]}, x67 = {x[6], x[7]};
#define FDR_L2_HI "op_sel:[0,1,0] op_sel_hi:[1,1,1]"
#define FDR_L2_LO "op_sel_hi:[1,0,1]"
      asm(
          "v_pk_fma_f32 %0, %4, %32, %0 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %1, %5, %32, %1 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %2, %6, %32, %2 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %3, %7, %32, %3 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %0, %8, %33, %0 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %1, %9, %33, %1 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %2, %10, %33, %2 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %3, %11, %33, %3 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %0, %12, %33, %0 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %1, %13, %33, %1 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %2, %14, %33, %2 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %3, %15, %33, %3 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %0, %16, %34, %0 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %1, %17, %34, %1 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %2, %18, %34, %2 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %3, %19, %34, %3 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %0, %20, %34, %0 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %1, %21, %34, %1 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %2, %22, %34, %2 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %3, %23, %34, %3 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %0, %24, %35, %0 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %1, %25, %35, %1 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %2, %26, %35, %2 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %3, %27, %35, %3 " FDR_L2_LO "\n"
          "v_pk_fma_f32 %0, %28, %35, %0 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %1, %29, %35, %1 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %2, %30, %35, %2 " FDR_L2_HI "\n"
          "v_pk_fma_f32 %3, %31, %35, %3 " FDR_L2_HI "\n"
          : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3])
          : "v"(w2[1]), "v"(w2[9]), "v"(w2[17]), "v"(w2[25]),
            "v"(w2[2]), "v"(w2[10]), "v"(w2[18]), "v"(w2[26]),
            "v"(w2[3]), "v"(w2[11]), "v"(w2[19]), "v"(w2[27]),
            "v"(w2[4]), "v"(w2[12]), "v"(w2[20]), "v"(w2[28]),
            "v"(w2[5]), "v"(w2[13]), "v"(w2[21]), "v"(w2[29]),
            "v"(w2[6]), "v"(w2[14]), "v"(w2[22]), "v"(w2[30]),
            "v"(w2[7]), "v"(w2[15]), "v"(w2[23]), "v"(w2[31]),
            "v"(x01), "v"(x23), "v"(x45), "v"(x67));
#undef FDR_L2_LO
#undef FDR_L2_HI
    }
    kB2 = 0.f;
    } else {
#pragma unroll
    for (int p = 0; p < 4; ++p) acc[p] = f2{0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
      for (int p = 0; p < 4; ++p) acc[p] = pk_fma(w2[p * 8 + k], f2{x[k], x[k]}, acc[p]);
    kB2 = b2;
    }
    // reduce-scatter over the 8 lanes of the half-row: slot i = acc[i / 2][i % 2]
    const float q0 = acc[0].x + dpp_mov<kDppHalfMirror>(acc[2].x);
    const float q1 = acc[0].y + dpp_mov<kDppHalfMirror>(acc[2].y);
    const float q2 = acc[1].x + dpp_mov<kDppHalfMirror>(acc[3].x);
    const float q3 = acc[1].y + dpp_mov<kDppHalfMirror>(acc[3].y);
    const float r0 = q0 + dpp_mov<kDppQuadXor2>(q2);
    const float r1 = q1 + dpp_mov<kDppQuadXor2>(q3);
    const float z = kAsm ? r0 + dpp_mov<kDppQuadXor1>(r1) : (r0 + dpp_mov<kDppQuadXor1>(r1)) + kB2;
    if constexpr (DISC) {
      return fmaf(fmaxf(z, 0.f), a2, c2);
    } else {
      return tanh_fast(z);
    }
  }

  // Discrete: softmax across the row (o = j & 15 < NA); returns p_o, 0 for o >= NA.  kAll: every lane
  // holds a logit (head2: output j & 1).  kFast (sampled lanes): exp as v_exp_f32 of x log2 e and
  // the normalisation as a v_rcp_f32 product -- 4 VALU instead of libm expf (13) + the IEEE division (11); the
  // probabilities move by ~1e-7 relative (inside the 1e-5 forward tolerance), so a sampled action can differ
  // from the exact form's only where u * sum p lies within that of a partition boundary.  Deterministic lanes
  // (argmax, the trap env's integer-exact episodes) keep the exact form.
  template <bool kAll = false, bool kFast = false>
  __device__ __forceinline__ float softmax(float logit, int j) const {
    const bool valid = kAll || (j & 15) < NOUT;
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

}  // namespace fdr
