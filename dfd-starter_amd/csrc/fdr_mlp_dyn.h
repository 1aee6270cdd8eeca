// fdr_mlp_dyn.h -- DynLane: MlpLane (fdr_mlp_lane.h) with the policy's n_in / n_act as runtime values, for the
// runtime-shaped kernel family of fdr_rollout_dyn.hip (rollout_dyn_kernel, policy_forward_dyn_kernel,
// theta_prime_dyn_kernel).  One wave per lane, hidden width 64 = the wave width: thread j owns hidden unit j.
//
// Same arithmetic as MlpLane, operation for operation (the same packed-FMA chains, reduce-scatter, DPP head and
// softmax), so a shape both families can run differs only where the compiler schedules differently:
//   W2        8 x 8 lane blocks in 64 VGPRs (H is a constant), MlpLane's layout and reduce-scatter;
//   W1 row j  always in the per-wave LDS tile ([chunk][lane] float4), round4(n_in) / 4 chunks -- a runtime loop.
//             MlpLane's bias rule: b1 folded into column n_in when n_in is not a multiple of 4, else a register
//             (so n_in == 64, which has no spare input slot, is the register case);
//   W3        lane (q, o): W3[o][16q .. 16q + 15] in the 4 chunks behind W1; o >= n_out holds zeros;
//   n_out     enters the head only through o < n_out: the row reductions run all four levels (lanes 0 .. n_out-1
//             get the values of MlpLane's truncated ones: the extra levels add zeros / compare with -FLT_MAX).
#pragma once
#include "fdr_mlp_lane.h"

namespace fdr {

// runtime limits of the family: what Layout states (fdr_mlp.h)
constexpr int kDynMaxIn = 64, kDynMaxActDisc = 16, kDynMaxActCont = 8;

// Layout<NIN, NA, DISC> with runtime n_in / n_act
template <bool DISC>
struct DynLayout {
  int n_in, n_act, n_out, nx;  // nx = round4(n_in)
  int64_t BN0W, BN0B, L1W, L1B, BN1W, BN1B, L2W, L2B, BN2W, BN2B, L3W, L3B, P;

  __host__ __device__ DynLayout(int n_in_, int n_act_) : n_in(n_in_), n_act(n_act_) {
    constexpr int64_t H = kHidden;
    n_out = DISC ? n_act : 2 * n_act;
    nx = round4(n_in);
    BN0W = 0;
    BN0B = n_in;
    L1W = DISC ? 2 * n_in : 0;
    L1B = L1W + H * n_in;
    BN1W = L1B + H;
    BN1B = BN1W + H;
    L2W = DISC ? BN1B + H : L1B + H;
    L2B = L2W + H * H;
    BN2W = L2B + H;
    BN2B = BN2W + H;
    L3W = DISC ? BN2B + H : L2B + H;
    L3B = L3W + (int64_t)n_out * H;
    P = L3B + n_out;
  }
  __host__ __device__ bool bias_col() const { return n_in < nx; }
  __host__ __device__ int w1_chunks() const { return nx / 4; }
  __host__ __device__ int tile_f4() const { return (w1_chunks() + 4) * kWave; }  // float4 per wave
};

template <bool DISC>
struct DynLane {
  using L = DynLayout<DISC>;
  using Scratch = WaveScratch;
  int n_in, n_out, nxc;  // nxc: W1 chunks
  float b1;
  const float4* tile;  // this lane's column of the tile (chunk m at tile[m * kWave])
  f2 w2[32];           // MlpLane::w2
  float b2, b3;
  float a0, c0, a1, c1, a2, c2;  // discrete: folded BN for input j / hidden unit j

  // Src: ParamSrc, or RecordSrc (the theta' read-back).  Every parameter is counted once into src.n2; every load is
  // unconditional (clamped indices, get_if).
  template <class Src>
  __device__ __forceinline__ void load(const L& l, Src& src, int j, const float* bn_mean, const float* bn_var,
                                       float4* lds_tile) {
    const int r = j >> 3, c = j & 7, o = j & 15, q = j >> 4;
    n_in = l.n_in;
    n_out = l.n_out;
    nxc = l.w1_chunks();
    tile = lds_tile + j;
    float4* my = lds_tile + j;
    const bool bias_col = l.bias_col();
    // column k of row j: W1[j][k], the folded bias at k == n_in, zero padding behind it (read from the bias's
    // address, not counted)
    auto w1v = [&](int k) {
      const bool w = k < n_in, use = w || (bias_col && k == n_in);
      const float v = src.get_if(w ? l.L1W + (int64_t)j * n_in + k : l.L1B + j, use);
      return use ? v : 0.f;
    };
    for (int m = 0; m < nxc; ++m) {
      const float e0 = w1v(4 * m), e1 = w1v(4 * m + 1), e2 = w1v(4 * m + 2), e3 = w1v(4 * m + 3);
      my[m * kWave] = float4{e0, e1, e2, e3};
    }
    {
      const float v = src.get_if(l.L1B + j, !bias_col);
      b1 = bias_col ? 0.f : v;
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int row0 = 8 * r + (c ^ l2_sigma(2 * p)), row1 = 8 * r + (c ^ l2_sigma(2 * p + 1));
#pragma unroll
      for (int k = 0; k < 8; ++k)
        w2[p * 8 + k] = f2{src.get(l.L2W + (int64_t)row0 * kHidden + 8 * c + k),
                           src.get(l.L2W + (int64_t)row1 * kHidden + 8 * c + k)};
      // the group's weights and norm terms are final here (MlpLane::load: no deferred work held in scratch)
#pragma unroll
      for (int k = 0; k < 8; ++k) asm volatile("" : "+v"(w2[p * 8 + k]));
      asm volatile("" : "+v"(src.n2));
      __builtin_amdgcn_sched_barrier(0);
    }
    b2 = src.get(l.L2B + j);
    {
      const bool has_o = o < n_out;
      const int oc = has_o ? o : 0;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int64_t base = l.L3W + (int64_t)oc * kHidden + 16 * q + 4 * m;
        const float e0 = src.get_if(base, has_o), e1 = src.get_if(base + 1, has_o), e2 = src.get_if(base + 2, has_o),
                    e3 = src.get_if(base + 3, has_o);
        my[(nxc + m) * kWave] = has_o ? float4{e0, e1, e2, e3} : float4{0.f, 0.f, 0.f, 0.f};
      }
      const float b3v = src.get_if(l.L3B + oc, has_o && q == 0);
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
        const bool in = j < n_in;
        const int jc = in ? j : 0;
        const float w = src.get_if(l.BN0W + jc, in), b = src.get_if(l.BN0B + jc, in);
        float rm, rv, a, cc;
        stat(jc, rm, rv);
        bn_fold(w, b, rm, rv, a, cc);
        a0 = in ? a : 0.f;
        c0 = in ? cc : 0.f;
      }
      {
        const float w = src.get(l.BN1W + j), b = src.get(l.BN1B + j);
        float rm, rv;
        stat(n_in + j, rm, rv);
        bn_fold(w, b, rm, rv, a1, c1);
      }
      {
        const float w = src.get(l.BN2W + j), b = src.get(l.BN2B + j);
        float rm, rv;
        stat(n_in + kHidden + j, rm, rv);
        bn_fold(w, b, rm, rv, a2, c2);
      }
    }
  }

  __device__ __forceinline__ float input_transform(float x) const {
    if constexpr (DISC) return fmaf(x, a0, c0);  // BatchNorm1d(n_in), eval mode
    else return x;
  }
  // the value thread j writes into the broadcast input slot: the transformed input, the 1 of the folded bias column
  // (only when the column exists: n_in == 64 has no slot 64), zero padding
  __device__ __forceinline__ float input_slot(int j, float xin) const { return j < n_in ? xin : (j == n_in ? 1.f : 0.f); }

  __device__ __forceinline__ float act1(float z) const {
    if constexpr (DISC) return fmaf(fmaxf(z, 0.f), a1, c1);
    else return tanh_fast(z);
  }

  // MlpLane::layer1 over a runtime chunk count: unit j against the broadcast input xs (LDS)
  __device__ __forceinline__ float layer1(const float* xs) const {
    const float4* x4 = reinterpret_cast<const float4*>(xs);
    f2 acc = {b1, 0.f};
    for (int q = 0; q < nxc; ++q) {
      const float4 w = tile[q * kWave], x = x4[q];
      acc = pk_fma(f2{w.x, w.y}, f2{x.x, x.y}, acc);
      acc = pk_fma(f2{w.z, w.w}, f2{x.z, x.w}, acc);
    }
    return act1(acc.x + acc.y);
  }

  // MlpLane::layer1_env_pk over a runtime chunk count: unit j's activation, env = M[j] . s
  __device__ __forceinline__ float layer1_env(const float* xs, const float* ss, const float* mrow, float& env) const {
    const float4* x4 = reinterpret_cast<const float4*>(xs);
    const float4* s4 = reinterpret_cast<const float4*>(ss);
    const float4* m4 = reinterpret_cast<const float4*>(mrow);
    f2 acc0 = {b1, 0.f}, acc1 = {0.f, 0.f}, accm0 = {0.f, 0.f}, accm1 = {0.f, 0.f};
    for (int q = 0; q < nxc; ++q) {
      const float4 xv = x4[q], mv = m4[q], sv = s4[q], w = tile[q * kWave];
      acc0 = pk_fma(f2{w.x, w.y}, f2{xv.x, xv.y}, acc0);
      accm0 = pk_fma(f2{mv.x, mv.y}, f2{sv.x, sv.y}, accm0);
      acc1 = pk_fma(f2{w.z, w.w}, f2{xv.z, xv.w}, acc1);
      accm1 = pk_fma(f2{mv.z, mv.w}, f2{sv.z, sv.w}, accm1);
    }
    const f2 am = accm0 + accm1, ah = acc0 + acc1;
    env = am.x + am.y;
    return act1(ah.x + ah.y);
  }

  // MlpLane::layer2 (the plain form) and the head: returns the head pre-activation of output o = j & 15
  __device__ __forceinline__ float layers23(float h, Scratch* sc, int j) const {
    const int c = j & 7;
    sc->h1[j] = h;
    wave_lds_sync();
    float x[8];
    lds_bcast<8>(sc->h1 + 8 * c, x);
    f2 acc[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) acc[p] = f2{0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
      for (int p = 0; p < 4; ++p) acc[p] = pk_fma(w2[p * 8 + k], f2{x[k], x[k]}, acc[p]);
    const float q0 = acc[0].x + dpp_mov<kDppHalfMirror>(acc[2].x);
    const float q1 = acc[0].y + dpp_mov<kDppHalfMirror>(acc[2].y);
    const float q2 = acc[1].x + dpp_mov<kDppHalfMirror>(acc[3].x);
    const float q3 = acc[1].y + dpp_mov<kDppHalfMirror>(acc[3].y);
    const float r0 = q0 + dpp_mov<kDppQuadXor2>(q2);
    const float r1 = q1 + dpp_mov<kDppQuadXor2>(q3);
    const float z = (r0 + dpp_mov<kDppQuadXor1>(r1)) + b2;
    float h2;
    if constexpr (DISC) h2 = fmaf(fmaxf(z, 0.f), a2, c2);
    else h2 = tanh_fast(z);
    float w3[16];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const float4 w = tile[(nxc + m) * kWave];
      w3[4 * m] = w.x;
      w3[4 * m + 1] = w.y;
      w3[4 * m + 2] = w.z;
      w3[4 * m + 3] = w.w;
    }
    return row_allreduce_sum(dot_row16(h2, w3)) + b3;
  }

  // MlpLane::softmax with a runtime output count: p_o, 0 for o >= n_out.  kFast: the sampled lanes' form.
  template <bool kFast>
  __device__ __forceinline__ float softmax(float logit, int j) const {
    const bool valid = (j & 15) < n_out;
    const float v = valid ? logit : -FLT_MAX;
    const float mx = row16_max(v);
    if constexpr (kFast) {
      const float e = valid ? __builtin_amdgcn_exp2f((v - mx) * 1.44269504088896341f) : 0.f;
      return e * __builtin_amdgcn_rcpf(row16_sum(e));
    } else {
      const float e = valid ? expf(v - mx) : 0.f;
      return e / row16_sum(e);
    }
  }
};

// lane o <- lane o + n of the same row (n_act + o < 16 wherever the result is used): MlpLane's
// dpp_mov<kDppRowShl + NA> with a runtime shift (ds_bpermute: no LDS memory is touched)
__device__ __forceinline__ float row_shl_dyn(float v, int j, int n) {
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(4 * ((j + n) & 63), __builtin_bit_cast(int, v)));
}

}  // namespace fdr
