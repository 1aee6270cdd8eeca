// fdr_impala_f32.hip -- ImpalaPolicy device code in f32: the conv stack, the LSTM core step in its per-lane, pair and
// pair-replay forms, and the two row GEMMs (entropy replay input projection, get_strategy fc).  The GEMMs' HALF
// instances read the half pack but are the same template.  Launched from fdr_impala.hip; declarations:
// fdr_impala_kernels.h; the core step's shared phases: fdr_impala_core.h.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "fdr_impala_core.h"

namespace fdr {
namespace impala {

// ------------------------------------------------------------------------------------------
// conv stack: one workgroup (8 waves) per (lane, env); everything between the frame and the
// 2048-feature stays in LDS (all 160 KiB; floats):
//   [guard 128][TE 23,488: padded input image T of the current conv + band scratch S][X 16,384]
//   [BN scale/shift 960]
// Padded planes are strided so the 4 lane groups of an MFMA A-read (4 input channels) start 16
// banks apart: plane % 64 == 16 (32x32 and 16x16 stages) -> conflict-free ds_read_b32.
// ------------------------------------------------------------------------------------------
constexpr int kGuard = 128;          // padded rows above T: the band of conv row -1 reads them
constexpr int kTE = 23488;
constexpr int kRX = 16 * 32 * 32;
constexpr int kConvLds = kGuard + kTE + kRX + 2 * kBnTab;  // 40,960 floats = 160 KiB
constexpr int kBand = 9;             // conv rows per entry-conv band: 4 pooled rows + 1 shared row

template <int H>
struct Plane {  // padded [H+2][H+2] image, bank-staggered plane stride
  static constexpr int WP = H + 2;
  static constexpr int RAW = WP * WP;
  static constexpr int P = H == 64 ? RAW : RAW + ((16 - RAW % 64) % 64 + 64) % 64 + (H == 8 ? 2 : 0);
};
static_assert(Plane<32>::P == 1168 && Plane<16>::P == 336 && Plane<8>::P == 146, "plane strides");

// Channel skew of a padded plane (words), for the strides = 16 (mod 32) banks.  ds_write_b32 banks are
// (a/4) mod 32 over 32-lane halves: an epilogue store of one M-tile (lanes: 16 channels x 2 pixel
// quads) then hits 4 banks in 32 without the skew, an 8-way conflict (r05 PMC: SQ_LDS_BANK_CONFLICT
// 15 % of the conv kernel's cycles).  With bits (c>>1)&1 -> 8 and (c>>2)&3 -> 0..3 the 32 lanes land on 32
// banks.  An MFMA A-read takes channels 4q + g (g = lane >> 4): its skew (g>>1) 8 + (q & 3) is uniform
// per 32-lane half, so the reads stay conflict-free.
template <int PLANE>
__device__ __forceinline__ constexpr int cskew(int c) {
  return PLANE % 32 == 16 ? ((c >> 1) & 1) * 8 + ((c >> 2) & 3) : 0;
}
constexpr int kSkewPad = 16;  // room for the last plane's skew (<= 11) before the next region

// X [C][H][H] with a per-channel XOR on bits 2-5 of the pixel index (HH >= 64): the residual read-modify-
// write of an epilogue (lane: channel n, 4 pixels) goes from 16 channels on one 4-bank group to 16
// distinct groups (ds_read_b128 / ds_write_b128 conflict-free); pool writes and the float4 reads of
// to_padded stay contiguous.
template <int HH>
__device__ __forceinline__ int xpos(int c, int m) {
  static_assert(HH >= 64, "swizzle spans 64 pixels");
  return c * HH + (m ^ ((c & 15) << 2));
}

static_assert(16 * Plane<32>::P + kSkewPad <= kTE && 3 * Plane<64>::P + 16 * kBand * 65 <= kTE, "LDS plan");
static_assert(16 * Plane<32>::P + kSkewPad + 32 * kBand * 33 + 32 * 16 * 16 <= kTE + kRX, "LDS plan, stage 2");
static_assert(32 * Plane<16>::P + kSkewPad + 32 * 17 * 17 + 32 * 8 * 8 <= kTE + kRX, "LDS plan, stage 3");


// B fragments of one conv for this wave's N-tile: bf[s] = B[k = 4s + (lane >> 4)][n], one VGPR each.
template <int CIN, int NT>
__device__ __forceinline__ void load_frag(const float* __restrict__ wf, float (&bf)[(9 * CIN + 3) / 4], int wave,
                                          int lane) {
  constexpr int KS = (9 * CIN + 3) / 4;
  const int nt = wave % NT;
#pragma unroll
  for (int s = 0; s < KS; ++s) bf[s] = wf[(s * NT + nt) * 64 + lane];
}

// acc[i] (tile q = wave + 8 i) = A_tile(q) * B over K = 9 * CIN on v_mfma_f32_16x16x4_f32, A gathered
// from the padded LDS image Tin ([CIN][*][WP] with plane stride PLANE, row 0 = padded row of output
// row 0).  M-tile = 16 consecutive output pixels (row-major, width W).
template <int CIN, int NT, int TPW, int W, int WP, int PLANE, int MT>
__device__ __forceinline__ void conv_mfma(const float* Tin, const float (&bf)[(9 * CIN + 3) / 4], f32x4 (&acc)[TPW],
                                          int wave, int lane) {
  constexpr int KS = (9 * CIN + 3) / 4;
  int base[TPW];
  const int g = lane >> 4;
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    int mt = (wave + 8 * i) / NT;
    mt = mt < MT ? mt : MT - 1;
    const int m = mt * 16 + (lane & 15);
    base[i] = (m / W) * WP + (m % W);
    acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  if constexpr ((CIN & 3) == 0) {
#pragma unroll
    for (int i = 0; i < TPW; ++i) base[i] += g * PLANE + cskew<PLANE>(g);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int tap = s / (CIN / 4), q = s % (CIN / 4);
      const int off = 4 * q * PLANE + cskew<PLANE>(4 * q) + (tap / 3) * WP + (tap % 3);
#pragma unroll
      for (int i = 0; i < TPW; ++i)
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(Tin[base[i] + off], bf[s], acc[i], 0, 0, 0);
    }
  } else {
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = 4 * s + g;
      const int tap = k / CIN, ci = k - tap * CIN;
      const int off = k < 9 * CIN ? ci * PLANE + cskew<PLANE>(ci) + (tap / 3) * WP + (tap % 3) : 0;  // pad k: weight 0
#pragma unroll
      for (int i = 0; i < TPW; ++i)
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(Tin[base[i] + off], bf[s], acc[i], 0, 0, 0);
    }
  }
}

// Visit the outputs of conv_mfma: f(n, m, v) for channel n, output pixel m (row-major, width W).
template <int NT, int TPW, int MT, typename F>
__device__ __forceinline__ void conv_out(const f32x4 (&acc)[TPW], int wave, int lane, F f) {
  const int n = (wave % NT) * 16 + (lane & 15);
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int q = wave + 8 * i;
    if (q / NT >= MT) continue;
    const int m0 = (q / NT) * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) f(n, m0 + r, acc[i][r]);
  }
}

// T <- BN(X) (optionally ReLU) into the padded image [C][H+2][H+2] (plane stride Plane<H>::P).
// BORDER: also write the zero border (needed when T last held another layout).
template <int C, int H, bool RELU, bool BORDER>
__device__ __forceinline__ void to_padded(const float* X, float* T, const float* sc, const float* sh) {
  constexpr int WP = Plane<H>::WP, PL = Plane<H>::P, LH = H == 64 ? 6 : (H == 32 ? 5 : (H == 16 ? 4 : 3));
  // interior, 4 consecutive x per thread (one ds_read_b128 of X)
  for (int i = threadIdx.x; i < C * H * H / 4; i += kConvThreads) {
    const int e = 4 * i, ch = e >> (2 * LH), y = (e >> LH) & (H - 1), x = e & (H - 1);
    const float4 v = *reinterpret_cast<const float4*>(X + xpos<H * H>(ch, e & (H * H - 1)));
    const float a = sc[ch], b = sh[ch];
    float o0 = fmaf(v.x, a, b), o1 = fmaf(v.y, a, b), o2 = fmaf(v.z, a, b), o3 = fmaf(v.w, a, b);
    if (RELU) { o0 = relu(o0); o1 = relu(o1); o2 = relu(o2); o3 = relu(o3); }
    float* d = T + ch * PL + cskew<PL>(ch) + (y + 1) * WP + x + 1;
    d[0] = o0; d[1] = o1; d[2] = o2; d[3] = o3;
  }
  if (BORDER) {  // 4 (H + 1) border cells per plane
    for (int i = threadIdx.x; i < C * 4 * (H + 1); i += kConvThreads) {
      const int ch = i / (4 * (H + 1)), r = i - ch * 4 * (H + 1), side = r / (H + 1), k = r - side * (H + 1);
      const int off = side == 0 ? k : side == 1 ? (H + 1) * WP + 1 + k : side == 2 ? (k + 1) * WP : k * WP + WP - 1;
      T[ch * PL + cskew<PL>(ch) + off] = 0.f;
    }
  }
}

// Stage entry: X <- maxpool3s2p1(conv3x3(T) + b) in bands of BR-1 new conv rows (8 b .. 8 b + 7 for
// BR = 9) through the scratch S [COUT][BR][1 + H], a RING of conv rows: conv row g lives in slot
// (g + 1) mod BR, so a band's pool window (rows 8 b - 1 .. 8 b + 7) is the previous band's last row
// plus the new ones -- no row is computed twice and every band is (BR-1) H / 16 tiles (a multiple
// of the 8 waves).  Column -1 of S is -inf (the pool's left pad) and conv row -1 (slot 0 before
// band 0) is -inf, so the pool is branch-free and separable -- one thread per (channel, pooled
// column): BR horizontal max3, then vertical max3.  The B fragments are loaded by the caller and
// reused by every band.
template <int CIN, int COUT, int H, int PLANE, int BR>
__device__ __forceinline__ void stage_entry(const float* T, float* S, float* X, const float (&bf)[(9 * CIN + 3) / 4],
                                            const float* __restrict__ bias, int wave, int lane, const StepArgs& a,
                                            int kst) {
  constexpr int WP = H + 2, NT = COUT / 16, NR = BR - 1, MT = NR * H / 16, PRB = NR / 2;
  constexpr int TPW = (MT * NT + 7) / 8, HO = H / 2, SW = H + 1;
  static_assert((NR * H) % 16 == 0 && H % NR == 0 && NR % 2 == 0, "band shape");
  const float bn_ = bias[(wave % NT) * 16 + (lane & 15)];
  uint64_t t_conv = 0, t_pool = 0, t0 = a.dbg ? clock64() : 0;  // diagnostics (fdr_impala_debug_clock)
  // H = 64: a scratch row holds the even columns, the pad (column -1), then the odd columns, so the pool's
  // reads of columns 2px-1, 2px, 2px+1 are unit-stride across the 32 lanes of one channel (interleaved: stride
  // 2, 2-way conflicts; stage-1 pool 10.2 K -> 7.5 K clocks).  H <= 32: the pad first, then columns in order --
  // a 32-lane half spans 2+ channels whose odd channel stride puts them on the other bank parity.
  constexpr bool DI = HO >= 32;
  constexpr int PAD = DI ? HO : 0;
  auto col = [](int x) { return DI ? ((x & 1) ? HO + 1 + (x >> 1) : (x >> 1)) : 1 + x; };
  for (int i = threadIdx.x; i < COUT * BR; i += kConvThreads) S[i * SW + PAD] = -FLT_MAX;  // pad column
  for (int i = threadIdx.x; i < COUT * H; i += kConvThreads)                              // conv row -1
    S[(i / H) * BR * SW + col(i % H)] = -FLT_MAX;
  for (int b = 0; b < H / NR; ++b) {
    const int rot = (NR * b) % BR;  // slot of conv row NR b - 1
    auto slot = [&](int r) { return rot + r >= BR ? rot + r - BR : rot + r; };  // conv row NR b - 1 + r
    f32x4 acc[TPW];
    conv_mfma<CIN, NT, TPW, H, WP, PLANE, MT>(T + NR * b * WP, bf, acc, wave, lane);
    conv_out<NT, TPW, MT>(acc, wave, lane, [&](int n, int m, float v) {
      const int r = m / H, x = m % H;
      S[(n * BR + slot(r + 1)) * SW + col(x)] = v + bn_;
    });
    __syncthreads();
    if (a.dbg) {
      const uint64_t t1 = clock64();
      t_conv += t1 - t0;
      t0 = t1;
    }
    for (int i = threadIdx.x; i < COUT * HO; i += kConvThreads) {
      const int ch = i / HO, px = i - ch * HO;
      // columns 2px-1, 2px, 2px+1
      const float* sc = S + ch * BR * SW + (DI ? px : 2 * px);
      constexpr int c0 = DI ? HO : 0, c1 = DI ? 0 : 1, c2 = DI ? HO + 1 : 2;
      float hm[BR];
#pragma unroll
      for (int r = 0; r < BR; ++r) {  // conv row NR b - 1 + r
        const int sl = slot(r);
        hm[r] = fmaxf(fmaxf(sc[sl * SW + c0], sc[sl * SW + c1]), sc[sl * SW + c2]);
      }
#pragma unroll
      for (int pr = 0; pr < PRB; ++pr)
        X[xpos<HO * HO>(ch, (PRB * b + pr) * HO + px)] = fmaxf(fmaxf(hm[2 * pr], hm[2 * pr + 1]), hm[2 * pr + 2]);
    }
    __syncthreads();
    if (a.dbg) {
      const uint64_t t1 = clock64();
      t_pool += t1 - t0;
      t0 = t1;
    }
  }
  if (a.dbg && blockIdx.x == 0 && threadIdx.x == 0) {  // summed over the bands
    a.dbg[kst] = t_conv;
    a.dbg[kst + 1] = t_pool;
  }
}

// Two residual blocks (policies/impala.py:77-105, 152-157) on X [C][H][H], T [C][H+2][H+2] as the conv
// input.  On entry T must hold relu(bn0(X)) of block 0 with a zero border, and bf the B fragments of
// block 0's first conv.  Every BN (+ReLU) that follows a conv is fused into that conv's epilogue:
//   block 0 conv1 epilogue: X <- X + conv + b; T <- relu(bn0_block1(X))
//   block 1 conv1 epilogue: LAST == 0: T <- bn_entry(stage+1)(X + conv + b)  (the next stage's input,
//                           same padded geometry); LAST == 1: out <- relu(X + conv + b) (the features)
// Weights of the next conv are fetched right after the MFMAs that last read bf, ahead of the barrier.
template <int C, int H, int LAST>
__device__ __forceinline__ void res_blocks(float* T, float* X, float (&bf)[(9 * C + 3) / 4], const float* __restrict__ pk,
                                           const Layout& L, int stage, const float* bsc, const float* bsh, int wave,
                                           int lane, const StepArgs& a, int k0, float* __restrict__ out) {
  constexpr int WP = H + 2, PLANE = Plane<H>::P, NT = C / 16, MT = H * H / 16;
  constexpr int TPW = (MT * NT + 7) / 8;
  const int n_ = (wave % NT) * 16 + (lane & 15);
  auto tpos = [&](int n, int m) { return n * PLANE + cskew<PLANE>(n) + (m / H + 1) * WP + (m % H) + 1; };
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int i0 = stage * 5 + 1 + 2 * r, i1 = i0 + 1;
    FDR_STAMP(a, k0 + 4 * r);
    f32x4 acc[TPW];
    conv_mfma<C, NT, TPW, H, WP, PLANE, MT>(T, bf, acc, wave, lane);
    const float b0 = pk[L.conv_b[i0] + n_], s1 = bsc[i1 * 32 + n_], h1 = bsh[i1 * 32 + n_];
    load_frag<C, NT>(pk + L.conv_w[i1], bf, wave, lane);
    __syncthreads();  // every wave is done reading T
    FDR_STAMP(a, k0 + 4 * r + 1);
    conv_out<NT, TPW, MT>(acc, wave, lane, [&](int n, int m, float v) { T[tpos(n, m)] = relu(fmaf(v + b0, s1, h1)); });
    __syncthreads();
    FDR_STAMP(a, k0 + 4 * r + 2);
    conv_mfma<C, NT, TPW, H, WP, PLANE, MT>(T, bf, acc, wave, lane);
    const float b1 = pk[L.conv_b[i1] + n_];
    // BN that consumes this block's output: block 1's bn0, or the next stage's entry BN
    const int inext = r == 0 ? i1 + 1 : (stage + 1) * 5;
    const float s2 = (r == 1 && LAST) ? 0.f : bsc[inext * 32 + n_];
    const float h2 = (r == 1 && LAST) ? 0.f : bsh[inext * 32 + n_];
    __syncthreads();  // every wave is done reading T
    FDR_STAMP(a, k0 + 4 * r + 3);
    if (r == 0) {
      // two passes over the accumulators (X update, then T) keep the live set small
#pragma unroll
      for (int i = 0; i < TPW; ++i) {
        const int q = wave + 8 * i;
        if (q / NT >= MT) continue;
        const int m0 = (q / NT) * 16 + (lane >> 4) * 4;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int xp = xpos<H * H>(n_, m0) + rr;  // the swizzle keeps the 4 pixels contiguous
          const float xn = (acc[i][rr] + b1) + X[xp];
          X[xp] = xn;
          acc[i][rr] = xn;
        }
      }
      conv_out<NT, TPW, MT>(acc, wave, lane, [&](int n, int m, float v) { T[tpos(n, m)] = relu(fmaf(v, s2, h2)); });
      load_frag<C, NT>(pk + L.conv_w[i1 + 1], bf, wave, lane);  // block 1's first conv
    } else if (!LAST) {
      conv_out<NT, TPW, MT>(acc, wave, lane, [&](int n, int m, float v) {
        T[tpos(n, m)] = fmaf((v + b1) + X[xpos<H * H>(n, m)], s2, h2);
      });
    } else {
      conv_out<NT, TPW, MT>(acc, wave, lane, [&](int n, int m, float v) {
        out[n * H * H + m] = relu((v + b1) + X[xpos<H * H>(n, m)]);   // flatten (C, H, W), impala.py:159-160
      });
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kConvThreads) void conv_kernel(Layout L, StepArgs a) {
  __shared__ float lds[kConvLds];
  // XCD-aware: the E workgroups of one lane run on one XCD, back to back (shared weights in L2)
  const int b = blockIdx.x, xcd = b & 7, slot = b >> 3;
  const int lane = (slot / a.envs) * 8 + xcd, e = slot % a.envs;
  if (lane >= a.n_lanes) return;
  const int wave = threadIdx.x >> 6, ln = threadIdx.x & 63;
  const int64_t env = (int64_t)lane * a.envs + e;
  const float* pk = a.pack + (int64_t)lane * a.pack_stride;
  float* T = lds + kGuard;
  float* X = T + kTE;
  float* bsc = X + kRX;
  float* bsh = bsc + kBnTab;
  constexpr int FW = 66, FPLANE = Plane<64>::P;

  float bf3[7];
  load_frag<3, 1>(pk + L.conv_w[0], bf3, wave, ln);
  FDR_STAMP(a, 0);
  // eval-mode BN folded per channel: y = x * (w / sqrt(rv + eps)) + (b - rm * scale).  Branch-free (r11, as
  // conv_kernel_h2's table): every load unconditional from a valid address, the unused values selected away after,
  // the layout offsets as scalar loads of the wave's two table rows -- a conditional load ends its basic block
  // with a full vmcnt wait, and the per-lane offset reads were a dependent round trip of their own
  static_assert(kBnTab <= kConvThreads, "one table entry per thread");
  {
    const int i = threadIdx.x, idx = i >> 5, ch = i & 31;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), hi = (threadIdx.x >> 5) & 1;
    const int r0 = min(2 * wv, kConvs - 1), r1 = min(2 * wv + 1, kConvs - 1);  // wave-uniform rows
    auto pick = [&](const int32_t* arr) { return hi ? arr[r1] : arr[r0]; };
    const float* bmp = a.bn_mean ? a.bn_mean : pk;
    const float* bvp = a.bn_var ? a.bn_var : pk;
    const int so = pick(L.bn_stat) + ch;
    const float rm_ = bmp[so], rv_ = bvp[so], w_ = pk[pick(L.bn_w) + ch], b_ = pk[pick(L.bn_b) + ch];
    const int nch = idx == 0 ? 3 : (idx == 5 ? 16 : (idx < 5 ? 16 : 32));
    const bool live = i < kBnTab && ch < nch;
    const float rm = a.bn_mean ? rm_ : 0.f, rv = a.bn_var ? rv_ : 1.f;
    const float inv = 1.f / sqrtf(rv + kBnEps);
    const float sc = live ? w_ * inv : 0.f;
    const float sh = live ? b_ - rm * sc : 0.f;
    if (i < kBnTab) {
      bsc[i] = sc;
      bsh[i] = sh;
    }
  }
  for (int i = threadIdx.x; i < kGuard + 3 * FPLANE; i += kConvThreads) lds[i] = 0.f;
  __syncthreads();
  FDR_STAMP(a, 1);

  // ---- frame (policies/impala.py:147: frame / 255) -> BN2d(3) -> padded [3][66][66] ----
  if (a.frames) {
    const float* fr = a.frames + (a.shared_frames ? (int64_t)e : env) * kFramePix;
    for (int p = threadIdx.x; p < kFramePix; p += kConvThreads) {
      const int ch = p >> 12, y = (p >> 6) & 63, x = p & 63;
      T[ch * FPLANE + (y + 1) * FW + x + 1] = fmaf(fr[p] / 255.0f, bsc[ch], bsh[ch]);
    }
  } else {
    const uint64_t gid = (uint64_t)(a.lane_offset * a.envs + env);
    for (int w = threadIdx.x; w < kFramePix / 8; w += kConvThreads) {
      const uint64_t ctr = (gid << 32) | ((uint64_t)a.t << 11) | (uint64_t)w;
      const uint64_t hb = mix64(a.fkey + ctr * kGolden);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int p = 8 * w + j, ch = p >> 12, y = (p >> 6) & 63, x = p & 63;
        const float v = (float)((uint32_t)(hb >> (8 * j)) & 255u);
        T[ch * FPLANE + (y + 1) * FW + x + 1] = fmaf(v / 255.0f, bsc[ch], bsh[ch]);
      }
    }
  }
  __syncthreads();
  FDR_STAMP(a, 2);

  // ---- stage 1: conv 3->16 @64x64, pool -> X1 [16][32][32], residual blocks ----
  stage_entry<3, 16, 64, FPLANE, kBand>(T, T + 3 * FPLANE, X, bf3, pk + L.conv_b[0], wave, ln, a, 40);
  {
    float bf[36];
    load_frag<16, 1>(pk + L.conv_w[1], bf, wave, ln);
    to_padded<16, 32, true, true>(X, T, bsc + 1 * 32, bsh + 1 * 32);
    __syncthreads();
    FDR_STAMP(a, 3);
    res_blocks<16, 32, 0>(T, X, bf, pk, L, 0, bsc, bsh, wave, ln, a, 4, nullptr);  // ends with T = BN5(X1)
  }
  // ---- stage 2: conv 16->32 @32x32 (S2 after T, over the dead X1), pool -> X2 [32][16][16] ----
  float* X2 = T + 16 * Plane<32>::P + kSkewPad + 32 * kBand * 33;
  {
    float bf[36];
    load_frag<16, 2>(pk + L.conv_w[5], bf, wave, ln);
    FDR_STAMP(a, 12);
    stage_entry<16, 32, 32, Plane<32>::P, kBand>(T, T + 16 * Plane<32>::P + kSkewPad, X2, bf, pk + L.conv_b[5], wave, ln, a, 48);
  }
  {
    float bf[72];
    load_frag<32, 2>(pk + L.conv_w[6], bf, wave, ln);
    to_padded<32, 16, true, true>(X2, T, bsc + 6 * 32, bsh + 6 * 32);
    __syncthreads();
    FDR_STAMP(a, 13);
    res_blocks<32, 16, 0>(T, X2, bf, pk, L, 1, bsc, bsh, wave, ln, a, 14, nullptr);  // ends with T = BN10(X2)
  }
  // ---- stage 3: conv 32->32 @16x16 in one 17-row band, pool -> X3 [32][8][8] ----
  float* X3 = T + 32 * Plane<16>::P + kSkewPad + 32 * 17 * 17;
  {
    float bf[72];
    load_frag<32, 2>(pk + L.conv_w[10], bf, wave, ln);
    FDR_STAMP(a, 22);
    stage_entry<32, 32, 16, Plane<16>::P, 17>(T, T + 32 * Plane<16>::P + kSkewPad, X3, bf, pk + L.conv_b[10], wave, ln, a, 56);
  }
  {
    float bf[72];
    load_frag<32, 2>(pk + L.conv_w[11], bf, wave, ln);
    to_padded<32, 8, true, true>(X3, T, bsc + 11 * 32, bsh + 11 * 32);
    __syncthreads();
    FDR_STAMP(a, 23);
    // ---- relu + flatten (C, H, W) fused into the last epilogue (policies/impala.py:159-160) ----
    res_blocks<32, 8, 1>(T, X3, bf, pk, L, 2, bsc, bsh, wave, ln, a, 24, a.feat + env * kFeat);
  }
  FDR_STAMP(a, 32);
}

// ------------------------------------------------------------------------------------------
// core: one workgroup (256 threads) per lane, E envs.  Thread j owns fc unit j and LSTM unit j
// (gate rows j, 256+j, 512+j, 768+j), so the cell update is thread-local; weights stream from the
// pack as coalesced rows of W^T, activations are LDS broadcasts.
// The phases every core form shares (cell, BN1d fold, head, pair operands, core-input rows): fdr_impala_core.h.
// ------------------------------------------------------------------------------------------
template <int E, int MODE>
__global__ __launch_bounds__(kCoreThreads) void core_kernel(Layout L, StepArgs a) {
  // xw: the BN'd features xs [2048][E] during the fc, then the fc partial sums [4][256][E] (first
  // half), then the LSTM gate pre-activations [1024][E] (first half) -- each phase separated by a
  // barrier.  The core input, h and the logits live in xw's second half once the features are dead:
  // 32 KiB per workgroup, so 5 lanes fit a CU and 1024 lanes run in one round (at 41 KiB only 3 did).
  __shared__ float xw[kFeat * E];
  float* cis = xw + kFeat * E / 2;   // core input, [k][e]
  float* hs = cis + kCoreIn * E;     // h (then BN(h')), [k][e]
  float* logit = hs + kHid * E;      // [e][kMaxAct]
  static_assert(kFeat * E / 2 + (kCoreIn + kHid) * E + E * kMaxAct <= kFeat * E, "core LDS aliasing");
  const int lane = blockIdx.x, j = threadIdx.x;
  const float* pk = a.pack + (int64_t)lane * a.pack_stride;
  const int64_t e0 = (int64_t)lane * E;
  const int A = a.n_act;
  const int c4 = j & 63, wq = j >> 6;  // float4 column group, wave index

  if constexpr (!seq_mode(MODE)) {
    // ---- BN1d(features) -> xs ----
    for (int k = j; k < kFeat; k += kCoreThreads) {
      float sc, sh;
      bn1d_fold(L, pk, 15, k, bn1d_stats(L, a, 15, k, a.pack), sc, sh);
#pragma unroll
      for (int e = 0; e < E; ++e) xw[k * E + e] = fmaf(a.feat[(e0 + e) * kFeat + k], sc, sh);
    }
    __syncthreads();
    // ---- fc (2048 -> 256): wave wq streams rows [512 wq, 512 wq + 512) of W^T as float4 (1 KiB / wave-load) ----
    float acc[4][E];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int e = 0; e < E; ++e) acc[c][e] = 0.f;
    const float4* w4 = reinterpret_cast<const float4*>(pk + L.fc_wt) + c4;
#pragma unroll FDR_CORE_UNROLL
    for (int k = wq * (kFeat / 4); k < (wq + 1) * (kFeat / 4); ++k) {
      const float4 w = ld_stream(w4 + (int64_t)k * (kHid / 4));
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const float x = xw[k * E + e];
        acc[0][e] = fmaf(w.x, x, acc[0][e]);
        acc[1][e] = fmaf(w.y, x, acc[1][e]);
        acc[2][e] = fmaf(w.z, x, acc[2][e]);
        acc[3][e] = fmaf(w.w, x, acc[3][e]);
      }
    }
    __syncthreads();  // xs is dead
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int e = 0; e < E; ++e) xw[(wq * kHid + 4 * c4 + c) * E + e] = acc[c][e];
    __syncthreads();
    // ---- core input [relu(fc) | clip(r)] ----
    const float bj = pk[L.fc_b + j];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const float y = ((xw[j * E + e] + xw[(kHid + j) * E + e]) + xw[(2 * kHid + j) * E + e]) + xw[(3 * kHid + j) * E + e];
      cis[j * E + e] = relu(y + bj);
    }
    if (j < E) {
      const float r = MODE == kForward ? (a.reward_in ? a.reward_in[e0 + j] : 0.f) : a.rprev[e0 + j];
      cis[kHid * E + j] = fminf(fmaxf(r, -1.f), 1.f);
    }
    if (MODE == kRollout && a.ci) {
      __syncthreads();
      store_ci_rows<E>(ci_step<E>(a, e0), cis);
    }
  } else if (!a.gx) {
    load_ci_rows<E>(ci_step<E>(a, e0), cis);
  }
  float cj[E];
  load_state<E, MODE>(a, e0, j, hs, cj);
  __syncthreads();

  // ---- LSTM gates (torch order i, f, g, o): thread j streams columns 4j .. 4j+3 of [W_ih | W_hh]^T, so
  // wave wq computes gate wq; gates = (W_ih x + b_ih) + (W_hh h + b_hh) ----
  {
    float ax[4][E], ah[4][E];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int e = 0; e < E; ++e) ax[c][e] = ah[c][e] = 0.f;
    const float4* wl = reinterpret_cast<const float4*>(pk + L.lstm_wt) + j;
    if (seq_mode(MODE) && a.gx) {  // x W_ih^T precomputed by lstm_xproj_kernel (same fma chain)
      const float4* g4 = reinterpret_cast<const float4*>(a.gx + ((int64_t)(a.t - a.gx_t0) * a.n_lanes * E + e0) * kGates);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const float4 g = ld_stream(g4 + (int64_t)e * (kGates / 4) + j);
        ax[0][e] = g.x;
        ax[1][e] = g.y;
        ax[2][e] = g.z;
        ax[3][e] = g.w;
      }
    } else {
#pragma unroll FDR_CORE_UNROLL
      for (int k = 0; k < kCoreIn; ++k) {
        const float4 w = ld_stream(wl + (int64_t)k * (kGates / 4));
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const float x = cis[k * E + e];
          ax[0][e] = fmaf(w.x, x, ax[0][e]);
          ax[1][e] = fmaf(w.y, x, ax[1][e]);
          ax[2][e] = fmaf(w.z, x, ax[2][e]);
          ax[3][e] = fmaf(w.w, x, ax[3][e]);
        }
      }
    }
#pragma unroll FDR_CORE_UNROLL
    for (int k = 0; k < kHid; ++k) {
      const float4 w = ld_stream(wl + (int64_t)(kCoreIn + k) * (kGates / 4));
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const float x = hs[k * E + e];
        ah[0][e] = fmaf(w.x, x, ah[0][e]);
        ah[1][e] = fmaf(w.y, x, ah[1][e]);
        ah[2][e] = fmaf(w.z, x, ah[2][e]);
        ah[3][e] = fmaf(w.w, x, ah[3][e]);
      }
    }
    const float4 bi = reinterpret_cast<const float4*>(pk + L.lstm_bih)[j];
    const float4 bh = reinterpret_cast<const float4*>(pk + L.lstm_bhh)[j];
    const float bif[4] = {bi.x, bi.y, bi.z, bi.w}, bhf[4] = {bh.x, bh.y, bh.z, bh.w};
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int e = 0; e < E; ++e) xw[(4 * j + c) * E + e] = (ax[c][e] + bif[c]) + (ah[c][e] + bhf[c]);
  }
  __syncthreads();  // gates complete; all reads of the old h are done
  // ---- cell, BN1d(h'), head ----
  float hj[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const float pre[4] = {xw[j * E + e], xw[(kHid + j) * E + e], xw[(2 * kHid + j) * E + e], xw[(3 * kHid + j) * E + e]};
    hj[e] = lstm_cell<false>(pre, cj[e]);
    a.h[(e0 + e) * kHid + j] = hj[e];
    a.c[(e0 + e) * kHid + j] = cj[e];
  }
  {
    float sc, sh;
    bn1d_fold(L, pk, 16, j, bn1d_stats(L, a, 16, j, pk), sc, sh);
#pragma unroll
    for (int e = 0; e < E; ++e) hs[j * E + e] = fmaf(hj[e], sc, sh);
  }
  __syncthreads();
  head_rows<E, E>(pk, pk, L, A, hs, logit);
  __syncthreads();
  if (j < E) core_finish<E, MODE>(a, logit, lane, j);
}

// ------------------------------------------------------------------------------------------
// Pair form of the f32 rollout core step (fdr_impala_desc.pairs).  Lanes 2p, 2p+1 of an antithetic pair
// share their table offset: their fc / LSTM weights are fl32(theta + s_l fl32(sigma eps)).  One workgroup
// per pair streams the pair's fl32(sigma eps) pack once from HBM and theta's pack (read by every workgroup:
// L2 / MALL) and forms w = fl32(theta + s_l E) in registers -- the per-lane pack's value bit for bit (an fma
// with s = +-1 rounds theta +- E once), so every env sees core_kernel's exact fma chains; half its HBM bytes.
// The pair's 2E envs are contiguous, biases / BN / head are each lane's own pack.
// Pair operands, gate biases, cell, BN1d fold and head: fdr_impala_core.h.
// ------------------------------------------------------------------------------------------
template <int E>
__global__ __launch_bounds__(kCoreThreads) void core_kernel_p(Layout L, StepArgs a) {
  constexpr int E2 = 2 * E;
  __shared__ float xw[kFeat * E2];
  float* cis = xw + kFeat * E2 / 2;
  float* hs = cis + kCoreIn * E2;
  float* logit = hs + kHid * E2;
  static_assert(kFeat * E2 / 2 + (kCoreIn + kHid) * E2 + E2 * kMaxAct <= kFeat * E2, "core LDS aliasing");
  const int pr = blockIdx.x, j = threadIdx.x;
  const int l0 = 2 * pr;
  const float* pk0 = a.pack + (int64_t)l0 * a.pack_stride;
  const float* pk1 = pk0 + a.pack_stride;
  // branch-free sign loads (a conditional load ends its block with a full vmcnt wait)
  const int8_t* sgp = a.sign ? a.sign + l0 : reinterpret_cast<const int8_t*>(pk0);
  const int8_t sg0v = sgp[0], sg1v = sgp[1];
  const float sg0 = a.sign ? (float)sg0v : 1.f, sg1 = a.sign ? (float)sg1v : 1.f;
  const float* ep = a.ep32 + (int64_t)pr * a.ep_stride;
  const int64_t e0 = (int64_t)l0 * E;
  const int A = a.n_act;
  const int c4 = j & 63, wq = j >> 6;
  auto pkof = [&](int e) { return e < E ? pk0 : pk1; };
  const PairF32<E> P{pk0, pk1, ep, sg0, sg1};

  // the statistics once per element (branch-free, as FDR_BN1D_STATS), the fold per lane
  const bool has_m = a.bn_mean != nullptr, has_v = a.bn_var != nullptr;
  const float* bmp = has_m ? a.bn_mean + L.bn_stat[15] : pk0;
  const float* bvp = has_v ? a.bn_var + L.bn_stat[15] : pk0;
#pragma unroll
  for (int it = 0; it < kFeat / kCoreThreads; ++it) {
    const int k = j + it * kCoreThreads;
    const float rmv = bmp[k], rvv = bvp[k];
    const float rm = has_m ? rmv : 0.f, rv = has_v ? rvv : 1.f;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const float* pk = hf ? pk1 : pk0;
      float sc, sh;
      FDR_BN1D_FOLD(pk[L.bn_w[15] + k], pk[L.bn_b[15] + k], rm, rv, sc, sh)
#pragma unroll
      for (int e = 0; e < E; ++e) xw[k * E2 + hf * E + e] = fmaf(a.feat[(e0 + hf * E + e) * kFeat + k], sc, sh);
    }
  }
  __syncthreads();
  {
    float acc[4][E2];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int e = 0; e < E2; ++e) acc[c][e] = 0.f;
    const float4* t4 = reinterpret_cast<const float4*>(a.th32 + L.fc_wt) + c4;
    const float4* d4 = reinterpret_cast<const float4*>(ep + L.fc_wt) + c4;
#pragma unroll FDR_CORE_UNROLL
    for (int k = wq * (kFeat / 4); k < (wq + 1) * (kFeat / 4); ++k)
      P.accum(acc, t4[(int64_t)k * (kHid / 4)], ld_stream(d4 + (int64_t)k * (kHid / 4)), xw + k * E2);
    __syncthreads();  // xs is dead
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int e = 0; e < E2; ++e) xw[(wq * kHid + 4 * c4 + c) * E2 + e] = acc[c][e];
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < E2; ++e) {
    const float y = ((xw[j * E2 + e] + xw[(kHid + j) * E2 + e]) + xw[(2 * kHid + j) * E2 + e]) +
                    xw[(3 * kHid + j) * E2 + e];
    cis[j * E2 + e] = relu(y + pkof(e)[L.fc_b + j]);
  }
  if (j < E2) cis[kHid * E2 + j] = fminf(fmaxf(a.rprev[e0 + j], -1.f), 1.f);
  if (a.ci) {
    __syncthreads();
    float* dst = a.ci + ((int64_t)a.t * a.n_lanes * E + e0) * kCoreIn;
    for (int i = j; i < kCoreIn * E2; i += kCoreThreads) {
      const int e = i / kCoreIn, k = i - e * kCoreIn;
      dst[i] = cis[k * E2 + e];
    }
  }
  float cj[E2];
#pragma unroll
  for (int e = 0; e < E2; ++e) {
    hs[j * E2 + e] = a.h[(e0 + e) * kHid + j];
    cj[e] = a.c[(e0 + e) * kHid + j];
  }
  __syncthreads();
  {
    float ax[4][E2], ah[4][E2];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int e = 0; e < E2; ++e) ax[c][e] = ah[c][e] = 0.f;
    const float4* tl = reinterpret_cast<const float4*>(a.th32 + L.lstm_wt) + j;
    const float4* dl = reinterpret_cast<const float4*>(ep + L.lstm_wt) + j;
#pragma unroll FDR_CORE_UNROLL
    for (int k = 0; k < kCoreIn; ++k)
      P.accum(ax, tl[(int64_t)k * (kGates / 4)], ld_stream(dl + (int64_t)k * (kGates / 4)), cis + k * E2);
#pragma unroll FDR_CORE_UNROLL
    for (int k = 0; k < kHid; ++k)
      P.accum(ah, tl[(int64_t)(kCoreIn + k) * (kGates / 4)], ld_stream(dl + (int64_t)(kCoreIn + k) * (kGates / 4)),
            hs + k * E2);
    const auto gb = P.gate_bias(L, j);
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int e = 0; e < E2; ++e) xw[(4 * j + c) * E2 + e] = P.gate_pre(gb, c, e, ax[c][e], ah[c][e]);
  }
  __syncthreads();
  float hj[E2];
#pragma unroll
  for (int e = 0; e < E2; ++e) {
    FDR_LSTM_CELL(sigm, tanhf, xw[j * E2 + e], xw[(kHid + j) * E2 + e], xw[(2 * kHid + j) * E2 + e],
                  xw[(3 * kHid + j) * E2 + e], cj[e], hj[e])
    a.h[(e0 + e) * kHid + j] = hj[e];
    a.c[(e0 + e) * kHid + j] = cj[e];
  }
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) {
    const float* pk = hf ? pk1 : pk0;
    FDR_BN1D_STATS(16, j, pk, rm, rv)
    float sc, sh;
    FDR_BN1D_FOLD(pk[L.bn_w[16] + j], pk[L.bn_b[16] + j], rm, rv, sc, sh)
#pragma unroll
    for (int e = 0; e < E; ++e) hs[j * E2 + hf * E + e] = fmaf(hj[hf * E + e], sc, sh);
  }
  __syncthreads();
  head_rows<E, E2>(pk0, pk1, L, A, hs, logit);
  __syncthreads();
  if (j < E2) core_finish<E, kRollout>(a, logit + (j >= E ? E * kMaxAct : 0), l0 + (j >= E ? 1 : 0), j % E);
}
// Replay (entropy pass) in the pair form: the x W_ih^T half of the gates comes precomputed per env
// (lstm_xproj_kernel, a.gx), the W_hh h half streams theta + s_l fl32(sigma eps) for the pair -- the same
// values and fma chains as core_kernel<E, kReplay> (bit-identical), half its W_hh bytes.
template <int E>
__global__ __launch_bounds__(kCoreThreads) void core_kernel_pr(Layout L, StepArgs a) {
  constexpr int E2 = 2 * E;
  __shared__ float xw[kGates * E2 + kHid * E2 + E2 * kMaxAct];
  float* hs = xw + kGates * E2;
  float* logit = hs + kHid * E2;
  const int pr = blockIdx.x, j = threadIdx.x;
  const int l0 = 2 * pr;
  const float* pk0 = a.pack + (int64_t)l0 * a.pack_stride;
  const float* pk1 = pk0 + a.pack_stride;
  const float sg0 = a.sign ? (float)a.sign[l0] : 1.f, sg1 = a.sign ? (float)a.sign[l0 + 1] : 1.f;
  const float* ep = a.ep32 + (int64_t)pr * a.ep_stride;
  const PairF32<E> P{pk0, pk1, ep, sg0, sg1};
  const int64_t e0 = (int64_t)l0 * E;
  const int A = a.n_act;
  float cj[E2];
#pragma unroll
  for (int e = 0; e < E2; ++e) {
    hs[j * E2 + e] = a.h[(e0 + e) * kHid + j];
    cj[e] = a.c[(e0 + e) * kHid + j];
  }
  __syncthreads();
  {
    float ah[4][E2];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int e = 0; e < E2; ++e) ah[c][e] = 0.f;
    const float4* tl = reinterpret_cast<const float4*>(a.th32 + L.lstm_wt) + j;
    const float4* dl = reinterpret_cast<const float4*>(ep + L.lstm_wt) + j;
#pragma unroll FDR_CORE_UNROLL
    for (int k = 0; k < kHid; ++k) {
      const float4 t = tl[(int64_t)(kCoreIn + k) * (kGates / 4)];
      const float4 d = ld_stream(dl + (int64_t)(kCoreIn + k) * (kGates / 4));
      P.accum(ah, t, d, hs + k * E2);
    }
    const float4* g4 = reinterpret_cast<const float4*>(a.gx + ((int64_t)(a.t - a.gx_t0) * a.n_lanes * E + e0) * kGates);
    const auto gb = P.gate_bias(L, j);
#pragma unroll
    for (int e = 0; e < E2; ++e) {
      const float4 g = ld_stream(g4 + (int64_t)e * (kGates / 4) + j);
      const float gxv[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) xw[(4 * j + c) * E2 + e] = P.gate_pre(gb, c, e, gxv[c], ah[c][e]);
    }
  }
  __syncthreads();
  float hj[E2];
#pragma unroll
  for (int e = 0; e < E2; ++e) {
    FDR_LSTM_CELL(sigm, tanhf, xw[j * E2 + e], xw[(kHid + j) * E2 + e], xw[(2 * kHid + j) * E2 + e],
                  xw[(3 * kHid + j) * E2 + e], cj[e], hj[e])
    a.h[(e0 + e) * kHid + j] = hj[e];
    a.c[(e0 + e) * kHid + j] = cj[e];
  }
  __syncthreads();  // every read of hs is done before BN(h') overwrites it
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) {
    const float* pk = hf ? pk1 : pk0;
    FDR_BN1D_STATS(16, j, pk, rm, rv)
    float sc, sh;
    FDR_BN1D_FOLD(pk[L.bn_w[16] + j], pk[L.bn_b[16] + j], rm, rv, sc, sh)
#pragma unroll
    for (int e = 0; e < E; ++e) hs[j * E2 + hf * E + e] = fmaf(hj[hf * E + e], sc, sh);
  }
  __syncthreads();
  head_rows<E, E2>(pk0, pk1, L, A, hs, logit);
  __syncthreads();
  if (j < E2) core_finish<E, kReplay>(a, logit + (j >= E ? E * kMaxAct : 0), l0 + (j >= E ? 1 : 0), j % E);
}
template __global__ void core_kernel_pr<1>(Layout, StepArgs);
template __global__ void core_kernel_pr<2>(Layout, StepArgs);
template __global__ void core_kernel_pr<4>(Layout, StepArgs);

template __global__ void core_kernel_p<1>(Layout, StepArgs);
template __global__ void core_kernel_p<2>(Layout, StepArgs);
template __global__ void core_kernel_p<4>(Layout, StepArgs);

// ------------------------------------------------------------------------------------------
// Entropy replay, input projection.  The reference's get_entropy runs the stored core inputs through
// the LSTM as ONE sequence (policies/impala.py:21-22, 166-182); the x W_ih^T half of every step's gates
// does not depend on h, so -- as torch's LSTM does -- it is one GEMM per lane over a chunk of steps:
// G[(t, e)][n] = sum_k x_(t,e)[k] W_ih^T[k][n] on v_mfma_f32_16x16x4_f32.  An f32 MFMA is a k-ordered
// fma chain, so G is bit-identical to the k-loop the replay kernel ran, while W_ih is read once per
// 64 rows instead of once per step (the replay then streams W_hh only).  fp16 mode reads the f16
// W_ih^T (exact in f32), as its replay did.
// Workgroup: 64 rows x 256 gate columns, 4 waves x (4 x 4) 16x16 tiles; K in LDS chunks of 32.
// ------------------------------------------------------------------------------------------
template <bool HALF>
__global__ __launch_bounds__(256) void lstm_xproj_kernel(Layout L, StepArgs a, int t0, int tc, float* __restrict__ gx) {
  constexpr int KC = 32, NKC = (kCoreIn + KC - 1) / KC, XP = 80, WP = 256 + 16;  // pads: conflict-free reads
  __shared__ float xs[KC * XP];  // [k][row]
  __shared__ float ws[KC * WP];  // [k][col]
  const int lane = blockIdx.x, E = a.envs, rows = tc * E;
  const int row0 = blockIdx.y * 64, n0 = blockIdx.z * 256;
  const int tid = threadIdx.x, wave = tid >> 6, ln = tid & 63, g = ln >> 4, r = ln & 15;
  const int64_t ne = (int64_t)a.n_lanes * E;
  f32x4 acc[4][4];
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kc = 0; kc < NKC; ++kc) {
    const int k0 = kc * KC;
#pragma unroll
    for (int m = 0; m < 8; ++m) {  // X tile: row-contiguous global reads (32 k of one row per half-wave)
      const int i = tid + 256 * m, row = i >> 5, k = i & 31;
      const int q = row0 + row;
      float v = 0.f;
      if (q < rows && k0 + k < kCoreIn) {
        const int64_t t = t0 + q / E, e = q % E;
        v = a.ci[((t * a.n_lanes + lane) * E + e) * kCoreIn + k0 + k];
      }
      xs[k * XP + row] = v;
    }
#pragma unroll
    for (int m = 0; m < 8; ++m) {  // W_ih^T tile [32 k][256 cols]
      const int i = tid + 256 * m, k = i >> 6, c4 = i & 63;
      float4 w = float4{0.f, 0.f, 0.f, 0.f};
      if (k0 + k < kCoreIn) {
        if constexpr (HALF) {
          typedef _Float16 h4v __attribute__((ext_vector_type(4)));
          const h4v hv = *reinterpret_cast<const h4v*>(a.hpack + (int64_t)lane * a.hpack_stride + L.lstm_wt_h +
                                                        (int64_t)(k0 + k) * kGates + n0 + 4 * c4);
          w = float4{(float)hv[0], (float)hv[1], (float)hv[2], (float)hv[3]};
        } else {
          w = *reinterpret_cast<const float4*>(a.pack + (int64_t)lane * a.pack_stride + L.lstm_wt +
                                               (int64_t)(k0 + k) * kGates + n0 + 4 * c4);
        }
      }
      *reinterpret_cast<float4*>(ws + k * WP + 4 * c4) = w;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < KC / 4; ++s) {
      const int k = 4 * s + g;
      float av[4], bv[4];
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) av[ti] = xs[k * XP + 16 * ti + r];
#pragma unroll
      for (int tj = 0; tj < 4; ++tj) bv[tj] = ws[k * WP + 64 * wave + 16 * tj + r];
#pragma unroll
      for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ti], bv[tj], acc[ti][tj], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int q = row0 + 16 * ti + 4 * g + v;
      if (q >= rows) continue;
      float* dst = gx + ((int64_t)(q / E) * ne + (int64_t)lane * E + q % E) * kGates + n0 + 64 * wave + r;
#pragma unroll
      for (int tj = 0; tj < 4; ++tj) dst[16 * tj] = acc[ti][tj][v];
    }
}

// ci[z][lane][0:256] = relu(BN1d(feat_(lane, z)) W_fc^T + b_fc), ci[z][lane][256] = clamp(reward_z, -1, 1)
// (policies/impala.py:161-164) on v_mfma_f32_16x16x4_f32: 64 rows x 256 columns per workgroup, K = 2048
// in LDS chunks of 32 with the eval-mode BN folded into the X-tile load.  fp16 mode reads the f16 W^T.
template <bool HALF>
__global__ __launch_bounds__(256) void fc_rows_kernel(Layout L, StepArgs a, int z0, int zc) {
  constexpr int KC = 32, XP = 80, WP = 256 + 16;
  __shared__ float xs[KC * XP];  // [k][row]
  __shared__ float ws[KC * WP];  // [k][col]
  const int lane = blockIdx.x, row0 = blockIdx.y * 64;
  const int tid = threadIdx.x, wave = tid >> 6, ln = tid & 63, g = ln >> 4, r = ln & 15;
  const float* pk = a.pack + (int64_t)lane * a.pack_stride;
  f32x4 acc[4][4];
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < kFeat; k0 += KC) {
    const int kk = k0 + (tid & 31);  // every X element this thread loads has this k
    float sc, sh;
    bn1d_fold(L, pk, 15, kk, bn1d_stats(L, a, 15, kk, a.pack), sc, sh);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int i = tid + 256 * m, row = i >> 5, q = row0 + row;
      xs[(i & 31) * XP + row] = q < zc ? fmaf(a.feat[((int64_t)lane * zc + q) * kFeat + kk], sc, sh) : 0.f;
    }
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int i = tid + 256 * m, k = i >> 6, c4 = i & 63;
      float4 w;
      if constexpr (HALF) {
        typedef _Float16 h4v __attribute__((ext_vector_type(4)));
        const h4v hv = *reinterpret_cast<const h4v*>(a.hpack + (int64_t)lane * a.hpack_stride + L.fc_wt_h +
                                                      (int64_t)(k0 + k) * kHid + 4 * c4);
        w = float4{(float)hv[0], (float)hv[1], (float)hv[2], (float)hv[3]};
      } else {
        w = *reinterpret_cast<const float4*>(pk + L.fc_wt + (int64_t)(k0 + k) * kHid + 4 * c4);
      }
      *reinterpret_cast<float4*>(ws + k * WP + 4 * c4) = w;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < KC / 4; ++s) {
      const int k = 4 * s + g;
      float av[4], bv[4];
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) av[ti] = xs[k * XP + 16 * ti + r];
#pragma unroll
      for (int tj = 0; tj < 4; ++tj) bv[tj] = ws[k * WP + 64 * wave + 16 * tj + r];
#pragma unroll
      for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ti], bv[tj], acc[ti][tj], 0, 0, 0);
    }
    __syncthreads();
  }
  float bias[4];
#pragma unroll
  for (int tj = 0; tj < 4; ++tj) bias[tj] = pk[L.fc_b + 64 * wave + 16 * tj + r];
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int q = row0 + 16 * ti + 4 * g + v;
      if (q >= zc) continue;
      float* dst = a.ci + ((int64_t)(z0 + q) * a.n_lanes + lane) * kCoreIn + 64 * wave + r;
#pragma unroll
      for (int tj = 0; tj < 4; ++tj) dst[16 * tj] = relu(acc[ti][tj][v] + bias[tj]);
    }
  if (blockIdx.y == 0 && tid < zc) {
    const float rw = a.reward_in ? a.reward_in[z0 + tid] : 0.f;
    a.ci[((int64_t)(z0 + tid) * a.n_lanes + lane) * kCoreIn + kHid] = fminf(fmaxf(rw, -1.f), 1.f);
  }
}

// the instances the launchers use (fdr_impala.hip)
template __global__ void core_kernel<1, kRollout>(Layout, StepArgs);
template __global__ void core_kernel<1, kReplay>(Layout, StepArgs);
template __global__ void core_kernel<2, kRollout>(Layout, StepArgs);
template __global__ void core_kernel<2, kReplay>(Layout, StepArgs);
template __global__ void core_kernel<4, kRollout>(Layout, StepArgs);
template __global__ void core_kernel<4, kReplay>(Layout, StepArgs);
template __global__ void core_kernel<8, kRollout>(Layout, StepArgs);
template __global__ void core_kernel<8, kReplay>(Layout, StepArgs);
template __global__ void core_kernel<1, kForward>(Layout, StepArgs);
template __global__ void core_kernel<1, kStrategy>(Layout, StepArgs);
template __global__ void lstm_xproj_kernel<false>(Layout, StepArgs, int, int, float*);
template __global__ void lstm_xproj_kernel<true>(Layout, StepArgs, int, int, float*);
template __global__ void fc_rows_kernel<false>(Layout, StepArgs, int, int);
template __global__ void fc_rows_kernel<true>(Layout, StepArgs, int, int);

}  // namespace impala
}  // namespace fdr
