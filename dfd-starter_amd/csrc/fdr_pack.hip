// fdr_pack.hip -- the per-lane parameter pack shared by the pack-based policies (ImpalaPolicy, AtariPolicy, the VBN
// pass): theta'_l gathered once per call into the order the kernels read, plus the init / finish kernels of a
// rollout call.  Declarations: fdr_pack.h.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "fdr_pack.h"

namespace fdr {
namespace impala {

constexpr int kPrepThreads = 256;
constexpr int kPrepPer = 4;
constexpr int kPrepSpan = kPrepThreads * kPrepPer;

// ------------------------------------------------------------------------------------------
// prep: pack[lane][j] = theta'_lane[src(j)]  (fl32(theta + fl32(sigma * +-eps)), no contraction)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t section_src(const Section& s, int32_t u) {
  if (s.kind == kCopy) return (int64_t)s.src + u;
  if (s.kind == kTranspose) {  // pack = W^T: u = k * rows + r  ->  W[r][k]
    const int32_t k = u / s.a, r = u - k * s.a;
    return (int64_t)s.src + (int64_t)r * s.b + k;
  }
  if (s.kind == kConvFragH) {
    // f16 A-fragment (v_mfma_f32_16x16x32_f16, weights as A): u = ((kstep * NT + nt) * 64 + l) * 8 + jj,
    // A[i = nt*16 + (l & 15)][k = 8 (l >> 4) + jj].  K order per k-step of 32: Cin % 8 == 0 -> lane group
    // g = l >> 4 holds 8 consecutive channels of one tap (taps per k-step 32 / Cin); Cin = 3 (frame image
    // with 4 channel slots) -> group g holds taps 8 kstep + 2g, +1 with 4 channel slots each.
    const int32_t cin = s.a, nt_n = s.b / 16;
    const int32_t jj = u & 7, l = (u >> 3) & 63, rest = u >> 9;
    const int32_t nt = rest % nt_n, ks = rest / nt_n;
    const int32_t i = nt * 16 + (l & 15), g = l >> 4;
    int32_t tap, ci;
    if (cin == 3) {
      tap = 8 * ks + 2 * g + (jj >> 2);
      ci = jj & 3;
      if (ci >= 3) return -1;
    } else {
      const int32_t cpg = cin / 8, tpk = 32 / cin;
      tap = ks * tpk + g / cpg;
      ci = 8 * (g % cpg) + jj;
    }
    if (tap >= 9) return -1;
    return (int64_t)s.src + ((int64_t)i * cin + ci) * 9 + tap;
  }
  // conv B-fragment (v_mfma_f32_16x16x4_f32): u = (kstep * NT + nt) * 64 + l; B[k][n] with
  // k = 4 * kstep + (l >> 4), n = nt * 16 + (l & 15).  K order: Cin % 4 == 0 -> tap-major,
  // cin = 4 * (kstep % (Cin/4)) + (l >> 4); Cin = 3 -> k = tap * 3 + cin, zero-padded to 28.
  const int32_t cin = s.a & 255, cout = s.b, nt_n = cout / 16;
  const int32_t ntaps = (s.a >> 8) ? (s.a >> 8) : 9;  // AtariPolicy convs: 8x8 / 4x4 kernels
  const int32_t ks = u / (nt_n * 64), rem = u - ks * nt_n * 64;
  const int32_t nt = rem >> 6, l = rem & 63;
  const int32_t n = nt * 16 + (l & 15);
  int32_t tap, ci;
  if ((cin & 3) == 0) {
    const int32_t q = cin >> 2;
    tap = ks / q;
    ci = 4 * (ks - tap * q) + (l >> 4);
  } else {
    const int32_t k = 4 * ks + (l >> 4);
    if (k >= 9 * cin) return -1;
    tap = k / cin;
    ci = k - tap * cin;
  }
  if (tap >= ntaps) return -1;
  return (int64_t)s.src + ((int64_t)n * cin + ci) * ntaps + tap;
}

template <typename OUT>
__global__ __launch_bounds__(kPrepThreads) void prep_kernel(Layout L, LanesArgs lanes, OUT* __restrict__ pack,
                                                            double* __restrict__ n2_part, int half, int n2_slots) {
  const int lane = blockIdx.y;
  ParamSrc src = lanes.src(lane);
  const int64_t j0 = (int64_t)blockIdx.x * kPrepSpan + threadIdx.x;
  const int64_t len = half ? L.hpack : L.pack;
  const Section* sec = half ? L.hsec : L.sec;
  const int nsec = half ? L.n_hsections : L.n_sections;
  OUT* out = pack + (int64_t)lane * len;
  const bool bad = src.n2 != src.n2;  // out-of-range table offset: NaN norm, unperturbed lane
  src.n2 = 0.0;
  {  // a block entirely inside one transposed section has nothing to do (prep_transpose_kernel)
    const int64_t b0 = (int64_t)blockIdx.x * kPrepSpan, b1 = b0 + kPrepSpan - 1;
    int lo = 0, hi = nsec - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (sec[mid].dst <= b0) lo = mid; else hi = mid - 1;
    }
    if (sec[lo].kind == kTranspose && b0 >= sec[lo].dst && b1 < (int64_t)sec[lo].dst + sec[lo].len) {
      if (!half && threadIdx.x == 0) n2_part[(int64_t)lane * n2_slots + blockIdx.x] = bad ? __builtin_nan("") : 0.0;
      return;
    }
  }
#pragma unroll
  for (int i = 0; i < kPrepPer; ++i) {
    const int64_t j = j0 + (int64_t)i * kPrepThreads;
    if (j >= len) break;
    int lo = 0, hi = nsec - 1;  // last section with dst <= j
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (sec[mid].dst <= j) lo = mid; else hi = mid - 1;
    }
    const Section& s = sec[lo];
    const int32_t u = (int32_t)(j - s.dst);
    if (s.kind == kTranspose && j >= s.dst && u < s.len) continue;  // prep_transpose_kernel's part
    const int64_t p = (j >= s.dst && u < s.len) ? section_src(s, u) : -1;
    out[j] = (OUT)(p >= 0 ? (half ? src.get_nocount(p) : src.get(p)) : 0.f);
  }
  if (half) return;
  double n2 = src.n2;
  // block reduce (deterministic): wave sums, then wave 0
  __shared__ double red[kPrepThreads / kWave];
  n2 = wave_sum(n2);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n2;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < kPrepThreads / kWave; ++w) t += red[w];
    n2_part[(int64_t)lane * n2_slots + blockIdx.x] = bad ? __builtin_nan("") : t;
  }
}

// Transposed sections (fc W^T, [W_ih | W_hh]^T: 90 % of the pack) through a 64 x 64 LDS tile: theta and
// the lane's noise-table slice are read along W's rows (coalesced) and W^T is written along its rows
// (coalesced) -- the element-order gather of prep_kernel read them at a 4-8 KB stride (one 64-B
// line per 4-byte element).  Same values (fl32(theta +- fl32(sigma eps))) and the same n2 terms.
constexpr int kTT = 64;  // transpose tile edge
__host__ __device__ inline int transpose_tiles(const Section& s) { return ((s.a + kTT - 1) / kTT) * ((s.b + kTT - 1) / kTT); }

// write = 0: the f32 call's n2 partials only (the same reads and reduce order, no tile, no stores) -- for fp16 calls,
// whose kernels take these weights from the half pack / the pair images
template <class OUT>
__global__ __launch_bounds__(256) void prep_transpose_kernel(Layout L, LanesArgs lanes, OUT* __restrict__ pack,
                                                             double* __restrict__ n2_part, int half, int n2_slot0,
                                                             int n2_slots, int write) {
  __shared__ float tile[kTT][kTT + 1];
  __shared__ double red[256 / kWave];
  const int lane = blockIdx.y;
  ParamSrc src = lanes.src(lane);
  const bool bad = src.n2 != src.n2;
  src.n2 = 0.0;
  const Section* sec = half ? L.hsec : L.sec;
  const int nsec = half ? L.n_hsections : L.n_sections;
  int t = blockIdx.x, si = 0;
  for (; si < nsec; ++si) {
    if (sec[si].kind != kTranspose) continue;
    const int n = transpose_tiles(sec[si]);
    if (t < n) break;
    t -= n;
  }
  const Section s = sec[si];
  const int tr = (s.a + kTT - 1) / kTT;
  const int r0 = (t % tr) * kTT, k0 = (t / tr) * kTT;
  OUT* out = pack + (int64_t)lane * (half ? L.hpack : L.pack) + s.dst;
#pragma unroll
  for (int m = 0; m < kTT * kTT / 256; ++m) {  // W[r][k] along k
    const int e = threadIdx.x + 256 * m, i = e / kTT, jj = e % kTT, r = r0 + i, k = k0 + jj;
    float v = 0.f;
    if (r < s.a && k < s.b) {
      const int64_t p = (int64_t)s.src + (int64_t)r * s.b + k;
      v = half ? src.get_nocount(p) : src.get(p);
    }
    if (write) tile[jj][i] = v;
  }
  if (write) {
    __syncthreads();
#pragma unroll
    for (int m = 0; m < kTT * kTT / 256; ++m) {  // W^T[k][r] along r
      const int e = threadIdx.x + 256 * m, jj = e / kTT, i = e % kTT, r = r0 + i, k = k0 + jj;
      if (r < s.a && k < s.b) out[(int64_t)k * s.a + r] = (OUT)tile[jj][i];
    }
  }
  if (half) return;
  double n2 = wave_sum(src.n2);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n2;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int w = 0; w < 256 / kWave; ++w) tot += red[w];
    n2_part[(int64_t)lane * n2_slots + n2_slot0 + blockIdx.x] = bad ? __builtin_nan("") : tot;
  }
}

static int generic_prep_blocks(const Layout& L, bool half) {
  return (int)(((half ? L.hpack : L.pack) + kPrepSpan - 1) / kPrepSpan);
}
static int transpose_prep_tiles(const Layout& L, bool half) {
  const Section* sec = half ? L.hsec : L.sec;
  const int nsec = half ? L.n_hsections : L.n_sections;
  int n = 0;
  for (int i = 0; i < nsec; ++i)
    if (sec[i].kind == kTranspose) n += transpose_tiles(sec[i]);
  return n;
}

// (modes: fdr_pack.h)
template <class OUT>
void launch_pack(const Layout& L, const LanesArgs& lanes, OUT* pack, double* n2, int n_lanes, int half,
                 hipStream_t stream, TransposedMode tmode, bool copies) {
  const int g = generic_prep_blocks(L, half != 0), tt = tmode == kTrSkip ? 0 : transpose_prep_tiles(L, half != 0);
  const int slots = prep_blocks(L);
  if (copies || !half)
    hipLaunchKernelGGL(prep_kernel<OUT>, dim3(g, n_lanes), dim3(kPrepThreads), 0, stream, L, lanes, pack, n2, half,
                       slots);
  if (tt > 0)
    hipLaunchKernelGGL(prep_transpose_kernel<OUT>, dim3(tt, n_lanes), dim3(256), 0, stream, L, lanes, pack, n2, half,
                       generic_prep_blocks(L, false), slots, tmode == kTrFull ? 1 : 0);
}

__global__ void init_kernel(int64_t n_env, float* h, float* c, float* rprev, double* ret, double* ent) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (h && i < n_env * kHid) { h[i] = 0.f; c[i] = 0.f; }
  if (i < n_env) {
    if (rprev) rprev[i] = 0.f;
    ret[i] = 0.0;
    ent[i] = 0.0;
  }
}

// n2 partial slots per lane: the generic prep blocks, then the transpose tiles
int prep_blocks(const Layout& L) { return generic_prep_blocks(L, false) + transpose_prep_tiles(L, false); }

int launch_prep(const Layout& L, const LanesArgs& lanes, float* pack, double* n2_part, int n_lanes,
                hipStream_t stream) {
  launch_pack<float>(L, lanes, pack, n2_part, n_lanes, 0, stream);
  return check_launch("prep_kernel");
}

__global__ void finish_kernel(int n_lanes, int envs, int T, int entropy, int jiggle, uint64_t akey,
                              int64_t lane_offset, const double* n2_part, int nblk, double* ret,
                              double* ent, int32_t* steps, double* norm2) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (int64_t)n_lanes * envs) {
    const uint64_t gid = (uint64_t)(lane_offset * envs + i);
    if (jiggle) ret[i] += (hash_ctr(akey, gid, kJiggleT, 15) & 1ull) ? 1e-12 : -1e-12;
    if (ent) ent[i] = entropy ? ent[i] / (double)T : 0.0;
    if (steps) steps[i] = T;
  }
  if (i < n_lanes && norm2) {
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += n2_part[i * nblk + b];
    norm2[i] = s;
  }
}

template void launch_pack<float>(const Layout&, const LanesArgs&, float*, double*, int, int, hipStream_t,
                                 TransposedMode, bool);
template void launch_pack<_Float16>(const Layout&, const LanesArgs&, _Float16*, double*, int, int, hipStream_t,
                                    TransposedMode, bool);

}  // namespace impala
}  // namespace fdr
