// fdr_noise_fill.hip -- counter-based noise rows (fdr_noise_fill): one kernel, its launcher and its C entry.
//
// Row r of `out` is the standard-normal vector of direction id d_r under the source's seed s, a pure function of
// (s, d_r, element): any rank, or the learner an epoch later, regenerates any direction alone.  Element quad j of a
// row (elements 4j .. 4j+3) is one Philox4x32-10 block (Salmon, Moraes, Dror & Shaw, SC'11; Random123's constants)
//   counter = (j, d & 0xffffffff, d >> 32, 0)      key = (s & 0xffffffff, s >> 32)
// whose words x0..x3 give four normals by two Box-Muller pairs (x0, x1) and (x2, x3); for a pair (a, b)
//   u1 = ((a >> 8) + 1) 2^-24 in (0, 1]     u2 = (b >> 8) 2^-24 in [0, 1)          (both exact in f32)
//   r = sqrtf(-2 logf(u1))                  (z0, z1) = (r cospif(2 u2), r sinpif(2 u2))
// The pi-scaled sine / cosine take the exact argument 2 u2 (forming 2 pi u2 in f32 first costs tens of ulp of the
// result); no fast-math intrinsic, and -2 logf(u1) is one exact scaling, so nothing here can be contracted.
// tests/philox_ref.py restates all of it in numpy.
//
// Layout: row r starts at r * row_stride; every quad of the stride is generated and written -- the elements between
// n_params and row_stride continue the row's stream (quad j of the row, whatever n_params is), so a row's first
// n_params values do not depend on row_stride and every thread's store is one aligned 16-byte vector.
// One thread per quad over the flat quad index n_rows * row_stride / 4 (int64), grid-stride: rows are not a grid
// dimension, so any n_rows runs.  20 32x32->64 multiplies per quad; write-bandwidth-bound at large n_params.
#include <algorithm>

#include "fdr_internal.h"

namespace fdr {
namespace {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;
constexpr int kFillBlock = 256;

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t (&x)[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(kPhiloxM0, c0), lo0 = kPhiloxM0 * c0;
    const uint32_t hi1 = __umulhi(kPhiloxM1, c2), lo1 = kPhiloxM1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  x[0] = c0;
  x[1] = c1;
  x[2] = c2;
  x[3] = c3;
}

__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float* z0, float* z1) {
  const float u1 = (float)((a >> 8) + 1u) * 0x1p-24f;
  const float u2 = (float)(b >> 8) * 0x1p-24f;
  const float r = sqrtf(-2.0f * logf(u1));
  float s, c;
  sincospif(2.0f * u2, &s, &c);
  *z0 = r * c;
  *z1 = r * s;
}

// step_rows / step_quads: the grid's stride (threads) as whole rows + quads, so the loop carries (row, quad)
// without a division per iteration
__global__ void __launch_bounds__(kFillBlock)
noise_fill_kernel(uint32_t k0, uint32_t k1, const uint64_t* __restrict__ ids, uint64_t first_id, int64_t n_rows,
                  uint32_t quads_per_row, int64_t step_rows, uint32_t step_quads, float* __restrict__ out) {
  const uint64_t q0 = (uint64_t)blockIdx.x * kFillBlock + threadIdx.x;
  int64_t row = (int64_t)(q0 / quads_per_row);
  uint32_t j = (uint32_t)(q0 % quads_per_row);
  while (row < n_rows) {
    const uint64_t d = ids ? ids[row] : first_id + (uint64_t)row;
    uint32_t x[4];
    philox4x32_10(j, (uint32_t)d, (uint32_t)(d >> 32), 0u, k0, k1, x);
    float4 z;
    box_muller(x[0], x[1], &z.x, &z.y);
    box_muller(x[2], x[3], &z.z, &z.w);
    *reinterpret_cast<float4*>(out + (row * (int64_t)quads_per_row + j) * 4) = z;
    row += step_rows;
    // j + step_quads < 2 quads_per_row <= 2^32 holds: quads_per_row <= 2^31 is checked at the entry
    j += step_quads;
    if (j >= quads_per_row) {
      j -= quads_per_row;
      ++row;
    }
  }
}

}  // namespace

int launch_noise_fill(const Context& ctx, uint64_t seed, const uint64_t* ids, uint64_t first_id, int64_t n_rows,
                      int64_t row_stride, float* out, hipStream_t stream) {
  const int64_t qpr = row_stride / 4;
  const int64_t total = n_rows * qpr;
  // memory-bound grid: enough blocks to fill the chip, the rest by the grid stride
  const int64_t cap = (int64_t)context_cus(ctx) * 8;
  const int64_t blocks = std::min<int64_t>((total + kFillBlock - 1) / kFillBlock, cap);
  const int64_t step = blocks * kFillBlock;
  hipLaunchKernelGGL(noise_fill_kernel, dim3((unsigned)blocks), dim3(kFillBlock), 0, stream, (uint32_t)seed,
                     (uint32_t)(seed >> 32), ids, first_id, n_rows, (uint32_t)qpr, step / qpr, (uint32_t)(step % qpr),
                     out);
  return check_launch("noise_fill_kernel");
}

}  // namespace fdr

extern "C" int fdr_noise_fill(fdr_ctx* ctx, uint64_t seed, const uint64_t* ids, uint64_t first_id, int64_t n_rows,
                              int32_t n_params, int64_t row_stride, float* out, fdr_stream stream) {
  using namespace fdr;
  Context* C = nullptr;
  const int rc = resolve_context(ctx, &C);
  if (rc) return rc;
  if (!out) return set_error(FDR_ERR_INVALID, "out is NULL");
  if (((uintptr_t)out & 15) != 0) return set_error(FDR_ERR_INVALID, "out must be 16-byte aligned");
  if (n_rows < 0) return set_error(FDR_ERR_INVALID, "n_rows < 0");
  if (n_params < 1) return set_error(FDR_ERR_INVALID, "n_params < 1");
  if (row_stride % 4 != 0 || row_stride < ((int64_t)n_params + 3) / 4 * 4)
    return set_error(FDR_ERR_INVALID, "row_stride must be a multiple of 4, at least n_params rounded up to 4");
  if (row_stride / 4 > (int64_t)1 << 31)
    return set_error(FDR_ERR_UNSUPPORTED, "row_stride above 2^33: the quad index is one 32-bit counter word");
  if (n_rows > INT64_MAX / 4 / row_stride)
    return set_error(FDR_ERR_INVALID, "n_rows * row_stride overflows an int64 byte offset");
  if (n_rows == 0) return FDR_OK;
  return launch_noise_fill(*C, seed, ids, first_id, n_rows, row_stride, out, (hipStream_t)stream);
}
