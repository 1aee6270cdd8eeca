// Device-side declarations of the ImpalaPolicy path: what the kernel units (fdr_impala_f32.hip, fdr_impala_h.hip) and
// the host launchers (fdr_impala.hip) share.  Each declaration sits under the unit that defines it.
#pragma once
#include "fdr_impala.h"

namespace fdr {
namespace impala {

#define FDR_CORE_UNROLL 4    // weight-stream loop unroll of the core kernels (loads in flight per thread)
#define FDR_CORE_UNROLL_H 2  // fp16 step kernel's fc / gate streams (A/B: 0.377 -> 0.360 ms per step vs 4)
constexpr int kCiPitch = (kCoreIn + 31) / 32 * 32;

// phase clock of the first conv workgroup (s_memtime), for the phase breakdown in DESIGN.md -- a diagnostics build
// only (make STAMPS=1 -> -DFDR_CONV_STAMPS; tools/impala_phases_h2.py).  In the product the stamps compile away: even
// runtime-gated, each conditional store was a control-flow join at which the waitcnt pass drained every load in flight
// (vmcnt(0), CDNA4 counts stores too), including the next conv's weight-block prefetch.
#ifdef FDR_CONV_STAMPS
#define FDR_STAMP(a, k)                                                      \
  do {                                                                       \
    if ((a).dbg && blockIdx.x == 0 && threadIdx.x == 0) (a).dbg[k] = clock64(); \
  } while (0)
#else
#define FDR_STAMP(a, k) \
  do {                  \
  } while (0)
#endif

// The core kernels' shared phases (cell, BN1d fold, head, pair operands, MFMA ring): fdr_impala_core.h, device-only.

// ---- f32 kernels (fdr_impala_f32.hip) ----
constexpr int kConvThreads = 512;
// the conv stack: one workgroup (8 waves) per (lane, env), 160 KiB LDS
__global__ void conv_kernel(Layout L, StepArgs a);
template <int E, int MODE>
__global__ void core_kernel(Layout L, StepArgs a);     // per-lane form, every CoreMode
template <int E>
__global__ void core_kernel_p(Layout L, StepArgs a);   // f32 pair form (rollout mode, bit-exact), grid n_lanes / 2
template <int E>
__global__ void core_kernel_pr(Layout L, StepArgs a);  // f32 pair form of the replay (with a.gx)
// x W_ih^T of a chunk of stored core inputs (entropy replay, get_strategy): grid (n_lanes, rows / 64, kGates / 256);
// HALF: W_ih^T from the half pack
template <bool HALF>
__global__ void lstm_xproj_kernel(Layout L, StepArgs a, int t0, int tc, float* gx);
// get_strategy: the fc over a lane's zc feature rows into a.ci; grid (n_lanes, zc / 64); HALF: W^T from the half pack
template <bool HALF>
__global__ void fc_rows_kernel(Layout L, StepArgs a, int z0, int zc);

// ---- fp16 mode kernels (fdr_impala_h.hip) ----
// the fp16 conv stack's folded BN / bias tables of n lanes (one workgroup per lane): tab [lane][3 * kBnTab]
__global__ void bn_table_kernel(Layout L, StepArgs a, float* tab);
// the conv stack: one env per 8-wave workgroup (kHThreads), 80 KiB LDS, <= 128 VGPRs -- two workgroups per CU
template <int NTH>
__global__ void conv_kernel_h2(Layout L, StepArgs a);
template <int E, int MODE>
__global__ void core_kernel_h(Layout L, StepArgs a);   // per-lane form (non-pair batches, forward)
// fp16 pair form on MFMA: theta x + s (E x) over fragment images, two antithetic pairs per workgroup (512 threads),
// grid n_lanes / 4 (n_lanes % 4 == 0)
template <int E, int MODE>
__global__ void core_kernel_hpm2(Layout L, StepArgs a);
// replay input projection of a chunk in the fp16 pair form on MFMA: grid xproj_grid(n_lanes) (XCD-aware, 1-D);
// H16: the core inputs from a.ci16 (the rollout), else from the f32 rows a.ci (lane strategies)
template <int E, bool H16>
__global__ void xproj_pair_kernel(Layout L, StepArgs a, int t0, int tc, float* gx);
inline dim3 xproj_grid(int n_lanes) { return dim3((unsigned)(((n_lanes / 2 + 7) / 8) * 8 * (kGateNT / 4))); }
// the entropy replay of one chunk (steps t0 .. t0 + tc - 1 on a.gx) in ONE launch: the W_hh step of the pair form
// for two pairs per workgroup in a loop, h / c / ent in registers, the next step's first W_hh fragments in flight
// under each epilogue
template <int E, int MODE>  // kReplay (entropy sums) or kStrategy (probabilities over a probe sequence)
__global__ void replay_chunk_hpm2(Layout L, StepArgs a, int t0, int tc);
// MFMA images (kMImg halves each) of n half packs: grid (kFcKS + 4 kGateKS, n)
__global__ void mfma_image_kernel(Layout L, const _Float16* src, int64_t src_stride, _Float16* dst);
constexpr int kHThreads = 512;

}  // namespace impala
}  // namespace fdr
