// Probe: issue cost per wave-instruction per SIMD of every instruction kind in rollout_pair_kernel's loop
// (DESIGN.md 3.0 ceiling table), at 1 / 2 / 4 waves per SIMD.  Each mode issues 64 independent instructions
// per iteration (8 rotating accumulators, operands in distinct registers), timed by HIP events over the
// whole grid (256 CUs x 4 SIMDs x W waves).  ns per instruction per SIMD; cycles at the clock given on the
// command line (the rollout's loaded clock from its PMC, GRBM_GUI_ACTIVE / 8 / duration).
//   hipcc --offload-arch=gfx950 -O3 tools/probes/mix_probe.hip -o tools/probes/mix_probe && ./mix_probe 2.13
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#define REP8(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)

template <int MODE>
__global__ __launch_bounds__(256) void k(float* out, int iters) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  __shared__ float4 lds[64];
  f2 a[8], w[8];
  float b[8];
  for (int i = 0; i < 8; ++i) {
    a[i] = f2{out[i] * 1e-3f, out[i + 8]};
    w[i] = f2{threadIdx.x * 1e-3f + i, 1.f + i};
    b[i] = out[i + 16] + 0.5f;
  }
  if (threadIdx.x < 64) lds[threadIdx.x] = float4{1.f, 2.f, 3.f, 4.f};
  __syncthreads();
  f2 x = f2{threadIdx.x * 1e-4f, 0.5f};
  float4 acc4 = float4{0.f, 0.f, 0.f, 0.f};
  [[maybe_unused]] const unsigned long long mask = 0x5555555555555555ull * (unsigned)iters;  // wave-uniform: an SGPR pair
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
#define PK(i) asm volatile("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(a[i]) : "v"(w[i]), "v"(x));
#define FMA(i) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(a[i].x) : "v"(w[i].y), "v"(b[i]));
#define ADD(i) asm volatile("v_add_f32 %0, %1, %0" : "+v"(a[i].x) : "v"(w[i].y));
#define MOV(i) asm volatile("v_mov_b32 %0, %1" : "=v"(a[i].x) : "v"(w[i].y));
#define FMACDPP(i) asm volatile("v_fmac_f32_dpp %0, %1, %2 row_newbcast:3 row_mask:0xf bank_mask:0xf" : "+v"(a[i].x) : "v"(w[i].y), "v"(b[i]));
#define ADDDPP(i) asm volatile("v_add_f32_dpp %0, %1, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1" : "+v"(a[i].x) : "v"(w[i].y));
#define EXP(i) asm volatile("v_exp_f32 %0, %1" : "=v"(a[i].x) : "v"(w[i].y));
#define RCP(i) asm volatile("v_rcp_f32 %0, %1" : "=v"(a[i].x) : "v"(w[i].y));
#define PKADD(i) asm volatile("v_pk_add_f32 %0, %1, %0" : "+v"(a[i]) : "v"(w[i]));
#define NOP0(i) asm volatile("s_nop 0");
#define NOP1(i) asm volatile("s_nop 1");
// The integer / 64-bit / select rows: eight instructions on eight accumulators in ONE asm statement (between asm statements
// that write one register or vcc the compiler pads with s_nop 0, which the v_mov / v_exp / v_rcp rows above carry).
// Operands: %0-%7 the accumulators, %8-%15 and %16-%23 the sources.
#define L8(F) F(0, 8, 16) F(1, 9, 17) F(2, 10, 18) F(3, 11, 19) F(4, 12, 20) F(5, 13, 21) F(6, 14, 22) F(7, 15, 23)
#define ACC32 "+v"(a[0].x), "+v"(a[1].x), "+v"(a[2].x), "+v"(a[3].x), "+v"(a[4].x), "+v"(a[5].x), "+v"(a[6].x), "+v"(a[7].x)
#define ACC64 "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7])
#define SRC_B "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]), "v"(b[4]), "v"(b[5]), "v"(b[6]), "v"(b[7])
#define SRC_WY "v"(w[0].y), "v"(w[1].y), "v"(w[2].y), "v"(w[3].y), "v"(w[4].y), "v"(w[5].y), "v"(w[6].y), "v"(w[7].y)
#define SRC_W "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(w[3]), "v"(w[4]), "v"(w[5]), "v"(w[6]), "v"(w[7])
#define MULLO_L(d, s, t) "v_mul_lo_u32 %" #d ", %" #d ", %" #s "\n\t"
#define MAD64_L(d, s, t) "v_mad_u64_u32 %" #d ", vcc, %" #s ", %" #t ", %" #d "\n\t"
#define LSHLADD64_L(d, s, t) "v_lshl_add_u64 %" #d ", %" #d ", 0, %" #s "\n\t"
#define CNDMASK_L(d, s, t) "v_cndmask_b32 %" #d ", %" #d ", %" #s ", vcc\n\t"
#define CNDMASKS_L(d, s, t) "v_cndmask_b32_e64 %" #d ", %" #d ", %" #s ", %24\n\t"
#define CVTF64_L(d, s, t) "v_cvt_f64_f32 %" #d ", %" #t "\n\t"
#define ADDF64_L(d, s, t) "v_add_f64 %" #d ", %" #d ", %" #s "\n\t"
#define MULLO8 asm volatile(L8(MULLO_L) : ACC32 : SRC_B, SRC_WY);
#define MAD648 asm volatile(L8(MAD64_L) : ACC64 : SRC_B, SRC_WY : "vcc");
#define LSHLADD648 asm volatile(L8(LSHLADD64_L) : ACC64 : SRC_W, SRC_B);
#define CNDMASK8 asm volatile(L8(CNDMASK_L) : ACC32 : SRC_B, SRC_WY);
#define CNDMASKS8 asm volatile(L8(CNDMASKS_L) : ACC32 : SRC_B, SRC_WY, "s"(mask));
#define CVTF648 asm volatile(L8(CVTF64_L) : ACC64 : SRC_W, SRC_B);
#define ADDF648 asm volatile(L8(ADDF64_L) : ACC64 : SRC_W, SRC_B);
#define DSRD(i) { float4 t; asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(8)" : "=v"(t) : "v"((unsigned)(i * 16))); acc4.x += t.x; }
      if constexpr (MODE == 0) { REP8(PK) }
      if constexpr (MODE == 1) { REP8(FMA) }
      if constexpr (MODE == 2) { REP8(ADD) }
      if constexpr (MODE == 3) { REP8(MOV) }
      if constexpr (MODE == 4) { REP8(FMACDPP) }
      if constexpr (MODE == 5) { REP8(ADDDPP) }
      if constexpr (MODE == 6) { REP8(EXP) }
      if constexpr (MODE == 7) { REP8(RCP) }
      if constexpr (MODE == 8) { REP8(PKADD) }
      if constexpr (MODE == 9) { REP8(NOP0) }
      if constexpr (MODE == 10) { REP8(NOP1) }
      if constexpr (MODE == 11) { REP8(DSRD) }
      if constexpr (MODE == 12) { MULLO8 }
      if constexpr (MODE == 13) { MAD648 }
      if constexpr (MODE == 14) { LSHLADD648 }
      if constexpr (MODE == 15) { CNDMASK8 }
      if constexpr (MODE == 18) { CNDMASKS8 }
      if constexpr (MODE == 16) { CVTF648 }
      if constexpr (MODE == 17) { ADDF648 }
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  float s = acc4.x;
  for (int i = 0; i < 8; ++i) s += a[i].x + a[i].y;
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

typedef void (*Kern)(float*, int);
int main(int argc, char** argv) {
  const double ghz = argc > 1 ? atof(argv[1]) : 2.13;
  float* d;
  hipMalloc(&d, 1 << 26);
  hipMemset(d, 0, 1 << 26);
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  const int iters = 2000;
  constexpr int kModes = 19;
  Kern ks[kModes] = {k<0>, k<1>, k<2>,  k<3>,  k<4>,  k<5>,  k<6>,  k<7>,  k<8>,
                     k<9>, k<10>, k<11>, k<12>, k<13>, k<14>, k<15>, k<16>, k<17>, k<18>};
  const char* names[kModes] = {"v_pk_fma_f32", "v_fma_f32", "v_add_f32", "v_mov_b32", "v_fmac_f32_dpp", "v_add_f32_dpp",
                               "v_exp_f32", "v_rcp_f32", "v_pk_add_f32", "s_nop 0", "s_nop 1", "ds_read_b128 (bcast)",
                               "v_mul_lo_u32", "v_mad_u64_u32", "v_lshl_add_u64", "v_cndmask_b32 (vcc)", "v_cvt_f64_f32",
                               "v_add_f64", "v_cndmask_b32 (sgpr pair)"};
  printf("%-22s %28s %28s %28s\n", "instruction", "1 wave/SIMD ns (cyc)", "2 waves/SIMD ns (cyc)", "4 waves/SIMD ns (cyc)");
  for (int mode = 0; mode < kModes; ++mode) {
    printf("%-22s", names[mode]);
    for (int wps : {1, 2, 4}) {
      const int blocks = 256 * wps;  // 256-thread blocks: 4 waves -> one per SIMD
      hipLaunchKernelGGL(ks[mode], dim3(blocks), dim3(256), 0, 0, d, iters);
      hipEventRecord(e0);
      hipLaunchKernelGGL(ks[mode], dim3(blocks), dim3(256), 0, 0, d, iters);
      hipEventRecord(e1);
      hipEventSynchronize(e1);
      float ms;
      hipEventElapsedTime(&ms, e0, e1);
      const double ns = ms * 1e6 / ((double)iters * 64 * wps);
      printf("   %12.3f (%6.2f cyc)   ", ns, ns * ghz);
    }
    printf("\n");
  }
  return 0;
}
