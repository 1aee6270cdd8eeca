// fdr_mlp.h -- what every MLP rollout / forward unit shares: the flat parameter layout, the compiled policy shapes
// and their host visitor (with_shape), the rollout feature bits and their compile-time walk (launch_feat_set), and
// the small device helpers of both loaders and all three rollout kernels.
//
// Declarations and templates only.  The kernels live in fdr_rollout_kernel.h (rollout_kernel), fdr_rollout_pair.hip
// (rollout_pair_kernel) and fdr_rollout.hip (the forward and the theta' read-backs); the loaders in fdr_mlp_lane.h
// and fdr_mlp_pair.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>

#include "../../include/fdr_diag.h"
#include "fdr_common.h"
#include "fdr_internal.h"
#include "fdr_wave.h"

namespace fdr {

constexpr int kLanesPerBlock = 4;

#ifdef FDR_PHASE_STAMPS
// diagnostics build only (make stamps): s_memtime cycles per step phase of wave 0 of block 0
// -- policy L1, L2, head, action, env -- summed over the episode (tools/rollout_phases.py).
// One array per rollout unit (no relocatable device code); a unit's launcher registers its reader
// (FDR_PHASE_UNIT), so fdr_debug_phase_read (fdr_rollout.hip) reads the array of the unit launched last.
[[maybe_unused]] static __device__ unsigned long long g_phase_stamps[5];
using PhaseReader = int (*)(unsigned long long* out5);
extern PhaseReader g_phase_reader;
[[maybe_unused]] static int phase_read_unit(unsigned long long* out5) {
  return hipMemcpyFromSymbol(out5, HIP_SYMBOL(g_phase_stamps), 5 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#define FDR_PHASE_UNIT() (::fdr::g_phase_reader = ::fdr::phase_read_unit)
#else
#define FDR_PHASE_UNIT() ((void)0)
#endif

__host__ __device__ constexpr int round4(int x) { return (x + 3) / 4 * 4; }

// Flat parameter layout = nn.Module.parameters() order (policies/policy.py:36-42).
template <int NIN, int NA, bool DISC>
struct Layout {
  static constexpr int H = kHidden;
  static constexpr int NOUT = DISC ? NA : 2 * NA;
  // discrete: bn0.w bn0.b l1.w l1.b bn1.w bn1.b l2.w l2.b bn2.w bn2.b l3.w l3.b
  // mujoco:   l1.w l1.b l2.w l2.b l3.w l3.b
  static constexpr int64_t BN0W = 0;
  static constexpr int64_t BN0B = NIN;
  static constexpr int64_t L1W = DISC ? 2 * NIN : 0;
  static constexpr int64_t L1B = L1W + H * NIN;
  static constexpr int64_t BN1W = L1B + H;
  static constexpr int64_t BN1B = BN1W + H;
  static constexpr int64_t L2W = DISC ? BN1B + H : L1B + H;
  static constexpr int64_t L2B = L2W + H * H;
  static constexpr int64_t BN2W = L2B + H;
  static constexpr int64_t BN2B = BN2W + H;
  static constexpr int64_t L3W = DISC ? BN2B + H : L2B + H;
  static constexpr int64_t L3B = L3W + NOUT * H;
  static constexpr int64_t P = L3B + NOUT;
  static_assert(NOUT <= 16, "policy head wider than 16 outputs not compiled");
  static_assert(NIN <= 64, "observation wider than 64 not supported");
};

// torch: two separately rounded tensor ops (utils/torch_helpers.py:25, Normal.sample).
__device__ __forceinline__ float std_from_tanh(float t) {
#pragma clang fp contract(off)
  return 0.55f + 0.45f * t;
}
__device__ __forceinline__ float gauss_action(float mean, float std, float z) {
#pragma clang fp contract(off)
  return mean + std * z;
}
// eval BatchNorm as torch CPU computes it: alpha = w * invstd, beta = b - mean * alpha
__device__ __forceinline__ void bn_fold(float w, float b, float rm, float rv, float& a, float& c) {
#pragma clang fp contract(off)
  const float invstd = 1.0f / sqrtf(rv + 1e-5f);
  a = invstd * w;
  c = b - rm * a;
}

// Categorical entropy term p_n log2 p_n of a discrete action (p_n = p / tot, torch normalises probs;
// the ln 2 scale is applied once in the epilogue).  Fast reciprocal and log2: the entropy is a reported
// statistic (parity 1e-5), not an input to the trajectory; terms below 1e-30 contribute nothing.
__device__ __forceinline__ float disc_entropy_term(float p, float tot) {
  const float pn = p * __builtin_amdgcn_rcpf(tot);
  return pn > 1e-30f ? pn * __builtin_amdgcn_logf(pn) : 0.f;
}

typedef float f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f2 pk_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
// c + a * (b.x, b.x) / c + a * (b.y, b.y): one element of a register pair broadcast by op_sel (hipcc 7.2 moves an
// odd element of a b128 load to an even register first: a v_mov per broadcast operand otherwise)
__device__ __forceinline__ f2 pk_fma_blo(f2 a, f2 b, f2 c) {
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(c) : "v"(a), "v"(b));
  return c;
}
__device__ __forceinline__ f2 pk_fma_bhi(f2 a, f2 b, f2 c) {
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(c) : "v"(a), "v"(b));
  return c;
}

// a * (b.x, b.x) / a * (b.y, b.y): the first term of an op_sel chain (no zeroed accumulator to move in)
__device__ __forceinline__ f2 pk_mul_blo(f2 a, f2 b) {
  f2 c;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(c) : "v"(a), "v"(b));
  return c;
}
__device__ __forceinline__ f2 pk_mul_bhi(f2 a, f2 b) {
  f2 c;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(c) : "v"(a), "v"(b));
  return c;
}

// broadcast read of N floats from a 16-B aligned LDS address (both loaders' cross-lane hand-offs)
template <int N>
__device__ __forceinline__ void lds_bcast(const float* v, float (&x)[N]) {  // N % 4 == 0
  const float4* v4 = reinterpret_cast<const float4*>(v);
#pragma unroll
  for (int q = 0; q < N / 4; ++q) {
    const float4 t = v4[q];
    x[4 * q] = t.x;
    x[4 * q + 1] = t.y;
    x[4 * q + 2] = t.z;
    x[4 * q + 3] = t.w;
  }
}

// ---------------------------------------------------------------------------------------------
// Compiled policy shapes and the host's one match over them
// ---------------------------------------------------------------------------------------------
template <int NIN_, int NA_, bool DISC_>
struct Shape {
  static constexpr int NIN = NIN_, NA = NA_;
  static constexpr bool DISC = DISC_;
  using L = Layout<NIN_, NA_, DISC_>;
};
template <class... S>
struct ShapeList {};
// every kernel family: forward, both loaders, rollout_kernel (synthetic env, one-lane and WIDE), rollout_pair_kernel
using MlpShapes = ShapeList<Shape<2, 9, true>, Shape<4, 2, true>, Shape<8, 4, true>, Shape<17, 6, false>,
                            Shape<11, 3, false>, Shape<8, 2, false>>;
template <class S, class... T>
constexpr bool shape_in(ShapeList<T...>) {
  return (std::is_same_v<S, T> || ...);
}
// Shapes only the physics envs use: every PhysicsSpec shape (fdr_internal.h) that MlpShapes lacks, in the table's
// order (all but CartPole's).  They get the one-lane rollout of their env, the batched forward and the lane loader's
// read-back -- no synthetic-env, pair or WIDE instance.
template <class List, int... KIND>
struct PhysicsOnly {
  using type = List;
};
template <class... T, int K, int... KIND>
struct PhysicsOnly<ShapeList<T...>, K, KIND...> {
  using S = Shape<PhysicsSpec<K>::NIN, PhysicsSpec<K>::NA, PhysicsSpec<K>::DISC>;
  using Own = ShapeList<T...>;
  using type = typename PhysicsOnly<std::conditional_t<shape_in<S>(MlpShapes{}) || shape_in<S>(Own{}), Own,
                                                       ShapeList<T..., S>>, KIND...>::type;
};
template <int... KIND>
typename PhysicsOnly<ShapeList<>, KIND...>::type physics_only_shapes(PhysicsKinds<KIND...>);
using PhysicsShapes = decltype(physics_only_shapes(PhysicsEnvKinds{}));
static_assert(Layout<3, 1, false>::P == 4546, "MujocoPolicy(3, 1) has 4546 parameters");
static_assert(Layout<6, 3, true>::P == 5071, "DiscretePolicy(6, 3) has 5071 parameters");
static_assert(Layout<2, 3, true>::P == 4807, "DiscretePolicy(2, 3) has 4807 parameters");
static_assert(Layout<2, 1, false>::P == 4482, "MujocoPolicy(2, 1) has 4482 parameters");

// Match k's (n_in, n_act, discrete) against the compiled shapes (MlpShapes, then PhysicsShapes when PHYSICS -- a
// template parameter: f is instantiated for the lists it can be called with, no more), check n_params against the
// layout once, and return f(Shape<NIN, NA, DISC>{}).  none_msg: the caller's FDR_ERR_UNSUPPORTED text when no
// shape matches.
template <class F, class... S>
int with_shape_in(ShapeList<S...>, const PolicyKey& k, bool& hit, F&& f) {
  int rc = FDR_OK;
  auto one = [&](auto s) {
    using T = decltype(s);
    if (k.n_in != T::NIN || k.n_act != T::NA || k.discrete != T::DISC) return false;
    rc = T::L::P != k.n_params ? set_error(FDR_ERR_INVALID, "n_params does not match the policy layout") : f(s);
    return true;
  };
  hit = (... || one(S{}));
  return rc;
}
template <bool PHYSICS, class F>
int with_shape(const PolicyKey& k, const char* none_msg, F&& f) {
  bool hit = false;
  int rc = with_shape_in(MlpShapes{}, k, hit, f);
  if constexpr (PHYSICS) {
    if (!hit) rc = with_shape_in(PhysicsShapes{}, k, hit, f);
  }
  return hit ? rc : set_error(FDR_ERR_UNSUPPORTED, none_msg);
}

// ---------------------------------------------------------------------------------------------
// Rollout feature bits (the FEAT template parameter of rollout_kernel / rollout_pair_kernel)
// ---------------------------------------------------------------------------------------------
constexpr int kFeatStates = 1;    // record visited observations (fdr_rollout_states)
constexpr int kFeatObsStats = 2;  // per-lane Welford obs statistics
constexpr int kFeatObsNorm = 4;   // observation normalisation (obs_mean / obs_std given)
constexpr int kFeatInject = 8;    // host-injected draws (u_inject)
constexpr int kFeatTerm = 16;     // terminating synthetic env (fdr_env_desc.done_threshold)

// The legal feature sets of each kernel family.  A family compiles every subset of its bits, except injected
// draws together with the Welford statistics (fdr_rollout_ex refuses that pair):
constexpr int kLaneFeatBits = kFeatStates | kFeatObsStats | kFeatObsNorm | kFeatInject | kFeatTerm;  // 24 sets
constexpr int kWideFeatBits = kFeatStates | kFeatObsStats | kFeatObsNorm | kFeatTerm;                // 16: no u_inject
constexpr int kPairFeatBits = kFeatStates | kFeatObsNorm | kFeatTerm;                                //  8
// physics envs: no kFeatTerm (each env's termination lives under its ENV branch)
constexpr int kPhysicsFeatBits = kFeatStates | kFeatObsStats | kFeatObsNorm | kFeatInject;           // 12
constexpr bool feat_legal(int family_bits, int f) {
  return (f & ~family_bits) == 0 && (f & (kFeatInject | kFeatObsStats)) != (kFeatInject | kFeatObsStats);
}

// The feature bits a launch asks for
inline int rollout_feat(const RolloutArgs& a, bool terminating) {
  return (a.states ? kFeatStates : 0) | (a.os_mean ? kFeatObsStats : 0) | (a.obs_mean ? kFeatObsNorm : 0) |
         (a.u_inject ? kFeatInject : 0) | (terminating ? kFeatTerm : 0);
}

// Walk the family's legal sets at compile time and call launch(std::integral_constant<int, F>{}) for the one equal
// to feat: only legal sets are instantiated.  false: feat is not one of them (nothing launched).
template <int BITS, class Launch, int... F>
bool launch_feat_set(int feat, Launch&& launch, std::integer_sequence<int, F...>) {
  auto one = [&](auto f) {
    if constexpr (feat_legal(BITS, decltype(f)::value)) {
      if (feat == decltype(f)::value) {
        launch(f);
        return true;
      }
    }
    return false;
  };
  return (one(std::integral_constant<int, F>{}) || ...);
}
template <int BITS, class Launch>
bool launch_feat_set(int feat, Launch&& launch) {
  return launch_feat_set<BITS>(feat, launch, std::make_integer_sequence<int, 2 * kFeatTerm>{});
}

}  // namespace fdr
