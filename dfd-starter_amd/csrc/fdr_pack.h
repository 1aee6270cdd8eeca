// The per-lane parameter pack and the episode bookkeeping that the pack-based policies share (ImpalaPolicy,
// AtariPolicy, the VBN pass).  Layout and StepArgs live here, in namespace fdr::impala, because AtariPolicy really
// shares them: its kernels take a Layout (the pack kernels walk its sections) and a StepArgs (core_finish reads it);
// the namespace is part of every kernel's mangled name, so it stays.
#pragma once
#include <cfloat>

#include "fdr_internal.h"

namespace fdr {
namespace impala {

constexpr int kConvs = 15;   // 3 stages x (entry conv + 2 residual blocks x 2 convs)
constexpr int kBns = 17;     // the 15 BatchNorm2d in front of them + fc BN1d + head BN1d
constexpr int kHid = 256;    // fc width == LSTM hidden (init_kernel zeroes a call's h / c; AtariPolicy has none)
constexpr int kMaxAct = 32;
constexpr int kMaxSections = 64;

// One contiguous run of the per-lane parameter pack: pack[dst + u] = theta'[src + f(u)].
enum SectionKind : int32_t { kCopy = 0, kConvFrag = 1, kTranspose = 2, kConvFragH = 3 };
struct Section {
  int32_t dst, len, src, kind, a, b;  // conv frag: a = Cin, b = Cout; transpose: a = rows, b = cols of W
};

// Per-lane parameter pack: theta' gathered ONCE per rollout into the order the kernels read
// (conv weights as MFMA B-fragments, fc / LSTM weights transposed for coalesced row streaming).
struct Layout {
  int32_t n_act;
  int32_t n_sections;
  int64_t P;     // reference parameter count (policies/impala.py)
  int64_t pack;  // floats per lane (multiple of 64)
  int32_t conv_w[kConvs], conv_b[kConvs];
  int32_t bn_w[kBns], bn_b[kBns], bn_stat[kBns];
  int32_t fc_wt, fc_b, lstm_wt, lstm_bih, lstm_bhh, head_w, head_b;
  int32_t n_bn_stats;
  Section sec[kMaxSections];
  // fp16 mode (BASELINE config 5): a second, half-precision pack of the MFMA/streamed weights
  int64_t hpack;                  // halves per lane (multiple of 64)
  int32_t conv_h[kConvs];         // f16 MFMA A-fragments of each conv (v_mfma_f32_16x16x32_f16)
  int32_t fc_wt_h, lstm_wt_h;     // W^T of fc / [W_ih | W_hh] in f16
  int32_t n_hsections;
  Section hsec[24];
};

struct StepArgs {
  const float* pack;
  int64_t pack_stride;  // floats between lanes' packs (0: every lane shares one pack)
  _Float16* hpack;      // fp16 mode: half pack (conv A-fragments, fc / LSTM W^T), or NULL
  int64_t hpack_stride;
  const float* bn_mean;
  const float* bn_var;
  int n_lanes, envs, n_act, t, T;
  int64_t lane_offset;
  uint64_t fkey, rkey, akey;
  const float* frames;     // external frames [lane*E+e][3][64][64] (forward API) or NULL
  int shared_frames;       // 1: every lane reads frames [e][3][64][64] (strategy probe set zeta)
  float* feat;             // [lane*E+e][2048]
  // core
  float* h;
  float* c;
  float* rprev;
  float* ci;               // [t][lane*E+e][257] (entropy replay) or NULL
  const float* gx;         // replay: x W_ih^T of steps [gx_t0, gx_t0 + kReplayChunk), [t - gx_t0][lane*E+e][1024], or NULL
  int gx_t0;
  double* ret;
  double* ent;
  int32_t* actions;        // [lane*E+e][T] or NULL
  float* probs;            // rollout: [lane*E+e][T][A]; forward: [lane*E+e][A]; or NULL
  const int8_t* deterministic;
  const float* reward_in;  // forward: reward carried by the obs
  const float* notdone;    // forward: done mask (policies/impala.py:170-176)
  uint64_t* dbg;           // diagnostics: phase clocks of conv workgroup 0 (fdr_impala_debug_clock) or NULL
  // pair form of the rollout core step (fdr_impala_desc.pairs): theta's (half) pack, the pairs' sigma-eps
  // (half) packs [n_lanes / 2][stride], the lanes' signs -- f16 operands in fp16 mode, f32 otherwise
  const _Float16* th;
  const _Float16* ep;
  const float* th32;
  const float* ep32;
  int64_t ep_stride;
  const int8_t* sign;
  // MFMA form (fp16 pairs): theta's image and the pairs' sigma-eps images [n_lanes / 2][kMImg]
  const _Float16* thm;
  const _Float16* epm;
  // fp16 conv: the lanes' folded BN / bias tables [lane][3][kBnTab] (scale | shift | conv bias), built once per rollout
  // by bn_table_kernel -- constant over the episode -- or NULL (each conv workgroup folds them itself)
  const float* bntab;
  // fp16 MFMA pair rollout with the replay GEMM: the core inputs as f16 rows of kCiPitch halves (zero beyond
  // kCoreIn) -- xproj_pair_kernel's B operand, rounded as it would round the f32 rows -- in place of ci, or NULL
  _Float16* ci16;
};

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;
constexpr float kBnEps = 1e-5f;
// kStrategy: the replay's sequence form over a probe set (get_strategy), probabilities out
enum CoreMode { kRollout = 0, kReplay = 1, kForward = 2, kStrategy = 3 };
constexpr bool seq_mode(int m) { return m == kReplay || m == kStrategy; }
constexpr int kCoreThreads = 256;

__device__ __forceinline__ float relu(float v) { return v > 0.f ? v : 0.f; }

// Streamed weights of the core kernels: each lane's W^T is read once per step and evicted before the
// next step needs it (GBs per step), so the loads are non-temporal (measured: f32 core 0.75 -> 0.68 ms,
// f16 0.41 -> 0.38 ms per step at 1024 lanes x 4 envs).
template <class T>
__device__ __forceinline__ T ld_stream(const T* p) {
  static_assert(sizeof(T) == 16 || sizeof(T) == 8, "8- or 16-byte streamed loads");
  typedef float fv __attribute__((ext_vector_type(sizeof(T) / 4)));
  const fv v = __builtin_nontemporal_load(reinterpret_cast<const fv*>(p));
  return __builtin_bit_cast(T, v);
}

// Softmax, action (argmax / inverse CDF on the counter stream), synthetic reward and return, or the
// entropy term (replay), or the probabilities (forward), for env e of lane `lane` (thread e < E).
// ent_acc (kReplay, optional): accumulate the step's entropy into this register instead of a.ent (a kernel that runs
// many replay steps stores it once)
// t_step >= 0: the step in place of a.t (a kernel that runs many steps)
template <int E, int MODE>
__device__ __forceinline__ void core_finish(const StepArgs& a, const float* logit, int lane, int j,
                                            bool step_entropy = false, double* ent_acc = nullptr, int t_step = -1) {
  const int at_t = t_step >= 0 ? t_step : a.t;
  const int A = a.n_act;
  const int64_t e0 = (int64_t)lane * E;
  const int e = j;
  const float* lg = logit + e * kMaxAct;
  float mx = -FLT_MAX;
  for (int i = 0; i < A; ++i) mx = fmaxf(mx, lg[i]);
  float p[kMaxAct];
  float sum = 0.f;
  for (int i = 0; i < A; ++i) {
    p[i] = expf(lg[i] - mx);
    sum += p[i];
  }
  const float inv = 1.f / sum;
  for (int i = 0; i < A; ++i) p[i] *= inv;
  const int64_t ge = e0 + e;
  if constexpr (MODE == kForward) {
    if (a.probs)
      for (int i = 0; i < A; ++i) a.probs[ge * A + i] = p[i];
  } else if constexpr (MODE == kStrategy) {
    for (int i = 0; i < A; ++i) a.probs[(ge * a.T + at_t) * A + i] = p[i];
  } else if constexpr (MODE == kRollout) {
    if (a.probs)
      for (int i = 0; i < A; ++i) a.probs[(ge * a.T + a.t) * A + i] = p[i];
    const uint64_t gid = (uint64_t)(a.lane_offset * E + ge);
    int act = 0;
    const bool det = a.deterministic && a.deterministic[lane];
    if (det) {
      float best = p[0];
      for (int i = 1; i < A; ++i)
        if (p[i] > best) { best = p[i]; act = i; }
    } else {  // inverse CDF, sequential f32 cumsum (oracle/policies.py categorical_inverse_cdf)
      float tot = 0.f;
      for (int i = 0; i < A; ++i) tot += p[i];
      const float u = uniform24(hash_ctr(a.akey, gid, (uint64_t)a.t, 0));
      const float target = u * tot;
      float cs = 0.f;
      for (int i = 0; i < A - 1; ++i) {
        cs += p[i];
        act += cs <= target ? 1 : 0;
      }
    }
    const uint64_t ctr = (gid << 32) | ((uint64_t)a.t << 11);
    const int tgt = (int)((mix64(a.rkey + ctr * kGolden) >> 40) % (uint64_t)A);
    const float r = act == tgt ? 1.f : (act == (tgt + 1) % A ? -1.f : 0.f);
    a.ret[ge] += (double)r;
    if (a.rprev) a.rprev[ge] = r;
    if (a.actions) a.actions[ge * a.T + a.t] = act;
  }
  // The step's entropy term -- the replay's, or a stateless policy's rollout (step_entropy: its mean per-step entropy
  // equals the batched one) -- as torch Categorical(probs).entropy(): normalise, log clamped at float min.
  if (MODE == kReplay || (MODE == kRollout && step_entropy)) {
    float tot = 0.f;
    for (int i = 0; i < A; ++i) tot += p[i];
    float h = 0.f;
    for (int i = 0; i < A; ++i) {
      const float pn = p[i] / tot;
      const float l = pn > 0.f ? logf(pn) : -FLT_MAX;
      h -= pn * l;
    }
    if (MODE == kReplay && ent_acc)
      *ent_acc += (double)h;
    else
      a.ent[ge] += (double)h;
  }
}

// Workspace carve-up of a call: consecutive 256-byte aligned regions, take() returns a region's byte offset
struct Carver {
  int64_t used = 0;
  int64_t take(int64_t bytes) {
    const int64_t at = used;
    used += (bytes > 0 ? bytes + 255 : 0) / 256 * 256;
    return at;
  }
};

// ---- fdr_pack.hip ----
// theta' pack (half = 0, f32, with the per-lane n2 partials) or half pack (half = 1, f16).  The transposed sections
// (fc W^T, [W_ih | W_hh]^T: 90 % of the pack) by tmode: kTrFull written; kTrNorm not written, n2 partials only (an
// fp16 call's f32 pack: its kernels read those weights from the half pack or the pair images); kTrSkip nothing
// (an fp16 call's f32 pack when n2 is not wanted, or its half pack under the pair core).  copies = false (half packs
// only: no n2): the other sections are not written either -- the pairs' sigma-eps packs that feed only the MFMA images
enum TransposedMode { kTrFull = 0, kTrNorm = 1, kTrSkip = 2 };
template <class OUT>  // float or _Float16
void launch_pack(const Layout& L, const LanesArgs& lanes, OUT* pack, double* n2, int n_lanes, int half,
                 hipStream_t stream, TransposedMode tmode = kTrFull, bool copies = true);
int launch_prep(const Layout& L, const LanesArgs& lanes, float* pack, double* n2_part, int n_lanes,
                hipStream_t stream);
int prep_blocks(const Layout& L);
__global__ void init_kernel(int64_t n_env, float* h, float* c, float* rprev, double* ret, double* ent);
__global__ void finish_kernel(int n_lanes, int envs, int T, int entropy, int jiggle, uint64_t akey,
                              int64_t lane_offset, const double* n2_part, int nblk, double* ret,
                              double* ent, int32_t* steps, double* norm2);

}  // namespace impala
}  // namespace fdr
