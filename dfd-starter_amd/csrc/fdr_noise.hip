// fdr_noise.hip -- host index draw (fdr_noise_draw_indices): host code only, no kernel.
//
// Host index draw (utils/noise_sources.py:44-47: one RandomState.randint(0, max_idx) per sample).  MT19937
// (Matsumoto & Nishimura 1998, the generator behind numpy's legacy RandomState) advanced in place from the
// state numpy reports (key[624], pos), and numpy's masked rejection for ranges that fit 32 bits: each draw takes
// 32-bit words masked by the smallest all-ones mask >= max_idx - 1 until one is <= max_idx - 1.  numpy makes
// one indirect generator call and one unpredictable branch per word (~11 ns per index on the build host); a block
// of tempered words with a branch-free compaction takes ~2.5 ns, which keeps an 8-rank step's 16,384-index draw
// (every rank consumes the whole stream) well under the rollout it overlaps.
#include "fdr_internal.h"

namespace {
constexpr int kMtN = 624, kMtM = 397;

void mt_refill(uint32_t* key) {
  auto mix = [](uint32_t hi, uint32_t lo, uint32_t far) {
    const uint32_t y = (hi & 0x80000000u) | (lo & 0x7fffffffu);
    return far ^ (y >> 1) ^ ((0u - (y & 1u)) & 0x9908b0dfu);
  };
  int i = 0;
  for (; i < kMtN - kMtM; ++i) key[i] = mix(key[i], key[i + 1], key[i + kMtM]);
  for (; i < kMtN - 1; ++i) key[i] = mix(key[i], key[i + 1], key[i + kMtM - kMtN]);
  key[kMtN - 1] = mix(key[kMtN - 1], key[0], key[kMtM - 1]);
}

inline uint32_t mt_temper(uint32_t y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  return y ^ (y >> 18);
}
}  // namespace

extern "C" int fdr_noise_draw_indices(uint32_t* key, int32_t* pos, int64_t max_idx, int32_t n, int64_t* out) {
  using namespace fdr;
  if (!key || !pos || (n > 0 && !out) || n < 0) return set_error(FDR_ERR_INVALID, "NULL pointer / bad n");
  if (max_idx < 1) return set_error(FDR_ERR_INVALID, "max_idx must be >= 1");
  if (*pos < 0 || *pos > kMtN) return set_error(FDR_ERR_INVALID, "MT19937 pos out of range");
  const uint64_t rng = (uint64_t)max_idx - 1;  // inclusive range of randint(0, max_idx)
  if (rng > 0xFFFFFFFFull) return set_error(FDR_ERR_UNSUPPORTED, "index range wider than 32 bits");
  if (rng == 0) {  // numpy returns the offset without drawing
    for (int32_t i = 0; i < n; ++i) out[i] = 0;
    return FDR_OK;
  }
  uint32_t mask = (uint32_t)rng;
  mask |= mask >> 1;
  mask |= mask >> 2;
  mask |= mask >> 4;
  mask |= mask >> 8;
  mask |= mask >> 16;
  // a refill block at a time: temper + mask the block's remaining words (vectorised), then a branch-free
  // compaction keeps the accepted ones; the last block stops at the word that completes the n-th index, as
  // numpy's loop does (no extra words consumed)
  int p = *pos;
  int32_t k = 0;
  uint32_t buf[kMtN];
  while (k < n) {
    if (p == kMtN) {
      mt_refill(key);
      p = 0;
    }
    const int m = kMtN - p;
    for (int i = 0; i < m; ++i) buf[i] = mt_temper(key[p + i]) & mask;
    if (n - k >= m) {  // the whole block fits: k < n at every write
      for (int i = 0; i < m; ++i) {
        out[k] = buf[i];
        k += buf[i] <= (uint32_t)rng;
      }
      p += m;
    } else {
      int i = 0;
      for (; i < m && k < n; ++i) {
        out[k] = buf[i];
        k += buf[i] <= (uint32_t)rng;
      }
      p += i;
    }
  }
  *pos = p;
  return FDR_OK;
}
