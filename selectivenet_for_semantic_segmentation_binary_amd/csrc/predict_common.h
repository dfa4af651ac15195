// What the whole-image prediction kernels share (predict_io.hip; predict_tta.hip, §7g): the
// reflect fold, the mask's classification rule, the probability level, the reduction of the pixel counts
// and the argument rules of the per-tile calls — one definition each, so that the plain and the
// test-time-augmented path decide every pixel alike.
#pragma once

#include "common.h"

namespace selunet {

constexpr int PRED_TPB = 256;
constexpr int PRED_MAX_HW = 65535;  // image height / width the calls take

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// numpy's 'reflect' padding as an index map onto [0, n): the edge is not repeated, period 2 (n - 1),
// folded as often as needed; 0 for n = 1.
__device__ __forceinline__ int reflect_index(int64_t i, int n) {
  if (n == 1) return 0;
  const int64_t period = 2 * ((int64_t)n - 1);
  int64_t m = i % period;
  m = m < 0 ? m + period : m;
  return (int)(m < n ? m : period - m);
}

struct rgb4 {
  uint32_t w[3];
};

// floor(255 sigmoid(v) + 0.5) as a byte; NaN -> 0
__device__ __forceinline__ uint32_t prob_level(float v) {
  const float p = 255.0f * sigmoidf_(v) + 0.5f;
  return p >= 0.0f ? (uint32_t)p : 0u;  // p in [0.5, 255.5]: the conversion truncates = floor; NaN fails the test
}

// A pixel's class {0 background, 1 tumor, 2 abstained}: `not (sel >= t_sel)` abstains, so a NaN selection
// abstains; a NaN output is background. The two comparisons are pixel_state's (metrics_common.h), the rule of
// the eval metrics, without a label: they must stay the same expressions.
__device__ __forceinline__ int pixel_class(bool selective, float s, float o, float t_sel, float t_out) {
  return (selective && !(s >= t_sel)) ? 2 : (o >= t_out ? 1 : 0);
}

// The mask's byte for a class: 0 background, 255 tumor, 127 abstained.
__device__ __forceinline__ uint32_t mask_level(int cls) { return cls == 2 ? 127u : (cls == 1 ? 255u : 0u); }

// counts += {c[0], c[1], c[2], c[0] + c[1] + c[2]} summed over the workgroup (PRED_TPB threads, all of them
// calling) by block_sum (common.h), then four integer atomics. Word 3, `pixels`, is the three classes' sum.
__device__ __forceinline__ void add_class_counts(const unsigned (&c)[3], unsigned long long* __restrict__ counts) {
  const unsigned c4[4] = {c[0], c[1], c[2], c[0] + c[1] + c[2]};
  const unsigned long long s = block_sum<4, PRED_TPB>(c4);
  if (threadIdx.x < 4 && s) atomicAdd(counts + threadIdx.x, s);
}

// The argument rules the per-tile calls share; `fn` names the call in the message.
inline int tile_args(const char* fn, const int32_t* origins, int32_t n, int32_t h, int32_t w, int32_t th, int32_t tw) {
  SELUNET_REQUIRE(origins, "%s: null origins", fn);
  SELUNET_REQUIRE(n >= 1, "%s: n must be >= 1 (got %d)", fn, n);
  SELUNET_REQUIRE(h >= 1 && h <= PRED_MAX_HW && w >= 1 && w <= PRED_MAX_HW,
                  "%s: image height and width must be in [1, %d] (got %d x %d)", fn, PRED_MAX_HW, h, w);
  SELUNET_REQUIRE(th >= 8 && tw >= 8 && th % 8 == 0 && tw % 8 == 0,
                  "%s: tile height and width must be multiples of 8, at least 8 (got %d x %d)", fn, th, tw);
  SELUNET_REQUIRE(((uintptr_t)origins & 3) == 0, "%s: origins must be 4-B aligned", fn);
  return SELUNET_OK;
}

}  // namespace selunet
