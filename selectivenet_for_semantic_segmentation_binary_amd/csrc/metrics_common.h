// What the eval metrics kernels share (train_io.hip, boundary.hip, calibration.hip): which pixels count and as
// what, the walk over the pixels, the threshold search and the per-image launch loop — one definition each, so
// that every report decides every pixel alike. The closing reduction (block_reduce) is in common.h.
#pragma once

#include "common.h"

namespace selunet {

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ the pixel rule
// One of PIXEL_STATES states per pixel: 0..3 the confusion-matrix cell label * 2 + pred (cm[label][pred],
// row-major, as Evaluator.confusion_matrix), 4 selected with a label >= 2 (counted in `pixels` only), 5 not
// selected. A pixel is selected iff there is no selection plane or sel >= t_sel (a NaN selection abstains);
// pred = out >= t_out (a NaN output predicts 0): t_out / t_sel are the smallest fp32 logits the reference's
// host rule maps to 1 (computed once on the host from the same numpy expression, see metrics.py).
// predict_common.h's pixel_class is the same two comparisons without a label. The rule's three expressions are
// functions of their own for the two kernels that do not want the state as a number: calibration_bins_kernel
// takes the states' exits one by one (testing the state's value cost it 5 % on the MI355X), and
// patch_auc_kernel needs the label of a counted pixel and no prediction (through the state: 0.7 % on 512 x 512).
constexpr int PIXEL_STATES = 6;
// label.astype('uint8') of a {0,1} float target (train.py:206; eval.py:229)
__device__ __forceinline__ int pixel_label(float t) { return (int)(uint8_t)t; }
__device__ __forceinline__ bool pixel_selected(float s, bool has_sel, float t_sel) { return !has_sel || s >= t_sel; }
__device__ __forceinline__ int pixel_pred(float o, float t_out) { return o >= t_out ? 1 : 0; }
__device__ __forceinline__ int pixel_state(float o, float s, float t, bool has_sel, float t_out, float t_sel) {
  const int lab = pixel_label(t);
  return !pixel_selected(s, has_sel, t_sel) ? 5 : lab >= 2 ? 4 : lab * 2 + pixel_pred(o, t_out);
}

// ------------------------------------------------------------------ the pixel walk
// A plane that may be absent: it reads as 0.
template <typename T> struct Nullable {
  const T* p;
};
template <typename T> __device__ __forceinline__ Nullable<T> nullable(const T* p) { return {p}; }

__device__ __forceinline__ f32x4 load4(const float* p, int64_t i) { return *reinterpret_cast<const f32x4*>(p + i * 4); }
__device__ __forceinline__ i32x4 load4(const int32_t* p, int64_t i) { return *reinterpret_cast<const i32x4*>(p + i * 4); }
__device__ __forceinline__ f32x4 load4(Nullable<float> n, int64_t i) { return n.p ? load4(n.p, i) : f32x4{0, 0, 0, 0}; }
template <typename T> __device__ __forceinline__ T load1(const T* p, int64_t i) { return p[i]; }
__device__ __forceinline__ float load1(Nullable<float> n, int64_t i) { return n.p ? n.p[i] : 0.0f; }

// f(one value of each plane) for every pixel of this workgroup's share of p: the workgroups blockIdx.x of
// gridDim.x (TPB threads each) stride over the p / 4 groups of four pixels with one 16-B load per plane, then
// over the scalar tail.
// vec = false walks everything as the tail (planes that are not 16-B aligned). The planes are float or int32
// pointers or `nullable(float pointer)`, not __restrict__: a caller's planes may alias.
template <int TPB, typename F, typename... P>
__device__ __forceinline__ void for_each_pixel(int64_t p, bool vec, F f, P... planes) {
  const int64_t p4 = vec ? p >> 2 : 0;
  const int64_t stride = (int64_t)gridDim.x * TPB;
  const int64_t first = blockIdx.x * (int64_t)TPB + threadIdx.x;
  auto four = [&](auto... v) {
#pragma unroll
    for (int j = 0; j < 4; ++j) f(v[j]...);
  };
  for (int64_t i = first; i < p4; i += stride) four(load4(planes, i)...);
  for (int64_t i = p4 * 4 + first; i < p; i += stride) f(load1(planes, i)...);
}

// ------------------------------------------------------------------ the threshold search
// thr[0 .. N-1] = the k <= N ascending thresholds t, NaN-padded: `s >= NaN` is false, so the padded list keeps
// its true-prefix shape for s = +inf too. Every thread of the workgroup calls it; a barrier follows.
template <int TPB, int N>
__device__ __forceinline__ void stage_thresholds(float (&thr)[N], const float* __restrict__ t, int k) {
  for (int i = threadIdx.x; i < N; i += TPB) thr[i] = i < k ? t[i] : __builtin_nanf("");
}

// #{j : s >= thr[j]} over thr[0 .. 2 * top - 2], the length of the true prefix, by binary search from stride top
__device__ __forceinline__ int true_prefix(const float* thr, float s, int top) {
  int b = 0;
  for (int st = top; st > 0; st >>= 1) b += s >= thr[b + st - 1] ? st : 0;
  return b;
}

// the first stride of true_prefix: the largest power of two <= k
inline int search_top(int k) {
  int top = 1;
  while (top * 2 <= k) top *= 2;
  return top;
}

// ------------------------------------------------------------------ per-image launches (host)
// blockIdx.y is the image: launch(first image, images) for at most `per` <= IMAGE_GRID_Y images at a time
constexpr int32_t IMAGE_GRID_Y = 32768;  // a grid's y dimension is 16 bits wide
template <typename L> inline void for_image_chunks(int32_t n, int32_t per, L launch) {
  for (int32_t i0 = 0; i0 < n; i0 += per) launch(i0, (unsigned)std::min(n - i0, per));
}

}  // namespace selunet
