// Calibration report of eval:
//
//  * selunet_calibration_bins: in one pass over a score plane, the reliability histogram of
//    sigmoid(score / T) against an event (the label, or "the prediction is right"), per bin the event
//    counts and the fixed-point sums of the probability, of its squared error and of its negative log
//    likelihood, and a fine histogram of the raw score by event that the host's temperature fit reads.
//
// The per-pixel values are formed in fp64 and rounded once to integers; everything summed is an integer
// and every atomic an integer atomic, so the result does not depend on the order of arrival.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "metrics_common.h"

namespace selunet {

constexpr int CALIB_TPB = 256;
// One workgroup per CU, as the sweep: every workgroup closes with atomics on the same cache lines.
constexpr int CALIB_GRID = 256;
constexpr int CALIB_EDGES = SELUNET_CALIB_MAX_EDGES + 1;  // the NaN-padded list the search walks
constexpr int CALIB_COLS = 5;
constexpr int CALIB_FINE_WORDS = SELUNET_CALIB_FINE_CELLS * 2;
// The accumulated sums hold 2^33 pixels of at most 2^30 each. Per launch a workgroup sees about p / CALIB_GRID
// <= 2^25 pixels: the bound of a 32-bit on-chip `fine` counter (the on-chip sums of `bins` are 64-bit).
constexpr int64_t CALIB_MAX_PIXELS = (int64_t)1 << 33;

// {P, B, L} of one considered pixel (selunet.h). No contraction: numpy evaluates the same expression
// operation by operation, and the two may differ only where a rounding tie falls differently.
struct CalibTerms {
  unsigned long long p, b, l;
};

__device__ __forceinline__ CalibTerms calib_terms(float score, int e, double inv_temperature) {
#pragma clang fp contract(off)
  const double x = (double)score * inv_temperature;
  const double s = x >= 0.0 ? 1.0 / (1.0 + exp(-x)) : exp(x) / (1.0 + exp(x));
  const double d = s - (double)e;
  const double v = e ? -x : x;
  const double nll = fmin(fmax(v, 0.0) + log1p(exp(-fabs(v))), (double)SELUNET_CALIB_NLL_MAX);
  CalibTerms t;
  t.p = (unsigned long long)llrint(s * (double)(1 << SELUNET_CALIB_FRAC_BITS));
  t.b = (unsigned long long)llrint(d * d * (double)(1 << SELUNET_CALIB_FRAC_BITS));
  t.l = (unsigned long long)llrint(nll * (double)(1 << SELUNET_CALIB_NLL_BITS));
  return t;
}

// Trained networks put most pixels into the two end bins and the two end cells, so same-address LDS
// atomics are the hazard. Each lane therefore keeps the sums of the bin (and the counts of the cell) it
// saw last in registers and adds them to the workgroup's on-chip histograms only when its bin (cell)
// changes and once at the end: a run of pixels in one bin costs no atomic at all, scores spread over
// many bins cost the plain per-pixel atomics on distinct addresses. The sums are 64-bit in registers and
// on chip (P, B and L reach 2^30 per pixel). The workgroup closes with one contiguous block of 64-bit
// global atomics over the cells it touched.
// top: the largest power of two <= m (the first binary-search stride); m <= 255, so eight halvings
// tell every bin apart.
__global__ __launch_bounds__(CALIB_TPB) void calibration_bins_kernel(
    const float* score, const float* out, const float* sel, const float* __restrict__ target, int64_t p, int event,
    float t_out, float t_sel, const float* __restrict__ edges, int m, int top, double inv_temperature,
    unsigned long long* __restrict__ bins, unsigned long long* __restrict__ fine, unsigned long long* __restrict__ misc) {
  __shared__ float thr[CALIB_EDGES];
  __shared__ unsigned long long lbins[CALIB_EDGES * CALIB_COLS];
  __shared__ unsigned lfine[CALIB_FINE_WORDS];
  __shared__ unsigned lmisc[2];
  const int cells = (m + 1) * CALIB_COLS;
  stage_thresholds<CALIB_TPB>(thr, edges, m);
  for (int i = threadIdx.x; i < cells; i += CALIB_TPB) lbins[i] = 0;
  if (fine)
    for (int i = threadIdx.x; i < CALIB_FINE_WORDS; i += CALIB_TPB) lfine[i] = 0;
  if (threadIdx.x < 2) lmisc[threadIdx.x] = 0;
  __syncthreads();

  int cur_bin = -1, cur_cell = -1;  // what this lane's registers hold
  unsigned n_ev[2] = {0, 0}, f_ev[2] = {0, 0}, nan_scores = 0, other_labels = 0;
  unsigned long long sum_p = 0, sum_b = 0, sum_l = 0;

  auto flush_bin = [&]() {
    if (cur_bin < 0) return;
    unsigned long long* row = lbins + cur_bin * CALIB_COLS;
    if (n_ev[0]) atomicAdd(row + 0, (unsigned long long)n_ev[0]);
    if (n_ev[1]) atomicAdd(row + 1, (unsigned long long)n_ev[1]);
    if (sum_p) atomicAdd(row + 2, sum_p);
    if (sum_b) atomicAdd(row + 3, sum_b);
    if (sum_l) atomicAdd(row + 4, sum_l);
    n_ev[0] = n_ev[1] = 0;
    sum_p = sum_b = sum_l = 0;
  };
  auto flush_cell = [&]() {
    if (cur_cell < 0) return;
    if (f_ev[0]) atomicAdd(&lfine[cur_cell * 2 + 0], f_ev[0]);
    if (f_ev[1]) atomicAdd(&lfine[cur_cell * 2 + 1], f_ev[1]);
    f_ev[0] = f_ev[1] = 0;
  };
  auto one = [&](float sc, float o, float s, float t) {
    // pixel_state's 5, 4 and cm cells in turn, from its own three expressions (a NaN score is in no cell)
    if (!pixel_selected(s, sel != nullptr, t_sel)) return;
    const int lab = pixel_label(t);
    if (lab >= 2) {
      other_labels += 1;
      return;
    }
    if (sc != sc) {
      nan_scores += 1;
      return;
    }
    const int e = event == 0 ? lab : (int)(pixel_pred(o, t_out) == lab);
    const int b = true_prefix(thr, sc, top);
    if (b != cur_bin) {
      flush_bin();
      cur_bin = b;
    }
    const CalibTerms v = calib_terms(sc, e, inv_temperature);
    n_ev[e] += 1;
    sum_p += v.p;
    sum_b += v.b;
    sum_l += v.l;
    if (fine) {
      const int cell = sc < -32.0f ? 0 : sc >= 32.0f ? SELUNET_CALIB_FINE_CELLS - 1 : 2049 + (int)floorf(sc * 64.0f);
      if (cell != cur_cell) {
        flush_cell();
        cur_cell = cell;
      }
      f_ev[e] += 1;
    }
  };

  // score may be the same plane as out or sel: for_each_pixel's planes are not __restrict__
  for_each_pixel<CALIB_TPB>(p, true, one, score, nullable(event ? out : nullptr), nullable(sel), target);
  flush_bin();
  flush_cell();
  const unsigned a = wave_sum(nan_scores), b = wave_sum(other_labels);
  if ((threadIdx.x & 63) == 0) {
    if (a) atomicAdd(&lmisc[0], a);
    if (b) atomicAdd(&lmisc[1], b);
  }
  __syncthreads();
  // One thread per word, so that a wave's atomic covers 512 contiguous bytes (as the sweep's closing block)
  for (int i = threadIdx.x; i < cells; i += CALIB_TPB)
    if (lbins[i]) atomicAdd(bins + i, lbins[i]);
  if (fine)
    for (int i = threadIdx.x; i < CALIB_FINE_WORDS; i += CALIB_TPB)
      if (lfine[i]) atomicAdd(fine + i, (unsigned long long)lfine[i]);
  if (threadIdx.x < 2 && lmisc[threadIdx.x]) atomicAdd(misc + threadIdx.x, (unsigned long long)lmisc[threadIdx.x]);
}

}  // namespace selunet

using namespace selunet;

extern "C" {

int selunet_calibration_bins(const float* score, const float* out, const float* sel, const float* target, int64_t p,
                             int32_t event, float t_out, float t_sel, const float* edges, int32_t m,
                             double inv_temperature, unsigned long long* bins, unsigned long long* fine,
                             unsigned long long* misc, void* stream) {
  SELUNET_REQUIRE(score && target && edges && bins && misc, "calibration_bins: null score, target, edges, bins or misc");
  SELUNET_REQUIRE(event == 0 || event == 1, "calibration_bins: event must be 0 (the label) or 1 (the prediction is "
                  "right) (got %d)", event);
  SELUNET_REQUIRE(event == 0 || out, "calibration_bins: null out with event 1");
  SELUNET_REQUIRE(p >= 1 && p <= CALIB_MAX_PIXELS, "calibration_bins: p must be in [1, 2^33] (got %lld)", (long long)p);
  SELUNET_REQUIRE(m >= 1 && m <= SELUNET_CALIB_MAX_EDGES, "calibration_bins: m must be in [1, %d] (got %d)",
                  SELUNET_CALIB_MAX_EDGES, m);
  SELUNET_REQUIRE(std::isfinite(inv_temperature) && inv_temperature > 0,
                  "calibration_bins: inv_temperature must be finite and > 0 (got %g)", inv_temperature);
  SELUNET_REQUIRE(aligned(15, score, target, sel) && (event == 0 || aligned(15, out)),
                  "calibration_bins: score, out, sel and target must be 16-B aligned");
  SELUNET_REQUIRE(aligned(3, edges), "calibration_bins: edges must be 4-B aligned");
  SELUNET_REQUIRE(aligned(7, bins, fine, misc), "calibration_bins: bins, fine and misc must be 8-B aligned");
  const int top = search_top(m);
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(p / 4 + 1, CALIB_TPB), CALIB_GRID));
  hipLaunchKernelGGL(calibration_bins_kernel, dim3(grid), dim3(CALIB_TPB), 0, as_stream(stream), score, out, sel,
                     target, p, (int)event, t_out, t_sel, edges, (int)m, top, inv_temperature, bins, fine, misc);
  return check_launch("calibration_bins");
}

}  // extern "C"
