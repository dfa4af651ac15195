// Boundary-distance metrics of eval:
//
//  * selunet_edt_sq: the exact squared Euclidean distance of every pixel of a thresholded plane to the
//    nearest pixel of the other class, in the separable form: a column pass leaves, per pixel, the squared
//    vertical distance to the nearest pixel of the other class in its column; a row pass takes
//    min over x' of (x - x')^2 + g(x'), g(x') = 0 where x' is of the other class and its column value
//    where it is of the pixel's own.
//  * selunet_boundary_bands: selunet_seg_metrics' six counts by band of that distance.
//  * selunet_boundary_rows: per image, the largest distance of a false positive / false negative to the
//    other mask (the squared directed Hausdorff distances) and the error counts within a tolerance.
//
// Integer work throughout; the sums and maxima close in integer atomics, so the order does not matter.
#include <algorithm>
#include <climits>

#include "common.h"
#include "metrics_common.h"

namespace selunet {

constexpr int EDT_COL_TPB = 64;     // one wave per 64 columns: n * w / 64 workgroups spread over the CUs
constexpr int EDT_ROW_TPB = 256;    // the row chunk: a thread takes pixels x, x + 256, ...
// "no pixel of the other class in this column". Above every distance (2 * 4095^2 < 2^26), and
// 4095^2 + EDT_INF < 2^29: the row pass adds without overflow.
constexpr int32_t EDT_INF = 1 << 28;
constexpr int EDT_FAR = 1 << 14;    // a row index no image has, on either side: |y - far| > 4095

// Column pass. Thread = one column of one image. Down: the distance (not squared) to the nearest pixel
// of the other class above, into v; up: the same below, the smaller of the two squared (EDT_INF when the
// column holds the pixel's class only). Every load and store is coalesced over the columns of a wave.
__global__ __launch_bounds__(EDT_COL_TPB) void edt_columns_kernel(const float* __restrict__ x, float t, int h,
                                                                  int w, int col_blocks, int32_t* __restrict__ v) {
  const int img = blockIdx.x / col_blocks;
  const int col = (blockIdx.x % col_blocks) * EDT_COL_TPB + threadIdx.x;
  if (col >= w) return;
  const int64_t base = (int64_t)img * h * w + col;
  int last[2] = {-EDT_FAR, -EDT_FAR};  // the last row seen of class 0 / 1
#pragma unroll 8
  for (int y = 0; y < h; ++y) {
    const int64_t at = base + (int64_t)y * w;
    const bool f = x[at] >= t;
    v[at] = y - (f ? last[0] : last[1]);
    if (f) last[1] = y; else last[0] = y;
  }
  int next[2] = {EDT_FAR, EDT_FAR};
#pragma unroll 8
  for (int y = h - 1; y >= 0; --y) {
    const int64_t at = base + (int64_t)y * w;
    const bool f = x[at] >= t;
    const int d = min(v[at], (f ? next[0] : next[1]) - y);
    v[at] = d >= SELUNET_EDT_MAX_SIDE ? EDT_INF : d * d;
    if (f) next[1] = y; else next[0] = y;
  }
}

// Row pass, in place: workgroup = one row of one image, read whole into LDS before any of it is written.
// cost[c][x'] is what a pixel of class c pays for column x': 0 where x' is of the other class, the column
// value where it is of class c. A pixel scans outward from its own column and stops once the horizontal
// term alone reaches the best sum so far. A row whose every cost of a class is EDT_INF (an image without
// the other class) skips the scan.
__global__ __launch_bounds__(EDT_ROW_TPB) void edt_rows_kernel(const float* __restrict__ x, float t, int w,
                                                               int32_t* __restrict__ d2) {
  extern __shared__ int32_t cost[];  // [2][w], then the two row minima
  int32_t* rmin = cost + 2 * w;
  const int64_t base = (int64_t)blockIdx.x * w;
  if (threadIdx.x < 2) rmin[threadIdx.x] = EDT_INF;
  __syncthreads();
  int32_t m0 = EDT_INF, m1 = EDT_INF;
  for (int i = threadIdx.x; i < w; i += EDT_ROW_TPB) {
    const bool f = x[base + i] >= t;
    const int32_t v = d2[base + i];  // >= 1
    const int32_t c0 = f ? 0 : v, c1 = f ? v : 0;
    cost[i] = c0;
    cost[w + i] = c1;
    m0 = min(m0, c0);
    m1 = min(m1, c1);
  }
  atomicMin(&rmin[0], m0);
  atomicMin(&rmin[1], m1);
  __syncthreads();
  const bool none[2] = {rmin[0] >= EDT_INF, rmin[1] >= EDT_INF};
  for (int i = threadIdx.x; i < w; i += EDT_ROW_TPB) {
    const int c = cost[i] == 0 ? 1 : 0;  // foreground pays nothing in cost[0]
    int32_t best = SELUNET_EDT_NONE;
    if (!none[c]) {
      const int32_t* cc = cost + c * w;
      best = cc[i];
      for (int d = 1; d < w; ++d) {
        const int32_t dd = d * d;
        if (dd >= best) break;
        const int l = i - d, r = i + d;
        if (l >= 0) best = min(best, dd + cc[l]);
        if (r < w) best = min(best, dd + cc[r]);
      }
      if (best >= EDT_INF) best = SELUNET_EDT_NONE;
    }
    d2[base + i] = best;
  }
}

constexpr int BND_TPB = 256;
constexpr int BND_STATES = PIXEL_STATES;  // pixel_state (metrics_common.h): selunet_seg_metrics' pixel rule
struct BandEdges {
  int32_t r2[SELUNET_BAND_MAX];
  int32_t k;
};

// One LDS histogram [band][state] per workgroup, one LDS atomic per pixel; the six words of a band
// follow from its states at the end (selected = states 0..4, pixels = all six).
__global__ __launch_bounds__(BND_TPB) void boundary_bands_kernel(
    const float* __restrict__ out, const float* __restrict__ sel, const float* __restrict__ target,
    const int32_t* __restrict__ d2, int64_t p, float t_out, float t_sel, BandEdges e,
    unsigned long long* __restrict__ bins) {
  __shared__ unsigned hist[(SELUNET_BAND_MAX + 2) * BND_STATES];
  const int nb = e.k + 2;
  for (int i = threadIdx.x; i < nb * BND_STATES; i += BND_TPB) hist[i] = 0;
  __syncthreads();
  auto one = [&](float o, float t, float s, int32_t d) {
    int b = 0;
    for (int j = 0; j < e.k; ++j) b += d > e.r2[j];
    if (d == SELUNET_EDT_NONE) b = e.k + 1;
    atomicAdd(&hist[b * BND_STATES + pixel_state(o, s, t, sel != nullptr, t_out, t_sel)], 1u);
  };
  for_each_pixel<BND_TPB>(p, true, one, out, target, nullable(sel), d2);
  __syncthreads();
  for (int i = threadIdx.x; i < nb * 6; i += BND_TPB) {
    const unsigned* hb = hist + (i / 6) * BND_STATES;
    const int word = i % 6;
    unsigned long long v = hb[word];  // words 0..3: the cm cells
    if (word == 4) v = (unsigned long long)hb[0] + hb[1] + hb[2] + hb[3] + hb[4];
    if (word == 5) v = (unsigned long long)hb[0] + hb[1] + hb[2] + hb[3] + hb[4] + hb[5];
    if (v) atomicAdd(bins + i, v);
  }
}

// blockIdx.y = the image, its hw pixels shared by the gridDim.x workgroups of the row.
__global__ __launch_bounds__(BND_TPB) void boundary_rows_kernel(
    const float* __restrict__ out, const float* __restrict__ sel, const float* __restrict__ target,
    const int32_t* __restrict__ d2_target, const int32_t* __restrict__ d2_pred, int64_t hw, float t_out,
    float t_sel, int32_t tol_sq, unsigned long long* __restrict__ rows) {
  const int64_t base = (int64_t)blockIdx.y * hw;
  out += base;
  target += base;
  d2_target += base;
  d2_pred += base;
  if (sel) sel += base;
  unsigned mx[2] = {0, 0};  // distances are non-negative int32
  unsigned cnt[4] = {0, 0, 0, 0};
  auto one = [&](float o, float t, float s, int32_t dt, int32_t dp) {
    const int st = pixel_state(o, s, t, sel != nullptr, t_out, t_sel);
    if (st == 1) {  // label 0, predicted 1
      mx[0] = max(mx[0], (unsigned)dt);
      cnt[0] += dt <= tol_sq;
      cnt[2] += 1;
    } else if (st == 2) {  // label 1, predicted 0
      mx[1] = max(mx[1], (unsigned)dp);
      cnt[1] += dp <= tol_sq;
      cnt[3] += 1;
    }
  };
  // image bases are 16-B aligned only when hw % 4 == 0
  for_each_pixel<BND_TPB>(hw, (hw & 3) == 0, one, out, target, nullable(sel), d2_target, d2_pred);
  unsigned long long* words = rows + (int64_t)blockIdx.y * 6 + threadIdx.x;
  const unsigned long long m = block_reduce<2, BND_TPB>(mx, [](auto a, auto b) { return max(a, b); });
  if (threadIdx.x < 2 && m) atomicMax(words, m);
  const unsigned long long v = block_sum<4, BND_TPB>(cnt);
  if (threadIdx.x < 4 && v) atomicAdd(words + 2, v);
}

}  // namespace selunet

using namespace selunet;

extern "C" {

int selunet_edt_sq(const float* x, float t, int32_t n, int32_t h, int32_t w, int32_t* d2, void* stream) {
  SELUNET_REQUIRE(x && d2, "edt_sq: null x or d2");
  SELUNET_REQUIRE(n >= 1, "edt_sq: n must be >= 1 (got %d)", n);
  SELUNET_REQUIRE(h >= 1 && h <= SELUNET_EDT_MAX_SIDE && w >= 1 && w <= SELUNET_EDT_MAX_SIDE,
                  "edt_sq: h and w must be in [1, %d], where squared distances fit 31 bits (got %d x %d)",
                  SELUNET_EDT_MAX_SIDE, h, w);
  SELUNET_REQUIRE((int64_t)n * std::max(h, w) <= INT32_MAX, "edt_sq: n * max(h, w) must be below 2^31 (got %d x %d x %d)",
                  n, h, w);
  SELUNET_REQUIRE(aligned(3, x, d2), "edt_sq: x and d2 must be 4-B aligned");
  const int col_blocks = (int)cdiv(w, EDT_COL_TPB);
  hipLaunchKernelGGL(edt_columns_kernel, dim3((unsigned)(n * col_blocks)), dim3(EDT_COL_TPB), 0, as_stream(stream), x,
                     t, h, w, col_blocks, d2);
  hipLaunchKernelGGL(edt_rows_kernel, dim3((unsigned)(n * h)), dim3(EDT_ROW_TPB), (size_t)(2 * w + 2) * sizeof(int32_t),
                     as_stream(stream), x, t, w, d2);
  return check_launch("edt_sq");
}

int selunet_boundary_bands(const float* out, const float* sel, const float* target, const int32_t* d2_target,
                           int32_t n, int64_t hw, float t_out, float t_sel, const int32_t* r2, int32_t k,
                           unsigned long long* bins, void* stream) {
  SELUNET_REQUIRE(out && target && d2_target && r2 && bins, "boundary_bands: null out, target, d2_target, r2 or bins");
  SELUNET_REQUIRE(n >= 1 && hw >= 1 && hw <= ((int64_t)1 << 40) / n,
                  "boundary_bands: n and hw must be >= 1 and n * hw <= 2^40 (got %d x %lld)", n, (long long)hw);
  SELUNET_REQUIRE(k >= 1 && k <= SELUNET_BAND_MAX, "boundary_bands: k must be in [1, %d] (got %d)", SELUNET_BAND_MAX, k);
  BandEdges e = {};
  e.k = k;
  for (int j = 0; j < k; ++j) {
    SELUNET_REQUIRE(r2[j] >= 1 && (j == 0 || r2[j] > r2[j - 1]),
                    "boundary_bands: r2 must be strictly increasing from r2[0] >= 1 (r2[%d] = %d)", j, r2[j]);
    e.r2[j] = r2[j];
  }
  SELUNET_REQUIRE(aligned(15, out, target, sel, d2_target), "boundary_bands: inputs must be 16-B aligned");
  SELUNET_REQUIRE(aligned(7, bins), "boundary_bands: bins must be 8-B aligned");
  const int64_t p = (int64_t)n * hw;
  // p <= 2^40 over at least min(p / 1024, 2048) workgroups: a 32-bit LDS count stays below 2^30 (at the default
  // grid; SELUNET_OPT_IO_GRID can make it smaller and is for tests and small inputs only, see selunet.h)
  const unsigned grid = (unsigned)io_grid(cdiv(p / 4 + 1, BND_TPB), 2048);
  hipLaunchKernelGGL(boundary_bands_kernel, dim3(grid), dim3(BND_TPB), 0, as_stream(stream), out, sel, target,
                     d2_target, p, t_out, t_sel, e, bins);
  return check_launch("boundary_bands");
}

int selunet_boundary_rows(const float* out, const float* sel, const float* target, const int32_t* d2_target,
                          const int32_t* d2_pred, int32_t n, int64_t hw, float t_out, float t_sel, int32_t tol_sq,
                          unsigned long long* rows, void* stream) {
  SELUNET_REQUIRE(out && target && d2_target && d2_pred && rows,
                  "boundary_rows: null out, target, d2_target, d2_pred or rows");
  SELUNET_REQUIRE(n >= 1, "boundary_rows: n must be >= 1 (got %d)", n);
  SELUNET_REQUIRE(hw >= 1 && hw <= ((int64_t)1 << 24), "boundary_rows: hw must be in [1, 2^24] (got %lld)",
                  (long long)hw);
  SELUNET_REQUIRE(tol_sq >= 0, "boundary_rows: tol_sq must be >= 0 (got %d)", tol_sq);
  SELUNET_REQUIRE(aligned((hw & 3) ? 3 : 15, out, target, sel, d2_target, d2_pred),
                  "boundary_rows: inputs must be 16-B aligned (4-B when hw is not a multiple of 4)");
  SELUNET_REQUIRE(aligned(7, rows), "boundary_rows: rows must be 8-B aligned");
  const unsigned gx = (unsigned)io_grid(cdiv(hw / 4, BND_TPB * 4), 64);
  for_image_chunks(n, IMAGE_GRID_Y, [&](int32_t i0, unsigned ny) {
    const int64_t o = (int64_t)i0 * hw;
    hipLaunchKernelGGL(boundary_rows_kernel, dim3(gx, ny), dim3(BND_TPB), 0, as_stream(stream), out + o,
                       sel ? sel + o : nullptr, target + o, d2_target + o, d2_pred + o, hw, t_out, t_sel, tol_sq,
                       rows + (int64_t)i0 * 6);
  });
  return check_launch("boundary_rows");
}

}  // extern "C"
