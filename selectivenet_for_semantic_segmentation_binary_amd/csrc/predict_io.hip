// Whole-image prediction I/O around the eval-mode forward:
//
//  * selunet_tile_gather: an RGB uint8 image on the device -> a batch of overlapping network-input tiles
//    (NCHW fp32, selunet_prep_batch_mode's per-pixel conversion), the image continued past its edges by
//    reflection (numpy's 'reflect' padding), so that every tile is a full tile whatever the image size.
//  * selunet_tile_stitch: the cores (tile minus halo) of a batch of output tiles -> the logit canvases, the
//    uint8 mask {0 background, 127 abstained, 255 tumor}, the uint8 probability map and the pixel counts.
//
// Both are pure data movement in one pass with 16-B stores and 64-bit index arithmetic; beside the forward
// of the same batch they are bound by their launch.
#include <algorithm>

#include "common.h"
#include "prep_pixel.h"

namespace selunet {

constexpr int PRED_TPB = 256;
constexpr int PRED_MAX_HW = 65535;  // image height / width the calls take

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

// One thread per (tile, row, 4-pixel group): 12 B of RGB in, CIN x 16 B of NCHW planes out. A group whose
// four source pixels lie inside the row (no fold) reads them as one 12-B load at whatever byte alignment
// the pixel has (rows are w * 3 bytes: no alignment to rely on); a group that crosses an edge folds each
// pixel's column on its own.
template <int CIN, bool HRGB>
__global__ void tile_gather_kernel(const uint8_t* __restrict__ img, int h, int w, const int32_t* __restrict__ origins,
                                   int n, int th, int tw, float* __restrict__ x) {
  const int wq = tw >> 2;
  const int64_t total = (int64_t)n * th * wq;
  const int64_t plane = (int64_t)th * tw;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int xq = (int)(i % wq);
    const int64_t r = i / wq;
    const int y = (int)(r % th);
    const int t = (int)(r / th);
    const int64_t y0 = origins[2 * t], x0 = origins[2 * t + 1];
    const int64_t src_row = (int64_t)reflect_index(y0 + y, h) * w;
    const int64_t xs0 = x0 + xq * 4;
    uint8_t px[4][3];
    if (xs0 >= 0 && xs0 + 3 < w) {
      rgb4 raw;
      __builtin_memcpy(&raw, img + (src_row + xs0) * 3, 12);
#pragma unroll
      for (int k = 0; k < 12; ++k) px[k / 3][k % 3] = (uint8_t)(raw.w[k >> 2] >> (8 * (k & 3)));
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint8_t* p = img + (src_row + reflect_index(xs0 + j, w)) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) px[j][c] = p[c];
      }
    }
    float xv[CIN][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v[CIN];
      prep_pixel<CIN, HRGB>(px[j][0], px[j][1], px[j][2], v);
#pragma unroll
      for (int c = 0; c < CIN; ++c) xv[c][j] = v[c];
    }
    const int64_t o = (int64_t)y * tw + xq * 4;
#pragma unroll
    for (int c = 0; c < CIN; ++c)
      *reinterpret_cast<f32x4*>(x + ((int64_t)t * CIN + c) * plane + o) = f32x4{xv[c][0], xv[c][1], xv[c][2], xv[c][3]};
  }
}

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// floor(255 sigmoid(v) + 0.5) as a byte; NaN -> 0
__device__ __forceinline__ uint32_t prob_level(float v) {
  const float p = 255.0f * sigmoidf_(v) + 0.5f;
  return p >= 0.0f ? (uint32_t)p : 0u;  // p in [0.5, 255.5]: the conversion truncates = floor; NaN fails the test
}

// One thread per (tile, core row, 8-pixel group): 2 x 16 B of each logit tile in; 2 x 16 B per logit
// canvas and 8 B per byte canvas out. th, tw, halo and the canvas width are multiples of 8 and so is a
// core's canvas column (the caller's duty for the origins: a group that is not, or that does not lie
// inside the canvas, is skipped — neither stored nor counted), so every access is aligned.
// counts += {background, tumor, abstained, pixels} over the canvas pixels with y < h and x < w: per thread
// in registers, per wave by shuffles, per workgroup through LDS, then four integer atomics.
__global__ __launch_bounds__(PRED_TPB) void tile_stitch_kernel(
    const float* __restrict__ out, const float* __restrict__ sel, const int32_t* __restrict__ origins, int n, int th,
    int tw, int halo, int h, int w, int hc, int wc, float t_out, float t_sel, float* __restrict__ logit_plane,
    float* __restrict__ sel_plane, uint8_t* __restrict__ mask, uint8_t* __restrict__ prob8,
    unsigned long long* __restrict__ counts) {
  const int ch = th - 2 * halo, cw8 = (tw - 2 * halo) >> 3;
  const int64_t total = (int64_t)n * ch * cw8;
  unsigned c[3] = {0, 0, 0};
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int g = (int)(i % cw8);
    const int64_t r = i / cw8;
    const int y = (int)(r % ch);
    const int t = (int)(r / ch);
    const int64_t cy = (int64_t)origins[2 * t] + halo + y;
    const int64_t cx = (int64_t)origins[2 * t + 1] + halo + g * 8;
    if (cy < 0 || cy >= hc || cx < 0 || cx + 8 > wc || (cx & 7)) continue;
    const int64_t src = ((int64_t)t * th + halo + y) * tw + halo + g * 8;
    const int64_t dst = cy * wc + cx;
    const f32x4 o0 = *reinterpret_cast<const f32x4*>(out + src), o1 = *reinterpret_cast<const f32x4*>(out + src + 4);
    *reinterpret_cast<f32x4*>(logit_plane + dst) = o0;
    *reinterpret_cast<f32x4*>(logit_plane + dst + 4) = o1;
    f32x4 s0 = {0, 0, 0, 0}, s1 = {0, 0, 0, 0};
    if (sel) {
      s0 = *reinterpret_cast<const f32x4*>(sel + src);
      s1 = *reinterpret_cast<const f32x4*>(sel + src + 4);
      *reinterpret_cast<f32x4*>(sel_plane + dst) = s0;
      *reinterpret_cast<f32x4*>(sel_plane + dst + 4) = s1;
    }
    u32x2 m = {0, 0}, p = {0, 0};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float o = j < 4 ? o0[j & 3] : o1[j & 3];
      const float s = j < 4 ? s0[j & 3] : s1[j & 3];
      // `not (sel >= t_sel)`: a NaN selection abstains; a NaN output is background (seg_metrics_kernel's rule)
      const int cls = (sel != nullptr && !(s >= t_sel)) ? 2 : (o >= t_out ? 1 : 0);
      const uint32_t level = cls == 2 ? 127u : (cls == 1 ? 255u : 0u);
      m[j >> 2] |= level << (8 * (j & 3));
      if (prob8) p[j >> 2] |= prob_level(o) << (8 * (j & 3));
      const bool counted = cy < h && cx + j < w;
#pragma unroll
      for (int k = 0; k < 3; ++k) c[k] += counted && cls == k;
    }
    *reinterpret_cast<u32x2*>(mask + dst) = m;
    if (prob8) *reinterpret_cast<u32x2*>(prob8 + dst) = p;
  }
  __shared__ unsigned red[PRED_TPB / 64][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    unsigned v = c[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    // words 0..2: the class of this thread; word 3, `pixels`: all three
    unsigned long long s = 0;
    for (int wv = 0; wv < PRED_TPB / 64; ++wv)
      for (int k = 0; k < 3; ++k)
        if (threadIdx.x == 3 || threadIdx.x == k) s += red[wv][k];
    if (s) atomicAdd(counts + threadIdx.x, s);
  }
}

// The argument rules the two calls share; `fn` names the call in the message.
static int tile_args(const char* fn, const int32_t* origins, int32_t n, int32_t h, int32_t w, int32_t th, int32_t tw) {
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

using namespace selunet;

extern "C" {

int selunet_tile_gather(const uint8_t* img, int32_t h, int32_t w, const int32_t* origins, int32_t n, int32_t th,
                        int32_t tw, int32_t mode, float* x, void* stream) {
  SELUNET_REQUIRE(img && x, "tile_gather: null img or x");
  if (int rc = tile_args("tile_gather", origins, n, h, w, th, tw)) return rc;
  SELUNET_REQUIRE(mode >= 0 && mode <= 2, "tile_gather: mode 0 'RGB', 1 'GH', 2 'H_RGB' (got %d)", mode);
  SELUNET_REQUIRE(((uintptr_t)x & 15) == 0, "tile_gather: x must be 16-B aligned");
  const int64_t total = (int64_t)n * th * (tw / 4);
  const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(total, PRED_TPB), 8192)));
  auto kernel = mode == 0 ? tile_gather_kernel<3, false> : mode == 1 ? tile_gather_kernel<2, false>
                                                                     : tile_gather_kernel<3, true>;
  hipLaunchKernelGGL(kernel, grid, dim3(PRED_TPB), 0, as_stream(stream), img, h, w, origins, n, th, tw, x);
  return check_launch("tile_gather");
}

int selunet_tile_stitch(const float* out, const float* sel, const int32_t* origins, int32_t n, int32_t th, int32_t tw,
                        int32_t halo, int32_t h, int32_t w, int32_t hc, int32_t wc, float t_out, float t_sel,
                        float* logit_plane, float* sel_plane, uint8_t* mask, uint8_t* prob8,
                        unsigned long long* counts, void* stream) {
  SELUNET_REQUIRE(out && logit_plane && mask && counts, "tile_stitch: null out, logit_plane, mask or counts");
  SELUNET_REQUIRE((sel == nullptr) == (sel_plane == nullptr),
                  "tile_stitch: sel and sel_plane must both be given or both be null");
  if (int rc = tile_args("tile_stitch", origins, n, h, w, th, tw)) return rc;
  SELUNET_REQUIRE(halo >= 0 && halo % 8 == 0 && 2 * (int64_t)halo < std::min(th, tw),
                  "tile_stitch: halo must be a multiple of 8 with 2 * halo < min(th, tw) (got %d for %d x %d)", halo,
                  th, tw);
  SELUNET_REQUIRE(hc >= h && wc >= w && wc % 8 == 0,
                  "tile_stitch: the canvas must hold the image and its width be a multiple of 8 (got %d x %d for "
                  "%d x %d)", hc, wc, h, w);
  SELUNET_REQUIRE(((uintptr_t)out & 15) == 0 && ((uintptr_t)sel & 15) == 0 && ((uintptr_t)logit_plane & 15) == 0 &&
                      ((uintptr_t)sel_plane & 15) == 0 && ((uintptr_t)mask & 15) == 0 && ((uintptr_t)prob8 & 15) == 0,
                  "tile_stitch: tiles and planes must be 16-B aligned");
  SELUNET_REQUIRE(((uintptr_t)counts & 7) == 0, "tile_stitch: counts must be 8-B aligned");
  // the per-thread and per-wave partial counts are 32 bits wide: no more core pixels than that in one call
  const int64_t total = (int64_t)n * (th - 2 * halo) * ((tw - 2 * halo) / 8);
  SELUNET_REQUIRE(total * 8 < ((int64_t)1 << 32), "tile_stitch: %lld core pixels in one call, at most 2^32 - 1",
                  (long long)total * 8);
  const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(cdiv(total, PRED_TPB), 2048));
  hipLaunchKernelGGL(tile_stitch_kernel, dim3((unsigned)blocks), dim3(PRED_TPB), 0, as_stream(stream), out, sel, origins,
                     n, th, tw, halo, h, w, hc, wc, t_out, t_sel, logit_plane, sel_plane, mask, prob8, counts);
  return check_launch("tile_stitch");
}

}  // extern "C"
