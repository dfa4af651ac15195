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
#include "predict_common.h"
#include "prep_pixel.h"

namespace selunet {

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
      const int cls = pixel_class(sel != nullptr, s, o, t_sel, t_out);
      const uint32_t level = mask_level(cls);
      m[j >> 2] |= level << (8 * (j & 3));
      if (prob8) p[j >> 2] |= prob_level(o) << (8 * (j & 3));
      const bool counted = cy < h && cx + j < w;
#pragma unroll
      for (int k = 0; k < 3; ++k) c[k] += counted && cls == k;
    }
    *reinterpret_cast<u32x2*>(mask + dst) = m;
    if (prob8) *reinterpret_cast<u32x2*>(prob8 + dst) = p;
  }
  add_class_counts(c, counts);
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
  const dim3 grid((unsigned)io_grid(cdiv(total, PRED_TPB), 8192));
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
  const int64_t blocks = io_grid(cdiv(total, PRED_TPB), 2048);
  hipLaunchKernelGGL(tile_stitch_kernel, dim3((unsigned)blocks), dim3(PRED_TPB), 0, as_stream(stream), out, sel, origins,
                     n, th, tw, halo, h, w, hc, wc, t_out, t_sel, logit_plane, sel_plane, mask, prob8, counts);
  return check_launch("tile_stitch");
}

}  // extern "C"
