// The tissue mask of whole-image prediction: which pixels of the image are bare glass, how
// many tissue pixels each tile's input window holds, and the mask's pixel counts over the tissue alone.
//
//  * selunet_tissue_plane: RGB uint8 -> a uint8 plane, 255 tissue / 0 glass, by an exact integer rule:
//    glass iff min(r,g,b) >= bright and max(r,g,b) - min(r,g,b) <= spread.
//  * selunet_tile_tissue_counts: per tile the number of tissue positions of the window that
//    selunet_tile_gather_flip would gather (the flipped plane continued by reflection: a reflected copy
//    counts again). A few workgroups per tile, each finishing with one integer atomic.
//  * selunet_tissue_class_counts: {background, tumor, abstained, pixels} of a 0 / 255 / 127 mask over the
//    tissue pixels, by the stitch kernel's reduction (add_class_counts).
//
// All three are integer arithmetic on bytes: every result is the same bit for bit on every run.
#include <algorithm>

#include "common.h"
#include "predict_common.h"

namespace selunet {

// One thread per (row, 4-pixel group of the padded row): 12 B of RGB in, one aligned word out. A group
// inside the row reads its 12 B in one load at whatever alignment the pixel has (rows are 3 w bytes); the
// row's last group reads its pixels one by one and writes 0 for the bytes beyond w.
__global__ __launch_bounds__(PRED_TPB) void tissue_plane_kernel(const uint8_t* __restrict__ img, int h, int w,
                                                                int bright, int spread, uint8_t* __restrict__ plane,
                                                                int pitch) {
  const int gq = pitch >> 2;
  const int64_t total = (int64_t)h * gq;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / gq), x = (int)(i % gq) * 4;
    const int n = std::max(0, std::min(4, w - x));
    const uint8_t* p = img + ((int64_t)y * w + x) * 3;
    uint8_t px[4][3] = {};
    if (n == 4) {
      rgb4 raw;
      __builtin_memcpy(&raw, p, 12);
#pragma unroll
      for (int k = 0; k < 12; ++k) px[k / 3][k % 3] = (uint8_t)(raw.w[k >> 2] >> (8 * (k & 3)));
    } else {
      for (int j = 0; j < n; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) px[j][c] = p[3 * j + c];
    }
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int lo = std::min((int)px[j][0], std::min((int)px[j][1], (int)px[j][2]));
      const int hi = std::max((int)px[j][0], std::max((int)px[j][1], (int)px[j][2]));
      const bool glass = lo >= bright && hi - lo <= spread;
      if (j < n && !glass) word |= 255u << (8 * j);
    }
    *reinterpret_cast<uint32_t*>(plane + (int64_t)y * pitch + x) = word;
  }
}

// Workgroup (t, s) counts slab s of tile t's window, gridDim.y slabs of whole rows: one thread per (window
// row, 4 columns). Four unfolded source columns are one 4-B load at byte alignment (under a column flip it
// starts at the group's last pixel; the order does not matter to a count); a group that crosses an edge
// folds each column on its own. A byte other than 0 is tissue. Per thread in a register, per wave by
// shuffles, per workgroup through LDS, then one integer atomic per workgroup. (One workgroup per tile, with
// a plain store, took 0.54 ms for the 121 windows of 512 x 512 of a 4096 x 4096 image: 1024 dependent
// iterations per thread on less than half of the CUs.)
constexpr int TISSUE_SLAB_ROWS = 32;

__global__ __launch_bounds__(PRED_TPB) void tile_tissue_counts_kernel(const uint8_t* __restrict__ plane, int64_t pitch,
                                                                      int h, int w, const int32_t* __restrict__ origins,
                                                                      int th, int tw, int flip,
                                                                      int32_t* __restrict__ counts) {
  const bool fy = flip & 2, fx = flip & 1;
  const int t = blockIdx.x;
  const int64_t y0 = origins[2 * t], x0 = origins[2 * t + 1];
  const int wq = tw >> 2;
  const int rows = (th + (int)gridDim.y - 1) / (int)gridDim.y;
  const int y_lo = std::min(th, (int)blockIdx.y * rows), y_hi = std::min(th, y_lo + rows);
  const int total = (y_hi - y_lo) * wq;  // th * tw < 2^31
  unsigned c[1] = {0};
  for (int i = threadIdx.x; i < total; i += PRED_TPB) {
    const int y = y_lo + i / wq, xq = i % wq;
    const int ys = reflect_index(y0 + y, h);
    const uint8_t* row = plane + (int64_t)(fy ? h - 1 - ys : ys) * pitch;
    const int64_t xs0 = x0 + xq * 4;
    if (xs0 >= 0 && xs0 + 3 < w) {
      uint32_t v;
      __builtin_memcpy(&v, row + (fx ? w - 4 - xs0 : xs0), 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) c[0] += ((v >> (8 * j)) & 255u) != 0u;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int xs = reflect_index(xs0 + j, w);
        c[0] += row[fx ? w - 1 - xs : xs] != 0;
      }
    }
  }
  const unsigned long long s = block_sum<1, PRED_TPB>(c);  // < 2^31: th * tw
  if (threadIdx.x == 0 && s) atomicAdd(counts + t, (int32_t)s);
}

// One thread per 4 pixels of a row, an aligned 4-B load of either plane where its row's address allows it
// (regions_apply_kernel's access). A mask byte other than 0 / 255 / 127 is in no class.
__device__ __forceinline__ uint32_t load_bytes(const uint8_t* p, int n) {
  if (n == 4 && ((uintptr_t)p & 3) == 0) return *reinterpret_cast<const uint32_t*>(p);
  uint32_t m = 0;
  for (int j = 0; j < n; ++j) m |= (uint32_t)p[j] << (8 * j);
  return m;
}

__global__ __launch_bounds__(PRED_TPB) void tissue_class_counts_kernel(const uint8_t* __restrict__ mask,
                                                                       int64_t mask_pitch,
                                                                       const uint8_t* __restrict__ plane, int64_t pitch,
                                                                       int h, int w,
                                                                       unsigned long long* __restrict__ counts) {
  const int gq = (w + 3) >> 2;
  const int64_t total = (int64_t)h * gq;
  unsigned c[3] = {0, 0, 0};
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / gq), x = (int)(i % gq) * 4;
    const int n = std::min(4, w - x);
    const uint32_t m = load_bytes(mask + (int64_t)y * mask_pitch + x, n);
    const uint32_t q = load_bytes(plane + (int64_t)y * pitch + x, n);
    for (int j = 0; j < n; ++j) {
      const uint32_t v = (m >> (8 * j)) & 255u;
      const bool tissue = ((q >> (8 * j)) & 255u) != 0u;
      c[0] += tissue && v == 0u;
      c[1] += tissue && v == 255u;
      c[2] += tissue && v == 127u;
    }
  }
  add_class_counts(c, counts);
}

}  // namespace selunet

using namespace selunet;

extern "C" {

int selunet_tissue_plane(const uint8_t* img, int32_t h, int32_t w, int32_t bright, int32_t spread, uint8_t* plane,
                         int32_t pitch, void* stream) {
  SELUNET_REQUIRE(img && plane, "tissue_plane: null img or plane");
  SELUNET_REQUIRE(h >= 1 && h <= PRED_MAX_HW && w >= 1 && w <= PRED_MAX_HW,
                  "tissue_plane: image height and width must be in [1, %d] (got %d x %d)", PRED_MAX_HW, h, w);
  SELUNET_REQUIRE(bright >= 0 && bright <= 255 && spread >= 0 && spread <= 255,
                  "tissue_plane: bright and spread must be in [0, 255] (got %d, %d)", bright, spread);
  SELUNET_REQUIRE(pitch >= w && pitch % 4 == 0,
                  "tissue_plane: the plane's row pitch must hold the width and be a multiple of 4 (got %d for %d)", pitch,
                  w);
  SELUNET_REQUIRE(aligned(3, plane), "tissue_plane: plane must be 4-B aligned");
  const int64_t total = (int64_t)h * (pitch / 4);
  const int64_t blocks = io_grid(cdiv(total, PRED_TPB), 8192);
  hipLaunchKernelGGL(tissue_plane_kernel, dim3((unsigned)blocks), dim3(PRED_TPB), 0, as_stream(stream), img, h, w,
                     bright, spread, plane, pitch);
  return check_launch("tissue_plane");
}

int selunet_tile_tissue_counts(const uint8_t* plane, int64_t pitch, int32_t h, int32_t w, const int32_t* origins,
                               int32_t n, int32_t th, int32_t tw, int32_t flip, int32_t* counts, void* stream) {
  SELUNET_REQUIRE(plane && counts, "tile_tissue_counts: null plane or counts");
  if (int rc = tile_args("tile_tissue_counts", origins, n, h, w, th, tw)) return rc;
  SELUNET_REQUIRE(pitch >= w, "tile_tissue_counts: the plane's row pitch must hold the width (got %lld for %d)",
                  (long long)pitch, w);
  SELUNET_REQUIRE(flip >= 0 && flip <= 3,
                  "tile_tissue_counts: flip must be in [0, 3]: bit 1 rows, bit 0 columns (got %d)", flip);
  SELUNET_REQUIRE((int64_t)th * tw < ((int64_t)1 << 31),
                  "tile_tissue_counts: a window of %d x %d positions does not fit a 32-bit count", th, tw);
  SELUNET_REQUIRE(aligned(3, counts), "tile_tissue_counts: counts must be 4-B aligned");
  const unsigned slabs = (unsigned)std::min<int64_t>(cdiv(th, TISSUE_SLAB_ROWS), 1024);
  hipLaunchKernelGGL(tile_tissue_counts_kernel, dim3((unsigned)n, slabs), dim3(PRED_TPB), 0, as_stream(stream), plane,
                     pitch, h, w, origins, th, tw, flip, counts);
  return check_launch("tile_tissue_counts");
}

int selunet_tissue_class_counts(const uint8_t* mask, int64_t mask_pitch, const uint8_t* plane, int64_t pitch,
                                int32_t h, int32_t w, unsigned long long* counts, void* stream) {
  SELUNET_REQUIRE(mask && plane && counts, "tissue_class_counts: null mask, plane or counts");
  SELUNET_REQUIRE(h >= 1 && h <= PRED_MAX_HW && w >= 1 && w <= PRED_MAX_HW,
                  "tissue_class_counts: image height and width must be in [1, %d] (got %d x %d)", PRED_MAX_HW, h, w);
  SELUNET_REQUIRE(mask_pitch >= w && pitch >= w,
                  "tissue_class_counts: the row pitches of mask and plane must hold the width %d (got %lld, %lld)", w,
                  (long long)mask_pitch, (long long)pitch);
  SELUNET_REQUIRE(aligned(7, counts), "tissue_class_counts: counts must be 8-B aligned");
  // the per-thread and per-wave partial counts are 32 bits wide; H W < 2^32 by the bound above
  const int64_t total = (int64_t)h * ((w + 3) / 4);
  const int64_t blocks = io_grid(cdiv(total, PRED_TPB), 2048);
  hipLaunchKernelGGL(tissue_class_counts_kernel, dim3((unsigned)blocks), dim3(PRED_TPB), 0, as_stream(stream), mask,
                     mask_pitch, plane, pitch, h, w, counts);
  return check_launch("tissue_class_counts");
}

}  // extern "C"
