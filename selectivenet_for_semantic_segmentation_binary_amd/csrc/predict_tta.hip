// Flip and D4 test-time augmentation around whole-image prediction. Member k of the
// ensemble is predict_image of T_k(image) mapped back by T_k^-1; bit 2 of k transposes, bit 1 flips the
// rows, bit 0 the columns. The image is transposed once (selunet_image_transpose), so members 4..7 are flips
// of the transposed image and the per-tile kernels only flip:
//
//  * selunet_tile_gather_flip: selunet_tile_gather of the flipped image, without forming it: the flip is
//    applied to the source index after the reflect fold.
//  * selunet_tta_accumulate: the cores of a batch of member tiles, flipped back, added to the running fp32
//    sums of the member's orientation class and, thresholded, to its vote planes.
//  * selunet_tta_finalize: the mean of the K members from the sums of the two classes (the transposed class
//    read through an LDS tile), then mask, prob8, votes and counts by tile_stitch_kernel's rules.
//
// Members run one after another on one stream and every sum pixel is touched by one thread per member,
// without atomics: the order of the additions is fixed and the result bit-reproducible.
#include <algorithm>

#include "common.h"
#include "predict_common.h"
#include "prep_pixel.h"

namespace selunet {

// tile_gather_kernel (predict_io.hip) with a flip: source row fy ? h - 1 - refl(y) : refl(y), column alike.
// A group of four unfolded source pixels is still one 12-B load: under a column flip it starts at the
// group's last pixel and the four results are stored in reverse.
template <int CIN, bool HRGB>
__global__ void tile_gather_flip_kernel(const uint8_t* __restrict__ img, int h, int w,
                                        const int32_t* __restrict__ origins, int n, int th, int tw, int flip,
                                        float* __restrict__ x) {
  const bool fy = flip & 2, fx = flip & 1;
  const int wq = tw >> 2;
  const int64_t total = (int64_t)n * th * wq;
  const int64_t plane = (int64_t)th * tw;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int xq = (int)(i % wq);
    const int64_t r = i / wq;
    const int y = (int)(r % th);
    const int t = (int)(r / th);
    const int64_t y0 = origins[2 * t], x0 = origins[2 * t + 1];
    const int ys = reflect_index(y0 + y, h);
    const int64_t src_row = (int64_t)(fy ? h - 1 - ys : ys) * w;
    const int64_t xs0 = x0 + xq * 4;
    // px[j]: the pixel of output column (fx ? 3 - j : j), i.e. in memory order; the order is put right at the store
    uint8_t px[4][3];
    if (xs0 >= 0 && xs0 + 3 < w) {
      rgb4 raw;
      __builtin_memcpy(&raw, img + (src_row + (fx ? w - 4 - xs0 : xs0)) * 3, 12);
#pragma unroll
      for (int k = 0; k < 12; ++k) px[k / 3][k % 3] = (uint8_t)(raw.w[k >> 2] >> (8 * (k & 3)));
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int xs = reflect_index(xs0 + (fx ? 3 - j : j), w);
        const uint8_t* p = img + (src_row + (fx ? w - 1 - xs : xs)) * 3;
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
      *reinterpret_cast<f32x4*>(x + ((int64_t)t * CIN + c) * plane + o) =
          fx ? f32x4{xv[c][3], xv[c][2], xv[c][1], xv[c][0]} : f32x4{xv[c][0], xv[c][1], xv[c][2], xv[c][3]};
  }
}

// uint8 RGB [h][w][3] -> [w][h][3] through an LDS tile of TR_TILE x TR_TILE pixels. Rows are 3 w (3 h)
// bytes, aligned to nothing, so both sides move bytes: consecutive threads take consecutive bytes of a
// tile row (192 contiguous bytes) on the way in and of a transposed row on the way out. LDS rows are padded
// to 49 dwords (odd), so the column walk of the way out meets every bank once.
constexpr int TR_TILE = 64;
constexpr int TR_ROW = TR_TILE * 3 + 4;

__global__ __launch_bounds__(PRED_TPB) void image_transpose_kernel(const uint8_t* __restrict__ src, int h, int w,
                                                                   uint8_t* __restrict__ dst) {
  __shared__ uint8_t tile[TR_TILE][TR_ROW];
  const int64_t y0 = (int64_t)blockIdx.y * TR_TILE, x0 = (int64_t)blockIdx.x * TR_TILE;
  const int rows = (int)std::min<int64_t>(TR_TILE, h - y0), cols = (int)std::min<int64_t>(TR_TILE, w - x0);
  for (int i = threadIdx.x; i < TR_TILE * TR_TILE * 3; i += PRED_TPB) {
    const int r = i / (TR_TILE * 3), b = i % (TR_TILE * 3);
    if (r < rows && b < cols * 3) tile[r][b] = src[((y0 + r) * w + x0) * 3 + b];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TR_TILE * TR_TILE * 3; i += PRED_TPB) {
    const int c = i / (TR_TILE * 3), b = i % (TR_TILE * 3);  // transposed row c, byte b = 3 r + channel
    if (c < cols && b < rows * 3) dst[((x0 + c) * h + y0) * 3 + b] = tile[b / 3][c * 3 + b % 3];
  }
}

// One thread per (tile, core row, 8-pixel group of the sums' row). The core's pixels inside the member's
// h x w image, columns [c_lo, c_hi) of canvas row cy, go to row (fy ? h - 1 - cy : cy), columns
// [d0, d1) = fx ? [w - c_hi, w - c_lo) : [c_lo, c_hi) of the sums, in reverse under fx. With w % 8 != 0 a
// flipped core does not start on a group boundary, so a core meets up to cw / 8 + 1 groups: a group it
// covers whole is one aligned 2 x 16-B read-modify-write per fp32 plane and 8 B per vote plane, fed by
// 32 B of the tile at dword alignment; a group it covers in part belongs to two cores, so its pixels
// are updated one by one and the neighbour's stay untouched. `first` stores instead of adding (member 0
// and 4: the sums start as the member itself, not as +0 + member, which would lose the sign of a -0).
__global__ __launch_bounds__(PRED_TPB) void tta_accumulate_kernel(
    const float* __restrict__ out, const float* __restrict__ sel, const int32_t* __restrict__ origins, int n, int th,
    int tw, int halo, int flip, int first, int h, int w, int ws, float t_out, float t_sel, float* __restrict__ sum_out,
    float* __restrict__ sum_sel, uint8_t* __restrict__ votes, uint8_t* __restrict__ sel_votes) {
  const bool fy = flip & 2, fx = flip & 1;
  const int ch = th - 2 * halo, cw = tw - 2 * halo, groups = (cw >> 3) + 1;
  const int64_t total = (int64_t)n * ch * groups;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int g = (int)(i % groups);
    const int64_t r = i / groups;
    const int y = (int)(r % ch);
    const int t = (int)(r / ch);
    const int64_t cy = (int64_t)origins[2 * t] + halo + y;
    const int64_t cx0 = (int64_t)origins[2 * t + 1] + halo;
    if (cy < 0 || cy >= h) continue;
    const int64_t c_lo = std::max<int64_t>(cx0, 0), c_hi = std::min<int64_t>(cx0 + cw, w);
    if (c_lo >= c_hi) continue;
    const int64_t d0 = fx ? w - c_hi : c_lo, d1 = fx ? w - c_lo : c_hi;
    const int64_t gx = (d0 & ~(int64_t)7) + 8 * g;
    if (gx >= d1) continue;
    const int64_t dst = (fy ? h - 1 - cy : cy) * ws + gx;
    // tile element of canvas column cx: src + cx
    const int64_t src = ((int64_t)t * th + halo + y) * tw + halo - cx0;
    if (gx >= d0 && gx + 8 <= d1) {
      const int64_t s0 = src + (fx ? w - 8 - gx : gx);
      float o[8], s[8];
      __builtin_memcpy(o, out + s0, 32);
      if (sel) __builtin_memcpy(s, sel + s0, 32);
      f32x4 a0 = {0, 0, 0, 0}, a1 = a0, b0 = a0, b1 = a0;
      u32x2 v = {0, 0}, sv = {0, 0};
      if (!first) {
        a0 = *reinterpret_cast<const f32x4*>(sum_out + dst);
        a1 = *reinterpret_cast<const f32x4*>(sum_out + dst + 4);
        v = *reinterpret_cast<const u32x2*>(votes + dst);
        if (sel) {
          b0 = *reinterpret_cast<const f32x4*>(sum_sel + dst);
          b1 = *reinterpret_cast<const f32x4*>(sum_sel + dst + 4);
          sv = *reinterpret_cast<const u32x2*>(sel_votes + dst);
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float oj = o[fx ? 7 - j : j];
        // `first`: the member itself (0 + m would turn a -0 into +0)
        if (j < 4) a0[j & 3] = first ? oj : a0[j & 3] + oj;
        else a1[j & 3] = first ? oj : a1[j & 3] + oj;
        v[j >> 2] += (uint32_t)(oj >= t_out) << (8 * (j & 3));  // at most 4 votes per byte: no carry
        if (sel) {
          const float sj = s[fx ? 7 - j : j];
          if (j < 4) b0[j & 3] = first ? sj : b0[j & 3] + sj;
          else b1[j & 3] = first ? sj : b1[j & 3] + sj;
          sv[j >> 2] += (uint32_t)(sj >= t_sel) << (8 * (j & 3));
        }
      }
      *reinterpret_cast<f32x4*>(sum_out + dst) = a0;
      *reinterpret_cast<f32x4*>(sum_out + dst + 4) = a1;
      *reinterpret_cast<u32x2*>(votes + dst) = v;
      if (sel) {
        *reinterpret_cast<f32x4*>(sum_sel + dst) = b0;
        *reinterpret_cast<f32x4*>(sum_sel + dst + 4) = b1;
        *reinterpret_cast<u32x2*>(sel_votes + dst) = sv;
      }
    } else {
      const int j0 = (int)std::max<int64_t>(d0 - gx, 0), j1 = (int)std::min<int64_t>(d1 - gx, 8);
      for (int j = j0; j < j1; ++j) {
        const int64_t cx = fx ? w - 1 - (gx + j) : gx + j;
        const float oj = out[src + cx];
        sum_out[dst + j] = first ? oj : sum_out[dst + j] + oj;
        votes[dst + j] = (uint8_t)((first ? 0 : votes[dst + j]) + (oj >= t_out));
        if (sel) {
          const float sj = sel[src + cx];
          sum_sel[dst + j] = first ? sj : sum_sel[dst + j] + sj;
          sel_votes[dst + j] = (uint8_t)((first ? 0 : sel_votes[dst + j]) + (sj >= t_sel));
        }
      }
    }
  }
}

// One workgroup per FIN_TILE x FIN_TILE pixels, one thread per 4 pixels of a row (16 B of each fp32 plane,
// 4 B of each byte plane, aligned: the row stride wa is a multiple of 8). For K = 8 the transposed class
// B [w][hb] is read along its rows (128 contiguous bytes per fp32 row of the tile) into LDS and taken out
// along the columns; fp32 rows are padded to 33 dwords, so both the row-wise stores and the column-wise
// loads of a half-wave meet 32 different banks.
// mean = A * 0.25 (K = 4) or (A + B^T) * 0.125 (K = 8); votes = votes_A + votes_B^T.
constexpr int FIN_TILE = 32;

__global__ __launch_bounds__(PRED_TPB) void tta_finalize_kernel(
    const float* __restrict__ a_out, const float* __restrict__ a_sel, const uint8_t* __restrict__ a_votes,
    const uint8_t* __restrict__ a_sel_votes, const float* __restrict__ b_out, const float* __restrict__ b_sel,
    const uint8_t* __restrict__ b_votes, const uint8_t* __restrict__ b_sel_votes, int members, int h, int w, int wa,
    int hb, float t_out, float t_sel, float* __restrict__ logit_plane, float* __restrict__ sel_plane,
    uint8_t* __restrict__ mask, uint8_t* __restrict__ prob8, uint8_t* __restrict__ votes,
    uint8_t* __restrict__ sel_votes, unsigned long long* __restrict__ counts) {
  __shared__ float tb[2][FIN_TILE][FIN_TILE + 1];
  __shared__ __attribute__((aligned(16))) uint8_t vb[2][FIN_TILE][FIN_TILE + 4];
  const bool selective = a_sel != nullptr, d4 = members == 8;
  const int64_t y0 = (int64_t)blockIdx.y * FIN_TILE, x0 = (int64_t)blockIdx.x * FIN_TILE;
  const int ty = threadIdx.x >> 3, tx = (threadIdx.x & 7) * 4;
  if (d4) {
    // row x0 + ty of B, columns y0 + tx .. + 3: inside B's rows when the column starts below hb (hb % 4 == 0)
    f32x4 o = {0, 0, 0, 0}, s = o;
    uint32_t v = 0, sv = 0;
    if (x0 + ty < w && y0 + tx < hb) {
      const int64_t at = (x0 + ty) * hb + y0 + tx;
      o = *reinterpret_cast<const f32x4*>(b_out + at);
      v = *reinterpret_cast<const uint32_t*>(b_votes + at);
      if (selective) {
        s = *reinterpret_cast<const f32x4*>(b_sel + at);
        sv = *reinterpret_cast<const uint32_t*>(b_sel_votes + at);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      tb[0][ty][tx + j] = o[j];
      tb[1][ty][tx + j] = s[j];
    }
    *reinterpret_cast<uint32_t*>(&vb[0][ty][tx]) = v;
    *reinterpret_cast<uint32_t*>(&vb[1][ty][tx]) = sv;
    __syncthreads();
  }
  unsigned c[3] = {0, 0, 0};
  const int64_t yy = y0 + ty, xx = x0 + tx;
  if (yy < h && xx < wa) {  // wa % 4 == 0: the four pixels lie inside the row
    const int64_t at = yy * wa + xx;
    const float scale = d4 ? 0.125f : 0.25f;
    f32x4 o = *reinterpret_cast<const f32x4*>(a_out + at), s = {0, 0, 0, 0};
    uint32_t v = *reinterpret_cast<const uint32_t*>(a_votes + at), sv = 0;
    if (selective) {
      s = *reinterpret_cast<const f32x4*>(a_sel + at);
      sv = *reinterpret_cast<const uint32_t*>(a_sel_votes + at);
    }
    uint32_t m = 0, p = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (d4) {
        o[j] += tb[0][tx + j][ty];
        s[j] += tb[1][tx + j][ty];
        v += (uint32_t)vb[0][tx + j][ty] << (8 * j);  // at most 4 + 4 votes per byte: no carry
        sv += (uint32_t)vb[1][tx + j][ty] << (8 * j);
      }
      o[j] *= scale;
      s[j] *= scale;
      const int cls = pixel_class(selective, s[j], o[j], t_sel, t_out);
      m |= mask_level(cls) << (8 * j);
      if (prob8) p |= prob_level(o[j]) << (8 * j);
      const bool counted = xx + j < w;
#pragma unroll
      for (int k = 0; k < 3; ++k) c[k] += counted && cls == k;
    }
    *reinterpret_cast<f32x4*>(logit_plane + at) = o;
    *reinterpret_cast<uint32_t*>(mask + at) = m;
    *reinterpret_cast<uint32_t*>(votes + at) = v;
    if (prob8) *reinterpret_cast<uint32_t*>(prob8 + at) = p;
    if (selective) {
      *reinterpret_cast<f32x4*>(sel_plane + at) = s;
      *reinterpret_cast<uint32_t*>(sel_votes + at) = sv;
    }
  }
  add_class_counts(c, counts);
}

}  // namespace selunet

using namespace selunet;

extern "C" {

int selunet_tile_gather_flip(const uint8_t* img, int32_t h, int32_t w, const int32_t* origins, int32_t n, int32_t th,
                             int32_t tw, int32_t mode, int32_t flip, float* x, void* stream) {
  SELUNET_REQUIRE(img && x, "tile_gather_flip: null img or x");
  if (int rc = tile_args("tile_gather_flip", origins, n, h, w, th, tw)) return rc;
  SELUNET_REQUIRE(mode >= 0 && mode <= 2, "tile_gather_flip: mode 0 'RGB', 1 'GH', 2 'H_RGB' (got %d)", mode);
  SELUNET_REQUIRE(flip >= 0 && flip <= 3, "tile_gather_flip: flip must be in [0, 3]: bit 1 rows, bit 0 columns (got %d)",
                  flip);
  SELUNET_REQUIRE(aligned(15, x), "tile_gather_flip: x must be 16-B aligned");
  const int64_t total = (int64_t)n * th * (tw / 4);
  const dim3 grid((unsigned)io_grid(cdiv(total, PRED_TPB), 8192));
  auto kernel = mode == 0 ? tile_gather_flip_kernel<3, false> : mode == 1 ? tile_gather_flip_kernel<2, false>
                                                                          : tile_gather_flip_kernel<3, true>;
  hipLaunchKernelGGL(kernel, grid, dim3(PRED_TPB), 0, as_stream(stream), img, h, w, origins, n, th, tw, flip, x);
  return check_launch("tile_gather_flip");
}

int selunet_image_transpose(const uint8_t* src, int32_t h, int32_t w, uint8_t* dst, void* stream) {
  SELUNET_REQUIRE(src && dst, "image_transpose: null src or dst");
  SELUNET_REQUIRE(src != dst, "image_transpose: src and dst must differ (not in place)");
  SELUNET_REQUIRE(h >= 1 && h <= PRED_MAX_HW && w >= 1 && w <= PRED_MAX_HW,
                  "image_transpose: image height and width must be in [1, %d] (got %d x %d)", PRED_MAX_HW, h, w);
  const dim3 grid((unsigned)cdiv(w, TR_TILE), (unsigned)cdiv(h, TR_TILE));
  hipLaunchKernelGGL(image_transpose_kernel, grid, dim3(PRED_TPB), 0, as_stream(stream), src, h, w, dst);
  return check_launch("image_transpose");
}

int selunet_tta_accumulate(const float* out, const float* sel, const int32_t* origins, int32_t n, int32_t th,
                           int32_t tw, int32_t halo, int32_t flip, int32_t first, int32_t h, int32_t w, int32_t ws,
                           float t_out, float t_sel, float* sum_out, float* sum_sel, uint8_t* votes,
                           uint8_t* sel_votes, void* stream) {
  SELUNET_REQUIRE(out && sum_out && votes, "tta_accumulate: null out, sum_out or votes");
  SELUNET_REQUIRE((sel == nullptr) == (sum_sel == nullptr) && (sel == nullptr) == (sel_votes == nullptr),
                  "tta_accumulate: sel, sum_sel and sel_votes must all be given or all be null");
  if (int rc = tile_args("tta_accumulate", origins, n, h, w, th, tw)) return rc;
  SELUNET_REQUIRE(halo >= 0 && halo % 8 == 0 && 2 * (int64_t)halo < std::min(th, tw),
                  "tta_accumulate: halo must be a multiple of 8 with 2 * halo < min(th, tw) (got %d for %d x %d)", halo,
                  th, tw);
  SELUNET_REQUIRE(flip >= 0 && flip <= 3, "tta_accumulate: flip must be in [0, 3]: bit 1 rows, bit 0 columns (got %d)",
                  flip);
  SELUNET_REQUIRE(first == 0 || first == 1, "tta_accumulate: first must be 0 or 1 (got %d)", first);
  SELUNET_REQUIRE(ws >= w && ws % 8 == 0,
                  "tta_accumulate: the sums' row stride must hold the image and be a multiple of 8 (got %d for width %d)",
                  ws, w);
  SELUNET_REQUIRE(aligned(15, out, sel, sum_out, sum_sel, votes, sel_votes),
                  "tta_accumulate: tiles and planes must be 16-B aligned");
  const int64_t total = (int64_t)n * (th - 2 * halo) * ((tw - 2 * halo) / 8 + 1);
  const int64_t blocks = io_grid(cdiv(total, PRED_TPB), 8192);
  hipLaunchKernelGGL(tta_accumulate_kernel, dim3((unsigned)blocks), dim3(PRED_TPB), 0, as_stream(stream), out, sel,
                     origins, n, th, tw, halo, flip, first, h, w, ws, t_out, t_sel, sum_out, sum_sel, votes, sel_votes);
  return check_launch("tta_accumulate");
}

int selunet_tta_finalize(const float* a_out, const float* a_sel, const uint8_t* a_votes, const uint8_t* a_sel_votes,
                         const float* b_out, const float* b_sel, const uint8_t* b_votes, const uint8_t* b_sel_votes,
                         int32_t members, int32_t h, int32_t w, int32_t wa, int32_t hb, float t_out, float t_sel,
                         float* logit_plane, float* sel_plane, uint8_t* mask, uint8_t* prob8, uint8_t* votes,
                         uint8_t* sel_votes, unsigned long long* counts, void* stream) {
  SELUNET_REQUIRE(members == 4 || members == 8, "tta_finalize: members must be 4 ('flips') or 8 ('d4') (got %d)",
                  members);
  SELUNET_REQUIRE(a_out && a_votes && logit_plane && mask && votes && counts,
                  "tta_finalize: null a_out, a_votes, logit_plane, mask, votes or counts");
  const bool selective = a_sel != nullptr;
  SELUNET_REQUIRE(selective == (a_sel_votes != nullptr) && selective == (sel_plane != nullptr) &&
                      selective == (sel_votes != nullptr),
                  "tta_finalize: a_sel, a_sel_votes, sel_plane and sel_votes must all be given or all be null");
  if (members == 8)
    SELUNET_REQUIRE(b_out && b_votes && selective == (b_sel != nullptr) && selective == (b_sel_votes != nullptr),
                    "tta_finalize: 8 members need b_out and b_votes, and b_sel and b_sel_votes exactly with a_sel");
  else
    SELUNET_REQUIRE(!b_out && !b_sel && !b_votes && !b_sel_votes,
                    "tta_finalize: 4 members have no transposed class: b_out, b_sel, b_votes, b_sel_votes must be null");
  SELUNET_REQUIRE(h >= 1 && h <= PRED_MAX_HW && w >= 1 && w <= PRED_MAX_HW,
                  "tta_finalize: image height and width must be in [1, %d] (got %d x %d)", PRED_MAX_HW, h, w);
  SELUNET_REQUIRE(wa >= w && wa % 8 == 0,
                  "tta_finalize: the row stride wa must hold the width and be a multiple of 8 (got %d for %d)", wa, w);
  SELUNET_REQUIRE(members == 4 || (hb >= h && hb % 8 == 0),
                  "tta_finalize: the transposed row stride hb must hold the height and be a multiple of 8 (got %d for %d)",
                  hb, h);
  SELUNET_REQUIRE(aligned(15, a_out, a_sel, a_votes, a_sel_votes, b_out, b_sel, b_votes, b_sel_votes, logit_plane,
                          sel_plane, mask, prob8, votes, sel_votes), "tta_finalize: planes must be 16-B aligned");
  SELUNET_REQUIRE(aligned(7, counts), "tta_finalize: counts must be 8-B aligned");
  const dim3 grid((unsigned)cdiv(wa, FIN_TILE), (unsigned)cdiv(h, FIN_TILE));
  hipLaunchKernelGGL(tta_finalize_kernel, grid, dim3(PRED_TPB), 0, as_stream(stream), a_out, a_sel, a_votes,
                     a_sel_votes, b_out, b_sel, b_votes, b_sel_votes, members, h, w, wa, hb, t_out, t_sel, logit_plane,
                     sel_plane, mask, prob8, votes, sel_votes, counts);
  return check_launch("tta_finalize");
}

}  // extern "C"
