// Macenko stain normalisation of whole-image prediction: the four per-pixel passes over an
// RGB uint8 image. The host does the small linear algebra between them in float64 (stain.py).
//
//  * selunet_stain_moments: {n, sums, second moments} of the Q12 optical densities of the stained pixels.
//  * selunet_stain_angle_hist: the histogram of each stained pixel's angle in the plane of the two leading
//    eigenvectors, K bins over (-pi/2, pi/2), found by integer comparisons against a table of directions.
//  * selunet_stain_conc_hist: per stain the histogram of the stained pixels' concentrations, CB bins of 1/128.
//  * selunet_stain_apply: every pixel re-rendered through a 3 x 3 integer matrix on its optical densities.
//
// Neither log nor exp runs here: optical density is a table of 256 words and the way back a table of bytes,
// both made by the caller. All four are integer arithmetic and integer atomics: every result is the same bit
// for bit on every run, in whatever order the pixels are met.
#include <algorithm>
#include <cstdlib>

#include "common.h"
#include "predict_common.h"

namespace selunet {

constexpr int STAIN_K = SELUNET_STAIN_ANGLE_BINS;
constexpr int STAIN_CB = SELUNET_STAIN_CONC_BINS;
constexpr int STAIN_EXP_MAX = SELUNET_STAIN_EXP_MAX;
static_assert(PRED_TPB == 256, "one thread stages one word of the optical-density table");
static_assert((STAIN_K & (STAIN_K - 1)) == 0, "the angle search halves its step down to 1");

struct stain_mat2 {
  int32_t v[2][3];
};
struct stain_mat3 {
  int32_t v[3][3];
};

// The walk all four kernels share, tissue_plane_kernel's: one item per (row, 4-pixel group), 12 B of RGB in
// one load at whatever alignment the pixel has where the group lies inside the row (rows are 3 w bytes), the
// row's last group pixel by pixel. Returns the group's pixel count n in [1, 4] and its first byte's offset.
__device__ __forceinline__ int load_group(const uint8_t* __restrict__ img, int w, int gq, int64_t i,
                                          uint8_t (&px)[4][3], int64_t& offset) {
  const int y = (int)(i / gq), x = (int)(i % gq) * 4;
  const int n = std::min(4, w - x);
  offset = ((int64_t)y * w + x) * 3;
  const uint8_t* p = img + offset;
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
  return n;
}

// The optical-density table into LDS, one word per thread. The caller's barrier follows.
__device__ __forceinline__ void stage_od(const int32_t* __restrict__ od_q, int32_t (&od_s)[256]) {
  od_s[threadIdx.x] = od_q[threadIdx.x];
}

// A pixel's Q12 optical densities; true iff it is stained: all three at least beta_q.
__device__ __forceinline__ bool pixel_od(const int32_t (&od_s)[256], const uint8_t (&p)[3], int beta_q,
                                         int32_t (&od)[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) od[c] = od_s[p[c]];
  return od[0] >= beta_q && od[1] >= beta_q && od[2] >= beta_q;
}

__device__ __forceinline__ int64_t dot3(const int32_t (&m)[3], const int32_t (&od)[3]) {
  return (int64_t)m[0] * od[0] + (int64_t)m[1] * od[1] + (int64_t)m[2] * od[2];
}

// Per thread ten 64-bit sums in registers. An optical density is < 2^15, so a product is < 2^30, and an image
// holds h w <= 65535^2 < 2^32 pixels: no sum reaches 2^62. block_sum adds 32-bit partial values whose sum
// over a wave must stay below 2^32, so each 64-bit register goes through it as three limbs of 21, 21 and 22
// bits (a wave's sum of a limb < 2^28); thread 3 q + l then holds limb l of quantity q, and thread 3 q adds the
// three, shifted back, to out[q]. (With one atomic per limb and 64-bit products the pass took 0.160 ms on a
// 4096 x 4096 image, this way 0.076 ms: DESIGN.md §7m.)
__global__ __launch_bounds__(PRED_TPB) void stain_moments_kernel(const uint8_t* __restrict__ img, int h, int w,
                                                                 const int32_t* __restrict__ od_q, int beta_q,
                                                                 unsigned long long* __restrict__ out) {
  __shared__ int32_t od_s[256];
  stage_od(od_q, od_s);
  __syncthreads();
  const int gq = (w + 3) >> 2;
  const int64_t total = (int64_t)h * gq;
  unsigned long long a[10] = {};
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    uint8_t px[4][3];
    int64_t offset;
    const int n = load_group(img, w, gq, i, px, offset);
    for (int j = 0; j < n; ++j) {
      int32_t od[3];
      if (!pixel_od(od_s, px[j], beta_q, od)) continue;
      const unsigned r = (unsigned)od[0], g = (unsigned)od[1], b = (unsigned)od[2];  // 32-bit products, < 2^30
      a[0] += 1, a[1] += r, a[2] += g, a[3] += b;
      a[4] += r * r, a[5] += r * g, a[6] += r * b, a[7] += g * g, a[8] += g * b, a[9] += b * b;
    }
  }
  unsigned c[30];
#pragma unroll
  for (int q = 0; q < 10; ++q) {
    c[3 * q] = (unsigned)(a[q] & 0x1fffffu);
    c[3 * q + 1] = (unsigned)((a[q] >> 21) & 0x1fffffu);
    c[3 * q + 2] = (unsigned)(a[q] >> 42);
  }
  const unsigned long long s = block_sum<30, PRED_TPB>(c);
  if (threadIdx.x < 64) {  // the first wave puts the three limbs of a quantity together: one atomic per word
    unsigned long long v = s << (21 * (threadIdx.x % 3));
    v += __shfl_down(v, 1, 64) + __shfl_down(v, 2, 64);
    if (threadIdx.x < 30 && threadIdx.x % 3 == 0 && v) atomicAdd(out + threadIdx.x / 3, v);
  }
}

// The workgroup's histogram in LDS (a workgroup meets fewer than 2^32 pixels: the image holds fewer), then the
// non-zero bins into the global words. With x > 0 the predicate cq_k y - sq_k x >= 0 holds for the
// directions up to the pixel's own angle and for none above, so the count of k in 1 .. K-1 that satisfy it is
// found in log2 K steps. The launcher bounds each row of B by sum |B| < 2^16, so with od < 2^15 x and y fit 32 bits
// and a product with |cq|, |sq| <= 2^14 is one 32 x 32 -> 64-bit multiply.
__global__ __launch_bounds__(PRED_TPB) void stain_angle_hist_kernel(const uint8_t* __restrict__ img, int h, int w,
                                                                    const int32_t* __restrict__ od_q, int beta_q,
                                                                    stain_mat2 B, const int32_t* __restrict__ dirs,
                                                                    unsigned long long* __restrict__ out) {
  __shared__ int32_t od_s[256];
  __shared__ int32_t dir_s[STAIN_K - 1][2];
  __shared__ unsigned hist[STAIN_K + 1];
  stage_od(od_q, od_s);
  for (int k = threadIdx.x; k < STAIN_K - 1; k += PRED_TPB) dir_s[k][0] = dirs[2 * k], dir_s[k][1] = dirs[2 * k + 1];
  for (int k = threadIdx.x; k <= STAIN_K; k += PRED_TPB) hist[k] = 0;
  __syncthreads();
  const int gq = (w + 3) >> 2;
  const int64_t total = (int64_t)h * gq;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    uint8_t px[4][3];
    int64_t offset;
    const int n = load_group(img, w, gq, i, px, offset);
    for (int j = 0; j < n; ++j) {
      int32_t od[3];
      if (!pixel_od(od_s, px[j], beta_q, od)) continue;
      const int32_t x = (int32_t)dot3(B.v[0], od), y = (int32_t)dot3(B.v[1], od);
      int bin = STAIN_K;  // the "skipped" word
      if (x > 0) {
        bin = 0;
#pragma unroll
        for (int step = STAIN_K / 2; step > 0; step >>= 1) {
          const int k = bin + step;  // in [1, K-1]
          if ((int64_t)dir_s[k - 1][0] * y - (int64_t)dir_s[k - 1][1] * x >= 0) bin = k;
        }
      }
      atomicAdd(&hist[bin], 1u);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k <= STAIN_K; k += PRED_TPB)
    if (hist[k]) atomicAdd(out + k, (unsigned long long)hist[k]);
}

// c = P_q[s] . od is Q24 (Q12 x Q12); a bin is 2^17 of it, 1/128 of a concentration, clamped at either end.
__global__ __launch_bounds__(PRED_TPB) void stain_conc_hist_kernel(const uint8_t* __restrict__ img, int h, int w,
                                                                   const int32_t* __restrict__ od_q, int beta_q,
                                                                   stain_mat2 P, unsigned long long* __restrict__ out) {
  __shared__ int32_t od_s[256];
  __shared__ unsigned hist[2 * STAIN_CB];
  stage_od(od_q, od_s);
  for (int k = threadIdx.x; k < 2 * STAIN_CB; k += PRED_TPB) hist[k] = 0;
  __syncthreads();
  const int gq = (w + 3) >> 2;
  const int64_t total = (int64_t)h * gq;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    uint8_t px[4][3];
    int64_t offset;
    const int n = load_group(img, w, gq, i, px, offset);
    for (int j = 0; j < n; ++j) {
      int32_t od[3];
      if (!pixel_od(od_s, px[j], beta_q, od)) continue;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int64_t bin = std::min<int64_t>(std::max<int64_t>(dot3(P.v[s], od) >> 17, 0), STAIN_CB - 1);
        atomicAdd(&hist[s * STAIN_CB + (int)bin], 1u);
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 2 * STAIN_CB; k += PRED_TPB)
    if (hist[k]) atomicAdd(out + k, (unsigned long long)hist[k]);
}

// o = T_q[c] . od is Q26 (Q14 x Q12), rounded to the Q10 index of the table of 255 exp(-i / 1024). Both tables
// sit in LDS. |T_q| < 2^20 and od < 2^15: |o| < 3 * 2^35. A whole group is written as 12 B in one store.
__global__ __launch_bounds__(PRED_TPB) void stain_apply_kernel(const uint8_t* __restrict__ img, int h, int w,
                                                               const int32_t* __restrict__ od_q, stain_mat3 T,
                                                               const uint8_t* __restrict__ exp_q, int n_exp,
                                                               uint8_t* __restrict__ out) {
  __shared__ int32_t od_s[256];
  __shared__ __attribute__((aligned(4))) uint8_t exp_s[STAIN_EXP_MAX];
  stage_od(od_q, od_s);
  const int n_words = ((uintptr_t)exp_q & 3) == 0 ? n_exp >> 2 : 0;  // by words where the table's address allows
  for (int k = threadIdx.x; k < n_words; k += PRED_TPB)
    reinterpret_cast<uint32_t*>(exp_s)[k] = reinterpret_cast<const uint32_t*>(exp_q)[k];
  for (int k = 4 * n_words + threadIdx.x; k < n_exp; k += PRED_TPB) exp_s[k] = exp_q[k];
  __syncthreads();
  const int gq = (w + 3) >> 2;
  const int64_t total = (int64_t)h * gq;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    uint8_t px[4][3];
    int64_t offset;
    const int n = load_group(img, w, gq, i, px, offset);
    rgb4 res = {};
    for (int j = 0; j < n; ++j) {
      int32_t od[3];
      pixel_od(od_s, px[j], 0, od);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int64_t idx = std::min<int64_t>(std::max<int64_t>((dot3(T.v[c], od) + (1 << 15)) >> 16, 0), n_exp - 1);
        const int k = 3 * j + c;
        res.w[k >> 2] |= (uint32_t)exp_s[idx] << (8 * (k & 3));
      }
    }
    uint8_t* q = out + offset;
    if (n == 4) {
      __builtin_memcpy(q, &res, 12);
    } else {
      for (int k = 0; k < 3 * n; ++k) q[k] = (uint8_t)(res.w[k >> 2] >> (8 * (k & 3)));
    }
  }
}

// The argument rules the four calls share; `fn` names the call in the message.
static int stain_args(const char* fn, const void* img, int32_t h, int32_t w, const void* od_q) {
  SELUNET_REQUIRE(img && od_q, "%s: null img or od_q", fn);
  SELUNET_REQUIRE(h >= 1 && h <= PRED_MAX_HW && w >= 1 && w <= PRED_MAX_HW,
                  "%s: image height and width must be in [1, %d] (got %d x %d)", fn, PRED_MAX_HW, h, w);
  SELUNET_REQUIRE(aligned(3, od_q), "%s: od_q must be 4-B aligned", fn);
  return SELUNET_OK;
}

static int64_t stain_items(int32_t h, int32_t w) { return (int64_t)h * ((w + 3) / 4); }

// The grid cap of all four: the fastest of 256 .. 16384 workgroups for each pass on a 4096 x 4096 image
// (profiles/stain_norm.txt). Below it the loop's own instructions are not hidden; above it the workgroups' closing
// atomics (up to 2 K words each) and the staging of the tables outweigh what more waves in flight bring.
constexpr int STAIN_GRID = 2048;

}  // namespace selunet

using namespace selunet;

extern "C" {

int selunet_stain_moments(const uint8_t* img, int32_t h, int32_t w, const int32_t* od_q, int32_t beta_q,
                          unsigned long long* out, void* stream) {
  if (int rc = stain_args("stain_moments", img, h, w, od_q)) return rc;
  SELUNET_REQUIRE(out, "stain_moments: null out");
  SELUNET_REQUIRE(aligned(7, out), "stain_moments: out must be 8-B aligned");
  const int64_t blocks = io_grid(cdiv(stain_items(h, w), PRED_TPB), STAIN_GRID);
  hipLaunchKernelGGL(stain_moments_kernel, dim3((unsigned)blocks), dim3(PRED_TPB), 0, as_stream(stream), img, h, w,
                     od_q, beta_q, out);
  return check_launch("stain_moments");
}

int selunet_stain_angle_hist(const uint8_t* img, int32_t h, int32_t w, const int32_t* od_q, int32_t beta_q,
                             const int32_t* B, const int32_t* dirs, unsigned long long* out, void* stream) {
  if (int rc = stain_args("stain_angle_hist", img, h, w, od_q)) return rc;
  SELUNET_REQUIRE(B && dirs && out, "stain_angle_hist: null B, dirs or out");
  SELUNET_REQUIRE(aligned(3, dirs) && aligned(7, out),
                  "stain_angle_hist: dirs must be 4-B aligned and out 8-B aligned");
  stain_mat2 b;
  for (int r = 0; r < 2; ++r) {
    int64_t sum = 0;
    for (int c = 0; c < 3; ++c) {
      b.v[r][c] = B[3 * r + c];
      sum += std::abs((int64_t)B[3 * r + c]);
    }
    SELUNET_REQUIRE(sum < (1 << 16),
                    "stain_angle_hist: B holds two unit vectors in Q14: each row's sum of |B| must be below 2^16 "
                    "(got %lld)", (long long)sum);
  }
  const int64_t blocks = io_grid(cdiv(stain_items(h, w), PRED_TPB), STAIN_GRID);
  hipLaunchKernelGGL(stain_angle_hist_kernel, dim3((unsigned)blocks), dim3(PRED_TPB), 0, as_stream(stream), img, h, w,
                     od_q, beta_q, b, dirs, out);
  return check_launch("stain_angle_hist");
}

int selunet_stain_conc_hist(const uint8_t* img, int32_t h, int32_t w, const int32_t* od_q, int32_t beta_q,
                            const int32_t* P_q, unsigned long long* out, void* stream) {
  if (int rc = stain_args("stain_conc_hist", img, h, w, od_q)) return rc;
  SELUNET_REQUIRE(P_q && out, "stain_conc_hist: null P_q or out");
  SELUNET_REQUIRE(aligned(7, out), "stain_conc_hist: out must be 8-B aligned");
  stain_mat2 p;
  for (int k = 0; k < 6; ++k) p.v[k / 3][k % 3] = P_q[k];  // any int32: |P_q . od| < 3 * 2^46
  const int64_t blocks = io_grid(cdiv(stain_items(h, w), PRED_TPB), STAIN_GRID);
  hipLaunchKernelGGL(stain_conc_hist_kernel, dim3((unsigned)blocks), dim3(PRED_TPB), 0, as_stream(stream), img, h, w,
                     od_q, beta_q, p, out);
  return check_launch("stain_conc_hist");
}

int selunet_stain_apply(const uint8_t* img, int32_t h, int32_t w, const int32_t* od_q, const int32_t* T_q,
                        const uint8_t* exp_q, int32_t n_exp, uint8_t* out, void* stream) {
  if (int rc = stain_args("stain_apply", img, h, w, od_q)) return rc;
  SELUNET_REQUIRE(T_q && exp_q && out, "stain_apply: null T_q, exp_q or out");
  SELUNET_REQUIRE(n_exp >= 1 && n_exp <= STAIN_EXP_MAX, "stain_apply: n_exp must be in [1, %d] (got %d)",
                  STAIN_EXP_MAX, n_exp);
  stain_mat3 t;
  for (int k = 0; k < 9; ++k) {
    SELUNET_REQUIRE(T_q[k] > -(1 << 20) && T_q[k] < (1 << 20),
                    "stain_apply: every |T_q| must be below 2^20, a factor of 64 (got %d)", T_q[k]);
    t.v[k / 3][k % 3] = T_q[k];
  }
  const int64_t bytes = (int64_t)h * w * 3;
  SELUNET_REQUIRE(out + bytes <= img || img + bytes <= out, "stain_apply: out must not alias img");
  const int64_t blocks = io_grid(cdiv(stain_items(h, w), PRED_TPB), STAIN_GRID);
  hipLaunchKernelGGL(stain_apply_kernel, dim3((unsigned)blocks), dim3(PRED_TPB), 0, as_stream(stream), img, h, w, od_q,
                     t, exp_q, n_exp, out);
  return check_launch("stain_apply");
}

}  // extern "C"
