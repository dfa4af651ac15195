// Connected regions of a prediction mask: canonical labels, the exact region table and the
// in-place clean-up of the mask, all on the device.
//
//  * selunet_regions_label: three launches on one stream.
//      local    one workgroup per REG_TILE x REG_TILE pixels: union-find on LDS words, every pixel's
//               tile-local root out as a position in the pitched plane. No traffic between workgroups.
//      seam     one thread per pixel next to a tile border: union(a, b) on the plane by atomicMin of the
//               larger root's word. Every access to the plane is an agent-scope atomic (the L2s of the XCDs
//               are not coherent and an L1 is never refreshed by another CU's stores); words only decrease,
//               finds halve their paths, and every loop carries a cap that sets the error word.
//      flatten  after the seam kernel has ended (the kernel boundary publishes the roots): every pixel
//               follows its chain to the root with plain loads and stores 1 + y W + x of that root into a
//               second plane, with a flag where the pixel is a root itself.
//  * selunet_regions_stats: a wave walks 64 pixels of a row; the lanes of a run of equal labels are combined
//    (run length from a ballot of the run heads, the two sums that are not a function of the run's ends from
//    one packed prefix sum by shuffles); the run heads of a 64 x 64 tile meet in a hash table in LDS, which
//    is flushed with one integer atomic per column and label.
//  * selunet_regions_apply: the mask rewritten in place by a per-region action, and the four pixel counts of
//    the result by the stitch kernel's reduction (add_class_counts).
//
// Nothing here waits on another workgroup: no grid barrier, no cooperative launch, no spin on a flag.
#include <algorithm>

#include "common.h"
#include "predict_common.h"

namespace selunet {

// 64 x 64: the tile's parents are 16 KB of LDS (up to 10 workgroups per CU), 16 pixels per thread, and a
// tile row is 256 B of the parent plane, so the stores of a quarter wave fill two whole 128-B lines. A
// smaller tile quadruples the seam pixels per area; a larger one does not fit 4-B parents at this occupancy.
constexpr int REG_TILE = 64;
constexpr int REG_PIX = REG_TILE * REG_TILE;
constexpr uint32_t REG_NONE = 0xFFFFFFFFu;  // parent word of a pixel that is not of the value
// Caps of the loops over the global plane. A chain strictly decreases, so it ends without them; they guard
// against a corrupted plane only. A find follows at most one word per tile-local root on its path.
constexpr uint32_t REG_FIND_CAP = 1u << 22;
constexpr uint32_t REG_RETRY_CAP = 1u << 16;
constexpr uint32_t REG_ERR_LOCAL = 1, REG_ERR_SEAM = 2, REG_ERR_FLATTEN = 4;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ local pass
__device__ __forceinline__ int lds_find(volatile int* L, int i, bool& bad) {
  for (int k = 0; k < REG_PIX; ++k) {  // a chain inside the tile has fewer than REG_PIX links
    const int p = L[i];
    if (p == i) return i;
    i = p;
  }
  bad = true;
  return i;
}

__device__ __forceinline__ void lds_union(int* L, int a, int b, bool& bad) {
  for (int k = 0; k < REG_PIX; ++k) {  // every retry follows a decrease of a word: fewer than REG_PIX
    a = lds_find(L, a, bad);
    b = lds_find(L, b, bad);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&L[a], b);  // a > b: hang the larger root under the smaller
    if (old == a) return;
    a = old;  // a was no root any more: go on from what it pointed to
  }
  bad = true;
}

__global__ __launch_bounds__(PRED_TPB) void regions_local_kernel(const uint8_t* __restrict__ mask, int64_t pitch, int h,
                                                                 int w, int value, int conn8, int tiles_x, int lp,
                                                                 uint32_t* __restrict__ parent,
                                                                 uint32_t* __restrict__ err) {
  __shared__ int L[REG_PIX];
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
  const int y0 = ty * REG_TILE, x0 = tx * REG_TILE;
  const int lx = (threadIdx.x & 15) * 4, ly0 = threadIdx.x >> 4;
  // 4 pixels of a row per thread and step: one 4-B load where the address allows it
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ly = ly0 + 16 * k, y = y0 + ly, x = x0 + lx;
    uint32_t m = ~0u;
    bool in[4] = {false, false, false, false};
    if (y < h && x < w) {
      const uint8_t* p = mask + (int64_t)y * pitch + x;
      if (x + 3 < w && ((uintptr_t)p & 3) == 0) {
        m = *reinterpret_cast<const uint32_t*>(p);
        in[0] = in[1] = in[2] = in[3] = true;
      } else {
        m = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x + j < w) {
            m |= (uint32_t)p[j] << (8 * j);
            in[j] = true;
          }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = ly * REG_TILE + lx + j;
      L[i] = (in[j] && (int)((m >> (8 * j)) & 255u) == value) ? i : -1;
    }
  }
  __syncthreads();
  bool bad = false;
  // a pixel of the value joins its left and upper neighbours inside the tile; under 8 the two upper
  // diagonals only where the upper pixel is not of the value (else they are joined through it)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ly = ly0 + 16 * k;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = lx + j, i = ly * REG_TILE + x;
      if (L[i] < 0) continue;
      if (x > 0 && L[i - 1] >= 0) lds_union(L, i, i - 1, bad);
      if (ly > 0) {
        if (L[i - REG_TILE] >= 0) {
          lds_union(L, i, i - REG_TILE, bad);
        } else if (conn8) {
          if (x > 0 && L[i - REG_TILE - 1] >= 0) lds_union(L, i, i - REG_TILE - 1, bad);
          if (x < REG_TILE - 1 && L[i - REG_TILE + 1] >= 0) lds_union(L, i, i - REG_TILE + 1, bad);
        }
      }
    }
  }
  __syncthreads();
  // roots are final: every pixel's root as a position in the pitched plane, 16 B per thread and row
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ly = ly0 + 16 * k, y = y0 + ly, x = x0 + lx;
    if (y >= h || x >= lp) continue;  // lp % 4 == 0: the four words lie inside the row or outside it
    u32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = ly * REG_TILE + lx + j;
      uint32_t g = REG_NONE;
      if (L[i] >= 0) {
        const int r = lds_find(L, i, bad);
        g = (uint32_t)(y0 + r / REG_TILE) * (uint32_t)lp + (uint32_t)(x0 + r % REG_TILE);
      }
      o[j] = g;
    }
    *reinterpret_cast<u32x4*>(parent + (int64_t)y * lp + x) = o;
  }
  if (bad) atomicOr(err, REG_ERR_LOCAL);
}

// ------------------------------------------------------------------ seam pass
__device__ __forceinline__ uint32_t seam_load(uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of i, halving the path on the way: a word on the path is lowered to its grandparent, which the
// parent's own word reaches without it, so no connection is lost while other threads link roots. Without it
// a chain of tile roots (a serpentine crosses thousands of tiles) would be walked link by link by every find.
__device__ __forceinline__ uint32_t seam_find(uint32_t* P, uint32_t i, bool& bad) {
  for (uint32_t k = 0; k < REG_FIND_CAP; ++k) {
    const uint32_t p = seam_load(P + i);
    if (p >= i) return i;  // p == i: a root (p > i cannot be: a word only goes down from its own position)
    const uint32_t g = seam_load(P + p);
    if (g >= p) return p;
    __hip_atomic_fetch_min(P + i, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    i = g;
  }
  bad = true;
  return i;
}

__device__ __forceinline__ void seam_union(uint32_t* P, uint32_t a, uint32_t b, bool& bad) {
  for (uint32_t k = 0; k < REG_RETRY_CAP; ++k) {
    a = seam_find(P, a, bad);
    b = seam_find(P, b, bad);
    if (bad || a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    const uint32_t old = __hip_atomic_fetch_min(P + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;
    a = old;  // the word had changed: a was no root any more, and what it pointed to is joined with b next
  }
  bad = true;
}

// Set A: the pixels of the first row of every tile row but the first, joined with the row above (up, and
// under 8 up-left / up-right). Set B: the pixels of the first column of every tile column but the first,
// joined with the column to the left (left, and under 8 up-left / down-left). Two adjacent pixels of
// different tiles differ in the tile row (then the lower one is in A) or only in the tile column (then the
// right one is in B), so every pair across a border is met, the diagonal ones at the tile corners included.
__global__ __launch_bounds__(PRED_TPB) void regions_seam_kernel(uint32_t* parent, int h, int w, int lp, int conn8,
                                                                int64_t n_a, int64_t n_b,
                                                                uint32_t* __restrict__ err) {
  bool bad = false;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_a + n_b;
       i += (int64_t)gridDim.x * blockDim.x) {
    int x, y;
    const bool set_a = i < n_a;
    if (set_a) {
      y = (int)(i / w + 1) * REG_TILE;
      x = (int)(i % w);
    } else {
      const int64_t j = i - n_a;
      x = (int)(j / h + 1) * REG_TILE;
      y = (int)(j % h);
    }
    const uint32_t at = (uint32_t)y * (uint32_t)lp + (uint32_t)x;
    if (seam_load(parent + at) == REG_NONE) continue;
    if (set_a) {
      const uint32_t up = at - (uint32_t)lp;
      if (seam_load(parent + up) != REG_NONE) {
        seam_union(parent, at, up, bad);
      } else if (conn8) {
        if (x > 0 && seam_load(parent + up - 1) != REG_NONE) seam_union(parent, at, up - 1, bad);
        if (x < w - 1 && seam_load(parent + up + 1) != REG_NONE) seam_union(parent, at, up + 1, bad);
      }
    } else {
      const uint32_t left = at - 1;
      if (seam_load(parent + left) != REG_NONE) {
        seam_union(parent, at, left, bad);
      } else if (conn8) {
        if (y > 0 && seam_load(parent + left - (uint32_t)lp) != REG_NONE)
          seam_union(parent, at, left - (uint32_t)lp, bad);
        if (y < h - 1 && seam_load(parent + left + (uint32_t)lp) != REG_NONE)
          seam_union(parent, at, left + (uint32_t)lp, bad);
      }
    }
  }
  if (bad) atomicOr(err, REG_ERR_SEAM);
}

// ------------------------------------------------------------------ flatten pass
// One thread per 4 words of a row. labels = 1 + y W + x of the root (0 where the pixel is not of the value,
// the padding columns included); roots = 1 where the pixel is its region's root.
// The forest is final here, so a word on a path may be lowered to any of its ancestors by a plain store (the
// path is halved for the pixels that follow), and a plain load that still sees the older word sees an ancestor
// too: roots are never written.
__global__ __launch_bounds__(PRED_TPB) void regions_flatten_kernel(uint32_t* parent, int h, int w, int lp,
                                                                   int32_t* __restrict__ labels,
                                                                   uint8_t* __restrict__ roots,
                                                                   uint32_t* __restrict__ err) {
  const int gq = lp >> 2;
  const int64_t total = (int64_t)h * gq;
  bool bad = false;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t at = i * 4;  // = y lp + x
    const u32x4 p = *reinterpret_cast<const u32x4*>(parent + at);
    i32x4 o = {0, 0, 0, 0};
    uint32_t flags = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (p[j] == REG_NONE) continue;
      uint32_t r = p[j];
      uint32_t k = 0;
      for (; k < REG_FIND_CAP; ++k) {
        const uint32_t q = parent[r];
        if (q >= r) break;
        const uint32_t g = parent[q];
        if (g >= q) {
          r = q;
          break;
        }
        parent[r] = g;
        r = g;
      }
      if (k == REG_FIND_CAP) bad = true;
      o[j] = (int32_t)(1u + (r / (uint32_t)lp) * (uint32_t)w + r % (uint32_t)lp);
      flags |= (uint32_t)(r == (uint32_t)at + j) << (8 * j);
    }
    *reinterpret_cast<i32x4*>(labels + at) = o;
    *reinterpret_cast<uint32_t*>(roots + at) = flags;
  }
  if (bad) atomicOr(err, REG_ERR_FLATTEN);
}

// ------------------------------------------------------------------ region table
// table: uint64 [REG_COLS][n_rows]; the caller sets the columns of sums to 0, of minima to a large value, of
// maxima to 0.
enum { RC_AREA = 0, RC_YMIN, RC_XMIN, RC_YMAX, RC_XMAX, RC_SUMY, RC_SUMX, RC_PROB, RC_CONTACT, REG_COLS };

// A minimum (maximum) only moves one way, so a value read earlier, however stale, that already is at or
// below (above) ours shows the atomic would change nothing.
__device__ __forceinline__ void table_min(unsigned long long* p, unsigned long long v) {
  if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > v) atomicMin(p, v);
}
__device__ __forceinline__ void table_max(unsigned long long* p, unsigned long long v) {
  if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v) atomicMax(p, v);
}

// One run's, or one workgroup's, share of a region into the table: an atomic per column that has something to add.
struct region_part {
  uint32_t area, y_min, x_min, y_max, x_max, prob, contacts;
  unsigned long long sum_y, sum_x;
};

__device__ __forceinline__ void table_add(unsigned long long* __restrict__ table, int64_t n_rows, int32_t l, int64_t hw,
                                          int w, const int32_t* __restrict__ rowidx, int rp, bool has_prob,
                                          const region_part& v) {
  if (l <= 0 || (int64_t)l > hw) return;
  const int64_t r0 = (int64_t)l - 1;
  const int64_t row = rowidx[(r0 / w) * rp + r0 % w];
  if (row < 0 || row >= n_rows) return;
  unsigned long long* t = table + row;
  atomicAdd(t + RC_AREA * n_rows, (unsigned long long)v.area);
  table_min(t + RC_YMIN * n_rows, (unsigned long long)v.y_min);
  table_min(t + RC_XMIN * n_rows, (unsigned long long)v.x_min);
  table_max(t + RC_YMAX * n_rows, (unsigned long long)v.y_max);
  table_max(t + RC_XMAX * n_rows, (unsigned long long)v.x_max);
  atomicAdd(t + RC_SUMY * n_rows, v.sum_y);
  atomicAdd(t + RC_SUMX * n_rows, v.sum_x);
  if (has_prob && v.prob) atomicAdd(t + RC_PROB * n_rows, (unsigned long long)v.prob);
  if (v.contacts) atomicAdd(t + RC_CONTACT * n_rows, (unsigned long long)v.contacts);
}

// One workgroup per REG_TILE x REG_TILE pixels, a wave per row (16 rows each). Stage 1, per wave: the lanes of a
// run of equal labels are combined by shuffles. Stage 2, per workgroup: the run heads add into a small hash
// table in LDS keyed by the label (LDS atomics), which is flushed with one global atomic per column and label
// at the end; a head that finds no slot within STAT_PROBES adds to the global table itself. A region that
// covers the tile thus costs one set of global atomics per tile instead of one per row of it: without stage 2
// the atomics of a plane-filling region queue up on one table row (both forms are measured in DESIGN.md §7h).
constexpr int STAT_SLOTS = 128, STAT_PROBES = 4;

__global__ __launch_bounds__(PRED_TPB) void regions_stats_kernel(
    const int32_t* __restrict__ labels, int lp, const uint8_t* __restrict__ mask, int64_t pitch,
    const uint8_t* __restrict__ prob8, int64_t prob_pitch, int h, int w, int tiles_x,
    const int32_t* __restrict__ rowidx, int rp, int64_t n_rows, unsigned long long* __restrict__ table) {
  __shared__ int key[STAT_SLOTS];  // 0: free (labels are > 0)
  __shared__ uint32_t s_area[STAT_SLOTS], s_ymin[STAT_SLOTS], s_xmin[STAT_SLOTS], s_ymax[STAT_SLOTS],
      s_xmax[STAT_SLOTS], s_prob[STAT_SLOTS], s_cont[STAT_SLOTS];
  __shared__ unsigned long long s_sumy[STAT_SLOTS], s_sumx[STAT_SLOTS];
  for (int i = threadIdx.x; i < STAT_SLOTS; i += PRED_TPB) {
    key[i] = 0;
    s_area[i] = s_ymax[i] = s_xmax[i] = s_prob[i] = s_cont[i] = 0u;
    s_ymin[i] = s_xmin[i] = 0xFFFFFFFFu;
    s_sumy[i] = s_sumx[i] = 0ull;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t hw = (int64_t)h * w;
  const int y0 = (int)(blockIdx.x / tiles_x) * REG_TILE, x = (int)(blockIdx.x % tiles_x) * REG_TILE + lane;
  for (int r = 0; r < REG_TILE / (PRED_TPB / 64); ++r) {
    const int y = y0 + r * (PRED_TPB / 64) + wave;
    if (y >= h) break;  // the same for the whole wave
    int32_t l = 0;
    uint32_t packed = 0;  // prob8 in bits 0..15 (at most 64 * 255), abstained 4-neighbours in bits 16..
    if (x < w) {
      l = labels[(int64_t)y * lp + x];
      if (l > 0) {
        const uint8_t* m = mask + (int64_t)y * pitch + x;
        const uint32_t c = (uint32_t)(y > 0 && m[-pitch] == 127) + (uint32_t)(y < h - 1 && m[pitch] == 127) +
                           (uint32_t)(x > 0 && m[-1] == 127) + (uint32_t)(x < w - 1 && m[1] == 127);
        packed = (c << 16) | (prob8 ? (uint32_t)prob8[(int64_t)y * prob_pitch + x] : 0u);
      }
    }
    // runs of equal labels along the lanes: the head of each run acts for it
    const int32_t lprev = __shfl_up(l, 1, 64);
    const bool head = lane == 0 || l != lprev;
    const unsigned long long heads = __ballot(head);
    uint32_t pre = packed;  // inclusive prefix sum over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(pre, o, 64);
      if (lane >= o) pre += t;
    }
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    const int len = above ? __ffsll((long long)above) : 64 - lane;  // lanes past w hold label 0: a run of their own
    const uint32_t pre_tail = __shfl(pre, lane + len - 1, 64);
    const uint32_t sum = pre_tail - (pre - packed);
    if (!head || l <= 0) continue;
    const unsigned long long n = (unsigned long long)len;
    region_part v;
    v.area = (uint32_t)len;
    v.y_min = v.y_max = (uint32_t)y;
    v.x_min = (uint32_t)x;
    v.x_max = (uint32_t)(x + len - 1);
    v.prob = sum & 0xFFFFu;
    v.contacts = sum >> 16;
    v.sum_y = n * (unsigned long long)y;
    v.sum_x = n * (unsigned long long)x + n * (n - 1) / 2;
    int slot = -1;
    uint32_t at = ((uint32_t)l * 2654435761u) >> 25;  // 7 bits: STAT_SLOTS
    for (int k = 0; k < STAT_PROBES; ++k, at = (at + 1) & (STAT_SLOTS - 1)) {
      const int old = atomicCAS(&key[at], 0, l);
      if (old == 0 || old == l) {
        slot = (int)at;
        break;
      }
    }
    if (slot < 0) {
      table_add(table, n_rows, l, hw, w, rowidx, rp, prob8 != nullptr, v);
      continue;
    }
    atomicAdd(&s_area[slot], v.area);
    atomicMin(&s_ymin[slot], v.y_min);
    atomicMin(&s_xmin[slot], v.x_min);
    atomicMax(&s_ymax[slot], v.y_max);
    atomicMax(&s_xmax[slot], v.x_max);
    atomicAdd(&s_sumy[slot], v.sum_y);
    atomicAdd(&s_sumx[slot], v.sum_x);
    if (v.prob) atomicAdd(&s_prob[slot], v.prob);
    if (v.contacts) atomicAdd(&s_cont[slot], v.contacts);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < STAT_SLOTS; i += PRED_TPB) {
    if (key[i] == 0) continue;
    region_part v;
    v.area = s_area[i];
    v.y_min = s_ymin[i];
    v.x_min = s_xmin[i];
    v.y_max = s_ymax[i];
    v.x_max = s_xmax[i];
    v.prob = s_prob[i];
    v.contacts = s_cont[i];
    v.sum_y = s_sumy[i];
    v.sum_x = s_sumx[i];
    table_add(table, n_rows, key[i], hw, w, rowidx, rp, prob8 != nullptr, v);
  }
}

// ------------------------------------------------------------------ apply
// One thread per 4 pixels of a row, one aligned 4-B load and store where the row's address allows it. With
// labels == nullptr nothing is written and the mask is only counted.
__global__ __launch_bounds__(PRED_TPB) void regions_apply_kernel(uint8_t* __restrict__ mask, int64_t pitch, int h, int w,
                                                                 const int32_t* __restrict__ labels, int lp,
                                                                 const int32_t* __restrict__ rowidx, int rp,
                                                                 const uint8_t* __restrict__ action, int64_t n_rows,
                                                                 unsigned long long* __restrict__ counts) {
  const int gq = (w + 3) >> 2;
  const int64_t total = (int64_t)h * gq, hw = (int64_t)h * w;
  unsigned c[3] = {0, 0, 0};
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / gq), x = (int)(i % gq) * 4;
    uint8_t* p = mask + (int64_t)y * pitch + x;
    const int n = std::min(4, w - x);
    const bool word = n == 4 && ((uintptr_t)p & 3) == 0;
    uint32_t m = 0;
    if (word) {
      m = *reinterpret_cast<const uint32_t*>(p);
    } else {
      for (int j = 0; j < n; ++j) m |= (uint32_t)p[j] << (8 * j);
    }
    uint32_t out = m;
    if (labels) {
      for (int j = 0; j < n; ++j) {
        const int32_t l = labels[(int64_t)y * lp + x + j];
        if (l <= 0 || (int64_t)l > hw) continue;
        const int64_t r0 = (int64_t)l - 1;
        const int64_t row = rowidx[(r0 / w) * rp + r0 % w];
        if (row < 0 || row >= n_rows) continue;
        const uint32_t a = action[row];
        if (a == 1) out &= ~(255u << (8 * j));
        else if (a == 2) out |= 255u << (8 * j);
      }
      if (out != m) {
        if (word) {
          *reinterpret_cast<uint32_t*>(p) = out;
        } else {
          for (int j = 0; j < n; ++j)
            if (((out ^ m) >> (8 * j)) & 255u) p[j] = (uint8_t)(out >> (8 * j));
        }
      }
    }
    for (int j = 0; j < n; ++j) {
      const uint32_t v = (out >> (8 * j)) & 255u;
      c[0] += v == 0u;
      c[1] += v == 255u;
      c[2] += v == 127u;
    }
  }
  add_class_counts(c, counts);
}

static int64_t grid_for(int64_t threads) {
  return io_grid(cdiv(threads, PRED_TPB), 16384);
}

// The rules every call shares: the image's size, and the pitched label plane that goes with it.
static int region_args(const char* fn, int32_t h, int32_t w) {
  SELUNET_REQUIRE(h >= 1 && w >= 1, "%s: height and width must be >= 1 (got %d x %d)", fn, h, w);
  SELUNET_REQUIRE((int64_t)h * w < 2147483647LL, "%s: H * W must be below 2^31 - 1 (got %d x %d)", fn, h, w);
  return SELUNET_OK;
}

}  // namespace selunet

using namespace selunet;

extern "C" {

int selunet_regions_label(const uint8_t* mask, int64_t mask_pitch, int32_t h, int32_t w, int32_t value,
                          int32_t connectivity, uint32_t* parent, int32_t* labels, uint8_t* roots, int32_t lp,
                          uint32_t* err, int32_t passes, void* stream) {
  SELUNET_REQUIRE(mask && parent && labels && roots && err, "regions_label: null mask, parent, labels, roots or err");
  if (int rc = region_args("regions_label", h, w)) return rc;
  SELUNET_REQUIRE(mask_pitch >= w, "regions_label: the mask's row pitch must hold the width (got %lld for %d)",
                  (long long)mask_pitch, w);
  SELUNET_REQUIRE(value >= 0 && value <= 255, "regions_label: value must be in [0, 255] (got %d)", value);
  SELUNET_REQUIRE(connectivity == 4 || connectivity == 8, "regions_label: connectivity must be 4 or 8 (got %d)",
                  connectivity);
  SELUNET_REQUIRE(lp >= w && lp % 4 == 0 && lp - w < 4,
                  "regions_label: the label pitch must be the width rounded up to a multiple of 4 (got %d for %d)", lp, w);
  SELUNET_REQUIRE((int64_t)h * lp < 4294967295LL,
                  "regions_label: H * pitch must be below 2^32 - 1 (got %d x %d)", h, lp);
  SELUNET_REQUIRE(((uintptr_t)parent & 15) == 0 && ((uintptr_t)labels & 15) == 0 && ((uintptr_t)roots & 3) == 0,
                  "regions_label: parent and labels must be 16-B aligned, roots 4-B aligned");
  SELUNET_REQUIRE(((uintptr_t)err & 3) == 0, "regions_label: err must be 4-B aligned");
  SELUNET_REQUIRE(passes >= 1 && passes <= 7, "regions_label: passes must be a set of 1 local, 2 seam, 4 flatten (got %d)",
                  passes);
  const int64_t tiles_x = cdiv(w, REG_TILE), tiles_y = cdiv(h, REG_TILE);
  SELUNET_REQUIRE(tiles_x * tiles_y < 2147483647LL, "regions_label: too many tiles (%lld)",
                  (long long)(tiles_x * tiles_y));
  const int conn8 = connectivity == 8;
  hipStream_t st = as_stream(stream);
  if (passes & 1) {
    hipLaunchKernelGGL(regions_local_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(PRED_TPB), 0, st, mask,
                       mask_pitch, h, w, value, conn8, (int)tiles_x, lp, parent, err);
    if (int rc = check_launch("regions_label (local)")) return rc;
  }
  const int64_t n_a = (tiles_y - 1) * w, n_b = (tiles_x - 1) * h;
  if ((passes & 2) && n_a + n_b > 0) {
    hipLaunchKernelGGL(regions_seam_kernel, dim3((unsigned)grid_for(n_a + n_b)), dim3(PRED_TPB), 0, st, parent, h, w, lp,
                       conn8, n_a, n_b, err);
    if (int rc = check_launch("regions_label (seam)")) return rc;
  }
  if (!(passes & 4)) return SELUNET_OK;
  hipLaunchKernelGGL(regions_flatten_kernel, dim3((unsigned)grid_for((int64_t)h * (lp / 4))), dim3(PRED_TPB), 0, st,
                     parent, h, w, lp, labels, roots, err);
  return check_launch("regions_label (flatten)");
}

int selunet_regions_stats(const int32_t* labels, int32_t lp, const uint8_t* mask, int64_t mask_pitch,
                          const uint8_t* prob8, int64_t prob_pitch, int32_t h, int32_t w, const int32_t* rowidx,
                          int32_t rp, int64_t n_rows, unsigned long long* table, void* stream) {
  SELUNET_REQUIRE(labels && mask && rowidx && table, "regions_stats: null labels, mask, rowidx or table");
  if (int rc = region_args("regions_stats", h, w)) return rc;
  SELUNET_REQUIRE(lp >= w && rp >= w && mask_pitch >= w && (!prob8 || prob_pitch >= w),
                  "regions_stats: every row pitch must hold the width %d (got labels %d, rowidx %d, mask %lld, prob8 %lld)",
                  w, lp, rp, (long long)mask_pitch, (long long)prob_pitch);
  SELUNET_REQUIRE(n_rows >= 1 && n_rows <= (int64_t)h * w, "regions_stats: n_rows must be in [1, H * W] (got %lld)",
                  (long long)n_rows);
  SELUNET_REQUIRE(((uintptr_t)labels & 3) == 0 && ((uintptr_t)rowidx & 3) == 0 && ((uintptr_t)table & 7) == 0,
                  "regions_stats: labels and rowidx must be 4-B aligned, table 8-B aligned");
  const int64_t tiles_x = cdiv(w, REG_TILE), tiles = tiles_x * cdiv(h, REG_TILE);
  SELUNET_REQUIRE(tiles < 2147483647LL, "regions_stats: too many tiles (%lld)", (long long)tiles);
  hipLaunchKernelGGL(regions_stats_kernel, dim3((unsigned)tiles), dim3(PRED_TPB), 0, as_stream(stream), labels, lp, mask,
                     mask_pitch, prob8, prob_pitch, h, w, (int)tiles_x, rowidx, rp, n_rows, table);
  return check_launch("regions_stats");
}

int selunet_regions_apply(uint8_t* mask, int64_t mask_pitch, int32_t h, int32_t w, const int32_t* labels, int32_t lp,
                          const int32_t* rowidx, int32_t rp, const uint8_t* action, int64_t n_rows,
                          unsigned long long* counts, void* stream) {
  SELUNET_REQUIRE(mask && counts, "regions_apply: null mask or counts");
  if (int rc = region_args("regions_apply", h, w)) return rc;
  SELUNET_REQUIRE(mask_pitch >= w, "regions_apply: the mask's row pitch must hold the width (got %lld for %d)",
                  (long long)mask_pitch, w);
  SELUNET_REQUIRE((labels != nullptr) == (rowidx != nullptr) && (labels != nullptr) == (action != nullptr),
                  "regions_apply: labels, rowidx and action must all be given or all be null (count only)");
  if (labels) {
    SELUNET_REQUIRE(lp >= w && rp >= w, "regions_apply: the pitches of labels and rowidx must hold the width %d (got %d, %d)",
                    w, lp, rp);
    SELUNET_REQUIRE(n_rows >= 1 && n_rows <= (int64_t)h * w, "regions_apply: n_rows must be in [1, H * W] (got %lld)",
                    (long long)n_rows);
    SELUNET_REQUIRE(((uintptr_t)labels & 3) == 0 && ((uintptr_t)rowidx & 3) == 0,
                    "regions_apply: labels and rowidx must be 4-B aligned");
  }
  SELUNET_REQUIRE(((uintptr_t)counts & 7) == 0, "regions_apply: counts must be 8-B aligned");
  const int64_t groups = (int64_t)h * cdiv(w, 4);
  hipLaunchKernelGGL(regions_apply_kernel, dim3((unsigned)grid_for(groups)), dim3(PRED_TPB), 0, as_stream(stream), mask,
                     mask_pitch, h, w, labels, lp, rowidx, rp, action, n_rows, counts);
  return check_launch("regions_apply");
}

}  // extern "C"
