// Training-loop I/O kernels around the UNet_B step:
//
//  * selunet_prep_batch: pre-decoded uint8 NHWC patches + uint8 label masks -> the network input
//    (NCHW fp32, `Normalization` + `ToTensor`, utils/data_utils.py:94-106,160-168, with the
//    per-image `RandomFlip` of utils/data_utils.py:108-125) and the fp32 BCE target
//    (`label/255.0` truncated to uint8, utils/data_utils.py:220-221, then `.type(FloatTensor)`,
//    train.py:189-191). Replaces the host-side PIL decode + numpy transforms of the DataLoader.
//  * selunet_prep_batch_aug: the same with the training augmentation in front of the per-pixel conversion —
//    the eight orientations of the square, a glass quadrant (the reference's unused PartialNonTissue,
//    utils/data_utils.py:127-157) and a per-image colour table.
//  * selunet_seg_metrics: the per-batch host metrics of train.py:211-238 / eval.py:218-246 —
//    prediction threshold, selection threshold, rejection count and the Evaluator's 2x2
//    confusion matrix (utils/compute_metric.py:10-26) — as integer counts accumulated on the
//    device, so the loop never copies the [N,H,W] outputs to the host.
//  * selunet_seg_metrics_sweep: the same counts at up to 256 selection cut-offs in one pass (the
//    risk-coverage curve), as a per-bin histogram the host suffix-sums.
//  * selunet_seg_metrics_rows / selunet_patch_auc: the per-patch report (the reference's unused
//    get_performance, utils/compute_metric.py:93-148): selunet_seg_metrics' counts per image, and the
//    exact integer Mann-Whitney statistic behind each image's ROC AUC.
//
// All are byte/int work (no MFMA) in one pass over the data with 16-B coalesced loads; at an eval
// batch the metrics kernels are bound by their launch and their closing atomics, not by HBM.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "metrics_common.h"
#include "prep_pixel.h"

namespace selunet {

constexpr int IO_TPB = 256;

// One thread per (image, row, 4-pixel group): reads 12 B of RGB + 4 B of label (the whole
// 4-pixel group), writes 3 x 16 B of NCHW planes + 16 B of target. Flips are applied on the
// READ side (output pixel (y, x) reads source (y', x')), so the stores stay contiguous.
// The per-pixel conversion (CIN = 2: input_type 'GH'; HRGB: 'H_RGB') is prep_pixel (prep_pixel.h).
template <int CIN, bool HRGB = false>
__global__ void prep_batch_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ lab,
                                  const uint8_t* __restrict__ flips, int n, int h, int w, float* __restrict__ x,
                                  float* __restrict__ target) {
  const int wq = w >> 2;
  const int64_t total = (int64_t)n * h * wq;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int xq = (int)(i % wq);
    const int64_t r = i / wq;
    const int y = (int)(r % h);
    const int b = (int)(r / h);
    const int f = flips ? flips[b] : 0;
    const int ys = (f & 2) ? h - 1 - y : y;  // np.flipud (utils/data_utils.py:118-121)
    const int64_t src_row = ((int64_t)b * h + ys) * w;
    float xv[CIN][4];
    float tv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int xo = xq * 4 + j;
      const int xs = (f & 1) ? w - 1 - xo : xo;  // np.fliplr (utils/data_utils.py:113-116)
      const uint8_t* p = img + (src_row + xs) * 3;
      float v[CIN];
      prep_pixel<CIN, HRGB>(p[0], p[1], p[2], v);
#pragma unroll
      for (int c = 0; c < CIN; ++c) xv[c][j] = v[c];
      // (label/255.0).astype(uint8): truncation, so only 255 -> 1
      tv[j] = (float)(uint8_t)((double)lab[src_row + xs] / 255.0);
    }
    const int64_t plane = (int64_t)h * w;
    const int64_t o = (int64_t)y * w + xq * 4;
#pragma unroll
    for (int c = 0; c < CIN; ++c)
      *reinterpret_cast<f32x4*>(x + ((int64_t)b * CIN + c) * plane + o) = f32x4{xv[c][0], xv[c][1], xv[c][2], xv[c][3]};
    *reinterpret_cast<f32x4*>(target + (int64_t)b * plane + o) = f32x4{tv[0], tv[1], tv[2], tv[3]};
  }
}

// Counter-based noise of the glass model: 32 uniform bits from (key, counter) alone, in uint32 arithmetic
// (the lowbias32 finaliser twice, the counter spread by the golden ratio in between). The counter is an output
// position, so the noise depends neither on the batch nor on the grid.
__device__ __forceinline__ unsigned aug_mix(unsigned v) {
  v ^= v >> 16;
  v *= 0x7feb352du;
  v ^= v >> 15;
  v *= 0x846ca68bu;
  v ^= v >> 16;
  return v;
}
__device__ __forceinline__ unsigned aug_hash(unsigned key, unsigned counter) {
  return aug_mix(aug_mix(key) + counter * 0x9E3779B9u);
}

// prep_batch_kernel with the training augmentation in front of the per-pixel conversion: the
// same thread shape and stores; per output pixel it chooses which three bytes and which label byte enter
// prep_pixel. Glass (quadrant `glass[b]` of the OUTPUT, 1..4): bytes table[hash >> 20], label 0. Elsewhere the
// source pixel of geom[b] (bit 2 transposes, bit 1 flips rows, bit 0 columns: predict_tta.hip's T_k; a
// transposed image is square), its bytes through lut[b][c][.] when given. gmask = 7 when the caller declared
// transposed images (h == w, checked by the launcher), else 3: an undeclared bit 2 is ignored, never an
// out-of-range read. A transposed image reads four source rows per thread (plain byte reads: §7l).
// EXTRA: glass or lut may be given. Without either (flips and transposes alone) the per-pixel branch is compiled
// out, so that a thread's sixteen byte loads are in flight together as in prep_batch_kernel (with the branch the
// flips-only call took 32.0 us against 28.2 us at 128 x 256 x 256, profiles/augment_prep.txt).
template <int CIN, bool HRGB, bool EXTRA>
__global__ void prep_batch_aug_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ lab,
                                      const uint8_t* __restrict__ geom, const uint8_t* __restrict__ glass,
                                      const uint32_t* __restrict__ key, const uint8_t* __restrict__ lut,
                                      const uint8_t* __restrict__ table, int gmask, int n, int h, int w,
                                      float* __restrict__ x, float* __restrict__ target) {
  const int wq = w >> 2;
  const int hh = h >> 1, hw = w >> 1;
  const int64_t total = (int64_t)n * h * wq;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int xq = (int)(i % wq);
    const int64_t r = i / wq;
    const int y = (int)(r % h);
    const int b = (int)(r / h);
    const int f = geom ? geom[b] & gmask : 0;
    const int gl = EXTRA && glass ? glass[b] : 0;
    // quadrant gl - 1 = 2 * (lower half) + (right half)
    const bool glass_row = gl >= 1 && gl <= 4 && ((y >= hh) == (((gl - 1) & 2) != 0));
    const bool glass_right = ((gl - 1) & 1) != 0;
    const unsigned k = glass_row ? key[b] : 0u;
    const int ys = (f & 2) ? h - 1 - y : y;
    const int64_t src_img = (int64_t)b * h * w;
    const uint8_t* lt = EXTRA && lut ? lut + (int64_t)b * 768 : nullptr;
    float xv[CIN][4];
    float tv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int xo = xq * 4 + j;
      unsigned p[3], l;
      if (EXTRA && glass_row && ((xo >= hw) == glass_right)) {
        const unsigned c0 = ((unsigned)y * (unsigned)w + (unsigned)xo) * 3u;
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = table[aug_hash(k, c0 + c) >> 20];
        l = 0;
      } else {
        const int xs = (f & 1) ? w - 1 - xo : xo;
        const int64_t s = src_img + ((f & 4) ? (int64_t)xs * w + ys : (int64_t)ys * w + xs);
        const uint8_t* q = img + s * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = EXTRA && lt ? lt[c * 256 + q[c]] : q[c];
        l = lab[s];
      }
      float v[CIN];
      prep_pixel<CIN, HRGB>(p[0], p[1], p[2], v);
#pragma unroll
      for (int c = 0; c < CIN; ++c) xv[c][j] = v[c];
      // (label/255.0).astype(uint8): truncation, so only 255 -> 1
      tv[j] = (float)(uint8_t)((double)l / 255.0);
    }
    const int64_t plane = (int64_t)h * w;
    const int64_t o = (int64_t)y * w + xq * 4;
#pragma unroll
    for (int c = 0; c < CIN; ++c)
      *reinterpret_cast<f32x4*>(x + ((int64_t)b * CIN + c) * plane + o) = f32x4{xv[c][0], xv[c][1], xv[c][2], xv[c][3]};
    *reinterpret_cast<f32x4*>(target + (int64_t)b * plane + o) = f32x4{tv[0], tv[1], tv[2], tv[3]};
  }
}

// counts[0..3] = confusion matrix cm[label][pred] over the counted pixels (row-major, as
// Evaluator.confusion_matrix), counts[4] = selected pixels, counts[5] = all pixels (label.size).
// A pixel is counted iff 0 <= label < 2 and selected: pixel_state's rule (metrics_common.h).
// The workgroups blockIdx.x of gridDim.x share the p pixels; a grid's y dimension is the caller's.
__device__ __forceinline__ void seg_metrics_block(const float* __restrict__ out, const float* __restrict__ sel,
                                                  const float* __restrict__ target, int64_t p, float t_out,
                                                  float t_sel, unsigned long long* __restrict__ counts) {
  unsigned c[5] = {0, 0, 0, 0, 0};
  auto one = [&](float o, float t, float s) {
    const int st = pixel_state(o, s, t, sel != nullptr, t_out, t_sel);
    c[4] += st != 5;
    if (st < 4) c[st] += 1;
  };
  for_each_pixel<IO_TPB>(p, true, one, out, target, nullable(sel));
  const unsigned long long s = block_sum<5, IO_TPB>(c);
  if (threadIdx.x < 5) atomicAdd(counts + threadIdx.x, s);
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(counts + 5, (unsigned long long)p);
}

__global__ void seg_metrics_kernel(const float* __restrict__ out, const float* __restrict__ sel,
                                   const float* __restrict__ target, int64_t p, float t_out, float t_sel,
                                   unsigned long long* __restrict__ counts) {
  seg_metrics_block(out, sel, target, p, t_out, t_sel, counts);
}

// The same counts per image: blockIdx.y is the image, its hw pixels shared by the gridDim.x workgroups
// of the row. A thread counts at most hw <= 2^20 pixels into its 32-bit counters.
__global__ void seg_metrics_rows_kernel(const float* __restrict__ out, const float* __restrict__ sel,
                                        const float* __restrict__ target, int64_t hw, float t_out, float t_sel,
                                        unsigned long long* __restrict__ rows) {
  const int64_t base = (int64_t)blockIdx.y * hw;
  seg_metrics_block(out + base, sel ? sel + base : nullptr, target + base, hw, t_out, t_sel, rows + blockIdx.y * 6);
}

// Exact per-image Mann-Whitney statistic of the prediction logit (the integer form of a ROC AUC with
// ties at one half). With P / N the considered pixels of label 1 / 0 (considered: label < 2, selected,
// logit not NaN),
//   two_u = sum over p in P of ( #{q in N: out_q < out_p} + #{q in N: out_q <= out_p} ),
// and AUC = two_u / (2 |P| |N|). fp32 values map to 32-bit keys whose unsigned order is the numeric
// order (-0 folded into +0 first; the sign bit flipped for v >= 0, every bit for v < 0), so "less" and
// "less or equal" are both lower bounds in a sorted key list: #{k <= x} = #{k < x + 1}.
//
// Workgroup (c, i) sorts the keys of the considered negatives of chunk c of image i in LDS (every other
// slot holds the sentinel 0xFFFFFFFF, which no considered value maps to: NaNs are left out and +inf is
// 0xFF800000; sentinels sort last and are below no search key), then streams all hw pixels of the
// image and, for each considered positive, adds the two lower bounds of its key in the chunk. Summed
// over the chunks of the image that is the statistic. Workgroup (0, i) also counts |P|, |N| and the NaN
// logits. Integer adds only, so the result does not depend on scheduling.
//
// 32-bit partial counts at the largest hw = 2^20: a thread streams hw / AUC_TPB = 2^10 pixels, each adds
// at most 2 * SELUNET_AUC_CHUNK = 2^13, so a thread's sum is <= 2^23 and a wave's (64 threads) <= 2^29;
// the class counts are <= 2^10 per thread. Waves are summed in 64 bits; two_u itself is at most
// 2 * (hw/2)^2 = 2^39 per image and call.
//
// 1024 threads: the searches are chains of dependent LDS reads, and sixteen waves per CU hide their
// latency where four did not (16 x 256 x 256 pixels: 168 us with 256 threads).
constexpr int64_t PATCH_MAX_HW = (int64_t)1 << 20;  // pixels per image the per-image calls take
constexpr int AUC_CHUNK = SELUNET_AUC_CHUNK;
constexpr int AUC_TPB = 1024;
constexpr unsigned AUC_SENTINEL = 0xFFFFFFFFu;
static_assert((AUC_CHUNK & (AUC_CHUNK - 1)) == 0 && AUC_CHUNK % (AUC_TPB * 4) == 0 && AUC_CHUNK <= 4096,
              "AUC chunk: a power of two, whole 16-B loads per thread, 2^23 per thread at hw = 2^20");

__device__ __forceinline__ unsigned auc_key(float v) {
  unsigned b = __float_as_uint(v);
  b = b == 0x80000000u ? 0u : b;  // -0 == +0
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

__global__ __launch_bounds__(AUC_TPB) void patch_auc_kernel(const float* __restrict__ out,
                                                            const float* __restrict__ sel,
                                                            const float* __restrict__ target, int64_t hw,
                                                            float t_sel, unsigned long long* __restrict__ rows) {
  __shared__ unsigned keys[AUC_CHUNK];
  const int64_t base = (int64_t)blockIdx.y * hw;
  out += base;
  target += base;
  if (sel) sel += base;
  const int tid = threadIdx.x;
  // the label of a counted pixel (pixel_state's cm cells, whatever the prediction), else 2; NaN logits are told
  // apart by the caller
  auto label_of = [&](float s, float t) {
    const int lab = pixel_label(t);
    return pixel_selected(s, sel != nullptr, t_sel) && lab < 2 ? lab : 2;
  };

  // ---- this chunk's considered negatives as keys, everything else (and the ragged tail) the sentinel
  const int64_t c0 = (int64_t)blockIdx.x * AUC_CHUNK;
  int any = 0;
#pragma unroll
  for (int r = 0; r < AUC_CHUNK / (AUC_TPB * 4); ++r) {
    const int slot = (r * AUC_TPB + tid) * 4;
    const int64_t px = c0 + slot;
    unsigned k[4] = {AUC_SENTINEL, AUC_SENTINEL, AUC_SENTINEL, AUC_SENTINEL};
    if (px < hw) {  // hw % 4 == 0: a 16-B load is inside the image or wholly outside
      const f32x4 o = *reinterpret_cast<const f32x4*>(out + px);
      const f32x4 t = *reinterpret_cast<const f32x4*>(target + px);
      const f32x4 s = sel ? *reinterpret_cast<const f32x4*>(sel + px) : f32x4{0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (label_of(s[j], t[j]) == 0 && o[j] == o[j]) {
          k[j] = auc_key(o[j]);
          any = 1;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) keys[slot + j] = k[j];
  }
  any = __syncthreads_or(any);  // (also the barrier after the key stores)
  // a chunk without a negative adds nothing to two_u; workgroup 0 still owes the class counts
  if (!any && blockIdx.x != 0) return;

  // ---- bitonic sort, ascending (sentinels last); skipped when every key is the sentinel
  if (any) {
    for (int k = 2; k <= AUC_CHUNK; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        // the pairs of a pass are disjoint: all of a thread's reads first (independent, in flight
        // together), then its exchanges
        constexpr int PAIRS = AUC_CHUNK / 2 / AUC_TPB;
        unsigned a[PAIRS], b[PAIRS];
#pragma unroll
        for (int r = 0; r < PAIRS; ++r) {
          const int t = r * AUC_TPB + tid;
          const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          a[r] = keys[lo];
          b[r] = keys[lo | j];
        }
#pragma unroll
        for (int r = 0; r < PAIRS; ++r) {
          const int t = r * AUC_TPB + tid;
          const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          if ((a[r] > b[r]) == ((lo & k) == 0)) {
            keys[lo] = b[r];
            keys[lo | j] = a[r];
          }
        }
        __syncthreads();
      }
    }
  }

  // ---- stream the image: per considered positive, #{key < x} + #{key < x + 1}. The eight pixels of
  // two loads are searched side by side (eight independent chains of dependent LDS reads); x = 0 (below
  // every key) for the other pixels. The first steps read one address per wave, which LDS broadcasts.
  // #{key < x + 1} differs from lo = #{key < x} only when keys[lo] == x, a tie: the second search runs
  // only in waves that hold one (real-valued logits rarely tie; quantised ones pay both searches).
  auto below = [&](const unsigned (&x)[8], unsigned (&b)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) b[q] = 0;
    for (int st = AUC_CHUNK / 2; st > 0; st >>= 1)
#pragma unroll
      for (int q = 0; q < 8; ++q) b[q] += keys[b[q] + st - 1] < x[q] ? st : 0;
    // b = the true-prefix length of `key < x` over keys[0 .. CHUNK-2]; the last key on its own
    const unsigned last = keys[AUC_CHUNK - 1];
#pragma unroll
    for (int q = 0; q < 8; ++q) b[q] += last < x[q] ? 1 : 0;
  };
  unsigned two_u = 0, n_pos = 0, n_neg = 0, n_nan = 0;
  const bool counting = blockIdx.x == 0;
  for (int64_t px0 = (int64_t)tid * 4; px0 < hw; px0 += AUC_TPB * 8) {
    unsigned x[8];
    bool search = false;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t px = px0 + h * (AUC_TPB * 4);
      const bool in = px < hw;  // hw % 4 == 0: a 16-B load is inside the image or wholly outside
      const f32x4 o = in ? *reinterpret_cast<const f32x4*>(out + px) : f32x4{0, 0, 0, 0};
      const f32x4 t = in ? *reinterpret_cast<const f32x4*>(target + px) : f32x4{2, 2, 2, 2};  // label 2: not counted
      const f32x4 s = in && sel ? *reinterpret_cast<const f32x4*>(sel + px) : f32x4{0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int lab = in ? label_of(s[j], t[j]) : 2;
        const bool nan = o[j] != o[j];
        const bool pos = lab == 1 && !nan;
        x[h * 4 + j] = pos ? auc_key(o[j]) : 0u;
        search |= pos;
        if (counting) {
          n_pos += pos;
          n_neg += lab == 0 && !nan;
          n_nan += lab < 2 && nan;
        }
      }
    }
    if (any && search) {
      unsigned lo[8];
      below(x, lo);
      bool tie = false;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        two_u += 2 * lo[q];
        // lo == CHUNK: every key is below x; x == 0 equals no key (a considered key is >= 0x007FFFFF, -inf)
        tie |= lo[q] < AUC_CHUNK && keys[lo[q] < AUC_CHUNK ? lo[q] : 0] == x[q];
      }
      if (tie) {
        unsigned x1[8], hi[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) x1[q] = x[q] ? x[q] + 1u : 0u;  // a considered key is <= 0xFF800000 (+inf): no wrap
        below(x1, hi);
#pragma unroll
        for (int q = 0; q < 8; ++q) two_u += hi[q] - lo[q];
      }
    }
  }

  // ---- one 64-bit integer atomic per word and workgroup
  const unsigned part[4] = {two_u, n_pos, n_neg, n_nan};
  const unsigned long long sum = block_sum<4, AUC_TPB>(part);
  if (tid < 4 && sum) atomicAdd(rows + blockIdx.y * 4 + tid, sum);
}

// Risk-coverage sweep: seg_metrics_kernel's counts at k selection thresholds in one pass. With the
// thresholds ascending, `sel >= t_sel[j]` is a prefix of the list, so a pixel belongs to one bin
// b = #{j : sel >= t_sel[j]} in [0, k] and is selected at threshold j exactly when b > j: the
// per-bin histogram, suffix-summed by the host, gives every threshold's counts.
//
// Per pixel one 32-bit LDS counter [bin][class], class = cm cell (label * 2 + pred) or 4 for a label
// >= 2 (in `pixels` only). Trained selection scores cluster in a few bins, so same-address LDS
// atomics are the hazard: each wave has a private histogram, and when a whole wave agrees on the
// bin (a wave-uniform branch) it adds one ballot population count per class instead of 64 ones.
constexpr int SWEEP_WAVES = IO_TPB / 64;
constexpr int SWEEP_CLASSES = 5;
// One workgroup per CU: every workgroup adds its bins to the same cache lines at the end, and those
// requests are served one after the other (measured on 16 x 256 x 256 pixels, k = 11, uniform bins:
// 12.2 us at 256 workgroups, 15.4 us at 512, 25.2 us at 1024).
constexpr int SWEEP_GRID = 256;
// A wave counts at most its share of p pixels into a 32-bit counter: ~p / (SWEEP_GRID * SWEEP_WAVES)
// once the grid is capped, < 2^30 at this bound.
constexpr int64_t SWEEP_MAX_PIXELS = (int64_t)1 << 40;

// top: the largest power of two <= min(k, SELUNET_SWEEP_MAX - 1) (the first binary-search stride)
__global__ __launch_bounds__(IO_TPB) void seg_metrics_sweep_kernel(
    const float* __restrict__ out, const float* __restrict__ sel, const float* __restrict__ target, int64_t p,
    float t_out, const float* __restrict__ t_sel, int k, int top, unsigned long long* __restrict__ bins) {
  __shared__ float thr[SELUNET_SWEEP_MAX];
  __shared__ unsigned hist[SWEEP_WAVES][(SELUNET_SWEEP_MAX + 1) * SWEEP_CLASSES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cells = (k + 1) * SWEEP_CLASSES;
  stage_thresholds<IO_TPB>(thr, t_sel, k);
  for (int i = threadIdx.x; i < cells; i += IO_TPB)
#pragma unroll
    for (int wv = 0; wv < SWEEP_WAVES; ++wv) hist[wv][i] = 0;
  __syncthreads();
  unsigned* mine = hist[wave];

  // the true-prefix length over thr[0 .. 2*top-2] by binary search, then the last entry on its own
  // (k = 256 has 257 bins, one more than 8 halvings tell apart)
  auto bin_of = [&](float s) { return true_prefix(thr, s, top) + (s >= thr[SELUNET_SWEEP_MAX - 1] ? 1 : 0); };
  // pixel_state without a selection plane: the cm cell, or 4 for a label >= 2
  auto class_of = [&](float o, float t) { return pixel_state(o, 0.0f, t, false, t_out, 0.0f); };
  auto count = [&](int b, int cls) {
    const unsigned long long active = __ballot(1);
    const int b0 = __builtin_amdgcn_readfirstlane(b);
    if (__ballot(b == b0) == active) {
      // the wave agrees on the bin: one add per class present, by the lowest lane of that class
      unsigned long long same = 0;
#pragma unroll
      for (int c = 0; c < SWEEP_CLASSES; ++c) {
        const unsigned long long m = __ballot(cls == c);
        same = cls == c ? m : same;
      }
      if (lane == __ffsll((long long)same) - 1) atomicAdd(&mine[b0 * SWEEP_CLASSES + cls], (unsigned)__popcll(same));
    } else {
      atomicAdd(&mine[b * SWEEP_CLASSES + cls], 1u);
    }
  };
  const int64_t p4 = p >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < p4; i += stride) {
    const f32x4 o = *reinterpret_cast<const f32x4*>(out + i * 4);
    const f32x4 t = *reinterpret_cast<const f32x4*>(target + i * 4);
    const f32x4 s = *reinterpret_cast<const f32x4*>(sel + i * 4);
    int b[4];  // the four searches first: independent chains of dependent LDS reads
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = bin_of(s[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) count(b[j], class_of(o[j], t[j]));
  }
  for (int64_t i = p4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < p; i += stride)
    count(bin_of(sel[i]), class_of(out[i], target[i]));
  __syncthreads();
  // One thread per cell of bins, so that a wave's atomic covers 512 contiguous bytes: the workgroups
  // all add to the same few cache lines, and device atomics on one line are served one request (a
  // wave-instruction's share of the line) after the other. Integer atomics: the sums do not depend on
  // the order the workgroups arrive in.
  for (int i = threadIdx.x; i < cells; i += IO_TPB) {
    unsigned long long s = 0;
#pragma unroll
    for (int wv = 0; wv < SWEEP_WAVES; ++wv) s += hist[wv][i];
    if (i % SWEEP_CLASSES == 4)  // `pixels`: the other-label class plus the four cm cells of the bin
      for (int d = 1; d < SWEEP_CLASSES; ++d)
#pragma unroll
        for (int wv = 0; wv < SWEEP_WAVES; ++wv) s += hist[wv][i - d];
    if (s) atomicAdd(bins + i, s);
  }
}

}  // namespace selunet

using namespace selunet;

extern "C" {

int selunet_prep_batch_mode(const uint8_t* img, const uint8_t* lab, const uint8_t* flips, int32_t n, int32_t h,
                            int32_t w, int32_t mode, float* x, float* target, void* stream) {
  SELUNET_REQUIRE(mode >= 0 && mode <= 2, "prep_batch_mode: mode 0 'RGB', 1 'GH', 2 'H_RGB' (got %d)", mode);
  if (mode != 2) return selunet_prep_batch(img, lab, flips, n, h, w, mode == 0 ? 3 : 2, x, target, stream);
  SELUNET_REQUIRE(img && lab && x && target && n > 0 && h > 0 && w > 0 && w % 4 == 0, "prep_batch: bad arguments");
  SELUNET_REQUIRE(aligned(15, x, target), "prep_batch: outputs must be 16-B aligned");
  const int64_t total = (int64_t)n * h * (w / 4);
  const unsigned grid = (unsigned)io_grid(cdiv(total, IO_TPB), 8192);
  hipLaunchKernelGGL((prep_batch_kernel<3, true>), dim3(grid), dim3(IO_TPB), 0, as_stream(stream), img, lab, flips, n, h,
                     w, x, target);
  return check_launch("prep_batch");
}

int selunet_prep_batch(const uint8_t* img, const uint8_t* lab, const uint8_t* flips, int32_t n, int32_t h, int32_t w,
                       int32_t cin, float* x, float* target, void* stream) {
  SELUNET_REQUIRE(img && lab && x && target && n > 0 && h > 0 && w > 0, "prep_batch: bad arguments");
  SELUNET_REQUIRE(cin == 3 || cin == 2, "prep_batch: cin 3 (input_type 'RGB') or 2 ('GH', utils/data_utils.py:223-224)");
  SELUNET_REQUIRE(w % 4 == 0, "prep_batch: width must be a multiple of 4");
  SELUNET_REQUIRE(aligned(15, x, target), "prep_batch: outputs must be 16-B aligned");
  const int64_t total = (int64_t)n * h * (w / 4);
  const unsigned grid = (unsigned)io_grid(cdiv(total, IO_TPB), 8192);
  hipLaunchKernelGGL(cin == 3 ? prep_batch_kernel<3> : prep_batch_kernel<2>, dim3(grid), dim3(IO_TPB), 0,
                     as_stream(stream), img, lab, flips, n, h, w, x, target);
  return check_launch("prep_batch");
}

int selunet_prep_batch_aug(const uint8_t* img, const uint8_t* lab, const uint8_t* geom, const uint8_t* glass,
                           const uint32_t* key, const uint8_t* lut, const uint8_t* table, int32_t transposed,
                           int32_t n, int32_t h, int32_t w, int32_t mode, float* x, float* target, void* stream) {
  SELUNET_REQUIRE(mode >= 0 && mode <= 2, "prep_batch_aug: mode 0 'RGB', 1 'GH', 2 'H_RGB' (got %d)", mode);
  SELUNET_REQUIRE(img && lab && x && target && n > 0 && h > 0 && w > 0, "prep_batch_aug: bad arguments");
  SELUNET_REQUIRE(w % 4 == 0, "prep_batch_aug: width must be a multiple of 4 (got %d)", w);
  SELUNET_REQUIRE(aligned(15, x, target), "prep_batch_aug: outputs must be 16-B aligned");
  SELUNET_REQUIRE(!transposed || (geom && h == w),
                  "prep_batch_aug: a transposed image (geom bit 2) needs geom and h == w (got %d x %d)", h, w);
  SELUNET_REQUIRE(!glass || (table && key), "prep_batch_aug: glass needs the glass table and the keys");
  SELUNET_REQUIRE(aligned(3, key), "prep_batch_aug: key must be 4-B aligned");
  const int64_t total = (int64_t)n * h * (w / 4);
  const unsigned grid = (unsigned)io_grid(cdiv(total, IO_TPB), 8192);
  auto pick = [&](auto extra) {
    constexpr bool E = decltype(extra)::value;
    return mode == 0 ? prep_batch_aug_kernel<3, false, E>
                     : mode == 1 ? prep_batch_aug_kernel<2, false, E> : prep_batch_aug_kernel<3, true, E>;
  };
  auto kernel = glass || lut ? pick(std::true_type{}) : pick(std::false_type{});
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(IO_TPB), 0, as_stream(stream), img, lab, geom, glass, key, lut, table,
                     transposed ? 7 : 3, n, h, w, x, target);
  return check_launch("prep_batch_aug");
}

int selunet_seg_metrics(const float* out, const float* sel, const float* target, int64_t p, float t_out, float t_sel,
                        unsigned long long* counts, void* stream) {
  SELUNET_REQUIRE(out && target && counts && p > 0, "seg_metrics: bad arguments");
  SELUNET_REQUIRE(aligned(15, out, target, sel), "seg_metrics: inputs must be 16-B aligned");
  const unsigned grid = (unsigned)io_grid(cdiv(p / 4 + 1, IO_TPB), 2048);
  hipLaunchKernelGGL(seg_metrics_kernel, dim3(grid), dim3(IO_TPB), 0, as_stream(stream), out, sel, target, p, t_out,
                     t_sel, counts);
  return check_launch("seg_metrics");
}

// The argument rules the two per-image calls share; `fn` names the call in the message.
static int patch_rows_args(const char* fn, const float* out, const float* sel, const float* target, int32_t n,
                           int64_t hw, const unsigned long long* rows) {
  SELUNET_REQUIRE(out && target && rows, "%s: null out, target or rows", fn);
  SELUNET_REQUIRE(n >= 1, "%s: n must be >= 1 (got %d)", fn, n);
  SELUNET_REQUIRE(hw >= 1 && hw % 4 == 0 && hw <= PATCH_MAX_HW,
                  "%s: hw must be a multiple of 4 in [4, 2^20] (got %lld)", fn, (long long)hw);
  SELUNET_REQUIRE(aligned(15, out, target, sel), "%s: inputs must be 16-B aligned", fn);
  SELUNET_REQUIRE(aligned(7, rows), "%s: rows must be 8-B aligned", fn);
  return SELUNET_OK;
}

int selunet_seg_metrics_rows(const float* out, const float* sel, const float* target, int32_t n, int64_t hw,
                             float t_out, float t_sel, unsigned long long* rows, void* stream) {
  if (int rc = patch_rows_args("seg_metrics_rows", out, sel, target, n, hw, rows)) return rc;
  // at least four 16-B loads per thread before a workgroup's five closing atomics
  const unsigned gx = (unsigned)io_grid(cdiv(hw / 4, IO_TPB * 4), 64);
  for_image_chunks(n, IMAGE_GRID_Y, [&](int32_t i0, unsigned ny) {
    const int64_t o = (int64_t)i0 * hw;
    hipLaunchKernelGGL(seg_metrics_rows_kernel, dim3(gx, ny), dim3(IO_TPB), 0, as_stream(stream), out + o,
                       sel ? sel + o : nullptr, target + o, hw, t_out, t_sel, rows + (int64_t)i0 * 6);
  });
  return check_launch("seg_metrics_rows");
}

int selunet_patch_auc(const float* out, const float* sel, const float* target, int32_t n, int64_t hw, float t_sel,
                      unsigned long long* rows, void* stream) {
  if (int rc = patch_rows_args("patch_auc", out, sel, target, n, hw, rows)) return rc;
  const unsigned gx = (unsigned)cdiv(hw, (int64_t)AUC_CHUNK);
  // images per launch: blockIdx.y's 16 bits, and at most 2^31 threads in a grid
  const int32_t per = (int32_t)std::min<int64_t>(IMAGE_GRID_Y, ((int64_t)1 << 31) / ((int64_t)gx * AUC_TPB));
  for_image_chunks(n, per, [&](int32_t i0, unsigned ny) {
    const int64_t o = (int64_t)i0 * hw;
    hipLaunchKernelGGL(patch_auc_kernel, dim3(gx, ny), dim3(AUC_TPB), 0, as_stream(stream), out + o,
                       sel ? sel + o : nullptr, target + o, hw, t_sel, rows + (int64_t)i0 * 4);
  });
  return check_launch("patch_auc");
}

int selunet_seg_metrics_sweep(const float* out, const float* sel, const float* target, int64_t p, float t_out,
                              const float* t_sel, int32_t k, unsigned long long* bins, void* stream) {
  SELUNET_REQUIRE(out && sel && target && t_sel && bins, "seg_metrics_sweep: null out, sel, target, t_sel or bins");
  SELUNET_REQUIRE(p > 0 && p <= SWEEP_MAX_PIXELS, "seg_metrics_sweep: p must be in [1, 2^40] (got %lld)", (long long)p);
  SELUNET_REQUIRE(k >= 1 && k <= SELUNET_SWEEP_MAX, "seg_metrics_sweep: k must be in [1, %d] (got %d)",
                  SELUNET_SWEEP_MAX, k);
  SELUNET_REQUIRE(aligned(15, out, target, sel), "seg_metrics_sweep: inputs must be 16-B aligned");
  SELUNET_REQUIRE(aligned(3, t_sel) && aligned(7, bins), "seg_metrics_sweep: t_sel must be 4-B and bins 8-B aligned");
  const int top = search_top(std::min(k, SELUNET_SWEEP_MAX - 1));
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(p / 4 + 1, IO_TPB), SWEEP_GRID));
  hipLaunchKernelGGL(seg_metrics_sweep_kernel, dim3(grid), dim3(IO_TPB), 0, as_stream(stream), out, sel, target, p,
                     t_out, t_sel, k, top, bins);
  return check_launch("seg_metrics_sweep");
}

}  // extern "C"
