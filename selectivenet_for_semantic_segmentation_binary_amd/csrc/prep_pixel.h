// One RGB uint8 pixel -> the network's input channels: the per-pixel part of PatchDataset.__getitem__'s
// transforms (utils/data_utils.py:13-41, 94-106, 220-226), shared by selunet_prep_batch (train_io.hip)
// selunet_tile_gather (predict_io.hip) and selunet_tile_gather_flip (predict_tta.hip) so that all of them
// give the same bits for the same pixel.
#pragma once

#include "common.h"

namespace selunet {

// CIN = 2: input_type 'GH' (utils/data_utils.py:13-27, applied before Normalization at :223-224):
// channel 0 = cv2 RGB2GRAY of the [0,1] fp32 image (0.299 R + 0.587 G + 0.114 B), channel 1 = the
// hematoxylin stain of skimage.color.separate_stains(rgb, hed_from_rgb) (stains = (log(max(rgb,
// 1e-6)) / log(1e-6)) @ hed_from_rgb, clamped at 0; column 0 of inv(rgb_from_hed)) min-max
// normalised with the reference's constants -0.66781543 / 1.87798274.
constexpr double HED_H0 = 1.8779827368521353, HED_H1 = -0.06590806222356332, HED_H2 = -0.6019073634392891;
constexpr double GH_HMIN = -0.66781543, GH_HMAX = 1.87798274;

// HRGB (CIN = 3): input_type 'H_RGB' (utils/data_utils.py:29-41): the hematoxylin stain h of
// separate_stains as above, recombined alone by skimage.color.combine_stains(stack(h, 0, 0),
// rgb_from_hed) = clip(exp(-h * (-log 1e-6) * rgb_from_hed[0]), 0, 1), rgb_from_hed[0] =
// (0.65, 0.70, 0.29).
//
// r, g, b: the pixel's bytes; o[c]: channel c of the normalised input.
// No multiply-add of this function is fused: left to the compiler, which products of a sum it fuses depends on
// the kernel around the call and on the pixel's place in a thread's group of four, so that two kernels — or
// two columns of one — could differ in the last bit for the same pixel.
template <int CIN, bool HRGB>
__device__ __forceinline__ void prep_pixel(unsigned r, unsigned g, unsigned b, float (&o)[CIN]) {
#pragma clang fp contract(off)
  // input/255.0 in float64, astype(float32) (utils/data_utils.py:220-221)
  const float v[3] = {(float)((double)r / 255.0), (float)((double)g / 255.0), (float)((double)b / 255.0)};
  if constexpr (HRGB) {
    const float la = logf(1e-6f);
    double st = 0.0;
    st += (double)(logf(fmaxf(v[0], 1e-6f)) / la) * HED_H0;
    st += (double)(logf(fmaxf(v[1], 1e-6f)) / la) * HED_H1;
    st += (double)(logf(fmaxf(v[2], 1e-6f)) / la) * HED_H2;
    const double h = fmax(st, 0.0) * -log(1e-6);
    const double rf[3] = {0.65, 0.70, 0.29};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float e = (float)fmin(fmax(exp(-h * rf[c]), 0.0), 1.0);
      o[c] = (e - 0.5f) / 0.5f;
    }
  } else if constexpr (CIN == 3) {
    // (x - 0.5) / 0.5 in float32 (Normalization, utils/data_utils.py:101)
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (v[c] - 0.5f) / 0.5f;
  } else {
    const float gray = v[0] * 0.299f + v[1] * 0.587f + v[2] * 0.114f;
    const float la = logf(1e-6f);
    double st = 0.0;
    st += (double)(logf(fmaxf(v[0], 1e-6f)) / la) * HED_H0;
    st += (double)(logf(fmaxf(v[1], 1e-6f)) / la) * HED_H1;
    st += (double)(logf(fmaxf(v[2], 1e-6f)) / la) * HED_H2;
    const float hn = (float)((fmax(st, 0.0) - GH_HMIN) / (GH_HMAX - GH_HMIN));
    o[0] = (gray - 0.5f) / 0.5f;
    o[1] = (hn - 0.5f) / 0.5f;
  }
}

}  // namespace selunet
