// resize.hpp — Pillow's separable BICUBIC resampling (libImaging/Resample.c:
// bicubic_filter a = -0.5, precompute_coeffs, normalize_coeffs_8bpc with
// PRECISION_BITS = 22, ImagingResampleHorizontal/Vertical_8bpc with clip8).
// torchvision's RandomResizedCrop PIL path (reference cpu.py:172-183) is
// img.crop(box).resize((S, S), BICUBIC): the resample runs on the *cropped*
// image, so taps are clamped to the crop, box = (0, 0, w, h).
//
// Coefficients are computed in double exactly as Pillow does (no FMA
// contraction: the library is built with -ffp-contract=off) and quantised to
// the same int32 fixed point, so the uint8 result is bit-identical.
#pragma once

#include "common.hpp"

namespace dino {

constexpr int kPrecisionBits = 32 - 8 - 2;

DHD double bicubic_filter(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// Pillow's ksize for resampling in_size -> out_size (support 2 for bicubic).
DHD int resample_ksize(int in_size, int out_size) {
  double scale = (double)(float)in_size / out_size;
  double fs = scale < 1.0 ? 1.0 : scale;
  double support = 2.0 * fs;
  return (int)ceil(support) * 2 + 1;
}

// Coefficients of output index xx for in_size -> out_size with box (0, in_size).
// Writes bounds (xmin, xmax) and ksize int32 taps (zero padded).  Mirrors
// precompute_coeffs + normalize_coeffs_8bpc for one output position.
DHD void resample_coeffs_one(int in_size, int out_size, int xx, int ksize, int32_t* xmin_out, int32_t* xmax_out,
                             int32_t* k_out) {
  double in0 = 0.0, in1 = (double)(float)in_size;
  double scale = (in1 - in0) / out_size;
  double filterscale = scale < 1.0 ? 1.0 : scale;
  double support = 2.0 * filterscale;
  double center = in0 + (xx + 0.5) * scale;
  double ss = 1.0 / filterscale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  double ww = 0.0;
  // first pass: weights (Pillow stores them in the double kk buffer)
  for (int x = 0; x < xmax; ++x) {
    double w = bicubic_filter((x + xmin - center + 0.5) * ss);
    ww += w;
  }
  for (int x = 0; x < ksize; ++x) {
    int32_t q = 0;
    if (x < xmax) {
      double w = bicubic_filter((x + xmin - center + 0.5) * ss);
      if (ww != 0.0) w /= ww;
      q = w < 0 ? (int32_t)(-0.5 + w * (1 << kPrecisionBits)) : (int32_t)(0.5 + w * (1 << kPrecisionBits));
    }
    k_out[x] = q;
  }
  *xmin_out = xmin;
  *xmax_out = xmax;
}

// acc + px * k for one 8-bit pixel and one tap of resample_coeffs_one, as a 24-bit signed
// multiply-add on the GPU (v_mad_i32_i24, full rate; the 32-bit multiply it replaces issues
// at a quarter of that).  Both return the same low 32 bits whenever each operand is its own
// sign extension from 24 bits, so the sums stay Pillow's.  px is 0..255.  |k| < 2^23:
// a tap is round(2^22 w / ww) with w = bicubic_filter(d) and ww the sum of the window's
// weights.  The window always holds the pixel whose centre is nearest the output's centre
// (that centre lies inside the image, and clipping at an edge removes taps on the far side
// of it only), at |d| <= 0.5, and every pixel between it and the window's ends.  The filter
// is positive over |d| < 1 (area 1.0833) and negative over 1 < |d| < 2 (area -0.0417 a
// side, never below -2/27).  Upscaling (tap spacing 1): the weights left are f(d) >= 0.5625
// and at most one more positive and two negative ones, so ww >= 0.5625 - 4/27 = 0.41 and
// |w / ww| <= 1 / 0.41 < 2; the worst case is a window clipped to f(0.5), f(1.5) =
// 0.5625, -0.0625, whose larger tap is 1.125.  Downscaling by s samples the same filter
// s times as densely, with the nearest pixel at |d| <= 0.5 / s: the positive lobe's taps
// sum to at least 0.54 s - 1 beside a largest weight of 1 and negative ones of at most
// 0.084 s + 4/27, which leaves the ratio smaller still.
// The identity tap 2^22 (a pass that only copies) is inside the range too.
// tests/test_rcoeffs_range_cpu.py sweeps sizes, scales and edge positions for the largest
// magnitude (1.125 x 2^22); k_hresize's digit split needs the same bound (k_rcoeffs).
DHD int32_t tap_mad(int32_t px, int32_t k, int32_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __mul24(px, k) + acc;
#else
  return px * k + acc;
#endif
}

// Pillow's Image.resize (as of 12.2) resamples an image more than 100 times as high as
// wide, when its height shrinks, in two calls with the vertical pass first, so the 8-bit
// intermediate is rounded in the other order.  True for a crop of cw x ch resampled to a
// height of rh with kh horizontal taps (0: no horizontal pass, the order is moot).
// Such a crop is at most kVFirstMaxW wide (sides are <= 65536).
constexpr int kVFirstMaxW = 656;
DHD bool resample_vfirst(int cw, int ch, int rh, int kh) {
  return kh != 0 && (int64_t)ch > (int64_t)cw * 100 && rh < ch && cw <= kVFirstMaxW;
}

// clip8 of the fixed-point accumulator (Resample.c).
DHD uint8_t clip8_acc(int32_t in) {
  if (in >= (1 << kPrecisionBits << 8)) return 255;
  if (in <= 0) return 0;
  return (uint8_t)(in >> kPrecisionBits);
}

}  // namespace dino
