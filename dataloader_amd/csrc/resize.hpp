// resize.hpp — Pillow's separable resampling (libImaging/Resample.c as of 12.2: the
// filters bicubic_filter a = -0.5, bilinear_filter, box_filter, hamming_filter,
// lanczos_filter; precompute_coeffs, normalize_coeffs_8bpc with PRECISION_BITS = 22,
// ImagingResampleHorizontal/Vertical_8bpc with clip8).
// torchvision's RandomResizedCrop PIL path (reference cpu.py:172-183) is
// img.crop(box).resize((S, S), BICUBIC): the resample runs on the *cropped*
// image, so taps are clamped to the crop, box = (0, 0, w, h).
//
// Coefficients are computed in double exactly as Pillow does (no FMA
// contraction: the library is built with -ffp-contract=off) and quantised to
// the same int32 fixed point, so the uint8 result is bit-identical.  BICUBIC (code 0) is
// every recipe's default; the other filters are a context's choice
// (dino_ctx_set_resample_filter).  NEAREST is another algorithm in Pillow and is not here.
#pragma once

#include <math.h>

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

DHD double bilinear_filter(double x) {
  if (x < 0.0) x = -x;
  if (x < 1.0) return 1.0 - x;
  return 0.0;
}

// (the bounds are Pillow's: a pixel centre exactly half a support away counts on one side only)
DHD double box_filter(double x) { return x > -0.5 && x <= 0.5 ? 1.0 : 0.0; }

constexpr double kPi = 3.14159265358979323846;  // M_PI

// Pillow writes the window's constants as float literals: 0.54f and 0.46f widened to double.
DHD double hamming_filter(double x) {
  if (x < 0.0) x = -x;
  if (x == 0.0) return 1.0;
  if (x >= 1.0) return 0.0;
  x = x * kPi;
  return sin(x) / x * ((double)0.54f + (double)0.46f * cos(x));
}

DHD double sinc_filter(double x) {
  if (x == 0.0) return 1.0;
  x = x * kPi;
  return sin(x) / x;
}

DHD double lanczos_filter(double x) {
  if (-3.0 <= x && x < 3.0) return sinc_filter(x) * sinc_filter(x / 3);
  return 0.0;
}

template <int F>
DHD double resample_filter(double x) {
  return F == kBilinear ? bilinear_filter(x)
         : F == kBox    ? box_filter(x)
         : F == kHamming ? hamming_filter(x)
         : F == kLanczos ? lanczos_filter(x)
                         : bicubic_filter(x);
}

// Pillow's ksize for resampling in_size -> out_size with the filter's support.
DHD int resample_ksize(int in_size, int out_size, int filter = kBicubic) {
  double scale = (double)(float)in_size / out_size;
  double fs = scale < 1.0 ? 1.0 : scale;
  double support = 0.5 * resample_support2(filter) * fs;
  return (int)ceil(support) * 2 + 1;
}

// Coefficients of output index xx for in_size -> out_size with box (0, in_size).
// Writes bounds (xmin, xmax) and ksize int32 taps (zero padded).  Mirrors
// precompute_coeffs + normalize_coeffs_8bpc for one output position.
template <int F>
DHD void resample_coeffs_filter(int in_size, int out_size, int xx, int ksize, int32_t* xmin_out, int32_t* xmax_out,
                                int32_t* k_out) {
  double in0 = 0.0, in1 = (double)(float)in_size;
  double scale = (in1 - in0) / out_size;
  double filterscale = scale < 1.0 ? 1.0 : scale;
  double support = 0.5 * resample_support2(F) * filterscale;
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
    double w = resample_filter<F>((x + xmin - center + 0.5) * ss);
    ww += w;
  }
  for (int x = 0; x < ksize; ++x) {
    int32_t q = 0;
    if (x < xmax) {
      double w = resample_filter<F>((x + xmin - center + 0.5) * ss);
      if (ww != 0.0) w /= ww;
      q = w < 0 ? (int32_t)(-0.5 + w * (1 << kPrecisionBits)) : (int32_t)(0.5 + w * (1 << kPrecisionBits));
    }
    k_out[x] = q;
  }
  *xmin_out = xmin;
  *xmax_out = xmax;
}

// The filter is a run-time value (a context's setting, the same for every lane of a launch):
// one branch per output position, none per tap.
DHD void resample_coeffs_one(int in_size, int out_size, int xx, int ksize, int32_t* xmin_out, int32_t* xmax_out,
                             int32_t* k_out, int filter = kBicubic) {
  switch (filter) {
    case kBilinear: return resample_coeffs_filter<kBilinear>(in_size, out_size, xx, ksize, xmin_out, xmax_out, k_out);
    case kBox: return resample_coeffs_filter<kBox>(in_size, out_size, xx, ksize, xmin_out, xmax_out, k_out);
    case kHamming: return resample_coeffs_filter<kHamming>(in_size, out_size, xx, ksize, xmin_out, xmax_out, k_out);
    case kLanczos: return resample_coeffs_filter<kLanczos>(in_size, out_size, xx, ksize, xmin_out, xmax_out, k_out);
    default: return resample_coeffs_filter<kBicubic>(in_size, out_size, xx, ksize, xmin_out, xmax_out, k_out);
  }
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
// The other filters.  BOX, BILINEAR and HAMMING are non-negative, so a normalised weight is
// at most 1 and a tap at most 2^22 (reached by any one-tap window, e.g. 1 -> 1); their taps
// sum to 2^22 plus at most half a unit of rounding each.  LANCZOS, L(d) = sinc(d) sinc(d / 3),
// is negative over 1 < |d| < 2 (area -0.0893 a side, never below -0.1473) and positive over
// |d| < 1 (area 1.1427) and 2 < |d| < 3 (0.0165 a side, at most 0.0312).  Upscaling, the
// nearest pixel lies at e, |e| <= 0.5, with L(e) >= L(0.5) = 0.6079, the window's other taps
// at e + j, and of the two neighbours at e +- 1 one is negative and the other positive.  A
// window clipped at the nearest pixel keeps e, e + 1, e + 2 (e > 0): L(e) / (L(e) + L(1 + e)
// + L(2 + e)) <= L(e) / (L(e) + L(1 + e)), which rises with e to L(0.5) / (L(0.5) + L(1.5)) =
// 0.6079 / (0.6079 - 0.1351) = 9/7 = 1.2857: a two-pixel side upscaled, the first output, as
// the output size grows.  Every other window adds positive weight faster than negative.
// Downscaling by s the ratio falls (1.283 at s = 1.1, 1.13 at s = 1.5, 1 from s = 2 on, by the
// same enumeration of clipped windows over a fine grid of phases), as for BICUBIC.
// sum|k| of one output is largest for the same window: (0.6079 + 0.1351) / 0.4728 = 11/7.
// tests/test_resample_filters_cpu.py sweeps the library's own coefficient code per filter:
//   filter    largest |k| / 2^22 at (in, out, position)   largest sum|k| / 2^22
//   BILINEAR  1.0000 at (1, 1, 0)                          1.0002 at (4096, 1, 0)
//   BOX       1.0000 at (1, 1, 0)                          1.0002 at (65535, 30, 0)
//   HAMMING   1.0000 at (1, 1, 0)                          1.0000 at (16384, 1, 0)
//   LANCZOS   1.2854 at (2, 1024, 0)                       1.5714 at (4, 5, 2)
// all below 2^23, inside k_rcoeffs' digit planes (k < 2^23 - 2^15 = 1.992 x 2^22), and 255 x
// sum|k| + 2^21 <= 1.57 x 2^30 < 2^31: no partial sum of a pass leaves int32 in any order.
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
