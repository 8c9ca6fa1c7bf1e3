// draft.hpp — reduced-size JPEG decode (Pillow's Image.draft, libjpeg's scale_num / scale_denom):
// the scale rule, each component's block size and the upsampling that is left, as k_draft,
// k_idct_red and k_color_red (kernels_draft.inc) and the host model use them.
#pragma once

#include "color.hpp"

namespace dino {

// JpegImagePlugin.py draft("RGB", (n, n)): k = min(W // n, H // n), the scale is the largest of
// 8, 4, 2, 1 that is <= k (fallback.draft_scale states the same rule).  Returns log2 of it.
DHD int draft_shift_of(int w, int h, int n) {
  if (n <= 0) return 0;
  const int k = (w < h ? w : h) / n;
  return k >= 8 ? 3 : (k >= 4 ? 2 : (k >= 2 ? 1 : 0));
}

DHD int draft_dim(int full, int shift) { return (full + (1 << shift) - 1) >> shift; }

// jdmaster.c jpeg_calc_output_dimensions: every component starts at min_size = 8 >> shift and
// doubles while that still divides its share of the output in both directions ("scale up the
// chroma components via IDCT scaling rather than upsampling").
DHD int draft_comp_size(const ImgDesc& d, int c) {
  const int mn = 8 >> d.draft_shift;
  const CompDesc& cd = d.comp[c];
  int size = mn;
  while (size < 8 && (d.max_h * mn) % (cd.h * size * 2) == 0 && (d.max_v * mn) % (cd.v * size * 2) == 0) size *= 2;
  return size;
}

// jdsample.c jinit_upsampler with the scaled sizes: fancy upsampling only while min_size > 1
// (do_fancy), h1v2 without it and every other ratio go to the integer box.
DHD int draft_upsample_method(int hf, int vf, int dw, bool fancy) {
  if (hf == 1 && vf == 1) return kUpFull;
  if (hf == 2 && vf == 1) return fancy && dw > 2 ? kUpH2V1Fancy : kUpH2V1Box;
  if (hf == 1 && vf == 2 && fancy) return kUpH1V2Fancy;
  if (hf == 2 && vf == 2) return fancy && dw > 2 ? kUpH2V2Fancy : kUpH2V2Box;
  return kUpInt;
}

// Component c's plane of a scaled image: `size` samples a block at pitch bw * size inside the
// component's full-size reservation; dw x dh = libjpeg's downsampled size after IDCT scaling;
// hf, vf = (max_h * min_size) / (h * size) and the same for v.
DHD PlaneView draft_plane_view(const ImgDesc& d, const uint8_t* planes, int c) {
  const CompDesc& cd = d.comp[c];
  const int mn = 8 >> d.draft_shift, size = draft_comp_size(d, c);
  PlaneView v;
  v.p = planes + cd.plane_off;
  v.pitch = cd.bw * size;
  v.dw = (int32_t)(((int64_t)d.full_w * (cd.h * size) + d.max_h * 8 - 1) / (d.max_h * 8));
  v.dh = (int32_t)(((int64_t)d.full_h * (cd.v * size) + d.max_v * 8 - 1) / (d.max_v * 8));
  v.hf = (d.max_h * mn) / (cd.h * size);
  v.vf = (d.max_v * mn) / (cd.v * size);
  v.method = draft_upsample_method(v.hf, v.vf, v.dw, mn > 1);
  return v;
}

}  // namespace dino
