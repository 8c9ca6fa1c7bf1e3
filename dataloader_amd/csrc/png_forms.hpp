// png_forms.hpp — the PNG forms beyond png_parse.hpp's: bit depths 1, 2, 4 and 16 and Adam7
// interlace.  Geometry of the passes, the IHDR rules and the pixel rules, host and device
// (k_pnghead_forms, k_unfilter_forms, dino_probe_png_forms, dino_debug_png_forms_decode).
//
// The zlib stream of such a file is the one of any PNG (inflate.hpp); what differs comes after:
//   * an Adam7 file holds up to seven reduced images ("passes") one after another, each with its
//     own row width and its own filter history (PNG specification 8.2; Pillow's ZipDecode.c
//     restarts `previous` at every pass);
//   * the filters work on bytes `u` apart, u = max(1, channels x depth / 8) (9.2);
//   * depths below 8 pack samples MSB first, a row ends on a byte (7.2);
//   * 16-bit samples are big-endian; Pillow 12 keeps the high byte of RGB, RGBA and gray + alpha
//     (modes RGB / RGBA from "RGB;16B" / "RGBA;16B" / "LA;16B") and turns 16-bit gray (mode I;16)
//     to RGB by clipping: min(v, 255) (tests/test_png_forms_cpu.py pins all 65 536 values).
// tRNS and PLTE rules depend on the colour type only: png_walk is used as it is.
#pragma once

#include "png_parse.hpp"

namespace dino {

// The form of one file: what IHDR says beyond width and height.
struct PngForm {
  int32_t W, H, color, depth, lace;
  DHD int channels() const { return png_channels(color); }
  DHD int unit() const {  // bytes between a byte and its left neighbour: 1, 2, 3, 4, 6 or 8
    const int b = channels() * depth / 8;
    return b < 1 ? 1 : b;
  }
};

// PNG's (colour type, depth) pairs: gray 1/2/4/8/16, RGB 8/16, palette 1/2/4/8, gray + alpha
// 8/16, RGBA 8/16.
DHD bool png_form_valid(int color, int depth) {
  const bool d8 = depth == 8, d16 = depth == 16, low = depth == 1 || depth == 2 || depth == 4;
  switch (color) {
    case 0: return low || d8 || d16;
    case 3: return low || d8;
    case 2: case 4: case 6: return d8 || d16;
    default: return false;
  }
}

// Pass p of Adam7 as (x0, y0, dx, dy): (0,0,8,8) (4,0,8,8) (0,4,4,8) (2,0,4,4) (0,2,2,4)
// (1,0,2,2) (0,1,1,2), a nibble each; a file without interlace is the one pass (0,0,1,1).
struct PngPass {
  int32_t x0, y0, dx, dy;
  int32_t w, h;    // pixels of a row, rows (both 0 for a pass without pixels)
  int32_t rb;      // bytes of a row without its filter byte
};
DHD PngPass png_form_pass(const PngForm& f, int p) {
  PngPass s;
  if (f.lace) {
    s.x0 = (0x0102040 >> (4 * p)) & 15;
    s.y0 = (0x1020400 >> (4 * p)) & 15;
    s.dx = (0x1224488 >> (4 * p)) & 15;
    s.dy = (0x2244888 >> (4 * p)) & 15;
  } else {
    s.x0 = s.y0 = 0;
    s.dx = s.dy = 1;
  }
  s.w = f.W > s.x0 ? (f.W - s.x0 + s.dx - 1) / s.dx : 0;
  s.h = f.H > s.y0 ? (f.H - s.y0 + s.dy - 1) / s.dy : 0;
  if (s.w == 0 || s.h == 0) s.w = s.h = 0;
  s.rb = (int32_t)(((int64_t)s.w * f.channels() * f.depth + 7) >> 3);
  return s;
}
DHD int png_form_passes(const PngForm& f) { return f.lace ? 7 : 1; }

// Rows of all passes together and the bytes they inflate to (a filter byte a row).
struct PngFormGeom {
  int32_t rows;
  int64_t bytes;
};
DHD PngFormGeom png_form_geom(const PngForm& f) {
  PngFormGeom g{0, 0};
  for (int p = 0; p < png_form_passes(f); ++p) {
    const PngPass s = png_form_pass(f, p);
    g.rows += s.h;
    g.bytes += (int64_t)s.h * (1 + (int64_t)s.rb);
  }
  return g;
}

// Row r of the concatenated pass sequence: its pass, its row there and where its filter byte
// lies in the inflated bytes.  Seven prefix sums walked in registers, no table in memory.
struct PngRowAt {
  PngPass pass;
  int32_t yp;     // row within the pass (0: the filters see no row above)
  int64_t off;    // of the filter byte
};
DHD PngRowAt png_form_row(const PngForm& f, int r) {
  PngRowAt a;
  int32_t row0 = 0;
  int64_t off0 = 0;
  a.pass = png_form_pass(f, 0);
  for (int p = 0;;) {
    if (r < row0 + a.pass.h || p + 1 >= png_form_passes(f)) break;
    row0 += a.pass.h;
    off0 += (int64_t)a.pass.h * (1 + (int64_t)a.pass.rb);
    a.pass = png_form_pass(f, ++p);
  }
  a.yp = r - row0;
  a.off = off0 + (int64_t)a.yp * (1 + (int64_t)a.pass.rb);
  return a;
}

// An extended-form descriptor keeps, besides what parse_png_head states for kind 4, in fields
// the JPEG stages of a kind-4 image never read: coef_bytes = the inflated bytes of all passes
// (never 0: it marks the extended form; png_inflated_bytes answers it), mcus_x = bit depth,
// mcus_y = interlace method, max_h = the filter unit u.
DHD bool png_is_form(const ImgDesc& d) { return d.kind == kPngKind && d.coef_bytes != 0; }
DHD PngForm png_form_of(const ImgDesc& d) { return PngForm{d.width, d.height, d.color, d.mcus_x, d.mcus_y}; }
// Units of the widest row: what the carry row of k_unfilter_forms holds (8 bytes each).
DHD int64_t png_form_max_units(const ImgDesc& d) {
  const PngForm f = png_form_of(d);
  return (((int64_t)f.W * f.channels() * f.depth + 7) >> 3) / f.unit();
}

// A file parse_png_head declined (d->status == kPngDecline, d->kind == kPngKind, width and
// height set and within check_dims): when depth or interlace alone were the reason, the
// descriptor becomes the extended-form one and the status DINO_IMG_OK.  Every byte index of
// the stages stays below 2^31: the rows hold up to 8 bytes a pixel.
DHD int parse_png_forms_head(const uint8_t* p, int64_t len, ImgDesc* d) {
  if (d->status != kPngDecline || d->kind != kPngKind || !png_signature(p, len) || len < 8 + 8 + 13 + 4) return d->status;
  if (rd32be(p + 12) != png_cid('I', 'H', 'D', 'R') || rd32be(p + 8) != 13) return d->status;
  const uint32_t w = rd32be(p + 16), h = rd32be(p + 20);
  const int depth = p[24], color = p[25], comp = p[26], filt = p[27], lace = p[28];
  if (w < 1 || h < 1 || w > 0x7FFFFFFFu || h > 0x7FFFFFFFu || (int32_t)w != d->width || (int32_t)h != d->height) return d->status;
  if (!png_form_valid(color, depth) || comp != 0 || filt != 0 || lace > 1) return d->status;
  if (depth == 8 && lace == 0) return d->status;  // (parse_png_head's own form, declined for its size)
  if ((int64_t)h * (1 + (int64_t)w * 8) > 0x7FFFFFF0ll || len > 0x7FFFFFF0ll) return d->status;
  const PngForm f{(int32_t)w, (int32_t)h, color, depth, lace};
  if (png_form_geom(f).bytes > 0x7FFFFFF0ll) return d->status;  // (Adam7 adds filter bytes: up to seven rows where there was one)
  d->ncomp = 4;
  d->color = color;
  d->max_h = f.unit();
  d->max_v = 1;
  d->mcus_x = depth;
  d->mcus_y = lace;
  d->scan_off = 8;
  d->scan_len = (int32_t)(len - 8);
  d->coef_bytes = png_form_geom(f).bytes;
  return (d->status = DINO_IMG_OK);
}

// convert("RGB") of pixel k of the reconstructed unit `v` (byte 0 of the unit in bits 0..7):
// a unit is one pixel at depths 8 and 16 (k = 0) and 8 / depth pixels of one byte below 8.
DHD void png_form_to_rgb(int color, int depth, uint64_t v, int k, const uint8_t* pal, uint8_t* rgb) {
  if (depth < 8) {
    const int s = ((int)v >> (8 - depth * (k + 1))) & ((1 << depth) - 1);
    if (color == 3) {
      rgb[0] = pal[3 * s], rgb[1] = pal[3 * s + 1], rgb[2] = pal[3 * s + 2];
    } else {
      rgb[0] = rgb[1] = rgb[2] = (uint8_t)(s * (depth == 1 ? 255 : depth == 2 ? 85 : 17));
    }
  } else if (depth == 8) {
    const uint8_t px[4] = {(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16), (uint8_t)(v >> 24)};
    png_to_rgb(color, px, pal, rgb);
  } else if (color == 2 || color == 6) {  // the high byte of each sample
    rgb[0] = (uint8_t)v, rgb[1] = (uint8_t)(v >> 16), rgb[2] = (uint8_t)(v >> 32);
  } else if (color == 4) {
    rgb[0] = rgb[1] = rgb[2] = (uint8_t)v;
  } else {  // I;16 -> RGB clips
    const int s = (((int)v & 255) << 8) | ((int)(v >> 8) & 255);
    rgb[0] = rgb[1] = rgb[2] = (uint8_t)(s > 255 ? 255 : s);
  }
}

// Where pixel xp of row yp of a pass lands in the W-wide image.
DHD int64_t png_form_dest(const PngPass& s, int W, int yp, int xp) {
  return (int64_t)(s.y0 + yp * s.dy) * W + s.x0 + xp * s.dx;
}

// The host's order of work over the inflated bytes of all passes: row after row, the filters
// reversed in place, every pixel to its final place.  False on a filter byte above 4.
inline bool png_forms_unfilter_rows(uint8_t* inf, const PngForm& f, const uint8_t* pal, uint8_t* rgb) {
  const int u = f.unit(), per = f.depth < 8 ? 8 / f.depth : 1;
  const int rows = png_form_geom(f).rows;
  for (int r = 0; r < rows; ++r) {
    const PngRowAt a = png_form_row(f, r);
    const int rb = a.pass.rb;
    uint8_t* row = inf + a.off + 1;
    const uint8_t* up = a.yp ? row - (1 + rb) : nullptr;
    const int ft = row[-1];
    if (ft > 4) return false;
    for (int i = 0; i < rb; ++i) {
      const int x = i >= u ? row[i - u] : 0, b = up ? up[i] : 0, c = up && i >= u ? up[i - u] : 0;
      row[i] = (uint8_t)(row[i] + png_predict(ft, x, b, c));
    }
    for (int i = 0; i < rb / u; ++i) {
      uint64_t v = 0;
      for (int c = 0; c < u; ++c) v |= (uint64_t)row[i * u + c] << (8 * c);
      for (int k = 0; k < per && i * per + k < a.pass.w; ++k)
        png_form_to_rgb(f.color, f.depth, v, k, pal, rgb + png_form_dest(a.pass, f.W, a.yp, i * per + k) * 3);
    }
  }
  return true;
}

}  // namespace dino
