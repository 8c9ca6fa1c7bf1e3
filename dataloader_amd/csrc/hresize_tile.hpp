// hresize_tile.hpp — tile shape of the horizontal resample pass (k_hresize): pure integer
// functions of (S, crop width, taps), shared by the kernels (kernels.hip) and the
// test-only host emulator, which sweeps them to aim the tests at every shape's first and
// last crop width.
#pragma once

#include "common.hpp"

namespace dino {

// LDS of k_hresize: taps (when they fit in kHresizeTapLds) + planar rows of one band.
constexpr int kHresizeLds = 26 * 1024;

constexpr int kHresizeMinRows = 8;  // rows per band the slice width is chosen for
constexpr int kHrBandsPerItem = 8;  // row bands of one slice per work item
constexpr int kHrDirectItems = 4;  // work items of a direct-path view

// Tile shape of a view's horizontal pass: the widest slice of outputs (all of S,
// else a multiple of 8) whose taps (16 bytes per output + 16 per output and group
// of 4 taps) and kHresizeMinRows staged rows fit kHresizeLds; then as many rows per
// band as fit (<= 16).  R = 0: even 8 outputs do not fit (direct path).
struct HrTile {
  int sw, pitch, R, R3p;
};
DHD int hresize_pitch(int S, int cw, int kh, int sw) {
  // widest source span of a slice (+ 4 for the word alignment of its first column)
  const int span = min(cw, (int)(((int64_t)sw * cw + S - 1) / S) + kh + 2) + 4;
  return ((span + 3) & ~3) + 8;  // + slack for the last group's upper word
}
// Words per staged source group: 3 R row-channel words + 2, rounded to 2 mod 4.  Even, so
// a row pair's six words are one 8-byte-aligned run; 2 mod 4, so the row pairs that the
// lanes of a ds_read_b64 group read at distinct source groups k fall on distinct bank
// pairs (k R3p mod 64): with R = 10 or 14 (R3p 32 / 44) up to 16-way conflicts, 52 % of
// the kernel's LDS cycles (SQ_LDS_BANK_CONFLICT, profiles/r05_c2_lds.txt).
DHD int hresize_r3p(int R) {
  const int r = 3 * R + 2;
  return (r & 3) == 0 ? r + 2 : r;
}
// LDS bytes of a band of R rows: (pitch / 4) source words x R3p row-channel words,
// plus room for the over-read of the last output's zero-tap groups (ng_max words).
DHD int hresize_rows_bytes(int pitch, int R, int ng_max) {
  return (pitch / 4 + ng_max + 1) * hresize_r3p(R) * 4;
}
DHD HrTile hresize_tile(int S, int cw, int kh) {
  const int ng_max = (kh + 3) / 4;
  const int tap_bytes = 16 * (1 + (ng_max | 1));
  HrTile t{0, 0, 0, 0};
  int sw = S;
  while (tap_bytes * sw + hresize_rows_bytes(hresize_pitch(S, cw, kh, sw), kHresizeMinRows, ng_max) > kHresizeLds) {
    sw = sw == S ? ((S - 1) & ~7) : sw - 8;
    if (sw < 8) return t;
  }
  t.sw = sw;
  t.pitch = hresize_pitch(S, cw, kh, sw);
  int R = 16;
  while (R > kHresizeMinRows && tap_bytes * sw + hresize_rows_bytes(t.pitch, R, ng_max) > kHresizeLds) R -= 2;
  t.R = R;
  t.R3p = hresize_r3p(R);
  return t;
}

// Work items of a view's horizontal pass (k_vsizes): kHrBandsPerItem row bands of one
// slice each, so that a batch of mixed crop sizes spreads over the persistent grid in
// pieces of similar size (a large crop's view is many items, a small one's few).
DHD int hr_view_chunks(int S, int cw, int ch, int kh) {
  const HrTile t = hresize_tile(S, cw, kh);
  if (t.R < 1) return kHrDirectItems;
  const int nsl = (S + t.sw - 1) / t.sw, nbands = (ch + t.R - 1) / t.R;
  return nsl * ((nbands + kHrBandsPerItem - 1) / kHrBandsPerItem);
}

}  // namespace dino
