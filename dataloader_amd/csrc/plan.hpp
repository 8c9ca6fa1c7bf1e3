// plan.hpp — workspace planning shared by k_plan / k_vplan (device) and the host
// probe dino_probe (capi.hip), so that the host computes exactly the bytes the
// kernels will ask for and can grow the workspaces before launching a batch.
#pragma once

#include "kernels.hpp"
#include "progressive.hpp"
#include "png_parse.hpp"
#include "pscan.hpp"
#include "lscan.hpp"
#include "resize.hpp"
#include "augment.hpp"

namespace dino {

// Per-lane state of the speculative decode (global, k_huff1 -> k_huff2 -> k_huff3).
struct LaneRec {
  HState S;       // start state used by the lane's current decode
  RangeOut R;     // its result
  RangeOut R1;    // result of the first (guessed-state) decode, for checkpoint syncs
  int32_t ncp;    // checkpoints recorded by the first decode
  int32_t blk0;   // first block the lane emits (k_huff2 scan)
  HState W;       // k_huff2 scratch: wanted start state
  int32_t pad;
};
static_assert(sizeof(LaneRec) == 68, "LaneRec layout");

// Lanes reserved for the speculative Huffman decode (restart images decode per interval).
DHD int32_t huff_lanes_cap(const ImgDesc& d) {
  if (d.restart_interval > 0 || d.kind != 0) return 0;
  const int64_t nbits = ((int64_t)d.scan_len + 64) * 8;  // >= the destuffed stream
  const int64_t seg = nbits <= kHuffSegBits ? 1 : (nbits + kHuffSegBits - 1) / kHuffSegBits;
  return (int32_t)(seg * kHuffThreads);
}

// Sparse entry capacity per block (see SparseSink): 63 u32 entries + 1 alignment halfword.
constexpr int kEntHalfwordsPerBlock = 128;

// Byte sizes of an image's workspace regions, in chunk order: destuffed entropy
// bytes, restart offsets, coefficients (baseline: sparse entries, 128 halfwords of
// capacity per block, see SparseSink; kind 1: the dense int16 buffer), block info
// (uint2 per block), component planes, RGB, speculative checkpoints, Huffman
// tables, lane records, destuff part counts.
struct ChunkSizes {
  int64_t ent, rst, coef, binfo, plane, rgb, cps, htab, hlane, dspart, tail;
  DHD int64_t sum() const { return ent + rst + coef + binfo + plane + rgb + cps + htab + hlane + dspart; }
  DHD int64_t total() const { return sum() + tail; }
};

// Image areas start 256-byte aligned (tail pads each image), and so does the sparse entry
// area (rst pads ent + rst): a lane's entry region starts at a multiple of 256 bytes in
// memory too (SparseSink stores groups of up to 64 bytes aligned to their size).
DHD int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }
DHD ChunkSizes chunk_finish(ChunkSizes z) {
  z.tail = align256(z.sum()) - z.sum();
  return z;
}

// Destuff work items of an image: 32 KiB parts of its scan (>= 1, so that the
// descriptor is always completed by k_destuff_write); none for kinds 1 and 2.
constexpr int kDsPartBytes = 32 * 1024;
DHD int ds_parts(const ImgDesc& d) {
  if (d.status != DINO_IMG_OK || d.kind != 0) return 0;
  const int n = (d.scan_len + 16 + kDsPartBytes - 1) / kDsPartBytes;
  return n > 1 ? n : 1;
}

// What part `part` of an image's ds_items parts does in k_destuff_write.  The scan has n
// bytes, the first of them `lead` bytes into part 0 (part p covers scan indices
// [p kDsPartBytes - lead, (p + 1) kDsPartBytes - lead)); E is the scan index of the first
// terminating marker, n when there is none.  A part writes the kept bytes of its range
// below E.  Exactly one part completes the descriptor (ent_len, n_rst, terminated, the
// TRUNCATED status, the 64-byte zero pad): the part whose range holds E, or the image's
// last part when nothing terminates the scan; it does so even when it writes no byte (E
// on its first byte; a last part past the end of a scan cut short).  ds_parts sizes from
// scan_len + 16 >= E + lead + 1, so the part that holds E exists.
struct DsRole {
  bool writes, finalises;
};
DHD DsRole ds_part_role(int part, int lead, int n, int E, int ds_items) {
  const int k0 = part * kDsPartBytes - lead, k1 = k0 + kDsPartBytes;
  return {k0 < E, E < n ? (E >= k0 && E < k1) : part == ds_items - 1};
}

// kPng: the caller may hold PNG images (kind 4).  k_plan of a context without dino_ctx_set_png is
// instantiated without them and stays the code it was.
template <bool kPng = true>
DHD ChunkSizes image_chunk_bytes(const ImgDesc& d) {
  ChunkSizes z{};
  if (d.status != DINO_IMG_OK) return z;
  z.rgb = align16((int64_t)d.width * d.height * 3 + 16);
  if (d.kind == 2) return chunk_finish(z);
  if (kPng && d.kind == kPngKind) {  // the joined zlib stream, one carried row, the filtered rows, the palette
    z.ent = align16((int64_t)d.scan_len + 64);
    z.coef = align16((int64_t)d.width * 4 + 16);
    z.plane = align16(png_inflated_bytes(d) + 64);
    z.htab = kPngPalBytes;
    return chunk_finish(z);
  }
  // the planes hold a byte per coefficient of the dense int16 layout coef_bytes counts
  // (jpeg_parse.hpp: 64 and 128 bytes a block of every component's bw x bh grid)
  z.plane = align16(d.coef_bytes / 2);
  if (d.kind == 1) {
    z.ent = align16((int64_t)d.scan_len + 64);  // each scan's destuffed bytes (k_pscan)
    z.coef = align16(d.coef_bytes);
    z.binfo = (d.coef_bytes / 128) * kLSideBytes;  // side records of the lane decoder (lscan.hpp)
    z.htab = kPRegionBytes;  // scan list + decoder tables (k_pwalk -> k_pscan)
    return chunk_finish(z);
  }
  z.ent = align16((int64_t)d.scan_len + 64);
  z.rst = align256(z.ent + 4 * ((int64_t)d.n_rst_max + 1)) - z.ent;
  z.coef = (int64_t)d.total_blocks * kEntHalfwordsPerBlock * 2;
  z.binfo = align16((int64_t)d.total_blocks * 8);
  const int64_t lanes = huff_lanes_cap(d);
  z.cps = lanes * kHuffCheckpoints * (int64_t)sizeof(Checkpoint);
  z.htab = align16((int64_t)sizeof(HuffTables));
  z.hlane = align16(lanes * (int64_t)sizeof(LaneRec));
  z.dspart = 16 * (int64_t)ds_parts(d);
  return chunk_finish(z);
}

// A restart image that k_htab moves to the coefficient-buffer path keeps its baseline
// table area: its one scan needs at most 4 DC + 4 AC tables there.
static_assert(((int64_t)sizeof(HuffTables) - kPTabOff) / (int64_t)sizeof(PTab) >= 8, "switched restart images");

// The two scratch layouts of the augment workspace.  These functions state where a table
// lives: the planners size and place with them and the kernels take their pointers from
// them.  The one deliberate second spelling is view_vcoefs below (vert_apply's vb and vt,
// kept as int32 steps for k_vert's sake and held equal to view_tables by
// tests/test_scratch_layout_cpu.py).  Each is written once over a position type P: a
// byte pointer into the workspace (kernels: the members are the tables' addresses) or
// int64_t from 0 (planners, host, tests: byte offsets).
//
// A view's coefficient tables, from ViewPlan::rcoef_off: hb[S][2] and vb[S][2] (first
// source index, tap count per output), ht[S][kh] and vt[S][kv] (int32 taps), then, 16-byte
// aligned, the horizontal taps in the signed-dot4 layout (k_hresize): hx[S], per output x
// an int4 {xmin, groups, corr, 0}, and hg[(kh + 3) / 4][S], groups of 4 taps as signed
// base-256 digit planes (both empty when kh == 0).
template <typename P>
struct ViewTables {
  P hb, vb, ht, vt, hx, hg, end;
};
template <typename P>
DHD ViewTables<P> view_tables(P at, int S, int kh, int kv) {
  ViewTables<P> t;
  t.hb = at;
  t.vb = at + (int64_t)S * 8;
  t.ht = at + (int64_t)S * 16;
  t.vt = t.ht + (int64_t)S * kh * 4;
  t.hx = at + align16((int64_t)S * (4 + kh + kv) * 4);
  t.hg = t.hx + (kh ? (int64_t)S * 16 : 0);
  t.end = t.hg + (kh ? (int64_t)S * 16 * ((kh + 3) / 4) : 0);
  return t;
}

// The vertical pass's tables (vb, vt) of the block at `tab`, for vert_apply (k_vert,
// k_vfinal).  The same positions as view_tables(tab, ...).vb and .vt (tests/
// test_scratch_layout_cpu.py holds the two together), spelled as int32 steps: k_vert's
// time follows the code this compiles to (with view_tables here its prologue grew by five
// scalar instructions and the kernel ran 7 % slower, 0.254 -> 0.272 ms).
DHD CoefView view_vcoefs(const uint8_t* tab, int S, int kh, int kv) {
  const int32_t* cbase = (const int32_t*)tab;
  return {cbase + 2 * S, cbase + 4 * S + (int64_t)S * kh, kv};
}

// Augment scratch of one view as byte offsets from ViewPlan::htmp_off: the horizontal
// pass's rows (planar u8 [3][crop_h][S], only when kh != 0), then the tables above
// (ViewPlan::rcoef_off is htmp_off + hb).
struct ViewScratch {
  int64_t htmp, hb, vb, ht, vt, hx, hg, total;
};
DHD ViewScratch view_scratch(int S, int crop_h, int kh, int kv) {
  const int64_t hb = kh ? align16((int64_t)crop_h * S * 3) : 0;
  const ViewTables<int64_t> t = view_tables(hb, S, kh, kv);
  return {0, t.hb, t.vb, t.ht, t.vt, t.hx, t.hg, t.end};
}

// Upper bound of a view's scratch over every crop of a W x H image (crop sides <= the
// image's; the tap count grows with the crop side).  The probes state it for BICUBIC; for a
// context with another filter the caller multiplies it by resample_bound_scale.
DHD int64_t view_scratch_bound(int S, int W, int H, int filter = kBicubic) {
  const int kh = resample_ksize(W > S ? W : S, S, filter), kv = resample_ksize(H > S ? H : S, S, filter);
  return view_scratch(S, H, kh, kv).total;
}

// Factor by which a filter's scratch can exceed BICUBIC's for the same sizes: the support
// ratio rounded up.  With u = ceil(2 fs), BICUBIC has k = 2 u + 1 taps and LANCZOS
// 2 ceil(3 fs) + 1 <= 2 (2 u) + 1 < 2 k, and its groups of 4 taps floor((2 k + 3) / 4) <=
// 2 floor((k + 3) / 4) for odd k >= 5; the rows of the horizontal pass do not depend on the
// filter, and every table's size is linear in its tap or group count plus a constant.  The
// filters of support <= 2 never have more taps than BICUBIC.
DHD int resample_bound_scale(int filter) { return (resample_support2(filter) + 3) / 4; }

// Decode-only scratch of one image (k_dplan), from ViewPlan::rcoef_off: hb[ow][2],
// ht[ow][kh], then vb[oh][2], vt[oh][kv], then the horizontal pass's rows (planar u8
// [3][H][ow], only when kh != 0; ViewPlan::htmp_off is their position).
template <typename P>
struct DecHTables {  // the horizontal pass's part (k_dhpass), which does not depend on oh
  P hb, ht;
};
template <typename P>
DHD DecHTables<P> dec_htables(P at, int ow) {
  return {at, at + (int64_t)ow * 8};
}
template <typename P>
struct DecScratch {
  P hb, ht, vb, vt, htmp, total;
};
template <typename P>
DHD DecScratch<P> dec_scratch(P at, int ow, int oh, int H, int kh, int kv) {
  const DecHTables<P> h = dec_htables(at, ow);
  DecScratch<P> t;
  t.hb = h.hb;
  t.ht = h.ht;
  t.vb = at + align16((int64_t)ow * (2 + kh) * 4);
  t.vt = t.vb + (int64_t)oh * 8;
  t.htmp = t.vb + align16((int64_t)oh * (2 + kv) * 4);
  t.total = t.htmp + (kh ? align16((int64_t)H * ow * 3) : 0);
  return t;
}

}  // namespace dino
