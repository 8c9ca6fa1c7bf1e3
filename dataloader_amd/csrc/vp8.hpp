// vp8.hpp — the lossy WebP bitstream (VP8 key frames, RFC 6386), written once for the host model
// (dino_debug_vp8_decode, dino_probe_webp_forms) and for k_vp8_tok / k_vp8_rec / k_vp8_rgb, to
// the letter of libwebp's decoder, which is what Pillow runs: its bool decoder and end-of-data
// rule, its dequantisation and int16 stores, its inverse transforms (the full 4x4 transform in
// 16-bit wrapping arithmetic, as its SSE2 path computes it, the DC-only and three-coefficient
// forms in 32 bits), its border rules, loop filters, fancy upsampler and 14-bit YUV -> RGB.
//
// The code is SPMD over `nl` lanes that run the same control flow (nl = 1 on the host, the 64
// lanes of a wave on the device): everything serial (bool decoder, header, modes, tokens) is
// uniform, the lane-parallel parts are loops `for (i = io.lane; i < n; i += io.nl)` with
// io.sync() between dependent steps.
//
// A file is kind 7 when vp8_walk verifies its container (as webp_parse.hpp does for VP8L) and the
// frame's 10 bytes.  The frame header's bool-coded part then declines (kWebpDecline: Pillow
// decides) what no encoder at hand produces: several token partitions, use_lf_delta = 1.  The
// first partition or the token partition running past its end is DINO_IMG_CORRUPT (libwebp
// fails the frame, Pillow raises); everything else decodes to what libwebp gives.
#pragma once

#include "vp8_tables.hpp"
#include "webp_parse.hpp"

namespace dino {

constexpr int kVp8Kind = 7;  // ImgDesc::kind of a lossy WebP the device decodes

// Frame record at the head of the coefficient region (k_vp8_tok -> k_vp8_rec).
struct Vp8Frame {
  int16_t dq[4][6];      // per segment: y1 dc, ac; y2 dc, ac; uv dc, ac
  uint8_t limit[4][2];   // per segment and "is 4x4-mode": 2 level + ilevel, 0 = not filtered
  uint8_t ilevel[4][2];
  uint8_t hev[4][2];
  uint8_t filter_type;   // 0 none, 1 simple, 2 complex
  uint8_t use_segment, update_map, use_skip, skip_p;
  uint8_t seg_p[3];
  int32_t cover[8];      // coverage (tests): 16x16 modes, sub-block modes, chroma modes, filter types,
                         // hev thresholds of filtered macroblocks, segments off / on, a skip, categories 3..6
  int32_t pad[4];
};
static_assert(sizeof(Vp8Frame) == 128, "Vp8Frame layout");

// One macroblock's record (binfo region).
struct Vp8Mb {
  uint8_t modes[16];  // the 16 sub-block modes, or the 16x16 mode in modes[0]
  uint8_t uvmode, segment, is_i4, inner;  // inner: the inner edges are filtered
  uint32_t nzy;       // 2 bits a luma block: 0 no coefficient, 1 DC only, 2 the first three, 3 more
  uint32_t nzuv;      // the same for U (bits 0..7) and V (8..15)
  uint32_t pad;
};
static_assert(sizeof(Vp8Mb) == 32, "Vp8Mb layout");

DHD int vp8_mbs(int side) { return (side + 15) >> 4; }
DHD int64_t vp8_nmb(int w, int h) { return (int64_t)vp8_mbs(w) * vp8_mbs(h); }
// Region bytes of a kind-7 image (plan.hpp): frame record + 384 int16 a macroblock; a Vp8Mb each;
// Y at pitch 16 mbw, then U and V at pitch 8 mbw.
DHD int64_t vp8_coef_bytes(int w, int h) { return (int64_t)sizeof(Vp8Frame) + 768 * vp8_nmb(w, h); }
DHD int64_t vp8_binfo_bytes(int w, int h) { return (int64_t)sizeof(Vp8Mb) * vp8_nmb(w, h); }
DHD int64_t vp8_plane_bytes(int w, int h) { return align16(384 * vp8_nmb(w, h) + 64); }

// The container walk of a lossy file: DINO_IMG_OK (w: the VP8 chunk's payload and the frame's
// size) or kWebpDecline.  One VP8 chunk, alone or in a VP8X without ALPH / ANIM / ANMF / EXIF and
// with the frame's canvas; a shown key frame whose first partition ends inside the chunk before
// its last byte; the start code; sides above 0.  The scale bits are ignored, as libwebp does.
DHD int vp8_walk(const uint8_t* p, int64_t len, WebpWalk* w) {
  w->off = w->len = w->width = w->height = 0;
  if (!webp_signature(p, len) || len > 0x7FFFFFF0ll) return kWebpDecline;
  const int64_t end = (int64_t)rd32le(p + 4) + 8;
  if (end != len || (end & 1)) return kWebpDecline;
  int64_t pos = 12;
  bool vp8x = false, first = true;
  int32_t cw = 0, ch = 0;
  while (pos < end) {
    if (pos + 8 > end) return kWebpDecline;
    const uint32_t cid = rd32le(p + pos);
    const int64_t n = rd32le(p + pos + 4), next = pos + 8 + n + (n & 1);
    if (next > end) return kWebpDecline;
    if (cid == webp_cid('V', 'P', '8', 'X')) {
      if (!first || n != 10 || (p[pos + 8] & 0x02)) return kWebpDecline;
      vp8x = true;
      cw = 1 + (int32_t)(p[pos + 12] | (p[pos + 13] << 8) | (p[pos + 14] << 16));
      ch = 1 + (int32_t)(p[pos + 15] | (p[pos + 16] << 8) | (p[pos + 17] << 16));
    } else if (cid == webp_cid('V', 'P', '8', ' ')) {
      if (w->len || n < 11 || (!first && !vp8x)) return kWebpDecline;
      w->off = (int32_t)(pos + 8);
      w->len = (int32_t)n;
    } else if (!vp8x || cid == webp_cid('V', 'P', '8', 'L') || cid == webp_cid('A', 'L', 'P', 'H') ||
               cid == webp_cid('A', 'N', 'I', 'M') || cid == webp_cid('A', 'N', 'M', 'F') ||
               cid == webp_cid('E', 'X', 'I', 'F')) {
      return kWebpDecline;
    }
    first = false;
    pos = next;
  }
  if (!w->len) return kWebpDecline;
  const uint8_t* q = p + w->off;
  const uint32_t tag = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
  if ((tag & 1) || ((tag >> 1) & 7) > 3 || !((tag >> 4) & 1) || 10 + (int64_t)(tag >> 5) >= w->len) return kWebpDecline;
  if (q[3] != 0x9d || q[4] != 0x01 || q[5] != 0x2a) return kWebpDecline;
  w->width = (int32_t)(q[6] | (q[7] << 8)) & 0x3FFF;
  w->height = (int32_t)(q[8] | (q[9] << 8)) & 0x3FFF;
  if (!w->width || !w->height || (vp8x && (cw != w->width || ch != w->height))) return kWebpDecline;
  return DINO_IMG_OK;
}

// The kind-7 descriptor of a file with the signature (scan_off / scan_len: the VP8 chunk's
// payload; ncomp 4 as for kinds 4 and 6).  Returns d->status.
DHD int parse_vp8_head(const uint8_t* p, int64_t len, int max_dim, ImgDesc* d) {
  WebpWalk w;
  d->status = vp8_walk(p, len, &w);
  if (d->status != DINO_IMG_OK) return d->status;
  d->kind = kVp8Kind;
  d->width = w.width;
  d->height = w.height;
  if (check_dims(d, max_dim) != DINO_IMG_OK) return d->status;
  d->ncomp = 4;
  d->color = 0;
  d->max_h = d->max_v = 1;
  d->scan_off = w.off;
  d->scan_len = w.len;
  d->coef_bytes = 0;
  return d->status;
}

DHD int vp8_clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
DHD int vp8_clamp(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
DHD int vp8_abs(int v) { return v < 0 ? -v : v; }

// libwebp's bool decoder (VP8GetBit, VP8GetSigned and VP8LoadFinalBytes, a byte at a time: the
// same bits, and the same moment at which the end is met).  `range` is the range minus one.
template <class IO>
struct Vp8Bool {
  int r;  // which of the IO's two input windows
  int64_t pos, end;
  uint32_t value, range;
  int bits;
  bool eof;
  DHD void load(IO& io) {
    if (pos < end) {
      bits += 8;
      value = io.in(r, pos++) | (value << 8);
    } else if (!eof) {
      value <<= 8;
      bits += 8;
      eof = true;
    } else {
      bits = 0;
    }
  }
  DHD void init(IO& io, int which, int64_t start, int64_t size) {
    r = which, pos = start, end = start + size, value = 0, range = 254, bits = -8, eof = false;
    load(io);
  }
  DHD int bit(IO& io, int prob) {
    if (bits < 0) load(io);
    const uint32_t split = (range * (uint32_t)prob) >> 8, v = value >> bits;
    uint32_t rg;
    int b;
    if (v > split) {
      rg = range - split;
      value -= (split + 1) << bits;
      b = 1;
    } else {
      rg = split + 1;
      b = 0;
    }
    const int shift = 7 ^ (31 - __builtin_clz(rg | 1u));
    bits -= shift;
    range = (rg << shift) - 1;
    return b;
  }
  DHD int sign(IO& io, int v) {  // VP8GetSigned: a bit at probability 1/2, always one shift
    if (bits < 0) load(io);
    const uint32_t split = range >> 1, val = value >> bits;
    const int32_t mask = (int32_t)(split - val) >> 31;
    value -= ((split + 1) & (uint32_t)mask) << bits;
    bits -= 1;
    range = (range + (uint32_t)mask) | 1u;
    return (v ^ mask) - mask;
  }
  DHD int val(IO& io, int n) {
    int v = 0;
    while (n-- > 0) v |= bit(io, 0x80) << n;
    return v;
  }
  DHD int sval(IO& io, int n) {
    const int v = val(io, n);
    return val(io, 1) ? -v : v;
  }
};

// Inverse Walsh-Hadamard transform of the Y2 block: output k (the DC of luma block k).
DHD int vp8_wht(const int16_t* in, int k) {
  const int i = k >> 2, j = k & 3;
  int t[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int a0 = in[c] + in[12 + c], a1 = in[4 + c] + in[8 + c], a2 = in[4 + c] - in[8 + c], a3 = in[c] - in[12 + c];
    t[c] = i == 0 ? a0 + a1 : i == 1 ? a3 + a2 : i == 2 ? a0 - a1 : a3 - a2;
  }
  const int dc = t[0] + 3, b0 = dc + t[3], b1 = t[1] + t[2], b2 = t[1] - t[2], b3 = dc - t[3];
  return (j == 0 ? b0 + b1 : j == 1 ? b3 + b2 : j == 2 ? b0 - b1 : b3 - b2) >> 3;
}

// The serial part: frame header, then per macroblock the modes (first partition) and the tokens
// (token partition).  IO: lane, nl, sync(), in(r, i) (byte i of the chunk's payload through
// window r, 0 outside it).  The caller gives the working memory (LDS on the device):
//   F       the frame record,
//   proba   the 1056 coefficient probabilities,
//   tmode   the modes above, four bytes a macroblock column; tnz: the non-zero flags above,
//   cbuf    400 int16: the macroblock's 384 coefficients and the Y2 block, zero between macroblocks,
//   M       the macroblock's record being built.
template <class IO>
struct Vp8Tok {
  IO& io;
  Vp8Frame& F;
  uint8_t* proba;
  uint32_t* tmode;
  uint16_t* tnz;
  int16_t* cbuf;
  Vp8Mb& M;
  Vp8Bool<IO> br, tk;
  int W, H, mbw, mbh;
  DHD Vp8Tok(IO& io_, Vp8Frame& f, uint8_t* pr, uint32_t* tm, uint16_t* tn, int16_t* cb, Vp8Mb& m)
      : io(io_), F(f), proba(pr), tmode(tm), tnz(tn), cbuf(cb), M(m) {}

  // DINO_IMG_OK, kWebpDecline or DINO_IMG_CORRUPT.  len: the chunk's bytes; cap: macroblock columns tmode / tnz hold.
  DHD int header(int64_t len, int cap) {
    const uint32_t tag = io.in(0, 0) | (io.in(0, 1) << 8) | (io.in(0, 2) << 16);
    const int64_t plen = tag >> 5;
    W = (int)(io.in(0, 6) | (io.in(0, 7) << 8)) & 0x3FFF;
    H = (int)(io.in(0, 8) | (io.in(0, 9) << 8)) & 0x3FFF;
    mbw = vp8_mbs(W), mbh = vp8_mbs(H);
    if ((tag & 1) || 10 + plen >= len || !W || !H || mbw > cap) return kWebpDecline;
    br.init(io, 0, 10, plen);
    br.val(io, 2);  // colour space, clamping type: libwebp ignores both
    for (int k = io.lane; k < (int)(sizeof(Vp8Frame) / 4); k += io.nl) ((int32_t*)&F)[k] = 0;
    io.sync();
    int quant[4] = {0, 0, 0, 0}, fstr[4] = {0, 0, 0, 0}, absolute = 1;
    int use_segment = br.val(io, 1), update_map = 0;
    uint8_t sp[3] = {255, 255, 255};
    if (use_segment) {
      update_map = br.val(io, 1);
      if (br.val(io, 1)) {
        absolute = br.val(io, 1);
        for (int s = 0; s < 4; ++s) quant[s] = br.val(io, 1) ? br.sval(io, 7) : 0;
        for (int s = 0; s < 4; ++s) fstr[s] = br.val(io, 1) ? br.sval(io, 6) : 0;
      }
      if (update_map)
        for (int s = 0; s < 3; ++s) sp[s] = br.val(io, 1) ? (uint8_t)br.val(io, 8) : 255;
    }
    if (br.eof) return DINO_IMG_CORRUPT;
    const int simple = br.val(io, 1), level = br.val(io, 6), sharp = br.val(io, 3), lf_delta = br.val(io, 1);
    if (br.eof) return DINO_IMG_CORRUPT;
    if (lf_delta) return kWebpDecline;
    if (br.val(io, 2) != 0) return kWebpDecline;  // more than one token partition
    tk.init(io, 1, 10 + plen, len - 10 - plen);
    const int base_q = br.val(io, 7);
    int dqd[5];
    for (int k = 0; k < 5; ++k) dqd[k] = br.val(io, 1) ? br.sval(io, 4) : 0;  // y1 dc, y2 dc, y2 ac, uv dc, uv ac
    const int ftype = level == 0 ? 0 : simple ? 1 : 2;
    if (io.lane == 0) {
      F.filter_type = (uint8_t)ftype, F.use_segment = (uint8_t)use_segment, F.update_map = (uint8_t)update_map;
      for (int s = 0; s < 3; ++s) F.seg_p[s] = sp[s];
      F.cover[3] = 1 << ftype;
      F.cover[5] = use_segment ? 2 : 1;
    }
    for (int s = 0; s < 4; ++s) {
      int q = use_segment ? quant[s] + (absolute ? 0 : base_q) : base_q;
      int y2ac = (kVp8AcQ[vp8_clamp(q + dqd[2], 0, 127)] * 101581) >> 16;
      if (y2ac < 8) y2ac = 8;
      int lv = use_segment ? fstr[s] + (absolute ? 0 : level) : level;
      if (io.lane == 0) {
        F.dq[s][0] = kVp8DcQ[vp8_clamp(q + dqd[0], 0, 127)];
        F.dq[s][1] = (int16_t)kVp8AcQ[vp8_clamp(q, 0, 127)];
        F.dq[s][2] = (int16_t)(kVp8DcQ[vp8_clamp(q + dqd[1], 0, 127)] * 2);
        F.dq[s][3] = (int16_t)y2ac;
        F.dq[s][4] = kVp8DcQ[vp8_clamp(q + dqd[3], 0, 117)];
        F.dq[s][5] = (int16_t)kVp8AcQ[vp8_clamp(q + dqd[4], 0, 127)];
        lv = vp8_clamp(lv, 0, 63);  // (per "is 4x4-mode" only through use_lf_delta, which is declined)
        int il = lv;
        if (sharp > 0) {
          il >>= sharp > 4 ? 2 : 1;
          if (il > 9 - sharp) il = 9 - sharp;
        }
        if (il < 1) il = 1;
        for (int k = 0; k < 2; ++k) {
          F.limit[s][k] = (uint8_t)(lv > 0 && ftype ? 2 * lv + il : 0);
          F.ilevel[s][k] = (uint8_t)il;
          F.hev[s][k] = (uint8_t)(lv >= 40 ? 2 : lv >= 15 ? 1 : 0);
        }
      }
    }
    br.val(io, 1);  // update_proba: ignored in a key frame
    for (int k = 0; k < 1056; ++k) {
      const int v = br.bit(io, kVp8CoefUpdate[k]) ? br.val(io, 8) : kVp8CoefProba0[k];
      if (io.lane == 0) proba[k] = (uint8_t)v;
    }
    const int use_skip = br.val(io, 1), skip_p = use_skip ? br.val(io, 8) : 0;
    if (io.lane == 0) F.use_skip = (uint8_t)use_skip, F.skip_p = (uint8_t)skip_p;
    for (int k = io.lane; k < mbw; k += io.nl) tmode[k] = 0, tnz[k] = 0;
    for (int k = io.lane; k < 200; k += io.nl) ((int32_t*)cbuf)[k] = 0;
    io.sync();
    return DINO_IMG_OK;
  }
  DHD int large(const uint8_t* p, int& cats) {
    if (!tk.bit(io, p[3])) return !tk.bit(io, p[4]) ? 2 : 3 + tk.bit(io, p[5]);
    if (!tk.bit(io, p[6])) {
      if (!tk.bit(io, p[7])) return 5 + tk.bit(io, 159);
      const int v = 7 + 2 * tk.bit(io, 165);
      return v + tk.bit(io, 145);
    }
    const int b1 = tk.bit(io, p[8]), b0 = tk.bit(io, p[9 + b1]), cat = 2 * b1 + b0;
    int v = 0;
    for (const uint8_t* t = kVp8Cat[cat]; *t; ++t) v += v + tk.bit(io, *t);
    cats |= 1 << cat;
    return v + 3 + (8 << cat);
  }

  // libwebp's GetCoeffs: the block's tokens from position n on -> the position after the last
  // non-zero one.  Values are dequantised and truncated to int16 where they are stored.
  DHD int coeffs(int type, int ctx, int dq0, int dq1, int n, int16_t* out, int& cats) {
    const uint8_t* p = proba + ((type * 8 + kVp8Bands[n]) * 3 + ctx) * 11;
    for (; n < 16; ++n) {
      if (!tk.bit(io, p[0])) return n;
      while (!tk.bit(io, p[1])) {
        p = proba + (type * 8 + kVp8Bands[++n]) * 33;
        if (n == 16) return 16;
      }
      const uint8_t* pn = proba + (type * 8 + kVp8Bands[n + 1]) * 33;
      int v;
      if (!tk.bit(io, p[2])) {
        v = 1;
        p = pn + 11;
      } else {
        v = large(p, cats);
        p = pn + 22;
      }
      const int16_t c = (int16_t)(tk.sign(io, v) * (n > 0 ? dq1 : dq0));
      if (io.lane == 0) out[kVp8Zigzag[n]] = c;
    }
    return 16;
  }
  DHD static uint32_t nz_code(uint32_t acc, int nz, bool dc_nz) { return (acc << 2) | (nz > 3 ? 3u : nz > 1 ? 2u : (uint32_t)dc_nz); }

  // Every macroblock in raster order: coefficients to coef (384 int16 each, after the frame
  // record), records to mbs.  False: a partition ran past its end.
  DHD bool body(int16_t* coef, Vp8Mb* mbs) {
    int cov_y = 0, cov_b = 0, cov_uv = 0, cov_hev = 0, cov_skip = 0, cats = 0;
    for (int my = 0; my < mbh; ++my) {
      uint32_t lmode = 0, lnz = 0;  // modes and non-zero flags to the left (bit 8: the Y2 block's)
      for (int mx = 0; mx < mbw; ++mx) {
        // --- modes (first partition)
        int seg = 0;
        if (F.update_map) seg = !br.bit(io, F.seg_p[0]) ? br.bit(io, F.seg_p[1]) : br.bit(io, F.seg_p[2]) + 2;
        const int skip = F.use_skip ? br.bit(io, F.skip_p) : 0;
        const int is_i4 = !br.bit(io, 145);
        if (!is_i4) {
          const int ym = br.bit(io, 156) ? (br.bit(io, 128) ? 1 : 3) : (br.bit(io, 163) ? 2 : 0);
          if (io.lane == 0) M.modes[0] = (uint8_t)ym, tmode[mx] = 0x01010101u * ym;
          lmode = 0x01010101u * ym;
          cov_y |= 1 << ym;
        } else {
          uint32_t top = tmode[mx];
          for (int y = 0; y < 4; ++y) {
            int ym = (lmode >> (8 * y)) & 255;
            for (int x = 0; x < 4; ++x) {
              const uint8_t* prob = kVp8BModeProba + (((top >> (8 * x)) & 255) * 10 + ym) * 9;
              int i = kVp8BModeTree[br.bit(io, prob[0])];
              while (i > 0) i = kVp8BModeTree[2 * i + br.bit(io, prob[i])];
              ym = -i;
              top = (top & ~(255u << (8 * x))) | ((uint32_t)ym << (8 * x));
              if (io.lane == 0) M.modes[4 * y + x] = (uint8_t)ym;
              cov_b |= 1 << ym;
            }
            lmode = (lmode & ~(255u << (8 * y))) | ((uint32_t)ym << (8 * y));
          }
          io.sync();
          if (io.lane == 0) tmode[mx] = top;
        }
        const int uvm = !br.bit(io, 142) ? 0 : !br.bit(io, 114) ? 2 : br.bit(io, 183) ? 1 : 3;
        cov_uv |= 1 << uvm;
        cov_skip |= skip;
        io.sync();  // (tmode[mx], tnz[mx] read below and before)
        // --- tokens (token partition)
        uint32_t nzy = 0, nzuv = 0;
        const uint32_t tn = tnz[mx];
        uint32_t out_t = tn, out_l = lnz;
        if (!skip) {
          const int16_t* dq = F.dq[seg];
          int16_t* dst = cbuf;
          int first = 0, type = 3;
          uint32_t t_dc = tn & 0x100, l_dc = lnz & 0x100;
          if (!is_i4) {
            const int nz = coeffs(1, (int)((tn >> 8) & 1) + (int)((lnz >> 8) & 1), dq[2], dq[3], 0, cbuf + 384, cats);
            t_dc = l_dc = nz > 0 ? 0x100u : 0u;
            io.sync();
            for (int k = io.lane; k < 16; k += io.nl) cbuf[16 * k] = (int16_t)vp8_wht(cbuf + 384, k);
            io.sync();
            first = 1, type = 0;
          }
          uint32_t t4 = tn & 15, l4 = lnz & 15;
          for (int y = 0; y < 4; ++y) {
            int l = l4 & 1;
            uint32_t acc = 0;
            for (int x = 0; x < 4; ++x) {
              const int nz = coeffs(type, l + (int)(t4 & 1), dq[0], dq[1], first, dst, cats);
              l = nz > first;
              t4 = (t4 >> 1) | ((uint32_t)l << 7);
              io.sync();
              acc = nz_code(acc, nz, dst[0] != 0);
              dst += 16;
            }
            t4 >>= 4;
            l4 = (l4 >> 1) | ((uint32_t)l << 7);
            nzy = (nzy << 8) | acc;
          }
          uint32_t ot = t4, ol = l4 >> 4;
          for (int ch = 0; ch < 4; ch += 2) {
            uint32_t acc = 0, t2 = (tn & 255) >> (4 + ch), l2 = (lnz & 255) >> (4 + ch);
            for (int y = 0; y < 2; ++y) {
              int l = l2 & 1;
              for (int x = 0; x < 2; ++x) {
                const int nz = coeffs(2, l + (int)(t2 & 1), dq[4], dq[5], 0, dst, cats);
                l = nz > 0;
                t2 = (t2 >> 1) | ((uint32_t)l << 3);
                io.sync();
                acc = nz_code(acc, nz, dst[0] != 0);
                dst += 16;
              }
              t2 >>= 2;
              l2 = (l2 >> 1) | ((uint32_t)l << 5);
            }
            nzuv |= acc << (4 * ch);
            ot |= (t2 << 4) << ch;
            ol |= (l2 & 0xf0) << ch;
          }
          out_t = (ot & 255) | t_dc, out_l = (ol & 255) | l_dc;
        } else {
          out_t = is_i4 ? (tn & 0x100) : 0, out_l = is_i4 ? (lnz & 0x100) : 0;
        }
        lnz = out_l;
        const int k4 = is_i4 ? 1 : 0;
        if (F.filter_type == 2 && F.limit[seg][k4]) cov_hev |= 1 << F.hev[seg][k4];
        if (io.lane == 0) {
          tnz[mx] = (uint16_t)out_t;
          M.uvmode = (uint8_t)uvm, M.segment = (uint8_t)seg, M.is_i4 = (uint8_t)is_i4;
          M.inner = (uint8_t)(is_i4 || (nzy | nzuv) != 0);
          M.nzy = nzy, M.nzuv = nzuv, M.pad = 0;
        }
        io.sync();
        // --- the lane-parallel tail: the macroblock's coefficients and record to the workspace
        const int64_t mb = (int64_t)my * mbw + mx;
        int32_t* cw = (int32_t*)(coef + 384 * mb);
        for (int k = io.lane; k < 192; k += io.nl) cw[k] = ((const int32_t*)cbuf)[k];
        for (int k = io.lane; k < 8; k += io.nl) ((int32_t*)(mbs + mb))[k] = ((const int32_t*)&M)[k];
        io.sync();
        for (int k = io.lane; k < 200; k += io.nl) ((int32_t*)cbuf)[k] = 0;
        io.sync();
      }
    }
    if (io.lane == 0) {
      F.cover[0] = cov_y, F.cover[1] = cov_b, F.cover[2] = cov_uv, F.cover[4] = cov_hev, F.cover[6] = cov_skip;
      F.cover[7] = cats;
    }
    io.sync();
    return !br.eof && !tk.eof;
  }
};

// --- reconstruction ---

// libwebp's 4x4 inverse transform of block `in` -> 16 residuals.  wrap: in 16-bit wrapping
// arithmetic (its SSE2 path, taken for a block with more than three coefficients and for a chroma
// plane that holds such a block); otherwise in 32 bits (its DC-only and three-coefficient forms,
// which are this arithmetic).  The two differ only where a damaged stream overflows 16 bits.
template <bool kWrap>
DHD void vp8_itransform(const int16_t* in, int16_t* out) {
#define VP8_W(x) (kWrap ? (int)(int16_t)(x) : (int)(x))
#define VP8_MUL1(a) VP8_W((((a) * 20091) >> 16) + (a))
#define VP8_MUL2(a) VP8_W(((a) * 35468) >> 16)
  int t[16];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int i0 = in[i], i1 = in[4 + i], i2 = in[8 + i], i3 = in[12 + i];
    const int a = VP8_W(i0 + i2), b = VP8_W(i0 - i2);
    const int c = VP8_W(VP8_MUL2(i1) - VP8_MUL1(i3)), d = VP8_W(VP8_MUL1(i1) + VP8_MUL2(i3));
    t[4 * i] = VP8_W(a + d), t[4 * i + 1] = VP8_W(b + c), t[4 * i + 2] = VP8_W(b - c), t[4 * i + 3] = VP8_W(a - d);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int dc = VP8_W(t[i] + 4), a = VP8_W(dc + t[8 + i]), b = VP8_W(dc - t[8 + i]);
    const int c = VP8_W(VP8_MUL2(t[4 + i]) - VP8_MUL1(t[12 + i])), d = VP8_W(VP8_MUL1(t[4 + i]) + VP8_MUL2(t[12 + i]));
    out[4 * i] = (int16_t)vp8_clamp(VP8_W(a + d) >> 3, -256, 256);
    out[4 * i + 1] = (int16_t)vp8_clamp(VP8_W(b + c) >> 3, -256, 256);
    out[4 * i + 2] = (int16_t)vp8_clamp(VP8_W(b - c) >> 3, -256, 256);
    out[4 * i + 3] = (int16_t)vp8_clamp(VP8_W(a - d) >> 3, -256, 256);
  }
#undef VP8_W
#undef VP8_MUL1
#undef VP8_MUL2
}

// Tiles of one macroblock being rebuilt: pixel (x, y) of the luma at T[(y + 1) * 32 + 4 + x], its
// left neighbour in column 3, the row above in row 0 with the corner at T[3] and the four pixels
// above-right at T[20..23] (repeated in rows 4, 8, 12 for the sub-blocks below); chroma plane c
// at C[c * 160 + (y + 1) * 16 + 4 + x]; R: the 384 residuals.
constexpr int kVp8TileBytes = 17 * 32 + 2 * 160;
#define VP8_AVG3(a, b, c) (((a) + 2 * (b) + (c) + 2) >> 2)
#define VP8_AVG2(a, b) (((a) + (b) + 1) >> 1)

// Sub-block predictor `mode` at (x, y) of the 4x4 block whose top-left pixel is at t.
DHD int vp8_pred4(int mode, const uint8_t* t, int x, int y) {
  int e[13];  // L K J I, the corner X, A..H
#pragma unroll
  for (int k = 0; k < 4; ++k) e[k] = t[(3 - k) * 32 - 1];
#pragma unroll
  for (int k = 0; k < 9; ++k) e[4 + k] = t[-32 - 1 + k];
  const int* T = e + 5;
  switch (mode) {
    case 0: {  // DC
      int s = 4;
      for (int k = 0; k < 4; ++k) s += e[k] + T[k];
      return s >> 3;
    }
    case 1: return vp8_clip8(T[x] + e[3 - y] - e[4]);                                        // TM
    case 2: return VP8_AVG3(e[4 + x], e[5 + x], e[6 + x]);                                   // VE
    case 3: return VP8_AVG3(e[4 - y], e[3 - y], e[y == 3 ? 0 : 2 - y]);                      // HE
    case 4: return VP8_AVG3(e[3 + x - y], e[4 + x - y], e[5 + x - y]);                       // RD
    case 5:                                                                                  // VR
      if (y == 0) return VP8_AVG2(e[4 + x], e[5 + x]);
      if (y == 1) return VP8_AVG3(e[3 + x], e[4 + x], e[5 + x]);
      if (y == 2) return x == 0 ? VP8_AVG3(e[2], e[3], e[4]) : VP8_AVG2(e[3 + x], e[4 + x]);
      return x == 0 ? VP8_AVG3(e[1], e[2], e[3]) : VP8_AVG3(e[2 + x], e[3 + x], e[4 + x]);
    case 6: {                                                                                // LD
      const int i = x + y;
      return VP8_AVG3(T[i], T[i + 1], T[i + 2 > 7 ? 7 : i + 2]);
    }
    case 7:                                                                                  // VL
      if (y == 0) return VP8_AVG2(T[x], T[x + 1]);
      if (y == 1) return VP8_AVG3(T[x], T[x + 1], T[x + 2]);
      if (y == 2) return x < 3 ? VP8_AVG2(T[x + 1], T[x + 2]) : VP8_AVG3(T[4], T[5], T[6]);
      return x < 3 ? VP8_AVG3(T[x + 1], T[x + 2], T[x + 3]) : VP8_AVG3(T[5], T[6], T[7]);
    case 8: {                                                                                // HD
      const int i = 2 * y - x;
      if (i < 0) return VP8_AVG3(e[2 - i], e[3 - i], e[4 - i]);
      if (!(i & 1)) return VP8_AVG2(e[3 - i / 2], e[4 - i / 2]);
      const int c = (7 - i) / 2;
      return VP8_AVG3(e[c - 1], e[c], e[c + 1]);
    }
    default: {                                                                               // HU
      const int i = x + 2 * y;
      if (i >= 6) return e[0];
      const int k = i >> 1;  // I J K L = e[3 - k]
      if (!(i & 1)) return VP8_AVG2(e[3 - k], e[2 - k]);
      return VP8_AVG3(e[3 - k], e[2 - k], e[k + 2 > 3 ? 0 : 1 - k]);
    }
  }
}

// 16x16 (n = 16) or chroma (n = 8) predictor at (x, y); t: the block's top-left pixel in a tile of
// pitch `pitch`; dc: the block's DC value (vp8_pred_dc).
DHD int vp8_pred_big(int mode, const uint8_t* t, int pitch, int x, int y, int dc) {
  switch (mode) {
    case 0: return dc;
    case 1: return vp8_clip8(t[-pitch + x] + t[y * pitch - 1] - t[-pitch - 1]);
    case 2: return t[-pitch + x];
    default: return t[y * pitch - 1];
  }
}
DHD int vp8_pred_dc(const uint8_t* t, int pitch, int n, bool has_top, bool has_left) {
  int s = 0;
  if (has_top)
    for (int k = 0; k < n; ++k) s += t[-pitch + k];
  if (has_left)
    for (int k = 0; k < n; ++k) s += t[k * pitch - 1];
  const int sh = n == 16 ? 4 : 3;
  if (has_top && has_left) return (s + n) >> (sh + 1);
  if (has_top || has_left) return (s + (n >> 1)) >> sh;
  return 128;
}

// Rebuilds macroblock (mx, my), unfiltered, into the planes.  IO: lane, nl, sync().
template <class IO>
DHD void vp8_rec_mb(IO& io, int mx, int my, int mbw, const int16_t* coef, const Vp8Mb& m, uint8_t* Y, uint8_t* U, uint8_t* V,
                    uint8_t* T, int16_t* R) {
  const int yp = 16 * mbw, cp = 8 * mbw;
  uint8_t* C = T + 17 * 32;
  // residuals, a block a lane
  for (int b = io.lane; b < 24; b += io.nl) {
    const uint32_t code = b < 16 ? (m.nzy >> (2 * (15 - b))) & 3 : (m.nzuv >> (8 * ((b - 16) >> 2) + 2 * (3 - (b & 3)))) & 3;
    const bool wrap = b < 16 ? code == 3 : ((m.nzuv >> (8 * ((b - 16) >> 2))) & 0xaa) != 0;
    if (wrap) vp8_itransform<true>(coef + 16 * b, R + 16 * b);
    else if (code) vp8_itransform<false>(coef + 16 * b, R + 16 * b);
    else
      for (int k = 0; k < 16; ++k) R[16 * b + k] = 0;
  }
  // borders: 127 above the first row, 129 left of the first column, libwebp's corners
  for (int k = io.lane; k < 21 + 16; k += io.nl) {
    if (k < 21) {  // the corner, 16 above, 4 above-right
      int v = 127;
      if (my > 0) {
        const uint8_t* above = Y + (int64_t)(16 * my - 1) * yp + 16 * mx;
        if (k == 0) v = mx > 0 ? above[-1] : 129;
        else if (k <= 16) v = above[k - 1];
        else v = mx == mbw - 1 ? above[15] : above[k - 1];
      }
      T[3 + k] = (uint8_t)v;
      if (k > 16) T[4 * 32 + 3 + k] = T[8 * 32 + 3 + k] = T[12 * 32 + 3 + k] = (uint8_t)v;
    } else {
      const int j = k - 21;
      T[(j + 1) * 32 + 3] = mx > 0 ? Y[(int64_t)(16 * my + j) * yp + 16 * mx - 1] : 129;
    }
  }
  for (int k = io.lane; k < 2 * 17; k += io.nl) {
    const int c = k / 17, j = k % 17;
    const uint8_t* P = c ? V : U;
    uint8_t* t = C + c * 160;
    if (j < 9) {
      int v = 127;
      if (my > 0) v = j == 0 ? (mx > 0 ? P[(int64_t)(8 * my - 1) * cp + 8 * mx - 1] : 129) : P[(int64_t)(8 * my - 1) * cp + 8 * mx + j - 1];
      t[3 + j] = (uint8_t)v;
    } else {
      t[(j - 8) * 16 + 3] = mx > 0 ? P[(int64_t)(8 * my + j - 9) * cp + 8 * mx - 1] : 129;
    }
  }
  io.sync();
  uint8_t* t0 = T + 32 + 4;
  if (!m.is_i4) {
    const int mode = m.modes[0];
    const int dc = mode == 0 ? vp8_pred_dc(t0, 32, 16, my > 0, mx > 0) : 0;
    for (int p = io.lane; p < 256; p += io.nl) {
      const int x = p & 15, y = p >> 4;
      const int v = vp8_pred_big(mode, t0, 32, x, y, dc) + R[16 * ((y >> 2) * 4 + (x >> 2)) + (y & 3) * 4 + (x & 3)];
      t0[y * 32 + x] = (uint8_t)vp8_clip8(v);
    }
  } else {
    for (int n = 0; n < 16; ++n) {  // raster order: a sub-block needs those left, above and above-right
      uint8_t* t = t0 + (n >> 2) * 4 * 32 + (n & 3) * 4;
      for (int p = io.lane; p < 16; p += io.nl) {
        const int v = vp8_pred4(m.modes[n], t, p & 3, p >> 2) + R[16 * n + p];
        R[16 * n + p] = (int16_t)vp8_clip8(v);  // (kept aside: the other lanes still read the block's borders)
      }
      io.sync();
      for (int p = io.lane; p < 16; p += io.nl) t[(p >> 2) * 32 + (p & 3)] = (uint8_t)R[16 * n + p];
      io.sync();
    }
  }
  {
    const int mode = m.uvmode;
    uint8_t* tu = C + 16 + 4;
    const int dcu = mode == 0 ? vp8_pred_dc(tu, 16, 8, my > 0, mx > 0) : 0;
    const int dcv = mode == 0 ? vp8_pred_dc(tu + 160, 16, 8, my > 0, mx > 0) : 0;
    for (int p = io.lane; p < 128; p += io.nl) {
      const int c = p >> 6, x = p & 7, y = (p >> 3) & 7;
      uint8_t* t = tu + c * 160;
      const int v = vp8_pred_big(mode, t, 16, x, y, c ? dcv : dcu) + R[16 * (16 + 4 * c + (y >> 2) * 2 + (x >> 2)) + (y & 3) * 4 + (x & 3)];
      t[y * 16 + x] = (uint8_t)vp8_clip8(v);
    }
  }
  io.sync();
  // rows back to the planes as aligned words
  for (int k = io.lane; k < 64 + 32; k += io.nl) {
    if (k < 64) {
      const int y = k >> 2, w = k & 3;
      *(uint32_t*)(Y + (int64_t)(16 * my + y) * yp + 16 * mx + 4 * w) = *(const uint32_t*)(t0 + y * 32 + 4 * w);
    } else {
      const int c = (k - 64) >> 4, y = ((k - 64) >> 1) & 7, w = k & 1;
      *(uint32_t*)((c ? V : U) + (int64_t)(8 * my + y) * cp + 8 * mx + 4 * w) = *(const uint32_t*)(C + c * 160 + (y + 1) * 16 + 4 + 4 * w);
    }
  }
  io.sync();
}

// --- loop filter ---

// One line across an edge: p points at the first sample past it, step apart.  kind 0: the simple
// filter; 1: a macroblock edge of the complex filter; 2: an inner edge of it.  t2 = 2 thresh + 1.
DHD void vp8_filter_line(uint8_t* p, int64_t step, int kind, int t2, int it, int hev_t) {
  const int p1 = p[-2 * step], p0 = p[-step], q0 = p[0], q1 = p[step];
  if (4 * vp8_abs(p0 - q0) + vp8_abs(p1 - q1) > t2) return;
  bool two = true;  // the two-sample filter (the simple one, or high edge variance)
  int p2 = 0, q2 = 0;
  if (kind != 0) {
    const int p3 = p[-4 * step], q3 = p[3 * step];
    p2 = p[-3 * step], q2 = p[2 * step];
    if (vp8_abs(p3 - p2) > it || vp8_abs(p2 - p1) > it || vp8_abs(p1 - p0) > it || vp8_abs(q3 - q2) > it ||
        vp8_abs(q2 - q1) > it || vp8_abs(q1 - q0) > it)
      return;
    two = vp8_abs(p1 - p0) > hev_t || vp8_abs(q1 - q0) > hev_t;
  }
  if (two) {
    const int a = 3 * (q0 - p0) + vp8_clamp(p1 - q1, -128, 127);
    const int a1 = vp8_clamp((a + 4) >> 3, -16, 15), a2 = vp8_clamp((a + 3) >> 3, -16, 15);
    p[-step] = (uint8_t)vp8_clip8(p0 + a2);
    p[0] = (uint8_t)vp8_clip8(q0 - a1);
  } else if (kind == 1) {
    const int a = vp8_clamp(3 * (q0 - p0) + vp8_clamp(p1 - q1, -128, 127), -128, 127);
    const int a1 = (27 * a + 63) >> 7, a2 = (18 * a + 63) >> 7, a3 = (9 * a + 63) >> 7;
    p[-3 * step] = (uint8_t)vp8_clip8(p2 + a3);
    p[-2 * step] = (uint8_t)vp8_clip8(p1 + a2);
    p[-step] = (uint8_t)vp8_clip8(p0 + a1);
    p[0] = (uint8_t)vp8_clip8(q0 - a1);
    p[step] = (uint8_t)vp8_clip8(q1 - a2);
    p[2 * step] = (uint8_t)vp8_clip8(q2 - a3);
  } else {
    const int a = 3 * (q0 - p0);
    const int a1 = vp8_clamp((a + 4) >> 3, -16, 15), a2 = vp8_clamp((a + 3) >> 3, -16, 15), a3 = (a1 + 1) >> 1;
    p[-2 * step] = (uint8_t)vp8_clip8(p1 + a3);
    p[-step] = (uint8_t)vp8_clip8(p0 + a2);
    p[0] = (uint8_t)vp8_clip8(q0 - a1);
    p[step] = (uint8_t)vp8_clip8(q1 - a3);
  }
}

// Filters macroblock (mx, my) in place, in libwebp's order: left edge, inner vertical edges, top
// edge, inner horizontal edges.  A step is 16 luma lines and, for the complex filter, 8 lines of
// each chroma plane (one inner chroma edge, at 4): 32 independent lines.
template <class IO>
DHD void vp8_filter_mb(IO& io, int mx, int my, int mbw, const Vp8Frame& F, const Vp8Mb& m, uint8_t* Y, uint8_t* U, uint8_t* V) {
  const int k4 = m.is_i4 ? 1 : 0, limit = F.limit[m.segment][k4];
  if (!limit) return;
  const int it = F.ilevel[m.segment][k4], hev = F.hev[m.segment][k4], simple = F.filter_type == 1;
  const int64_t yp = 16 * mbw, cp = 8 * mbw;
  uint8_t* y0 = Y + (int64_t)16 * my * yp + 16 * mx;
  uint8_t* u0 = U + (int64_t)8 * my * cp + 8 * mx;
  uint8_t* v0 = V + (int64_t)8 * my * cp + 8 * mx;
  for (int dir = 0; dir < 2; ++dir) {  // 0: vertical edges (lines are rows), 1: horizontal edges
    for (int e = 0; e < 4; ++e) {
      if (e == 0 ? (dir == 0 ? mx == 0 : my == 0) : !m.inner) continue;
      const int t2 = 2 * (limit + (e == 0 ? 4 : 0)) + 1, kind = simple ? 0 : e == 0 ? 1 : 2;
      for (int l = io.lane; l < (simple ? 16 : 32); l += io.nl) {
        if (l < 16) {
          uint8_t* p = dir == 0 ? y0 + l * yp + 4 * e : y0 + (int64_t)4 * e * yp + l;
          vp8_filter_line(p, dir == 0 ? 1 : yp, kind, t2, it, hev);
        } else if (e < 2) {
          uint8_t* c0 = l < 24 ? u0 : v0;
          const int j = l & 7;
          uint8_t* p = dir == 0 ? c0 + j * cp + 4 * e : c0 + (int64_t)4 * e * cp + j;
          vp8_filter_line(p, dir == 0 ? 1 : cp, kind, t2, it, hev);
        }
      }
      io.sync();
    }
  }
}

// --- planes -> RGB ---

// libwebp's fancy upsampler: the chroma sample of pixel (x, y) from the nearer chroma row n and
// the farther one f (vp8_uv_rows), in its two-step rounding.
DHD void vp8_uv_rows(int y, int H, int* n, int* f) {
  if (y == 0) *n = *f = 0;
  else if (y & 1) *n = (y - 1) >> 1, *f = y < H - 1 ? *n + 1 : *n;
  else *n = y >> 1, *f = *n - 1;
}
DHD int vp8_upsample(const uint8_t* nr, const uint8_t* fr, int x, int W) {
  const int k = (x + 1) >> 1;
  if (x == 0) return (3 * nr[0] + fr[0] + 2) >> 2;
  if ((x & 1) && k > ((W - 1) >> 1)) return (3 * nr[k - 1] + fr[k - 1] + 2) >> 2;
  const int a = nr[k - 1], b = nr[k], c = fr[k - 1], d = fr[k], avg = a + b + c + d + 8;
  return (x & 1) ? (((avg + 2 * (b + c)) >> 3) + a) >> 1 : (((avg + 2 * (a + d)) >> 3) + b) >> 1;
}
DHD int vp8_yuv_clip(int v) { return (v & ~16383) == 0 ? v >> 6 : v < 0 ? 0 : 255; }
// Pixel (x, y) as R | G << 8 | B << 16.
DHD uint32_t vp8_rgb_px(const uint8_t* Y, const uint8_t* U, const uint8_t* V, int mbw, int x, int y, int W, int H) {
  int n, f;
  vp8_uv_rows(y, H, &n, &f);
  const int64_t cp = 8 * mbw;
  const int yy = Y[(int64_t)y * 16 * mbw + x], u = vp8_upsample(U + n * cp, U + f * cp, x, W), v = vp8_upsample(V + n * cp, V + f * cp, x, W);
  const int y1 = (yy * 19077) >> 8;
  const int r = vp8_yuv_clip(y1 + ((v * 26149) >> 8) - 14234);
  const int g = vp8_yuv_clip(y1 - ((u * 6419) >> 8) - ((v * 13320) >> 8) + 8708);
  const int b = vp8_yuv_clip(y1 + ((u * 33050) >> 8) - 17685);
  return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
}

}  // namespace dino
