// vp8l.hpp — the WebP lossless bitstream (VP8L), written once for the host model and for k_vp8l /
// k_vp8l_inv, from the format specification ("WebP Lossless Bitstream Specification").
//
// The entropy layer is SPMD over `nl` lanes that all run the same control flow, as inflate.hpp
// is (nl = 1 on the host, the 64 lanes of one wave on the device): the bit buffer and every
// decision are uniform, lane 0 stores single pixels, and table builds, group staging,
// back-reference copies and colour-cache updates are spread over the lanes with io.sync()
// between dependent steps.  It errors where libwebp's decoder does (Pillow raises on any of it):
//   header:     a transform given twice, colour-cache bits outside 1..11;
//   codes:      a simple code's symbol outside the alphabet leaves no symbol; max_symbol above
//               the alphabet; a repeat past the alphabet; a code (or the code-length code) with
//               no symbol, over-subscribed or incomplete, unless it has one symbol (no bits read);
//   pixels:     a back-reference before the first pixel or past the last one (of the main image
//               or of a sub-image);
//   the stream ending before the last bit read.
// One routine, pixels(), decodes the ARGB image of the transforms' sub-images, of the entropy
// image and of the main image (sub_stream() and body() read the codes it uses).
#pragma once

#include "common.hpp"

namespace dino {

constexpr int kVp8lGreenMax = 256 + 24 + 2048;  // literals, length prefixes, an 11-bit colour cache
constexpr int kVp8lSyms = kVp8lGreenMax + 3 * 256 + 40;
constexpr int kVp8lLens = kVp8lGreenMax + 8 + 24;  // code lengths of one code, then the code-length code's own 19
constexpr int kVp8lCacheMax = 2048;
// Codes of one group in canonical form: per code the symbols per length (count[c][0] = 1 marks a
// code of a single symbol, read with no bits) and its symbols in code order.
struct Vp8lGroup {
  uint16_t count[5][16];
  uint16_t sym[kVp8lSyms];  // green, red, blue, alpha, distance
};
static_assert(sizeof(Vp8lGroup) == 6432 && sizeof(Vp8lGroup) % 16 == 0, "Vp8lGroup layout");
DHD int vp8l_sym_off(int c) { return c == 0 ? 0 : kVp8lGreenMax + (c - 1) * 256; }

// What the inverse transforms need (k_vp8l -> k_vp8l_inv through the head of the sub-image area).
struct Vp8lPlan {
  int32_t ntr, xs;     // transforms in stream order; width of the decoded ARGB image (W unless bundled)
  int32_t type[4];     // 0 predictor, 1 cross-colour, 2 subtract-green, 3 colour indexing
  int32_t bits[4];     // block bits (0, 1); bundling width bits (3): 8 >> bits index bits a pixel
  int32_t xs_in[4];    // image width the transform sees (after inverse: xs_in of the one before it)
  int32_t sub_off[4];  // its sub-image, words from the start of the sub-image words
  int32_t feat[6];     // transforms seen (bit per type), cache bits, groups, bundling bits + 1, distance codes < 120 / >= 120
  int32_t pad[8];
};
static_assert(sizeof(Vp8lPlan) == 128, "Vp8lPlan layout");

// Sub-image words a W x H file can need: predictor, cross-colour and entropy images of at most
// ceil(W / 4) x ceil(H / 4) pixels each (block bits >= 2) and a palette of 256.
DHD int64_t vp8l_block_px(int w, int h) { return (int64_t)((w + 3) >> 2) * ((h + 3) >> 2); }
DHD int64_t vp8l_sub_words(int w, int h) { return 3 * vp8l_block_px(w, h) + 256; }

// The 120 short distance codes as (yi << 4) | (8 - xi): distance = xi + yi * xsize, at least 1.
constexpr uint8_t kVp8lDistMap[120] = {
    0x18, 0x07, 0x17, 0x19, 0x28, 0x06, 0x27, 0x29, 0x16, 0x1a, 0x26, 0x2a, 0x38, 0x05, 0x37, 0x39, 0x15, 0x1b, 0x36, 0x3a,
    0x25, 0x2b, 0x48, 0x04, 0x47, 0x49, 0x14, 0x1c, 0x35, 0x3b, 0x46, 0x4a, 0x24, 0x2c, 0x58, 0x45, 0x4b, 0x34, 0x3c, 0x03,
    0x57, 0x59, 0x13, 0x1d, 0x56, 0x5a, 0x23, 0x2d, 0x44, 0x4c, 0x55, 0x5b, 0x33, 0x3d, 0x68, 0x02, 0x67, 0x69, 0x12, 0x1e,
    0x66, 0x6a, 0x22, 0x2e, 0x54, 0x5c, 0x43, 0x4d, 0x65, 0x6b, 0x32, 0x3e, 0x78, 0x01, 0x77, 0x79, 0x53, 0x5d, 0x11, 0x1f,
    0x64, 0x6c, 0x42, 0x4e, 0x76, 0x7a, 0x21, 0x2f, 0x75, 0x7b, 0x31, 0x3f, 0x63, 0x6d, 0x52, 0x5e, 0x00, 0x74, 0x7c, 0x41,
    0x4f, 0x10, 0x20, 0x62, 0x6e, 0x30, 0x73, 0x7d, 0x51, 0x5f, 0x40, 0x72, 0x7e, 0x61, 0x6f, 0x50, 0x71, 0x7f, 0x60, 0x70};
constexpr uint8_t kVp8lClOrder[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};

// --- pixel rules of the inverse transforms (host model and k_vp8l_inv) ---
DHD uint32_t vp8l_add(uint32_t a, uint32_t b) {  // per-channel sum mod 256
  return (((a & 0xFF00FF00u) + (b & 0xFF00FF00u)) & 0xFF00FF00u) | (((a & 0x00FF00FFu) + (b & 0x00FF00FFu)) & 0x00FF00FFu);
}
DHD uint32_t vp8l_avg2(uint32_t a, uint32_t b) { return (((a ^ b) & 0xFEFEFEFEu) >> 1) + (a & b); }
DHD int vp8l_clip(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
DHD int vp8l_absd(uint32_t a, uint32_t b, int s) {
  const int d = (int)((a >> s) & 255) - (int)((b >> s) & 255);
  return d < 0 ? -d : d;
}
// Predictor `mode` of the pixel whose neighbours are L, T, TL, TR (modes 14 and 15 predict as 0).
DHD uint32_t vp8l_predict(int mode, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR) {
  switch (mode) {
    case 1: return L;
    case 2: return T;
    case 3: return TR;
    case 4: return TL;
    case 5: return vp8l_avg2(vp8l_avg2(L, TR), T);
    case 6: return vp8l_avg2(L, TL);
    case 7: return vp8l_avg2(L, T);
    case 8: return vp8l_avg2(TL, T);
    case 9: return vp8l_avg2(T, TR);
    case 10: return vp8l_avg2(vp8l_avg2(L, TL), vp8l_avg2(T, TR));
    case 11: {  // Select: the neighbour nearer to L + T - TL in Manhattan distance
      int pl = 0, pt = 0;
      for (int s = 0; s < 32; s += 8) pl += vp8l_absd(T, TL, s), pt += vp8l_absd(L, TL, s);
      return pl < pt ? L : T;
    }
    case 12: {  // ClampAddSubtractFull
      uint32_t v = 0;
      for (int s = 0; s < 32; s += 8)
        v |= (uint32_t)vp8l_clip((int)((L >> s) & 255) + (int)((T >> s) & 255) - (int)((TL >> s) & 255)) << s;
      return v;
    }
    case 13: {  // ClampAddSubtractHalf
      const uint32_t a = vp8l_avg2(L, T);
      uint32_t v = 0;
      for (int s = 0; s < 32; s += 8) {
        const int x = (int)((a >> s) & 255), y = (int)((TL >> s) & 255);
        v |= (uint32_t)vp8l_clip(x + (x - y) / 2) << s;
      }
      return v;
    }
    default: return 0xFF000000u;
  }
}
// The mode of pixel (x, y): the top row and the left column have fixed ones.
DHD int vp8l_pred_mode(int x, int y, uint32_t block) { return y == 0 ? (x == 0 ? 0 : 1) : x == 0 ? 2 : (int)((block >> 8) & 15); }
DHD uint32_t vp8l_add_green(uint32_t p) {
  const uint32_t g = (p >> 8) & 255;
  return (p & 0xFF00FF00u) | (((p & 0x00FF00FFu) + ((g << 16) | g)) & 0x00FF00FFu);
}
DHD int vp8l_cdelta(uint32_t t, uint32_t c) { return ((int)(int8_t)t * (int)(int8_t)c) >> 5; }
DHD uint32_t vp8l_cross(uint32_t p, uint32_t block) {  // block: red_to_blue << 16 | green_to_blue << 8 | green_to_red
  const uint32_t g = (p >> 8) & 255;
  const uint32_t r = ((p >> 16) + (uint32_t)vp8l_cdelta(block, g)) & 255;
  const uint32_t b = (p + (uint32_t)vp8l_cdelta(block >> 8, g) + (uint32_t)vp8l_cdelta(block >> 16, r)) & 255;
  return (p & 0xFF00FF00u) | (r << 16) | b;
}
// Pixel x of a row of bundled indices (`bits`: 3, 2, 1, 0 for 1, 2, 4, 8 index bits) through the palette.
DHD uint32_t vp8l_index(const uint32_t* row, const uint32_t* pal, int x, int bits) {
  const int per = 8 >> bits;
  const uint32_t g = (row[x >> bits] >> 8) & 255;
  return pal[(g >> ((x & ((1 << bits) - 1)) * per)) & ((1u << per) - 1u)];
}

// The decoder's state.  IO gives:
//   int lane, nl;                          this lane and the lane count
//   void sync();                           orders the lanes' memory accesses (no-op for nl = 1)
//   uint32_t in(int64_t i);                byte i of the VP8L payload, 0 past its end (uniform call)
//   uint64_t ballot(bool); int below(uint64_t m);   lanes voting true; of those, the ones below this lane
//   void amax(uint32_t* p, uint32_t v);    atomic max
//   uint32_t *cache, *stamp;               kVp8lCacheMax words each
//   uint8_t* lens;                         kVp8lLens bytes
//   Vp8lGroup* stage;                      the group the pixel loop reads its codes from
template <class IO>
struct Vp8l {
  IO& io;
  int64_t in_len;
  Vp8lGroup* groups;  // ngroups records (sub-images use the first)
  int groups_cap;
  uint32_t* sub;      // sub-image words
  int64_t sub_cap;
  Vp8lPlan& plan;     // (memory every lane reaches: indexed at run time)
  int W = 0, H = 0;
  int cache_bits = 0, pbits = 0, ngroups = 1, ew = 0;
  const uint32_t* ent = nullptr;
  int64_t sub_used = 0;
  int64_t inpos = 0;
  uint64_t bb = 0;  // bit buffer, next bit in bit 0
  int nb = 0;

  DHD Vp8l(IO& io_, int64_t in_len_, Vp8lGroup* g, int gcap, uint32_t* sub_, int64_t sub_cap_, Vp8lPlan& plan_)
      : io(io_), in_len(in_len_), groups(g), groups_cap(gcap), sub(sub_), sub_cap(sub_cap_), plan(plan_) {}

  DHD void fill() {
    while (nb <= 56) {
      bb |= (uint64_t)io.in(inpos++) << nb;
      nb += 8;
    }
  }
  DHD uint32_t take(int n) {  // n <= 18 bits
    if (nb < n) fill();
    const uint32_t v = (uint32_t)bb & ((1u << n) - 1u);
    bb >>= n;
    nb -= n;
    return v;
  }
  DHD bool overrun() const { return inpos * 8 - nb > in_len * 8; }

  // Canonical decode of the next symbol of a code (first bit of the code in bit 0); -1: no such code.
  DHD int walk(const uint16_t* cnt, const uint16_t* sy) {
    if (cnt[0]) return sy[0];
    if (nb < 15) fill();
    uint32_t bits = (uint32_t)bb;
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; ++len) {
      code |= (int)(bits & 1u);
      bits >>= 1;
      const int count = cnt[len];
      if (code - count < first) {
        bb >>= len;
        nb -= len;
        return sy[index + (code - first)];
      }
      index += count;
      first = (first + count) << 1;
      code <<= 1;
    }
    return -1;
  }
  DHD int sym(int c) { return walk(io.stage->count[c], io.stage->sym + vp8l_sym_off(c)); }

  // lens[0..n) -> canonical form.  False where libwebp's table builder returns 0.
  DHD bool build(const uint8_t* lens, int n, uint16_t* count, uint16_t* sy) {
    int cnt[16], offs[16];
#pragma unroll
    for (int l = 0; l < 16; ++l) cnt[l] = 0;
    io.sync();
    for (int i0 = 0; i0 < n; i0 += io.nl) {
      const int i = i0 + io.lane, l = i < n ? lens[i] : 0;
#pragma unroll
      for (int L = 1; L <= 15; ++L) cnt[L] += __builtin_popcountll(io.ballot(l == L));
    }
    int below15 = 0, left = 1;  // below15: symbols of 1..14 bits
    bool over = false;
#pragma unroll
    for (int L = 1; L <= 15; ++L) {
      if (L < 15) below15 += cnt[L];
      left = (left << 1) - cnt[L];
      over |= left < 0;
    }
    if (below15 + cnt[15] == 0) return false;
    const bool single = below15 + cnt[15] == 1;
    if (!single && (over || left != 0)) return false;
    offs[1] = 0;
#pragma unroll
    for (int L = 1; L < 15; ++L) offs[L + 1] = offs[L] + cnt[L];
    if (io.lane == 0) {
      count[0] = single ? 1 : 0;
#pragma unroll
      for (int L = 1; L <= 15; ++L) count[L] = (uint16_t)cnt[L];
    }
    for (int i0 = 0; i0 < n; i0 += io.nl) {
      const int i = i0 + io.lane, l = i < n ? lens[i] : 0;
#pragma unroll
      for (int L = 1; L <= 15; ++L) {
        const uint64_t m = io.ballot(l == L);
        if (l == L) sy[offs[L] + io.below(m)] = (uint16_t)i;
        offs[L] += __builtin_popcountll(m);
      }
    }
    io.sync();
    return true;
  }

  // One prefix code over an alphabet of n symbols -> code c of group G.
  DHD bool read_code(int n, Vp8lGroup* G, int c) {
    uint8_t* lens = io.lens;
    io.sync();
    for (int i = io.lane; i < kVp8lLens; i += io.nl) lens[i] = 0;
    io.sync();
    if (take(1)) {  // simple: one or two symbols, of 1 or 8 bits
      const int two = (int)take(1), wide = (int)take(1);
      const int s0 = (int)take(wide ? 8 : 1), s1 = two ? (int)take(8) : s0;
      if (io.lane == 0) lens[s0] = 1, lens[s1] = 1;
    } else {
      uint8_t* cl = lens + kVp8lGreenMax + 8;
      const int nc = 4 + (int)take(4);
      for (int i = 0; i < nc; ++i) {
        const uint32_t v = take(3);
        if (io.lane == 0) cl[kVp8lClOrder[i]] = (uint8_t)v;
      }
      int max_symbol = n;
      if (take(1)) {
        const int lb = 2 + 2 * (int)take(3);
        max_symbol = 2 + (int)take(lb);
        if (max_symbol > n) return false;
      }
      if (overrun()) return false;
      // the code-length code borrows the staged group's distance slot: no pixel loop runs now
      uint16_t* ccnt = io.stage->count[4];
      uint16_t* csy = io.stage->sym + vp8l_sym_off(4);
      if (!build(cl, 19, ccnt, csy)) return false;
      int have = 0, prev = 8;
      while (have < n && max_symbol-- > 0) {
        const int s = walk(ccnt, csy);
        if (s < 0 || overrun()) return false;
        if (s < 16) {
          if (io.lane == 0) lens[have] = (uint8_t)s;
          ++have;
          if (s) prev = s;
          continue;
        }
        const int rep = s == 16 ? 3 + (int)take(2) : s == 17 ? 3 + (int)take(3) : 11 + (int)take(7);
        if (have + rep > n) return false;
        if (s == 16)
          for (int k = io.lane; k < rep; k += io.nl) lens[have + k] = (uint8_t)prev;
        have += rep;
      }
    }
    if (overrun()) return false;
    return build(lens, n, G->count[c], G->sym + vp8l_sym_off(c));
  }

  DHD bool read_group(Vp8lGroup* G, int cbits) {
    return read_code(256 + 24 + (cbits ? 1 << cbits : 0), G, 0) && read_code(256, G, 1) && read_code(256, G, 2) &&
           read_code(256, G, 3) && read_code(40, G, 4);
  }

  // The codes of group g to io.stage: the counts, then the symbols each code has.
  DHD void stage_group(int g) {
    const Vp8lGroup* G = groups + g;
    io.sync();
    for (int i = io.lane; i < 40; i += io.nl) ((uint32_t*)io.stage->count)[i] = ((const uint32_t*)G->count)[i];
    io.sync();
    for (int c = 0; c < 5; ++c) {
      int n = 0;
      for (int l = 1; l <= 15; ++l) n += io.stage->count[c][l];
      const uint32_t* s = (const uint32_t*)(G->sym + vp8l_sym_off(c));
      uint32_t* d = (uint32_t*)(io.stage->sym + vp8l_sym_off(c));
      for (int i = io.lane; i < (n + 1) / 2; i += io.nl) d[i] = s[i];
    }
    io.sync();
  }

  DHD int prefix_value(int s) {  // length or distance code of prefix symbol s
    if (s < 4) return s + 1;
    const int extra = (s - 2) >> 1;
    return ((2 + (s & 1)) << extra) + (int)take(extra) + 1;
  }

  // Colour cache, filled lazily: the pixels [from, to) of out enter in order, the last writer of
  // a slot wins.  Each lane stamps its slot with its pixel's index by atomic max (indices only
  // grow over a stream), then the lane whose stamp stands stores the colour.
  DHD void cache_catch_up(const uint32_t* out, int64_t from, int64_t to, int cbits) {
    io.sync();
    for (int64_t i0 = from; i0 < to; i0 += io.nl) {
      const int64_t i = i0 + io.lane;
      uint32_t c = 0, slot = 0;
      if (i < to) {
        c = out[i];
        slot = (0x1e35a7bdu * c) >> (32 - cbits);
        io.amax(&io.stamp[slot], (uint32_t)i + 1u);
      }
      io.sync();
      if (i < to && io.stamp[slot] == (uint32_t)i + 1u) io.cache[slot] = c;
    }
    io.sync();
  }

  // xs x ys ARGB pixels to out, entropy-coded with the groups the entropy image e names (null: group 0).
  DHD bool pixels(uint32_t* out, int xs, int ys, int cbits, const uint32_t* e, int ebits, int e_w) {
    const int64_t total = (int64_t)xs * ys;
    if (cbits) {
      io.sync();
      for (int i = io.lane; i < kVp8lCacheMax; i += io.nl) io.cache[i] = 0, io.stamp[i] = 0;
    }
    const int mask = e ? (1 << ebits) - 1 : -1;
    int64_t pos = 0, cached = 0;
    int x = 0, y = 0, cur = -1;
    bool look = true;
    while (pos < total) {
      if (look || (x & mask) == 0) {
        const int g = e ? (int)((e[(int64_t)(y >> ebits) * e_w + (x >> ebits)] >> 8) & 0xFFFF) : 0;
        if (g != cur) stage_group(cur = g);
        look = false;
      }
      const int s = sym(0);
      if (s < 0) return false;
      int n = 1;
      if (s < 256) {
        const int r = sym(1), b = sym(2), a = sym(3);
        if ((r | b | a) < 0) return false;
        if (io.lane == 0) out[pos] = ((uint32_t)a << 24) | ((uint32_t)r << 16) | ((uint32_t)s << 8) | (uint32_t)b;
      } else if (s < 256 + 24) {
        n = prefix_value(s - 256);
        const int ds = sym(4);
        if (ds < 0) return false;
        const int dc = prefix_value(ds);
        int64_t dist = dc - 120;
        if (dc <= 120) {
          const int m = kVp8lDistMap[dc - 1];
          dist = (int64_t)(m >> 4) * xs + (8 - (m & 15));
          if (dist < 1) dist = 1;
        }
        plan.feat[dc <= 120 ? 4 : 5] = 1;
        if (overrun() || dist > pos || n > total - pos) return false;
        // all lanes copy; with dist < n the source of pixel i is pos - dist + i % dist: only pixels from before the match
        io.sync();
        const int dd = (int)dist;
        for (int i = io.lane; i < n; i += io.nl) out[pos + i] = out[pos - dist + (dist < n ? i % dd : i)];
        look = true;
      } else {
        if (cached < pos) cache_catch_up(out, cached, pos, cbits);
        cached = pos;
        const uint32_t c = io.cache[s - (256 + 24)];
        if (io.lane == 0) out[pos] = c;
      }
      pos += n;
      x += n;
      if (x >= xs) y += x / xs, x %= xs;
      if (overrun()) return false;
    }
    io.sync();
    return true;
  }

  DHD bool read_cache_bits(int* cbits) {
    *cbits = 0;
    if (take(1)) {
      *cbits = (int)take(4);
      if (*cbits < 1 || *cbits > 11) return false;
    }
    return true;
  }

  // The image stream of a sub-image: its colour cache, one group, the pixels.
  DHD bool sub_stream(int xs, int ys, uint32_t** out) {
    const int64_t n = (int64_t)xs * ys;
    if (sub_used + n > sub_cap) return false;
    *out = sub + sub_used;
    sub_used += n;
    int cbits;
    if (!read_cache_bits(&cbits) || groups_cap < 1 || !read_group(groups, cbits)) return false;
    return pixels(*out, xs, ys, cbits, nullptr, 0, 0);
  }

  // The main image's stream up to its codes: the transforms with their sub-images, the colour
  // cache, the entropy image and the number of groups it names.
  DHD bool prologue() {
    if (take(8) != 0x2f) return false;
    W = 1 + (int)take(14), H = 1 + (int)take(14);
    take(1);
    if (take(3) != 0) return false;
    io.sync();
    for (int i = io.lane; i < (int)(sizeof(Vp8lPlan) / 4); i += io.nl) ((int32_t*)&plan)[i] = 0;
    io.sync();
    plan.xs = W;
    uint32_t* img;
    while (take(1)) {
      const int t = (int)take(2), k = plan.ntr;
      if ((plan.feat[0] >> t) & 1) return false;
      plan.feat[0] |= 1 << t;
      plan.type[k] = t;
      plan.xs_in[k] = plan.xs;
      plan.sub_off[k] = (int32_t)sub_used;
      if (t < 2) {
        const int b = plan.bits[k] = 2 + (int)take(3);
        if (!sub_stream((plan.xs + (1 << b) - 1) >> b, (H + (1 << b) - 1) >> b, &img)) return false;
      } else if (t == 3) {
        const int n = 1 + (int)take(8), b = plan.bits[k] = n > 16 ? 0 : n > 4 ? 1 : n > 2 ? 2 : 3;
        if (sub_used + 256 > sub_cap) return false;
        io.sync();
        for (int i = io.lane; i < 256; i += io.nl) sub[sub_used + i] = 0;
        if (!sub_stream(n, 1, &img)) return false;
        sub_used = plan.sub_off[k] + 256;  // (entries past n stay transparent black)
        if (io.lane == 0)
          for (int i = 1; i < n; ++i) img[i] = vp8l_add(img[i], img[i - 1]);
        io.sync();
        plan.xs = (plan.xs + (1 << b) - 1) >> b;
        plan.feat[3] = b + 1;
      }
      ++plan.ntr;
    }
    if (!read_cache_bits(&cache_bits)) return false;
    if (take(1)) {
      pbits = 2 + (int)take(3);
      ew = (plan.xs + (1 << pbits) - 1) >> pbits;
      const int eh = (H + (1 << pbits) - 1) >> pbits;
      if (!sub_stream(ew, eh, &img)) return false;
      ent = img;
      uint32_t mx = 0;
      for (int64_t i = io.lane; i < (int64_t)ew * eh; i += io.nl) {
        const uint32_t g = (img[i] >> 8) & 0xFFFF;
        mx = g > mx ? g : mx;
      }
      if (io.lane == 0) io.stamp[0] = 0;
      io.sync();
      io.amax(&io.stamp[0], mx);
      io.sync();
      ngroups = 1 + (int)io.stamp[0];
    }
    plan.feat[1] = cache_bits, plan.feat[2] = ngroups;
    return !overrun();
  }

  // The codes and the pixels of the main image: plan.xs x H ARGB words to out.
  DHD bool body(uint32_t* out) {
    if (ngroups > groups_cap) return false;
    for (int g = 0; g < ngroups; ++g)
      if (!read_group(groups + g, cache_bits)) return false;
    return pixels(out, plan.xs, H, cache_bits, ent, pbits, ew);
  }
};

// The host's order of work over the decoded image: the transforms undone last to first in place
// (colour indexing into `tmp`, W x H words), then RGB with alpha dropped.
inline void vp8l_inverse_host(const Vp8lPlan& p, const uint32_t* sub, uint32_t* img, uint32_t* tmp, int W, int H, uint8_t* rgb) {
  for (int k = p.ntr - 1; k >= 0; --k) {
    const int xs = p.xs_in[k], b = p.bits[k], bw = (xs + (1 << b) - 1) >> b;
    const uint32_t* s = sub + p.sub_off[k];
    if (p.type[k] == 3) {
      const int pw = (xs + (1 << b) - 1) >> b;
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < xs; ++x) tmp[(int64_t)y * xs + x] = vp8l_index(img + (int64_t)y * pw, s, x, b);
      for (int64_t i = 0; i < (int64_t)xs * H; ++i) img[i] = tmp[i];
      continue;
    }
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < xs; ++x) {
        uint32_t* q = img + (int64_t)y * xs + x;
        const uint32_t blk = p.type[k] == 2 ? 0 : s[(int64_t)(y >> b) * bw + (x >> b)];
        if (p.type[k] == 2) *q = vp8l_add_green(*q);
        else if (p.type[k] == 1) *q = vp8l_cross(*q, blk);
        else {
          const uint32_t L = x ? q[-1] : 0, T = y ? q[-xs] : 0, TL = x && y ? q[-xs - 1] : 0;
          const uint32_t TR = y ? q[-xs + 1] : 0;  // (x == xs - 1: the row's own first pixel, as the format says)
          *q = vp8l_add(*q, vp8l_predict(vp8l_pred_mode(x, y, blk), L, T, TL, TR));
        }
      }
  }
  for (int64_t i = 0; i < (int64_t)W * H; ++i)
    rgb[3 * i] = (uint8_t)(img[i] >> 16), rgb[3 * i + 1] = (uint8_t)(img[i] >> 8), rgb[3 * i + 2] = (uint8_t)img[i];
}

}  // namespace dino
