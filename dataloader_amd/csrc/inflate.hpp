// inflate.hpp — zlib-wrapped DEFLATE (RFC 1950 / 1951) for the PNG path, written once for the
// host model and for k_inflate.
//
// The code is SPMD over `nl` lanes that all run the same control flow (nl = 1 on the host, the
// 64 lanes of one wave on the device): the bit buffer and every decision are uniform, lane 0
// writes single bytes, and table fills, stored-block copies, match copies and flushes are
// spread over the lanes with io.sync() between dependent steps.  It errors where zlib 1.2.11's
// inflate() does (inflate.c, inftrees.c; Pillow's ZipDecode.c raises on any negative return):
//   header: (CMF << 8 | FLG) % 31 != 0, CM != 8, CINFO > 7 -> error; FDICT -> Z_NEED_DICT, which
//           Pillow never answers (the file ends "truncated"): an error too;
//   blocks: type 3; a stored LEN != ~NLEN; HLIT > 286 or HDIST > 30; a repeat with no previous
//           length or past HLIT + HDIST; no end-of-block code; an over-subscribed set; an
//           incomplete set unless it is one code of one bit (inftrees.c: left > 0 && (type ==
//           CODES || max != 1)); the code-length code may not be incomplete at all;
//   codes:  a bit pattern no code has; length symbols 286 / 287, distance symbols 30 / 31;
//           a distance beyond the bytes produced so far;
//   the input ending before the last byte Pillow needs (ImageFile.load: "image file is truncated").
// Decoding stops at `want` bytes (H rows): ZipDecode.c returns at the last row whatever follows,
// so what lies after the last byte it needs, the Adler-32 included, is not read here.
#pragma once

#include "common.hpp"

namespace dino {

constexpr int kInfLook = 9;         // lookahead bits of both tables
constexpr int kInfWin = 32768;      // history ring
constexpr int kInfHalf = kInfWin / 2;
constexpr int kInfMaxLens = 320;    // HLIT + HDIST <= 286 + 30, plus slack for the last repeat's check

// One Huffman code: counts per length and symbols in code order (the canonical decode walks
// them bit by bit), plus a lookahead table over the next kInfLook bits: (symbol << 4) | length,
// 0 where the code is longer or no code matches.
struct InfTab {
  uint16_t count[16];
  uint16_t symbol[288];
  uint16_t look[1 << kInfLook];
};

// Canonical decode from the low bits of `bits` (first bit of the code in bit 0), at most
// `maxlen` bits: (symbol << 4) | length, or 0 when no code of <= maxlen bits matches.
DHD uint32_t inf_walk(const InfTab& t, uint32_t bits, int maxlen) {
  int code = 0, first = 0, index = 0;
  for (int len = 1; len <= maxlen; ++len) {
    code |= (int)(bits & 1u);
    bits >>= 1;
    const int count = t.count[len];
    if (code - count < first) return ((uint32_t)t.symbol[index + (code - first)] << 4) | (uint32_t)len;
    index += count;
    first = (first + count) << 1;
    code <<= 1;
  }
  return 0;
}

enum InfType { kInfCodes = 0, kInfLens = 1, kInfDists = 2 };

// Builds t from lens[0..n).  False where inftrees.c inflate_table returns an error.
template <class IO>
DHD bool inf_build(IO& io, InfTab* t, const uint8_t* lens, int n, int type) {
  int count[16], offs[16];
  for (int i = 0; i < 16; ++i) count[i] = 0;
  for (int i = 0; i < n; ++i) count[lens[i]] += 1;
  int max = 15;
  while (max >= 1 && count[max] == 0) --max;
  int left = 1;
  for (int len = 1; len <= 15; ++len) {
    left = (left << 1) - count[len];
    if (left < 0) return false;  // over-subscribed
  }
  if (max >= 1 && left > 0 && (type == kInfCodes || max != 1)) return false;  // incomplete
  // (max == 0, no code at all: inflate_table succeeds with a table of invalid codes; inf_walk
  // then matches nothing)
  io.sync();  // the previous table's readers are done
  if (io.lane == 0) {
    t->count[0] = 0;
    offs[1] = 0;
    for (int len = 1; len <= 15; ++len) {
      t->count[len] = (uint16_t)count[len];
      if (len < 15) offs[len + 1] = offs[len] + count[len];
    }
    for (int i = 0; i < n; ++i)
      if (lens[i]) t->symbol[offs[lens[i]]++] = (uint16_t)i;
  }
  io.sync();
  for (int idx = io.lane; idx < (1 << kInfLook); idx += io.nl) t->look[idx] = (uint16_t)inf_walk(*t, (uint32_t)idx, kInfLook);
  io.sync();
  return true;
}

constexpr uint16_t kInfLenBase[31] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27, 31,
                                      35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258, 0,  0};
constexpr uint8_t kInfLenExtra[31] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0, 0, 0};
constexpr uint16_t kInfDistBase[32] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129, 193,
                                       257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577, 0,   0};
constexpr uint8_t kInfDistExtra[32] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 0, 0};
constexpr uint8_t kInfClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// The decoder's state.  IO gives:
//   int lane, nl;                     this lane and the lane count
//   void sync();                      orders the lanes' window / table accesses (no-op for nl = 1)
//   uint32_t in(int64_t i);           byte i of the zlib stream, 0 past its end (uniform call)
//   uint8_t* win;                     kInfWin bytes of history ring
//   void flush(int64_t at, int n);    ring bytes of output [at, at + n) -> the inflated area
//   InfTab *lt, *dt;  uint8_t* lens;  tables and kInfMaxLens code lengths
template <class IO>
struct Inflater {
  IO& io;
  int64_t in_len;   // bytes of the stream
  int64_t want;     // bytes to produce
  int64_t inpos = 0;
  uint64_t bb = 0;  // bit buffer, next bit in bit 0
  int nb = 0;
  int64_t pos = 0, flushed = 0;

  DHD Inflater(IO& io_, int64_t in_len_, int64_t want_) : io(io_), in_len(in_len_), want(want_) {}

  DHD void fill() {
    while (nb <= 56) {
      bb |= (uint64_t)io.in(inpos++) << nb;
      nb += 8;
    }
  }
  DHD uint32_t take(int n) {  // n <= 16 bits
    if (nb < n) fill();
    const uint32_t v = (uint32_t)bb & ((1u << n) - 1u);
    bb >>= n;
    nb -= n;
    return v;
  }
  // the input ended before the bits taken so far
  DHD bool overrun() const { return inpos * 8 - nb > in_len * 8; }

  DHD int sym(const InfTab& t) {  // -1: no such code
    if (nb < 15) fill();
    uint32_t e = t.look[(uint32_t)bb & ((1u << kInfLook) - 1u)];
    if (e == 0) e = inf_walk(t, (uint32_t)bb, 15);
    if (e == 0) return -1;
    bb >>= (e & 15);
    nb -= (int)(e & 15);
    return (int)(e >> 4);
  }

  DHD void flush_halves() {
    while (pos - flushed >= kInfHalf) {
      io.sync();
      io.flush(flushed, kInfHalf);
      flushed += kInfHalf;
    }
  }

  // n <= 258 bytes from `dist` back; all lanes, reads of a round before its writes.  With
  // dist < n the source of byte i is pos - dist + i % dist: only bytes from before the match.
  DHD void copy_match(int n, int dist) {
    io.sync();
    for (int i0 = 0; i0 < n; i0 += io.nl) {
      const int i = i0 + io.lane;
      uint8_t b = 0;
      if (i < n) b = io.win[(pos - dist + (dist < n ? i % dist : i)) & (kInfWin - 1)];
      io.sync();
      if (i < n) io.win[(pos + i) & (kInfWin - 1)] = b;
    }
    io.sync();
    pos += n;
  }

  DHD bool stored() {
    // drop the bits up to the byte boundary and give whole bytes back to the stream
    const int drop = nb & 7;
    bb >>= drop;
    nb -= drop;
    inpos -= nb >> 3;
    bb = 0;
    nb = 0;
    const uint32_t len = take(16), nlen = take(16);
    if (overrun() || (len ^ 0xFFFFu) != nlen) return false;
    inpos -= nb >> 3;
    bb = 0;
    nb = 0;
    uint32_t left = len;
    while (left > 0 && pos < want) {
      int n = left < 256u ? (int)left : 256;
      if (n > want - pos) n = (int)(want - pos);
      if (inpos + n > in_len) return false;  // the input ends inside the block
      // (io.in is a uniform call: each round fetches its bytes one lane after another)
      io.sync();
      for (int i0 = 0; i0 < n; i0 += io.nl) {
        uint32_t mine = 0;
        for (int k = 0; k < io.nl && i0 + k < n; ++k) {
          const uint32_t b = io.in(inpos + i0 + k);
          if (k == io.lane) mine = b;
        }
        if (i0 + io.lane < n) io.win[(pos + i0 + io.lane) & (kInfWin - 1)] = (uint8_t)mine;
      }
      io.sync();
      pos += n;
      inpos += n;
      left -= (uint32_t)n;
      flush_halves();
    }
    return true;  // (a block that runs past `want` is left unread: decoding is over)
  }

  DHD bool dynamic_tables() {
    const int nlen = (int)take(5) + 257, ndist = (int)take(5) + 1, ncode = (int)take(4) + 4;
    if (nlen > 286 || ndist > 30) return false;
    uint8_t cl[19];
    for (int i = 0; i < 19; ++i) cl[i] = 0;
    for (int i = 0; i < ncode; ++i) cl[kInfClOrder[i]] = (uint8_t)take(3);
    if (overrun()) return false;
    bool any = false;
    for (int i = 0; i < 19; ++i) any |= cl[i] != 0;
    // (no code-length code at all: zlib reads every length as 0 and then misses the
    // end-of-block code, or runs out of input: an error either way)
    if (!any || !inf_build(io, io.lt, cl, 19, kInfCodes)) return false;
    int have = 0;
    while (have < nlen + ndist) {
      const int s = sym(*io.lt);
      if (s < 0 || overrun()) return false;
      if (s < 16) {
        if (io.lane == 0) io.lens[have] = (uint8_t)s;
        ++have;
        continue;
      }
      int prev = 0, rep;
      if (s == 16) {
        if (have == 0) return false;
        io.sync();
        prev = io.lens[have - 1];
        rep = 3 + (int)take(2);
      } else if (s == 17) {
        rep = 3 + (int)take(3);
      } else {
        rep = 11 + (int)take(7);
      }
      if (have + rep > nlen + ndist) return false;
      if (io.lane == 0)
        for (int k = 0; k < rep; ++k) io.lens[have + k] = (uint8_t)prev;
      have += rep;
    }
    if (overrun()) return false;
    io.sync();
    if (io.lens[256] == 0) return false;  // no end-of-block code
    // the distance lengths move out of the way of the literal/length table's build
    uint8_t dl[30];
    for (int i = 0; i < ndist; ++i) dl[i] = io.lens[nlen + i];
    if (!inf_build(io, io.lt, io.lens, nlen, kInfLens)) return false;
    return inf_build(io, io.dt, dl, ndist, kInfDists);
  }

  DHD bool fixed_tables() {
    io.sync();
    for (int i = io.lane; i < 288; i += io.nl) io.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    io.sync();
    if (!inf_build(io, io.lt, io.lens, 288, kInfLens)) return false;
    uint8_t dl[32];
    for (int i = 0; i < 32; ++i) dl[i] = 5;
    return inf_build(io, io.dt, dl, 32, kInfDists);
  }

  DHD bool coded_block() {
    while (pos < want) {
      const int s = sym(*io.lt);
      if (s < 0 || overrun()) return false;
      if (s < 256) {
        if (io.lane == 0) io.win[pos & (kInfWin - 1)] = (uint8_t)s;
        ++pos;
      } else if (s == 256) {
        return true;
      } else {
        if (s > 285) return false;  // 286, 287: the fixed code has them, no length does
        const int n = kInfLenBase[s - 257] + (int)take(kInfLenExtra[s - 257]);
        const int ds = sym(*io.dt);
        if (ds < 0 || ds > 29) return false;
        const int ebits = kInfDistExtra[ds];
        if (nb < ebits) fill();
        const int dist = kInfDistBase[ds] + (int)((uint32_t)bb & ((1u << ebits) - 1u));
        bb >>= ebits;
        nb -= ebits;
        if (overrun() || dist > pos) return false;  // before the first byte: "invalid distance too far back"
        copy_match(n < want - pos ? n : (int)(want - pos), dist);
      }
      flush_halves();
    }
    return true;
  }

  // Produces `want` bytes.  DINO_IMG_OK or DINO_IMG_CORRUPT.
  DHD int run() {
    const uint32_t cmf = take(8), flg = take(8);
    if (overrun() || ((cmf << 8) | flg) % 31u != 0 || (cmf & 15u) != 8 || (cmf >> 4) > 7 || (flg & 0x20u)) return DINO_IMG_CORRUPT;
    bool last = false;
    while (pos < want) {
      if (last) return DINO_IMG_CORRUPT;  // the stream ends short of the last row
      last = take(1) != 0;
      const uint32_t type = take(2);
      if (overrun()) return DINO_IMG_CORRUPT;
      bool ok;
      if (type == 0) ok = stored();
      else if (type == 1) ok = fixed_tables() && coded_block();
      else if (type == 2) ok = dynamic_tables() && coded_block();
      else ok = false;
      if (!ok) return DINO_IMG_CORRUPT;
    }
    io.sync();
    if (pos > flushed) io.flush(flushed, (int)(pos - flushed));
    return DINO_IMG_OK;
  }
};

}  // namespace dino
