// gif_lzw.hpp — GIF's LZW stream decoded 64 codes at a time, one text for k_giflzw (a wave, a
// lane per code) and the host model (dino_debug_gif_decode: the lanes as a loop over slots).
//
// Two properties of the format make the entropy stage parallel within one image:
//   * a code's width depends only on how many codes were read since the last clear code (the table
//     grows by one entry per code), so the bit offset of the j-th code since a clear is a closed
//     form (gif_code_offset) and 64 lanes read 64 codes at once;
//   * every table entry is the previous code's string plus the first byte of the next one, which
//     is a contiguous range of the output already written, so the table holds (position, length)
//     and a code becomes a literal or a copy of an earlier output range.
// The rules are those of Pillow's decoder (libImaging/GifDecode.c): a stream need not start with a
// clear code; the first code after a clear must be a literal; a code may equal the entry being
// created (KwKwK) and a larger one is a broken stream; at 4096 entries the width stays 12 and no
// entry is added until a clear; decoding ends at w x h pixels, whatever follows; an end code or
// the end of the data before that is a truncated file.
//
// IO gives the wave's primitives over kSlots per-lane slots (1 on the device: the lane's own
// registers; 64 on the host): lane(s), shfl(dst, src, idx), ballot(pred), bcast(v, lane), sync()
// and the table dpos[4096] / dlen[4096] (LDS on the device).
#pragma once

#include "gif_parse.hpp"

namespace dino {

constexpr int kGifTable = 4096;
constexpr int kGifMaxWidth = 12;

// Entries the table holds when code j since the last clear is read: clear, end and one entry per
// code after the first.
DHD int gif_table_fill(int bits, int64_t j) {
  const int64_t n = (1 << bits) + 2 + (j > 1 ? j - 1 : 0);
  return n > kGifTable ? kGifTable : (int)n;
}
// Its width: the bit length of that count (entry 2^c - 1 makes the width c + 1), 12 at most.
DHD int gif_code_width(int bits, int64_t j) {
  const int n = gif_table_fill(bits, j);
  int w = bits + 1;
  while (w < kGifMaxWidth && (1 << w) <= n) ++w;
  return w;
}
// Bits between the last clear and code j: code i is wider than c from i = 2^c - clear - 1 on.
DHD int64_t gif_code_offset(int bits, int64_t j) {
  int64_t off = j * (bits + 1);
  for (int c = bits + 1; c < kGifMaxWidth; ++c) {
    const int64_t first = (1 << c) - (1 << bits) - 1;
    if (j > first) off += j - first;
  }
  return off;
}
// w <= 12 bits at bit offset b of the payload (words; 8 readable bytes follow the last one).
DHD int gif_read_code(const uint32_t* ent, int64_t b, int w) {
  const uint32_t* p = ent + (b >> 5);
  const uint64_t v = (uint64_t)p[0] | ((uint64_t)p[1] << 32);
  return (int)((v >> (b & 31)) & ((1u << w) - 1u));
}

// Decodes the payload (ent_len bytes, zero bytes after them) into the npx colour indices of
// `plane` in coded order.  DINO_IMG_OK or DINO_IMG_CORRUPT, uniform over the lanes.
template <class IO>
DHD int gif_lzw_decode(IO& io, const uint32_t* ent, int64_t ent_len, int bits, uint8_t* plane, int64_t npx) {
  constexpr int S = IO::kSlots;
  const int clear = 1 << bits, end = clear + 1;
  const int64_t nbits = ent_len * 8;
  int64_t base = 0;  // bit offset of code 0 since the last clear (or the start)
  int64_t j0 = 0;    // codes read since then
  int64_t out = 0;   // indices written
  int prev_pos = 0, prev_len = 0;  // where the previous code's string lies (j0 > 0)
  for (;;) {
    int code[S], len[S], ptr[S], ref[S], src[S], ex[S], tmp[S], tmp2[S], idx[S];
    bool p_clear[S], p_end[S], p_bad[S];
    // 1. a code per lane; the group ends before the first clear, end, missing or broken code
    for (int s = 0; s < S; ++s) {
      const int64_t j = j0 + io.lane(s), b = base + gif_code_offset(bits, j);
      const int w = gif_code_width(bits, j);
      const bool have = b + w <= nbits;
      const int c = have ? gif_read_code(ent, b, w) : end;
      const int64_t made = (int64_t)clear + 1 + j;  // the entry this code creates (j > 0, below 4096)
      code[s] = c;
      p_clear[s] = c == clear;
      p_end[s] = c == end;
      p_bad[s] = c > end && (j == 0 || c > made);
    }
    const uint64_t m_clear = io.ballot(p_clear), m_end = io.ballot(p_end), m_bad = io.ballot(p_bad);
    const uint64_t m_cut = m_clear | m_end | m_bad;
    const int n = m_cut ? __builtin_ctzll(m_cut) : 64;
    // 2. string lengths: a literal, a table entry, or an entry a lane of this group creates
    //    (the string of the code before that lane, plus one): pointer jumping over the lanes
    const int64_t first_made = (int64_t)clear + 1 + j0;  // lane k creates entry first_made + k
    for (int s = 0; s < S; ++s) {
      const int lane = io.lane(s), c = code[s];
      len[s] = 0, ptr[s] = -1, ref[s] = -1, src[s] = -1;
      if (lane >= n) continue;
      len[s] = 1;
      if (c < clear) continue;
      const int64_t k = c - first_made;
      if (k < 0) {
        len[s] = io.dlen[c], src[s] = (int)io.dpos[c];
      } else if (k == 0) {
        len[s] = prev_len + 1, src[s] = prev_pos;
      } else {
        ptr[s] = ref[s] = (int)k - 1;
      }
    }
    for (int r = 0; r < 6; ++r) {
      for (int s = 0; s < S; ++s) p_bad[s] = ptr[s] >= 0;
      if (!io.ballot(p_bad)) break;
      for (int s = 0; s < S; ++s) idx[s] = ptr[s] >= 0 ? ptr[s] : io.lane(s);
      io.shfl(tmp, len, idx);
      io.shfl(tmp2, ptr, idx);
      for (int s = 0; s < S; ++s)
        if (ptr[s] >= 0) len[s] += tmp[s], ptr[s] = tmp2[s];
    }
    // 3. output positions: an exclusive scan of the lengths (lanes from n on get the total)
    for (int s = 0; s < S; ++s) ex[s] = len[s];
    for (int d = 1; d < 64; d <<= 1) {
      for (int s = 0; s < S; ++s) idx[s] = io.lane(s) >= d ? io.lane(s) - d : io.lane(s);
      io.shfl(tmp, ex, idx);
      for (int s = 0; s < S; ++s)
        if (io.lane(s) >= d) ex[s] += tmp[s];
    }
    const int total = io.bcast(ex, 63);
    for (int s = 0; s < S; ++s) ex[s] -= len[s];
    // (positions stay below 2^31: out < npx <= the bomb limit, total <= 64 x 4096)
    for (int s = 0; s < S; ++s) idx[s] = ref[s] >= 0 ? ref[s] : io.lane(s);
    io.shfl(tmp, ex, idx);
    for (int s = 0; s < S; ++s)
      if (ref[s] >= 0) src[s] = (int)out + tmp[s];
    // 4. the new entries: (where the previous code's string lies, its length + 1)
    for (int s = 0; s < S; ++s) idx[s] = io.lane(s) > 0 ? io.lane(s) - 1 : 0;
    io.shfl(tmp, ex, idx);
    io.shfl(tmp2, len, idx);
    for (int s = 0; s < S; ++s) {
      const int lane = io.lane(s);
      const int64_t made = first_made + lane;
      if (lane >= n || j0 + lane == 0 || made >= kGifTable) continue;
      io.dpos[made] = lane ? (uint32_t)((int)out + tmp[s]) : (uint32_t)prev_pos;
      io.dlen[made] = (uint16_t)((lane ? tmp2[s] : prev_len) + 1);
    }
    // 5. the bytes, 64 at a time in output order: each finds its code by a search over the
    //    scanned positions and its source, a strictly earlier output byte; one inside the chunk
    //    is chased by pointer jumping until it is a literal or lies before the chunk
    for (int cb = 0; cb < total && out + cb < npx; cb += 64) {
      int val[S], hop[S];
      const int64_t chunk = out + cb;
      for (int s = 0; s < S; ++s) idx[s] = 0;
      for (int step = 32; step >= 1; step >>= 1) {
        for (int s = 0; s < S; ++s) tmp2[s] = (idx[s] + step) & 63;
        io.shfl(tmp, ex, tmp2);
        for (int s = 0; s < S; ++s)
          if (idx[s] + step < 64 && tmp[s] <= cb + io.lane(s)) idx[s] += step;
      }
      io.shfl(tmp, ex, idx);
      io.shfl(tmp2, src, idx);
      io.shfl(val, code, idx);
      for (int s = 0; s < S; ++s) {
        const int i = cb + io.lane(s);
        hop[s] = -1;
        if (i >= total || tmp2[s] < 0) continue;  // past the group, or a literal
        const int64_t a = (int64_t)tmp2[s] + (i - tmp[s]);
        if (a < chunk) val[s] = plane[a];
        else hop[s] = (int)(a - chunk);
      }
      for (int r = 0; r < 6; ++r) {
        for (int s = 0; s < S; ++s) p_bad[s] = hop[s] >= 0;
        if (!io.ballot(p_bad)) break;
        for (int s = 0; s < S; ++s) idx[s] = hop[s] >= 0 ? hop[s] : io.lane(s);
        io.shfl(tmp, val, idx);
        io.shfl(tmp2, hop, idx);
        for (int s = 0; s < S; ++s)
          if (hop[s] >= 0) val[s] = tmp[s], hop[s] = tmp2[s];
      }
      for (int s = 0; s < S; ++s) {
        const int i = cb + io.lane(s);
        if (i < total && chunk + io.lane(s) < npx) plane[chunk + io.lane(s)] = (uint8_t)val[s];
      }
      io.sync();  // the stores (and the entries) before the loads of later chunks and groups
    }
    if (n > 0) {
      prev_pos = (int)out + io.bcast(ex, n - 1);
      prev_len = io.bcast(len, n - 1);
    }
    out += total;
    if (out >= npx) return DINO_IMG_OK;  // (Pillow stops here: what follows is not read)
    if (n == 64) {
      j0 += 64;
      continue;
    }
    if (!((m_clear >> n) & 1)) return DINO_IMG_CORRUPT;  // truncated, or a broken stream
    base += gif_code_offset(bits, j0 + n) + gif_code_width(bits, j0 + n);
    j0 = 0;
  }
}

// The host model of k_gifwalk, k_giflzw and k_gif_rgb: the text above with the 64 lanes as a loop
// over slots (dino_debug_gif_decode, the stand-alone sanitizer program).
struct GifHostIO {
  static constexpr int kSlots = 64;
  uint32_t* dpos;
  uint16_t* dlen;
  int lane(int s) const { return s; }
  void shfl(int* dst, const int* src, const int* idx) const {
    int t[64];
    for (int s = 0; s < 64; ++s) t[s] = src[idx[s] & 63];
    for (int s = 0; s < 64; ++s) dst[s] = t[s];
  }
  uint64_t ballot(const bool* p) const {
    uint64_t m = 0;
    for (int s = 0; s < 64; ++s) m |= (uint64_t)p[s] << s;
    return m;
  }
  int bcast(const int* v, int l) const { return v[l]; }
  void sync() const {}
};

// d: the kind-8 descriptor of parse_gif_head (status OK).  ent: align16(scan_len + 64) bytes,
// 4-byte aligned; plane: w h bytes; pal: kGifPalBytes; rgb: 3 w h bytes.  Returns the status.
inline int gif_decode_host(const uint8_t* p, int64_t len, const ImgDesc& d, uint8_t* ent, uint8_t* plane, uint8_t* pal,
                           uint8_t* rgb) {
  for (int i = 0; i < kGifPalBytes; ++i) pal[i] = i < 3 * d.n_scans ? p[d.first_sos + i] : (uint8_t)0;
  int64_t pos = d.scan_off, o = 0, at = 0;
  for (int n; (n = gif_next_block(p, len, pos, &at)) > 0; pos = at + n)
    for (int k = 0; k < n; ++k) ent[o++] = p[at + k];
  for (int k = 0; k < 64; ++k) ent[o + k] = 0;
  uint32_t dpos[kGifTable];
  uint16_t dlen[kGifTable];
  GifHostIO io{dpos, dlen};
  const int64_t npx = (int64_t)d.width * d.height;
  const int st = gif_lzw_decode(io, (const uint32_t*)ent, o, d.color, plane, npx);
  if (st != DINO_IMG_OK) return st;
  for (int y = 0; y < d.height; ++y) {
    const uint8_t* row = plane + (int64_t)gif_coded_row(y, d.height, d.mcus_y) * d.width;
    for (int x = 0; x < d.width; ++x)
      for (int c = 0; c < 3; ++c) rgb[((int64_t)y * d.width + x) * 3 + c] = pal[3 * row[x] + c];
  }
  return st;
}

}  // namespace dino
