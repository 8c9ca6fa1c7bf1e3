// png_parse.hpp — chunk walk, row filters and pixel rules of the PNG forms the device decodes.
//
// Restates what Pillow's PngImagePlugin (PIL/PngImagePlugin.py) does for the file the
// reference opens with Image.open(b).convert("RGB") (cpu.py:251):
//   * _accept: the 8-byte signature (PngImageFile._open raises "not a PNG file" otherwise);
//   * _open: every chunk up to the first IDAT goes through ChunkStream.crc, which raises
//     "bad header checksum" on a CRC-32 mismatch whatever the chunk (critical or ancillary);
//     the chunk handlers (chunk_IHDR, chunk_PLTE, chunk_tRNS, chunk_gAMA, ...) raise on
//     payloads shorter than they read;
//   * load_read: the CRC of an IDAT chunk is read and dropped (self.fp.read(4)), never checked;
//     empty IDAT chunks are allowed; the run ends at the first chunk that is not IDAT;
//   * load_end: walks on to IEND, calling the handlers of what lies between (CRCs unchecked);
//     a read that fails (struct.error on fewer than 8 bytes) ends the walk without an error.
// A file is decoded here (ImgDesc::kind 4) only when the walk verifies all of it: IHDR of 13
// bytes first, 8 bits, colour type 0 / 2 / 3 / 4 / 6, no interlace, methods 0; before the IDAT
// run only PLTE, tRNS and the ancillary chunks listed in png_plain_chunk with the lengths their
// handlers read; after the run IEND or fewer than 8 bytes.  Everything else with the signature
// is "PNG, not for the device" (kPngDecline): Pillow decides it through the hand-over.
// Conditions on which Pillow raises map to DINO_IMG_CORRUPT.
#pragma once

#include "jpeg_parse.hpp"

namespace dino {

constexpr int kPngKind = 4;          // ImgDesc::kind of a PNG the device decodes
constexpr int kPngKindDeclined = 5;  // the probes' kind of a PNG it leaves to Pillow
constexpr int kPngDecline = DINO_IMG_UNSUPPORTED;
constexpr int kPngPalBytes = 1024;   // the image's palette area: 256 RGB entries (zero-filled), padded

// (rd32be: jpeg_parse.hpp)
DHD bool png_signature(const uint8_t* p, int64_t len) {
  return len >= 8 && p[0] == 0x89 && p[1] == 'P' && p[2] == 'N' && p[3] == 'G' && p[4] == 0x0D && p[5] == 0x0A &&
         p[6] == 0x1A && p[7] == 0x0A;
}
DHD uint32_t png_cid(char a, char b, char c, char d) {
  return ((uint32_t)(uint8_t)a << 24) | ((uint32_t)(uint8_t)b << 16) | ((uint32_t)(uint8_t)c << 8) | (uint32_t)(uint8_t)d;
}

// CRC-32 (ISO 3309, the PNG polynomial) bit by bit: the chunks checked are a few dozen bytes.
DHD uint32_t png_crc32(const uint8_t* p, int64_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (int64_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  }
  return c ^ 0xFFFFFFFFu;
}

// Channels of a colour type at 8 bits (0 for a type the device does not decode).
DHD int png_channels(int color) {
  switch (color) {
    case 0: return 1;
    case 2: return 3;
    case 3: return 1;
    case 4: return 2;
    case 6: return 4;
    default: return 0;
  }
}

// Bytes of the inflated stream Pillow's decoder consumes: H rows of a filter byte and W pixels.
DHD int64_t png_inflated_bytes(const ImgDesc& d) { return (int64_t)d.height * (1 + (int64_t)d.width * d.max_h); }

// Signature and IHDR fields (no CRC: png_walk checks it).  A kind-4 descriptor keeps the PNG's
// own numbers in fields the JPEG stages of a kind-4 image never read: color = colour type,
// max_h = bytes per pixel, scan_off / scan_len = the bytes after the signature.  ncomp is 4 so
// that the three-component IDCT and colour kernels pass the image by, as they do a
// four-component frame.  Returns d->status: OK (kind 4), kPngDecline, or what check_dims says.
DHD int parse_png_head(const uint8_t* p, int64_t len, int max_dim, ImgDesc* d) {
  d->status = DINO_IMG_CORRUPT;
  if (!png_signature(p, len)) return d->status;
  d->kind = kPngKind;
  // (Pillow needs the whole IHDR chunk: a shorter file raises in _open)
  if (len < 8 + 8 + 13 + 4) return d->status;
  if (rd32be(p + 12) != png_cid('I', 'H', 'D', 'R') || rd32be(p + 8) != 13) return (d->status = kPngDecline);
  const uint32_t w = rd32be(p + 16), h = rd32be(p + 20);
  const int depth = p[24], color = p[25], comp = p[26], filt = p[27], lace = p[28];
  if (w < 1 || h < 1 || w > 0x7FFFFFFFu || h > 0x7FFFFFFFu) return (d->status = kPngDecline);
  d->width = (int32_t)w;
  d->height = (int32_t)h;
  d->status = DINO_IMG_OK;
  if (check_dims(d, max_dim) != DINO_IMG_OK) return d->status;  // bomb: Pillow raises; side limit: hand-over
  if (depth != 8 || png_channels(color) == 0 || comp != 0 || filt != 0 || lace != 0) return (d->status = kPngDecline);
  // every byte index of the stages stays below 2^31 (the bomb limit bounds W x H x 3; the
  // filtered rows hold up to 4 bytes a pixel)
  if ((int64_t)h * (1 + (int64_t)w * 4) > 0x7FFFFFF0ll || len > 0x7FFFFFF0ll) return (d->status = kPngDecline);
  d->ncomp = 4;
  d->color = color;
  d->max_h = png_channels(color);
  d->max_v = 1;
  d->scan_off = 8;
  d->scan_len = (int32_t)(len - 8);
  d->coef_bytes = 0;
  return d->status;
}

// Ancillary chunks Pillow reads before IDAT without touching the pixels, with the payload
// length its handler needs (chunk_gAMA, chunk_sRGB, chunk_cHRM, chunk_pHYs raise on shorter
// ones; bKGD, sBIT, tIME and hIST have no handler and are skipped).  -1: not one of them.
DHD int png_plain_chunk(uint32_t cid, uint32_t n) {
  if (cid == png_cid('g', 'A', 'M', 'A')) return n == 4;
  if (cid == png_cid('s', 'R', 'G', 'B')) return n == 1;
  if (cid == png_cid('c', 'H', 'R', 'M')) return n == 32;
  if (cid == png_cid('p', 'H', 'Y', 's')) return n == 9;
  if (cid == png_cid('b', 'K', 'G', 'D')) return n <= 6;
  if (cid == png_cid('s', 'B', 'I', 'T')) return n <= 4;
  if (cid == png_cid('t', 'I', 'M', 'E')) return n == 7;
  if (cid == png_cid('h', 'I', 'S', 'T')) return n <= 512;
  return -1;
}

// What the walk found: the IDAT run and the palette.
struct PngWalk {
  int32_t idat_off;    // the length field of the first IDAT chunk (image-relative)
  int32_t idat_chunks; // chunks of the run
  int64_t idat_bytes;  // their payload bytes together: the zlib stream
  int32_t plte_off;    // PLTE payload (image-relative), 0 when there is none
  int32_t plte_n;      // its bytes
};

// The whole walk over p[0..len) of a file parse_png_head accepted.  Returns DINO_IMG_OK,
// DINO_IMG_CORRUPT (Pillow raises) or kPngDecline.
DHD int png_walk(const uint8_t* p, int64_t len, int color, PngWalk* w) {
  w->idat_off = w->idat_chunks = w->plte_off = w->plte_n = 0;
  w->idat_bytes = 0;
  int64_t pos = 8;
  bool first = true, trns = false;
  for (;;) {
    // (a file that ends before its first IDAT: Pillow's read fails inside _open)
    if (pos + 8 > len) return DINO_IMG_CORRUPT;
    const uint32_t n = rd32be(p + pos), cid = rd32be(p + pos + 4);
    if (n > 0x7FFFFFFFu || pos + 12 + (int64_t)n > len) return kPngDecline;  // runs past the file
    if (cid == png_cid('I', 'D', 'A', 'T')) break;
    if (first) {
      if (cid != png_cid('I', 'H', 'D', 'R') || n != 13) return kPngDecline;
    } else if (cid == png_cid('P', 'L', 'T', 'E')) {
      // chunk_PLTE keeps the bytes for mode P only; ImagePalette.raw("RGB", ...) raises on
      // more than 768 bytes.  One PLTE of whole entries, not on the gray types.
      if (w->plte_off || trns || n < 3 || n > 768 || n % 3 != 0 || color == 0 || color == 4) return kPngDecline;
      w->plte_off = (int32_t)(pos + 8);
      w->plte_n = (int32_t)n;
    } else if (cid == png_cid('t', 'R', 'N', 'S')) {
      // chunk_tRNS: P keeps the alpha bytes, L reads 2 bytes, RGB 6; convert("RGB") ignores
      // info["transparency"] for all three
      if (trns) return kPngDecline;
      trns = true;
      if (color == 0 ? n != 2 : color == 2 ? n != 6 : color == 3 ? (n < 1 || n > 256 || !w->plte_off) : true)
        return kPngDecline;
    } else if (png_plain_chunk(cid, n) != 1) {
      return kPngDecline;  // iCCP, text, APNG control, eXIf, private chunks, a second IHDR, ...
    }
    // ChunkStream.crc: every chunk before the first IDAT whose handler returns (the ones above)
    if (png_crc32(p + pos + 4, 4 + (int64_t)n) != rd32be(p + pos + 8 + n)) return DINO_IMG_CORRUPT;
    first = false;
    pos += 12 + (int64_t)n;
  }
  if (first || (color == 3 && !w->plte_off)) return kPngDecline;
  w->idat_off = (int32_t)pos;
  // the IDAT run (load_read): CRCs dropped unread
  for (;;) {
    if (pos + 8 > len) return DINO_IMG_OK;  // no IEND: load_end's read fails and the walk ends
    const uint32_t n = rd32be(p + pos), cid = rd32be(p + pos + 4);
    if (cid != png_cid('I', 'D', 'A', 'T')) {
      // load_end stops at IEND whatever its length and CRC; any other chunk runs a handler
      return cid == png_cid('I', 'E', 'N', 'D') ? DINO_IMG_OK : kPngDecline;
    }
    if (n > 0x7FFFFFFFu || pos + 12 + (int64_t)n > len) return kPngDecline;
    w->idat_chunks += 1;
    w->idat_bytes += n;
    pos += 12 + (int64_t)n;
  }
}

// Filter type `f` of a byte with neighbours a (left), b (up), c (up-left), all 0 outside the
// image: the predictor added mod 256 (PNG specification 9.2; Pillow's ZipDecode.c).
DHD int png_predict(int f, int a, int b, int c) {
  switch (f) {
    case 1: return a;
    case 2: return b;
    case 3: return (a + b) >> 1;
    case 4: {
      const int pa = b - c, pb = a - c;  // p - a, p - b with p = a + b - c
      const int qa = pa < 0 ? -pa : pa, qb = pb < 0 ? -pb : pb, pc = pa + pb, qc = pc < 0 ? -pc : pc;
      return qa <= qb && qa <= qc ? a : (qb <= qc ? b : c);  // ties: a, then b
    }
    default: return 0;
  }
}

// convert("RGB") of one reconstructed pixel px[0..bpp): gray replicated, alpha dropped, a
// palette index looked up (entries the PLTE chunk does not hold are black: Pillow pads the
// palette with zeros).  pal: 768 bytes, zero-filled past the chunk.
DHD void png_to_rgb(int color, const uint8_t* px, const uint8_t* pal, uint8_t* rgb) {
  if (color == 2 || color == 6) {
    rgb[0] = px[0], rgb[1] = px[1], rgb[2] = px[2];
  } else if (color == 3) {
    rgb[0] = pal[3 * px[0]], rgb[1] = pal[3 * px[0] + 1], rgb[2] = pal[3 * px[0] + 2];
  } else {
    rgb[0] = rgb[1] = rgb[2] = px[0];
  }
}

// Rows of `inf` (H x (1 + W bpp) filtered bytes) reversed in place, one after another, and
// written to rgb as HWC.  False on a filter byte above 4 (ZipDecode.c: IMAGING_CODEC_UNKNOWN,
// Pillow raises).  The host's order of work; k_unfilter runs 64 rows skewed by a pixel.
inline bool png_unfilter_rows(uint8_t* inf, int W, int H, int bpp, int color, const uint8_t* pal, uint8_t* rgb) {
  const int64_t stride = 1 + (int64_t)W * bpp;
  for (int y = 0; y < H; ++y) {
    uint8_t* row = inf + y * stride + 1;
    const uint8_t* up = y ? row - stride : nullptr;
    const int f = row[-1];
    if (f > 4) return false;
    for (int64_t i = 0; i < (int64_t)W * bpp; ++i) {
      const int a = i >= bpp ? row[i - bpp] : 0, b = up ? up[i] : 0, c = up && i >= bpp ? up[i - bpp] : 0;
      row[i] = (uint8_t)(row[i] + png_predict(f, a, b, c));
    }
    for (int x = 0; x < W; ++x) png_to_rgb(color, row + (int64_t)x * bpp, pal, rgb + ((int64_t)y * W + x) * 3);
  }
  return true;
}

}  // namespace dino
