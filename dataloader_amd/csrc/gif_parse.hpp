// gif_parse.hpp — the GIF header walk, host and device (k_gifhead, k_gifwalk, dino_probe_gif,
// dino_debug_gif_decode).
//
// Restates what Pillow 12's GifImagePlugin does for Image.open(b).convert("RGB"): _open reads the
// logical screen and the global colour table, _seek(0) skips extensions up to the first image
// descriptor, takes the local colour table over the global one and leaves the LZW stream to the
// decoder; later frames are never read, transparency is ignored by P -> RGB.
// A file is decoded on the device (ImgDesc::kind 8) only when the walk verifies all of it inside
// the first kGifHeadMax bytes: GIF87a / GIF89a, only extension blocks (0x21, any label) with sound
// sub-blocks before the first image descriptor, a descriptor that covers exactly the logical
// screen, a colour table (local or global) that Pillow keeps as a palette, LZW minimum code size
// 2..8.  Everything else with the signature is "GIF, not for the device" (kGifDecline): Pillow
// decides it through the hand-over.  That covers no table at all or a table that is the gray ramp
// 0, 1, 2, .. (Pillow opens both as "L"), a frame that is not the screen (Pillow composes it onto
// a background), a trailer or an unknown block before the image, and an application extension
// "XMP Data" (Image.getexif searches it for an orientation under exif_transpose).  A logical
// screen with a zero side is DINO_IMG_CORRUPT: Image.open raises on it whatever follows.  So is
// what is wrong inside a verified file's LZW stream (gif_lzw.hpp): Pillow raises.
#pragma once

#include "jpeg_parse.hpp"

namespace dino {

constexpr int kGifKind = 8;  // ImgDesc::kind of a GIF the device decodes
constexpr int kGifDecline = DINO_IMG_UNSUPPORTED;
constexpr int kGifHeadMax = 4096;   // the walk ends inside this prefix or declines
constexpr int kGifPalBytes = 1024;  // the image's table area: 256 RGB entries (zero-filled), padded

DHD bool gif_signature(const uint8_t* p, int64_t len) {
  return len >= 6 && p[0] == 'G' && p[1] == 'I' && p[2] == 'F' && p[3] == '8' && (p[4] == '7' || p[4] == '9') && p[5] == 'a';
}

// What the walk found (offsets image-relative): the colour table in force, the LZW minimum code
// size, the interlace flag and the first sub-block's length byte.
struct GifWalk {
  int32_t width, height;
  int32_t pal_off, pal_n;  // table offset and entries (2..256)
  int32_t bits, lace;
  int32_t data_off;
};

// DINO_IMG_OK, kGifDecline or DINO_IMG_CORRUPT (a zero side) for a file with the signature.
DHD int gif_walk(const uint8_t* p, int64_t len, GifWalk* w) {
  w->width = w->height = w->pal_off = w->pal_n = w->bits = w->lace = w->data_off = 0;
  if (!gif_signature(p, len) || len < 13 || len > 0x7FFFFFF0ll) return kGifDecline;
  const int sw = p[6] | (p[7] << 8), sh = p[8] | (p[9] << 8);
  if (sw < 1 || sh < 1) return DINO_IMG_CORRUPT;
  int64_t pos = 13;
  if (p[10] & 0x80) {
    w->pal_off = 13;
    w->pal_n = 2 << (p[10] & 7);
    pos += 3 * w->pal_n;
  }
  for (;;) {
    if (pos + 1 >= len || pos > kGifHeadMax) return kGifDecline;
    const int intro = p[pos++];
    if (intro == 0x21) {  // an extension: a label, then sub-blocks up to a zero length
      const int label = p[pos++];
      for (bool first = true;; first = false) {
        if (pos >= len || pos > kGifHeadMax) return kGifDecline;
        const int n = p[pos++];
        if (n == 0) break;
        if (pos + n > len) return kGifDecline;
        if (first && label == 0xFF && n >= 8) {
          const char* id = "XMP Data";
          bool xmp = true;
          for (int k = 0; k < 8; ++k) xmp = xmp && p[pos + k] == (uint8_t)id[k];
          if (xmp) return kGifDecline;
        }
        pos += n;
      }
      continue;
    }
    if (intro != 0x2C) return kGifDecline;  // the trailer, or a byte Pillow skips
    if (pos + 9 > len) return kGifDecline;
    const int left = p[pos] | (p[pos + 1] << 8), top = p[pos + 2] | (p[pos + 3] << 8);
    const int fw = p[pos + 4] | (p[pos + 5] << 8), fh = p[pos + 6] | (p[pos + 7] << 8), flags = p[pos + 8];
    pos += 9;
    if (left != 0 || top != 0 || fw != sw || fh != sh) return kGifDecline;
    if (flags & 0x80) {
      w->pal_off = (int32_t)pos;
      w->pal_n = 2 << (flags & 7);
      pos += 3 * w->pal_n;
    }
    if (w->pal_n == 0 || pos + 1 > len || pos > kGifHeadMax) return kGifDecline;
    bool ramp = true;  // GifImageFile._is_palette_needed: the table 0, 1, 2, .. makes the image "L"
    for (int i = 0; i < w->pal_n && ramp; ++i) {
      const uint8_t* c = p + w->pal_off + 3 * i;
      ramp = c[0] == i && c[1] == i && c[2] == i;
    }
    if (ramp) return kGifDecline;
    w->bits = p[pos++];
    if (w->bits < 2 || w->bits > 8) return kGifDecline;
    w->width = fw, w->height = fh;
    w->lace = (flags >> 6) & 1;
    w->data_off = (int32_t)pos;
    return DINO_IMG_OK;
  }
}

// The descriptor of a file with the signature.  A kind-8 descriptor keeps the GIF's own numbers
// in fields the JPEG stages of such an image never read: color = the LZW minimum code size,
// mcus_y = the interlace flag, first_sos / n_scans = the colour table's offset and entries,
// scan_off / scan_len = the sub-blocks and the bytes from there to the end of the file (which
// bounds the joined payload).  ncomp is 4 so that the three-component IDCT and colour kernels pass
// the image by, as they do a PNG.  Returns d->status: OK (kind 8), kGifDecline, CORRUPT, or what check_dims says.
DHD int parse_gif_head(const uint8_t* p, int64_t len, int max_dim, ImgDesc* d) {
  GifWalk w;
  d->status = gif_walk(p, len, &w);
  if (d->status != DINO_IMG_OK) return d->status;
  d->kind = kGifKind;
  d->width = w.width;
  d->height = w.height;
  if (check_dims(d, max_dim) != DINO_IMG_OK) return d->status;  // side limit: hand-over (65535^2 is past the bomb limit)
  d->ncomp = 4;
  d->color = w.bits;
  d->max_h = d->max_v = 1;
  d->mcus_y = w.lace;
  d->first_sos = w.pal_off;
  d->n_scans = w.pal_n;
  d->scan_off = w.data_off;
  d->scan_len = (int32_t)(len - w.data_off);
  d->coef_bytes = 0;
  return d->status;
}

// The sub-block chain from `pos` (a length byte): the next block's payload [*at, *at + n) with n
// returned, 0 at the terminator or at the end of the file.  A block the file cuts short ends the
// data too: Pillow's decoder takes a block only once all of it is there, so the bytes of a cut
// block never reach the codes, even when they would complete the image.
DHD int gif_next_block(const uint8_t* p, int64_t len, int64_t pos, int64_t* at) {
  if (pos >= len) return 0;
  const int64_t n = p[pos];
  *at = pos + 1;
  return pos + 1 + n <= len ? (int)n : 0;
}

// The coded row (the order the stream writes them) of output row y: the four interlace passes
// hold rows 0, 8, ..; 4, 12, ..; 2, 6, ..; 1, 3, ...
DHD int gif_coded_row(int y, int h, int lace) {
  if (!lace) return y;
  const int n1 = (h + 7) >> 3, n2 = (h + 3) >> 3, n3 = (h + 1) >> 2;
  if ((y & 7) == 0) return y >> 3;
  if ((y & 7) == 4) return n1 + (y >> 3);
  if ((y & 3) == 2) return n1 + n2 + (y >> 2);
  return n1 + n2 + n3 + (y >> 1);
}

}  // namespace dino
