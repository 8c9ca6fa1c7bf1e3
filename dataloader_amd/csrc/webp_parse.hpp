// webp_parse.hpp — RIFF / WebP container walk and the VP8L header, host and device (k_webphead,
// dino_probe_webp, dino_debug_webp_decode).
//
// A file is decoded on the device (ImgDesc::kind 6) only when the walk verifies all of it:
//   RIFF <size> WEBP with size + 8 equal to the file's length, every chunk inside it, and either
//     * one VP8L chunk and nothing else, or
//     * a VP8X chunk of 10 bytes with the animation flag clear and the canvas of the VP8L header,
//       then exactly one VP8L chunk among chunks Pillow reads no pixels from (ICCP, XMP, unknown
//       ones).
// VP8 (lossy), ALPH, ANIM / ANMF, an EXIF chunk (ImageOps.exif_transpose may turn the image), a
// second VP8L, a size that does not add up or a side above max_image_dim make the file "WebP, not
// for the device" (kWebpDecline): Pillow decides it through the hand-over.  What is wrong inside
// a verified file's VP8L payload (vp8l.hpp) is DINO_IMG_CORRUPT: Pillow raises on it.
#pragma once

#include "jpeg_parse.hpp"

namespace dino {

constexpr int kWebpKind = 6;  // ImgDesc::kind of a lossless WebP the device decodes
constexpr int kWebpDecline = DINO_IMG_UNSUPPORTED;

// (rd32le: jpeg_parse.hpp)
DHD uint32_t webp_cid(char a, char b, char c, char d) {
  return (uint32_t)(uint8_t)a | ((uint32_t)(uint8_t)b << 8) | ((uint32_t)(uint8_t)c << 16) | ((uint32_t)(uint8_t)d << 24);
}
DHD bool webp_signature(const uint8_t* p, int64_t len) {
  return len >= 12 && rd32le(p) == webp_cid('R', 'I', 'F', 'F') && rd32le(p + 8) == webp_cid('W', 'E', 'B', 'P');
}

// The VP8L chunk's payload (image-relative) of a verified file.
struct WebpWalk {
  int32_t off, len;
  int32_t width, height;
};

// DINO_IMG_OK or kWebpDecline for a file with the signature.
DHD int webp_walk(const uint8_t* p, int64_t len, WebpWalk* w) {
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
    } else if (cid == webp_cid('V', 'P', '8', 'L')) {
      if (w->len || n < 5 || (!first && !vp8x)) return kWebpDecline;
      w->off = (int32_t)(pos + 8);
      w->len = (int32_t)n;
    } else if (!vp8x || cid == webp_cid('V', 'P', '8', ' ') || cid == webp_cid('A', 'L', 'P', 'H') ||
               cid == webp_cid('A', 'N', 'I', 'M') || cid == webp_cid('A', 'N', 'M', 'F') ||
               cid == webp_cid('E', 'X', 'I', 'F')) {
      return kWebpDecline;
    }
    first = false;
    pos = next;
  }
  if (!w->len) return kWebpDecline;
  // the VP8L header: signature, 14-bit width - 1 and height - 1, the alpha hint, version 0
  const uint8_t* q = p + w->off;
  const uint32_t bits = rd32le(q + 1);
  if (q[0] != 0x2f || (bits >> 29) != 0) return kWebpDecline;
  w->width = 1 + (int32_t)(bits & 0x3FFF);
  w->height = 1 + (int32_t)((bits >> 14) & 0x3FFF);
  if (vp8x && (cw != w->width || ch != w->height)) return kWebpDecline;
  return DINO_IMG_OK;
}

// The descriptor of a file with the signature.  A kind-6 descriptor keeps the payload's place in
// scan_off / scan_len; ncomp is 4 so that the three-component IDCT and colour kernels pass the
// image by, as they do a PNG.  Returns d->status: OK (kind 6), kWebpDecline, or what check_dims says.
DHD int parse_webp_head(const uint8_t* p, int64_t len, int max_dim, ImgDesc* d) {
  WebpWalk w;
  d->status = webp_walk(p, len, &w);
  if (d->status != DINO_IMG_OK) return d->status;
  d->kind = kWebpKind;
  d->width = w.width;
  d->height = w.height;
  if (check_dims(d, max_dim) != DINO_IMG_OK) return d->status;  // bomb: Pillow raises; side limit: hand-over
  d->ncomp = 4;
  d->color = 0;
  d->max_h = d->max_v = 1;
  d->scan_off = w.off;
  d->scan_len = w.len;
  d->coef_bytes = 0;
  return d->status;
}

}  // namespace dino
