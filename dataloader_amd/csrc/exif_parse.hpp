// exif_parse.hpp — the EXIF Orientation tag of a JPEG as Pillow 12.2.0 reads it, and the eight
// orientations as one mapping (k_exif / k_orient in kernels_orient.inc, dino_probe_orient).
//
// What ImageOps.exif_transpose acts on is Image.getexif().get(0x0112):
//  * JpegImagePlugin.APP keeps the payload of the first APP1 segment that starts with
//    "Exif\0\0" in info["exif"] and appends the payload of every later one to it; an APP1 payload
//    that starts with "http://ns.adobe.com/xap/1.0/\0" becomes info["xmp"].  Only the segments
//    before the first SOS are read (JpegImageFile._open stops there).
//  * Image.getexif hands info["exif"] to Exif.load: the "Exif\0\0" prefixes are stripped, the next
//    8 bytes are a TIFF header (TiffImagePlugin.ImageFileDirectory_v2: "II*\0" or "MM\0*", else
//    SyntaxError) whose last 4 bytes seek to IFD0, and ImageFileDirectory_v2.load reads a 2-byte
//    entry count and 12-byte entries (tag, type, count, 4 value bytes), a later entry of a tag
//    replacing an earlier one; running out of bytes ends the load with a warning and keeps the
//    entries read so far.  When that gave no Orientation, getexif searches info["xmp"] for
//    tiff:Orientation.
//  * ImageOps.exif_transpose maps 2..8 to a transpose method and leaves every other value alone.
// The rule is png_parse.hpp's: the walk answers an orientation, or "none", only where it has
// verified every step above on the plain form a camera writes; whatever else it meets is
// "unverified" and Pillow decides (the caller hands the file over).
#pragma once

#include "jpeg_parse.hpp"

namespace dino {

constexpr int kOrientNone = 0;          // no tag, or the value 1: the image stays as it is
constexpr int kOrientUnverified = 255;  // Pillow decides

DHD bool bytes_start(const uint8_t* s, int n, const char* id, int k) {
  if (n < k) return false;
  for (int i = 0; i < k; ++i)
    if (s[i] != (uint8_t)id[i]) return false;
  return true;
}

// The payload of an "Exif\0\0" APP1 segment after those 6 bytes, t[0..n): 1..8, kOrientNone (a
// well-formed IFD0 without the tag) or kOrientUnverified.
DHD int tiff_orientation(const uint8_t* t, int n) {
  if (n < 8) return kOrientUnverified;  // (an empty or cut header: Exif.load returns early or raises)
  const bool le = t[0] == 'I' && t[1] == 'I' && t[2] == 0x2A && t[3] == 0;
  const bool be = t[0] == 'M' && t[1] == 'M' && t[2] == 0 && t[3] == 0x2A;
  if (!le && !be) return kOrientUnverified;  // BigTIFF, the swapped magics Pillow also accepts, a second "Exif\0\0"
  const uint32_t off = le ? rd32le(t + 4) : rd32be(t + 4);
  if (off < 8 || (int64_t)off + 2 > n) return kOrientUnverified;
  const int cnt = le ? (t[off] | (t[off + 1] << 8)) : rd16(t + off);
  if ((int64_t)off + 2 + 12 * (int64_t)cnt > n) return kOrientUnverified;  // (Pillow keeps the entries before the cut)
  int found = kOrientNone, seen = 0;
  for (int k = 0; k < cnt; ++k) {
    const uint8_t* e = t + off + 2 + 12 * k;
    const int tag = le ? (e[0] | (e[1] << 8)) : rd16(e);
    if (tag != 0x0112) continue;
    if (++seen > 1) return kOrientUnverified;
    const int typ = le ? (e[2] | (e[3] << 8)) : rd16(e + 2);
    const uint32_t count = le ? rd32le(e + 4) : rd32be(e + 4);
    const int v = le ? (e[8] | (e[9] << 8)) : rd16(e + 8);
    if (typ != 3 || count != 1 || v < 1 || v > 8) return kOrientUnverified;
    found = v;
  }
  return found;
}

// The orientation of the JPEG p[0..len): kOrientNone, 2..8 or kOrientUnverified.  The marker
// walk is parse_jpeg's (next_marker_at, the length rules of marker_skipped); a file on which that
// parse fails gets no decode either way, so what the walk answers there does not matter.
DHD int exif_orientation(const uint8_t* p, int64_t len) {
  if (len < 4 || p[0] != 0xFF || p[1] != 0xD8 || p[2] != 0xFF) return kOrientNone;
  int exif = -1;  // -1: no Exif segment yet
  bool xmp = false;
  int64_t pos = 2;
  for (;;) {
    int64_t after;
    const int m = next_marker_at(p, len, pos, &after);
    if (m < 0 || m == 0xDA) break;
    pos = after;
    if (m >= 0xD0 && m <= 0xD7) continue;
    if (m == 0x01 || m == 0xD8 || m == 0xD9 || marker_unknown_to_libjpeg(m)) break;
    if (pos + 2 > len) break;
    int seglen = rd16(p + pos);
    if (seglen < 2) {
      if (!marker_skipped(m)) break;
      seglen = 2;
    }
    if (pos + seglen > len) break;
    const uint8_t* s = p + pos + 2;
    const int n = seglen - 2;
    if (m == 0xE1) {
      if (bytes_start(s, n, "Exif\0\0", 6)) {
        if (exif >= 0) return kOrientUnverified;  // Pillow joins the payloads
        exif = tiff_orientation(s + 6, n - 6);
        if (exif == kOrientUnverified) return exif;
      } else if (bytes_start(s, n, "http://ns.adobe.com/xap/1.0/\0", 29)) {
        xmp = true;
      }
    }
    pos += seglen;
  }
  if (exif >= 1) return exif == 1 ? kOrientNone : exif;
  return xmp ? kOrientUnverified : kOrientNone;  // getexif searches the packet for tiff:Orientation
}

// The eight orientations, once.  Pillow's exif_transpose table reads 2 FLIP_LEFT_RIGHT, 3
// ROTATE_180, 4 FLIP_TOP_BOTTOM, 5 TRANSPOSE, 6 ROTATE_270, 7 TRANSVERSE, 8 ROTATE_90, with
// rotations counter-clockwise; here an orientation o is three bits of o - 1 and nothing else:
//   swap = bit 2        the output's columns run along the source's rows (5..8): OW = H, OH = W
//   fy   = bit 1        the output's rows are mirrored (3, 4, 7, 8)
//   fx   = bit 0 ^ bit 1   the output's columns are mirrored (2, 3, 6, 7)
// Source pixel (x, y) of a W x H image goes to (ox, oy): with (u, v) = swap ? (y, x) : (x, y),
// ox = fx ? OW - 1 - u : u and oy = fy ? OH - 1 - v : v.  The mapping is its own inverse with
// (W, H) and (OW, OH) exchanged, which is how k_orient reads it (output position -> source).
struct OrientMap {
  bool swap, fx, fy;
};
DHD OrientMap orient_map(int o) {
  const int b = (o - 1) & 7;
  return {(b & 4) != 0, ((b ^ (b >> 1)) & 1) != 0, (b & 2) != 0};
}
DHD void orient_forward(int o, int W, int H, int x, int y, int* ox, int* oy) {
  const OrientMap m = orient_map(o);
  const int OW = m.swap ? H : W, OH = m.swap ? W : H;
  const int u = m.swap ? y : x, v = m.swap ? x : y;
  *ox = m.fx ? OW - 1 - u : u;
  *oy = m.fy ? OH - 1 - v : v;
}

}  // namespace dino
