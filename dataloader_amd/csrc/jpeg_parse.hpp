// jpeg_parse.hpp — marker-segment parser for baseline/extended sequential JPEG.
//
// Restates what libjpeg-turbo (inside Pillow, the decoder the reference calls at
// cpu.py:251) does before the first scan: jdmarker.c (SOF/DHT/DQT/DRI/SOS/APPn),
// jdapimin.c default_decompress_parms (colour-space guess), jdinput.c
// initial_setup / per_scan_setup (component and MCU geometry).  Conditions on
// which libjpeg raises (and the reference therefore zero-fills, cpu.py:252)
// map to negative statuses; JPEG flavours libjpeg decodes but this backend
// does not map to positive statuses.
#pragma once

#include "common.hpp"

namespace dino {

// jpeg_natural_order + 16 safety entries (jutils.c): zigzag index -> natural index.
constexpr uint8_t kNaturalOrder[80] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63,
    63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63};

DHD int rd16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Parse markers of one JPEG held in p[0..len).  Fills geometry, tables and the
// entropy-data offset.  Returns d->status.
// Pillow's DecompressionBombError threshold: 2 x Image.MAX_IMAGE_PIXELS (PIL/Image.py).
constexpr int64_t kPilBombPixels = 2ll * 89478485;

DHD uint32_t rd32le(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// Size checks shared by both image kinds: Pillow refuses decompression bombs at
// Image.open (the reference then zero-fills).  The bomb limit also bounds every pixel
// index of the colour / resize kernels (3 x 2 x 89478485 bytes < 2^31), so any side the
// JPEG format allows (<= 65535) decodes; a caller-chosen side limit (max_dim < 65535)
// reports DINO_IMG_LIMIT for JPEGs, which the Python layer hands to Pillow.  Raw
// containers (already Pillow's output) are only bound by the bomb limit.
DHD int check_dims(ImgDesc* d, int max_dim) {
  if ((int64_t)d->width * d->height > kPilBombPixels) return (d->status = DINO_IMG_TOO_LARGE);
  if (d->kind != 2 && (d->width > max_dim || d->height > max_dim)) return (d->status = DINO_IMG_LIMIT);
  return d->status;
}

DHD uint32_t rd32be(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

// libjpeg next_marker() (jdmarker.c): from pos, skip garbage up to an FF, then fill FFs; an FF00
// pair is garbage too (Pillow's loop skips it as "extraneous data (escaped 0xFF)").  Returns
// the marker code and sets *after to the byte after it, or -1 at the end of the data.
DHD int next_marker_at(const uint8_t* p, int64_t len, int64_t pos, int64_t* after) {
  for (;;) {
    while (pos < len && p[pos] != 0xFF) ++pos;
    if (pos >= len) return -1;
    while (pos < len && p[pos] == 0xFF) ++pos;
    if (pos >= len) return -1;
    const int c = p[pos++];
    if (c != 0) {
      *after = pos;
      return c;
    }
  }
}

// Markers that read_markers (jdmarker.c) has no case for end the decode wherever they stand:
// RES (02..BF), DHP, EXP and JPGn fall to its default (JERR_UNKNOWN_MARKER), JPG shares the
// case of the unsupported SOFs (JERR_SOF_UNSUPPORTED).
DHD bool marker_unknown_to_libjpeg(int m) {
  return (m >= 0x02 && m < 0xC0) || m == 0xC8 || m == 0xDE || m == 0xDF || (m >= 0xF0 && m <= 0xFD);
}
// Segments both walks only skip: APPn, COM (skip_variable / get_interesting_appn; Pillow's APP
// and COM handlers) and DNL (skip_variable; Pillow's Skip).  A length field below 2 costs its
// two bytes and nothing else: libjpeg skips only `if (length > 0)` after `length -= 2`, and
// Pillow's _safe_read returns b"" for a size <= 0.
DHD bool marker_skipped(int m) { return (m >= 0xE0 && m <= 0xEF) || m == 0xFE || m == 0xDC; }

// Pillow's APP handler walks the image resource blocks of an APP13 "Photoshop 3.0" segment
// (JpegImagePlugin.APP) and catches struct.error only: a block that ends right after its
// two-byte resource code leaves an IndexError at the name length (`s[offset]`), Image.open
// raises and the reference zero-fills.  s[0..n): the payload.  True: Pillow raises.
DHD bool photoshop_raises(const uint8_t* s, int n) {
  if (n < 14 || s[13] != 0) return false;
  const char* id = "Photoshop 3.0";
  for (int k = 0; k < 13; ++k)
    if (s[k] != (uint8_t)id[k]) return false;
  int64_t o = 14;
  while (o + 4 <= n && s[o] == '8' && s[o + 1] == 'B' && s[o + 2] == 'I' && s[o + 3] == 'M') {
    o += 4;
    if (o + 2 > n) return false;  // i16(s, offset): struct.error, caught
    const int code = rd16(s + o);
    o += 2;
    if (o >= n) return true;      // name_len = s[offset]: IndexError
    o += 1 + s[o];
    o += o & 1;
    if (o + 4 > n) return false;  // i32(s, offset): struct.error
    const int64_t size = rd32be(s + o);
    o += 4;
    // ResolutionInfo reads 14 bytes of the (clipped) data: struct.error on fewer
    if (code == 0x03ED && (o + size < n ? size : n - o) < 14) return false;
    o += size;
    o += o & 1;
  }
  return false;
}

// allow_raw: the caller marked this image as a pre-decoded RGB container (raw mask of
// dino_decode / dino_probe).  The container's magic is never trusted in user data: an
// unmarked file that starts with it is parsed as what it is (not a JPEG -> corrupt, as
// Pillow would raise).
// four_component: decode four-component frames (Adobe CMYK / YCCK) on the coefficient-buffer
// path (dino_ctx_set_four_component); off, they are DINO_IMG_UNSUPPORTED at the SOF marker.
DHD int parse_jpeg(const uint8_t* p, int64_t len, int max_dim, ImgDesc* d, bool allow_raw = false,
                   bool four_component = false) {
  d->status = DINO_IMG_CORRUPT;
  d->width = d->height = d->ncomp = 0;
  d->restart_interval = 0;
  d->scan_off = d->scan_len = 0;
  d->kind = 0;
  d->progressive = 0;
  d->first_sos = 0;
  d->n_scans = 0;
  d->qt_seen_mask = 0;
  d->aug_status = 0;
  d->rst_bad = 0;
  d->ent_len = d->n_rst = d->terminated = 0;  // (k_destuff_write fills them for a kind-0 image)
  d->total_blocks = 0;
  for (int i = 0; i < 8; ++i) d->huff_off[i] = -1;
  for (int t = 0; t < 4; ++t)
    for (int k = 0; k < 64; ++k) d->qt[t][k] = 0;
  bool qt_seen[4] = {false, false, false, false};
  // pre-decoded RGB container (include/dino_ingest.h DINO_RAW_MAGIC)
  if (allow_raw) {
    if (len < 16 || rd32le(p) != DINO_RAW_MAGIC) return d->status;
    const uint32_t w = rd32le(p + 4), h = rd32le(p + 8);
    if (w < 1 || h < 1 || w > 65535 || h > 65535 || (int64_t)w * h * 3 > len - 16) return d->status;
    d->kind = 2;
    d->width = (int32_t)w;
    d->height = (int32_t)h;
    d->ncomp = 3;
    d->color = kRGB;
    d->scan_off = 16;
    d->scan_len = (int32_t)((int64_t)w * h * 3 > 0x7FFFFFFF ? 0x7FFFFFFF : (int64_t)w * h * 3);
    d->status = DINO_IMG_OK;
    return check_dims(d, max_dim);
  }
  // Pillow's _accept: the file must start with FF D8 FF
  if (len < 4 || p[0] != 0xFF || p[1] != 0xD8 || p[2] != 0xFF) return d->status;

  bool saw_sof = false, saw_jfif = false, saw_adobe = false;
  int adobe_transform = 0;
  // Pillow's SOF handler sorts the APP2 "ICC_PROFILE\0" payloads seen so far and reads byte 13
  // of the first (`self.icclist[0][13]`): an IndexError, so Image.open raises, when that one is
  // shorter than 14 bytes.  All share their first 12 bytes, so the first is a 12-byte payload
  // if there is one, else the 13-byte payload with the smallest sequence byte unless a longer
  // payload has a smaller one (an equal one sorts after its 13-byte prefix).
  bool icc12 = false;
  int icc13_min = 256, icc_long_min = 256;
  int64_t pos = 2;
  for (;;) {
    int64_t after;
    int m = next_marker_at(p, len, pos, &after);
    if (m < 0) return d->status;  // no SOS: Pillow raises
    pos = after;
    if (m >= 0xD0 && m <= 0xD7) continue;  // RSTn: parameterless for both walks
    // TEM is parameterless for libjpeg, but Pillow's loop (JpegImagePlugin._open) has no FF01
    // in its MARKER table: "no marker found".  A second SOI: get_soi JERR_SOI_DUPLICATE.
    if (m == 0x01 || m == 0xD8) return d->status;
    if (m == 0xD9) return d->status;  // EOI before SOS
    if (marker_unknown_to_libjpeg(m)) return d->status;
    if (pos + 2 > len) return d->status;
    int seglen = rd16(p + pos);
    if (seglen < 2) {
      if (!marker_skipped(m)) return d->status;  // get_dqt / get_dht / get_dri / get_sof / get_sos: JERR_BAD_LENGTH
      seglen = 2;
    }
    if (pos + seglen > len) return d->status;
    const uint8_t* s = p + pos + 2;
    int n = seglen - 2;
    switch (m) {
      case 0xC0:
      case 0xC1:
      case 0xC2: {  // SOF0 baseline / SOF1 extended sequential / SOF2 progressive, Huffman
        if (saw_sof || n < 6) return (d->status = DINO_IMG_CORRUPT);
        if (icc12 || (icc13_min < 256 && icc13_min <= icc_long_min)) return (d->status = DINO_IMG_CORRUPT);
        saw_sof = true;
        d->progressive = m == 0xC2;
        int prec = s[0];
        d->height = rd16(s + 1);
        d->width = rd16(s + 3);
        int nf = s[5];
        // get_sof: `if (length != (cinfo->num_components * 3)) ERREXIT(JERR_BAD_LENGTH)`
        if (n != 6 + 3 * nf || nf <= 0) return (d->status = DINO_IMG_CORRUPT);
        // Pillow's SOF handler raises for precision != 8 and for layer counts other than
        // 1, 3, 4 (JpegImagePlugin.SOF): the reference zero-fills those
        if (prec != 8) return (d->status = DINO_IMG_CORRUPT);
        if (nf != 1 && nf != 3 && nf != 4) return (d->status = DINO_IMG_CORRUPT);
        if (nf == 4 && !four_component) return (d->status = DINO_IMG_UNSUPPORTED);  // CMYK / YCCK
        if (nf == 4) d->ncomp = 4;  // (the probes tell a four-component file by it whatever fails later)
        if (d->height == 0) return (d->status = DINO_IMG_UNSUPPORTED);  // DNL
        if (d->width == 0) return (d->status = DINO_IMG_CORRUPT);
        d->ncomp = nf;
        for (int c = 0; c < nf; ++c) {
          CompDesc& cd = d->comp[c];
          cd.id = s[6 + 3 * c];
          cd.h = s[7 + 3 * c] >> 4;
          cd.v = s[7 + 3 * c] & 15;
          cd.tq = s[8 + 3 * c];
          if (cd.h < 1 || cd.h > 4 || cd.v < 1 || cd.v > 4 || cd.tq > 3)
            return (d->status = DINO_IMG_BADDATA);
        }
        break;
      }
      case 0xC3: case 0xC5: case 0xC6: case 0xC7:
      case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE: case 0xCF:
        // lossless / hierarchical / arithmetic: left to the host (Pillow decides)
        if (n >= 1 && s[0] != 8) return (d->status = DINO_IMG_CORRUPT);  // Pillow: "cannot handle N-bit layers"
        return (d->status = DINO_IMG_UNSUPPORTED);
      case 0xCC:  // DAC: arithmetic coding
        return (d->status = DINO_IMG_UNSUPPORTED);
      case 0xC4: {  // DHT (may hold several tables)
        int q = 0;
        while (q < n) {
          if (q + 17 > n) return (d->status = DINO_IMG_CORRUPT);
          int tc = s[q] >> 4, th = s[q] & 15;
          int cnt = 0;
          for (int i = 1; i <= 16; ++i) cnt += s[q + i];
          if (cnt > 256 || q + 17 + cnt > n || tc > 1 || th > 3) return (d->status = DINO_IMG_CORRUPT);
          d->huff_off[tc * 4 + th] = (int32_t)(pos + 2 + q + 1);
          q += 17 + cnt;
        }
        break;
      }
      case 0xDB: {  // DQT
        int q = 0;
        while (q < n) {
          int pq = s[q] >> 4, tq = s[q] & 15;
          // get_dqt: `prec = n >> 4 ... if (prec) 16-bit`; Pillow's DQT: `1 if v // 16 == 0 else 2`
          // bytes: any non-zero precision nibble is a 16-bit table
          if (tq > 3) return (d->status = DINO_IMG_CORRUPT);
          int need = pq ? 128 : 64;
          if (q + 1 + need > n) return (d->status = DINO_IMG_CORRUPT);
          for (int k = 0; k < 64; ++k) {
            int v = pq ? rd16(s + q + 1 + 2 * k) : s[q + 1 + k];
            d->qt[tq][kNaturalOrder[k]] = (uint16_t)v;
          }
          qt_seen[tq] = true;
          q += 1 + need;
        }
        break;
      }
      case 0xDD:  // DRI (get_dri: `if (length != 4) ERREXIT(JERR_BAD_LENGTH)`)
        if (n != 2) return (d->status = DINO_IMG_CORRUPT);
        d->restart_interval = rd16(s);
        break;
      case 0xE0:  // APP0: JFIF?
        if (n >= 4 && s[0] == 'J' && s[1] == 'F' && s[2] == 'I' && s[3] == 'F') {
          // Pillow's APP handler reads the version at payload bytes 5..6 of anything that
          // starts with "JFIF" and raises on a shorter one (the reference zero-fills)
          if (n < 7) return (d->status = DINO_IMG_CORRUPT);
          // jdmarker.c examine_app0: JFIF only with the whole 14-byte header (APP0_DATA_LEN)
          if (n >= 14 && s[4] == 0) saw_jfif = true;
        }
        break;
      case 0xE2:  // APP2: ICC profile chunks before the frame header (see icc12 above)
        if (!saw_sof && n >= 12) {
          const char* id = "ICC_PROFILE";
          bool is_icc = s[11] == 0;
          for (int k = 0; k < 11; ++k) is_icc = is_icc && s[k] == (uint8_t)id[k];
          if (is_icc) {
            if (n == 12) icc12 = true;
            else if (n == 13) icc13_min = s[12] < icc13_min ? s[12] : icc13_min;
            else icc_long_min = s[12] < icc_long_min ? s[12] : icc_long_min;
          }
        }
        break;
      case 0xED:  // APP13: Photoshop image resources
        if (photoshop_raises(s, n)) return (d->status = DINO_IMG_CORRUPT);
        break;
      case 0xEE:  // APP14: Adobe transform flag
        if (n >= 5 && s[0] == 'A' && s[1] == 'd' && s[2] == 'o' && s[3] == 'b' && s[4] == 'e') {
          if (n < 7) return (d->status = DINO_IMG_CORRUPT);  // Pillow reads the version at bytes 5..6
          if (n >= 12) {  // examine_app14: APP14_DATA_LEN
            saw_adobe = true;
            adobe_transform = s[11];
          }
        }
        break;
      case 0xDA: {  // SOS
        if (!saw_sof || n < 1) return (d->status = DINO_IMG_CORRUPT);
        int ns = s[0];
        // get_sos: `if (length != (n * 2 + 6) || n < 1 || n > MAX_COMPS_IN_SCAN) ERREXIT(JERR_BAD_LENGTH)`
        if (n != 4 + 2 * ns || ns < 1 || ns > 4) return (d->status = DINO_IMG_CORRUPT);
        // One interleaved scan of every component in frame order decodes on the
        // baseline path; anything else (progressive, components spread over several
        // scans, another component order) on the coefficient-buffer path (k_prog),
        // whose marker walk re-reads this SOS.
        d->first_sos = (int32_t)(pos - 2);  // (a baseline image may still move to k_prog, k_destuff_write)
        // (a four-component frame always takes the coefficient-buffer path: the speculative
        // Huffman kernels are sized for kMaxComp components)
        bool one_scan = !d->progressive && ns == d->ncomp && d->ncomp <= kMaxComp;
        for (int k = 0; k < ns && one_scan; ++k) {
          int cs = s[1 + 2 * k];
          int ci = -1;
          for (int c = 0; c < d->ncomp; ++c)
            if (d->comp[c].id == cs) ci = c;
          if (ci != k) one_scan = false;
        }
        if (!one_scan) {
          d->kind = 1;
          d->scan_off = (int32_t)(pos + seglen);
          d->scan_len = (int32_t)(len - d->scan_off);
          goto have_scan;
        }
        for (int k = 0; k < ns; ++k) {
          int t = s[2 + 2 * k];
          d->comp[k].td = t >> 4;
          d->comp[k].ta = t & 15;
          if (d->comp[k].td > 3 || d->comp[k].ta > 3) return (d->status = DINO_IMG_CORRUPT);
        }
        // Ss/Se/Ah/Al of a sequential scan are ignored (libjpeg: JWRN_NOT_SEQUENTIAL warning)
        d->scan_off = (int32_t)(pos + seglen);
        d->scan_len = (int32_t)(len - d->scan_off);
        goto have_scan;
      }
      default:
        break;  // APPn, COM, DNL: skipped
    }
    pos += seglen;
  }

have_scan:
  d->status = DINO_IMG_OK;
  if (check_dims(d, max_dim) != DINO_IMG_OK) return d->status;
  d->status = DINO_IMG_CORRUPT;
  for (int t = 0; t < 4; ++t) d->qt_seen_mask |= qt_seen[t] ? 1 << t : 0;
  if (d->kind == 0) {  // (kind 1: tables and quant latching are checked per scan by prog_walk)
    for (int c = 0; c < d->ncomp; ++c) {
      const CompDesc& cd = d->comp[c];
      if (!qt_seen[cd.tq]) return (d->status = DINO_IMG_CORRUPT);  // libjpeg JERR_NO_QUANT_TABLE
      if (d->huff_off[cd.td] < 0 || d->huff_off[4 + cd.ta] < 0)
        return (d->status = DINO_IMG_CORRUPT);                      // JERR_NO_HUFF_TABLE
    }
  }
  // colour space (jdapimin.c default_decompress_parms)
  if (d->ncomp == 1) {
    d->color = kGray;
  } else if (d->ncomp == 4) {
    // case 4: an Adobe marker with transform 0 is CMYK, 2 is YCCK, any other value YCCK
    // too (WARNMS1 JWRN_ADOBE_XFORM); without an Adobe marker CMYK.  JFIF plays no part.
    d->color = saw_adobe && adobe_transform != 0 ? kYCCK : kCMYK;
  } else if (saw_jfif) {
    d->color = kYCbCr;
  } else if (saw_adobe) {
    d->color = adobe_transform == 0 ? kRGB : kYCbCr;
  } else if (d->comp[0].id == 82 && d->comp[1].id == 71 && d->comp[2].id == 66) {
    d->color = kRGB;
  } else {
    d->color = kYCbCr;
  }
  // geometry (jdinput.c initial_setup / per_scan_setup)
  int mh = 1, mv = 1;
  for (int c = 0; c < d->ncomp; ++c) {
    mh = d->comp[c].h > mh ? d->comp[c].h : mh;
    mv = d->comp[c].v > mv ? d->comp[c].v : mv;
  }
  d->max_h = mh;
  d->max_v = mv;
  for (int c = 0; c < d->ncomp; ++c) {
    CompDesc& cd = d->comp[c];
    // jdsample.c: only integral upsampling ratios are implemented
    if (mh % cd.h != 0 || mv % cd.v != 0) return (d->status = DINO_IMG_BADDATA);
    cd.dw = (int32_t)(((int64_t)d->width * cd.h + mh - 1) / mh);
    cd.dh = (int32_t)(((int64_t)d->height * cd.v + mv - 1) / mv);
  }
  if (d->ncomp == 1) {
    CompDesc& cd = d->comp[0];
    d->mcus_x = ceil_div(cd.dw, 8);
    d->mcus_y = ceil_div(cd.dh, 8);
    d->blocks_per_mcu = 1;
    cd.bw = d->mcus_x;
    cd.bh = d->mcus_y;
    d->mcu_comp[0] = 0;
    d->mcu_bx[0] = 0;
    d->mcu_by[0] = 0;
  } else {
    d->mcus_x = ceil_div(d->width, 8 * mh);
    d->mcus_y = ceil_div(d->height, 8 * mv);
    // libjpeg limits the blocks of an MCU per interleaved scan (per_scan_setup,
    // JERR_BAD_MCU_SIZE), not per frame: the one scan of a kind-0 image holds every
    // component; a kind-1 image is checked scan by scan (prog_walk) and never reads the
    // frame's MCU table, which stays empty when the frame's blocks do not fit it
    int frame_blocks = 0;
    for (int c = 0; c < d->ncomp; ++c) frame_blocks += d->comp[c].h * d->comp[c].v;
    const bool fits = frame_blocks <= kMaxBlocksPerMcu;
    if (!fits && d->kind == 0) return (d->status = DINO_IMG_BADDATA);
    int b = 0;
    for (int c = 0; c < d->ncomp; ++c) {
      CompDesc& cd = d->comp[c];
      for (int y = 0; y < cd.v && fits; ++y)
        for (int x = 0; x < cd.h; ++x) {
          d->mcu_comp[b] = (uint8_t)c;
          d->mcu_bx[b] = (uint8_t)x;
          d->mcu_by[b] = (uint8_t)y;
          ++b;
        }
      cd.bw = d->mcus_x * cd.h;
      cd.bh = d->mcus_y * cd.v;
    }
    d->blocks_per_mcu = b;
  }
  int64_t mcus = (int64_t)d->mcus_x * d->mcus_y;
  d->total_blocks = (int32_t)(mcus * d->blocks_per_mcu);
  d->n_rst_max = d->restart_interval > 0 ? (int32_t)((mcus + d->restart_interval - 1) / d->restart_interval) : 0;
  int64_t co = 0, po = 0;
  for (int c = 0; c < d->ncomp; ++c) {
    CompDesc& cd = d->comp[c];
    cd.coef_off = co;
    cd.plane_off = po;
    co += (int64_t)cd.bw * cd.bh * 128;
    po += (int64_t)cd.bw * cd.bh * 64;
  }
  d->coef_bytes = co;
  d->status = DINO_IMG_OK;
  return d->status;
}

// Per-image workspace sizes (bytes), used by k_plan.
DHD int64_t align16(int64_t x) { return (x + 15) & ~(int64_t)15; }

}  // namespace dino
