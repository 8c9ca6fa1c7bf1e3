// probe.hpp — host pre-screen of one image (dino_probe / dino_probe_spans /
// dino_gather_probe / the native feed): the device parser run on the CPU.
#pragma once

#include "jpeg_parse.hpp"
#include "plan.hpp"
#include "png_parse.hpp"
#include "progressive.hpp"

namespace dino {

constexpr int32_t kMaxImageDim = 65535;

// One image of dino_probe / dino_probe_spans / dino_gather_probe: its info row and workspace bytes.
inline void probe_one(const uint8_t* p, int64_t len, bool raw, int32_t max_image_dim, const dino_aug_config* cfg,
               ScanRec* scans, int32_t* info_row, int64_t* ws, int64_t* aws) {
  ImgDesc d;
  // A file with the PNG signature keeps the status every context without dino_ctx_set_png gives
  // it (DINO_IMG_CORRUPT); the kind says what a context with the option on does: 4, decodes it
  // (its workspace and views are counted, as for kind 3), or 5, declines it (bit depths other
  // than 8, Adam7, APNG, chunks the walk does not verify, a side above max_image_dim).  A PNG
  // on which Pillow raises keeps kind -1.
  if (len > 0 && !raw && png_signature(p, len)) {
    d.kind = 0;
    d.width = d.height = 0;
    int st = parse_png_head(p, len, max_image_dim, &d);
    PngWalk w;
    if (st == DINO_IMG_OK) st = png_walk(p, len, d.color, &w);
    const bool dev = st == DINO_IMG_OK, declined = st > 0;
    if (info_row) {
      info_row[0] = DINO_IMG_CORRUPT;
      info_row[1] = dev ? d.width : 0;
      info_row[2] = dev ? d.height : 0;
      info_row[3] = dev ? kPngKind : (declined ? kPngKindDeclined : -1);
    }
    if (!dev) return;
    d.status = DINO_IMG_OK;
    *ws += image_chunk_bytes(d).total();
    if (cfg) {
      for (int v = 0; v < cfg->n_global + cfg->n_local; ++v)
        *aws += view_scratch_bound(v < cfg->n_global ? cfg->global_size : cfg->local_size, d.width, d.height);
    }
    return;
  }
  if (len <= 0) {
    d.status = DINO_IMG_CORRUPT;
    d.width = d.height = d.ncomp = 0;
  } else {
    // a probe has no context: a four-component frame is parsed as a context with
    // dino_ctx_set_four_component on would, and reported below as kind 3
    parse_jpeg(p, len, max_image_dim, &d, raw, true);
    // a table that a scan uses and libjpeg rejects (JERR_BAD_HUFF_TABLE) fails the image in
    // k_htab / k_pwalk: the same check here, so that the status is the decode's
    HuffDerived tab;
    if (d.status == DINO_IMG_OK && d.kind == 0) {
      for (int c = 0; c < d.ncomp; ++c)
        if (!huff_build_derived(p + d.huff_off[d.comp[c].td], true, &tab) ||
            !huff_build_derived(p + d.huff_off[4 + d.comp[c].ta], false, &tab))
          d.status = DINO_IMG_CORRUPT;
    }
    if (d.status == DINO_IMG_OK && d.kind == 1) {
      HostMarkerFinder find;
      if (prog_walk(p, len, &d, scans, find) == DINO_IMG_OK) {
        // k_pwalk's table slots: more distinct tables than the region holds -> Pillow
        int32_t slot_off[kPMaxTabs];
        uint8_t slot_dc[kPMaxTabs];
        uint64_t ts[kMaxScans];
        const int ntab = prog_table_slots(scans, d.n_scans, slot_off, slot_dc, ts, kPMaxTabs);
        if (ntab < 0) d.status = DINO_IMG_UNSUPPORTED;
        for (int s = 0; s < ntab; ++s)
          if (!huff_build_derived(p + slot_off[s], slot_dc[s] != 0, &tab)) d.status = DINO_IMG_CORRUPT;
      }
    }
  }
  // Four components: status DINO_IMG_UNSUPPORTED whatever else the file is (what a context
  // with the option off reports at the SOF marker), and kind 3 when a context with the option
  // on decodes it; its workspace is counted then, so that a dino_reserve from these numbers
  // covers it (a little too much for a context that hands the file over instead).
  const bool four = d.ncomp == 4;
  const bool counted = d.status == DINO_IMG_OK;
  if (four) d.status = DINO_IMG_UNSUPPORTED;
  if (info_row) {
    info_row[0] = d.status;
    info_row[1] = d.status == DINO_IMG_OK || d.status > 0 ? d.width : 0;
    info_row[2] = d.status == DINO_IMG_OK || d.status > 0 ? d.height : 0;
    info_row[3] = !counted ? -1 : (four ? 3 : d.kind);
  }
  if (!counted) return;
  d.status = DINO_IMG_OK;
  *ws += image_chunk_bytes(d).total();
  if (cfg) {
    for (int v = 0; v < cfg->n_global + cfg->n_local; ++v)
      *aws += view_scratch_bound(v < cfg->n_global ? cfg->global_size : cfg->local_size, d.width, d.height);
  }
}

}  // namespace dino
