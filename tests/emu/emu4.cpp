// Host emulator of the four-component (CMYK / YCCK) decode — TEST INFRASTRUCTURE ONLY.
//
// Like emu.cpp, this compiles the __host__ __device__ functions the kernels use
// (dataloader_amd/csrc/*.hpp) for the CPU: the parser with the four-component option on,
// the marker walk and scan decoders of the coefficient-buffer path (k_pwalk / k_pscan),
// idct_block per plane (k_idct) and four_to_rgb per pixel (k_color4).  The product library
// never links this file.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../dataloader_amd/csrc/color.hpp"
#include "../../dataloader_amd/csrc/idct.hpp"
#include "../../dataloader_amd/csrc/jpeg_parse.hpp"
#include "../../dataloader_amd/csrc/pscan.hpp"

using namespace dino;

extern "C" {

// out[3 i ..] = four_to_rgb of the samples s[4 i ..] as libjpeg hands them over.
void emu4_four_to_rgb(const uint8_t* s, int64_t n, int ycck, uint8_t* out) {
  for (int64_t i = 0; i < n; ++i) four_to_rgb(s[4 * i], s[4 * i + 1], s[4 * i + 2], s[4 * i + 3], ycck != 0, out + 3 * i);
}

// info = {status, width, height, ncomp, color, kind}
int emu4_parse(const uint8_t* p, int64_t len, int four_component, int32_t* info) {
  ImgDesc d;
  parse_jpeg(p, len, 1 << 16, &d, false, four_component != 0);
  info[0] = d.status;
  info[1] = d.width;
  info[2] = d.height;
  info[3] = d.ncomp;
  info[4] = d.color;
  info[5] = d.kind;
  return d.status;
}

// Decode with the option on (any component count the parser accepts): out_rgb w*h*3.
int emu4_decode(const uint8_t* p, int64_t len, uint8_t* out_rgb) {
  ImgDesc d;
  if (parse_jpeg(p, len, 1 << 16, &d, false, true) != DINO_IMG_OK) return d.status;
  if (d.kind != 1) return 100;  // (the three-component kinds are emu.cpp's)
  std::vector<ScanRec> scans(kMaxScans);
  HostMarkerFinder find;
  if (prog_walk(p, len, &d, scans.data(), find) != DINO_IMG_OK) return d.status;
  std::vector<int32_t> slot_off(kPMaxTabs);
  std::vector<uint8_t> slot_dc(kPMaxTabs);
  std::vector<uint64_t> ts(kMaxScans);
  const int ntab = prog_table_slots(scans.data(), d.n_scans, slot_off.data(), slot_dc.data(), ts.data(), kPMaxTabs);
  if (ntab < 0) return DINO_IMG_UNSUPPORTED;
  std::vector<PTab> tabs(ntab > 0 ? ntab : 1);
  for (int s = 0; s < ntab; ++s) {
    ProgTable t;
    if (!huff_build_derived(p + slot_off[s], slot_dc[s] != 0, &t)) return DINO_IMG_CORRUPT;
    ptab_fill_derived(&t, &tabs[s]);
    for (int i = 0; i < (1 << kPLookBits); ++i) tabs[s].look[i] = ptab_look_entry(&t, i);
  }
  std::vector<int16_t> coef(d.coef_bytes / 2, 0);
  std::vector<uint8_t> clean(len + 16, 0);
  for (int i = 0; i < d.n_scans; ++i) {
    const ScanRec& sr = scans[i];
    HostCoefSink sink{coef.data()};
    const HostTabs tb{tabs.data(), ts[i]};
    if (sr.restart_interval == 0) {
      HostClean r{clean.data(), host_destuff(p, len, sr.data_off, clean.data())};
      pscan_decode(r, tb, &d, sr, d.progressive != 0, sink);
      std::fill(clean.begin(), clean.end(), 0);
    } else {
      RawReader r;
      pb_init(r.b, (uintptr_t)p, len, sr.data_off);
      pscan_decode(r, tb, &d, sr, d.progressive != 0, sink);
    }
  }
  int64_t psz = 0;
  for (int c = 0; c < d.ncomp; ++c) psz += (int64_t)d.comp[c].bw * d.comp[c].bh * 64;
  std::vector<uint8_t> planes(psz);
  PlaneView pv[kMaxFrameComp];
  for (int c = 0; c < d.ncomp; ++c) {
    const CompDesc& cd = d.comp[c];
    const int pitch = cd.bw * 8;
    for (int by = 0; by < cd.bh; ++by)
      for (int bx = 0; bx < cd.bw; ++bx)
        idct_block(coef.data() + cd.coef_off / 2 + ((int64_t)by * cd.bw + bx) * 64, d.qt[cd.tq],
                   planes.data() + cd.plane_off + (int64_t)by * 8 * pitch + bx * 8, pitch);
    pv[c].p = planes.data() + cd.plane_off;
    pv[c].pitch = pitch;
    pv[c].dw = cd.dw;
    pv[c].dh = cd.dh;
    pv[c].hf = d.max_h / cd.h;
    pv[c].vf = d.max_v / cd.v;
    pv[c].method = upsample_method(pv[c].hf, pv[c].vf, cd.dw);
  }
  for (int y = 0; y < d.height; ++y)
    for (int x = 0; x < d.width; ++x) {
      uint8_t* o = out_rgb + ((int64_t)y * d.width + x) * 3;
      if (d.ncomp == 4) {
        four_to_rgb(upsample_at(pv[0], x, y), upsample_at(pv[1], x, y), upsample_at(pv[2], x, y), upsample_at(pv[3], x, y),
                    d.color == kYCCK, o);
      } else if (d.ncomp == 1) {
        o[0] = o[1] = o[2] = (uint8_t)upsample_at(pv[0], x, y);
      } else {
        const int a = upsample_at(pv[0], x, y), b = upsample_at(pv[1], x, y), c = upsample_at(pv[2], x, y);
        if (d.color == kYCbCr) {
          ycc_to_rgb(a, b, c, o);
        } else {
          o[0] = (uint8_t)a;
          o[1] = (uint8_t)b;
          o[2] = (uint8_t)c;
        }
      }
    }
  return DINO_IMG_OK;
}

}  // extern "C"
