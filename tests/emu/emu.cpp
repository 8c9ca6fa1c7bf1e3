// Host emulator of the HIP kernels' per-lane logic — TEST INFRASTRUCTURE ONLY.
//
// Compiles the very same __host__ __device__ functions the kernels use
// (dataloader_amd/csrc/*.hpp) for the CPU, and drives them with plain loops
// that mimic the kernels' lane/phase structure, so the CPU test suite can
// check the device algorithms against Pillow without a GPU.  The product
// library never links this file.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../dataloader_amd/csrc/color.hpp"
#include "../../dataloader_amd/csrc/huffman.hpp"
#include "../../dataloader_amd/csrc/idct.hpp"
#include "../../dataloader_amd/csrc/jpeg_parse.hpp"
#include "../../dataloader_amd/csrc/pixel_ops.hpp"
#include "../../dataloader_amd/csrc/resize.hpp"
#include "../../dataloader_amd/csrc/hresize_tile.hpp"
#include "../../dataloader_amd/csrc/plan.hpp"
#include "../../dataloader_amd/csrc/augment.hpp"
#include "../../dataloader_amd/csrc/mask.hpp"
#include "models.hpp"
#include "../../dataloader_amd/csrc/sampler.hpp"

using namespace dino;

extern "C" {

// ---- exhaustive pixel-op tables --------------------------------------------
void emu_rgb_to_hsv_all(uint8_t* out) {
  for (int r = 0; r < 256; ++r)
    for (int g = 0; g < 256; ++g)
      for (int b = 0; b < 256; ++b) {
        int h, s, v;
        rgb_to_hsv(r, g, b, &h, &s, &v);
        size_t i = (((size_t)r << 16) | (g << 8) | b) * 3;
        out[i] = (uint8_t)h;
        out[i + 1] = (uint8_t)s;
        out[i + 2] = (uint8_t)v;
      }
}

void emu_hsv_to_rgb_all(uint8_t* out) {
  for (int h = 0; h < 256; ++h)
    for (int s = 0; s < 256; ++s)
      for (int v = 0; v < 256; ++v) {
        int r, g, b;
        hsv_to_rgb(h, s, v, &r, &g, &b);
        size_t i = (((size_t)h << 16) | (s << 8) | v) * 3;
        out[i] = (uint8_t)r;
        out[i + 1] = (uint8_t)g;
        out[i + 2] = (uint8_t)b;
      }
}

void emu_rgb_to_l_all(uint8_t* out) {
  for (int r = 0; r < 256; ++r)
    for (int g = 0; g < 256; ++g)
      for (int b = 0; b < 256; ++b) out[((size_t)r << 16) | (g << 8) | b] = (uint8_t)rgb_to_l(r, g, b);
}

// out[a*256+b] = blend(a, b, alpha)
void emu_blend_table(float alpha, uint8_t* out) {
  for (int a = 0; a < 256; ++a)
    for (int b = 0; b < 256; ++b) out[a * 256 + b] = blend_u8(a, b, alpha);
}

void emu_normalize(const uint8_t* in, int64_t n, float mean, float std, uint16_t* bf16_out, float* f32_out) {
  for (int64_t i = 0; i < n; ++i) {
    float v = u8_normalize(in[i], mean, std);
    f32_out[i] = v;
    bf16_out[i] = f32_to_bf16(v);
  }
}

void emu_fp8(const float* in, int64_t n, uint8_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = f32_to_fp8e4m3(in[i]);
}

// ---- JPEG -------------------------------------------------------------------
int emu_parse(const uint8_t* p, int64_t len, int32_t* info /* status,w,h,ncomp,color,bpm,ri,scan_off */) {
  ImgDesc d;
  parse_jpeg(p, len, 1 << 16, &d);
  info[0] = d.status;
  info[1] = d.width;
  info[2] = d.height;
  info[3] = d.ncomp;
  info[4] = d.color;
  info[5] = d.blocks_per_mcu;
  info[6] = d.restart_interval;
  info[7] = d.scan_off;
  return d.status;
}

// Full decode through the kernel-model pipeline.  mode 0: sequential Huffman,
// mode 1: speculative parallel Huffman with `lanes` lanes.  out_rgb: w*h*3.
// stats (nullable): int32[4] = {sync rounds, redecoded subsequences, lanes used, 0}
int emu_decode(const uint8_t* p, int64_t len, int mode, int lanes, uint8_t* out_rgb, int32_t* stats) {
  return host_model_decode(p, len, mode, lanes, out_rgb, stats);
}

// Stage outputs of the decode model (for GPU debugging): sizes returned in sizes[3].
int emu_decode_stages(const uint8_t* p, int64_t len, int mode, int lanes, uint8_t* rgb, uint8_t* ent, int64_t ent_cap,
                      int16_t* coef, int64_t coef_cap, uint8_t* planes, int64_t plane_cap, int64_t* sizes) {
  StageCapture cap;
  int r = host_model_decode(p, len, mode, lanes, rgb, nullptr, &cap);
  sizes[0] = (int64_t)cap.ent.size();
  sizes[1] = (int64_t)cap.coef.size() * 2;
  sizes[2] = (int64_t)cap.planes.size();
  if (ent) memcpy(ent, cap.ent.data(), std::min<int64_t>(ent_cap, sizes[0]));
  if (coef) memcpy(coef, cap.coef.data(), std::min<int64_t>(coef_cap, sizes[1]));
  if (planes) memcpy(planes, cap.planes.data(), std::min<int64_t>(plane_cap, sizes[2]));
  return r;
}

// ---- destuffing ---------------------------------------------------------------
// model_destuff over a scan of n bytes: info = {len, n_rst, terminated, rst_bad}; the bytes
// with their zero pad into `bytes` (up to cap; returns how many there are) and the restart
// offsets into `rst` (up to rst_cap).
int64_t emu_destuff(const uint8_t* scan, int n, uint8_t* bytes, int64_t cap, int32_t* rst, int32_t rst_cap,
                    int32_t* info) {
  const Destuffed d = model_destuff(scan, n);
  info[0] = d.len;
  info[1] = (int32_t)d.rst.size();
  info[2] = d.terminated;
  info[3] = d.rst_bad;
  memcpy(bytes, d.bytes.data(), (size_t)std::min<int64_t>(cap, (int64_t)d.bytes.size()));
  memcpy(rst, d.rst.data(), 4 * (size_t)std::min<int64_t>(rst_cap, (int64_t)d.rst.size()));
  return (int64_t)d.bytes.size();
}

// ds_parts of a baseline scan of scan_len bytes, and ds_part_role (plan.hpp)
int emu_ds_parts(int scan_len) {
  ImgDesc d{};
  d.status = DINO_IMG_OK;
  d.kind = 0;
  d.scan_len = scan_len;
  return ds_parts(d);
}

// over every part of one image: out[2 p] = writes, out[2 p + 1] = finalises
void emu_ds_part_roles(int lead, int n, int E, int ds_items, uint8_t* out) {
  for (int p = 0; p < ds_items; ++p) {
    const DsRole r = ds_part_role(p, lead, n, E, ds_items);
    out[2 * p] = r.writes;
    out[2 * p + 1] = r.finalises;
  }
}

// offsetof of the descriptor fields k_destuff_write fills (dino_debug_region 0):
// out = {status, scan_off, scan_len, ent_len, n_rst, terminated, rst_bad, sizeof(ImgDesc)}.
void emu_desc_layout(int32_t* out) {
  const size_t v[8] = {offsetof(ImgDesc, status),  offsetof(ImgDesc, scan_off),   offsetof(ImgDesc, scan_len),
                       offsetof(ImgDesc, ent_len), offsetof(ImgDesc, n_rst),      offsetof(ImgDesc, terminated),
                       offsetof(ImgDesc, rst_bad), sizeof(ImgDesc)};
  for (int i = 0; i < 8; ++i) out[i] = (int32_t)v[i];
}

// Per-scan symbol counts of a multi-scan image (analysis aid): out[i] = symbols of scan
// i, levels[i] = its dependency level; returns the number of scans (< 0: status).
int emu_prog_scan_stats(const uint8_t* p, int64_t len, int64_t* out, int32_t* levels, int32_t cap) {
  ImgDesc d;
  if (parse_jpeg(p, len, 1 << 16, &d) != DINO_IMG_OK || d.kind != 1) return -1;
  std::vector<ScanRec> scans(kMaxScans);
  HostMarkerFinder find;
  if (prog_walk(p, len, &d, scans.data(), find) != DINO_IMG_OK) return d.status;
  std::vector<int16_t> coef(d.coef_bytes / 2, 0);
  std::vector<ProgTable> tabs(8);
  for (int i = 0; i < d.n_scans && i < cap; ++i) {
    const ScanRec& sr = scans[i];
    ScanTables tb;
    for (int k = 0; k < 4; ++k) {
      tb.dc[k] = tb.ac[k] = &tabs[0];
      if (sr.dc_tab[k] >= 0 && prog_build_table(p + sr.dc_tab[k], true, &tabs[k])) tb.dc[k] = &tabs[k];
      if (sr.ac_tab[k] >= 0 && prog_build_table(p + sr.ac_tab[k], false, &tabs[4 + k])) tb.ac[k] = &tabs[4 + k];
    }
    const long before = g_prog_host_symbols;
    prog_decode_scan(p, len, d, sr, tb, coef.data(), kNaturalOrder);
    out[i] = g_prog_host_symbols - before;
    levels[i] = sr.level;
  }
  return d.n_scans;
}

// ---- resize + augment ---------------------------------------------------------
// Full per-view augment: src RGB (HWC), params, -> out (3*S*S) of dtype out_dtype.
int emu_augment_view(const uint8_t* rgb, int W, int H, const dino_view_params* vp, const float* mean,
                     const float* stdv, int out_dtype, void* out) {
  return host_model_augment(rgb, W, H, *vp, mean, stdv, out_dtype, out);
}

// Stage checkpoint: resized+flipped uint8 crop (HWC) only.
int emu_resized_crop(const uint8_t* rgb, int W, int H, const dino_view_params* vp, uint8_t* out) {
  return host_model_resized_crop(rgb, W, H, *vp, out);
}

// Tile shape of k_hresize for a crop of cw x ch at view size S with kh taps (the kernel's
// own hresize_tile / hr_view_chunks): out = {sw, pitch, R, R3p, work items}.  R = 0: direct path.
void emu_hresize_tile(int S, int cw, int ch, int kh, int32_t* out) {
  const HrTile t = hresize_tile(S, cw, kh);
  out[0] = t.sw;
  out[1] = t.pitch;
  out[2] = t.R;
  out[3] = t.R3p;
  out[4] = hr_view_chunks(S, cw, ch, kh);
}

// Pillow's tap count for in_size -> out_size (0: the axis is not resampled).
int emu_resample_ksize(int in_size, int out_size) { return in_size == out_size ? 0 : resample_ksize(in_size, out_size); }

// The scratch layouts of the augment workspace (plan.hpp), as byte offsets:
// out = {htmp, hb, vb, ht, vt, hx, hg, total} of a view, relative to the view's base.
void emu_view_scratch(int S, int crop_h, int kh, int kv, int64_t* out) {
  const ViewScratch L = view_scratch(S, crop_h, kh, kv);
  const int64_t v[8] = {L.htmp, L.hb, L.vb, L.ht, L.vt, L.hx, L.hg, L.total};
  memcpy(out, v, sizeof v);
}

// out = byte offsets {vb, vt} of view_vcoefs' tables from the coefficient block's start.
void emu_view_vcoefs(int S, int kh, int kv, int64_t* out) {
  const std::vector<int32_t> block((size_t)S * (4 + kh + kv) + 1);  // a coefficient block's int32 tables
  const CoefView cv = view_vcoefs((const uint8_t*)block.data(), S, kh, kv);
  out[0] = (int64_t)(cv.bounds - block.data()) * 4;
  out[1] = (int64_t)(cv.taps - block.data()) * 4;
}

// out = {hb, ht, vb, vt, htmp, total} of a decode-only image of height H.
void emu_dec_scratch(int ow, int oh, int H, int kh, int kv, int64_t* out) {
  const DecScratch<int64_t> L = dec_scratch((int64_t)0, ow, oh, H, kh, kv);
  const int64_t v[6] = {L.hb, L.ht, L.vb, L.vt, L.htmp, L.total};
  memcpy(out, v, sizeof v);
}

// ---- masks ----------------------------------------------------------------------
int emu_masks(int H, int W, int target, int minp, int maxp, double la0, double la1, int n, uint32_t* py_state,
              uint32_t* np_state, uint8_t* out) {
  MaskParams mp{H, W, target, minp, maxp, la0, la1};
  MtState py, np;
  mt_load(py, py_state);
  mt_load(np, np_state);
  std::vector<uint8_t> scratch((size_t)H * W * 4 + 16);
  for (int i = 0; i < n; ++i) gen_mask(mp, py, np, out + (size_t)i * H * W, (int32_t*)scratch.data());
  mt_store(py, py_state);
  mt_store(np, np_state);
  return 0;
}

// ---- sampler ----------------------------------------------------------------------
int emu_sample_params(const dino_aug_config* cfg, uint64_t seed, uint64_t batch_index, int sample, int W,
                      int H, int ok, dino_view_params* out) {
  int nv = cfg->n_global + cfg->n_local;
  for (int v = 0; v < nv; ++v) sample_view(*cfg, seed, batch_index, sample, v, W, H, ok, &out[v]);
  return nv;
}

}  // extern "C"
