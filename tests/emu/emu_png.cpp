// Host model of the PNG decode — TEST INFRASTRUCTURE ONLY.
//
// Like emu.cpp and emu4.cpp, this compiles the __host__ __device__ code the kernels use
// (dataloader_amd/csrc/png_parse.hpp, inflate.hpp) for the CPU, with one lane: the IHDR parse
// (k_pnghead), the chunk walk and IDAT concatenation (k_pngwalk), the inflater (k_inflate) and
// the row filters and pixel rules (k_unfilter).  The product library never links this file.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../dataloader_amd/csrc/inflate.hpp"
#include "../../dataloader_amd/csrc/plan.hpp"
#include "../../dataloader_amd/csrc/png_parse.hpp"

using namespace dino;

namespace {
struct HostIO {
  int lane = 0, nl = 1;
  const uint8_t* z;
  int64_t zn;
  uint8_t* out;
  int64_t out_cap;
  uint8_t* win;
  InfTab *lt, *dt;
  uint8_t* lens;
  void sync() {}
  uint32_t in(int64_t i) const { return i >= 0 && i < zn ? z[i] : 0u; }
  void flush(int64_t at, int n) {
    for (int i = 0; i < n; ++i)
      if (at + i < out_cap) out[at + i] = win[(at + i) & (kInfWin - 1)];
  }
};
}  // namespace

extern "C" {

// Raw inflate of a zlib stream to `want` bytes (the model's inflater alone).  Returns the status.
int emu_png_inflate(const uint8_t* z, int64_t zn, uint8_t* out, int64_t want) {
  std::vector<uint8_t> win(kInfWin), lens(kInfMaxLens);
  InfTab lt, dt;
  HostIO io;
  io.z = z, io.zn = zn, io.out = out, io.out_cap = want, io.win = win.data(), io.lt = &lt, io.dt = &dt, io.lens = lens.data();
  Inflater<HostIO> inf(io, zn, want);
  return inf.run();
}

// The workspace layout of a kind-4 file (plan.hpp image_chunk_bytes, what k_plan places and
// dino_probe counts) and what the kernels use of it: out = {total, ent region (zcap of
// k_pngwalk / k_inflate), carry region, plane region (out_cap of k_inflate), palette region, rgb
// region, joined stream + its 64-byte pad, carry bytes k_unfilter writes, inflated bytes + the
// last flush's 16-byte round-up, rgb bytes}.  Returns the status of the head parse and walk.
int emu_png_layout(const uint8_t* p, int64_t len, int max_dim, int64_t* out) {
  ImgDesc d;
  d.kind = 0;
  d.width = d.height = 0;
  int st = parse_png_head(p, len, max_dim, &d);
  PngWalk w;
  if (st == DINO_IMG_OK) st = png_walk(p, len, d.color, &w);
  if (st != DINO_IMG_OK) return st;
  d.status = DINO_IMG_OK;
  const ChunkSizes z = image_chunk_bytes(d);
  out[0] = z.total(), out[1] = z.ent, out[2] = z.coef, out[3] = z.plane, out[4] = z.htab, out[5] = z.rgb;
  out[6] = w.idat_bytes + 64;
  out[7] = 4 * (int64_t)d.width;
  out[8] = align16(png_inflated_bytes(d));
  out[9] = (int64_t)d.width * d.height * 3;
  return st;
}

// The whole decode.  info = {status, width, height, kind (4, 5 or -1), zlib bytes, inflated bytes}.
// zs (>= len bytes) receives the concatenated stream, inf (>= H (1 + 4 W)) the filtered rows
// as inflated (copied before the filters are reversed), rgb (>= 3 W H) the pixels.
int emu_png_decode(const uint8_t* p, int64_t len, int max_dim, uint8_t* zs, uint8_t* inf, uint8_t* rgb, int64_t rgb_cap,
                   int64_t inf_cap, int32_t* info) {
  ImgDesc d;
  d.kind = 0;
  d.width = d.height = 0;
  info[0] = parse_png_head(p, len, max_dim, &d);
  info[1] = info[2] = info[4] = info[5] = 0;
  info[3] = d.status == DINO_IMG_OK ? kPngKind : (d.status == kPngDecline ? kPngKindDeclined : -1);
  if (d.status != DINO_IMG_OK) return d.status;
  PngWalk w;
  d.status = png_walk(p, len, d.color, &w);
  info[0] = d.status;
  info[3] = d.status == DINO_IMG_OK ? kPngKind : (d.status == kPngDecline ? kPngKindDeclined : -1);
  if (d.status != DINO_IMG_OK) return d.status;
  info[1] = d.width;
  info[2] = d.height;
  int64_t pos = w.idat_off, zn = 0;
  for (int c = 0; c < w.idat_chunks; ++c) {
    const uint32_t n = rd32be(p + pos);
    memcpy(zs + zn, p + pos + 8, n);
    zn += n;
    pos += 12 + (int64_t)n;
  }
  info[4] = (int32_t)zn;
  const int64_t want = png_inflated_bytes(d);
  info[5] = (int32_t)want;
  if (want > inf_cap || (int64_t)d.width * d.height * 3 > rgb_cap) return (info[0] = DINO_IMG_NO_SPACE);
  d.status = emu_png_inflate(zs, zn, inf, want);
  info[0] = d.status;
  if (d.status != DINO_IMG_OK) return d.status;
  uint8_t pal[768];
  memset(pal, 0, sizeof(pal));
  if (w.plte_off) memcpy(pal, p + w.plte_off, w.plte_n);
  std::vector<uint8_t> rows(inf, inf + want);
  if (!png_unfilter_rows(rows.data(), d.width, d.height, d.max_h, d.color, pal, rgb)) info[0] = DINO_IMG_CORRUPT;
  return info[0];
}

}  // extern "C"
