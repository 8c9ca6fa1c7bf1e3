// kernels_png.inc — part of kernels.hip's translation unit (not compiled on its own).  Needs nothing from earlier fragments.
// ---------------------------------------------------------------------------
// PNG (kind 4): k_pnghead -> k_pngwalk -> k_inflate -> k_unfilter
// ---------------------------------------------------------------------------
// Launched only by a context with dino_ctx_set_png on (no other context has a kind-4 image).
// The image's regions (plan.hpp image_chunk_bytes): ent = the IDAT payloads joined into one
// zlib stream, plane = the inflated, still-filtered rows, coef = one reconstructed row carried
// from a band of 64 rows to the next, htab = the palette, rgb = the pixels.

// One lane per image, between k_parse and k_plan: a file with the PNG signature, which k_parse
// left DINO_IMG_CORRUPT with a cleared descriptor, gets the descriptor of parse_png_head (the
// signature and IHDR; the chunk walk is k_pngwalk's).  A kernel of its own so that k_parse stays
// the code it was.
__global__ void __launch_bounds__(64) k_pnghead(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ offsets,
                                                const int64_t* __restrict__ lengths, const uint8_t* __restrict__ raw_mask,
                                                int B, int max_dim, ImgDesc* __restrict__ desc) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= B || (raw_mask != nullptr && raw_mask[i] != 0)) return;
  const int64_t off = offsets[i], len = lengths ? lengths[i] : offsets[i + 1] - off;
  if (!png_signature(bytes + off, len)) return;
  parse_png_head(bytes + off, len, max_dim, &desc[i]);
}

// One workgroup per image.  Lane 0 walks the chunks (png_walk: CRCs, PLTE / tRNS rules, the
// IDAT run and what follows it); then all lanes step through the run together and join the
// payloads, whole destination words where a chunk covers them and bytes at its edges (chunks of
// length 0 and 1 have only edges).  Fills the palette (zeros past PLTE) and ent_len, and zeroes
// the ticket counter of k_inflate.
constexpr int kPngWalkThreads = 256;
__global__ void __launch_bounds__(kPngWalkThreads) k_pngwalk(const uint8_t* __restrict__ bytes,
                                                             const int64_t* __restrict__ offsets,
                                                             const int64_t* __restrict__ lengths, ImgDesc* __restrict__ desc,
                                                             uint8_t* __restrict__ ws, PCtl* __restrict__ pctl) {
  __shared__ PngWalk s_w;
  __shared__ int s_status;
  const int img = blockIdx.x, tid = threadIdx.x;
  if (img == 0 && tid == 0) pctl->pad = 0;
  ImgDesc& d = desc[img];
  if (d.status != DINO_IMG_OK || d.kind != kPngKind) return;
  const int64_t off = offsets[img], len = lengths ? lengths[img] : offsets[img + 1] - off;
  const uint8_t* src = bytes + off;
  if (tid == 0) s_status = png_walk(src, len, d.color, &s_w);
  __syncthreads();
  if (s_status != DINO_IMG_OK) {
    if (tid == 0) d.status = s_status;
    return;
  }
  uint8_t* pal = ws + d.htab_off;
  for (int i = tid; i < kPngPalBytes; i += kPngWalkThreads) pal[i] = i < s_w.plte_n ? src[s_w.plte_off + i] : (uint8_t)0;
  uint8_t* ent = ws + d.ent_off;
  const int64_t cap = d.rst_off - d.ent_off;  // align16(scan_len + 64) >= the payloads + 64
  int64_t pos = s_w.idat_off, o = 0;
  if (s_w.idat_bytes + 64 > cap) {  // (cannot happen: the payloads lie inside the scan_len bytes)
    if (tid == 0) d.status = DINO_IMG_CORRUPT;
    return;
  }
  for (int c = 0; c < s_w.idat_chunks; ++c) {
    const int64_t n = rd32be(src + pos);
    const uint8_t* q = src + pos + 8;
    const int64_t head = min(n, (int64_t)((4 - (o & 3)) & 3)), nw = (n - head) >> 2;
    if (tid < head) ent[o + tid] = q[tid];
    uint32_t* dw = (uint32_t*)(ent + o + head);
    for (int64_t k = tid; k < nw; k += kPngWalkThreads) {
      const uint8_t* s = q + head + 4 * k;
      dw[k] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
    }
    const int64_t t0 = head + 4 * nw;
    if (t0 + tid < n) ent[o + t0 + tid] = q[t0 + tid];
    o += n;
    pos += 12 + n;
  }
  if (tid < 64) ent[o + tid] = 0;
  if (tid == 0) d.ent_len = (int32_t)o;
}

// One wave per image, persistent: a wave takes the next batch index as its ticket and inflates
// that image if it is a PNG (inflate.hpp, the code of the host model with nl = 64).  The wave's
// LDS holds the 32 KiB history ring, a 1 KiB input ring refilled by all lanes with 16-byte
// loads, both lookahead tables and the code lengths: kInfLdsBytes, four waves per CU.  The ring
// is flushed to the image's plane region 16 KiB at a time in aligned 16-byte stores; matches
// read the ring only, never the flushed bytes.
constexpr int kInfRing = 1024;
struct InfLds {
  __attribute__((aligned(16))) uint8_t win[kInfWin];
  __attribute__((aligned(16))) uint8_t ring[kInfRing];
  InfTab lt, dt;
  uint8_t lens[kInfMaxLens];
};
constexpr int kInfLdsBytes = (int)sizeof(InfLds);
static_assert(kInfLdsBytes <= 40 * 1024, "four inflate waves per CU");

struct InfDevIO {
  int lane, nl;
  const uint8_t* z;  // the stream's region (16-byte aligned), zcap bytes
  int64_t zcap, ring_base;
  uint8_t* ring;
  uint8_t* out;      // the inflated region (16-byte aligned), out_cap bytes
  int64_t out_cap;
  uint8_t* win;
  InfTab *lt, *dt;
  uint8_t* lens;
  __device__ __forceinline__ void sync() { __syncthreads(); }
  __device__ __forceinline__ uint32_t in(int64_t i) {
    if (i < ring_base || i >= ring_base + kInfRing) {  // uniform
      ring_base = i & ~(int64_t)15;
      __syncthreads();
      const int64_t at = ring_base + 16 * lane;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (at >= 0 && at + 16 <= zcap) v = *(const uint4*)(z + at);
      *(uint4*)(ring + 16 * lane) = v;
      __syncthreads();
    }
    return ring[i - ring_base];
  }
  __device__ __forceinline__ void flush(int64_t at, int n) {
    for (int j = 16 * lane; j < n; j += 16 * 64)
      if (at + j + 16 <= out_cap) *(uint4*)(out + at + j) = *(const uint4*)(win + ((at + j) & (kInfWin - 1)));
  }
};

__global__ void __launch_bounds__(64) k_inflate(ImgDesc* __restrict__ desc, uint8_t* __restrict__ ws, PCtl* __restrict__ pctl,
                                                int B) {
  __shared__ InfLds L;
  __shared__ uint32_t s_ticket;
  for (;;) {
    __syncthreads();
    if (threadIdx.x == 0) s_ticket = atomicAdd(&pctl->pad, 1u);
    __syncthreads();
    const uint32_t t = s_ticket;
    if (t >= (uint32_t)B) return;
    ImgDesc& d = desc[t];
    if (d.status != DINO_IMG_OK || d.kind != kPngKind) continue;
    InfDevIO io;
    io.lane = threadIdx.x, io.nl = 64;
    io.z = ws + d.ent_off, io.zcap = d.rst_off - d.ent_off, io.ring_base = -(int64_t)kInfRing * 2, io.ring = L.ring;
    io.out = ws + d.plane_off, io.out_cap = d.rgb_off - d.plane_off;
    io.win = L.win, io.lt = &L.lt, io.dt = &L.dt, io.lens = L.lens;
    const int64_t want = png_inflated_bytes(d);
    int st = DINO_IMG_CORRUPT;
    if (want + 16 <= io.out_cap) {
      Inflater<InfDevIO> inf(io, d.ent_len, want);
      st = inf.run();
    }
    if (st != DINO_IMG_OK && threadIdx.x == 0) d.status = st;
  }
}

// One wave per image reverses the row filters 64 rows at a time, lane r on row y0 + r one pixel
// behind lane r - 1: at step t it reconstructs pixel x = t - r from its own previous pixel
// (left), the pixel lane r - 1 reconstructed a step before (up) and the one before that
// (up-left), all in registers (four channels packed in a word).  Lane 63's row goes to the
// image's carry row for lane 0 of the next band.  Writes HWC RGB (png_to_rgb).  A filter byte
// above 4 fails the image, as in ZipDecode.c.
__global__ void __launch_bounds__(64) k_unfilter(ImgDesc* __restrict__ desc, uint8_t* __restrict__ ws) {
  ImgDesc& d = desc[blockIdx.x];
  if (d.status != DINO_IMG_OK || d.kind != kPngKind) return;
  const int W = d.width, H = d.height, bpp = d.max_h, color = d.color, lane = threadIdx.x;
  const int64_t stride = 1 + (int64_t)W * bpp;
  const uint8_t* inf = ws + d.plane_off;
  const uint8_t* pal = ws + d.htab_off;
  uint32_t* carry = (uint32_t*)(ws + d.coef_off);  // W words
  uint8_t* rgb = ws + d.rgb_off;
  int bad = 0;
  for (int y0 = 0; y0 < H; y0 += 64) {
    const int y = y0 + lane;
    const bool active = y < H;
    const uint8_t* row = inf + (active ? y : 0) * stride + 1;
    int f = active ? row[-1] : 0;
    if (f > 4) bad = 1, f = 0;
    uint32_t left = 0, upleft = 0, mine = 0;
    for (int t = 0; t < W + 63; ++t) {
      const int x = t - lane;
      const bool in = active && x >= 0 && x < W;
      uint32_t up = __shfl_up(mine, 1);
      if (lane == 0) up = (y0 > 0 && in) ? carry[x] : 0u;
      mine = 0;
      if (in) {
        uint8_t px[4] = {0, 0, 0, 0};
        for (int c = 0; c < bpp; ++c) {
          const int sh = 8 * c;
          const int v = row[(int64_t)x * bpp + c] + png_predict(f, (left >> sh) & 255, (up >> sh) & 255, (upleft >> sh) & 255);
          px[c] = (uint8_t)v;
          mine |= (uint32_t)px[c] << sh;
        }
        png_to_rgb(color, px, pal, rgb + ((int64_t)y * W + x) * 3);
        if (lane == 63) carry[x] = mine;
      }
      left = mine;
      upleft = up;
    }
    __threadfence_block();
    __syncthreads();
  }
  if (__syncthreads_or(bad) && lane == 0) d.status = DINO_IMG_CORRUPT;
}
