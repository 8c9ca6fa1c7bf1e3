// kernels_gif.inc — part of kernels.hip's translation unit (not compiled on its own).  Needs nothing from earlier fragments.
// ---------------------------------------------------------------------------
// GIF (kind 8): k_gifhead -> k_gifwalk -> k_giflzw -> k_gif_rgb
// ---------------------------------------------------------------------------
// Launched only by a context with dino_ctx_set_gif on (no other context has a kind-8 image).
// The image's regions (plan.hpp image_chunk_bytes): ent = the sub-blocks' payloads joined into
// one LZW stream, plane = the w x h colour indices in coded row order, htab = the colour table
// (256 x RGB, zeros past the file's entries), rgb = the pixels.

// One lane per image, between k_parse and k_plan: a file with the GIF signature, which k_parse
// left DINO_IMG_CORRUPT with a cleared descriptor, gets the descriptor of parse_gif_head (the
// header walk up to the first image's LZW stream).  A kernel of its own so that k_parse stays the
// code it was.
__global__ void __launch_bounds__(64) k_gifhead(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ offsets,
                                                const int64_t* __restrict__ lengths, const uint8_t* __restrict__ raw_mask,
                                                int B, int max_dim, ImgDesc* __restrict__ desc) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= B || (raw_mask != nullptr && raw_mask[i] != 0)) return;
  const int64_t off = offsets[i], len = lengths ? lengths[i] : offsets[i + 1] - off;
  if (!gif_signature(bytes + off, len)) return;
  parse_gif_head(bytes + off, len, max_dim, &desc[i]);
}

// One workgroup per image.  All lanes step through the sub-block chain together (a length byte
// per hop: a serial chain of at most len / 256 hops, each a uniform load) and join the payloads
// into `ent`: whole destination words where a block covers them, bytes at its edges.  Fills the
// colour table (zeros past the file's entries: Pillow pads its palette the same way), ent_len and
// the 64 zero bytes after the stream.
constexpr int kGifWalkThreads = 256;
__global__ void __launch_bounds__(kGifWalkThreads) k_gifwalk(const uint8_t* __restrict__ bytes,
                                                             const int64_t* __restrict__ offsets,
                                                             const int64_t* __restrict__ lengths, ImgDesc* __restrict__ desc,
                                                             uint8_t* __restrict__ ws) {
  const int img = blockIdx.x, tid = threadIdx.x;
  ImgDesc& d = desc[img];
  if (d.status != DINO_IMG_OK || d.kind != kGifKind) return;
  const int64_t off = offsets[img], len = lengths ? lengths[img] : offsets[img + 1] - off;
  const uint8_t* src = bytes + off;
  uint8_t* pal = ws + d.htab_off;
  const int pal_bytes = 3 * d.n_scans;
  for (int i = tid; i < kGifPalBytes; i += kGifWalkThreads) pal[i] = i < pal_bytes ? src[d.first_sos + i] : (uint8_t)0;
  uint8_t* ent = ws + d.ent_off;
  // (the region holds align16(scan_len + 64) bytes and the payloads lie inside the scan_len bytes)
  int64_t pos = d.scan_off, o = 0, at = 0;
  for (int n; (n = gif_next_block(src, len, pos, &at)) > 0; pos = at + n) {
    const uint8_t* q = src + at;
    const int head = min(n, (int)((4 - (o & 3)) & 3)), nw = (n - head) >> 2;
    if (tid < head) ent[o + tid] = q[tid];
    if (tid < nw) {
      const uint8_t* s = q + head + 4 * tid;
      ((uint32_t*)(ent + o + head))[tid] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
    }
    const int t0 = head + 4 * nw;
    if (t0 + tid < n) ent[o + t0 + tid] = q[t0 + tid];
    o += n;
  }
  if (tid < 64) ent[o + tid] = 0;
  if (tid == 0) d.ent_len = (int32_t)o;
}

// One wave per image runs gif_lzw.hpp with a code per lane.  The table lives in LDS as the
// output position and length of each entry's string (24 KiB: six waves per CU of 160 KiB); the
// strings themselves are the index plane, which the wave reads back where a source lies before
// the 64-byte chunk being written.  Those loads follow stores of other lanes of the same wave:
// io.sync is __syncthreads, HIP's workgroup-scope release fence, barrier and acquire fence, which
// orders them (DESIGN.md).  Plain vector stores only.
struct GifLds {
  uint32_t dpos[kGifTable];
  uint16_t dlen[kGifTable];
};
constexpr int kGifLdsBytes = (int)sizeof(GifLds);
static_assert(kGifLdsBytes <= 26 * 1024, "six LZW waves per CU");

struct GifDevIO {
  static constexpr int kSlots = 1;
  int me;
  uint32_t* dpos;
  uint16_t* dlen;
  __device__ __forceinline__ int lane(int) const { return me; }
  __device__ __forceinline__ void shfl(int* dst, const int* src, const int* idx) const { dst[0] = __shfl(src[0], idx[0], 64); }
  __device__ __forceinline__ uint64_t ballot(const bool* p) const { return __ballot(p[0]); }
  __device__ __forceinline__ int bcast(const int* v, int l) const { return __builtin_amdgcn_readlane(v[0], l); }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
};

__global__ void __launch_bounds__(64) k_giflzw(ImgDesc* __restrict__ desc, uint8_t* __restrict__ ws) {
  __shared__ GifLds s;
  ImgDesc& d = desc[blockIdx.x];
  if (d.status != DINO_IMG_OK || d.kind != kGifKind) return;
  GifDevIO io{(int)threadIdx.x, s.dpos, s.dlen};
  const int st = gif_lzw_decode(io, (const uint32_t*)(ws + d.ent_off), d.ent_len, d.color, ws + d.plane_off,
                                (int64_t)d.width * d.height);
  __syncthreads();
  if (threadIdx.x == 0 && st != DINO_IMG_OK) d.status = st;
}

// Grid (row tiles, B), 256 lanes, the colour table in LDS.  A tile is kGifRgbRows output rows;
// each reads its coded row (gif_coded_row: the closed form of the four interlace passes) and
// writes HWC RGB.  The tile's bytes are one contiguous run of the RGB region: a lane makes one
// aligned word of it from the four bytes' pixels, edge bytes of the run go out singly.
constexpr int kGifRgbRows = 8;
constexpr int kGifRgbWgs = 16;  // row tiles in flight per image (a 640 x 480 image has 60 tiles)
__global__ void __launch_bounds__(256) k_gif_rgb(const ImgDesc* __restrict__ desc, uint8_t* __restrict__ ws) {
  __shared__ uint32_t s_pal[256];
  const ImgDesc& d = desc[blockIdx.y];
  if (d.status != DINO_IMG_OK || d.kind != kGifKind) return;
  const int W = d.width, H = d.height, lace = d.mcus_y;
  const uint8_t* pal = ws + d.htab_off;
  const int t = threadIdx.x;
  s_pal[t] = (uint32_t)pal[3 * t] | ((uint32_t)pal[3 * t + 1] << 8) | ((uint32_t)pal[3 * t + 2] << 16);
  __syncthreads();
  const uint8_t* plane = ws + d.plane_off;
  uint8_t* rgb = ws + d.rgb_off;  // 16-byte aligned
  for (int y0 = blockIdx.x * kGifRgbRows; y0 < H; y0 += gridDim.x * kGifRgbRows) {
    const int rows = min(kGifRgbRows, H - y0);
    const int64_t b0 = (int64_t)y0 * W * 3, b1 = b0 + (int64_t)rows * W * 3;  // the tile's bytes [b0, b1)
    for (int64_t wd = (b0 >> 2) + t; wd * 4 < b1; wd += 256) {
      uint32_t v = 0;
      for (int k = 0; k < 4; ++k) {
        const int64_t b = wd * 4 + k;
        if (b < b0 || b >= b1) continue;
        const uint32_t px = (uint32_t)b / 3u, c = (uint32_t)b - 3u * px;  // (b < 3 w h < 2^31)
        const int y = (int)(px / (uint32_t)W), x = (int)(px - (uint32_t)y * (uint32_t)W);
        const uint32_t e = s_pal[plane[(int64_t)gif_coded_row(y, H, lace) * W + x]];
        v |= ((e >> (8 * c)) & 0xFFu) << (8 * k);
      }
      if (wd * 4 >= b0 && wd * 4 + 4 <= b1) {
        *(uint32_t*)(rgb + wd * 4) = v;
      } else {
        for (int k = 0; k < 4; ++k)
          if (wd * 4 + k >= b0 && wd * 4 + k < b1) rgb[wd * 4 + k] = (uint8_t)(v >> (8 * k));
      }
    }
  }
}
