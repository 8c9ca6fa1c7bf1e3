// kernels_vp8.inc — part of kernels.hip's translation unit (not compiled on its own).  Needs nothing from earlier fragments.
// ---------------------------------------------------------------------------
// Lossy WebP (kind 7): k_vp8head -> k_vp8_tok -> k_vp8_rec -> k_vp8_rgb
// ---------------------------------------------------------------------------
// Launched only by a context with dino_ctx_set_webp and dino_ctx_set_webp_forms on (no other
// context has a kind-7 image).  The image's regions (plan.hpp image_chunk_bytes): coef = the
// Vp8Frame record and 384 dequantised int16 coefficients a macroblock (the Y2 transform already
// folded into the luma DCs), binfo = a Vp8Mb record a macroblock, plane = Y at pitch 16 mbw, then
// U and V at pitch 8 mbw, unfiltered and then filtered in place, rgb = the pixels.  The VP8
// payload is read where the file lies.

// One lane per image, between k_webphead and k_plan: a file with the RIFF / WEBP signature that
// parse_webp_head declined gets the descriptor of parse_vp8_head (the container walk and the
// frame's ten bytes), or stays declined.  A kernel of its own so that k_webphead stays the code it was.
__global__ void __launch_bounds__(64) k_vp8head(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ offsets,
                                                const int64_t* __restrict__ lengths, const uint8_t* __restrict__ raw_mask,
                                                int B, int max_dim, ImgDesc* __restrict__ desc) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= B || (raw_mask != nullptr && raw_mask[i] != 0) || desc[i].status != kWebpDecline) return;
  const int64_t off = offsets[i], len = lengths ? lengths[i] : offsets[i + 1] - off;
  if (!webp_signature(bytes + off, len)) return;
  parse_vp8_head(bytes + off, len, max_dim, &desc[i]);
}

// One wave per image runs vp8.hpp's Vp8Tok with nl = 64: the serial part.  Both bool decoders
// (first partition, token partition) keep value, range and bit count in wave-uniform registers
// and read the payload through a 1 KiB LDS window each, refilled by all lanes (16-byte loads
// where the file's bytes are aligned).  LDS also holds the coefficient probabilities, the frame
// record, the modes and non-zero flags above for a whole macroblock row (1024 columns: every width
// the format has), the record being built and the 400-halfword coefficient buffer, which the
// lanes copy to the workspace as words and clear after every macroblock: 10.3 KiB.
constexpr int kVp8Ring = 1024;
constexpr int kVp8MaxMbw = 1024;  // 16383 pixels
struct Vp8TokLds {
  __attribute__((aligned(16))) uint8_t ring[2][kVp8Ring];
  __attribute__((aligned(16))) int16_t cbuf[400];
  Vp8Frame F;
  Vp8Mb M;
  uint32_t tmode[kVp8MaxMbw];
  uint16_t tnz[kVp8MaxMbw];
  uint8_t proba[1056];
};

struct Vp8DevIO {
  int lane, nl;
  const uint8_t* z;  // the payload, zlen bytes
  int64_t zlen, ring_base[2];
  uint8_t* ring;
  __device__ __forceinline__ void sync() {
    __threadfence_block();
    __syncthreads();
  }
  __device__ __forceinline__ uint32_t in(int r, int64_t i) {
    if (i < ring_base[r] || i >= ring_base[r] + kVp8Ring) {  // uniform
      ring_base[r] = i - (int64_t)((uintptr_t)(z + i) & 15);  // (16-byte aligned in memory; up to 15 bytes before i)
      __syncthreads();
      const int64_t at = ring_base[r] + 16 * lane;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (at >= 0 && at + 16 <= zlen) {
        v = *(const uint4*)(z + at);
      } else {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if (at + k >= 0 && at + k < zlen) w[k >> 2] |= (uint32_t)z[at + k] << (8 * (k & 3));
        v = make_uint4(w[0], w[1], w[2], w[3]);
      }
      *(uint4*)(ring + r * kVp8Ring + 16 * lane) = v;
      __syncthreads();
    }
    return ring[r * kVp8Ring + (i - ring_base[r])];
  }
};

__global__ void __launch_bounds__(64) k_vp8_tok(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ offsets,
                                                ImgDesc* __restrict__ desc, uint8_t* __restrict__ ws) {
  __shared__ Vp8TokLds L;
  ImgDesc& d = desc[blockIdx.x];
  if (d.status != DINO_IMG_OK || d.kind != kVp8Kind) return;
  Vp8DevIO io;
  io.lane = threadIdx.x, io.nl = 64;
  io.z = bytes + offsets[blockIdx.x] + d.scan_off, io.zlen = d.scan_len;
  io.ring_base[0] = io.ring_base[1] = -(int64_t)kVp8Ring * 2;
  io.ring = &L.ring[0][0];
  Vp8Tok<Vp8DevIO> tok(io, L.F, L.proba, L.tmode, L.tnz, L.cbuf, L.M);
  int st = tok.header(d.scan_len, kVp8MaxMbw);
  // (the plan sized the regions from the same ten bytes; a chunk that does not hold them is not written)
  if (st == DINO_IMG_OK && (tok.W != d.width || tok.H != d.height || d.binfo_off - d.coef_off < vp8_coef_bytes(d.width, d.height) ||
                            d.plane_off - d.binfo_off < vp8_binfo_bytes(d.width, d.height)))
    st = DINO_IMG_CORRUPT;
  if (st == DINO_IMG_OK && !tok.body((int16_t*)(ws + d.coef_off + sizeof(Vp8Frame)), (Vp8Mb*)(ws + d.binfo_off))) st = DINO_IMG_CORRUPT;
  io.sync();
  if (st != DINO_IMG_OK) {
    if (threadIdx.x == 0) d.status = st;
    return;
  }
  if (threadIdx.x < (int)(sizeof(Vp8Frame) / 4)) ((int32_t*)(ws + d.coef_off))[threadIdx.x] = ((const int32_t*)&L.F)[threadIdx.x];
}

// One workgroup of four waves per image: unfiltered reconstruction of every macroblock, a
// workgroup barrier, then the loop filter in place (one launch: the filter reads what the
// reconstruction's last step wrote, and nothing else runs between them).  Both passes walk the
// same schedule: macroblock (x, y) needs (x - 1, y), (x, y - 1) and (x + 1, y - 1), so step t
// takes the macroblocks with x + 2 y = t, a macroblock a wave, and a fenced __syncthreads()
// separates steps: no flags, no spinning.  Inside a macroblock the wave's lanes run vp8_rec_mb /
// vp8_filter_mb (vp8.hpp) with nl = 64 over the wave's own LDS tiles (luma 17 rows of 32 with the
// borders, two chroma tiles of 9 rows of 16) and its 384 residuals; io.sync() is a
// workgroup-scope fence and a wave barrier (the lanes of one wave only).
constexpr int kVp8RecThreads = 256;
struct Vp8RecLds {
  Vp8Frame F;
  __attribute__((aligned(16))) uint8_t T[kVp8RecThreads / 64][(kVp8TileBytes + 15) / 16 * 16];
  __attribute__((aligned(16))) int16_t R[kVp8RecThreads / 64][384];
};
struct Vp8WaveIO {
  int lane, nl;
  __device__ __forceinline__ void sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
};

__global__ void __launch_bounds__(kVp8RecThreads) k_vp8_rec(const ImgDesc* __restrict__ desc, uint8_t* __restrict__ ws) {
  __shared__ Vp8RecLds L;
  const ImgDesc& d = desc[blockIdx.x];
  if (d.status != DINO_IMG_OK || d.kind != kVp8Kind) return;
  const int tid = threadIdx.x, wave = tid >> 6, mbw = vp8_mbs(d.width), mbh = vp8_mbs(d.height);
  const int64_t nmb = (int64_t)mbw * mbh;
  if (d.rgb_off - d.plane_off < 384 * nmb) return;  // (never: the plan's own size)
  if (tid < (int)(sizeof(Vp8Frame) / 4)) ((int32_t*)&L.F)[tid] = ((const int32_t*)(ws + d.coef_off))[tid];
  __syncthreads();
  const int16_t* coef = (const int16_t*)(ws + d.coef_off + sizeof(Vp8Frame));
  const Vp8Mb* mbs = (const Vp8Mb*)(ws + d.binfo_off);
  uint8_t* Y = ws + d.plane_off;
  uint8_t* U = Y + 256 * nmb;
  uint8_t* V = U + 64 * nmb;
  Vp8WaveIO io;
  io.lane = tid & 63, io.nl = 64;
  const int steps = (mbw - 1) + 2 * (mbh - 1) + 1;
  for (int pass = 0; pass < (L.F.filter_type ? 2 : 1); ++pass)
    for (int t = 0; t < steps; ++t) {
      const int y_lo = t > mbw - 1 ? (t - (mbw - 1) + 1) >> 1 : 0, y_hi = min(mbh - 1, t >> 1);
      for (int y = y_lo + wave; y <= y_hi; y += kVp8RecThreads / 64) {
        const int x = t - 2 * y;
        const int64_t mb = (int64_t)y * mbw + x;
        if (pass == 0) vp8_rec_mb(io, x, y, mbw, coef + 384 * mb, mbs[mb], Y, U, V, L.T[wave], L.R[wave]);
        else vp8_filter_mb(io, x, y, mbw, L.F, mbs[mb], Y, U, V);
      }
      __threadfence_block();
      __syncthreads();
    }
}

// Planes -> HWC RGB with the crop to W x H: a thread makes four consecutive pixels (the fancy
// upsampler and the fixed-point colour conversion of vp8_rgb_px) and stores them as three
// aligned words (the RGB region is padded past its last pixel).  A 2D grid: row of workgroups x images.
constexpr int kVp8RgbWgs = 16;
__global__ void __launch_bounds__(256) k_vp8_rgb(const ImgDesc* __restrict__ desc, uint8_t* __restrict__ ws) {
  const ImgDesc& d = desc[blockIdx.y];
  if (d.status != DINO_IMG_OK || d.kind != kVp8Kind) return;
  const int W = d.width, H = d.height, mbw = vp8_mbs(W);
  const int64_t nmb = vp8_nmb(W, H), n = (int64_t)W * H;
  const uint8_t* Y = ws + d.plane_off;
  const uint8_t* U = Y + 256 * nmb;
  const uint8_t* V = U + 64 * nmb;
  uint32_t* rgbw = (uint32_t*)(ws + d.rgb_off);
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; 4 * q < n; q += (int64_t)gridDim.x * 256) {
    uint32_t p[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t i = 4 * q + k;
      const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
      p[k] = i < n ? vp8_rgb_px(Y, U, V, mbw, x, y, W, H) : 0u;
    }
    rgbw[3 * q] = p[0] | (p[1] << 24);
    rgbw[3 * q + 1] = (p[1] >> 8) | (p[2] << 16);
    rgbw[3 * q + 2] = (p[2] >> 16) | (p[3] << 8);
  }
}
