// kernels_webp.inc — part of kernels.hip's translation unit (not compiled on its own).  Needs nothing from earlier fragments.
// ---------------------------------------------------------------------------
// Lossless WebP (kind 6): k_webphead -> k_vp8l -> k_vp8l_inv
// ---------------------------------------------------------------------------
// Launched only by a context with dino_ctx_set_webp on (no other context has a kind-6 image).
// The image's regions (plan.hpp image_chunk_bytes): coef = a Vp8lPlan and the sub-images
// (predictor, cross-colour and entropy images, the palette), binfo = the groups' codes
// (Vp8lGroup records), plane = the entropy-decoded ARGB words, rgb = the pixels.  The VP8L
// payload is read where the file lies.

// One lane per image, between k_parse and k_plan: a file with the RIFF / WEBP signature, which
// k_parse left DINO_IMG_CORRUPT with a cleared descriptor, gets the descriptor of
// parse_webp_head (the container walk and the VP8L header).  A kernel of its own so that k_parse
// stays the code it was.
__global__ void __launch_bounds__(64) k_webphead(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ offsets,
                                                 const int64_t* __restrict__ lengths, const uint8_t* __restrict__ raw_mask,
                                                 int B, int max_dim, ImgDesc* __restrict__ desc) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= B || (raw_mask != nullptr && raw_mask[i] != 0)) return;
  const int64_t off = offsets[i], len = lengths ? lengths[i] : offsets[i + 1] - off;
  if (!webp_signature(bytes + off, len)) return;
  parse_webp_head(bytes + off, len, max_dim, &desc[i]);
}

// One wave per image runs vp8l.hpp with nl = 64: the transforms' sub-images, the entropy image,
// the groups' codes and the pixels, all through one bit buffer in registers.  The wave's LDS
// holds a 1 KiB input ring refilled by all lanes (16-byte loads where the file's bytes are
// aligned), the staged group (counts and symbols of its five codes: the pixel loop reads no code
// from global memory; a group is staged again only when the entropy image names another), the
// colour cache with its stamps, the code lengths being read and the Vp8lPlan: kVp8lLdsBytes,
// five waves per CU.  Pixels go straight to the ARGB plane: lane 0 stores a literal or a cache
// hit, all lanes copy a back-reference from the plane (words the wave stored earlier: io.sync is
// a workgroup-scope fence and a barrier).  The colour cache is filled lazily, wave-parallel
// (Vp8l::cache_catch_up: atomic max of the pixel index per slot, the winner stores the colour).
constexpr int kVp8lRing = 1024;
struct Vp8lLds {
  __attribute__((aligned(16))) uint8_t ring[kVp8lRing];
  __attribute__((aligned(16))) Vp8lGroup stage;
  uint32_t cache[kVp8lCacheMax], stamp[kVp8lCacheMax];
  Vp8lPlan plan;
  uint8_t lens[kVp8lLens];
};
constexpr int kVp8lLdsBytes = (int)sizeof(Vp8lLds);
static_assert(kVp8lLdsBytes <= 32 * 1024, "five VP8L waves per CU");

struct Vp8lDevIO {
  int lane, nl;
  const uint8_t* z;  // the payload, zlen bytes
  int64_t zlen, ring_base;
  uint8_t* ring;
  uint32_t *cache, *stamp;
  uint8_t* lens;
  Vp8lGroup* stage;
  __device__ __forceinline__ void sync() {
    __threadfence_block();
    __syncthreads();
  }
  __device__ __forceinline__ uint32_t in(int64_t i) {
    if (i < ring_base || i >= ring_base + kVp8lRing) {  // uniform
      ring_base = i - (int64_t)((uintptr_t)(z + i) & 15);  // (16-byte aligned in memory; up to 15 bytes before i)
      __syncthreads();
      const int64_t at = ring_base + 16 * lane;
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
      *(uint4*)(ring + 16 * lane) = v;
      __syncthreads();
    }
    return ring[i - ring_base];
  }
  __device__ __forceinline__ uint64_t ballot(bool b) { return __ballot(b); }
  __device__ __forceinline__ int below(uint64_t m) { return __popcll(m & ((1ull << lane) - 1ull)); }
  __device__ __forceinline__ void amax(uint32_t* p, uint32_t v) { atomicMax(p, v); }
};

__global__ void __launch_bounds__(64) k_vp8l(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ offsets,
                                             ImgDesc* __restrict__ desc, uint8_t* __restrict__ ws) {
  __shared__ Vp8lLds L;
  ImgDesc& d = desc[blockIdx.x];
  if (d.status != DINO_IMG_OK || d.kind != kWebpKind) return;
  Vp8lDevIO io;
  io.lane = threadIdx.x, io.nl = 64;
  io.z = bytes + offsets[blockIdx.x] + d.scan_off, io.zlen = d.scan_len, io.ring_base = -(int64_t)kVp8lRing * 2;
  io.ring = L.ring, io.cache = L.cache, io.stamp = L.stamp, io.lens = L.lens, io.stage = &L.stage;
  uint32_t* sub = (uint32_t*)(ws + d.coef_off + sizeof(Vp8lPlan));
  const int64_t sub_cap = (d.binfo_off - d.coef_off - (int64_t)sizeof(Vp8lPlan)) / 4;
  const int gcap = (int)((d.plane_off - d.binfo_off) / (int64_t)sizeof(Vp8lGroup));
  const int64_t out_cap = (d.rgb_off - d.plane_off) / 4;
  Vp8l<Vp8lDevIO> dec(io, d.scan_len, (Vp8lGroup*)(ws + d.binfo_off), gcap, sub, sub_cap, L.plan);
  const bool ok = dec.prologue() && dec.W == d.width && dec.H == d.height && (int64_t)d.width * d.height <= out_cap &&
                  dec.body((uint32_t*)(ws + d.plane_off));
  io.sync();
  if (!ok) {
    if (threadIdx.x == 0) d.status = DINO_IMG_CORRUPT;
    return;
  }
  if (threadIdx.x < (int)(sizeof(Vp8lPlan) / 4)) ((int32_t*)(ws + d.coef_off))[threadIdx.x] = ((const int32_t*)&L.plan)[threadIdx.x];
}

// Four ARGB pixels -> the 12 bytes of four RGB pixels (alpha dropped, as Pillow's RGBA -> RGB).
__device__ __forceinline__ void vp8l_store_rgb4(uint32_t* rgbw, int64_t q, const uint32_t p[4]) {
  const uint32_t r0 = (p[0] >> 16) & 255, g0 = (p[0] >> 8) & 255, b0 = p[0] & 255, r1 = (p[1] >> 16) & 255;
  const uint32_t g1 = (p[1] >> 8) & 255, b1 = p[1] & 255, r2 = (p[2] >> 16) & 255, g2 = (p[2] >> 8) & 255;
  const uint32_t b2 = p[2] & 255, r3 = (p[3] >> 16) & 255, g3 = (p[3] >> 8) & 255, b3 = p[3] & 255;
  rgbw[3 * q] = r0 | (g0 << 8) | (b0 << 16) | (r1 << 24);
  rgbw[3 * q + 1] = g1 | (b1 << 8) | (r2 << 16) | (g2 << 24);
  rgbw[3 * q + 2] = b2 | (r3 << 8) | (g3 << 16) | (b3 << 24);
}

// A per-pixel stage over n pixels, four consecutive pixels a lane: f(i) is pixel i's new value.
// It goes back to the plane as one 16-byte store, or, for the last stage, to the RGB region as
// three aligned words (both regions are padded past their last pixel).
constexpr int kVp8lInvThreads = 256;
template <class F>
__device__ __forceinline__ void vp8l_map(int64_t n, uint32_t* img, uint32_t* rgbw, bool last, F f) {
  for (int64_t q = threadIdx.x; 4 * q < n; q += kVp8lInvThreads) {
    uint32_t p[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = 4 * q + k < n ? f(4 * q + k) : 0u;
    if (last) vp8l_store_rgb4(rgbw, q, p);
    else *(uint4*)(img + 4 * q) = make_uint4(p[0], p[1], p[2], p[3]);
  }
}

// One workgroup per image undoes the transforms, last to first, in place in the ARGB plane; the
// last stage writes HWC RGB instead (an image without transforms gets a copy stage).
//   add-green, cross-colour: vp8l_map over the pixels;
//   colour indexing: as the last stage (where libwebp's encoder puts it) vp8l_map reads the
//     bundled rows and writes RGB; elsewhere the rows are expanded in place, last row and last
//     chunk first (a chunk's destination lies at or past every source still to be read);
//   predictor: wave 0 runs 64 rows as a skewed wavefront, lane r on row y0 + r two pixels behind
//     lane r - 1 (the top-right neighbour must be final).  At step t it reconstructs pixel
//     x = t - 2 r: left is its own previous pixel, top-right comes from lane r - 1 by one
//     __shfl_up, top and top-left are the top-right of the two steps before, all in registers;
//     the rightmost pixel takes the row's own first pixel as top-right, as the format says.
//     Lane 0 reads the row above from the plane, where the band before left it final.
__global__ void __launch_bounds__(kVp8lInvThreads) k_vp8l_inv(ImgDesc* __restrict__ desc, uint8_t* __restrict__ ws) {
  const ImgDesc& d = desc[blockIdx.x];
  if (d.status != DINO_IMG_OK || d.kind != kWebpKind) return;
  __shared__ Vp8lPlan P;
  const int tid = threadIdx.x, W = d.width, H = d.height;
  if (tid < (int)(sizeof(Vp8lPlan) / 4)) ((int32_t*)&P)[tid] = ((const int32_t*)(ws + d.coef_off))[tid];
  __syncthreads();
  const uint32_t* sub = (const uint32_t*)(ws + d.coef_off + sizeof(Vp8lPlan));
  uint32_t* img = (uint32_t*)(ws + d.plane_off);
  uint32_t* rgbw = (uint32_t*)(ws + d.rgb_off);
  uint8_t* rgb = ws + d.rgb_off;
  if (P.ntr == 0) vp8l_map((int64_t)W * H, img, rgbw, true, [&](int64_t i) { return img[i]; });
  for (int k = P.ntr - 1; k >= 0; --k) {
    const int type = P.type[k], xs = P.xs_in[k], b = P.bits[k], bw = (xs + (1 << b) - 1) >> b;
    const bool last = k == 0;
    const uint32_t* s = sub + P.sub_off[k];
    const int64_t n = (int64_t)xs * H;
    if (type == 2) {
      vp8l_map(n, img, rgbw, last, [&](int64_t i) { return vp8l_add_green(img[i]); });
    } else if (type == 1) {
      vp8l_map(n, img, rgbw, last, [&](int64_t i) {
        const int y = (int)(i / xs), x = (int)(i - (int64_t)y * xs);
        return vp8l_cross(img[i], s[(int64_t)(y >> b) * bw + (x >> b)]);
      });
    } else if (type == 3 && last) {
      vp8l_map(n, img, rgbw, true, [&](int64_t i) {
        const int y = (int)(i / xs), x = (int)(i - (int64_t)y * xs);
        return vp8l_index(img + (int64_t)y * bw, s, x, b);
      });
    } else if (type == 3) {
      for (int y = H - 1; y >= 0; --y)
        for (int c0 = (xs - 1) / kVp8lInvThreads * kVp8lInvThreads; c0 >= 0; c0 -= kVp8lInvThreads) {
          const int x = c0 + tid;
          const uint32_t v = x < xs ? vp8l_index(img + (int64_t)y * bw, s, x, b) : 0u;
          __syncthreads();
          if (x < xs) img[(int64_t)y * xs + x] = v;
          __threadfence_block();
          __syncthreads();
        }
    } else {
      for (int y0 = 0; y0 < H; y0 += 64) {
        if (tid < 64) {
          const int y = y0 + tid;
          const bool active = y < H;
          uint32_t* row = img + (int64_t)(active ? y : 0) * xs;
          uint32_t left = 0, first = 0, T = 0, TL = 0, mine = 0;
          if (tid == 0 && y0 > 0) T = row[-xs];  // (lane 0 has no step at x = -1 to take its first top from)
          for (int t = 0; t < xs + 126; ++t) {
            const int x = t - 2 * tid;
            const bool in = active && x >= 0 && x < xs;
            uint32_t tr = __shfl_up(mine, 1);
            if (tid == 0) tr = (y0 > 0 && x + 1 >= 0 && x + 1 < xs) ? row[x + 1 - xs] : 0u;
            if (x == xs - 1) tr = first;
            if (in) {
              const int mode = vp8l_pred_mode(x, y, s[(int64_t)(y >> b) * bw + (x >> b)]);
              mine = vp8l_add(row[x], vp8l_predict(mode, left, T, TL, tr));
              row[x] = mine;
              if (last) {
                uint8_t* o = rgb + ((int64_t)y * xs + x) * 3;
                o[0] = (uint8_t)(mine >> 16), o[1] = (uint8_t)(mine >> 8), o[2] = (uint8_t)mine;
              }
              if (x == 0) first = mine;
              left = mine;
            }
            TL = T;
            T = tr;
          }
        }
        __threadfence_block();
        __syncthreads();
      }
    }
    __threadfence_block();
    __syncthreads();
  }
}
