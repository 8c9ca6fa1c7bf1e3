// kernels_orient.inc — part of kernels.hip's translation unit (not compiled on its own).  Needs
// exif_parse.hpp and plan.hpp (rgb_region_bytes).
// ---------------------------------------------------------------------------
// EXIF orientation (ImageOps.exif_transpose): k_exif -> k_orient_scan -> .. -> k_orient -> k_orient_done
// ---------------------------------------------------------------------------
// Launched only by a context with dino_ctx_set_exif_transpose on.  k_exif reads each JPEG's
// Orientation tag before the plan and k_orient_scan numbers the tiles, so that k_plan reserves a
// second RGB region for the images that turn; the decode runs as ever, on the coded width and height; k_orient then writes each
// such image upright into its second region, tile by tile, and k_orient_done points the
// descriptor at it and swaps width and height for orientations 5..8.  Everything after the decode
// (k_info, k_copy_rgb*, k_params, the resize and augment kernels) sees the upright image only.

// One lane per image, between k_parse / k_pnghead / k_draft and k_plan (k_parse stays the code it
// was): the image's orientation goes to pad0[0]: 2..8, or 0 for an image that stays as it is (no
// tag, value 1, an unverified file, which the caller hands to Pillow, a raw container, which is
// upright already, anything that is not a decodable JPEG).
__global__ void __launch_bounds__(64) k_exif(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ offsets,
                                             const int64_t* __restrict__ lengths, const uint8_t* __restrict__ raw_mask,
                                             int B, ImgDesc* __restrict__ desc) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= B) return;
  ImgDesc& d = desc[i];
  int o = kOrientNone;
  if (d.status == DINO_IMG_OK && d.kind <= 1 && !(raw_mask != nullptr && raw_mask[i] != 0)) {
    const int64_t off = offsets[i];
    o = exif_orientation(bytes + off, lengths ? lengths[i] : offsets[i + 1] - off);
    if (o < 2 || o > 8) o = kOrientNone;
  }
  d.pad0[0] = (uint8_t)o;
}

// One workgroup, after k_exif: the exclusive scan of the images' tile counts into OCtl::base
// (lane t takes the images [t per, (t + 1) per), per = ceil(B / 1024), as scan_and_place), and
// the ticket counter cleared.
__device__ __forceinline__ int32_t orient_tiles(const ImgDesc& d) {
  return d.pad0[0] ? ceil_div(d.width, kOrientTile) * ceil_div(d.height, kOrientTile) : 0;
}
__global__ void __launch_bounds__(1024) k_orient_scan(const ImgDesc* __restrict__ desc, int B, OCtl* __restrict__ octl) {
  __shared__ int32_t part[1024];
  const int t = threadIdx.x;
  const int per = (B + 1023) / 1024;
  int32_t local = 0;
  for (int k = 0; k < per && t * per + k < B; ++k) local += orient_tiles(desc[t * per + k]);
  part[t] = local;
  __syncthreads();
  for (int s = 1; s < 1024; s <<= 1) {  // Hillis-Steele inclusive scan
    const int32_t v = t >= s ? part[t - s] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int32_t base = t ? part[t - 1] : 0;
  for (int k = 0; k < per && t * per + k < B; ++k) {
    octl->base[t * per + k] = base;
    base += orient_tiles(desc[t * per + k]);
  }
  if (t == 1023) {
    octl->base[B] = part[1023];
    octl->total = (uint32_t)part[1023];
    octl->ticket = 0;
  }
}

// The pixel whose first byte lies `at` bytes into an RGB region (4-byte aligned, at least 8 bytes
// of slack behind its last pixel: rgb_region_bytes), from the two aligned words that hold it.
__device__ __forceinline__ uint32_t orient_load_px(const uint8_t* __restrict__ rgb, int64_t at) {
  const uint32_t* w = (const uint32_t*)(rgb + (at & ~(int64_t)3));
  const uint64_t v = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
  return (uint32_t)(v >> (8 * (int)(at & 3))) & 0xFFFFFFu;
}

// One wave writes n <= 64 pixels of a destination row from `row` on (any byte alignment): lane l
// owns the aligned word l of the row's span, builds it from the one or two pixels it straddles
// (get(i): pixel i of the run as 0x00BBGGRR, called by every lane) and stores it whole; only the
// words that the run's first and last bytes share with its neighbours go out as bytes.
template <typename Get>
__device__ __forceinline__ void orient_store_row(uint8_t* __restrict__ row, int n, int lane, Get get) {
  const int p0 = 4 * lane - (int)((uintptr_t)row & 3);  // the word's first byte, relative to the run's (>= -3)
  const int ia = (p0 + 3) / 3 - 1;                      // floor(p0 / 3): the pixel that byte belongs to
  const int sh = p0 - 3 * ia;                           // 0..2: where the word starts inside that pixel
  const uint32_t a = get(min(max(ia, 0), n - 1)), b = get(min(max(ia + 1, 0), n - 1));
  const uint32_t word = (uint32_t)((((uint64_t)b << 24) | a) >> (8 * sh));
  const int lo = max(0, -p0), hi = min(4, 3 * n - p0);
  if (hi - lo == 4) {
    *(uint32_t*)(row + p0) = word;
  } else {
    for (int k = lo; k < hi; ++k) row[p0 + k] = (uint8_t)(word >> (8 * k));
  }
}

// Persistent workgroups of four waves; a ticket is one kOrientTile x kOrientTile tile of a
// turning image (OCtl), so a large photograph spreads over the whole device and an image that
// stays as it is costs nothing.  The mapping is exif_parse.hpp's orient_map, read from the
// output's side: destination row j of the tile, column i <- source (row, column) of the tile.
//  * Orientations 2..4 (rows map to rows): a wave takes a row segment, lane c the pixel c (two
//    aligned words, funnel-shifted), and the lanes exchange pixels in registers (__shfl) in
//    mirrored or plain order while packing the destination words.
//  * Orientations 5..8 (rows become columns): the tile goes to LDS one pixel a word, rows of
//    kOrientTile + 1 words; a wave then packs the words of one destination row from one column
//    of it: lane l reads the pixels floor((4 l - s) / 3) and the next, that is two reads in each
//    of which every lane is on a different row of the column, and with the odd pitch on a
//    different one of the 64 banks.
// Either way global memory is read and written in aligned words, source rows and destination
// rows both contiguous across the wave; bytes only at the two ends of a row segment.
constexpr int kOrientPitch = kOrientTile + 1;
static_assert(kOrientTile == 64, "k_orient: one lane per pixel of a row segment, 64 LDS banks");
__global__ void __launch_bounds__(256) k_orient(const ImgDesc* __restrict__ desc, uint8_t* __restrict__ ws,
                                                OCtl* __restrict__ octl, int B) {
  __shared__ uint32_t tile[kOrientTile * kOrientPitch];
  __shared__ uint32_t s_ticket;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (;;) {
    __syncthreads();
    if (tid == 0) s_ticket = atomicAdd(&octl->ticket, 1u);
    __syncthreads();
    const uint32_t t = s_ticket;
    if (t >= octl->total) return;
    int img = 0, hi = B - 1;  // the last image whose base is <= t (those without tiles share the next one's base)
    while (img < hi) {
      const int mid = (img + hi + 1) >> 1;
      if ((uint32_t)octl->base[mid] <= t) img = mid;
      else hi = mid - 1;
    }
    const ImgDesc& d = desc[img];
    if (d.status != DINO_IMG_OK || d.pad0[0] < 2) continue;  // (failed in the decode: zero-filled by the caller)
    const int W = d.width, H = d.height;
    const OrientMap m = orient_map(d.pad0[0]);
    const int tiles_x = ceil_div(W, kOrientTile), lt = (int)t - octl->base[img];
    const int x0 = (lt % tiles_x) * kOrientTile, y0 = (lt / tiles_x) * kOrientTile;
    const int tw = min(kOrientTile, W - x0), th = min(kOrientTile, H - y0);
    const uint8_t* src = ws + d.rgb_off;
    uint8_t* dst = ws + d.rgb_off + rgb_region_bytes(W, H);
    const int OW = m.swap ? H : W, OH = m.swap ? W : H;
    const int nu = m.swap ? th : tw, nv = m.swap ? tw : th;  // the tile on the output's side: nv rows of nu pixels
    const int u0 = m.swap ? y0 : x0, v0 = m.swap ? x0 : y0;
    const int ox0 = m.fx ? OW - (u0 + nu) : u0, oy0 = m.fy ? OH - (v0 + nv) : v0;
    if (m.swap) {
      for (int k = tid; k < th * kOrientTile; k += 256) {
        const int r = k / kOrientTile, c = k % kOrientTile;
        if (c < tw) tile[r * kOrientPitch + c] = orient_load_px(src, ((int64_t)(y0 + r) * W + x0 + c) * 3);
      }
      __syncthreads();
    }
    for (int j = wave; j < nv; j += 4) {
      const int lv = m.fy ? nv - 1 - j : j;
      uint8_t* row = dst + ((int64_t)(oy0 + j) * OW + ox0) * 3;
      if (m.swap) {
        orient_store_row(row, nu, lane, [&](int i) { return tile[(m.fx ? nu - 1 - i : i) * kOrientPitch + lv]; });
      } else {
        const uint32_t px = lane < tw ? orient_load_px(src, ((int64_t)(y0 + lv) * W + x0 + lane) * 3) : 0u;
        orient_store_row(row, nu, lane, [&](int i) { return (uint32_t)__shfl((int)px, m.fx ? nu - 1 - i : i); });
      }
    }
  }
}

// One lane per image, after k_orient: the descriptor of an image that turned shows the upright
// image (its second region, and the swapped width and height for orientations 5..8).
__global__ void __launch_bounds__(64) k_orient_done(ImgDesc* __restrict__ desc, int B) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= B) return;
  ImgDesc& d = desc[i];
  if (d.status != DINO_IMG_OK || d.pad0[0] < 2) return;
  d.rgb_off += rgb_region_bytes(d.width, d.height);
  if (orient_map(d.pad0[0]).swap) {
    const int32_t w = d.width;
    d.width = d.height;
    d.height = w;
  }
}
