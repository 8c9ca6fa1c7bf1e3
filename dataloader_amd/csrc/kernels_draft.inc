// kernels_draft.inc — part of kernels.hip's translation unit (not compiled on its own).  Needs
// draft.hpp, xcd_blk, wave_lds_sync, kIdctBlocksPerWg, kIdctPre, idct_load_pre, idct_group_dense /
// _sparse / _pass1 / _pass2 (kernels.hip).
// ---------------------------------------------------------------------------
// Reduced-size JPEG decode (Pillow's Image.draft): k_draft -> .. -> k_idct_red -> k_color_red
// ---------------------------------------------------------------------------
// Launched only by a context with dino_ctx_set_draft on.  An image whose sides allow a scale of
// 2, 4 or 8 never exists at its coded size: each block is transformed straight to 4x4, 2x2 or
// 1x1 samples (idct.hpp, jidctred.c), chroma blocks one size larger where that spares the
// upsampling (draft.hpp draft_comp_size), and the colour stage reads planes that are already
// at, or nearer to, the output size.  Entropy decode and coefficients are untouched.

// One lane per image, between k_parse (k_pnghead) and k_plan, so that k_parse stays the code it
// was: a decodable JPEG of up to three components gets its scale, keeps its coded size in
// full_w / full_h and shows every later stage (k_plan's RGB size, k_params, k_vsizes, k_info) the
// scaled one.  The block grids (bw, bh, mcus_*), dw / dh and the plane reservation stay those of
// the coded size: the entropy stages read nothing else.
__global__ void __launch_bounds__(64) k_draft(ImgDesc* __restrict__ desc, int B, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= B) return;
  ImgDesc& d = desc[i];
  if (d.status != DINO_IMG_OK || d.kind > 1 || d.ncomp > kMaxComp) return;
  const int sh = draft_shift_of(d.width, d.height, n);
  if (sh == 0) return;
  d.draft_shift = sh;
  d.full_w = d.width;
  d.full_h = d.height;
  d.width = draft_dim(d.width, sh);
  d.height = draft_dim(d.height, sh);
}

// The group steps of a block scaled to 4x4 and 2x2 (sb: the group's LDS block, rows of 9 words,
// as k_idct).  Pass 1: lane l takes column l where the transform reads it and leaves its
// results in rows 0 .. size - 1 of that column; pass 2: lane l < size takes row l.
__device__ __forceinline__ void idct_group_pass1_red(int32_t* sb, int l, const uint16_t* q, int size) {
  if (size == 4 ? l == 4 : (l != 0 && !(l & 1))) return;  // jidctred.c: columns the second pass never uses
  int32_t raw[8], qq[8], w[4];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    raw[r] = sb[r * 9 + l];
    qq[r] = (int32_t)(int16_t)q[r * 8 + l];
  }
  if (size == 4) {
    idct4_pass1(raw, qq, w);
#pragma unroll
    for (int r = 0; r < 4; ++r) sb[r * 9 + l] = w[r];
  } else {
    idct2_pass1(raw, qq, w);
    sb[l] = w[0];
    sb[9 + l] = w[1];
  }
}
// Returns row l's samples in the low `size` bytes (lanes l < size); every lane clears row l.
__device__ __forceinline__ uint32_t idct_group_pass2_red(int32_t* sb, int l, int size) {
  union {
    uint8_t b[4];
    uint32_t u;
  } o;
  o.u = 0u;
  if (l < size) {
    int32_t row[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) row[j] = sb[l * 9 + j];
    if (size == 4) idct4_pass2(row, o.b);
    else idct2_pass2(row, o.b);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) sb[l * 9 + j] = 0;
  return o.u;
}

// Grid (kIdctWgs, B) as k_idct; takes every component of every scaled image, one component
// after the other, so that the block size (and with it the path) is uniform over the workgroup:
//   8, 4, 2  a group of 8 lanes per block over the component's blocks in plane order (a wave's
//            eight blocks are one run of a plane row); k_idct's loads and LDS layout, then the
//            passes of the size; lane l stores row l: 8, 4 or 2 bytes at pitch bw * size;
//   1        no LDS and no entries: a lane takes four consecutive blocks of the plane (pitch bw:
//            the plane is its blocks in order), reads each DC from the block record (kind 0) or
//            coefficient 0 (kind 1) and stores the four samples as one word.
__global__ void __launch_bounds__(256) k_idct_red(const ImgDesc* __restrict__ desc, uint8_t* __restrict__ ws) {
  const BlkIdx bk = xcd_blk();
  __shared__ int32_t s_blk[kIdctBlocksPerWg][72];
  __shared__ uint8_t s_nat[80];
  const ImgDesc& d = desc[bk.y];
  if (d.status != DINO_IMG_OK || d.draft_shift == 0) return;
  const bool dense = d.kind == 1;
  if (threadIdx.x < 80) s_nat[threadIdx.x] = (uint8_t)((kNaturalOrder[threadIdx.x] >> 3) * 9 + (kNaturalOrder[threadIdx.x] & 7));
  const int ncomp = d.ncomp;
  const uint32_t* ent = (const uint32_t*)(ws + d.coef_off);
  const uint16_t* ent16 = (const uint16_t*)ent;
  const uint2* binfo = (const uint2*)(ws + d.binfo_off);
  uint8_t* planes = ws + d.plane_off;
  int moff[kMaxComp] = {0, 0, 0};  // first position of each component inside the MCU
  for (int i = d.blocks_per_mcu - 1; i >= 0; --i) moff[d.mcu_comp[i] < kMaxComp ? d.mcu_comp[i] : 0] = i;
  const int grp = threadIdx.x >> 3, l = threadIdx.x & 7;
  int32_t* sb = s_blk[grp];
#pragma unroll
  for (int j = 0; j < 8; ++j) sb[l * 9 + j] = 0;
  __syncthreads();
  for (int c = 0; c < ncomp; ++c) {
    const CompDesc& cd = d.comp[c];
    const int size = draft_comp_size(d, c);
    const int nb = cd.bw * cd.bh;  // < 2^31 / 64
    const uint16_t* q = d.qt[cd.tq];
    // plane block k -> its record in decode order (-1: no MCU covers it, it stays all zero)
    auto record = [&](int k) {
      const int by = k / cd.bw, bx = k - by * cd.bw;
      int b;
      if (ncomp == 1) {
        b = bx < d.mcus_x ? by * d.mcus_x + bx : -1;
      } else {
        const int my = by / cd.v, mx = bx / cd.h;
        b = (my * d.mcus_x + mx) * d.blocks_per_mcu + moff[c] + (by - my * cd.v) * cd.h + (bx - mx * cd.h);
      }
      return b >= 0 && b < d.total_blocks ? binfo[b] : make_uint2(0u, 0u);
    };
    if (size == 1) {
      const int32_t q0 = (int32_t)(int16_t)q[0];
      const int16_t* coef = (const int16_t*)(ws + d.coef_off + cd.coef_off);
      uint32_t* out = (uint32_t*)(planes + cd.plane_off);
      for (int w = bk.x * 256 + threadIdx.x; 4 * w < nb; w += gridDim.x * 256) {
        uint32_t v = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = 4 * w + j;
          if (k < nb) {
            const int32_t dc = dense ? (int32_t)coef[(int64_t)k * 64] : (int32_t)record(k).y >> 16;
            v |= (uint32_t)idct1_sample(dc, q0) << (8 * j);
          }
        }
        out[w] = v;
      }
      continue;
    }
    const int step = gridDim.x * kIdctBlocksPerWg, pitch = cd.bw * size;
    // as k_idct: the next block's record a turn ahead, its first entries once the record is there
    int gn = bk.x * kIdctBlocksPerWg + grp;
    uint2 bin = !dense && gn < nb ? record(gn) : make_uint2(0u, 0u);
    uint32_t pre[kIdctPre] = {};
    if (!dense && gn < nb) idct_load_pre(pre, l, bin, ent16);
    for (int g0 = bk.x * kIdctBlocksPerWg; g0 < nb; g0 += step) {
      const int k = gn;
      const bool valid = k < nb;
      const uint2 bi = bin;
      gn += step;
      if (!dense && gn < nb) bin = record(gn);
      if (valid && dense) idct_group_dense(sb, l, ws + d.coef_off + cd.coef_off + (int64_t)k * 128);
      else if (valid) idct_group_sparse(sb, l, s_nat, bi, pre, ent16, ent);
      wave_lds_sync();
      if (valid) {
        if (size == 8) idct_group_pass1(sb, l, q);
        else idct_group_pass1_red(sb, l, q, size);
      }
      wave_lds_sync();
      if (valid) {
        const int by = k / cd.bw, bx = k - by * cd.bw;
        uint8_t* at = planes + cd.plane_off + ((int64_t)by * size + l) * pitch + bx * size;
        if (size == 8) {
          *(uint64_t*)at = idct_group_pass2(sb, l);
        } else {
          const uint32_t v = idct_group_pass2_red(sb, l, size);
          if (l < size) {
            if (size == 4) *(uint32_t*)at = v;
            else *(uint16_t*)at = (uint16_t)v;
          }
        }
      }
      if (!dense && gn < nb) idct_load_pre(pre, l, bin, ent16);
      wave_lds_sync();
    }
  }
}

// Four samples of row y from column x on: the aligned word that holds the first and, where the
// address is not a multiple of 4 (pitch bw * size with size 1 or 2), the next one, joined by
// v_alignbyte.  (The second word may lie past the row: planes are followed by more workspace.)
__device__ __forceinline__ uint32_t pv_quad(const PlaneView& v, int x, int y) {
  const uintptr_t a = (uintptr_t)(v.p + (int64_t)y * v.pitch + x);
  const uint32_t* r = (const uint32_t*)(a & ~(uintptr_t)3);
  const uint32_t sh = (uint32_t)(a & 3);
  const uint32_t lo = r[0], hi = sh ? r[1] : 0u;
  return __builtin_amdgcn_alignbyte(hi, lo, sh);
}

// Grid (kColorWgs, B), one band of rows per workgroup and four consecutive pixels per lane as
// k_color; takes every scaled image.  When every component is at the output's resolution
// already (gray, 4:4:4 and, the IDCT having widened its chroma, 4:2:0, at every scale) a quad
// inside one row is one word per plane; a quad that wraps a row and every other sampling go per
// pixel through upsample_at's clamps with the method jdsample.c picks for the scaled sizes
// (draft.hpp draft_plane_view).
__global__ void __launch_bounds__(256) k_color_red(const ImgDesc* __restrict__ desc, uint8_t* __restrict__ ws) {
  const BlkIdx bk = xcd_blk();
  const ImgDesc& d = desc[bk.y];
  if (d.status != DINO_IMG_OK || d.draft_shift == 0) return;
  const int nc = d.ncomp;
  const uint8_t* planes = ws + d.plane_off;
  const PlaneView p0 = draft_plane_view(d, planes, 0);
  const PlaneView p1 = nc > 1 ? draft_plane_view(d, planes, 1) : p0;
  const PlaneView p2 = nc > 1 ? draft_plane_view(d, planes, 2) : p0;
  const bool ycc = nc > 1 && d.color == kYCbCr;
  const bool full = p0.method == kUpFull && p1.method == kUpFull && p2.method == kUpFull;
  uint32_t* rgb = (uint32_t*)(ws + d.rgb_off);
  const int W = d.width;
  const int64_t npx = (int64_t)W * d.height;
  const int64_t nq = (npx + 3) >> 2;
  const int64_t band = ((nq + gridDim.x - 1) / gridDim.x + blockDim.x - 1) / blockDim.x * blockDim.x;
  const int64_t qend = min(nq, (int64_t)(bk.x + 1) * band);
  for (int64_t q = (int64_t)bk.x * band + threadIdx.x; q < qend; q += blockDim.x) {
    const int64_t i0 = q * 4;
    int y = (int)((uint32_t)i0 / (uint32_t)W), x = (int)((uint32_t)i0 - (uint32_t)y * (uint32_t)W);
    union {
      uint8_t b[12];
      uint32_t w[3];
    } o;
    if (full && x + 3 < W) {
      const uint32_t s0 = pv_quad(p0, x, y);
      if (nc == 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) o.b[3 * j] = o.b[3 * j + 1] = o.b[3 * j + 2] = (uint8_t)(s0 >> (8 * j));
      } else {
        const uint32_t s1 = pv_quad(p1, x, y), s2 = pv_quad(p2, x, y);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int a = (int)((s0 >> (8 * j)) & 255u), b = (int)((s1 >> (8 * j)) & 255u), c = (int)((s2 >> (8 * j)) & 255u);
          if (ycc) {
            ycc_to_rgb(a, b, c, o.b + 3 * j);
          } else {
            o.b[3 * j] = (uint8_t)a;
            o.b[3 * j + 1] = (uint8_t)b;
            o.b[3 * j + 2] = (uint8_t)c;
          }
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (i0 + j < npx) {
          if (nc == 1) {
            o.b[3 * j] = o.b[3 * j + 1] = o.b[3 * j + 2] = (uint8_t)upsample_at(p0, x, y);
          } else {
            const int a = upsample_at(p0, x, y), b = upsample_at(p1, x, y), c = upsample_at(p2, x, y);
            if (ycc) {
              ycc_to_rgb(a, b, c, o.b + 3 * j);
            } else {
              o.b[3 * j] = (uint8_t)a;
              o.b[3 * j + 1] = (uint8_t)b;
              o.b[3 * j + 2] = (uint8_t)c;
            }
          }
        } else {
          o.b[3 * j] = o.b[3 * j + 1] = o.b[3 * j + 2] = 0;
        }
        if (++x == W) {
          x = 0;
          ++y;
        }
      }
    }
    rgb[3 * q] = o.w[0];
    rgb[3 * q + 1] = o.w[1];
    rgb[3 * q + 2] = o.w[2];
  }
}
