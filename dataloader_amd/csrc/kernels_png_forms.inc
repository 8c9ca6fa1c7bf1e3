// kernels_png_forms.inc — part of kernels.hip's translation unit (not compiled on its own).  Needs kernels_png.inc.
// ---------------------------------------------------------------------------
// PNG forms beyond 8 bits without interlace (png_forms.hpp): k_pnghead_forms, k_unfilter_forms
// ---------------------------------------------------------------------------
// Launched only by a context with dino_ctx_set_png_forms on.  Between them k_pngwalk and k_inflate
// run as for any kind-4 image: the zlib stream is the same, and png_inflated_bytes answers the
// bytes of all passes.

// One lane per image, right after k_pnghead, which stays the code it is: a file it declined for
// its bit depth or its interlace alone gets the extended-form descriptor (parse_png_forms_head:
// coef_bytes = inflated bytes, mcus_x = depth, mcus_y = interlace, max_h = filter unit; fields
// the JPEG stages of a kind-4 image never read).
__global__ void __launch_bounds__(64) k_pnghead_forms(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ offsets,
                                                      const int64_t* __restrict__ lengths,
                                                      const uint8_t* __restrict__ raw_mask, int B,
                                                      ImgDesc* __restrict__ desc) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= B || (raw_mask != nullptr && raw_mask[i] != 0)) return;
  if (desc[i].status != kPngDecline || desc[i].kind != kPngKind) return;
  const int64_t off = offsets[i], len = lengths ? lengths[i] : offsets[i + 1] - off;
  parse_png_forms_head(bytes + off, len, &desc[i]);
}

// One wave per extended-form image reverses the row filters over the rows of all passes laid end
// to end, 64 rows at a time: lane r takes row y0 + r of that sequence and runs one filter unit
// (u = 1, 2, 3, 4, 6 or 8 bytes) behind lane r - 1.  At step t it reconstructs unit x = t - r from
// its own previous unit (left), the unit lane r - 1 reconstructed a step before (up, two
// __shfl_up) and the one before that (up-left); a unit is two 32-bit registers.  A row that is
// the first of its pass takes up = 0, so a band may hold rows of several passes and of several
// widths; it runs for the units of its longest row + 63 steps.  Lane 63's row goes to the carry
// row (8 bytes a unit) unless the next band starts a pass.
//
// Data movement: a lane's row is contiguous in the inflated region.  The lane streams it in
// aligned 16-byte loads into its own ring of two chunks in LDS, the chunk after the one a step
// may touch is in flight in registers (loaded when the lane enters the chunk before it), and a
// step reads its u bytes from the ring as three words at the lane's own offset: LDS is the store
// that takes a per-lane index (a register array would go to scratch).  Rings are kFormPitch = 9
// words apart: lanes of a half wave at equal ring offsets hit 32 distinct banks; at unequal
// offsets a bank is within reach of 8 lanes (the worst conflict).  64 x 36 = 2304 bytes.
//
// Each pixel of a unit (8 / depth of them below 8 bits, else one) goes through png_form_to_rgb
// straight to its place in the image, rgb[(y0p + yp dy) W + x0p + xp dx]: Adam7 needs no second
// pass.  Byte stores, as in k_unfilter.  A filter byte above 4 fails the image.
constexpr int kFormPitch = 9;  // words between two lanes' rings (8 words each)
__device__ __forceinline__ uint4 form_chunk(const uint8_t* inf, int64_t cap, int64_t c) {
  return c >= 0 && 16 * c + 16 <= cap ? *(const uint4*)(inf + 16 * c) : make_uint4(0u, 0u, 0u, 0u);
}
__device__ __forceinline__ void form_ring_put(uint32_t* ring, int64_t c, uint4 v) {
  uint32_t* q = ring + 4 * (int)(c & 1);
  q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
}

__global__ void __launch_bounds__(64) k_unfilter_forms(ImgDesc* __restrict__ desc, uint8_t* __restrict__ ws) {
  __shared__ uint32_t s_ring[64 * kFormPitch];
  ImgDesc& d = desc[blockIdx.x];
  if (d.status != DINO_IMG_OK || !png_is_form(d)) return;
  const PngForm f = png_form_of(d);
  const int lane = threadIdx.x, u = f.unit(), depth = f.depth, color = f.color, W = f.W;
  const int per = depth < 8 ? 8 / depth : 1;  // pixels of a unit
  const int R = png_form_geom(f).rows;
  const uint8_t* inf = ws + d.plane_off;
  const int64_t cap = d.rgb_off - d.plane_off;
  const uint8_t* pal = ws + d.htab_off;
  uint2* carry = (uint2*)(ws + d.coef_off);
  const int64_t ncarry = (d.plane_off - d.coef_off - 16) / 8;  // >= png_form_max_units(d)
  uint8_t* rgb = ws + d.rgb_off;
  uint32_t* ring = s_ring + lane * kFormPitch;
  const uint64_t umask = u == 8 ? ~0ull : ((1ull << (8 * u)) - 1);
  int bad = 0;
  for (int y0 = 0; y0 < R; y0 += 64) {
    const int r = y0 + lane;
    const bool active = r < R;
    const PngRowAt at = png_form_row(f, active ? r : 0);
    const PngPass& ps = at.pass;
    const int nu = active ? ps.rb / u : 0;  // units of the row
    const bool top = at.yp == 0;            // first row of its pass: nothing above
    int ft = active ? inf[at.off] : 0;
    if (ft > 4) bad = 1, ft = 0;
    // the band's steps: its longest row
    int steps = nu;
    for (int m = 32; m >= 1; m >>= 1) steps = max(steps, __shfl_xor(steps, m));
    // lane 63's row feeds lane 0 of the next band unless that row starts a pass (or there is none)
    const bool carry_out = y0 + 64 < R && png_form_row(f, y0 + 64 < R ? y0 + 64 : 0).yp != 0;
    const bool carry_in = y0 > 0 && !top;  // (read by lane 0 only)
    // the ring: chunks c0 and c0 + 1 in place, c0 + 2 in flight
    const int64_t a0 = at.off + 1;  // the row's first data byte
    int64_t cn = (a0 >> 4) + 2;
    uint4 nxt = make_uint4(0u, 0u, 0u, 0u);
    if (active) {
      form_ring_put(ring, cn - 2, form_chunk(inf, cap, cn - 2));
      form_ring_put(ring, cn - 1, form_chunk(inf, cap, cn - 1));
      nxt = form_chunk(inf, cap, cn);
    }
    uint64_t left = 0, upleft = 0, mine = 0;
    for (int t = 0; t < steps + 63; ++t) {
      const int x = t - lane;
      const bool in = x >= 0 && x < nu;
      uint64_t up = (uint64_t)(uint32_t)__shfl_up((uint32_t)mine, 1) | ((uint64_t)(uint32_t)__shfl_up((uint32_t)(mine >> 32), 1) << 32);
      if (lane == 0) {
        up = 0;
        if (carry_in && in && x < ncarry) {
          const uint2 cv = carry[x];
          up = (uint64_t)cv.x | ((uint64_t)cv.y << 32);
        }
      }
      if (top) up = 0;
      mine = 0;
      if (in) {
        const int64_t a = a0 + (int64_t)x * u;
        if ((a >> 4) + 1 == cn) {  // entering the last chunk in the ring: the one in flight lands, the next leaves
          form_ring_put(ring, cn, nxt);
          ++cn;
          nxt = form_chunk(inf, cap, cn);
        }
        const int o = (int)(a & 31), wi = o >> 2, sh = 8 * (o & 3);
        const uint32_t w0 = ring[wi], w1 = ring[(wi + 1) & 7], w2 = ring[(wi + 2) & 7];
        uint64_t cur = ((uint64_t)w0 | ((uint64_t)w1 << 32)) >> sh;
        if (sh) cur |= (uint64_t)w2 << (64 - sh);
        cur &= umask;
        for (int c = 0; c < u; ++c) {
          const int s = 8 * c;
          const int v = (int)((cur >> s) & 255) +
                        png_predict(ft, (int)((left >> s) & 255), (int)((up >> s) & 255), (int)((upleft >> s) & 255));
          mine |= (uint64_t)(v & 255) << s;
        }
        for (int k = 0; k < per; ++k) {
          const int xp = x * per + k;
          if (xp < ps.w) png_form_to_rgb(color, depth, mine, k, pal, rgb + png_form_dest(ps, W, at.yp, xp) * 3);
        }
        if (lane == 63 && carry_out && x < ncarry) carry[x] = make_uint2((uint32_t)mine, (uint32_t)(mine >> 32));
      }
      left = mine;
      upleft = up;
    }
    __threadfence_block();
    __syncthreads();
  }
  if (__syncthreads_or(bad) && lane == 0) d.status = DINO_IMG_CORRUPT;
}
