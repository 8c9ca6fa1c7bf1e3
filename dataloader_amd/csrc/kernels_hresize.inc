// kernels_hresize.inc — part of kernels.hip's translation unit (not compiled on its own).  Needs main_prio (kernels.hip).
// Horizontal pass.  A workgroup owns bands of R source rows of one view.  The
// crop's pixels for those rows are staged in LDS as RGBX words (each lane turns
// 12 source bytes = 4 pixels into one 16-byte LDS store); the view's taps are
// staged in LDS too when they fit.  Each lane then resamples one (row, x) with
// one LDS word per tap and writes the three channels to planar temp rows
// [3][crop_h][S].  Crops too wide for LDS take a direct (global) path.
// The tile shape (hresize_tile, hr_view_chunks) is in hresize_tile.hpp.
constexpr int kHrStageUnroll = 4;  // staging loads in flight per lane (2: 168.0k, 8: 168.8k, 4: 170.2k img/s C2)

// The view of work item c among the nc class views (b, v0 + j), j = view index mod nvc:
// the last view whose first item is <= c (views without items share their successor's
// first item).  64-ary search by each wave: two rounds of loads for 4096 views.
__device__ __forceinline__ int hr_find_view(const ViewPlan* __restrict__ plan, int nv, int v0, int nvc, int nc, int c) {
  int lo = 0, len = nc;
  const int lane = threadIdx.x & 63;
  while (len > 1) {
    const int step = (len + 63) >> 6;
    const int cand = lo + lane * step;
    bool le = false;
    if (cand < lo + len) {
      const int b = cand / nvc;
      le = plan[b * nv + v0 + (cand - b * nvc)].hr_base <= c;
    }
    const uint64_t m = __ballot(le);  // bit 0 set: plan[lo].hr_base <= c holds throughout
    const int last = 63 - __builtin_clzll(m);
    lo += last * step;
    len = min(step, len - last * step);
  }
  return lo;
}

// One tile: nr staged rows x the outputs [x0, x0 + sw) of a slice.  Lane (row pair, x)
// accumulates three signed-dot4 digit products per row, channel and group of 4 taps.
// Rows are staged with the sign bit flipped (p - 128 as int8) from source column c0,
// word-interleaved: word (gw, r, c) = 4 pixels gw of row r, channel c at gw * R3p + 3 r + c
// (R3p = hresize_r3p(R): even, so a row pair's six words are one 8-byte-aligned run: three
// ds_read_b64 per group and one address for all of them).  The taps' pixels start at xmin,
// so each group's 4 pixels are one v_alignbyte of a word and the next group's (carried).
// The group loop runs the view's ng_max groups for every lane (taps past an output's own
// count are zero digits, k_rcoeffs), a wave-uniform trip count the compiler unrolls for
// NG <= 8.  Exact: the int32 sum equals Pillow's.
template <int NG>
__device__ __forceinline__ void hresize_tile_dot(const uint32_t* __restrict__ rows, int R3p, int nr, int r0, int x0,
                                                 int sw, int c0, int S, int ng, int ngp, const int4* __restrict__ hx,
                                                 const uint4* __restrict__ hg, uint8_t* __restrict__ tmp, int64_t cpl) {
  if (NG) ng = NG;
  const int npair = (nr + 1) >> 1;
  const int qs = R3p >> 1;  // uint2 stride per source group
  // lane task (row pair rp, output xl), advanced by the block size without dividing again
  const int dq = (int)blockDim.x / sw, dr = (int)blockDim.x - dq * sw;
  int rp = (int)threadIdx.x / sw, xl = (int)threadIdx.x - rp * sw;
  for (; rp < npair; rp += dq, xl += dr, (xl >= sw ? (xl -= sw, ++rp) : 0)) {
    const int ra = 2 * rp;  // rows ra, ra + 1 (a band's odd last row pairs with an unstored row: not written)
    const int4 h = hx[xl];
    const int lo = h.x - c0;
    const uint32_t sh = (uint32_t)(lo & 3);
    const uint2* q = (const uint2*)(rows + __umul24((uint32_t)(lo >> 2), (uint32_t)R3p) + 3 * ra);
    uint32_t lw[6];
    {
      const uint2 a0 = q[0], a1 = q[1], a2 = q[2];
      lw[0] = a0.x, lw[1] = a0.y, lw[2] = a1.x, lw[3] = a1.y, lw[4] = a2.x, lw[5] = a2.y;
    }
    int32_t acc[6][3];  // digit 0 starts at the rounding + sign-flip correction h.z
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[k][0] = h.z, acc[k][1] = acc[k][2] = 0;
    const uint4* dgp = hg + xl * ngp;  // this output's taps: ngp consecutive groups (immediate offsets)
#pragma unroll
    for (int g = 0; g < ng; ++g) {
      const uint4 dg = dgp[g];
      const uint2* qn = q + (g + 1) * qs;
      const uint2 b0 = qn[0], b1 = qn[1], b2 = qn[2];
      const uint32_t uw[6] = {b0.x, b0.y, b1.x, b1.y, b2.x, b2.y};
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const int32_t pa = (int32_t)__builtin_amdgcn_alignbyte(uw[k], lw[k], sh);
        acc[k][0] = __builtin_amdgcn_sdot4(pa, (int32_t)dg.x, acc[k][0], false);
        acc[k][1] = __builtin_amdgcn_sdot4(pa, (int32_t)dg.y, acc[k][1], false);
        acc[k][2] = __builtin_amdgcn_sdot4(pa, (int32_t)dg.z, acc[k][2], false);
        lw[k] = uw[k];
      }
    }
    // int32 wrap-around is harmless: the true sum (Pillow's int32 ss) fits in int32
    // (clip8_acc as one med3: the sum is < 2^30 unless it clips to 255, and <= 0 clips to 0;
    // 32-bit offsets: a view's planes hold < 3 x 2^20 x 1024 bytes)
    const uint32_t ob = (uint32_t)((r0 + ra) * S + x0 + xl);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (ra + i >= nr) break;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int k = 3 * i + c;
        const uint32_t so = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)(i * S) + (uint32_t)c * (uint32_t)cpl));
        const int32_t sum = (int32_t)((uint32_t)acc[k][0] + ((uint32_t)acc[k][1] << 8) + ((uint32_t)acc[k][2] << 16));
        tmp[ob + so] = (uint8_t)min(max(sum >> kPrecisionBits, 0), 255);
      }
    }
  }
}

// Horizontal pass in tiles of (slice of outputs) x (band of rows), shaped by
// hresize_tile: the slice's taps always come from LDS, and the band stages only the
// source columns the slice reads [xmin(x0), xmin(x1-1) + xcnt(x1-1)), so wide crops
// take narrower slices to keep >= kHresizeMinRows rows per band.  A persistent grid
// takes the class's work items (kHrBandsPerItem bands of one slice, hr_view_chunks) in
// turn: with mixed crop sizes (C3) a fixed number of workgroups per view left the
// largest views' workgroups running alone at the end of the launch.
__device__ __forceinline__ void hresize_item(const ImgDesc* __restrict__ desc, const dino_view_params* __restrict__ prm,
                                             const ViewPlan* __restrict__ plan, int nv, int v0, int nvc, int nc, int c,
                                             const uint8_t* __restrict__ ws, uint8_t* __restrict__ aws, uint8_t* smem);

#ifndef DINO_HRESIZE_WAVES  // (A/B: minimum waves per SIMD the register allocation must allow)
#define DINO_HRESIZE_WAVES 1
#endif
__global__ void __launch_bounds__(256, DINO_HRESIZE_WAVES) k_hresize(const ImgDesc* __restrict__ desc, const dino_view_params* __restrict__ prm,
                                                 ViewPlan* __restrict__ plan, int nv, int v0, int nvc, int B,
                                                 const uint8_t* __restrict__ ws, uint8_t* __restrict__ aws) {
  main_prio();
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  __shared__ int s_item[2];
  const int nc = B * nvc;
  // persistent grid over the class's work items (k_vplan's per-class prefix), taken in turn
  // from the class's counter (zeroed by k_vplan), the next one fetched while this one runs
  const ViewPlan vl = plan[(B - 1) * nv + v0 + nvc - 1];
  const int nitems_all = vl.hr_base + vl.hr_chunks;
  int* ctr = v0 == 0 ? &plan[B * nv].hr_chunks : &plan[B * nv].hr_base;
  if (threadIdx.x == 0) s_item[0] = atomicAdd(ctr, 1);
  __syncthreads();
  for (int it = 0, c = s_item[0]; c < nitems_all; ++it) {
    if (threadIdx.x == 0) s_item[(it + 1) & 1] = atomicAdd(ctr, 1);
    hresize_item(desc, prm, plan, nv, v0, nvc, nc, c, ws, aws, smem);
    __syncthreads();
    c = s_item[(it + 1) & 1];
  }
}

__device__ __forceinline__ void hresize_item(const ImgDesc* __restrict__ desc, const dino_view_params* __restrict__ prm,
                                             const ViewPlan* __restrict__ plan, int nv, int v0, int nvc, int nc, int c,
                                             const uint8_t* __restrict__ ws, uint8_t* __restrict__ aws, uint8_t* smem) {
  {
    const int j = hr_find_view(plan, nv, v0, nvc, nc, c);
    const int b = j / nvc;
    const int i = b * nv + v0 + (j - b * nvc);
    const ViewPlan vp = plan[i];
    if (!vp.ok || !vp.kh) return;  // (no items: not reached)
    const int item = c - vp.hr_base;
    const dino_view_params p = prm[i];
    const ImgDesc& d = desc[b];
    const int S = p.out_size, W = d.width, cw = p.crop_w, kh = vp.kh;
    const ViewTables<const uint8_t*> T = view_tables((const uint8_t*)aws + vp.rcoef_off, S, vp.kh, vp.kv);
    const int32_t *gb = (const int32_t*)T.hb, *gt = (const int32_t*)T.ht;
    const int4* ghx = (const int4*)T.hx;
    const uint4* ghg = (const uint4*)T.hg;
    const uint8_t* rgb = ws + d.rgb_off;
    uint8_t* tmp = aws + vp.htmp_off;
    const int64_t cpl = (int64_t)p.crop_h * S;
    const int ng_max = (kh + 3) / 4;
    const int ngp = ng_max | 1;  // tap groups per output in LDS: odd, so 16 lanes' b128 reads hit distinct banks
    const HrTile tl = hresize_tile(S, cw, kh);
    const int sw = tl.sw, pitch = tl.pitch, R = tl.R, R3p = tl.R3p;
    if (R < 1) {  // direct path: taps and pixels from global memory (crops too wide for LDS)
      const SrcView src{rgb + ((int64_t)p.crop_top * W + p.crop_left) * 3, (int64_t)W * 3, 3, 1};
      const CoefView cv{gb, gt, kh};
      for (int64_t e = (int64_t)item * blockDim.x + threadIdx.x; e < cpl; e += (int64_t)kHrDirectItems * blockDim.x) {
        const int r = (int)(e / S), x = (int)(e - (int64_t)r * S);
        for (int ch = 0; ch < 3; ++ch) tmp[ch * cpl + e] = hresize_at(src, cv, r, x, ch);
      }
      return;
    }
    // LDS: the staged rows first (an edge output's zero-tap over-read stays inside the rows'
    // pad), then the slice's taps
    uint32_t* rows = (uint32_t*)smem;
    int4* lx = (int4*)(smem + ((hresize_rows_bytes(pitch, R, ng_max) + 15) & ~15));
    uint4* lg = (uint4*)(lx + sw);
    const int nbands = (p.crop_h + R - 1) / R;
    const int nbg = (nbands + kHrBandsPerItem - 1) / kHrBandsPerItem;
    // the item: slice sl (outputs [x0, x0 + swn)), bands [band0, band1)
    const int sl = item / nbg;
    const int band0 = (item - sl * nbg) * kHrBandsPerItem, band1 = min(nbands, band0 + kHrBandsPerItem);
    const int x0 = sl * sw, swn = min(sw, S - x0);
    const int c0 = ghx[x0].x & ~3;  // first source column staged (4-aligned within the crop)
    const int c1 = min(cw, ghx[x0 + swn - 1].x + gb[2 * (x0 + swn - 1) + 1]);
    const int ngroups = (c1 - c0 + 3) >> 2;  // staged groups of 4 pixels per row
    // taps of the slice -> LDS (the previous item ended with a barrier)
    for (int k = threadIdx.x; k < swn; k += blockDim.x) lx[k] = ghx[x0 + k];
    for (int k = threadIdx.x; k < swn * ng_max; k += blockDim.x) {
      const int g = k / swn, xl = k - g * swn;
      lg[xl * ngp + g] = ghg[(int64_t)g * S + x0 + xl];
    }
    // staging item e of a band: row e / ngroups, group e % ngroups (12 source bytes = 4
    // pixels -> one word per channel, de-interleaved by v_perm byte selects, sign bit
    // flipped).  kHrStageUnroll items per lane in flight: their 16-byte loads are issued
    // together and waited on once (one item at a time waited a full memory latency per
    // item: k_hresize 0.95 -> 0.85 ms per C2 step).  (Issuing the next band's first chunk
    // before this band's dot products, registers held across them, measured slower: 114-147
    // VGPRs, 3-4 waves per SIMD instead of 5.)
    const int64_t spitch = (int64_t)W * 3;
    const int dr = (int)blockDim.x / ngroups, dg = (int)blockDim.x - dr * ngroups;
    struct Stage {
      const uint8_t* base;
      int nst, e, sr, sg;
    };
    auto stage_begin = [&](int band) {
      const int r0 = band * R;
      Stage st;
      st.base = rgb + ((int64_t)(p.crop_top + r0) * W + p.crop_left + c0) * 3;
      st.nst = min(R, p.crop_h - r0) * ngroups;
      st.e = (int)threadIdx.x;
      st.sr = (int)threadIdx.x / ngroups;
      st.sg = (int)threadIdx.x - st.sr * ngroups;
      return st;
    };
    uint4 wv[kHrStageUnroll];
    uint32_t shv[kHrStageUnroll], dov[kHrStageUnroll];
    auto stage_issue = [&](Stage& st) {  // loads of the chunk at st.e (none past the band)
#pragma unroll
      for (int u = 0; u < kHrStageUnroll; ++u) {
        const bool ok = st.e + u * (int)blockDim.x < st.nst;
        // past the band: load the band's first words again (in bounds), nothing is stored
        const uint8_t* src = ok ? st.base + st.sr * spitch + 12 * st.sg : st.base;
        const uint32_t mis = (uint32_t)((uintptr_t)src & 3);
        wv[u] = *(const uint4*)(src - mis);
        shv[u] = ok ? 8u * mis : 0xFFFFFFFFu;
        dov[u] = (uint32_t)(st.sg * R3p + 3 * st.sr);
        st.sr += dr;
        st.sg += dg;
        if (st.sg >= ngroups) st.sg -= ngroups, ++st.sr;
      }
      st.e += kHrStageUnroll * (int)blockDim.x;
    };
    auto stage_commit = [&]() {
#pragma unroll
      for (int u = 0; u < kHrStageUnroll; ++u) {
        if (shv[u] == 0xFFFFFFFFu) break;
        const uint32_t sh = shv[u];
        const uint32_t q0 = (uint32_t)((((uint64_t)wv[u].y << 32) | wv[u].x) >> sh);  // R0 G0 B0 R1
        const uint32_t q1 = (uint32_t)((((uint64_t)wv[u].z << 32) | wv[u].y) >> sh);  // G1 B1 R2 G2
        const uint32_t q2 = (uint32_t)((((uint64_t)wv[u].w << 32) | wv[u].z) >> sh);  // B2 R3 G3 B3
        const uint32_t cr = __builtin_amdgcn_perm(q2, __builtin_amdgcn_perm(q1, q0, 0x0C060300u), 0x05020100u);
        const uint32_t cg = __builtin_amdgcn_perm(q2, __builtin_amdgcn_perm(q1, q0, 0x0C070401u), 0x06020100u);
        const uint32_t cb = __builtin_amdgcn_perm(q2, __builtin_amdgcn_perm(q1, q0, 0x0C0C0502u), 0x07040100u);
        uint32_t* dst = rows + dov[u];
        dst[0] = cr ^ 0x80808080u;
        dst[1] = cg ^ 0x80808080u;
        dst[2] = cb ^ 0x80808080u;
      }
    };
    for (int band = band0; band < band1; ++band) {
      const int r0 = band * R, nr = min(R, p.crop_h - r0);
      Stage st = stage_begin(band);
      while (st.e < st.nst) {
        stage_issue(st);
        stage_commit();
      }
      __syncthreads();
      switch (ng_max) {
#define DINO_HR_CASE(N) \
  case N: \
    hresize_tile_dot<N>(rows, R3p, nr, r0, x0, swn, c0, S, ng_max, ngp, lx, lg, tmp, cpl); \
    break;
        DINO_HR_CASE(1)
        DINO_HR_CASE(2)
        DINO_HR_CASE(3)
        DINO_HR_CASE(4)
        DINO_HR_CASE(5)
        DINO_HR_CASE(6)
        DINO_HR_CASE(7)
        DINO_HR_CASE(8)
#undef DINO_HR_CASE
        default:
          hresize_tile_dot<0>(rows, R3p, nr, r0, x0, swn, c0, S, ng_max, ngp, lx, lg, tmp, cpl);
      }
      __syncthreads();
    }
  }
}
