// kernels_view_plan.inc — part of kernels.hip's translation unit (not compiled on its own).  Needs scan_and_place (kernels.hip).
// ---------------------------------------------------------------------------
// Augment half
// ---------------------------------------------------------------------------
__global__ void k_params(const ImgDesc* __restrict__ desc, int B, dino_aug_config cfg, uint64_t seed,
                         uint64_t batch_index, dino_view_params* __restrict__ out) {
  const int nv = cfg.n_global + cfg.n_local;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * nv) return;
  int b = i / nv, v = i - b * nv;
  const ImgDesc& d = desc[b];
  int ok = d.status == DINO_IMG_OK;
  if (!ok && d.status < 0 && cfg.recipe == DINO_RECIPE_LEJEPA) {
    // CPULeJEPAPipeline (cpu.py:446-448) crops an undecodable image's views from a black
    // 224 x 224 canvas: the draws are those of that canvas (k_final writes its values)
    sample_view(cfg, seed, batch_index, b, v, 224, 224, 1, &out[i]);
    return;
  }
  sample_view(cfg, seed, batch_index, b, v, ok ? d.width : 1, ok ? d.height : 1, ok, &out[i]);
}

// Resample target of a view's crop box (0 in the record means the view size S).
__device__ __forceinline__ int view_rw(const dino_view_params& p) { return p.resize_w > 0 ? p.resize_w : p.out_size; }
__device__ __forceinline__ int view_rh(const dino_view_params& p) { return p.resize_h > 0 ? p.resize_h : p.out_size; }

// Host-supplied records are validated before any kernel indexes memory with them.
__device__ bool params_valid(const dino_view_params& p, const ImgDesc& d, int S) {
  if (p.out_size != S) return false;
  if (p.crop_top < 0 || p.crop_left < 0 || p.crop_h < 1 || p.crop_w < 1) return false;
  if ((int64_t)p.crop_top + p.crop_h > d.height || (int64_t)p.crop_left + p.crop_w > d.width) return false;
  if (p.blur && (p.ksize < 1 || p.ksize > 15 || (p.ksize & 1) == 0 || !(p.sigma > 0.0) || p.ksize / 2 >= S))
    return false;  // torch reflect padding needs pad < S
  for (int k = 0; k < 4; ++k)
    if (p.order[k] > 3) return false;
  // window of the resampled box: inside it, and an axis that is not resampled has no window
  const int rw = view_rw(p), rh = view_rh(p);
  if (rw < S || rh < S || rw > 65536 || rh > 65536 || p.out_x < 0 || p.out_y < 0) return false;
  if (p.out_x + S > rw || p.out_y + S > rh) return false;
  if (p.crop_w == rw && (rw != S || p.out_x != 0)) return false;
  if (p.crop_h == rh && (rh != S || p.out_y != 0)) return false;
  return true;
}

// k_vsizes: one lane per view: validity and scratch bytes into plan[i] (htmp_off holds
// the size and rcoef_off the offset of the coefficient tables inside it until k_vplan
// places the view), so that the single-workgroup scan only reads packed records.
__global__ void __launch_bounds__(256) k_vsizes(const ImgDesc* __restrict__ desc, const dino_view_params* __restrict__ prm,
                                                int B, int nv, int n_global, int gsize, int lsize, int filter,
                                                ViewPlan* __restrict__ plan) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * nv) return;
  const ImgDesc& d = desc[i / nv];
  const int S = (i % nv) < n_global ? gsize : lsize;
  const int ok = d.status == DINO_IMG_OK && params_valid(prm[i], d, S);
  const dino_view_params& p = prm[i];
  const int32_t kh = ok && p.crop_w != view_rw(p) ? resample_ksize(p.crop_w, view_rw(p), filter) : 0;
  const int32_t kv = ok && p.crop_h != view_rh(p) ? resample_ksize(p.crop_h, view_rh(p), filter) : 0;
  const ViewScratch L = view_scratch(S, p.crop_h, kh, kv);
  ViewPlan vp;
  vp.ok = ok;
  vp.lsum = 0;
  vp.kh = kh;
  vp.kv = kv;
  vp.htmp_off = ok ? L.total : 0;  // 0: the view is not rendered
  vp.rcoef_off = L.hb;
  // (a vertical-first view is resampled by k_rcoeffs: no k_hresize items)
  const bool vfirst = ok && resample_vfirst(p.crop_w, p.crop_h, view_rh(p), kh);
  vp.hr_chunks = ok && kh && !vfirst ? hr_view_chunks(S, p.crop_w, p.crop_h, kh) : 0;
  vp.hr_base = 0;
  plan[i] = vp;
}

// Per-view scratch offsets and k_hresize work-item bases from k_vsizes' records
// (scan_and_place).  A view that cannot be placed is not rendered and its image is marked
// DINO_IMG_NO_SPACE (reported by dino_batch_info; the host sizes the workspace with
// dino_probe + dino_reserve so that this does not happen on the product path).
struct ViewSum {
  int64_t bytes;
  int32_t hg, hl;  // k_hresize work items of the global / local views
  __device__ ViewSum operator+(const ViewSum& o) const { return {bytes + o.bytes, hg + o.hg, hl + o.hl}; }
};

__global__ void __launch_bounds__(1024) k_vplan(ImgDesc* __restrict__ desc, const dino_view_params* __restrict__ prm,
                                                int B, int nv, int n_global, int gsize, int lsize, int64_t aws_size,
                                                ViewPlan* __restrict__ plan) {
  const int t = threadIdx.x, N = B * nv;
  for (int b = t; b < B; b += 1024) desc[b].aug_status = 0;
  if (t == 0) plan[N] = ViewPlan{};  // k_hresize's work-item counters (global, local views): hr_chunks, hr_base
  scan_and_place<ViewSum>(
      N, aws_size,
      [&](int i) {  // k_vsizes: htmp_off holds the view's scratch bytes until it is placed
        const int32_t c = plan[i].hr_chunks;
        const bool g = (i % nv) < n_global;
        return ViewSum{plan[i].htmp_off, g ? c : 0, g ? 0 : c};
      },
      [&](int i, const ViewSum&, const ViewSum& base, bool placed) {
        ViewPlan vp = plan[i];
        vp.ok = vp.ok && placed;
        vp.htmp_off = base.bytes;
        vp.rcoef_off += base.bytes;
        vp.hr_base = (i % nv) < n_global ? base.hg : base.hl;
        plan[i] = vp;
      },
      [&](int i) { desc[i / nv].aug_status = DINO_IMG_NO_SPACE; });
}

__global__ void __launch_bounds__(256) k_rcoeffs(const ImgDesc* __restrict__ desc, const dino_view_params* __restrict__ prm,
                                                 const ViewPlan* __restrict__ plan, int nv, int v0, int filter,
                                                 const uint8_t* __restrict__ ws, uint8_t* __restrict__ aws) {
  const int i = blockIdx.y * nv + v0 + blockIdx.x;
  const ViewPlan vp = plan[i];
  if (!vp.ok) return;
  const dino_view_params p = prm[i];
  const int S = p.out_size;
  const ViewTables<uint8_t*> T = view_tables(aws + vp.rcoef_off, S, vp.kh, vp.kv);
  int32_t *hb = (int32_t*)T.hb, *vb = (int32_t*)T.vb, *ht = (int32_t*)T.ht, *vt = (int32_t*)T.vt;
  int4* hx = (int4*)T.hx;
  uint4* hg = (uint4*)T.hg;
  for (int x = threadIdx.x; x < S; x += blockDim.x) {
    if (vp.kh) {
      int32_t* k = ht + (int64_t)x * vp.kh;
      resample_coeffs_one(p.crop_w, view_rw(p), p.out_x + x, vp.kh, &hb[2 * x], &hb[2 * x + 1], k, filter);
      // sum_t p_t k_t = sum_t (p_t - 128) k_t + 128 sum_t k_t, and k_t = D0 + 256 D1 + 65536 D2
      // with signed digits D in [-128, 127] (exact for -2^23 - 2^15 <= k < 2^23 - 2^15 = 1.992 x
      // 2^22; the largest tap of any filter is LANCZOS's 1.2851 x 2^22, resize.hpp tap_mad): three
      // v_dot4 products per 4 taps
      const int cnt = hb[2 * x + 1], ng = (cnt + 3) / 4;
      int32_t ksum = 0;
      for (int g = 0; g < ng; ++g) {
        uint32_t dp[3] = {0u, 0u, 0u};
        for (int j = 0; j < 4; ++j) {
          const int t = 4 * g + j;
          const int32_t kt = t < cnt ? k[t] : 0;
          ksum += kt;
          const int32_t d0 = (int32_t)(int8_t)(uint8_t)(kt & 0xFF);
          const int32_t r1 = (kt - d0) >> 8;
          const int32_t d1 = (int32_t)(int8_t)(uint8_t)(r1 & 0xFF);
          const int32_t d2 = (r1 - d1) >> 8;
          dp[0] |= (uint32_t)(uint8_t)d0 << (8 * j);
          dp[1] |= (uint32_t)(uint8_t)d1 << (8 * j);
          dp[2] |= (uint32_t)(uint8_t)d2 << (8 * j);
        }
        hg[(int64_t)g * S + x] = make_uint4(dp[0], dp[1], dp[2], 0u);
      }
      // k_hresize runs the view's ng_max groups for every output: zero taps past this one's
      for (int g = ng; g < (vp.kh + 3) / 4; ++g) hg[(int64_t)g * S + x] = make_uint4(0u, 0u, 0u, 0u);
      hx[x] = make_int4(hb[2 * x], ng, 128 * ksum + (1 << (kPrecisionBits - 1)), 0);
    }
    if (vp.kv)
      resample_coeffs_one(p.crop_h, view_rh(p), p.out_y + x, vp.kv, &vb[2 * x], &vb[2 * x + 1], vt + (int64_t)x * vp.kv,
                          filter);
  }
  if (!resample_vfirst(p.crop_w, p.crop_h, view_rh(p), vp.kh)) return;
  // Vertical pass first (resample_vfirst: a crop over 100 times as high as wide, which no
  // RandomResizedCrop draws; Pillow rounds its 8-bit intermediate in this order).  This
  // workgroup resamples the whole view, an output row at a time: the row's vertical pass over
  // the crop's columns into LDS, then its horizontal pass into row y of the temp planes,
  // where k_hresize (which has no items of this view) would have put crop row y.  The
  // vertical tables then become the identity on those rows, so that k_vert / k_vfinal copy.
  __shared__ uint8_t s_row[3 * kVFirstMaxW];
  const ImgDesc& d = desc[blockIdx.y];
  const int cw = p.crop_w;
  const int64_t spitch = (int64_t)d.width * 3, cpl = (int64_t)p.crop_h * S;
  const uint8_t* src = ws + d.rgb_off + (int64_t)p.crop_top * spitch + (int64_t)p.crop_left * 3;
  uint8_t* tmp = aws + vp.htmp_off;
  __syncthreads();  // the tables above
  for (int y = 0; y < S; ++y) {
    const int ymin = vb[2 * y], ycnt = vb[2 * y + 1];
    const int32_t* kv = vt + (int64_t)y * vp.kv;
    for (int e = threadIdx.x; e < 3 * cw; e += blockDim.x) {
      const uint8_t* q = src + (int64_t)ymin * spitch + e;
      int32_t acc = 1 << (kPrecisionBits - 1);
      for (int t = 0; t < ycnt; ++t) acc = tap_mad(q[(int64_t)t * spitch], kv[t], acc);
      s_row[e] = clip8_acc(acc);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 3 * S; e += blockDim.x) {
      const int c = e / S, x = e - c * S;
      const int xmin = hb[2 * x], xcnt = hb[2 * x + 1];
      const int32_t* kk = ht + (int64_t)x * vp.kh;
      int32_t acc = 1 << (kPrecisionBits - 1);
      for (int t = 0; t < xcnt; ++t) acc = tap_mad(s_row[3 * (xmin + t) + c], kk[t], acc);
      tmp[c * cpl + (int64_t)y * S + x] = clip8_acc(acc);
    }
    __syncthreads();
  }
  for (int y = threadIdx.x; y < S; y += blockDim.x) {
    vb[2 * y] = y;
    vb[2 * y + 1] = 1;
    vt[(int64_t)y * vp.kv] = 1 << kPrecisionBits;
  }
}
