// kernels_decode_only.inc — part of kernels.hip's translation unit (not compiled on its own).  Needs scan_and_place and out_cast (kernels.hip).
// ---------------------------------------------------------------------------
// Decode-only recipe (reference CPUUserAugPipeline, cpu.py:484-500; DALI
// _build_decode_only_pipeline, pipeline.py:693-756): every image of the batch
// resampled whole (Pillow BICUBIC or the context's filter, horizontal pass then vertical, each only when
// that axis changes size) to ow x oh, normalised and cast, NCHW.  Scratch per
// image (k_dplan, the ViewPlan slot of view 0): coefficient tables of both axes +
// the horizontal pass's rows (planar u8 [3][H][ow]).
// ---------------------------------------------------------------------------
// The image's scratch layout (zero bytes when it did not decode) and tap counts.
__device__ DecScratch<int64_t> dec_layout(const ImgDesc& d, int ow, int oh, int filter, int32_t* kh, int32_t* kv) {
  const bool ok = d.status == DINO_IMG_OK;
  *kh = ok && d.width != ow ? resample_ksize(d.width, ow, filter) : 0;
  *kv = ok && d.height != oh ? resample_ksize(d.height, oh, filter) : 0;
  return ok ? dec_scratch((int64_t)0, ow, oh, d.height, *kh, *kv) : DecScratch<int64_t>{};
}

struct DecSum {
  int64_t bytes;
  __device__ DecSum operator+(const DecSum& o) const { return {bytes + o.bytes}; }
};

__global__ void __launch_bounds__(1024) k_dplan(ImgDesc* __restrict__ desc, int B, int ow, int oh, int filter,
                                                int64_t aws_size, ViewPlan* __restrict__ plan) {
  for (int b = threadIdx.x; b < B; b += 1024) desc[b].aug_status = 0;
  scan_and_place<DecSum>(
      B, aws_size,
      [&](int i) {
        int32_t kh, kv;
        return DecSum{dec_layout(desc[i], ow, oh, filter, &kh, &kv).total};
      },
      [&](int i, const DecSum&, const DecSum& base, bool placed) {
        ViewPlan vp{};
        const DecScratch<int64_t> L = dec_layout(desc[i], ow, oh, filter, &vp.kh, &vp.kv);
        vp.ok = placed && L.total != 0;
        vp.rcoef_off = base.bytes;
        vp.htmp_off = base.bytes + L.htmp;
        plan[i] = vp;
      },
      [&](int i) { desc[i].aug_status = DINO_IMG_NO_SPACE; });
}

__global__ void __launch_bounds__(256) k_dcoeffs(const ImgDesc* __restrict__ desc, const ViewPlan* __restrict__ plan,
                                                 int ow, int oh, int filter, uint8_t* __restrict__ aws) {
  const int b = blockIdx.x;
  const ViewPlan vp = plan[b];
  if (!vp.ok) return;
  const ImgDesc& d = desc[b];
  const DecScratch<uint8_t*> L = dec_scratch(aws + vp.rcoef_off, ow, oh, d.height, vp.kh, vp.kv);
  int32_t *hb = (int32_t*)L.hb, *ht = (int32_t*)L.ht, *vb = (int32_t*)L.vb, *vt = (int32_t*)L.vt;
  if (vp.kh)
    for (int x = threadIdx.x; x < ow; x += blockDim.x)
      resample_coeffs_one(d.width, ow, x, vp.kh, &hb[2 * x], &hb[2 * x + 1], ht + (int64_t)x * vp.kh, filter);
  if (vp.kv)
    for (int y = threadIdx.x; y < oh; y += blockDim.x)
      resample_coeffs_one(d.height, oh, y, vp.kv, &vb[2 * y], &vb[2 * y + 1], vt + (int64_t)y * vp.kv, filter);
}

__global__ void __launch_bounds__(256) k_dhpass(const ImgDesc* __restrict__ desc, const ViewPlan* __restrict__ plan,
                                                int ow, const uint8_t* __restrict__ ws, uint8_t* __restrict__ aws) {
  const int b = blockIdx.y;
  const ViewPlan vp = plan[b];
  if (!vp.ok || !vp.kh) return;
  const ImgDesc& d = desc[b];
  const DecHTables<const uint8_t*> L = dec_htables((const uint8_t*)aws + vp.rcoef_off, ow);
  const CoefView cv{(const int32_t*)L.hb, (const int32_t*)L.ht, vp.kh};
  const SrcView src{ws + d.rgb_off, (int64_t)d.width * 3, 3, 1};
  uint8_t* tmp = aws + vp.htmp_off;
  const int64_t n = (int64_t)d.height * ow, plane = n;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(e / ow), x = (int)(e - (int64_t)y * ow);
#pragma unroll
    for (int c = 0; c < 3; ++c) tmp[c * plane + e] = hresize_at(src, cv, y, x, c);
  }
}

template <typename OutT>
__global__ void __launch_bounds__(256) k_dvpass(const ImgDesc* __restrict__ desc, const ViewPlan* __restrict__ plan,
                                                int ow, int oh, const uint8_t* __restrict__ ws,
                                                const uint8_t* __restrict__ aws, OutT* __restrict__ out, float m0,
                                                float m1, float m2, float s0, float s1, float s2,
                                                const float* __restrict__ norm) {
  const int b = blockIdx.y;
  const ViewPlan vp = plan[b];
  const ImgDesc& d = desc[b];
  const int64_t n = (int64_t)oh * ow;
  OutT* o = out + (int64_t)b * 3 * n;
  const float* nb = norm ? norm + (int64_t)b * 6 : nullptr;
  const float mean[3] = {nb ? nb[0] : m0, nb ? nb[1] : m1, nb ? nb[2] : m2};
  const float stdv[3] = {nb ? nb[3] : s0, nb ? nb[4] : s1, nb ? nb[5] : s2};
  if (!vp.ok) {  // undecodable (cpu.py:496-497) or not placed: zeros
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < 3 * n; e += (int64_t)gridDim.x * blockDim.x)
      o[e] = (OutT)0;
    return;
  }
  const DecScratch<const uint8_t*> L = dec_scratch(aws + vp.rcoef_off, ow, oh, d.height, vp.kh, vp.kv);
  const CoefView cv{(const int32_t*)L.vb, (const int32_t*)L.vt, vp.kv};
  const SrcView src = vp.kh ? SrcView{aws + vp.htmp_off, (int64_t)ow, 1, (int64_t)d.height * ow}
                            : SrcView{ws + d.rgb_off, (int64_t)d.width * 3, 3, 1};
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(e / ow), x = (int)(e - (int64_t)y * ow);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int v = vp.kv ? vresize_at(src, cv, y, x, c)
                          : src.base[(int64_t)y * src.pitch + (int64_t)x * src.px + c * src.cs];
      o[c * n + e] = out_cast<OutT>(u8_normalize(v, mean[c], stdv[c]));
    }
  }
}

template <typename OutT>
static hipError_t launch_dec_out(const DecodeOnlyArgs& a, hipStream_t s) {
  const int gx = 64;
  k_dvpass<OutT><<<dim3(gx, a.batch), 256, 0, s>>>(a.desc, a.plan, a.ow, a.oh, a.ws, a.aws, (OutT*)a.out, a.mean[0],
                                                   a.mean[1], a.mean[2], a.std[0], a.std[1], a.std[2], a.norm);
  return hipGetLastError();
}

hipError_t launch_decode_only(const DecodeOnlyArgs& a, hipStream_t s) {
  if (a.batch <= 0) return hipSuccess;
  k_dplan<<<1, 1024, 0, s>>>(a.desc, a.batch, a.ow, a.oh, a.filter, a.aws_size, a.plan);
  k_dcoeffs<<<a.batch, 256, 0, s>>>(a.desc, a.plan, a.ow, a.oh, a.filter, a.aws);
  k_dhpass<<<dim3(64, a.batch), 256, 0, s>>>(a.desc, a.plan, a.ow, a.ws, a.aws);
  switch (a.out_dtype) {
    case DINO_OUT_FP32: return launch_dec_out<float>(a, s);
    case DINO_OUT_FP8_E4M3: return launch_dec_out<uint8_t>(a, s);
    default: return launch_dec_out<uint16_t>(a, s);
  }
}
