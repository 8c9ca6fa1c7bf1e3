// kernels_launch.inc — part of kernels.hip's translation unit (not compiled on its own).
// Host code, and k_pixel_ops beside its launcher.  Needs every kernel it launches and, with them,
// their block sizes, grids and LDS sizes: kDestuffThreads, kHuff2Threads, kHuffLdsBytes,
// kHuff3LdsBytes, kPWalkThreads, kPScanThreads, kPLscanLds, kPApplyWgs, kDcScanThreads, kIdctWgs,
// kColorWgs, vert_rows, final_rows, final_tile_bytes, FinalLds, kVFinalMaxS, kVFinalThreads,
// kVfStripBytes, vfinal_strip_off (kernels.hip); kMaskLdsMaxPatches (kernels_small.inc);
// kPngWalkThreads (kernels_png.inc); g_sync_check (kernels_timer.inc); in DINO_HUFF_PHASES
// builds g_huff_phase and kPhaseItems (kernels.hip).
static const char* const kKernelNames[kKNumKernels] = {"k_parse", "k_plan", "k_destuff", "k_huff1", "k_idct",
                                                       "k_color", "k_params", "k_vplan", "k_rcoeffs", "k_hresize",
                                                       "k_final_global", "k_final_local", "k_vert_global",
                                                       "k_vert_local", "k_dcscan", "k_htab", "k_hseg", "k_huff2",
                                                       "k_huff3", "k_prog", "k_pwalk", "k_plscan",
                                                       "k_papply", "k_png"};
const char* g_failed_kernel = "";

#define TIMED(tm, kid, s, launch)                          \
  do {                                                     \
    if (tm) (tm)->begin(kid, s);                           \
    launch;                                                \
    if (tm) (tm)->end(s);                                  \
    if (g_sync_check) {                                    \
      hipError_t se_ = hipStreamSynchronize(s);            \
      if (se_ == hipSuccess) se_ = hipGetLastError();      \
      if (se_ != hipSuccess) {                             \
        g_failed_kernel = kKernelNames[kid];               \
        fprintf(stderr, "[dino] %s failed: %s\n", kKernelNames[kid], hipGetErrorString(se_)); \
        return se_;                                        \
      }                                                    \
    }                                                      \
  } while (0)

// Persistent grids of the segment kernels: as many workgroups as can be resident
// on the device at once (occupancy query x CUs); items beyond them come in later turns.
static int persistent_grid(const void* fn, int lds, int cus) {
  int per = 4;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, fn, kHuffThreads, lds) != hipSuccess || per < 1) per = 4;
  return per * cus;
}

// Per-device launch geometry (called by dino_ctx_create with `device` current).
hipError_t init_launch_geom(int device, LaunchGeom* g) {
  int cus = 256;
  hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  if (e != hipSuccess) return e;
  if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_huff1), hipFuncAttributeMaxDynamicSharedMemorySize,
                               kHuffLdsBytes)) != hipSuccess)
    return e;
  if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_huff3), hipFuncAttributeMaxDynamicSharedMemorySize,
                               kHuff3LdsBytes)) != hipSuccess)
    return e;
  g->grid_ds = 4 * cus;
  g->grid3 = persistent_grid(reinterpret_cast<const void*>(&k_huff3), kHuff3LdsBytes, cus);
  g->grid1 = persistent_grid(reinterpret_cast<const void*>(&k_huff1), kHuffLdsBytes, cus);
  if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_hresize), hipFuncAttributeMaxDynamicSharedMemorySize,
                               kHresizeLds)) != hipSuccess)
    return e;
  g->grid_hr = persistent_grid(reinterpret_cast<const void*>(&k_hresize), kHresizeLds, cus);
  // k_vfinal's tile and strip pass 64 KiB above S = 100
  const int vf_lds = vfinal_strip_off<float>(kVFinalMaxS) + kVfStripBytes;
  if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_vfinal<uint16_t>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               vf_lds)) != hipSuccess ||
      (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_vfinal<float>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               vf_lds)) != hipSuccess ||
      (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_vfinal<uint8_t>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               vf_lds)) != hipSuccess)
    return e;
  // views up to this size take k_vfinal, larger ones k_vert + k_final (DINO_VFINAL_MAX_S: 0 sends
  // every view through the two kernels, for parity tests and A/B runs)
  const char* vm = getenv("DINO_VFINAL_MAX_S");
  g->vfinal_max_s = vm ? min(max(atoi(vm), 0), kVFinalMaxS) : kVFinalMaxS;
  if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_plscan), hipFuncAttributeMaxDynamicSharedMemorySize,
                               kPLscanLds)) != hipSuccess)
    return e;
  // scan waves: one per CU by default.  A scan's serial decode runs on the CU's one scalar
  // unit, which the CU's waves share: two scan waves on a CU each run at about half speed
  // (DINO_PSCAN_PER_CU: waves per CU, measured in profiles/r03_prog_*).
  const char* pc = getenv("DINO_PSCAN_PER_CU");
  const int per_cu = pc && atoi(pc) > 0 ? atoi(pc) : 1;
  g->grid_ps = per_cu * cus;
  // lane scan waves: one ticket each (a 512-image pool of libjpeg-default files: 80); the rest exit
  const char* ls = getenv("DINO_PLSCAN_WAVES");
  g->grid_ls = ls && atoi(ls) > 0 ? atoi(ls) : 2 * cus;
  // the scan waves' issue priority: 0 below the batch kernels (s_setprio 3, main_prio), 1 level
  const char* sp = getenv("DINO_SCAN_PRIO");
  g->scan_prio = sp ? atoi(sp) : 0;
  // inflate waves (PNG): four per CU fit its LDS (kInfLdsBytes each); DINO_INFLATE_WAVES sets the grid
  const char* iw = getenv("DINO_INFLATE_WAVES");
  g->grid_inf = iw && atoi(iw) > 0 ? atoi(iw) : 4 * cus;
  // the lane decoder is opt-in (DINO_PROG_LANE=1): its throughput is higher but a scan's latency
  // is ~3x a scan wave's, more than the side route's look-ahead covers (DESIGN.md §5)
  const char* pl = getenv("DINO_PROG_LANE");
  g->prog_lane = pl ? (atoi(pl) != 0) : 0;
  return hipSuccess;
}

hipError_t launch_decode(const DecodeArgs& a, hipStream_t s, KernelTimer* tm) {
  const int B = a.batch;
  if (B <= 0) return hipSuccess;
  TIMED(tm, kKParse, s, (k_parse<<<B, 64, 0, s>>>(a.bytes, a.offsets, a.lengths, a.raw_mask, B, a.max_dim, a.four_component,
                                                  a.desc)));
  // a context with dino_ctx_set_png on: PNG files get their descriptor before the plan
  if (a.png) TIMED(tm, kKPng, s, (k_pnghead<<<(B + 63) / 64, 64, 0, s>>>(a.bytes, a.offsets, a.lengths, a.raw_mask, B, a.max_dim, a.desc)));
  // (k_plan<true> also sizes kind-4 images; without the option there is none and k_plan<false> is the code it was)
  if (a.png) TIMED(tm, kKPlan, s, (k_plan<true><<<1, 1024, 0, s>>>(a.desc, B, a.ws_size, a.pctl)));
  else TIMED(tm, kKPlan, s, (k_plan<false><<<1, 1024, 0, s>>>(a.desc, B, a.ws_size, a.pctl)));
  const int grid_ds = a.geom.grid_ds, grid1 = a.geom.grid1, grid3 = a.geom.grid3;
  TIMED(tm, kKDestuff, s, (k_destuff_count<<<grid_ds, kDestuffThreads, 0, s>>>(a.bytes, a.offsets, B, a.desc, a.ws)));
  TIMED(tm, kKDestuff, s, (k_destuff_write<<<grid_ds, kDestuffThreads, 0, s>>>(a.bytes, a.offsets, B, a.desc, a.ws)));
  TIMED(tm, kKHtab, s, (k_htab<<<B, kHuffThreads, 0, s>>>(a.bytes, a.offsets, a.desc, a.ws)));
  // after k_htab's kind switch
  TIMED(tm, kKPwalk, s, (k_pwalk<<<B, kPWalkThreads, 0, s>>>(a.bytes, a.offsets, a.lengths, a.desc, a.ws, a.pctl,
                                                               a.geom.prog_lane)));
  TIMED(tm, kKProg, s, (k_pscan<<<a.geom.grid_ps, kPScanThreads, 0, s>>>(a.bytes, a.offsets, a.lengths, a.desc, a.ws, a.pctl,
                                                                             a.geom.scan_prio)));
  if (a.geom.prog_lane) {  // the lane decoder (opt-in): k_pwalk registers no lane image otherwise
    TIMED(tm, kKPlscan, s, (k_plscan<<<a.geom.grid_ls, 64, kPLscanLds, s>>>(a.desc, a.ws, a.pctl, a.geom.scan_prio)));
    TIMED(tm, kKPapply, s, (k_papply<<<dim3(kPApplyWgs, B), 256, 0, s>>>(a.desc, a.ws, a.pctl)));
  }
  TIMED(tm, kKHseg, s, (k_hseg<<<1, 1024, 0, s>>>(a.desc, B)));
  TIMED(tm, kKHuff1, s, (k_huff1<<<grid1, kHuffThreads, kHuffLdsBytes, s>>>(a.desc, B, a.ws)));
  TIMED(tm, kKHuff2, s, (k_huff2<<<B, kHuff2Threads, 0, s>>>(a.desc, a.ws)));
  TIMED(tm, kKHuff3, s, (k_huff3<<<grid3, kHuffThreads, kHuff3LdsBytes, s>>>(a.desc, B, a.ws)));
  TIMED(tm, kKDcscan, s, (k_dcscan<<<B, kDcScanThreads, 0, s>>>(a.desc, a.ws)));
  TIMED(tm, kKIdct, s, (k_idct<<<dim3(kIdctWgs, B), 256, 0, s>>>(a.desc, a.ws)));
  if (a.four_component) TIMED(tm, kKIdct, s, (k_idct4<<<dim3(kIdctWgs, B), 256, 0, s>>>(a.desc, a.ws)));
  TIMED(tm, kKColor, s, (k_color<<<dim3(kColorWgs, B), 256, 0, s>>>(a.bytes, a.offsets, a.desc, a.ws)));
  if (a.four_component) TIMED(tm, kKColor, s, (k_color4<<<dim3(kColorWgs, B), 256, 0, s>>>(a.desc, a.ws)));
  if (a.png) {  // PNG images (kind 4): no other context has one
    TIMED(tm, kKPng, s, (k_pngwalk<<<B, kPngWalkThreads, 0, s>>>(a.bytes, a.offsets, a.lengths, a.desc, a.ws, a.pctl)));
    TIMED(tm, kKPng, s, (k_inflate<<<min(B, a.geom.grid_inf), 64, 0, s>>>(a.desc, a.ws, a.pctl, B)));
    TIMED(tm, kKPng, s, (k_unfilter<<<B, 64, 0, s>>>(a.desc, a.ws)));
  }
  return hipGetLastError();
}

hipError_t launch_params(const ImgDesc* desc, int batch, const dino_aug_config& cfg, uint64_t seed,
                         uint64_t batch_index, dino_view_params* out, hipStream_t s, KernelTimer* tm) {
  const int n = batch * (cfg.n_global + cfg.n_local);
  if (n <= 0) return hipSuccess;
  TIMED(tm, kKParams, s, (k_params<<<(n + 63) / 64, 64, 0, s>>>(desc, batch, cfg, seed, batch_index, out)));
  return hipGetLastError();
}

template <typename OutT>
static hipError_t launch_augment_class(const AugmentArgs& a, int v0, int nvc, int S, hipStream_t s, KernelTimer* tm) {
  const int B = a.batch, nv = a.cfg.n_global + a.cfg.n_local;
  if (nvc <= 0) return hipSuccess;
  const int kfin = v0 == 0 ? kKFinalGlobal : kKFinalLocal;
  const int kvert = v0 == 0 ? kKVertGlobal : kKVertLocal;
  const int rc_threads = S < 256 ? (S + 63) / 64 * 64 : 256;  // one lane per output column
  TIMED(tm, kKRcoeffs, s, (k_rcoeffs<<<dim3(nvc, B), rc_threads, 0, s>>>(a.desc, a.params, a.plan, nv, v0, a.filter, a.ws, a.aws)));
  TIMED(tm, kKHresize, s,
        (k_hresize<<<a.grid_hr, 256, kHresizeLds, s>>>(a.desc, a.params, a.plan, nv, v0, nvc, B, a.ws, a.aws)));
  if (S <= a.vfinal_max_s) {  // small views: vertical pass and epilogue fused, the view stays in LDS
    const int lds = vfinal_strip_off<OutT>(S) + kVfStripBytes;
    TIMED(tm, kfin, s,
          (k_vfinal<OutT><<<dim3(nvc, B), kVFinalThreads, lds, s>>>(a.desc, a.params, a.plan, nv, v0, a.ws, a.aws, a.views, a.cfg,
                                                         S, a.norm)));
    return hipGetLastError();
  }
  TIMED(tm, kvert, s,
        (k_vert<<<dim3((S + vert_rows(S) - 1) / vert_rows(S), nvc, B), 256, 0, s>>>(a.desc, a.params, a.plan, nv, v0, B,
                                                                             a.ws, a.aws, a.gcrop, a.cfg, S)));
  const int lds = (int)sizeof(FinalLds) + final_tile_bytes(S) + 3 * 256 * (int)sizeof(OutT);
  TIMED(tm, kfin, s,
        (k_final<OutT><<<dim3((S + final_rows(S) - 1) / final_rows(S), nvc, B), 256, lds, s>>>(
            a.desc, a.params, a.plan, nv, v0, B, a.gcrop, a.views, a.cfg, S, a.norm)));
  return hipGetLastError();
}

template <typename OutT>
static hipError_t launch_augment_t(const AugmentArgs& a, hipStream_t s, KernelTimer* tm) {
  hipError_t e = launch_augment_class<OutT>(a, 0, a.cfg.n_global, a.cfg.global_size, s, tm);
  if (e != hipSuccess) return e;
  return launch_augment_class<OutT>(a, a.cfg.n_global, a.cfg.n_local, a.cfg.local_size, s, tm);
}

hipError_t launch_augment(const AugmentArgs& a, hipStream_t s, KernelTimer* tm) {
  const int B = a.batch, nv = a.cfg.n_global + a.cfg.n_local;
  if (B <= 0 || nv <= 0) return hipSuccess;
  TIMED(tm, kKVplan, s, (k_vsizes<<<(B * nv + 255) / 256, 256, 0, s>>>(a.desc, a.params, B, nv, a.cfg.n_global,
                                                                       a.cfg.global_size, a.cfg.local_size, a.filter, a.plan)));
  TIMED(tm, kKVplan, s, (k_vplan<<<1, 1024, 0, s>>>(a.desc, a.params, B, nv, a.cfg.n_global, a.cfg.global_size,
                                                     a.cfg.local_size, a.aws_size, a.plan)));
  switch (a.cfg.out_dtype) {
    case DINO_OUT_FP32:
      return launch_augment_t<float>(a, s, tm);
    case DINO_OUT_FP8_E4M3:
      return launch_augment_t<uint8_t>(a, s, tm);
    default:
      return launch_augment_t<uint16_t>(a, s, tm);
  }
}

hipError_t launch_info(const ImgDesc* desc, int batch, int32_t* info, hipStream_t s) {
  if (batch <= 0) return hipSuccess;
  k_info<<<(batch + 63) / 64, 64, 0, s>>>(desc, batch, info);
  return hipGetLastError();
}

// The per-pixel colour operators over all 2^24 inputs (index = a << 16 | b << 8 | c):
// op 0 RGB -> HSV, op 1 HSV -> RGB, op 2 hue_shift by `param` (the ColorJitter hue op);
// out[3 * index + k].  For the exhaustive device-side checks against Pillow.
__global__ void __launch_bounds__(256) k_pixel_ops(int op, int param, uint8_t* __restrict__ out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  int x = (idx >> 16) & 255, y = (idx >> 8) & 255, z = idx & 255;
  if (op == 0) {
    int h, sv, v;
    rgb_to_hsv(x, y, z, &h, &sv, &v);
    x = h, y = sv, z = v;
  } else if (op == 1) {
    hsv_to_rgb(x, y, z, &x, &y, &z);
  } else {
    hue_shift(x, y, z, param);
  }
  out[3 * (int64_t)idx] = (uint8_t)x;
  out[3 * (int64_t)idx + 1] = (uint8_t)y;
  out[3 * (int64_t)idx + 2] = (uint8_t)z;
}

hipError_t launch_pixel_ops(int op, int param, uint8_t* out, hipStream_t s) {
  k_pixel_ops<<<(1 << 24) / 256, 256, 0, s>>>(op, param, out);
  return hipGetLastError();
}

hipError_t launch_copy_rgb(const ImgDesc* desc, int idx, const uint8_t* ws, uint8_t* dst, hipStream_t s) {
  k_copy_rgb<<<256, 256, 0, s>>>(desc, idx, ws, dst);
  return hipGetLastError();
}

hipError_t launch_copy_rgb_packed(const ImgDesc* desc, int B, int n, const int32_t* idx, const int64_t* off,
                                  const uint8_t* ws, uint8_t* base, int header, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  k_copy_rgb_packed<<<dim3(16, n), 256, 0, s>>>(desc, B, idx, off, ws, base, header);
  return hipGetLastError();
}

hipError_t launch_masks(int H, int W, int target, int minp, int maxp, double la0, double la1, int n, uint32_t* py,
                        uint32_t* np, uint8_t* out, hipStream_t s) {
  MaskParams mp{H, W, target, minp, maxp, la0, la1};
  if ((int64_t)H * W > kMaskLdsMaxPatches) return hipErrorInvalidValue;
  k_masks<<<1, 64, 5 * H * W + 16, s>>>(mp, n, py, np, out);
  return hipGetLastError();
}

#ifdef DINO_HUFF_PHASES
hipError_t copy_huff_phases(uint64_t* host, int64_t n_items) {
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return e;
  const int64_t n = n_items < kPhaseItems ? n_items : kPhaseItems;
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_huff_phase), sizeof(uint64_t) * 5 * n);
}
#endif

hipError_t launch_bf16_to_fp8(const uint16_t* in, uint8_t* out, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  k_bf16_to_fp8<<<(unsigned)blocks, 256, 0, s>>>(in, out, n);
  return hipGetLastError();
}
