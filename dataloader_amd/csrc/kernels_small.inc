// kernels_small.inc — part of kernels.hip's translation unit (not compiled on its own).  Needs nothing from earlier fragments.
// ---------------------------------------------------------------------------
// iBOT masks: one lane runs the (inherently sequential) generator; the mask and
// the completion scratch live in LDS (dynamic, 5 bytes per patch), the MT states too.
// ---------------------------------------------------------------------------
constexpr int kMaskLdsMaxPatches = 8192;  // 40 KiB of dynamic LDS (grids up to 90 x 90)

__global__ void k_masks(MaskParams mp, int n, uint32_t* __restrict__ py_state, uint32_t* __restrict__ np_state,
                        uint8_t* __restrict__ out) {
  __shared__ MtState py, np;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int hw = mp.H * mp.W;
  int32_t* scratch = reinterpret_cast<int32_t*>(smem);
  uint8_t* mask = smem + 4 * hw;
  if (threadIdx.x == 0) {
    mt_load(py, py_state);
    mt_load(np, np_state);
  }
  __syncthreads();
  for (int k = 0; k < n; ++k) {
    if (threadIdx.x == 0) gen_mask(mp, py, np, mask, scratch);
    __syncthreads();
    for (int i = threadIdx.x; i < hw; i += blockDim.x) out[(int64_t)k * hw + i] = mask[i];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    mt_store(py, py_state);
    mt_store(np, np_state);
  }
}

__global__ void k_bf16_to_fp8(const uint16_t* __restrict__ in, uint8_t* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = f32_to_fp8e4m3(bf16_to_f32(in[i]));
}

// copy of one decoded image out of the workspace (tests / debug)
__global__ void k_copy_rgb(const ImgDesc* __restrict__ desc, int idx, const uint8_t* __restrict__ ws,
                           uint8_t* __restrict__ dst) {
  const ImgDesc& d = desc[idx];
  if (d.status != DINO_IMG_OK) return;
  const int64_t n = (int64_t)d.width * d.height * 3;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = ws[d.rgb_off + i];
}

// Decoded images -> raw containers (the side decoder): image idx[k]'s RGB to base + off[k]
// (base null: off[k] is the destination's device address), grid (x, n).  16-byte copies when
// source and destination are both 16-byte aligned (the workspace's RGB areas are; the
// containers' data starts 16 bytes into a 16-byte aligned slice), the tail and unaligned
// cases bytewise.  With `header`, the 16 bytes before the data get the container header
// {DINO_RAW_MAGIC, width, height, 0} (little-endian words).
__global__ void k_copy_rgb_packed(const ImgDesc* __restrict__ desc, int B, const int32_t* __restrict__ idx,
                                  const int64_t* __restrict__ off, const uint8_t* __restrict__ ws,
                                  uint8_t* __restrict__ base, int header) {
  const int k = blockIdx.y, i = idx[k];
  if (i < 0 || i >= B) return;
  const ImgDesc& d = desc[i];
  if (d.status != DINO_IMG_OK) return;
  const int64_t n = (int64_t)d.width * d.height * 3;
  const uint8_t* src = ws + d.rgb_off;
  uint8_t* dst = base ? base + off[k] : reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(off[k]));
  if (header && blockIdx.x == 0 && threadIdx.x < 16) {
    const uint32_t w[4] = {DINO_RAW_MAGIC, (uint32_t)d.width, (uint32_t)d.height, 0u};
    const int j = threadIdx.x;
    dst[j - 16] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
  }
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, ts = (int64_t)gridDim.x * blockDim.x;
  int64_t head = 0;
  if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
    const int64_t n16 = n >> 4;
    for (int64_t q = t0; q < n16; q += ts) ((uint4*)dst)[q] = ((const uint4*)src)[q];
    head = n16 << 4;
  }
  for (int64_t q = head + t0; q < n; q += ts) dst[q] = src[q];
}

__global__ void k_info(const ImgDesc* __restrict__ desc, int B, int32_t* __restrict__ info) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const ImgDesc& d = desc[i];
  info[4 * i + 0] = d.status != DINO_IMG_OK ? d.status : d.aug_status;
  info[4 * i + 1] = d.width;
  info[4 * i + 2] = d.height;
  info[4 * i + 3] = d.ncomp;
}
