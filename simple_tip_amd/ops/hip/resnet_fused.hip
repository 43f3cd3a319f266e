// Fused ResNet-20 inference kernels for gfx950, one RESIDUAL BLOCK per
// launch (bf16 NHWC, CDNA4 MFMA). Motivation, layout and the conv device
// code: resnet_fused_device.h. The stage-resident kernels that keep the
// plane in LDS across blocks are a translation unit of their own
// (resnet_stages.hip): compiled together with these kernels they change
// the register allocation of resblock_kernel<8,8,64> (110 -> 133 registers,
// 4 -> 3 waves/SIMD).

#include "resnet_fused_device.h"

// ---- kernels ----

// Equal-channel residual block: x -> conv1+relu (LDS) -> conv2+bias+x+relu
// -> global. One image per workgroup.
template <int H, int W, int C>
__launch_bounds__(256) __global__ void resblock_kernel(
    const short* __restrict__ gin,   // [B, H*W*C] NHWC bf16
    short* __restrict__ gout,        // [B, H*W*C]
    const short* __restrict__ w1, const float* __restrict__ b1,
    const short* __restrict__ w2, const float* __restrict__ b2) {
  extern __shared__ short lds[];
  short* bufX = lds;                                // image of Img<H,W,C>
  short* bufH = lds + Img<H, W, C>::UNITS * 8;      // second image
  const int64_t img_off = (int64_t)blockIdx.x * H * W * C;
  stage_plane<H, W, C>(bufX, gin + img_off);
  // zero bufH halo (stage_plane zeroes everything first; emulate)
  {
    const short8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int u = threadIdx.x; u < Img<H, W, C>::UNITS; u += blockDim.x)
      lds_write_unit(bufH, u, zero);
  }
  __syncthreads();
  conv3x3<H, W, C, C, true, false, 1>(bufX, bufH, nullptr, nullptr, w1, b1);
  __syncthreads();
  conv3x3<H, W, C, C, false, true, 1>(
      bufH, nullptr, gout + img_off, bufX, w2, b2);
}

// Downsample block: conv1 (stride 2, C -> 2C) + relu -> conv2 (2C) +
// shortcut(1x1 s2) + relu -> global.
template <int H, int W, int C>
__launch_bounds__(256) __global__ void downblock_kernel(
    const short* __restrict__ gin,   // [B, H*W*C]
    short* __restrict__ gout,        // [B, (H/2)*(W/2)*2C]
    const short* __restrict__ w1, const float* __restrict__ b1,
    const short* __restrict__ w2, const float* __restrict__ b2,
    const short* __restrict__ wsc, const float* __restrict__ bsc) {
  constexpr int OH = H / 2, OW = W / 2, C2 = 2 * C;
  extern __shared__ short lds[];
  short* bufX = lds;                                   // Img<H,W,C>
  short* bufH = bufX + Img<H, W, C>::UNITS * 8;        // Img<OH,OW,C2>
  short* bufR = bufH + Img<OH, OW, C2>::UNITS * 8;     // Img<OH,OW,C2>
  const int64_t in_off = (int64_t)blockIdx.x * H * W * C;
  const int64_t out_off = (int64_t)blockIdx.x * OH * OW * C2;
  stage_plane<H, W, C>(bufX, gin + in_off);
  {
    const short8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int u = threadIdx.x; u < Img<OH, OW, C2>::UNITS; u += blockDim.x) {
      lds_write_unit(bufH, u, zero);
      lds_write_unit(bufR, u, zero);
    }
  }
  __syncthreads();
  conv3x3<H, W, C, C2, true, false, 2>(bufX, bufH, nullptr, nullptr, w1, b1);
  shortcut1x1_s2<H, W, C, C2>(bufX, bufR, wsc, bsc);
  __syncthreads();
  conv3x3<OH, OW, C2, C2, false, true, 1>(
      bufH, nullptr, gout + out_off, bufR, w2, b2);
}

// Stem: conv3x3 Cin=8 (4 real + 4 zero-pad channels; 8 keeps units whole)
// -> 16, relu, to global.
template <int H, int W, int CIN, int COUT>
__launch_bounds__(256) __global__ void stem_kernel(
    const short* __restrict__ gin,   // [B, H*W*CIN]
    short* __restrict__ gout,        // [B, H*W*COUT]
    const short* __restrict__ w, const float* __restrict__ b) {
  extern __shared__ short lds[];
  short* bufX = lds;
  const int64_t in_off = (int64_t)blockIdx.x * H * W * CIN;
  const int64_t out_off = (int64_t)blockIdx.x * H * W * COUT;
  stage_plane<H, W, CIN>(bufX, gin + in_off);
  __syncthreads();
  conv3x3<H, W, CIN, COUT, false, false, 1>(
      bufX, nullptr, gout + out_off, nullptr, w, b);
}

// MFMA layout probe: D = A @ B for A [16, 32], B [32, 16] bf16 (row-major)
// with the exact fragment code paths used above.
__global__ void mfma_probe_kernel(
    const short* __restrict__ A, const short* __restrict__ B,
    float* __restrict__ D) {
  const int lane = lane_id();
  const int j = lane & 15, g = lane >> 4;
  short8 a = *reinterpret_cast<const short8*>(A + (j * 32 + g * 8));
  short8 b;
  for (int e = 0; e < 8; ++e) b[e] = B[(g * 8 + e) * 16 + j];
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
  for (int reg = 0; reg < 4; ++reg) D[(g * 4 + reg) * 16 + j] = acc[reg];
}

// ---- launchers ----

void launch_mfma_probe(const short* a, const short* b, float* d, hipStream_t s) {
  mfma_probe_kernel<<<1, 64, 0, s>>>(a, b, d);
}

template <int H, int W, int C>
static void resblock(int batch, const short* gin, short* gout, const short* w1,
                     const float* b1, const short* w2, const float* b2,
                     hipStream_t s) {
  const int lds_bytes = 2 * Img<H, W, C>::UNITS * 16;
  auto k = resblock_kernel<H, W, C>;
  hipFuncSetAttribute((const void*)k,
                      hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  k<<<batch, 256, lds_bytes, s>>>(gin, gout, w1, b1, w2, b2);
}

void launch_resblock(int variant, int batch, const short* gin, short* gout,
                     const short* w1, const float* b1, const short* w2,
                     const float* b2, hipStream_t s) {
  if (variant == 0) resblock<32, 32, 16>(batch, gin, gout, w1, b1, w2, b2, s);
  else if (variant == 1) resblock<16, 16, 32>(batch, gin, gout, w1, b1, w2, b2, s);
  else resblock<8, 8, 64>(batch, gin, gout, w1, b1, w2, b2, s);
}

template <int H, int W, int C>
static void downblock(int batch, const short* gin, short* gout,
                      const short* w1, const float* b1, const short* w2,
                      const float* b2, const short* wsc, const float* bsc,
                      hipStream_t s) {
  constexpr int OH = H / 2, OW = W / 2, C2 = 2 * C;
  const int lds_bytes =
      (Img<H, W, C>::UNITS + 2 * Img<OH, OW, C2>::UNITS) * 16;
  auto k = downblock_kernel<H, W, C>;
  hipFuncSetAttribute((const void*)k,
                      hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  k<<<batch, 256, lds_bytes, s>>>(gin, gout, w1, b1, w2, b2, wsc, bsc);
}

void launch_downblock(int variant, int batch, const short* gin, short* gout,
                      const short* w1, const float* b1, const short* w2,
                      const float* b2, const short* wsc, const float* bsc,
                      hipStream_t s) {
  if (variant == 0)
    downblock<32, 32, 16>(batch, gin, gout, w1, b1, w2, b2, wsc, bsc, s);
  else
    downblock<16, 16, 32>(batch, gin, gout, w1, b1, w2, b2, wsc, bsc, s);
}

void launch_stem(int batch, const short* gin, short* gout, const short* w,
                 const float* b, hipStream_t s) {
  constexpr int H = 32, W = 32, CIN = 8, COUT = 16;
  const int lds_bytes = Img<H, W, CIN>::UNITS * 16;
  auto k = stem_kernel<H, W, CIN, COUT>;
  hipFuncSetAttribute((const void*)k,
                      hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  k<<<batch, 256, lds_bytes, s>>>(gin, gout, w, b);
}
