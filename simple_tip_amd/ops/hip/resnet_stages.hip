// Stage-resident ResNet-20 inference kernels for gfx950: three launches
// run the whole forward (conv device code: resnet_fused_device.h).

#include "resnet_fused_device.h"

// Three kernels run the whole forward; the activation plane stays in LDS
// from block to block and only each stage's final plane goes to HBM.
// One image per workgroup of 256 threads, as in the per-block kernels.
//
// In-place residual: conv2 of a block reads its A operand from the
// intermediate image only, and reads the residual at exactly the element it
// then writes, so the block output overwrites the block input and one X/H
// image pair serves a whole stage. For a down block the projected shortcut
// image is the residual and takes the output.
//
// Zero-once halos: every epilogue writes interiors only, so an image's halo
// is zeroed once per geometry per workgroup (zero_halo), not before every
// conv, and again only when a region is reused under another geometry.

struct ResW {
  const short* w1; const float* b1;
  const short* w2; const float* b2;
};
struct DownW {
  const short* w1; const float* b1;
  const short* w2; const float* b2;
  const short* wsc; const float* bsc;
};
struct Stage1Args {
  const short* stem_w; const float* stem_b;
  ResW res[3];
  DownW down;
};
struct Stage2Args {
  ResW res[2];
  DownW down;
};
struct Stage3Args {
  ResW res[2];
  const float* fc_w;  // [10, 64] row-major
  const float* fc_b;  // [10]
};

// Zero the 1-pixel halo ring of an LDS image; the interior is not touched,
// so this needs no barrier against writers of the interior.
template <int H, int W, int C>
TIP_DEV void zero_halo(short* lds) {
  using L = Img<H, W, C>;
  constexpr int RING = 2 * (W + 2) + 2 * H;  // halo pixels
  const short8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < RING * L::UPP; i += blockDim.x) {
    const int hp = i / L::UPP;
    const int h = i - hp * L::UPP;
    int y, x;
    if (hp < 2 * (W + 2)) {          // top and bottom rows
      const int bottom = hp >= W + 2;
      y = bottom ? H + 1 : 0;
      x = hp - bottom * (W + 2);
    } else {                         // left and right columns of rows 1..H
      const int k = hp - 2 * (W + 2);
      y = 1 + (k >> 1);
      x = (k & 1) ? W + 1 : 0;
    }
    lds_write_unit(lds, L::unit(y, x, h), zero);
  }
}

// Copy the interior of an LDS image to a contiguous NHWC plane in global
// memory, one 16-byte store per unit. The caller barriers first.
template <int H, int W, int C>
TIP_DEV void store_interior(const short* lds, short* __restrict__ gdst) {
  using L = Img<H, W, C>;
  constexpr int UNITS = H * W * C / 8;
  constexpr int UPP = C / 8;
  for (int u = threadIdx.x; u < UNITS; u += blockDim.x) {
    const int p = u / UPP;
    const int h = u - p * UPP;
    const int y = p / W, x = p - y * W;
    *reinterpret_cast<short8*>(gdst + (int64_t)u * 8) =
        lds_read_unit(lds, L::unit(y + 1, x + 1, h));
  }
}

// fp32 -> bf16, round to nearest even, NaN -> 0x7FC0: the bits of
// tensor.to(torch.bfloat16).
TIP_DEV short f32_to_bf16_bits(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (short)0x7fc0;
  u += 0x7fffu + ((u >> 16) & 1u);
  return (short)(u >> 16);
}

// Stage one contiguous fp32 [32, 32, 3] image into the interior of an
// 8-channel LDS image (channels 3..7 zero). Each thread converts 4
// consecutive pixels of one row from three 16-byte loads (gsrc must be
// 16-byte aligned).
TIP_DEV void stage_input_f32(short* lds, const float* __restrict__ gsrc) {
  using L = Img<32, 32, 8>;
  for (int t = threadIdx.x; t < 32 * 32 / 4; t += blockDim.x) {
    const float4* g4 = reinterpret_cast<const float4*>(gsrc) + 3 * t;
    const float4 v0 = g4[0], v1 = g4[1], v2 = g4[2];
    const float f[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y,
                         v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
    const int p0 = 4 * t;
    const int y = p0 >> 5, x = p0 & 31;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const short8 v = {f32_to_bf16_bits(f[3 * q]),
                        f32_to_bf16_bits(f[3 * q + 1]),
                        f32_to_bf16_bits(f[3 * q + 2]), 0, 0, 0, 0, 0};
      lds_write_unit(lds, L::unit(y + 1, x + q + 1, 0), v);
    }
  }
}

// Equal-channel residual block on LDS images, output in place of the input:
// X -> conv1+relu -> Hb -> conv2+bias+X+relu -> X. Both halos are zero on
// entry and stay zero. Ends on a barrier.
template <int H, int W, int C>
TIP_DEV void res_block_lds(short* X, short* Hb, const ResW& p) {
  conv3x3<H, W, C, C, true, false, 1>(X, Hb, nullptr, nullptr, p.w1, p.b1);
  __syncthreads();
  conv3x3<H, W, C, C, true, true, 1, true>(
      Hb, X, nullptr, nullptr, p.w2, p.b2);
  __syncthreads();
}

// Downsample block on LDS images: X [H,W,C] -> R [H/2,W/2,2C]. Hb and R are
// regions no wave still reads (the caller has barriered); they get a new
// geometry here, so their halos are zeroed again. The projected shortcut is
// written to R, and conv2 adds it in place. Ends on a barrier.
template <int H, int W, int C>
TIP_DEV void down_block_lds(const short* X, short* Hb, short* R,
                            const DownW& p) {
  constexpr int OH = H / 2, OW = W / 2, C2 = 2 * C;
  zero_halo<OH, OW, C2>(Hb);
  zero_halo<OH, OW, C2>(R);
  conv3x3<H, W, C, C2, true, false, 2>(X, Hb, nullptr, nullptr, p.w1, p.b1);
  shortcut1x1_s2<H, W, C, C2>(X, R, p.wsc, p.bsc);
  __syncthreads();
  conv3x3<OH, OW, C2, C2, true, true, 1, true>(
      Hb, R, nullptr, nullptr, p.w2, p.b2);
  __syncthreads();
}

// LDS budgets (bytes): the X image of the stage plus a second region that
// holds the H image during the res blocks and the two half-size images of
// the down block afterwards.
constexpr int kStage1Lds =
    (Img<32, 32, 16>::UNITS + 2 * Img<16, 16, 32>::UNITS) * 16;  // 78464
constexpr int kStage2Lds =
    (Img<16, 16, 32>::UNITS + 2 * Img<8, 8, 64>::UNITS) * 16;    // 46912
constexpr int kStage3Lds = 2 * Img<8, 8, 64>::UNITS * 16;        // 26176
static_assert(2 * Img<16, 16, 32>::UNITS >= Img<32, 32, 16>::UNITS &&
              2 * Img<8, 8, 64>::UNITS >= Img<16, 16, 32>::UNITS,
              "second region must hold the stage's H image");
static_assert(3 * kStage2Lds <= 160 * 1024 && 4 * kStage3Lds <= 160 * 1024,
              "the padded 8x8x64 image must not cost a workgroup per CU");

// Stage 1: fp32 input -> bf16, stem, 3 x res<32,32,16>, down<32,32,16>.
// The 8-channel input image lives in the second region until the stem has
// read it.
__launch_bounds__(256) __global__ void stage1_kernel(
    const float* __restrict__ gin,   // [B, 32*32*3] fp32 NHWC
    short* __restrict__ gout,        // [B, 16*16*32]
    const Stage1Args a) {
  extern __shared__ short lds[];
  short* X = lds;                                  // Img<32,32,16>
  short* Hb = X + Img<32, 32, 16>::UNITS * 8;      // Img<32,32,16> | 2 halves
  short* R = Hb + Img<16, 16, 32>::UNITS * 8;      // Img<16,16,32>
  zero_halo<32, 32, 16>(X);
  zero_halo<32, 32, 8>(Hb);
  stage_input_f32(Hb, gin + (int64_t)blockIdx.x * 32 * 32 * 3);
  __syncthreads();
  conv3x3<32, 32, 8, 16, true, false, 1>(
      Hb, X, nullptr, nullptr, a.stem_w, a.stem_b);
  __syncthreads();
  zero_halo<32, 32, 16>(Hb);  // new geometry; conv1 writes the interior
#pragma unroll 1
  for (int i = 0; i < 3; ++i) res_block_lds<32, 32, 16>(X, Hb, a.res[i]);
  down_block_lds<32, 32, 16>(X, Hb, R, a.down);
  store_interior<16, 16, 32>(R, gout + (int64_t)blockIdx.x * 16 * 16 * 32);
}

// Stage 2: 2 x res<16,16,32>, down<16,16,32>.
__launch_bounds__(256) __global__ void stage2_kernel(
    const short* __restrict__ gin,   // [B, 16*16*32]
    short* __restrict__ gout,        // [B, 8*8*64]
    const Stage2Args a) {
  extern __shared__ short lds[];
  short* X = lds;                                  // Img<16,16,32>
  short* Hb = X + Img<16, 16, 32>::UNITS * 8;      // Img<16,16,32> | 2 halves
  short* R = Hb + Img<8, 8, 64>::UNITS * 8;        // Img<8,8,64>
  zero_halo<16, 16, 32>(X);
  zero_halo<16, 16, 32>(Hb);
  load_interior<16, 16, 32>(X, gin + (int64_t)blockIdx.x * 16 * 16 * 32);
  __syncthreads();
#pragma unroll 1
  for (int i = 0; i < 2; ++i) res_block_lds<16, 16, 32>(X, Hb, a.res[i]);
  down_block_lds<16, 16, 32>(X, Hb, R, a.down);
  store_interior<8, 8, 64>(R, gout + (int64_t)blockIdx.x * 8 * 8 * 64);
}

// Stage 3: 2 x res<8,8,64>, then the head on the plane still in LDS.
// Head order (fixed, so a row's logits do not depend on its batch):
// pooled[c] = (sum over the 64 pixels, ascending, sequential fp32 adds) / 64;
// logits[k] = fma chain over c ascending from 0, then + b[k].
// The register allocator is asked for 4 waves per SIMD (<= 128 registers):
// left alone it takes 134 - 140 and runs at 3, measured 2.4 % slower; 5 or
// more would spill to scratch.
__launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4)))
__global__ void stage3_kernel(
    const short* __restrict__ gin,   // [B, 8*8*64]
    short* __restrict__ gout,        // [B, 8*8*64] — the stage-3 AT tap
    float* __restrict__ logits,      // [B, 10]
    const Stage3Args a) {
  using L = Img<8, 8, 64>;
  extern __shared__ short lds[];
  short* X = lds;
  short* Hb = X + L::UNITS * 8;
  zero_halo<8, 8, 64>(X);
  zero_halo<8, 8, 64>(Hb);
  load_interior<8, 8, 64>(X, gin + (int64_t)blockIdx.x * 8 * 8 * 64);
  __syncthreads();
#pragma unroll 1
  for (int i = 0; i < 2; ++i) res_block_lds<8, 8, 64>(X, Hb, a.res[i]);
  store_interior<8, 8, 64>(X, gout + (int64_t)blockIdx.x * 8 * 8 * 64);
  float* pooled = reinterpret_cast<float*>(Hb);  // Hb is free after conv2
  if (threadIdx.x < 64) {
    const int c = threadIdx.x;
    float s = 0.f;
    for (int p = 0; p < 64; ++p) {
      const short* unit = X + swz(L::unit((p >> 3) + 1, (p & 7) + 1, c >> 3)) * 8;
      s += __bfloat162float(reinterpret_cast<const bf16*>(unit)[c & 7]);
    }
    pooled[c] = s * (1.f / 64.f);
  }
  __syncthreads();
  if (threadIdx.x < 10) {
    const int k = threadIdx.x;
    float acc = 0.f;
    for (int c = 0; c < 64; ++c) acc = fmaf(pooled[c], a.fc_w[k * 64 + c], acc);
    logits[(int64_t)blockIdx.x * 10 + k] = acc + a.fc_b[k];
  }
}

// ---- launchers ----

// Stage launchers. `p` lists the stage's parameter pointers in forward
// order: [stem w, b]; per res block w1, b1, w2, b2; for the down block w1,
// b1, w2, b2, wsc, bsc; [fc w, b].
static ResW res_w(const void* const* p) {
  return ResW{(const short*)p[0], (const float*)p[1], (const short*)p[2],
              (const float*)p[3]};
}

static DownW down_w(const void* const* p) {
  return DownW{(const short*)p[0], (const float*)p[1], (const short*)p[2],
               (const float*)p[3], (const short*)p[4], (const float*)p[5]};
}

void launch_stage1(int batch, const float* gin, short* gout,
                   const void* const* p, hipStream_t s) {
  Stage1Args a;
  a.stem_w = (const short*)p[0];
  a.stem_b = (const float*)p[1];
  for (int i = 0; i < 3; ++i) a.res[i] = res_w(p + 2 + 4 * i);
  a.down = down_w(p + 14);
  hipFuncSetAttribute((const void*)stage1_kernel,
                      hipFuncAttributeMaxDynamicSharedMemorySize, kStage1Lds);
  stage1_kernel<<<batch, 256, kStage1Lds, s>>>(gin, gout, a);
}

void launch_stage2(int batch, const short* gin, short* gout,
                   const void* const* p, hipStream_t s) {
  Stage2Args a;
  for (int i = 0; i < 2; ++i) a.res[i] = res_w(p + 4 * i);
  a.down = down_w(p + 8);
  hipFuncSetAttribute((const void*)stage2_kernel,
                      hipFuncAttributeMaxDynamicSharedMemorySize, kStage2Lds);
  stage2_kernel<<<batch, 256, kStage2Lds, s>>>(gin, gout, a);
}

void launch_stage3(int batch, const short* gin, short* gout, float* logits,
                   const void* const* p, hipStream_t s) {
  Stage3Args a;
  for (int i = 0; i < 2; ++i) a.res[i] = res_w(p + 4 * i);
  a.fc_w = (const float*)p[8];
  a.fc_b = (const float*)p[9];
  hipFuncSetAttribute((const void*)stage3_kernel,
                      hipFuncAttributeMaxDynamicSharedMemorySize, kStage3Lds);
  stage3_kernel<<<batch, 256, kStage3Lds, s>>>(gin, gout, logits, a);
}
