// Device code shared by the fused ResNet-20 inference kernels for gfx950
// (bf16 NHWC, CDNA4 MFMA): resnet_fused.hip (one residual block per launch)
// and resnet_stages.hip (one stage per launch).
//
// Motivation (profiles/r01_bench_kernels.md): MIOpen runs the bench's
// AT-extraction forward at ~26 TF effective — per-layer launches, im2col
// staging and BatchNorm inference dominate. These kernels compute one
// RESIDUAL BLOCK per launch: the input plane (with 1-pixel halo) is staged
// into LDS once, conv1 -> relu writes the intermediate plane to LDS only,
// conv2 + bias + residual-add + relu writes the block output to HBM. HBM
// traffic per block = read input + write output; the intermediate never
// leaves the CU.
//
// Layout/geometry:
// - activations: NHWC bf16; LDS image [(H+2) x (W+2) x C] with zeroed halo,
//   in 16-byte units, packed unit-row-major (the XOR swizzle family below
//   lost its sweep and is off), except the 8x8x64 image, whose rows are
//   padded by two units against bank conflicts (see Img).
// - MFMA: v_mfma_f32_16x16x32_bf16. M = 16 consecutive output pixels
//   (row-major in the plane), N = 16 output channels, K = 32 consecutive
//   (tap, channel) pairs of the 3x3xC patch (zero-padded to a multiple
//   of 32). Pixel fragment: lane l holds P[i = l&15][k = (l>>4)*8 + e]
//   (one 16-B LDS read per lane); the weight fragment comes pre-packed on
//   the host into [ksteps][64][8] bf16, lane l holding W[k = (l>>4)*8 + e]
//   [cout = l&15], so each lane reads its 16 B straight from global
//   (L2-resident; weights are <= 73 KB per layer). The A and B lane maps of
//   this instruction are the same (row/col l&15, k = (l>>4)*8 + e), so the
//   weight fragment goes in as the FIRST operand and the pixel fragment as
//   the second: D = W^T P^T, col = lane&15 = pixel, row = (lane>>4)*4 + reg
//   = cout, which gives a lane 4 consecutive couts of one pixel to store.
//   (The layout is verified at runtime by the mfma_probe test kernel, and
//   that the swap changes no fp32 bit by test_gpu_resnet_conv_epilogue.)
// - one workgroup = one image; 4 waves split the plane's 16-pixel tiles
//   (the 8x8x64 planes: 2 cout tiles x 2 pixel tiles per wave).

#pragma once

#include "tip_common.h"

#include <hip/hip_bf16.h>

using bf16 = __hip_bfloat16;
using short8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

// 16-B-unit XOR swizzle family: u ^= ((u>>4) * M) & 15 (injective: only
// bits 0-3 change, driven by bits >= 4). M = 0 (identity, default) won a
// 9-variant hardware sweep by +22% (364 vs ~300 TF on resblock<32,32,16>):
// the ds_read_b128 lane-service groups are non-contiguous, and for this
// access pattern the linear image's residual conflicts cost less than the
// per-access XOR address math (profiles/r01_optimization_ladder.md).
#ifndef TIP_SWZ_M
#define TIP_SWZ_M 0
#endif
TIP_DEV int swz(int u) {
  if (TIP_SWZ_M == 0) return u;
  return u ^ (((u >> 4) * TIP_SWZ_M) & 15);
}

// LDS image layout. Round-1 PMC runs measured residual bank conflicts on
// the per-tap A-fragment gathers (profiles/r01_optimization_ladder.md) and
// sketched a "half-channel plane" layout (C/8 planes of one 16-B unit per
// pixel, making same-row gathers stride-1) as the fix. MEASURED IN ROUND 2
// AND REJECTED: on hardware the half-plane layout RAISES
// SQ_LDS_BANK_CONFLICT 3.2x (1.68e7 -> 5.45e7 per 3-launch probe) and
// costs 8% (382 -> 353 TF on resblock<32,32,16>) — the b128 service
// grouping evidently pairs lanes across k-groups, where the packed
// layout's (tap, half-channel) offsets already land in distinct bank
// groups and the stride-C/8 pixel walk does not collide the way a
// same-row-lanes model predicts. The packed unit-row-major image
// (TIP_HALFPLANE=0) stays the default; the half-plane variant is kept
// compilable for future counter runs.
#ifndef TIP_HALFPLANE
#define TIP_HALFPLANE 0
#endif

// Strides of the 8x8x64 image, in 16-B units (packed: 8 and 80). A pixel
// tile of the 8x8 plane is two rows of 8, and a ds_read_b128 lane group
// holds x = 0..3 of one row and x = 4..7 of the other, for each of two
// k-groups. Packed, the pixel stride (128 B) and the row stride (1280 B = 0
// mod 256) put the 8 lanes of a k-group on two 16-B bank slots: 4-way. A row
// stride of 82 (1312 B) moves the second row to other slots: 2-way, for 288
// bytes per image. Enumerated over every tap, k-step and tile: 864 extra
// LDS cycles per conv packed, 288 at (8, 82), 0 at (10, 112); the last
// costs stage 2 a workgroup per CU and measured no faster in stage 3 once
// the tiles are dealt 2 x 2 (profiles/r14_small_plane_weights.md). Every
// fragment address stays base + compile-time constant: no per-read XOR.
#ifndef TIP_IMG64_PS
#define TIP_IMG64_PS 8
#endif
#ifndef TIP_IMG64_RS
#define TIP_IMG64_RS 82
#endif
// Cout tiles per wave in conv3x3's small-plane path (1, 2 or 4).
#ifndef TIP_SP_NC
#define TIP_SP_NC 2
#endif

template <int H, int W, int C>
struct Img {
  static constexpr int UPP = C / 8;  // 16-B units per pixel
#if TIP_HALFPLANE
  static constexpr int RS1 = W + 2;          // units per halo row per plane
  static constexpr int PLANE = (H + 2) * RS1;
  static constexpr int UNITS = UPP * PLANE;
  static constexpr int XSTEP = 1;            // unit step per +1 output x
  static TIP_DEV int unit(int y, int x, int h) {
    return h * PLANE + y * RS1 + x;
  }
#else
  // The layout is a property of the geometry: padded strides for the
  // 8x8x64 image, packed unit-row-major for every other.
  static constexpr bool PADDED = (H == 8 && W == 8 && C == 64);
  static constexpr int PS = PADDED ? TIP_IMG64_PS : UPP;  // units per pixel step
  static constexpr int RS = PADDED ? TIP_IMG64_RS : (W + 2) * UPP;  // per row
  static_assert(PS >= UPP && RS >= (W + 2) * PS, "strides overlap");
  static constexpr int UNITS = (H + 1) * RS + (W + 2) * PS;
  static constexpr int XSTEP = PS;
  static TIP_DEV int unit(int y, int x, int h) {
    // the packed images keep the expression their code was tuned with: the
    // strided form of the same value compiles stage 1 to 3 % slower code
    if constexpr (!PADDED) return (y * (W + 2) + x) * UPP + h;
    return y * RS + x * PS + h;
  }
#endif
};

// Load a 16-B unit (8 bf16) from the swizzled LDS image.
TIP_DEV short8 lds_read_unit(const short* lds, int u) {
  return *reinterpret_cast<const short8*>(lds + swz(u) * 8);
}

TIP_DEV void lds_write_unit(short* lds, int u, short8 v) {
  *reinterpret_cast<short8*>(lds + swz(u) * 8) = v;
}

// Copy one NHWC plane [H x W x C] from global into the interior of the LDS
// image [(H+2) x (W+2) x C]; the halo is not touched.
template <int H, int W, int C>
TIP_DEV void load_interior(short* lds, const short* __restrict__ gsrc) {
  using L = Img<H, W, C>;
  constexpr int UNITS = H * W * C / 8;
  constexpr int UPP = C / 8;  // units per pixel
  for (int u = threadIdx.x; u < UNITS; u += blockDim.x) {
    const int p = u / UPP;
    const int h = u - p * UPP;
    const int y = p / W, x = p - y * W;
    const int lu = L::unit(y + 1, x + 1, h);
    short8 v = *reinterpret_cast<const short8*>(gsrc + (int64_t)u * 8);
    lds_write_unit(lds, lu, v);
  }
}

// Stage one NHWC plane [H x W x C] from global into the LDS image
// [(H+2) x (W+2) x C] interior; halo is zeroed first. 256 threads.
template <int H, int W, int C>
TIP_DEV void stage_plane(short* lds, const short* __restrict__ gsrc) {
  using L = Img<H, W, C>;
  const short8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int u = threadIdx.x; u < L::UNITS; u += blockDim.x)
    lds_write_unit(lds, u, zero);
  __syncthreads();
  load_interior<H, W, C>(lds, gsrc);
}

// Epilogue helpers. The convs issue the
// MFMA with the WEIGHT fragment as the first operand and the PIXEL fragment
// as the second, so D comes out transposed: lane = pixel l&15, registers =
// couts (l>>4)*4 + reg. A lane then owns 4 consecutive couts of one pixel —
// 8 contiguous bytes of one 16-B unit — and the epilogue is one 8-byte
// residual read, one 16-byte bias load, two packed conversions and one
// 8-byte store.

using f32x2 = __attribute__((ext_vector_type(2))) float;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;

// Two fp32 -> two bf16 in one dword (lo in bits 0-15): a plain vector cast,
// which is the hardware packed convert (round to nearest even, NaN stays
// NaN) — the instruction __float2bfloat16 compiles to, fed two values.
TIP_DEV unsigned pack2_bf16(float lo, float hi) {
  const f32x2 v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}

TIP_DEV uint2 pack4_bf16(const f32x4& v) {
  return uint2{pack2_bf16(v[0], v[1]), pack2_bf16(v[2], v[3])};
}

// acc += four bf16 (8 bytes, lowest address first), exactly.
TIP_DEV void add4_bf16(f32x4& acc, const uint2 r) {
  acc[0] += __uint_as_float(r.x << 16);
  acc[1] += __uint_as_float(r.x & 0xffff0000u);
  acc[2] += __uint_as_float(r.y << 16);
  acc[3] += __uint_as_float(r.y & 0xffff0000u);
}

// Output pixel (row, column) of lane-row j in pixel tile pt: the row of the
// pixel fragment this lane gathers AND the pixel its D registers belong to.
struct TilePix {
  int oy, ox;
};
template <int OW>
TIP_DEV TilePix tile_pix(int pt, int j) {
  const int p = pt * 16 + j;
  const int oy = p / OW;
  return TilePix{oy, p - oy * OW};
}

// 3x3 conv over the LDS image: computes the [16-pixel x 16-cout] tiles
// this wave owns and applies bias (+ optional residual from rlds) + relu,
// then writes either to the out LDS image interior or to global NHWC.
// K layout: k = tap*C + ci, taps row-major dy,dx in [0,3)x[0,3).
// INPLACE (needs TO_LDS && RESID): the residual is read from out_lds itself,
// at exactly the 8 bytes the same thread then overwrites, and rlds is
// unused — so the block output can replace the block input in LDS without
// handing the compiler two __restrict__ pointers to one image.
// Every pixel fragment read from LDS feeds ALL the cout tiles of its group
// (CTG = 2 where COUT_TILES is even): one ds_read_b128 per k-step, not one
// per MFMA. Each (pixel tile, cout tile) accumulator is still one chain
// over ks ascending, so every sum is the same sequence of adds.
template <int H, int W, int C, int COUT, bool TO_LDS, bool RESID, int STRIDE,
          bool INPLACE = false>
TIP_DEV void conv3x3(
    const short* __restrict__ in_lds,   // [(H+2)(W+2)C] swizzled
    short* __restrict__ out_lds,        // TO_LDS: [(OH+2)(OW+2)COUT]
    short* __restrict__ gout,           // !TO_LDS: global NHWC [OH*OW*COUT]
    const short* __restrict__ rlds,     // RESID: residual LDS image (COUT ch)
    const short* __restrict__ wpack,    // [ksteps][64][8] per cout-tile:
                                        // [cout_tiles][ksteps][64][8]
    const float* __restrict__ bias) {   // [COUT], 16-byte aligned
  constexpr int OH = H / STRIDE, OW = W / STRIDE;
  constexpr int K = 9 * C;
  constexpr int KSTEPS = (K + 31) / 32;
  constexpr int NPIX = OH * OW;
  constexpr int PIX_TILES = NPIX / 16;
  constexpr int COUT_TILES = COUT / 16;
  constexpr int CTG = (COUT_TILES % 2) == 0 ? 2 : 1;  // cout tiles per A read
  using In = Img<H, W, C>;
  using Out = Img<OH, OW, COUT>;
  static_assert(!INPLACE || (TO_LDS && RESID), "INPLACE is an LDS residual");

  const int lane = lane_id();
  const int wid = wave_id();
  const int j = lane & 15;        // pixel within tile (operand row, D lane)
  const int g = lane >> 4;        // k-group (8 consecutive k); cout quad of D

  // LDS unit offset of k-step ks relative to a pixel's top-left tap
  // (constexpr after full unroll): k decomposes into (tap, channel) with
  // power-of-two C, dy = tap/3 via mul-shift (tap < 10).
  auto read_a = [&](int base, int ks) {
    const int k0 = ks * 32 + g * 8;
    if (k0 >= K) return short8{0, 0, 0, 0, 0, 0, 0, 0};
    const int tap = k0 / C;
    const int ci = k0 & (C - 1);
    const int dy = (tap * 11) >> 5;
    const int dx = tap - dy * 3;
    return lds_read_unit(in_lds, base + In::unit(dy, dx, ci >> 3));
  };
  auto a_base = [&](const TilePix& p) {
    return In::unit(p.oy * STRIDE, p.ox * STRIDE, 0);
  };
  auto load_bias = [&](int ct) {
    return *reinterpret_cast<const f32x4*>(bias + ct * 16 + g * 4);
  };
  // this lane's 4 couts ct*16 + g*4 .. +3 of pixel p (tile pt)
  auto epilogue = [&](int pt, const TilePix& p, int ct, const f32x4& acc,
                      const f32x4& bs) {
    const int c0 = ct * 16 + g * 4;
    const int so = swz(Out::unit(p.oy + 1, p.ox + 1, c0 >> 3)) * 8 + (c0 & 7);
    f32x4 v = acc + bs;
    if (RESID) {
      const short* rimg = INPLACE ? out_lds : rlds;
      add4_bf16(v, *reinterpret_cast<const uint2*>(rimg + so));
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
    const uint2 o = pack4_bf16(v);
    if (TO_LDS) {
      *reinterpret_cast<uint2*>(out_lds + so) = o;
    } else {
      *reinterpret_cast<uint2*>(gout + (int64_t)(pt * 16 + j) * COUT + c0) = o;
    }
  };

  // Small-plane specialization (4 pixel tiles x 4 cout tiles: the 8x8x64
  // output planes). Dealing the PIXEL tiles to the waves, as the generic path
  // does, makes every wave of the workgroup load the whole weight tensor:
  // four fetches of each weight byte per image, which kept stage 3 waiting
  // on vector memory (profiles/r14_small_plane_weights.md). Here a wave owns
  // NC cout tiles x NP pixel tiles (NC * NP = 4). NC = 2 ships: each weight
  // fragment is loaded by two waves of the workgroup instead of four, each
  // pixel fragment read by two instead of one (as before), and a wave runs
  // four independent MFMA chains. NC = 1 loads every weight byte once but
  // doubles the ds_read_b128 count, which then binds: slower than the old
  // dealing on the packed image, and only level with NC = 2 on a
  // conflict-free one. The weight fragments are loaded per k-step (the
  // unrolled loop lets the compiler issue them ahead); operand roles and
  // epilogue are the generic path's. Each (pixel tile, cout tile)
  // accumulator is one chain from zero over ks ascending, as everywhere.
  if constexpr (PIX_TILES == 4 && COUT_TILES == 4) {
    constexpr int NC = TIP_SP_NC, NP = 4 / NC;
    static_assert(NC == 1 || NC == 2 || NC == 4, "NC divides the 4 cout tiles");
    const int ct0 = (wid % (4 / NC)) * NC;
    const int pt0 = (wid / (4 / NC)) * NP;
    const short* wp = wpack + ((int64_t)ct0 * KSTEPS) * 64 * 8 + lane * 8;
    TilePix p[NP];
    int base[NP];
    f32x4 acc[NC][NP];
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      p[t] = tile_pix<OW>(pt0 + t, j);
      base[t] = a_base(p[t]);
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
      short8 b[NC], a[NP];
#pragma unroll
      for (int c = 0; c < NC; ++c)
        b[c] = *reinterpret_cast<const short8*>(
            wp + ((int64_t)c * KSTEPS + ks) * 64 * 8);
#pragma unroll
      for (int t = 0; t < NP; ++t) a[t] = read_a(base[t], ks);
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int t = 0; t < NP; ++t)
          acc[c][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              b[c], a[t], acc[c][t], 0, 0, 0);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const f32x4 bs = load_bias(ct0 + c);
#pragma unroll
      for (int t = 0; t < NP; ++t)
        epilogue(pt0 + t, p[t], ct0 + c, acc[c][t], bs);
    }
    return;
  }

  // cout-group outer loop: the group's weight fragments are preloaded into
  // registers ONCE (CTG x KSTEPS x 16 B per lane) so the MFMA loop is pure
  // ds_read + mfma — no global loads on the critical path (the per-mfma
  // L2 weight load was the previous bound at ~2 waves/SIMD occupancy).
  for (int ct = 0; ct < COUT_TILES; ct += CTG) {
    short8 wfrag[CTG][KSTEPS];
    f32x4 bs[CTG];
#pragma unroll
    for (int c = 0; c < CTG; ++c) {
      const short* wp =
          wpack + ((int64_t)(ct + c) * KSTEPS) * 64 * 8 + lane * 8;
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks)
        wfrag[c][ks] =
            *reinterpret_cast<const short8*>(wp + (int64_t)ks * 64 * 8);
      bs[c] = load_bias(ct + c);
    }

    // Two independent pixel tiles per iteration (times CTG cout tiles):
    // the MFMA accumulation chains interleave, hiding the
    // dependent-accumulator and LDS-read latency that a single chain
    // serialises on.
    int pt = wid;
    for (; pt + 4 < PIX_TILES; pt += 8) {
      const TilePix p0 = tile_pix<OW>(pt, j), p1 = tile_pix<OW>(pt + 4, j);
      const int b0 = a_base(p0), b1 = a_base(p1);
      f32x4 acc0[CTG], acc1[CTG];
#pragma unroll
      for (int c = 0; c < CTG; ++c) {
        acc0[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        acc1[c] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks) {
        const short8 a0 = read_a(b0, ks);
        const short8 a1 = read_a(b1, ks);
#pragma unroll
        for (int c = 0; c < CTG; ++c) {
          acc0[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              wfrag[c][ks], a0, acc0[c], 0, 0, 0);
          acc1[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              wfrag[c][ks], a1, acc1[c], 0, 0, 0);
        }
      }
#pragma unroll
      for (int c = 0; c < CTG; ++c) {
        epilogue(pt, p0, ct + c, acc0[c], bs[c]);
        epilogue(pt + 4, p1, ct + c, acc1[c], bs[c]);
      }
    }
    for (; pt < PIX_TILES; pt += 4) {
      const TilePix p0 = tile_pix<OW>(pt, j);
      const int b0 = a_base(p0);
      f32x4 acc[CTG];
#pragma unroll
      for (int c = 0; c < CTG; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks) {
        const short8 a = read_a(b0, ks);
#pragma unroll
        for (int c = 0; c < CTG; ++c)
          acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              wfrag[c][ks], a, acc[c], 0, 0, 0);
      }
#pragma unroll
      for (int c = 0; c < CTG; ++c) epilogue(pt, p0, ct + c, acc[c], bs[c]);
    }
  }
}

// 1x1 stride-2 shortcut projection, accumulated in the conv2 epilogue is
// complex; instead we compute the projected residual into rlds first.
// rlds: [(OH+2) x (OW+2) x COUT] swizzled image (interior only written;
// halo must be pre-zeroed). wpack1x1: K = C padded to 32. Operand roles and
// epilogue as in conv3x3 (no relu); a wave reads the pixel fragments of a
// tile once and runs them against every cout tile.
template <int H, int W, int C, int COUT>
TIP_DEV void shortcut1x1_s2(
    const short* __restrict__ in_lds, short* __restrict__ rlds,
    const short* __restrict__ wpack, const float* __restrict__ bias) {
  constexpr int OH = H / 2, OW = W / 2;
  constexpr int KSTEPS = (C + 31) / 32;
  constexpr int NPIX = OH * OW;
  constexpr int PIX_TILES = NPIX / 16;
  constexpr int COUT_TILES = COUT / 16;
  using In = Img<H, W, C>;
  using Out = Img<OH, OW, COUT>;
  const int lane = lane_id();
  const int wid = wave_id();
  const int j = lane & 15;
  const int g = lane >> 4;
  for (int pt = wid; pt < PIX_TILES; pt += 4) {
    const TilePix p = tile_pix<OW>(pt, j);
    short8 a[KSTEPS];
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
      const int k0 = ks * 32 + g * 8;
      a[ks] = short8{0, 0, 0, 0, 0, 0, 0, 0};
      // center tap, halo coords
      if (k0 < C)
        a[ks] = lds_read_unit(
            in_lds, In::unit(p.oy * 2 + 1, p.ox * 2 + 1, k0 >> 3));
    }
#pragma unroll
    for (int ct = 0; ct < COUT_TILES; ++ct) {
      const short* wp = wpack + ((int64_t)ct * KSTEPS) * 64 * 8 + lane * 8;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks) {
        const short8 b =
            *reinterpret_cast<const short8*>(wp + (int64_t)ks * 64 * 8);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, a[ks], acc, 0, 0, 0);
      }
      const int c0 = ct * 16 + g * 4;
      const int so =
          swz(Out::unit(p.oy + 1, p.ox + 1, c0 >> 3)) * 8 + (c0 & 7);
      const f32x4 v = acc + *reinterpret_cast<const f32x4*>(bias + c0);
      *reinterpret_cast<uint2*>(rlds + so) = pack4_bf16(v);
    }
  }
}
