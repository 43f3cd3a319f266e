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
//   16-byte units XOR-swizzled (u ^= (u>>4)&7) so the per-tap
//   ds_read_b128 gathers are bank-conflict-free for C in {16, 32, 64}.
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
//   (The small-plane path of conv3x3 keeps pixel-first operands; see there.)
//   (The layout is verified at runtime by the mfma_probe test kernel, and
//   that the swap changes no fp32 bit by test_gpu_resnet_conv_epilogue.)
// - one workgroup = one image; 4 waves split the plane's 16-pixel tiles.

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
  static constexpr int UNITS = (H + 2) * (W + 2) * UPP;
  static constexpr int XSTEP = UPP;
  static TIP_DEV int unit(int y, int x, int h) {
    return (y * (W + 2) + x) * UPP + h;
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

// Epilogue helpers. The convs (all but conv3x3's small-plane path) issue the
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

  // Small-plane specialization (PIX_TILES <= 4, i.e. the 8x8 stage): each
  // wave owns at most ONE pixel tile, so the generic path's dual-PIXEL
  // MFMA chains collapse to a single dependent chain (measured 24% slower
  // per FLOP than the 32x32 stage). Interleave TWO COUT tiles instead:
  // the pixel fragment is shared, the weight fragments load from L2 per
  // k-step (high occupancy here — 6 blocks/CU — hides the load latency the
  // preload design was protecting the low-occupancy stages from).
  // This path keeps the ORIGINAL operand roles (pixel fragment first, D
  // col = lane&15 = cout, row = (lane>>4)*4 + reg = pixel) and the
  // element-wise epilogue: it waits on the L2 weight loads, not on LDS, and
  // with the swapped roles and the packed epilogue it measured 5.6 % slower
  // in stage 3 and lost stage 2 its whole gain (sharing the fragment across
  // all four cout tiles: no better); profiles/r09_conv_lds_traffic.md. The
  // sums are the same either way, bit for bit.
  if constexpr (PIX_TILES <= 4 && CTG == 2) {
    const int pt = wid;
    if (pt >= PIX_TILES) return;
    const int apix = pt * 16 + j;
    const int aoy = apix / OW, aox = apix - aoy * OW;
    const int abase = In::unit(aoy * STRIDE, aox * STRIDE, 0);
    for (int ct = 0; ct < COUT_TILES; ct += 2) {
      const short* wp0 = wpack + ((int64_t)ct * KSTEPS) * 64 * 8 + lane * 8;
      const short* wp1 = wp0 + (int64_t)KSTEPS * 64 * 8;
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f};
      f32x4 acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks) {
        const int k0 = ks * 32 + g * 8;
        short8 a;
        if (k0 < K) {
          const int tap = k0 / C;
          const int ci = k0 & (C - 1);
          const int dy = (tap * 11) >> 5;
          const int dx = tap - dy * 3;
          a = lds_read_unit(in_lds, abase + In::unit(dy, dx, ci >> 3));
        } else {
          a = short8{0, 0, 0, 0, 0, 0, 0, 0};
        }
        const short8 b0 =
            *reinterpret_cast<const short8*>(wp0 + (int64_t)ks * 64 * 8);
        const short8 b1 =
            *reinterpret_cast<const short8*>(wp1 + (int64_t)ks * 64 * 8);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b1, acc1, 0, 0, 0);
      }
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int cout = (ct + half) * 16 + j;
        const float bs = bias[cout];
        const f32x4& acc = half ? acc1 : acc0;
        const int pix0 = pt * 16 + g * 4;
        const int oy = pix0 / OW, ox = pix0 - oy * OW;
        const int u0 = Out::unit(oy + 1, ox + 1, cout >> 3);
        const int e = cout & 7;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          float v = acc[reg] + bs;
          if (RESID) {
            const short* rimg = INPLACE ? out_lds : rlds;
            const short* runit = rimg + swz(u0 + reg * Out::XSTEP) * 8;
            v += __bfloat162float(reinterpret_cast<const bf16*>(runit)[e]);
          }
          v = fmaxf(v, 0.f);
          const bf16 ov = __float2bfloat16(v);
          if (TO_LDS) {
            short* unit = out_lds + swz(u0 + reg * Out::XSTEP) * 8;
            reinterpret_cast<bf16*>(unit)[e] = ov;
          } else {
            reinterpret_cast<bf16*>(gout)[(int64_t)(pix0 + reg) * COUT + cout] =
                ov;
          }
        }
      }
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
