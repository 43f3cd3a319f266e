// Fused MC-dropout tail of a one-block post-LN transformer: variation-ratio
// votes, and optionally the sample statistics, for models with four dropout
// sites behind a deterministic attention prefix.
//
// The S samples of one input share the embedding x [T][E] and the attention
// output attn [T][E]; they differ only in
//   h = LN1(x + drop1(attn))                          per token
//   y = LN2(h + drop2(W2 relu(W1 h + b1) + b2))       per token
//   g = mean_t y
//   z = relu(W3 drop3(g) + b3)
//   l = W4 drop4(z) + b4
// This kernel evaluates all S tails of a row in one block, the masks made in
// registers by the stateless generator of mcdropout.hip (same r, key, word;
// keep = word >= T_site). The four sites share one flat element axis:
//   drop1 (t, e) -> t*E + e            drop3 e -> 2*T*E + e
//   drop2 (t, e) -> T*E + t*E + e      drop4 h -> 2*T*E + E + h
// A dropped site is v + m * u with m = keep ? scale : 0, the product and the
// sum rounded separately (as the CPU oracle does).
//
// Layout of the work:
//   - one row per 256-thread block iteration, grid-stride over rows (grid
//     sized from the CU count); the row's x and attn are staged to LDS as
//     [T][E], the parameters once per block: W1 [F][E], W2 transposed to
//     [F][E], W3 [H][E], W4 transposed to [H][4], the vectors behind them;
//   - samples live on lanes: thread i owns sample s0 + i of the current
//     256-sample chunk, so every LDS read is wave-uniform (a broadcast);
//   - per token a lane keeps h[E] in registers and streams the FFN over f:
//     hidden unit f is a dot product over e, goes through the ReLU and is
//     folded into out[E] at once. LN2 follows and the result is added into
//     pooled[E]. After the token loop W3 is streamed over h straight into
//     the C logits. No hidden, z or [S*N, T, E] array exists anywhere;
//   - every float sum of a sample runs in a fixed order in its own lane
//     (e, f, t, h ascending); no float atomics. Votes are one ballot +
//     popcount per class and wave, merged over the waves in integers;
//   - statistics variant: per-lane softmax and entropy as in mcdropout.hip,
//     summed over the chunks in the lane, one 64-lane xor butterfly per row,
//     then the four waves added in ascending order.
// A row's outputs depend only on (seed, global row, its x / attn, the
// parameters), never on batch, grid or block.

#include "tip_common.h"

#include <stdexcept>
#include <string>

constexpr int MCT_THREADS = 256;               // one sample per thread
constexpr int MCT_WAVES = MCT_THREADS / WAVE;
constexpr int MCT_E = 32;                      // embedding width (fixed)
constexpr int MCT_MAX_T = 128;
constexpr int MCT_MAX_F = 64;
constexpr int MCT_MAX_H = 64;
constexpr int MCT_MAX_C = 4;
constexpr int MCT_CP = 4;                      // classes padded to one float4
constexpr int MCT_WAVES_PER_SIMD = 3;          // 168 VGPRs per lane
constexpr int MCT_BLOCKS_PER_CU = MCT_WAVES_PER_SIMD;  // 4 waves per block
constexpr int MCT_LDS_PER_CU = 160 * 1024;

struct MctParams {
  const float *ln1_w, *ln1_b, *w1, *b1, *w2, *b2, *ln2_w, *ln2_b, *w3, *b3,
      *w4, *b4;
  float eps;
  uint32_t thresh[4];
  float scale[4];
};

static void mct_check(hipError_t e, const char* what) {
  if (e != hipSuccess)
    throw std::runtime_error(std::string("mc_transformer: ") + what + ": " +
                             hipGetErrorString(e));
}

// LDS image in floats; every section starts on a 16-byte boundary.
struct MctLayout {
  int x, a, w1, w2t, w3, w4t, b1, b3, vec, red, total;
};

__host__ __device__ inline MctLayout mct_layout(int T, int F, int H) {
  MctLayout l;
  const int fp = (F + 3) / 4 * 4, hp = (H + 3) / 4 * 4;
  l.x = 0;
  l.a = l.x + T * MCT_E;
  l.w1 = l.a + T * MCT_E;
  l.w2t = l.w1 + F * MCT_E;
  l.w3 = l.w2t + F * MCT_E;
  l.w4t = l.w3 + H * MCT_E;
  l.b1 = l.w4t + H * MCT_CP;
  l.b3 = l.b1 + fp;
  l.vec = l.b3 + hp;              // ln1_w, ln1_b, ln2_w, ln2_b, b2 [E]; b4 [4]
  l.red = l.vec + 5 * MCT_E + MCT_CP;  // per-wave votes [4][4], sums [4][8]
  l.total = l.red + MCT_WAVES * MCT_CP + MCT_WAVES * 8;
  return l;
}

// E floats from a 16-byte aligned, wave-uniform LDS address.
TIP_DEV void mct_row(const float* p, float (&v)[MCT_E]) {
  const float4* q = reinterpret_cast<const float4*>(p);
#pragma unroll
  for (int i = 0; i < MCT_E / 4; ++i) {
    const float4 t = q[i];
    v[4 * i + 0] = t.x;
    v[4 * i + 1] = t.y;
    v[4 * i + 2] = t.z;
    v[4 * i + 3] = t.w;
  }
}

// v <- (v - mean) * rstd * w + b over the E elements, biased variance, sums
// e-ascending; 1 / sqrtf is the correctly rounded division of the correctly
// rounded square root.
TIP_DEV void mct_layer_norm(float (&v)[MCT_E], const float* w, const float* b,
                            float eps) {
  float sum = 0.f;
#pragma unroll
  for (int e = 0; e < MCT_E; ++e) sum += v[e];
  const float mean = sum / (float)MCT_E;
  float sq = 0.f;
#pragma unroll
  for (int e = 0; e < MCT_E; ++e) {
    v[e] -= mean;
    sq = fmaf(v[e], v[e], sq);
  }
  const float rstd = 1.f / sqrtf(sq / (float)MCT_E + eps);
  const float4* w4 = reinterpret_cast<const float4*>(w);
  const float4* b4 = reinterpret_cast<const float4*>(b);
#pragma unroll
  for (int i = 0; i < MCT_E / 4; ++i) {
    const float4 ww = w4[i], bb = b4[i];
    v[4 * i + 0] = fmaf(v[4 * i + 0] * rstd, ww.x, bb.x);
    v[4 * i + 1] = fmaf(v[4 * i + 1] * rstd, ww.y, bb.y);
    v[4 * i + 2] = fmaf(v[4 * i + 2] * rstd, ww.z, bb.z);
    v[4 * i + 3] = fmaf(v[4 * i + 3] * rstd, ww.w, bb.w);
  }
}

// scale if element d of this sample is kept, else 0. thresh == 0 keeps all.
TIP_DEV float mct_keep(uint32_t key, uint32_t d, uint32_t thresh,
                       float scale) {
  return mix32(key ^ (d * 0x85EBCA6Bu)) >= thresh ? scale : 0.f;
}

template <bool STATS>
__global__ __launch_bounds__(MCT_THREADS, MCT_WAVES_PER_SIMD) void mc_transformer_kernel(
    const float* __restrict__ x, const float* __restrict__ attn, MctParams P,
    int n_rows, int T, int F, int H, int C, int S, uint32_t seed_lo,
    uint32_t seed_hi, uint32_t row_offset, int* __restrict__ votes,
    float* __restrict__ mean_probs, float* __restrict__ mean_entropy) {
  extern __shared__ float4 mct_lds[];
  float* lds = reinterpret_cast<float*>(mct_lds);
  const MctLayout L = mct_layout(T, F, H);
  const int tid = threadIdx.x;
  const int lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane(wave_id());

  // ---- parameters, once per block ----
  for (int i = tid; i < F * MCT_E; i += MCT_THREADS) {
    lds[L.w1 + i] = P.w1[i];
    const int f = i / MCT_E, e = i - f * MCT_E;
    lds[L.w2t + i] = P.w2[e * F + f];
  }
  for (int i = tid; i < H * MCT_E; i += MCT_THREADS) lds[L.w3 + i] = P.w3[i];
  for (int i = tid; i < H * MCT_CP; i += MCT_THREADS) {
    const int h = i / MCT_CP, c = i - h * MCT_CP;
    lds[L.w4t + i] = c < C ? P.w4[c * H + h] : 0.f;
  }
  for (int i = tid; i < F; i += MCT_THREADS) lds[L.b1 + i] = P.b1[i];
  for (int i = tid; i < H; i += MCT_THREADS) lds[L.b3 + i] = P.b3[i];
  if (tid < MCT_E) {
    lds[L.vec + 0 * MCT_E + tid] = P.ln1_w[tid];
    lds[L.vec + 1 * MCT_E + tid] = P.ln1_b[tid];
    lds[L.vec + 2 * MCT_E + tid] = P.ln2_w[tid];
    lds[L.vec + 3 * MCT_E + tid] = P.ln2_b[tid];
    lds[L.vec + 4 * MCT_E + tid] = P.b2[tid];
  }
  if (tid < MCT_CP) lds[L.vec + 5 * MCT_E + tid] = tid < C ? P.b4[tid] : 0.f;

  const float* b4 = lds + L.vec + 5 * MCT_E;
  int* wave_votes = reinterpret_cast<int*>(lds + L.red);
  float* wave_sums = lds + L.red + MCT_WAVES * MCT_CP;
  const uint32_t te = (uint32_t)(T * MCT_E);
  const float t_den = (float)T;

  for (int64_t n = blockIdx.x; n < n_rows; n += gridDim.x) {
    // ---- this row's x and attn -> LDS (the barrier also covers the
    // parameters on the first pass and the previous row's last readers) ----
    __syncthreads();
    {
      const float4* xs = reinterpret_cast<const float4*>(x + n * T * MCT_E);
      const float4* as = reinterpret_cast<const float4*>(attn + n * T * MCT_E);
      for (int i = tid; i < T * MCT_E / 4; i += MCT_THREADS) {
        mct_lds[L.x / 4 + i] = xs[i];
        mct_lds[L.a / 4 + i] = as[i];
      }
    }
    __syncthreads();

    uint32_t r = mix32(row_offset + (uint32_t)n + 0x6A09E667u);
    r = mix32(r ^ seed_lo);
    r = mix32(r ^ seed_hi);
    int row_votes = 0;  // thread c < C accumulates votes[n][c]
    float psum[MCT_CP] = {0.f, 0.f, 0.f, 0.f};
    float hsum = 0.f;

    for (int s0 = 0; s0 < S; s0 += MCT_THREADS) {
      const bool valid = s0 + tid < S;
      int best = 0;
      float logit[MCT_CP] = {0.f, 0.f, 0.f, 0.f};
      // a wave with no sample in this chunk skips the arithmetic (uniform)
      if (s0 + wave * WAVE < S) {
        const uint32_t key =
            mix32(r + (uint32_t)(s0 + tid) * 0x9E3779B9u);
        float pooled[MCT_E];
#pragma unroll
        for (int e = 0; e < MCT_E; ++e) pooled[e] = 0.f;

        for (int t = 0; t < T; ++t) {
          // The LN vectors and b2 do not change over the token loop; read
          // through an address the optimizer cannot see through, or it
          // hoists all 160 loads out of the loop and the lane runs out of
          // registers.
          int vec = L.vec;
          asm volatile("" : "+v"(vec));
          const float* ln1_w = lds + vec;
          const float* ln1_b = ln1_w + MCT_E;
          const float* ln2_w = ln1_b + MCT_E;
          const float* ln2_b = ln2_w + MCT_E;
          const float* b2 = ln2_b + MCT_E;
          float h[MCT_E], out[MCT_E];
          // h = LN1(x + drop1(attn))
          mct_row(lds + L.x + t * MCT_E, h);
          mct_row(lds + L.a + t * MCT_E, out);
          const uint32_t d1 = (uint32_t)(t * MCT_E);
          if (P.thresh[0]) {
#pragma unroll
            for (int e = 0; e < MCT_E; ++e) {
#pragma clang fp contract(off)
              h[e] = h[e] + mct_keep(key, d1 + e, P.thresh[0], P.scale[0]) * out[e];
            }
          } else {
#pragma unroll
            for (int e = 0; e < MCT_E; ++e) h[e] += out[e];
          }
          mct_layer_norm(h, ln1_w, ln1_b, P.eps);

          // out = W2 relu(W1 h + b1) + b2, hidden unit by hidden unit
          mct_row(b2, out);
          for (int f = 0; f < F; ++f) {
            const float4* w1r =
                reinterpret_cast<const float4*>(lds + L.w1 + f * MCT_E);
            float a = lds[L.b1 + f];
#pragma unroll
            for (int i = 0; i < MCT_E / 4; ++i) {
              const float4 w = w1r[i];
              a = fmaf(w.x, h[4 * i + 0], a);
              a = fmaf(w.y, h[4 * i + 1], a);
              a = fmaf(w.z, h[4 * i + 2], a);
              a = fmaf(w.w, h[4 * i + 3], a);
            }
            a = fmaxf(a, 0.f);
            const float4* w2r =
                reinterpret_cast<const float4*>(lds + L.w2t + f * MCT_E);
#pragma unroll
            for (int i = 0; i < MCT_E / 4; ++i) {
              const float4 w = w2r[i];
              out[4 * i + 0] = fmaf(w.x, a, out[4 * i + 0]);
              out[4 * i + 1] = fmaf(w.y, a, out[4 * i + 1]);
              out[4 * i + 2] = fmaf(w.z, a, out[4 * i + 2]);
              out[4 * i + 3] = fmaf(w.w, a, out[4 * i + 3]);
            }
          }

          // pooled += LN2(h + drop2(out))
          if (P.thresh[1]) {
#pragma unroll
            for (int e = 0; e < MCT_E; ++e) {
#pragma clang fp contract(off)
              out[e] = h[e] +
                       mct_keep(key, te + d1 + e, P.thresh[1], P.scale[1]) * out[e];
            }
          } else {
#pragma unroll
            for (int e = 0; e < MCT_E; ++e) out[e] += h[e];
          }
          mct_layer_norm(out, ln2_w, ln2_b, P.eps);
#pragma unroll
          for (int e = 0; e < MCT_E; ++e) pooled[e] += out[e];
        }

        // g = drop3(pooled / T). The element base is made opaque so that
        // the 32 per-element hash constants are not kept in scalar registers
        // across the whole row loop.
        uint32_t d3 = 2 * te;
        asm volatile("" : "+s"(d3));
#pragma unroll
        for (int e = 0; e < MCT_E; ++e) {
          pooled[e] = pooled[e] / t_den;
          if (P.thresh[2])
            pooled[e] *= mct_keep(key, d3 + e, P.thresh[2], P.scale[2]);
        }
        // l = W4 drop4(relu(W3 g + b3)) + b4, hidden unit by hidden unit
        {
          const float4 bb = *reinterpret_cast<const float4*>(b4);
          logit[0] = bb.x;
          logit[1] = bb.y;
          logit[2] = bb.z;
          logit[3] = bb.w;
        }
        for (int hh = 0; hh < H; ++hh) {
          const float4* w3r =
              reinterpret_cast<const float4*>(lds + L.w3 + hh * MCT_E);
          float z = lds[L.b3 + hh];
#pragma unroll
          for (int i = 0; i < MCT_E / 4; ++i) {
            const float4 w = w3r[i];
            z = fmaf(w.x, pooled[4 * i + 0], z);
            z = fmaf(w.y, pooled[4 * i + 1], z);
            z = fmaf(w.z, pooled[4 * i + 2], z);
            z = fmaf(w.w, pooled[4 * i + 3], z);
          }
          z = fmaxf(z, 0.f);
          if (P.thresh[3])
            z *= mct_keep(key, d3 + MCT_E + hh, P.thresh[3], P.scale[3]);
          const float4 w =
              *reinterpret_cast<const float4*>(lds + L.w4t + hh * MCT_CP);
          logit[0] = fmaf(w.x, z, logit[0]);
          logit[1] = fmaf(w.y, z, logit[1]);
          logit[2] = fmaf(w.z, z, logit[2]);
          logit[3] = fmaf(w.w, z, logit[3]);
        }

        // first-max argmax over the real classes
        float best_v = logit[0];
#pragma unroll
        for (int c = 1; c < MCT_CP; ++c)
          if (c < C && logit[c] > best_v) {
            best_v = logit[c];
            best = c;
          }

        if constexpr (STATS) {
          // softmax and entropy of this sample in its own lane: every
          // exponent is <= 0 and z >= 1 (see mcdropout.hip)
          float zs = 0.f, ts = 0.f, ex[MCT_CP];
#pragma unroll
          for (int c = 0; c < MCT_CP; ++c) {
            const float dlt = logit[c] - best_v;
            ex[c] = c < C ? expf(dlt) : 0.f;
            zs += ex[c];
            ts = fmaf(ex[c], dlt, ts);
          }
          float inv = 1.f / zs;
          float ent = logf(zs) - ts * inv;
          if (!valid) {  // idle sample slot: add zero
            inv = 0.f;
            ent = 0.f;
          }
#pragma unroll
          for (int c = 0; c < MCT_CP; ++c) psum[c] = fmaf(ex[c], inv, psum[c]);
          hsum += ent;
        }
      }

      // votes of this chunk: ballot + popcount per wave, merged in integers
      {
        int mine = 0;
#pragma unroll
        for (int c = 0; c < MCT_CP; ++c) {
          const int cnt = __popcll(__ballot(valid && best == c));
          if (lane == c) mine = cnt;
        }
        if (lane < MCT_CP) wave_votes[wave * MCT_CP + lane] = mine;
      }
      __syncthreads();
      if (tid < MCT_CP) {
#pragma unroll
        for (int w = 0; w < MCT_WAVES; ++w)
          row_votes += wave_votes[w * MCT_CP + tid];
      }
      __syncthreads();
    }

    if (tid < C) votes[n * C + tid] = row_votes;
    if constexpr (STATS) {
#pragma unroll
      for (int off = WAVE / 2; off >= 1; off >>= 1) {
#pragma unroll
        for (int c = 0; c < MCT_CP; ++c) psum[c] += __shfl_xor(psum[c], off);
        hsum += __shfl_xor(hsum, off);
      }
      if (lane == 0) {
#pragma unroll
        for (int c = 0; c < MCT_CP; ++c) wave_sums[wave * 8 + c] = psum[c];
        wave_sums[wave * 8 + MCT_CP] = hsum;
      }
      __syncthreads();
      // Opaque copy of tid: the output addresses are formed here, once per
      // row, instead of being carried in registers through the token loop.
      int c = tid;
      asm volatile("" : "+v"(c));
      if (c <= MCT_CP) {  // the waves in ascending order
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < MCT_WAVES; ++w) tot += wave_sums[w * 8 + c];
        const float inv_s = 1.f / (float)S;
        if (c < C) mean_probs[n * C + c] = tot * inv_s;
        if (c == MCT_CP) mean_entropy[n] = tot * inv_s;
      }
      // the next iteration's first barrier orders these reads before the
      // next row's writes to wave_sums
    }
  }
}

int mc_transformer_lds_bytes(int T, int F, int H) {
  return mct_layout(T, F, H).total * (int)sizeof(float);
}

// Blocks the launcher uses at most: LDS-bound blocks per CU (capped at
// MCT_BLOCKS_PER_CU) times the CU count.
int mc_transformer_max_grid(int T, int F, int H) {
  const int lds_bytes = mc_transformer_lds_bytes(T, F, H);
  int dev = 0, cus = 0;
  mct_check(hipGetDevice(&dev), "hipGetDevice");
  mct_check(
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev),
      "hipDeviceGetAttribute");
  int per_cu = MCT_LDS_PER_CU / (lds_bytes > 0 ? lds_bytes : 1);
  if (per_cu > MCT_BLOCKS_PER_CU) per_cu = MCT_BLOCKS_PER_CU;
  if (per_cu < 1) per_cu = 1;
  return (cus > 0 ? cus : 1) * per_cu;
}

// {E, max T, max F, max H, max C}
void mc_transformer_limits(int* out) {
  out[0] = MCT_E;
  out[1] = MCT_MAX_T;
  out[2] = MCT_MAX_F;
  out[3] = MCT_MAX_H;
  out[4] = MCT_MAX_C;
}

// Caller guarantees the envelope (E == 32, T <= 128, F <= 64, H <= 64,
// C <= 4, all >= 1), n_rows >= 1, 1 <= S <= 65535 and 16-byte aligned x / attn.
// ptrs: ln1_w, ln1_b, w1, b1, w2, b2, ln2_w, ln2_b, w3, b3, w4, b4.
void launch_mc_transformer(const float* x, const float* attn,
                           const float* const* ptrs, float eps,
                           const uint32_t* thresh, const float* scale,
                           int n_rows, int T, int F, int H, int C, int S,
                           uint32_t seed_lo, uint32_t seed_hi,
                           uint32_t row_offset, int* votes, float* mean_probs,
                           float* mean_entropy, bool stats, hipStream_t s) {
  MctParams P;
  P.ln1_w = ptrs[0];
  P.ln1_b = ptrs[1];
  P.w1 = ptrs[2];
  P.b1 = ptrs[3];
  P.w2 = ptrs[4];
  P.b2 = ptrs[5];
  P.ln2_w = ptrs[6];
  P.ln2_b = ptrs[7];
  P.w3 = ptrs[8];
  P.b3 = ptrs[9];
  P.w4 = ptrs[10];
  P.b4 = ptrs[11];
  P.eps = eps;
  for (int i = 0; i < 4; ++i) {
    P.thresh[i] = thresh[i];
    P.scale[i] = scale[i];
  }
  const int lds_bytes = mc_transformer_lds_bytes(T, F, H);
  int grid = n_rows;
  const int cap = mc_transformer_max_grid(T, F, H);
  if (grid > cap) grid = cap;
  auto k = stats ? mc_transformer_kernel<true> : mc_transformer_kernel<false>;
  mct_check(hipFuncSetAttribute((const void*)k,
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                lds_bytes),
            "hipFuncSetAttribute");
  k<<<grid, MCT_THREADS, lds_bytes, s>>>(x, attn, P, n_rows, T, F, H, C, S,
                                         seed_lo, seed_hi, row_offset, votes,
                                         mean_probs, mean_entropy);
  mct_check(hipGetLastError(), "launch");
}
