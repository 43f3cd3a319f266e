// Fused MC-dropout head: variation-ratio votes, and optionally the sample
// statistics (mean softmax, mean per-sample entropy), in one kernel.
//
// For a model whose only stochastic layer is a Dropout directly in front of
// the final Linear, the S MC samples of one input differ only in which of
// the D features reach a [C, D] mat-vec. This kernel takes the deterministic
// features once and evaluates all S masked heads per row, generating the
// dropout masks in registers from a stateless counter hash (no [S*N, D]
// tensor is ever written) and counting the argmax votes on the fly.
//
// Mask generator (bit-identical to ops/fallback.py::dropout_keep_mask; all
// arithmetic unsigned 32-bit, wrapping):
//   r    = mix32(mix32(mix32(g + 0x6A09E667) ^ seed_lo) ^ seed_hi)   per row
//   key  = mix32(r + s * 0x9E3779B9)                        per (row, sample)
//   word = mix32(key ^ (d * 0x85EBCA6B))                    per element
//   keep = word >= T,  T = floor(p * 2^32)
//
// Layout of the work:
//   - the weights are staged once per block into LDS, transposed to
//     [D][CP] (CP = C rounded up to 4, pad classes zero), so one feature's
//     weight row is CP/4 aligned 16-byte reads;
//   - one wave per row, grid-stride over rows (grid sized from the CU count,
//     so the staging cost is O(grid), not O(N));
//   - samples live on lanes: lane l owns samples l, l+64, l+128, l+192 of
//     the current 256-sample chunk, 4 x CP accumulators in registers. The
//     feature value and the weight row are wave-uniform: the LDS reads are
//     broadcasts that serve four samples each;
//   - each lane loads one of 64 consecutive features; a ballot of the
//     non-zero ones drives a uniform loop that visits only those (post-ReLU
//     / post-pool features are mostly zero). The mask is stateless, so
//     skipping a feature changes no other mask bit;
//   - no cross-lane float reduction, no float atomics: every sample's sum
//     runs d-ascending in its own lane (bitwise reproducible). Votes are
//     counted with one ballot+popcount per class; lane c stores votes[n][c].
//
// Statistics variant (STATS = true, mc_dropout_stats): same masks, staging,
// grid and logits; after a chunk's feature loop each lane turns its samples'
// logits into a softmax (max over the C real classes subtracted, expf,
// one reciprocal) and the entropy log Z - sum_c e_c (v_c - max) / Z, and adds
// both to CP + 1 per-lane running sums: ascending j within a chunk, chunks
// ascending, lanes whose sample index is >= S add zero. Once per row a
// 64-lane xor butterfly (offsets 32, 16, ..., 1) reduces the sums, which are
// scaled by 1/S and stored by lanes 0..C-1 (mean_probs) and lane 0
// (mean_entropy). The order is fixed, so a row's floats depend only on
// (seed, global row, feats row, head). No float atomics.

#include "tip_common.h"

#include <stdexcept>
#include <string>

constexpr int MCD_THREADS = 512;                 // 8 waves per block
constexpr int MCD_WAVES = MCD_THREADS / WAVE;    // rows in flight per block
constexpr int MCD_SPL = 4;                       // samples per lane per chunk
constexpr int MCD_CHUNK = WAVE * MCD_SPL;        // 256 samples per chunk
constexpr int MCD_MAX_C = 16;
constexpr int MCD_MAX_D = 2048;
constexpr int MCD_BLOCKS_PER_CU = 2;             // 16 waves/CU = 4 per SIMD
constexpr int MCD_LDS_PER_CU = 160 * 1024;

static void mcd_check(hipError_t e, const char* what) {
  if (e != hipSuccess)
    throw std::runtime_error(std::string("mc_dropout_votes: ") + what + ": " +
                             hipGetErrorString(e));
}

template <int CP, bool STATS>
__global__ __launch_bounds__(MCD_THREADS) void mc_dropout_votes_kernel(
    const float* __restrict__ feats, const float* __restrict__ weight,
    const float* __restrict__ bias, int n_rows, int D, int C, int S,
    uint32_t thresh, float scale, uint32_t seed_lo, uint32_t seed_hi,
    uint32_t row_offset, int* __restrict__ votes,
    float* __restrict__ mean_probs, float* __restrict__ mean_entropy) {
  // Samples per lane per chunk. A lane owns the samples congruent to its
  // index mod 64 whatever the chunk size, in ascending order, so the chunk
  // size changes no result. The statistics variant at CP = 16 carries 17
  // more live accumulators than the votes kernel; with 4 x 16 logit
  // accumulators it would need 145 VGPRs (3 waves per SIMD), so it runs
  // 2 samples per lane per chunk (128-sample chunks) to stay under 128.
  constexpr int SPL = (STATS && CP == 16) ? MCD_SPL / 2 : MCD_SPL;
  constexpr int CHUNK = WAVE * SPL;
  extern __shared__ float4 mcd_lds[];  // wT[D + 1][CP], row D = bias
  float* wT = reinterpret_cast<float*>(mcd_lds);

  // Stage weight [C][D] -> wT[D][CP] and the bias as row D; consecutive
  // threads write consecutive LDS dwords (conflict-free), pad classes are 0.
  for (int i = threadIdx.x; i < (D + 1) * CP; i += MCD_THREADS) {
    const int d = i / CP, c = i - d * CP;
    float v = 0.f;
    if (c < C) v = d < D ? weight[(int64_t)c * D + d] : bias[c];
    wT[i] = v;
  }
  __syncthreads();

  const int lane = lane_id();
  // wave-uniform by construction; readfirstlane lets the row loop, the
  // feature ballot loop and the LDS addresses live in scalar registers
  const int wave = __builtin_amdgcn_readfirstlane(wave_id());

  for (int64_t n = (int64_t)blockIdx.x * MCD_WAVES + wave; n < n_rows;
       n += (int64_t)gridDim.x * MCD_WAVES) {
    const float* frow = feats + n * D;
    uint32_t r = mix32(row_offset + (uint32_t)n + 0x6A09E667u);
    r = mix32(r ^ seed_lo);
    r = mix32(r ^ seed_hi);
    int my_votes = 0;  // lane c accumulates votes[n][c]
    // STATS: this lane's running sums of softmax[c] and of the entropy
    float psum[CP];
    float hsum = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) psum[c] = 0.f;

    for (int s0 = 0; s0 < S; s0 += CHUNK) {
      uint32_t key[SPL];
      float acc[SPL][CP];
#pragma unroll
      for (int j = 0; j < SPL; ++j) {
        key[j] = mix32(r + (uint32_t)(s0 + lane + WAVE * j) * 0x9E3779B9u);
#pragma unroll
        for (int c = 0; c < CP; ++c) acc[j][c] = 0.f;
      }

      for (int d0 = 0; d0 < D; d0 += WAVE) {
        const float fv = d0 + lane < D ? frow[d0 + lane] : 0.f;
        unsigned long long nz = __ballot(fv != 0.f);
        while (nz) {
          const int jl = __builtin_ctzll(nz);
          nz &= nz - 1;
          const float f = __builtin_bit_cast(
              float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, fv), jl));
          const int d = d0 + jl;
          const uint32_t dk = (uint32_t)d * 0x85EBCA6Bu;
          const float4* wrow = mcd_lds + d * (CP / 4);
          float w[CP];
#pragma unroll
          for (int q = 0; q < CP / 4; ++q) {
            const float4 t = wrow[q];
            w[4 * q + 0] = t.x;
            w[4 * q + 1] = t.y;
            w[4 * q + 2] = t.z;
            w[4 * q + 3] = t.w;
          }
#pragma unroll
          for (int j = 0; j < SPL; ++j) {
            const float x = mix32(key[j] ^ dk) >= thresh ? f : 0.f;
#pragma unroll
            for (int c = 0; c < CP; ++c) acc[j][c] = fmaf(x, w[c], acc[j][c]);
          }
        }
      }

      // logits, first-max argmax, vote count for this chunk
      float b[CP];
#pragma unroll
      for (int q = 0; q < CP / 4; ++q) {
        const float4 t = mcd_lds[D * (CP / 4) + q];
        b[4 * q + 0] = t.x;
        b[4 * q + 1] = t.y;
        b[4 * q + 2] = t.z;
        b[4 * q + 3] = t.w;
      }
#pragma unroll
      for (int j = 0; j < SPL; ++j) {
        const bool valid = s0 + lane + WAVE * j < S;
        int best = 0;
        float best_v = 0.f;
#pragma unroll
        for (int c = 0; c < CP; ++c) {
          // scale applied once after the sum, then the bias; two separately
          // rounded ops to match the CPU oracle exactly. __fmul_rn/__fadd_rn
          // are plain * and + in the HIP headers and were contracted into one
          // v_fma_f32 (a different last bit whenever scale is no power of
          // two), so contraction is switched off for this statement.
          float v;
          {
#pragma clang fp contract(off)
            v = scale * acc[j][c] + b[c];
          }
          if constexpr (STATS) acc[j][c] = v;
          if (c == 0) {
            best_v = v;
          } else if (c < C && v > best_v) {
            best_v = v;
            best = c;
          }
        }
#pragma nounroll
        for (int c = 0; c < C; ++c) {
          const int cnt = __popcll(__ballot(valid && best == c));
          if (lane == c) my_votes += cnt;
        }
        if constexpr (STATS) {
          // softmax of this sample's logits in its own lane; best_v is the
          // max over the real classes, so every exponent is <= 0, z >= 1 and
          // an underflowing class contributes 0 * finite = 0, never NaN
          float z = 0.f, t = 0.f;
#pragma unroll
          for (int c = 0; c < CP; ++c) {
            const float dlt = acc[j][c] - best_v;
            const float e = c < C ? expf(dlt) : 0.f;
            z += e;
            t = fmaf(e, dlt, t);
            acc[j][c] = e;
          }
          float inv = 1.f / z;
          float h = logf(z) - t * inv;
          if (!valid) {  // idle sample slot: add zero
            inv = 0.f;
            h = 0.f;
          }
#pragma unroll
          for (int c = 0; c < CP; ++c) psum[c] = fmaf(acc[j][c], inv, psum[c]);
          hsum += h;
        }
      }
    }
    if (lane < C) votes[n * C + lane] = my_votes;
    if constexpr (STATS) {
      // one xor butterfly per row over the CP class sums and the entropy sum
#pragma unroll
      for (int off = WAVE / 2; off >= 1; off >>= 1) {
#pragma unroll
        for (int c = 0; c < CP; ++c) psum[c] += __shfl_xor(psum[c], off);
        hsum += __shfl_xor(hsum, off);
      }
      const float inv_s = 1.f / (float)S;
      float mine = 0.f;  // select chain: no dynamic register index
#pragma unroll
      for (int c = 0; c < CP; ++c)
        if (lane == c) mine = psum[c];
      if (lane < C) mean_probs[n * C + lane] = mine * inv_s;
      if (lane == 0) mean_entropy[n] = hsum * inv_s;
    }
  }
}

// Blocks the launcher will use at most: LDS-bound blocks per CU (capped at
// MCD_BLOCKS_PER_CU) times the CU count.
int mc_dropout_max_grid(int D, int C) {
  const int cp = (C + 3) / 4 * 4;
  const int lds_bytes = (D + 1) * cp * (int)sizeof(float);
  int dev = 0, cus = 0;
  mcd_check(hipGetDevice(&dev), "hipGetDevice");
  mcd_check(
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev),
      "hipDeviceGetAttribute");
  int per_cu = MCD_LDS_PER_CU / (lds_bytes > 0 ? lds_bytes : 1);
  if (per_cu > MCD_BLOCKS_PER_CU) per_cu = MCD_BLOCKS_PER_CU;
  if (per_cu < 1) per_cu = 1;
  return (cus > 0 ? cus : 1) * per_cu;
}

int mc_dropout_rows_per_block() { return MCD_WAVES; }
int mc_dropout_max_classes() { return MCD_MAX_C; }
int mc_dropout_max_features() { return MCD_MAX_D; }

template <int CP, bool STATS>
static void mc_dropout_launch(const float* feats, const float* weight,
                              const float* bias, int n_rows, int D, int C,
                              int S, uint32_t thresh, float scale,
                              uint32_t seed_lo, uint32_t seed_hi,
                              uint32_t row_offset, int* votes,
                              float* mean_probs, float* mean_entropy,
                              hipStream_t s) {
  const int lds_bytes = (D + 1) * CP * (int)sizeof(float);
  int grid = ceil_div(n_rows, MCD_WAVES);
  const int cap = mc_dropout_max_grid(D, C);
  if (grid > cap) grid = cap;
  auto k = mc_dropout_votes_kernel<CP, STATS>;
  mcd_check(hipFuncSetAttribute((const void*)k,
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                lds_bytes),
            "hipFuncSetAttribute");
  k<<<grid, MCD_THREADS, lds_bytes, s>>>(feats, weight, bias, n_rows, D, C, S,
                                         thresh, scale, seed_lo, seed_hi,
                                         row_offset, votes, mean_probs,
                                         mean_entropy);
  mcd_check(hipGetLastError(), "launch");
}

template <bool STATS>
static void mc_dropout_dispatch(const float* feats, const float* weight,
                                const float* bias, int n_rows, int D, int C,
                                int S, uint32_t thresh, float scale,
                                uint32_t seed_lo, uint32_t seed_hi,
                                uint32_t row_offset, int* votes,
                                float* mean_probs, float* mean_entropy,
                                hipStream_t s) {
  if (C <= 4)
    mc_dropout_launch<4, STATS>(feats, weight, bias, n_rows, D, C, S, thresh,
                                scale, seed_lo, seed_hi, row_offset, votes,
                                mean_probs, mean_entropy, s);
  else if (C <= 8)
    mc_dropout_launch<8, STATS>(feats, weight, bias, n_rows, D, C, S, thresh,
                                scale, seed_lo, seed_hi, row_offset, votes,
                                mean_probs, mean_entropy, s);
  else if (C <= 12)
    mc_dropout_launch<12, STATS>(feats, weight, bias, n_rows, D, C, S, thresh,
                                 scale, seed_lo, seed_hi, row_offset, votes,
                                 mean_probs, mean_entropy, s);
  else
    mc_dropout_launch<16, STATS>(feats, weight, bias, n_rows, D, C, S, thresh,
                                 scale, seed_lo, seed_hi, row_offset, votes,
                                 mean_probs, mean_entropy, s);
}

// Caller guarantees 1 <= C <= 16, 1 <= D <= 2048, n_rows >= 1, S >= 1.
void launch_mc_dropout_votes(const float* feats, const float* weight,
                             const float* bias, int n_rows, int D, int C,
                             int S, uint32_t thresh, float scale,
                             uint32_t seed_lo, uint32_t seed_hi,
                             uint32_t row_offset, int* votes, hipStream_t s) {
  mc_dropout_dispatch<false>(feats, weight, bias, n_rows, D, C, S, thresh,
                             scale, seed_lo, seed_hi, row_offset, votes,
                             nullptr, nullptr, s);
}

// Same guarantees; mean_probs is [n_rows, C] and mean_entropy [n_rows].
void launch_mc_dropout_stats(const float* feats, const float* weight,
                             const float* bias, int n_rows, int D, int C,
                             int S, uint32_t thresh, float scale,
                             uint32_t seed_lo, uint32_t seed_hi,
                             uint32_t row_offset, int* votes,
                             float* mean_probs, float* mean_entropy,
                             hipStream_t s) {
  mc_dropout_dispatch<true>(feats, weight, bias, n_rows, D, C, S, thresh,
                            scale, seed_lo, seed_hi, row_offset, votes,
                            mean_probs, mean_entropy, s);
}
