// Fused neuron-coverage suite for gfx950: every NAC / SNAC / NBC / KMNC
// profile of a batch from ONE pass over the tapped layers, every TKNC
// profile from a second one. The layers are read where they lie (no
// concatenated copy); the bit layouts and every comparison are those of
// coverage.hip, so each word equals what profile_kernel / tknc_kernel give
// for the concatenated input.
//
// Threshold kernel. The grid is (row tiles, chunks of the concatenated
// neuron axis). A chunk is SUITE_CHUNK = 4 * 64 neurons: each of the block's
// four waves owns one 64-neuron group, i.e. word c0/64 of NAC and SNAC,
// words 2*c0/64.. of NBC and words S*c0/64.. of KMNC -- whole words of every
// family, written by nobody else, so the stores are plain. A lane loads its
// neuron's table values once and keeps them in registers for the tile's
// SUITE_ROW_TILE rows. Rows go through in batches of eight: the eight
// activation loads are issued together, ahead of the first ballot. Ballot r
// of a batch is parked in lane r, so after the batch lanes 0..7 hold one
// word each for eight rows and a single store instruction writes them.
// NBC's two ballots are interleaved bit by bit in those lanes; KMNC keeps a
// neuron's section bits in a 16-bit mask, and word j of the group is a
// second ballot over masks fetched from lane (j*64 + lane) / S.
// Popcounts meet in LDS and leave the block as integer atomic adds.
//
// Top-k kernel. One 256-thread block per (row, layer) sweeps the layer with
// four loads in flight per thread, keeps a sorted quad of tknc_key keys per
// lane, merges across the wave and the block, and sets the bits of every
// requested k with atomicOr.

#include "coverage_suite.h"
#include "tip_common.h"

#include <climits>

namespace {

constexpr int SUITE_WAVES = 4;
constexpr int SUITE_CHUNK = SUITE_WAVES * WAVE;
constexpr int SUITE_ROW_TILE = 32;
constexpr int SUITE_ROW_BATCH = 8;
constexpr int SUITE_SLOTS = 4 * SUITE_MAX_FAMILY;

// KMNC section boundary lo + jump*s, rounded twice as fallback.kmnc_profile
// and profile_kernel round it (see the comment there): no contraction.
TIP_DEV float kmnc_bound(float lo, float jump, int s) {
#pragma clang fp contract(off)
  const float step = jump * s;
  return lo + step;
}

// Bit i of x goes to bit 2*i.
TIP_DEV unsigned long long spread_bits(unsigned int x32) {
  unsigned long long x = x32;
  x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
  x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
  x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | (x << 2)) & 0x3333333333333333ull;
  x = (x | (x << 1)) & 0x5555555555555555ull;
  return x;
}

__global__ __launch_bounds__(SUITE_CHUNK) void suite_threshold_kernel(
    const SuiteArgs a) {
  __shared__ int cnt[SUITE_SLOTS * SUITE_ROW_TILE];  // [slot][row of tile]
  const int lane = lane_id();
  const int row0 = blockIdx.x * SUITE_ROW_TILE;
  const int c0 = blockIdx.y * SUITE_CHUNK + wave_id() * WAVE;

  for (int i = threadIdx.x; i < SUITE_SLOTS * SUITE_ROW_TILE; i += SUITE_CHUNK)
    cnt[i] = 0;
  __syncthreads();

  if (c0 < a.K) {  // wave-uniform: the group holds at least one neuron
    const int col = c0 + lane;
    const bool live = col < a.K;
    const int wi = c0 >> 6;
    const int w_flat = (a.K + 63) >> 6;
    const int w_nbc = (2 * a.K + 63) >> 6;

    // column -> (layer pointer, column in the layer); a group may straddle
    // layer boundaries, so this is per lane
    const float* base = a.layer[0];
    int lcol = col, kl = a.width[0];
#pragma unroll
    for (int l = 1; l < SUITE_MAX_LAYERS; ++l) {
      if (col >= a.off[l]) {
        base = a.layer[l];
        lcol = col - a.off[l];
        kl = a.width[l];
      }
    }
    const float* ap = base + (int64_t)row0 * kl + lcol;

    // this neuron's table values, kept for every row of the tile
    float shi[SUITE_MAX_FAMILY], blo[SUITE_MAX_FAMILY], bhi[SUITE_MAX_FAMILY];
    float kjump[SUITE_MAX_FAMILY] = {0.f, 0.f, 0.f, 0.f};
    float klo = 0.f;
#pragma unroll
    for (int u = 0; u < SUITE_MAX_FAMILY; ++u) {
      shi[u] = (live && u < a.n_snac) ? a.snac_hi[(int64_t)u * a.K + col] : 0.f;
      blo[u] = (live && u < a.n_nbc) ? a.nbc_lo[(int64_t)u * a.K + col] : 0.f;
      bhi[u] = (live && u < a.n_nbc) ? a.nbc_hi[(int64_t)u * a.K + col] : 0.f;
    }
    if (a.n_kmnc > 0) {
      klo = live ? a.kmnc_lo[col] : 0.f;
      const float khi = live ? a.kmnc_hi[col] : 0.f;
#pragma unroll
      for (int u = 0; u < SUITE_MAX_FAMILY; ++u)
        kjump[u] = (u < a.n_kmnc) ? (khi - klo) / a.kmnc_sec[u] : 0.f;
    }

    for (int rb = 0; rb < SUITE_ROW_TILE; rb += SUITE_ROW_BATCH) {
      if (row0 + rb >= a.rows) break;  // wave-uniform
      float v[SUITE_ROW_BATCH];
#pragma unroll
      for (int r = 0; r < SUITE_ROW_BATCH; ++r)
        v[r] = (live && row0 + rb + r < a.rows) ? ap[(int64_t)(rb + r) * kl]
                                                : 0.f;
      // lanes 0..7 store the batch's words: lane r holds row r's
      const int myrow = row0 + rb + lane;
      const bool st = lane < SUITE_ROW_BATCH && myrow < a.rows;
      int* mycnt = cnt + rb + (lane & (SUITE_ROW_BATCH - 1));

#pragma unroll
      for (int t = 0; t < SUITE_MAX_FAMILY; ++t) {
        if (t < a.n_nac) {
          const float thr = a.nac_thr[t];
          unsigned long long w = 0ull;
#pragma unroll
          for (int r = 0; r < SUITE_ROW_BATCH; ++r) {
            const unsigned long long b = __ballot(live && v[r] > thr);
            if (lane == r) w = b;
          }
          if (st) {
            a.words[t][(int64_t)myrow * w_flat + wi] = w;
            if (w) atomicAdd(mycnt + t * SUITE_ROW_TILE, __popcll(w));
          }
        }
      }

#pragma unroll
      for (int u = 0; u < SUITE_MAX_FAMILY; ++u) {
        if (u < a.n_snac) {
          unsigned long long w = 0ull;
#pragma unroll
          for (int r = 0; r < SUITE_ROW_BATCH; ++r) {
            const unsigned long long b = __ballot(live && v[r] >= shi[u]);
            if (lane == r) w = b;
          }
          if (st) {
            a.words[SUITE_MAX_FAMILY + u][(int64_t)myrow * w_flat + wi] = w;
            if (w)
              atomicAdd(mycnt + (SUITE_MAX_FAMILY + u) * SUITE_ROW_TILE,
                        __popcll(w));
          }
        }
      }

#pragma unroll
      for (int u = 0; u < SUITE_MAX_FAMILY; ++u) {
        if (u < a.n_nbc) {
          unsigned long long wl = 0ull, wu = 0ull;
#pragma unroll
          for (int r = 0; r < SUITE_ROW_BATCH; ++r) {
            const unsigned long long bl = __ballot(live && v[r] <= blo[u]);
            const unsigned long long bu = __ballot(live && v[r] >= bhi[u]);
            if (lane == r) {
              wl = bl;
              wu = bu;
            }
          }
          if (st) {
            // bit 2*n + side: neurons 0..31 fill the first word
            unsigned long long* dst = a.words[2 * SUITE_MAX_FAMILY + u] +
                                      (int64_t)myrow * w_nbc + 2 * wi;
            dst[0] = spread_bits((unsigned int)wl) |
                     (spread_bits((unsigned int)wu) << 1);
            if (2 * wi + 1 < w_nbc)  // else neurons 32..63 are past K
              dst[1] = spread_bits((unsigned int)(wl >> 32)) |
                       (spread_bits((unsigned int)(wu >> 32)) << 1);
            const int c = __popcll(wl) + __popcll(wu);
            if (c)
              atomicAdd(mycnt + (2 * SUITE_MAX_FAMILY + u) * SUITE_ROW_TILE, c);
          }
        }
      }

#pragma unroll
      for (int u = 0; u < SUITE_MAX_FAMILY; ++u) {
        if (u < a.n_kmnc) {
          const int S = a.kmnc_sec[u];
          const float jump = kjump[u];
          const int w_kmnc = (int)(((int64_t)a.K * S + 63) >> 6);
          // bit s of m[r]: row r's activation lies in section s
          unsigned int m[SUITE_ROW_BATCH];
#pragma unroll
          for (int r = 0; r < SUITE_ROW_BATCH; ++r) m[r] = 0u;
          float b0 = kmnc_bound(klo, jump, 0);
          for (int s = 0; s < S; ++s) {
            const float b1 = kmnc_bound(klo, jump, s + 1);
#pragma unroll
            for (int r = 0; r < SUITE_ROW_BATCH; ++r)
              if (live && (b0 <= v[r]) && (v[r] < b1)) m[r] |= 1u << s;
            b0 = b1;
          }
          int c = 0;
          for (int j = 0; j < S; ++j) {
            // word j of the group: bit `lane` is section s of neuron n
            const int bit = j * WAVE + lane;
            const int n = bit / S;
            const int s = bit - n * S;
            unsigned long long w = 0ull;
#pragma unroll
            for (int r = 0; r < SUITE_ROW_BATCH; ++r) {
              const unsigned int mo = __shfl(m[r], n);
              const unsigned long long b = __ballot((mo >> s) & 1u);
              if (lane == r) w = b;
            }
            const int widx = wi * S + j;
            if (st && widx < w_kmnc) {
              a.words[3 * SUITE_MAX_FAMILY + u][(int64_t)myrow * w_kmnc + widx] = w;
              c += __popcll(w);
            }
          }
          if (st && c)
            atomicAdd(mycnt + (3 * SUITE_MAX_FAMILY + u) * SUITE_ROW_TILE, c);
        }
      }
    }
  }
  __syncthreads();

  // slot -> profile index (active slots in family order), row fastest
  for (int i = threadIdx.x; i < SUITE_SLOTS * SUITE_ROW_TILE; i += SUITE_CHUNK) {
    const int slot = i / SUITE_ROW_TILE;
    const int row = row0 + i % SUITE_ROW_TILE;
    const int fam = slot / SUITE_MAX_FAMILY, idx = slot % SUITE_MAX_FAMILY;
    const int nf = fam == 0 ? a.n_nac : fam == 1 ? a.n_snac
                 : fam == 2 ? a.n_nbc : a.n_kmnc;
    const int before = fam == 0 ? 0 : fam == 1 ? a.n_nac
                     : fam == 2 ? a.n_nac + a.n_snac
                                : a.n_nac + a.n_snac + a.n_nbc;
    const int c = cnt[i];
    if (c != 0 && idx < nf && row < a.rows)
      atomicAdd(reinterpret_cast<unsigned long long*>(a.scores) +
                    (int64_t)(before + idx) * a.rows + row,
                (unsigned long long)c);
  }
}

// Insert into a descending quad; the smaller key of each step moves on. Key
// 0 (empty) changes nothing.
TIP_DEV void topk_insert(unsigned long long (&tk)[SUITE_MAX_TOPK],
                         unsigned long long key) {
#pragma unroll
  for (int q = 0; q < SUITE_MAX_TOPK; ++q) {
    const unsigned long long hi = tk[q] > key ? tk[q] : key;
    key = tk[q] > key ? key : tk[q];
    tk[q] = hi;
  }
}

constexpr int TOPK_THREADS = 256;
constexpr int TOPK_LOADS = 4;  // independent loads per thread and step

__global__ __launch_bounds__(TOPK_THREADS) void suite_topk_kernel(
    const SuiteTopkArgs a) {
  __shared__ unsigned long long wkeys[TOPK_THREADS / WAVE][SUITE_MAX_TOPK];
  const int row = blockIdx.x;
  const int l = blockIdx.y;
  const int lane = lane_id();
  const float* base = a.layer[0];
  int kl = a.width[0], off = a.off[0];
#pragma unroll
  for (int i = 1; i < SUITE_MAX_LAYERS; ++i) {
    if (l == i) {
      base = a.layer[i];
      kl = a.width[i];
      off = a.off[i];
    }
  }
  const float* arow = base + (int64_t)row * kl;

  unsigned long long tk[SUITE_MAX_TOPK];
#pragma unroll
  for (int q = 0; q < SUITE_MAX_TOPK; ++q) tk[q] = 0ull;
  for (int c = threadIdx.x; c < kl; c += TOPK_THREADS * TOPK_LOADS) {
    float v[TOPK_LOADS];
#pragma unroll
    for (int j = 0; j < TOPK_LOADS; ++j) {
      const int cj = c + j * TOPK_THREADS;
      v[j] = cj < kl ? arow[cj] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < TOPK_LOADS; ++j) {
      const int cj = c + j * TOPK_THREADS;
      topk_insert(tk, cj < kl ? tknc_key(v[j], cj) : 0ull);
    }
  }
  // butterfly over the wave: the two sides of a step hold disjoint columns
  for (int o = 32; o >= 1; o >>= 1) {
    unsigned long long ok[SUITE_MAX_TOPK];
#pragma unroll
    for (int q = 0; q < SUITE_MAX_TOPK; ++q) ok[q] = __shfl_xor(tk[q], o);
#pragma unroll
    for (int q = 0; q < SUITE_MAX_TOPK; ++q) topk_insert(tk, ok[q]);
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < SUITE_MAX_TOPK; ++q) wkeys[wave_id()][q] = tk[q];
  }
  __syncthreads();
  if (wave_id() != 0) return;

  unsigned long long top[SUITE_MAX_TOPK];
#pragma unroll
  for (int q = 0; q < SUITE_MAX_TOPK; ++q) top[q] = 0ull;
#pragma unroll
  for (int w = 0; w < TOPK_THREADS / WAVE; ++w)
#pragma unroll
    for (int q = 0; q < SUITE_MAX_TOPK; ++q) topk_insert(top, wkeys[w][q]);
  // lane q < 4 owns the q-th largest entry of the layer
  const unsigned long long key = lane == 0   ? top[0]
                                 : lane == 1 ? top[1]
                                 : lane == 2 ? top[2]
                                             : top[3];
  // the layer's real entries outrank every empty slot, so the first
  // min(k, kl) keys are real; the column check keeps the store inside the
  // layer's bits whatever happens
  const unsigned int col = ~(unsigned int)key;
  const bool real = lane < SUITE_MAX_TOPK && key != 0ull && col < (unsigned int)kl;
  const int bit = off + (int)col;
#pragma unroll
  for (int t = 0; t < SUITE_MAX_FAMILY; ++t) {
    if (t < a.n) {
      const bool set = real && lane < a.k[t];
      if (set)
        atomicOr(&a.words[t][(int64_t)row * a.W + (bit >> 6)],
                 1ull << (bit & 63));
      const int c = __popcll(__ballot(set));
      if (lane == 0 && c)
        atomicAdd(reinterpret_cast<unsigned long long*>(a.scores[t]) + row,
                  (unsigned long long)c);
    }
  }
}

}  // namespace

int coverage_suite_chunk() { return SUITE_CHUNK; }

void launch_coverage_suite_threshold(const SuiteArgs& a, hipStream_t s) {
  dim3 grid(ceil_div(a.rows, SUITE_ROW_TILE), ceil_div(a.K, SUITE_CHUNK));
  suite_threshold_kernel<<<grid, SUITE_CHUNK, 0, s>>>(a);
}

void launch_coverage_suite_topk(const SuiteTopkArgs& a, hipStream_t s) {
  dim3 grid(a.rows, a.L);
  suite_topk_kernel<<<grid, TOPK_THREADS, 0, s>>>(a);
}
