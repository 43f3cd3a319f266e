// Device-side segment plan and gathered whitening for the sync-free grouped
// scoring path (engine/serving.py, FusedPrioritizer fast path).
//
// The grouped pairwise kernels (pairwise.hip) want the batch class-sorted and
// padded to 128-row segments. Building that layout on the host costs a
// device-to-host copy per step and a padded copy of the activation traces.
// Here the layout exists only as an index plan:
//   tseg[C+1]      padded segment offsets (multiples of 128)
//   rowmap[bp_max] padded row -> source row, -1 for pad rows / rows >= tseg[C]
//   dest[B]        source row -> padded row, -1 for an out-of-range class
// and the consumers gather source rows through rowmap. Within a class the
// source rows keep ascending order (what a stable argsort gives), and every
// value is an integer, so the plan equals the torch reference
// (ops/fallback.py: segment_plan) exactly.

#include "tip_common.h"

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4b = __attribute__((ext_vector_type(4))) float;

constexpr int PLAN_THREADS = 1024;
constexpr int PLAN_WAVES = PLAN_THREADS / WAVE;
constexpr int PLAN_MAX_C = 256;
constexpr int SEG = 128;  // segment granularity = pairwise row-block height

// One block walks the batch twice: a class histogram (integer LDS atomics),
// then a stable rank pass in tiles of PLAN_THREADS rows. Inside a tile a row's
// rank among same-class rows is (rows of earlier tiles) + (same-class rows in
// lower waves of this tile) + (same-class lower lanes of its wave).
__launch_bounds__(PLAN_THREADS) __global__ void segment_plan_kernel(
    const int64_t* __restrict__ pred, int B, int C, int bp_max,
    int* __restrict__ tseg, int* __restrict__ rowmap, int* __restrict__ dest) {
  __shared__ int running[PLAN_MAX_C];  // histogram, then rows placed so far
  __shared__ int seg[PLAN_MAX_C + 1];
  __shared__ int wcnt[PLAN_WAVES * PLAN_MAX_C];
  const int t = threadIdx.x;
  const int lane = lane_id();
  const int w = wave_id();

  for (int c = t; c < C; c += PLAN_THREADS) running[c] = 0;
  for (int p = t; p < bp_max; p += PLAN_THREADS) rowmap[p] = -1;
  __syncthreads();
#pragma unroll 4
  for (int i = t; i < B; i += PLAN_THREADS) {
    const int64_t c = pred[i];
    if (c >= 0 && c < C) atomicAdd(&running[(int)c], 1);
  }
  __syncthreads();
  if (t == 0) {
    int acc = 0;
    for (int c = 0; c < C; ++c) {
      seg[c] = acc;
      acc += (running[c] + SEG - 1) / SEG * SEG;
    }
    seg[C] = acc;
  }
  __syncthreads();
  for (int c = t; c <= C; c += PLAN_THREADS) tseg[c] = seg[c];
  for (int c = t; c < C; c += PLAN_THREADS) running[c] = 0;

  // the next tile's prediction is loaded one tile ahead, so its latency
  // hides under the current tile's rank pass
  int64_t c_next = (t < B) ? pred[t] : -1;
  for (int base = 0; base < B; base += PLAN_THREADS) {
    const int i = base + t;
    const int64_t c64 = c_next;
    const int c = (i < B && c64 >= 0 && c64 < C) ? (int)c64 : -1;
    c_next = (i + PLAN_THREADS < B) ? pred[i + PLAN_THREADS] : -1;
    for (int x = t; x < PLAN_WAVES * C; x += PLAN_THREADS) wcnt[x] = 0;
    __syncthreads();  // also orders the running[] reset / update before use
    int rank = 0;
    bool later = false;
#pragma unroll
    for (int l = 0; l < WAVE; ++l) {
      const int cl = __shfl(c, l);
      if (cl == c) {
        if (l < lane) ++rank;
        if (l > lane) later = true;
      }
    }
    if (c >= 0 && !later) wcnt[w * C + c] = rank + 1;
    __syncthreads();
    if (c >= 0) {
      int intra = running[c] + rank;
      for (int ww = 0; ww < w; ++ww) intra += wcnt[ww * C + c];
      const int p = seg[c] + intra;
      dest[i] = p;
      if (p < bp_max) rowmap[p] = i;
    } else if (i < B) {
      dest[i] = -1;
    }
    __syncthreads();
    for (int cc = t; cc < C; cc += PLAN_THREADS) {
      int s = 0;
      for (int ww = 0; ww < PLAN_WAVES; ++ww) s += wcnt[ww * C + cc];
      running[cc] += s;
    }
    __syncthreads();
  }
}

TIP_DEV float bf16_bits_to_float(short h) {
  return __uint_as_float(((unsigned)(unsigned short)h) << 16);
}

// Round-to-nearest-even fp32 -> bf16 (what a bf16 GEMM output applies).
TIP_DEV short float_to_bf16_bits(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (short)0x7fc0;  // NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (short)(u >> 16);
}

// fp32 squared norms of bf16 rows, one wave per row, fixed summation order.
// `limit` (optional, device) holds a row count: rows at or past it are left
// alone (the rows of a padded workspace beyond the last segment).
__global__ void rownorm_bf16_kernel(
    const short* __restrict__ X, int rows, int K,
    const int* __restrict__ limit, float* __restrict__ out) {
  const int row = blockIdx.x * (blockDim.x / WAVE) + wave_id();
  if (row >= rows) return;
  if (limit != nullptr && row >= *limit) return;
  const short* p = X + (int64_t)row * K;
  const int lane = lane_id();
  float s = 0.f;
  if ((K & 7) == 0) {
    for (int k8 = lane; k8 < K / 8; k8 += WAVE) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(p + k8 * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float f = bf16_bits_to_float(v[e]);
        s = fmaf(f, f, s);
      }
    }
  } else {
    for (int k = lane; k < K; k += WAVE) {
      const float f = bf16_bits_to_float(p[k]);
      s = fmaf(f, f, s);
    }
  }
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) out[row] = s;
}

// Grouped whitening: for padded row p of class c
//   white[p, n] = bf16( sum_k ats[rowmap[p], keep[c, k]] * wt[c, n, k] )
// with fp32 accumulation on v_mfma_f32_16x16x32_bf16. One block = 64 padded
// rows (half a 128-aligned segment, so one class) x ALL output columns: the
// scattered source columns are gathered exactly once, the whole [64, KP]
// operand tile into LDS with every load in flight together (consecutive
// threads read ascending kept columns of one row). The per-class matrix is
// stored zero-padded and K-contiguous as wt[C, NP, KP] (NP, KP multiples of
// 16 / 32), so each lane's B fragment is one aligned 16-byte load from L2 and
// needs no staging. Wave w owns rows 16w..16w+15 and NT 16-column tiles.
// Fragment layout as in the bf16 pairwise kernel: A lane l holds row l&15,
// k = (l>>4)*8+e; B lane l holds output column l&15, same k; D row =
// (l>>4)*4+reg, col = l&15. Blocks of classes without a fused KDE (empty
// whitened-train range) and blocks past tseg[C] return at once: their rows
// of `white` are never read.
constexpr int WROWS = 64;        // padded rows per block
constexpr int WKP_MAX = 320;     // widest supported (padded) K
constexpr int WAROW = WKP_MAX + 8;  // LDS halves per A row (bank spread)

template <int NT>
__launch_bounds__(256) __global__ void grouped_whiten_bf16_kernel(
    const short* __restrict__ ats,    // [B, D] bf16 source rows
    int B, int D,
    const int* __restrict__ rowmap,   // [bp_max]
    const int* __restrict__ tseg,     // [C+1]
    const int* __restrict__ wseg,     // [C+1] whitened-train offsets
    int nclasses,
    const int* __restrict__ keep,     // [C, d] kept source columns
    const short* __restrict__ wt,     // [C, NP, KP] bf16, zero-padded
    int d, int NP, int KP,
    short* __restrict__ white) {      // [bp_max, d] bf16
  __shared__ short As[WROWS * WAROW];
  __shared__ int skeep[WKP_MAX];
  __shared__ int srow[WROWS];

  const int row0 = blockIdx.x * WROWS;
  if (row0 >= tseg[nclasses]) return;
  int cls = 0;
  for (int c = 0; c < nclasses; ++c)
    if (tseg[c] <= row0) cls = c;
  if (wseg[cls + 1] <= wseg[cls]) return;

  const int t = threadIdx.x;
  if (t < WROWS) {
    const int s = rowmap[row0 + t];
    srow[t] = (s >= 0 && s < B) ? s : -1;
  }
  for (int k = t; k < KP; k += 256)
    skeep[k] = (k < d) ? keep[(int64_t)cls * d + k] : -1;
  __syncthreads();

  const int lane = lane_id();
  const int wid = wave_id();

  // Gather the whole A tile (zeros for pad rows and for k >= d). Wave w
  // fills its own 16 rows; a lane walks the kept columns k = lane, lane+64,
  // ... and loads 8 rows per batch. Every load is unconditional (indices
  // clamped to row 0 / column 0, the value selected afterwards), so the
  // batch stays in flight together instead of one branch + wait per element.
  for (int k = lane; k < KP; k += WAVE) {
    const int col = skeep[k];
    const int colc = col < 0 ? 0 : col;
#pragma unroll
    for (int rb = 0; rb < 16; rb += 8) {
      short v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int src = srow[wid * 16 + rb + u];
        const short x = ats[(int64_t)(src < 0 ? 0 : src) * D + colc];
        v[u] = (src >= 0 && col >= 0) ? x : (short)0;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) As[(wid * 16 + rb + u) * WAROW + k] = v[u];
    }
  }
  __syncthreads();

  const int fj = lane & 15;
  const int fg = lane >> 4;
  const short* wc = wt + (int64_t)cls * NP * KP;

  f32x4b acc[NT] = {};
  for (int k0 = 0; k0 < KP; k0 += 32) {
    const bf16x8 af = *reinterpret_cast<const bf16x8*>(
        &As[(wid * 16 + fj) * WAROW + k0 + fg * 8]);
#pragma unroll
    for (int tc = 0; tc < NT; ++tc) {
      if (tc * 16 < NP) {
        const bf16x8 bf = *reinterpret_cast<const bf16x8*>(
            &wc[(int64_t)(tc * 16 + fj) * KP + k0 + fg * 8]);
        acc[tc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc[tc], 0,
                                                          0, 0);
      }
    }
  }

#pragma unroll
  for (int tc = 0; tc < NT; ++tc) {
    const int col = tc * 16 + fj;
    if (col >= d) continue;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = row0 + wid * 16 + fg * 4 + reg;
      white[(int64_t)row * d + col] = float_to_bf16_bits(acc[tc][reg]);
    }
  }
}

// Grouped centring for the Gaussian scorers (pairwise.hip,
// grouped_quad_kernel): for padded row p of group g and component slot s
//   dc[s][p][:] = float(x[rowmap[p]][:]) - means[comp_off[g] + s][:]
// and zeros for pad rows and for slots the group does not have, so the tile
// main loop needs no gather and no mean. One wave per (slot, padded row);
// rows at or past tseg[G] belong to no group and are never read, so they are
// skipped. Memory-bound: 16-byte stores (and fp32 loads) where D % 4 == 0.
// The difference is taken in fp32 on the (exact) widened input, which is the
// value the oracle centres too.
template <bool BF16>
__launch_bounds__(256) __global__ void grouped_center_kernel(
    const void* __restrict__ xv,       // [B, D] fp32 or bf16 source rows
    int B, int D,
    const int* __restrict__ rowmap,    // [Bp]
    const int* __restrict__ tseg,      // [G+1]
    const int* __restrict__ comp_off,  // [G+1]
    int ngroups, int Bp,
    const float* __restrict__ means,   // [J, D]
    float* __restrict__ dc) {          // [S, Bp, D]
  const int p = blockIdx.x * (blockDim.x / WAVE) + wave_id();
  const int s = blockIdx.y;
  if (p >= Bp || p >= tseg[ngroups]) return;
  int g = 0;
  for (int c = 0; c < ngroups; ++c)
    if (tseg[c] <= p) g = c;
  int src = rowmap[p];
  if (src >= B) src = -1;
  const bool live = src >= 0 && s < comp_off[g + 1] - comp_off[g];
  float* o = dc + ((int64_t)s * Bp + p) * D;
  const int lane = lane_id();
  const float* mu = means + (int64_t)(live ? comp_off[g] + s : 0) * D;
  const float* xf =
      static_cast<const float*>(xv) + (int64_t)(live ? src : 0) * D;
  const short* xh =
      static_cast<const short*>(xv) + (int64_t)(live ? src : 0) * D;
  if ((D & 3) == 0) {
    for (int k4 = lane; k4 < D / 4; k4 += WAVE) {
      float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
      if (live) {
        const float4 m = *reinterpret_cast<const float4*>(mu + k4 * 4);
        float4 v;
        if (BF16) {
          const short4 h = *reinterpret_cast<const short4*>(xh + k4 * 4);
          v = make_float4(bf16_bits_to_float(h.x), bf16_bits_to_float(h.y),
                          bf16_bits_to_float(h.z), bf16_bits_to_float(h.w));
        } else {
          v = *reinterpret_cast<const float4*>(xf + k4 * 4);
        }
        r = make_float4(v.x - m.x, v.y - m.y, v.z - m.z, v.w - m.w);
      }
      *reinterpret_cast<float4*>(o + k4 * 4) = r;
    }
  } else {
    for (int k = lane; k < D; k += WAVE) {
      float r = 0.f;
      if (live) r = (BF16 ? bf16_bits_to_float(xh[k]) : xf[k]) - mu[k];
      o[k] = r;
    }
  }
}

// ---- host-side launchers (called from bindings.cpp) ----

void launch_grouped_center(const void* x, bool bf16, int b, int d,
                           const int* rowmap, const int* tseg,
                           const int* comp_off, int ngroups, int bp,
                           const float* means, int slots, float* dc,
                           hipStream_t s) {
  const int wpb = 4;
  dim3 grid(ceil_div(bp, wpb), slots);
  if (bf16) {
    grouped_center_kernel<true><<<grid, wpb * WAVE, 0, s>>>(
        x, b, d, rowmap, tseg, comp_off, ngroups, bp, means, dc);
  } else {
    grouped_center_kernel<false><<<grid, wpb * WAVE, 0, s>>>(
        x, b, d, rowmap, tseg, comp_off, ngroups, bp, means, dc);
  }
}

int segment_plan_max_classes() { return PLAN_MAX_C; }

void launch_segment_plan(const int64_t* pred, int b, int c, int bp_max,
                         int* tseg, int* rowmap, int* dest, hipStream_t s) {
  segment_plan_kernel<<<1, PLAN_THREADS, 0, s>>>(pred, b, c, bp_max, tseg,
                                                 rowmap, dest);
}

void launch_rownorm_bf16(const short* x, int rows, int k, const int* limit,
                         float* out, hipStream_t s) {
  const int wpb = 4;
  rownorm_bf16_kernel<<<ceil_div(rows, wpb), wpb * WAVE, 0, s>>>(
      x, rows, k, limit, out);
}

int grouped_whiten_max_features() { return WKP_MAX; }

void launch_grouped_whiten_bf16(const short* ats, int b, int dfull,
                                const int* rowmap, const int* tseg,
                                const int* wseg, int nclasses, const int* keep,
                                const short* wt, int d, int np, int kp,
                                int bp_max, short* white, hipStream_t s) {
  const int grid = bp_max / WROWS;
  if (np <= 64) {
    grouped_whiten_bf16_kernel<4><<<grid, 256, 0, s>>>(
        ats, b, dfull, rowmap, tseg, wseg, nclasses, keep, wt, d, np, kp,
        white);
  } else {
    grouped_whiten_bf16_kernel<WKP_MAX / 16><<<grid, 256, 0, s>>>(
        ats, b, dfull, rowmap, tseg, wseg, nclasses, keep, wt, d, np, kp,
        white);
  }
}
