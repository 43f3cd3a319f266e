// MFMA pairwise-distance kernel family for gfx950 (CDNA4).
//
// The workload's hot core: squared L2 distances
// between a test-AT matrix A [M,K] and a train-AT matrix B [N,K], computed
// as ||a||^2 + ||b||^2 - 2 a.b with the Gram matrix on the f32-input MFMA
// (v_mfma_f32_32x32x2_f32: exact fp32 fmaf-chain numerics at the 157 TF f32
// peak), staged through LDS in k-major tiles, with three fused epilogues:
//   EPI_FULL   - write the D tile            (silhouette, debugging)
//   EPI_ROWMIN - per-row min + argmin        (DSA, kmeans assign)
//   EPI_KDE    - per-row online logsumexp(-d/2) partials (LSA KDE)
// Per-(block-column) partials are combined by small deterministic
// second-pass kernels so 1-GPU and sharded runs are bitwise reproducible.
//
// Geometry: 256 threads = 4 waves as 2x2; block tile 128x128, K-step 32;
// each wave owns a 64x64 sub-tile = 2x2 MFMA 32x32 accumulators.
//
// Structure. A kernel is index computation around shared device code, each
// piece of which exists once:
//   tile_mainloop_f32    fp32 staging + MFMA loop of one 128x128 tile
//   tile_epilogue_f32    fp32 per-row epilogue (distance, clamp, half-wave
//                        reduction into red_*), then merge_halves_store
//   merge_halves_store   merges the two 64-column halves of a block row
//                        (kde_merge_pair for KDE) and writes the partial;
//                        the fp32 kernels and the bf16 kernel all end in it
//   fold_rowmin/fold_kde fold the column-block partials of one row, bj
//                        ascending; all six combine kernels call them
//   class_of_row         class of a padded row from the segment table
//   tile_epilogue_quad   EPI_QUAD: per-row sum of (tile .* centred row), for
//                        grouped_quad_kernel (Gaussian quadratic forms); it
//                        shares the main loop and merge_halves_store
//   silhouette_sums_kernel  x against itself; its epilogue adds the tile's
//                        distances into per-row cluster bins instead of
//                        writing them (batched k-means discovery)
// pairwise_kernel (flat: XCD swizzle, EPI_FULL) and grouped_pairwise_kernel
// (class segments) differ only in how a block finds its tile and its bounds,
// so a grouped result equals the per-class flat result bit for bit, and the
// plan-driven *_final_kernels fold exactly as the *_combine_kernels do.
// grouped_pairwise_bf16_kernel keeps a main loop and per-row epilogue of its
// own (16x16x32 bf16 MFMA, another fragment layout). Where one variant
// behaves differently from its siblings, a comment at that line says so.

#include "tip_common.h"

#include <cfloat>
#include <cmath>

using f32x16 = __attribute__((__vector_size__(16 * sizeof(float)))) float;

constexpr int BM = 128;
constexpr int BN = 128;
constexpr int BK = 32;
constexpr int LDS_PAD = 4;  // pad k-major rows to de-conflict staging writes

enum Epilogue { EPI_FULL = 0, EPI_ROWMIN = 1, EPI_KDE = 2, EPI_QUAD = 3 };

// Staging is split T14-style (issue-early / write-late): the global loads
// for tile t+1 are issued into registers BEFORE tile t's MFMA loop (HBM
// latency hides under the ~4k-cycle f32-MFMA compute phase) and the LDS
// write pass runs after the barrier. LDS image is k-major
// lds[BK][BM+pad]: lds[k][r] = src[row0+r][k0+k]; 256 threads, 16 floats
// each (4x float4).

struct StageRegs {
  float4 v[4];
};

TIP_DEV StageRegs stage_load(
    const float* __restrict__ src, int rows, int K, int row0, int k0) {
  StageRegs sr;
  const int t = threadIdx.x;
  const int r = t >> 1;                 // 0..127
  const int kq = (t & 1) * (BK / 2);    // 0 or 16
  const int grow = row0 + r;
  const bool row_ok = grow < rows;
#pragma unroll
  for (int q4 = 0; q4 < 4; ++q4) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    const int gk = k0 + kq + q4 * 4;
    // float4 path only when rows are 16B-aligned (K % 4 == 0)
    if (row_ok && gk + 3 < K && (K & 3) == 0) {
      v = *reinterpret_cast<const float4*>(&src[(int64_t)grow * K + gk]);
    } else if (row_ok) {
      // K tail: scalar guarded loads (zeros contribute nothing to the dot)
      float tmp[4] = {0.f, 0.f, 0.f, 0.f};
      for (int e = 0; e < 4; ++e)
        if (gk + e < K) tmp[e] = src[(int64_t)grow * K + gk + e];
      v = make_float4(tmp[0], tmp[1], tmp[2], tmp[3]);
    }
    sr.v[q4] = v;
  }
  return sr;
}

TIP_DEV void stage_write(float* lds, const StageRegs& sr) {
  const int t = threadIdx.x;
  const int r = t >> 1;
  const int kq = (t & 1) * (BK / 2);
#pragma unroll
  for (int q4 = 0; q4 < 4; ++q4) {
    lds[(kq + q4 * 4 + 0) * (BM + LDS_PAD) + r] = sr.v[q4].x;
    lds[(kq + q4 * 4 + 1) * (BM + LDS_PAD) + r] = sr.v[q4].y;
    lds[(kq + q4 * 4 + 2) * (BM + LDS_PAD) + r] = sr.v[q4].z;
    lds[(kq + q4 * 4 + 3) * (BM + LDS_PAD) + r] = sr.v[q4].w;
  }
}

// The wave's 64x64 sub-tile of A.B^T: t[m][n] is the 32x32 accumulator of
// row half m, column half n.
struct TileAcc {
  f32x16 t[2][2];
};

// fp32 main loop of the block tile at (row0, col0). T14 pipeline: the
// prologue stages tile 0; each iteration issues tile t+1's global loads
// before tile t's MFMAs and writes them to LDS afterwards. Rows of A at or
// past a_rows and rows of B at or past b_rows stage zeros.
TIP_DEV TileAcc tile_mainloop_f32(
    const float* __restrict__ A, int a_rows, const float* __restrict__ B,
    int b_rows, int K, int row0, int col0, float* As, float* Bs) {
  const int lane = lane_id();
  const int wr = wave_id() >> 1;  // wave row (0..1) -> 64 rows
  const int wc = wave_id() & 1;   // wave col (0..1) -> 64 cols

  TileAcc acc = {};
  StageRegs ra = stage_load(A, a_rows, K, row0, 0);
  StageRegs rb = stage_load(B, b_rows, K, col0, 0);
  stage_write(As, ra);
  stage_write(Bs, rb);
  __syncthreads();

  for (int k0 = 0; k0 < K; k0 += BK) {
    const bool has_next = (k0 + BK) < K;
    if (has_next) {
      ra = stage_load(A, a_rows, K, row0, k0 + BK);
      rb = stage_load(B, b_rows, K, col0, k0 + BK);
    }
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      const int k = kk + (lane >> 5);
      const float* as = &As[k * (BM + LDS_PAD) + wr * 64 + (lane & 31)];
      const float* bs = &Bs[k * (BM + LDS_PAD) + wc * 64 + (lane & 31)];
      const float a0 = as[0], a1 = as[32];
      const float b0 = bs[0], b1 = bs[32];
      acc.t[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc.t[0][0], 0, 0, 0);
      acc.t[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc.t[0][1], 0, 0, 0);
      acc.t[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc.t[1][0], 0, 0, 0);
      acc.t[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc.t[1][1], 0, 0, 0);
    }
    __syncthreads();  // all reads of tile t done
    if (has_next) {
      stage_write(As, ra);
      stage_write(Bs, rb);
    }
    __syncthreads();  // tile t+1 visible
  }
  return acc;
}

// Streaming-logsumexp merge of two (max, sum) pairs; a pair with sum 0 is
// empty and its max is not looked at.
TIP_DEV float2 kde_merge_pair(float m0, float s0, float m1, float s1) {
  if (m0 >= m1)
    return make_float2(m0, s0 + ((s1 > 0.f) ? s1 * __expf(m1 - m0) : 0.f));
  return make_float2(m1, s1 + ((s0 > 0.f) ? s0 * __expf(m0 - m1) : 0.f));
}

// Merge the two 64-column halves of every block row (red_*[r][wc]; wc = 0
// covers the lower columns, so ties prefer it) and store the block's partial
// for column block bj. Rows at or past row_end store nothing. The caller has
// put a barrier between the writes to red_* and this call.
template <int EPI>
TIP_DEV void merge_halves_store(
    const float (*red_v)[2], const int (*red_i)[2], const float (*red_s)[2],
    int row0, int row_end, int stride, int bj, float* __restrict__ pmin_val,
    int* __restrict__ pmin_idx, float2* __restrict__ pkde) {
  for (int r = threadIdx.x; r < BM; r += blockDim.x) {
    const int i = row0 + r;
    if (i >= row_end) continue;
    if (EPI == EPI_ROWMIN) {
      const MinIdx best = min_idx_combine(
          MinIdx{red_v[r][0], red_i[r][0]}, MinIdx{red_v[r][1], red_i[r][1]});
      pmin_val[(int64_t)bj * stride + i] = best.v;
      pmin_idx[(int64_t)bj * stride + i] = best.i;
    } else if (EPI == EPI_QUAD) {
      // plain sum, low half first; the partial goes where ROWMIN's value does
      pmin_val[(int64_t)bj * stride + i] = red_v[r][0] + red_v[r][1];
    } else {
      pkde[(int64_t)bj * stride + i] =
          kde_merge_pair(red_v[r][0], red_s[r][0], red_v[r][1], red_s[r][1]);
    }
  }
}

// fp32 epilogue of the block tile at (row0, col0): distances of rows below
// row_end against columns below col_end, then the EPI's output. EPI_FULL
// writes the [row_end, col_end] matrix out_full; the others write the
// partial of column block bj, [*, stride].
// C/D layout of v_mfma_f32_32x32x2_f32 (standard 32x32 map):
//   col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
template <int EPI>
TIP_DEV void tile_epilogue_f32(
    const TileAcc& acc, const float* __restrict__ anorm,
    const float* __restrict__ bnorm, int row0, int row_end, int col0,
    int col_end, int stride, int bj, float (*red_v)[2], int (*red_i)[2],
    float (*red_s)[2], float* __restrict__ out_full,
    float* __restrict__ pmin_val, int* __restrict__ pmin_idx,
    float2* __restrict__ pkde) {
  const int lane = lane_id();
  const int wr = wave_id() >> 1;
  const int wc = wave_id() & 1;
  const int jl0 = col0 + wc * 64 + (lane & 31);  // n=0 column
  // differs from the bf16 epilogue, which reads bnorm per tile column
  // inside the range guard
  const float bn0 = (jl0 < col_end) ? bnorm[jl0] : 0.f;
  const float bn1 = (jl0 + 32 < col_end) ? bnorm[jl0 + 32] : 0.f;

#pragma unroll
  for (int m = 0; m < 2; ++m) {
    // process the 16 regs; rows repeat across n, so handle n jointly
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row_local = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
      const int block_row = wr * 64 + m * 32 + row_local;
      const int i = row0 + block_row;
      const float an = (i < row_end) ? anorm[i] : 0.f;
      float d0 = an + bn0 - 2.f * acc.t[m][0][reg];
      float d1 = an + bn1 - 2.f * acc.t[m][1][reg];
      d0 = fmaxf(d0, 0.f);
      d1 = fmaxf(d1, 0.f);
      if (jl0 >= col_end) d0 = FLT_MAX;
      if (jl0 + 32 >= col_end) d1 = FLT_MAX;

      if (EPI == EPI_FULL) {
        if (i < row_end) {
          if (jl0 < col_end) out_full[(int64_t)i * col_end + jl0] = d0;
          if (jl0 + 32 < col_end)
            out_full[(int64_t)i * col_end + jl0 + 32] = d1;
        }
      } else if (EPI == EPI_ROWMIN) {
        MinIdx mi{d0, jl0};
        mi = min_idx_combine(mi, MinIdx{d1, jl0 + 32});
        mi = half_reduce_min(mi);
        if ((lane & 31) == 0) {
          red_v[block_row][wc] = mi.v;
          red_i[block_row][wc] = mi.i;
        }
      } else {  // EPI_KDE: per-row max of t=-d/2 and sum exp(t - max)
        MinIdx mi{d0, 0};
        mi = min_idx_combine(mi, MinIdx{d1, 0});
        mi = half_reduce_min(mi);
        // = max_j(-d/2) over these 64 cols. Differs from the bf16 epilogue:
        // a half with no column in range gives -0.5f * FLT_MAX here
        const float tmax = -0.5f * mi.v;
        float s = 0.f;
        if (d0 != FLT_MAX) s += __expf(-0.5f * d0 - tmax);
        if (d1 != FLT_MAX) s += __expf(-0.5f * d1 - tmax);
        s = half_reduce_sum(s);
        if ((lane & 31) == 0) {
          red_v[block_row][wc] = tmax;
          red_s[block_row][wc] = s;
        }
      }
    }
  }

  if (EPI == EPI_FULL) return;
  __syncthreads();
  merge_halves_store<EPI>(red_v, red_i, red_s, row0, row_end, stride, bj,
                          pmin_val, pmin_idx, pkde);
}

// EPI_QUAD epilogue of the block tile at (row0, col0), for A = centred rows
// d [row_end, ncols] and B = one symmetric matrix M: the tile holds (d.M) and
// the row's partial quadratic form is sum_j (d.M)[r][j] * d[r][j] over the
// tile's columns. `a` is the matrix-local origin of d (row i, local column j
// at a[i * ncols + j]); lcol0 is the tile's first local column. Columns at
// or past ncols contribute zero (their accumulators are zero as well: B
// staged zeros there). Same C/D layout as tile_epilogue_f32. Summation
// order is fixed: n = 0 then n = 1 in the lane, the 32-lane xor tree, the
// low 64-column half before the high one.
TIP_DEV void tile_epilogue_quad(
    const TileAcc& acc, const float* __restrict__ a, int ncols, int row0,
    int row_end, int lcol0, int stride, int bj, float (*red_v)[2],
    float* __restrict__ pquad) {
  const int lane = lane_id();
  const int wr = wave_id() >> 1;
  const int wc = wave_id() & 1;
  const int jl0 = lcol0 + wc * 64 + (lane & 31);  // n=0 local column
  const bool ok0 = jl0 < ncols;
  const bool ok1 = jl0 + 32 < ncols;

#pragma unroll
  for (int m = 0; m < 2; ++m) {
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row_local = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
      const int block_row = wr * 64 + m * 32 + row_local;
      const int i = row0 + block_row;
      const bool row_ok = i < row_end;
      const float* ar = a + (int64_t)(row_ok ? i : 0) * ncols;
      const float d0 = (row_ok && ok0) ? ar[jl0] : 0.f;
      const float d1 = (row_ok && ok1) ? ar[jl0 + 32] : 0.f;
      float s = acc.t[m][0][reg] * d0;
      s += acc.t[m][1][reg] * d1;
      s = half_reduce_sum(s);
      if ((lane & 31) == 0) red_v[block_row][wc] = s;
    }
  }
  __syncthreads();
  merge_halves_store<EPI_QUAD>(red_v, nullptr, nullptr, row0, row_end, stride,
                               bj, pquad, nullptr, nullptr);
}

// Class of padded row `row`: the last class whose segment starts at or
// before it (segments are 128-aligned, so one row block is one class).
TIP_DEV int class_of_row(const int* __restrict__ tseg, int nclasses, int row) {
  int cls = 0;
  for (int c = 0; c < nclasses; ++c)
    if (tseg[c] <= row) cls = c;
  return cls;
}

template <int EPI>
__launch_bounds__(256, 2) __global__ void pairwise_kernel(
    const float* __restrict__ A,      // [M, K]
    const float* __restrict__ B,      // [N, K]
    const float* __restrict__ anorm,  // [M] row squared norms
    const float* __restrict__ bnorm,  // [N]
    int M, int N, int K,
    float* __restrict__ out_full,     // EPI_FULL: [M, N]
    float* __restrict__ pmin_val,     // EPI_ROWMIN: [jblocks, M]
    int* __restrict__ pmin_idx,       //             [jblocks, M]
    float2* __restrict__ pkde) {      // EPI_KDE:   [jblocks, M] (max, sum)
  __shared__ float lds[2 * BK * (BM + LDS_PAD)];
  // reduction scratch: per block row x 2 column-halves
  __shared__ float red_v[BM][2];
  __shared__ int red_i[BM][2];
  __shared__ float red_s[BM][2];

  // XCD-aware block swizzle (T1, bijective form): consecutive remapped ids
  // land on one XCD and share the A panel in that XCD's L2.
  int bi, bj;
  {
    const int nwg = gridDim.x * gridDim.y;
    const int id = blockIdx.y * gridDim.x + blockIdx.x;
    const int q = nwg / 8, r = nwg % 8;
    const int xcd = id % 8, pos = id / 8;
    const int newid =
        (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
    bi = newid / gridDim.x;
    bj = newid % gridDim.x;
  }
  const int row0 = bi * BM;
  const int col0 = bj * BN;

  const TileAcc acc = tile_mainloop_f32(A, M, B, N, K, row0, col0, lds,
                                        lds + BK * (BM + LDS_PAD));
  tile_epilogue_f32<EPI>(acc, anorm, bnorm, row0, M, col0, N, M, bj, red_v,
                         red_i, red_s, out_full, pmin_val, pmin_idx, pkde);
}

// ---------------------------------------------------------------------------
// Grouped (segmented) variant: test rows are sorted by class and padded to
// 128-row segments (tseg offsets, C+1 entries); train rows are the
// class-concatenated set with raw offsets (nseg). One launch covers every
// class. Each block derives its class from its row-block (segments are
// 128-aligned), and only columns inside the class's train range
// participate. Argmin indices are GLOBAL train rows, so the precomputed DSA
// b-table gathers directly. Column block fast, row block slow: the mapping
// kept from the sweep in profiles/r02_grouped_mapping_sweep.md.
// ---------------------------------------------------------------------------

template <int EPI>
__launch_bounds__(256, 2) __global__ void grouped_pairwise_kernel(
    const float* __restrict__ A,      // [Bp, K] class-sorted, 128-padded
    const float* __restrict__ B,      // [Ntot, K] class-concatenated
    const float* __restrict__ anorm,  // [Bp]
    const float* __restrict__ bnorm,  // [Ntot]
    const int* __restrict__ tseg,     // [C+1] padded test offsets (x128)
    const int* __restrict__ nseg,     // [C+1] train offsets
    int nclasses, int Bp, int K,
    float* __restrict__ pmin_val,     // [jb_max, Bp]
    int* __restrict__ pmin_idx,
    float2* __restrict__ pkde) {
  __shared__ float lds[2 * BK * (BM + LDS_PAD)];
  __shared__ float red_v[BM][2];
  __shared__ int red_i[BM][2];
  __shared__ float red_s[BM][2];

  const int bj = blockIdx.x;
  const int row0 = blockIdx.y * BM;
  if (row0 >= Bp) return;
  const int cls = class_of_row(tseg, nclasses, row0);
  const int ncol1 = nseg[cls + 1];
  const int col0 = nseg[cls] + bj * BN;
  if (col0 >= ncol1) return;  // this class has fewer column blocks

  const TileAcc acc = tile_mainloop_f32(A, Bp, B, ncol1, K, row0, col0, lds,
                                        lds + BK * (BM + LDS_PAD));
  tile_epilogue_f32<EPI>(acc, anorm, bnorm, row0, Bp, col0, ncol1, Bp, bj,
                         red_v, red_i, red_s, nullptr, pmin_val, pmin_idx,
                         pkde);
}

// ---------------------------------------------------------------------------
// Grouped Gaussian quadratic forms (pc-MDSA / pc-MLSA / pc-MMDSA scoring).
// Padded row p of group g holds, per component slot s, the centred row
// dc[s][p][:] = x - mean[comp_off[g] + s] (segment.hip). The "train side" is
// the stack of all precision matrices, mats [J * D, D]: each is symmetric,
// so its rows are its columns and the tile of A.B^T against rows
// [j * D, (j + 1) * D) is (d . M_j). Grid: x = column blocks of D, y = row
// blocks of the padded batch, z = component slot. Exact fp32 only (the
// dynamic range of near-singular precisions is not validated for bf16
// operands). Partials: pquad[(s * gridDim.x + bj) * Bp + p].
// ---------------------------------------------------------------------------

__launch_bounds__(256, 2) __global__ void grouped_quad_kernel(
    const float* __restrict__ dc,        // [S, Bp, D] centred rows
    const float* __restrict__ mats,      // [J * D, D] symmetric matrices
    const int* __restrict__ tseg,        // [G+1] padded row offsets (x128)
    const int* __restrict__ comp_off,    // [G+1] first component of a group
    int ngroups, int Bp, int D,
    float* __restrict__ pquad) {         // [S, jb, Bp]
  __shared__ float lds[2 * BK * (BM + LDS_PAD)];
  __shared__ float red_v[BM][2];

  const int bj = blockIdx.x;
  const int row0 = blockIdx.y * BM;
  const int s = blockIdx.z;
  if (row0 >= Bp || row0 >= tseg[ngroups]) return;
  const int g = class_of_row(tseg, ngroups, row0);
  if (s >= comp_off[g + 1] - comp_off[g]) return;
  const int mrow0 = (comp_off[g] + s) * D;  // first row of this matrix
  const float* a = dc + (int64_t)s * Bp * D;

  const TileAcc acc =
      tile_mainloop_f32(a, Bp, mats, mrow0 + D, D, row0, mrow0 + bj * BN, lds,
                        lds + BK * (BM + LDS_PAD));
  tile_epilogue_quad(acc, a, D, row0, Bp, bj * BN, Bp, s * gridDim.x + bj,
                     red_v, pquad);
}

// Folds the column-block partials of each (slot, padded row) in ascending bj
// and writes the row's final score to its source row. mode 0: the quadratic
// form of slot 0 (Mahalanobis). mode 1: -logsumexp_s(logc - q / 2) over the
// group's slots (mixture NLL), with accurate expf / logf. A group without
// components scores +inf; pad rows and rows at or past tseg[ngroups] write
// nothing (`out` is pre-filled with +inf by the caller).
constexpr int QUAD_MAX_SLOTS = 8;

__global__ void grouped_gauss_final_kernel(
    const float* __restrict__ pquad, const int* __restrict__ tseg,
    const int* __restrict__ comp_off, int ngroups, int Bp, int jb,
    const int* __restrict__ rowmap, int out_rows,
    const float* __restrict__ logc,  // [J], mode 1 only
    int mode, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Bp || i >= tseg[ngroups]) return;
  const int src = rowmap[i];
  if (src < 0 || src >= out_rows) return;
  const int g = class_of_row(tseg, ngroups, i);
  const int c0 = comp_off[g];
  int ncomp = comp_off[g + 1] - c0;
  if (ncomp > QUAD_MAX_SLOTS) ncomp = QUAD_MAX_SLOTS;
  if (ncomp <= 0) {
    out[src] = INFINITY;
    return;
  }
  float t[QUAD_MAX_SLOTS];
  float tmax = -INFINITY;
#pragma unroll
  for (int s = 0; s < QUAD_MAX_SLOTS; ++s) {
    t[s] = -INFINITY;
    if (s < ncomp) {
      float q = 0.f;
      for (int b = 0; b < jb; ++b) q += pquad[((int64_t)s * jb + b) * Bp + i];
      t[s] = (mode == 0) ? q : (logc[c0 + s] - 0.5f * q);
      tmax = fmaxf(tmax, t[s]);
    }
  }
  if (mode == 0) {
    out[src] = t[0];
    return;
  }
  if (!(tmax > -INFINITY && tmax < INFINITY)) {
    // every component underflowed to -inf (score +inf), or a NaN / +inf term
    out[src] = (tmax == -INFINITY) ? INFINITY : -tmax;
    return;
  }
  float sum = 0.f;
#pragma unroll
  for (int s = 0; s < QUAD_MAX_SLOTS; ++s)
    if (s < ncomp) sum += expf(t[s] - tmax);
  out[src] = -(tmax + logf(sum));
}

// ---------------------------------------------------------------------------
// bf16 grouped variant (fp32 accumulate). The activation traces come out of
// a bf16 forward, so bf16 operands lose almost nothing while the MFMA
// throughput ceiling rises ~16x over v_mfma_f32_32x32x2_f32 (the fp32 path
// measured ~95-119 TF; dense bf16 peak is ~2.5 PF). Fragment layout is the
// one hardware-verified by mfma_probe (resnet_fused.hip): A lane l holds
// A[i=l&15][k=(l>>4)*8+e]; B lane l holds B-col[j=l&15][same k]; D row =
// (l>>4)*4+reg, col = l&15. LDS tiles are [128][BROW] halves. ds_read_b128
// is served in four groups of 16 lanes that are NOT contiguous ({0-3, 12-15,
// 20-27}, ...), so a group spans two fg values: the 5-unit row stride of
// BROW = 40 is coprime to the 16-unit bank row only within one fg, and the
// fragment reads are 2-way conflicted (as at 56 and 72; 48 models
// conflict-free). The pipelined kernel below uses unpadded 128-B rows with
// an XOR swizzle instead. Partial outputs are identical in format to the
// fp32 grouped kernel, so the same combine kernels run afterwards.
// ---------------------------------------------------------------------------

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4b = __attribute__((ext_vector_type(4))) float;

constexpr int BBK = 32;             // k per MFMA / staging step
// LDS halves per tile row. Must be a multiple of 8 (16-B-aligned b128
// reads); the pad past BBK sets the bank-group stride of the fragment
// gathers. TIP_BROW is sweepable on hardware (40 = 5-unit stride default;
// profiles/r10_rowmin_pipeline.md has the sweep against 48).
#ifndef TIP_BROW
#define TIP_BROW 40
#endif
constexpr int BROW = TIP_BROW;

// Stage a [128, 32] bf16 tile: thread t loads row r = t>>1, halves
// kq = (t&1)*16 .. +15 (two 16-B units); OOB rows/ks stage zeros.
struct BStage {
  bf16x8 v[2];
};

// `grow` is the source row to stage and `ok` whether it exists at all.
TIP_DEV BStage bstage_load_row(const short* __restrict__ src, int grow,
                               bool ok, int K, int k0) {
  BStage s;
  const int kq = (threadIdx.x & 1) * 16;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int gk = k0 + kq + h * 8;
    if (ok && gk + 7 < K) {
      s.v[h] = *reinterpret_cast<const bf16x8*>(&src[(int64_t)grow * K + gk]);
    } else if (ok) {
      bf16x8 tmp = zero;
      for (int e = 0; e < 8; ++e)
        if (gk + e < K) tmp[e] = src[(int64_t)grow * K + gk + e];
      s.v[h] = tmp;
    } else {
      s.v[h] = zero;
    }
  }
  return s;
}

TIP_DEV BStage bstage_load(const short* __restrict__ src, int rows, int K,
                           int row0, int k0) {
  const int grow = row0 + (threadIdx.x >> 1);
  return bstage_load_row(src, grow, grow < rows, K, k0);
}

TIP_DEV void bstage_write(short* lds, const BStage& s) {
  const int t = threadIdx.x;
  const int r = t >> 1;
  const int kq = (t & 1) * 16;
  *reinterpret_cast<bf16x8*>(&lds[r * BROW + kq]) = s.v[0];
  *reinterpret_cast<bf16x8*>(&lds[r * BROW + kq + 8]) = s.v[1];
}

// Per-row epilogue of the bf16 block tile at (row0, col0), shared by the
// generic and the pipelined kernel. red_* must not alias LDS that another
// wave may still be reading when this is called.
template <int EPI, bool GATHER>
TIP_DEV void bf16_tile_epilogue(
    const f32x4b (&acc)[4][4], const float* __restrict__ anorm,
    const float* __restrict__ bnorm, const int* __restrict__ rowmap,
    int a_rows, int row0, int col0, int ncol1, int Bp, int bj,
    float (*red_v)[2], int (*red_i)[2], float (*red_s)[2],
    float* __restrict__ pmin_val, int* __restrict__ pmin_idx,
    float2* __restrict__ pkde);

// GATHER: A is the UNPADDED source [a_rows, K] and padded row p reads source
// row rowmap[p] (zeros where it is -1), its norm through the same index, so
// no class-sorted padded copy of the batch exists; Bp is then the static row
// bound of the plan (rows at or past tseg[nclasses] hold nothing).
template <int EPI, bool GATHER>
__launch_bounds__(256, 2) __global__ void grouped_pairwise_bf16_kernel(
    const short* __restrict__ A,      // [Bp, K] bf16, class-sorted padded
    const short* __restrict__ B,      // [Ntot, K] bf16 class-concatenated
    const float* __restrict__ anorm,  // [Bp] norms of the bf16 values
    const float* __restrict__ bnorm,  // [Ntot]
    const int* __restrict__ tseg, const int* __restrict__ nseg,
    const int* __restrict__ rowmap,   // GATHER: [Bp] padded row -> A row
    int a_rows,                       // GATHER: rows of A
    int nclasses, int Bp, int K,
    float* __restrict__ pmin_val, int* __restrict__ pmin_idx,
    float2* __restrict__ pkde) {
  __shared__ short As[128 * BROW];
  __shared__ short Bs[128 * BROW];
  __shared__ float red_v[BM][2];
  __shared__ int red_i[BM][2];
  __shared__ float red_s[BM][2];

  const int bi = blockIdx.y;
  const int bj = blockIdx.x;
  const int row0 = bi * BM;
  // a row block past the last segment belongs to no class (differs from the
  // fp32 grouped kernel, whose row bound is Bp alone)
  if (row0 >= tseg[nclasses]) return;
  const int cls = class_of_row(tseg, nclasses, row0);
  const int ncol0 = nseg[cls], ncol1 = nseg[cls + 1];
  const int col0 = ncol0 + bj * BN;
  if (col0 >= ncol1) return;

  const int lane = lane_id();
  const int wid = wave_id();
  const int wr = wid >> 1;  // row half (64 rows)
  const int wc = wid & 1;   // col half (64 cols)
  const int fj = lane & 15;
  const int fg = lane >> 4;

  // the A row this thread stages (fixed over the k loop)
  int arow = row0 + (threadIdx.x >> 1);
  bool arow_ok = arow < Bp;
  if (GATHER) {
    arow = arow_ok ? rowmap[arow] : -1;
    arow_ok = arow >= 0 && arow < a_rows;
  }

  f32x4b acc[4][4] = {};
  BStage ra = bstage_load_row(A, arow, arow_ok, K, 0);
  BStage rb = bstage_load(B, ncol1, K, col0, 0);
  bstage_write(As, ra);
  bstage_write(Bs, rb);
  __syncthreads();
  for (int k0 = 0; k0 < K; k0 += BBK) {
    const bool has_next = (k0 + BBK) < K;
    if (has_next) {
      ra = bstage_load_row(A, arow, arow_ok, K, k0 + BBK);
      rb = bstage_load(B, ncol1, K, col0, k0 + BBK);
    }
    bf16x8 af[4], bf[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int i = wr * 64 + t * 16 + fj;
      const int j = wc * 64 + t * 16 + fj;
      af[t] = *reinterpret_cast<const bf16x8*>(&As[i * BROW + fg * 8]);
      bf[t] = *reinterpret_cast<const bf16x8*>(&Bs[j * BROW + fg * 8]);
    }
#pragma unroll
    for (int tr = 0; tr < 4; ++tr)
#pragma unroll
      for (int tc = 0; tc < 4; ++tc)
        acc[tr][tc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af[tr], bf[tc], acc[tr][tc], 0, 0, 0);
    __syncthreads();
    if (has_next) {
      bstage_write(As, ra);
      bstage_write(Bs, rb);
    }
    __syncthreads();
  }

  bf16_tile_epilogue<EPI, GATHER>(acc, anorm, bnorm, rowmap, a_rows, row0,
                                  col0, ncol1, Bp, bj, red_v, red_i, red_s,
                                  pmin_val, pmin_idx, pkde);
}

template <int EPI, bool GATHER>
TIP_DEV void bf16_tile_epilogue(
    const f32x4b (&acc)[4][4], const float* __restrict__ anorm,
    const float* __restrict__ bnorm, const int* __restrict__ rowmap,
    int a_rows, int row0, int col0, int ncol1, int Bp, int bj,
    float (*red_v)[2], int (*red_i)[2], float (*red_s)[2],
    float* __restrict__ pmin_val, int* __restrict__ pmin_idx,
    float2* __restrict__ pkde) {
  const int lane = lane_id();
  const int wr = wave_id() >> 1;
  const int wc = wave_id() & 1;
  const int fj = lane & 15;
  const int fg = lane >> 4;

  // Epilogue. D tile (tr, tc): row i = wr*64 + tr*16 + fg*4 + reg,
  // col j = wc*64 + tc*16 + fj. Per row: reduce over this wave's 64 cols
  // (4 tc in registers + 16 fj lanes via xor shuffles), stash per col-half.
#pragma unroll
  for (int tr = 0; tr < 4; ++tr) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row_local = wr * 64 + tr * 16 + fg * 4 + reg;
      const int gi = row0 + row_local;
      float an;
      if (GATHER) {
        const int src = rowmap[gi];
        an = (src >= 0 && src < a_rows) ? anorm[src] : 0.f;
      } else {
        an = anorm[gi];
      }
      MinIdx mi{FLT_MAX, 0x7fffffff};
      float dvals[4];
#pragma unroll
      for (int tc = 0; tc < 4; ++tc) {
        const int gj = col0 + wc * 64 + tc * 16 + fj;
        float d;
        // differs from the fp32 epilogue, which preloads bn0 / bn1 and
        // overwrites the out-of-range distances afterwards
        if (gj < ncol1) {
          d = fmaxf(an + bnorm[gj] - 2.f * acc[tr][tc][reg], 0.f);
        } else {
          d = FLT_MAX;
        }
        dvals[tc] = d;
        mi = min_idx_combine(mi, MinIdx{d, gj});
      }
      // 16-lane (same fg) xor reduce; offsets < 16 stay in the group
      for (int off = 8; off >= 1; off >>= 1) {
        MinIdx o;
        o.v = __shfl_xor(mi.v, off);
        o.i = __shfl_xor(mi.i, off);
        mi = min_idx_combine(mi, o);
      }
      if (EPI == EPI_ROWMIN) {
        if (fj == 0) {
          red_v[row_local][wc] = mi.v;
          red_i[row_local][wc] = mi.i;
        }
      } else {
        // differs from the fp32 epilogue, which takes -0.5f * min even for
        // a half with no column in range
        const float tmax = (mi.v == FLT_MAX) ? -FLT_MAX : -0.5f * mi.v;
        float s = 0.f;
#pragma unroll
        for (int tc = 0; tc < 4; ++tc)
          if (dvals[tc] != FLT_MAX) s += __expf(-0.5f * dvals[tc] - tmax);
        for (int off = 8; off >= 1; off >>= 1) s += __shfl_xor(s, off);
        if (fj == 0) {
          red_v[row_local][wc] = tmax;
          red_s[row_local][wc] = s;
        }
      }
    }
  }
  __syncthreads();
  merge_halves_store<EPI>(red_v, red_i, red_s, row0, Bp, Bp, bj, pmin_val,
                          pmin_idx, pkde);
}

// ---------------------------------------------------------------------------
// Pipelined bf16 grouped row-min (docs/kernels.md "Pipelined row-min"). Same
// tile, waves, MFMA and epilogue as grouped_pairwise_bf16_kernel<EPI_ROWMIN>,
// and every accumulator is the same chain over k ascending in steps of 32, so
// the partials are the same bits. What differs is the staging: K-tiles of
// PBK = 64 go global -> LDS by 16-byte direct-to-LDS loads into PNBUF = 2
// buffers, tile t+1 issued before tile t's fragment reads, one barrier per
// tile. Serves K % PBK == 0 and 16-byte-aligned operands only; the
// launchers dispatch.
//
// LDS image of one operand tile: [128 rows][8 units of 16 B], lane-linear as
// the DMA writes it (thread t, pass q: row q*32 + t/8, unit t%8). Unit u of
// row r holds k-unit u ^ (r & 7): the XOR is applied to the per-lane SOURCE
// address and again on the fragment read, which makes every ds_read_b128
// lane group hit 16 distinct 16-B slots of the 256-B bank row.
//
// Tile t (buffer t & 1) is staged in iteration t-1 after the barrier, retired
// by the vmcnt(0) every wave executes before iteration t's barrier, read only
// after that barrier, and restaged in iteration t+1 after the next one. At
// most one tile is in flight and none crosses a barrier un-waited, so plain
// __syncthreads() is enough (full accounting: docs/kernels.md).
// ---------------------------------------------------------------------------

constexpr int PBK = 64;              // k per staged tile: two MFMA k-steps
constexpr int PNBUF = 2;             // LDS buffers per operand
constexpr int PTILE = 128 * PBK;     // halves per operand tile (16 KiB)

// Source of all-zero units for pad rows: the DMA of such a lane reads here
// (and does not advance with k) instead of being branched around.
static __device__ __attribute__((aligned(128))) short g_zero_units[PBK];

// Block order of the pipelined kernel: 1 deals contiguous runs of the
// (column block fast, row block slow) order to the blocks that share an XCD
// (T1, bijective), so that a row panel's column blocks meet in one L2; 0
// keeps (blockIdx.x, blockIdx.y) as they come, which deals them across all
// eight. 1 measured 6 - 7 % faster (profiles/r10_rowmin_pipeline.md).
#ifndef TIP_ROWMIN_XCD
#define TIP_ROWMIN_XCD 1
#endif

using lds_ptr_t = __attribute__((address_space(3))) void*;
using glb_ptr_t = const __attribute__((address_space(1))) void*;

template <bool GATHER>
__launch_bounds__(256, 2) __global__ void grouped_rowmin_bf16_pipe_kernel(
    const short* __restrict__ A,      // [Bp, K] bf16 (GATHER: [a_rows, K])
    const short* __restrict__ B,      // [Ntot, K] bf16 class-concatenated
    const float* __restrict__ anorm, const float* __restrict__ bnorm,
    const int* __restrict__ tseg, const int* __restrict__ nseg,
    const int* __restrict__ rowmap,   // GATHER: [Bp] padded row -> A row
    int a_rows,                       // GATHER: rows of A
    int nclasses, int Bp, int K,
    float* __restrict__ pmin_val, int* __restrict__ pmin_idx) {
  // one array: staging ring [PNBUF][A, B][128][PBK]; its head is reused as
  // red_v / red_i after the loop
  __shared__ __attribute__((aligned(16))) short lds[PNBUF * 2 * PTILE];

  int bi = blockIdx.y, bj = blockIdx.x;
  if (TIP_ROWMIN_XCD) {
    const int nwg = gridDim.x * gridDim.y;
    const int id = blockIdx.y * gridDim.x + blockIdx.x;
    const int q = nwg / 8, r = nwg % 8;
    const int xcd = id % 8, pos = id / 8;
    const int newid =
        (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
    bi = newid / gridDim.x;
    bj = newid % gridDim.x;
  }
  const int row0 = bi * BM;
  if (row0 >= tseg[nclasses]) return;
  const int cls = class_of_row(tseg, nclasses, row0);
  const int ncol0 = nseg[cls], ncol1 = nseg[cls + 1];
  const int col0 = ncol0 + bj * BN;
  if (col0 >= ncol1) return;

  const int t = threadIdx.x;
  const int lane = lane_id();
  const int wid = wave_id();
  const int wr = wid >> 1;
  const int wc = wid & 1;
  const int fj = lane & 15;
  const int fg = lane >> 4;

  // Staging sources: pass q of this thread fills row q*32 + t/8, unit t%8,
  // from k-unit (t%8) ^ (row & 7); a pad row reads g_zero_units, step 0.
  const int sunit = (t & 7) ^ ((t >> 3) & 7);
  const short* asrc[4];
  const short* bsrc[4];
  int astep[4], bstep[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = q * 32 + (t >> 3);
    int arow = row0 + r;
    bool aok = arow < Bp;
    if (GATHER) {
      arow = aok ? rowmap[arow] : -1;
      aok = arow >= 0 && arow < a_rows;
    }
    asrc[q] = (aok ? A + (int64_t)arow * K : g_zero_units) + sunit * 8;
    astep[q] = aok ? PBK : 0;
    const int brow = col0 + r;
    const bool bok = brow < ncol1;
    bsrc[q] = (bok ? B + (int64_t)brow * K : g_zero_units) + sunit * 8;
    bstep[q] = bok ? PBK : 0;
  }
  // wave-uniform LDS destination of pass q: the hardware adds lane * 16 B
  auto stage = [&](int buf) {
    short* dst = lds + buf * 2 * PTILE + wid * 64 * 8;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      __builtin_amdgcn_global_load_lds((glb_ptr_t)asrc[q],
                                       (lds_ptr_t)(dst + q * 256 * 8), 16, 0,
                                       0);
      __builtin_amdgcn_global_load_lds(
          (glb_ptr_t)bsrc[q], (lds_ptr_t)(dst + PTILE + q * 256 * 8), 16, 0, 0);
      asrc[q] += astep[q];
      bsrc[q] += bstep[q];
    }
  };

  // fragment read offsets (halves) inside an operand tile: row wX*64 + fj
  // (+ 16 rows per fragment), k-step s at unit (s*4 + fg) ^ (fj & 7)
  const int aoff = (wr * 64 + fj) * PBK;
  const int boff = PTILE + (wc * 64 + fj) * PBK;
  const int uoff[2] = {((fg) ^ (fj & 7)) * 8, ((4 + fg) ^ (fj & 7)) * 8};

  f32x4b acc[4][4] = {};
  const int ntiles = K / PBK;
  stage(0);
  for (int kt = 0; kt < ntiles; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < ntiles) stage((kt + 1) & 1);
    const short* cur = lds + (kt & 1) * 2 * PTILE;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 af[4], bf[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        af[f] = *reinterpret_cast<const bf16x8*>(
            &cur[aoff + f * 16 * PBK + uoff[s]]);
        bf[f] = *reinterpret_cast<const bf16x8*>(
            &cur[boff + f * 16 * PBK + uoff[s]]);
      }
#pragma unroll
      for (int tr = 0; tr < 4; ++tr)
#pragma unroll
        for (int tc = 0; tc < 4; ++tc)
          acc[tr][tc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[tr], bf[tc], acc[tr][tc], 0, 0, 0);
    }
  }

  __syncthreads();  // every wave is done reading before red_* reuse the ring
  float(*red_v)[2] = reinterpret_cast<float(*)[2]>(lds);
  int(*red_i)[2] = reinterpret_cast<int(*)[2]>(lds + BM * 2 * 2);
  bf16_tile_epilogue<EPI_ROWMIN, GATHER>(
      acc, anorm, bnorm, rowmap, a_rows, row0, col0, ncol1, Bp, bj, red_v,
      red_i, nullptr, pmin_val, pmin_idx, nullptr);
}

// ---------------------------------------------------------------------------
// Cross-block-column combines. One thread per row folds that row's jcount
// partials (row i of column block b is at [b * stride + i]) in ascending b:
// ascending keeps np.argmin's lowest-index tie rule, a fixed order keeps the
// results bitwise stable across launches and shard counts.
// ---------------------------------------------------------------------------

TIP_DEV MinIdx fold_rowmin(const float* __restrict__ pval,
                           const int* __restrict__ pidx, int jcount,
                           int stride, int i) {
  MinIdx best{FLT_MAX, 0x7fffffff};
  for (int b = 0; b < jcount; ++b)
    best = min_idx_combine(best, MinIdx{pval[(int64_t)b * stride + i],
                                        pidx[(int64_t)b * stride + i]});
  return best;
}

// Streaming logsumexp over the (max, sum) partials; -FLT_MAX when every
// partial is empty (jcount == 0, or every term underflowed).
TIP_DEV float fold_kde(const float2* __restrict__ pkde, int jcount, int stride,
                       int i) {
  float mm = -FLT_MAX, ss = 0.f;
  for (int b = 0; b < jcount; ++b) {
    const float2 p = pkde[(int64_t)b * stride + i];
    if (p.y <= 0.f) continue;
    if (p.x > mm) {
      ss = p.y + ((ss > 0.f) ? ss * __expf(mm - p.x) : 0.f);
      mm = p.x;
    } else {
      ss += p.y * __expf(p.x - mm);
    }
  }
  return (ss > 0.f) ? (mm + __logf(ss)) : -FLT_MAX;
}

// Column blocks of class cls.
TIP_DEV int class_jcount(const int* __restrict__ nseg, int cls) {
  return (nseg[cls + 1] - nseg[cls] + BN - 1) / BN;
}

__global__ void rowmin_combine_kernel(
    const float* __restrict__ pval, const int* __restrict__ pidx, int jblocks,
    int M, float* __restrict__ out_dist, int64_t* __restrict__ out_idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const MinIdx best = fold_rowmin(pval, pidx, jblocks, M, i);
  out_dist[i] = sqrtf(best.v);
  out_idx[i] = best.i;
}

__global__ void kde_combine_kernel(
    const float2* __restrict__ pkde, int jblocks, int M,
    float* __restrict__ out_lse) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  out_lse[i] = fold_kde(pkde, jblocks, M, i);
}

__global__ void grouped_rowmin_combine_kernel(
    const float* __restrict__ pval, const int* __restrict__ pidx,
    const int* __restrict__ tseg, const int* __restrict__ nseg, int nclasses,
    int Bp, float* __restrict__ out_dist, int64_t* __restrict__ out_idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Bp) return;
  const int jcount = class_jcount(nseg, class_of_row(tseg, nclasses, i));
  const MinIdx best = fold_rowmin(pval, pidx, jcount, Bp, i);
  if (jcount == 0) {
    // differs from grouped_rowmin_final_kernel: FLT_MAX, and no NaN guard
    out_dist[i] = FLT_MAX;
    out_idx[i] = -1;
  } else {
    out_dist[i] = sqrtf(best.v);
    out_idx[i] = best.i;
  }
}

__global__ void grouped_kde_combine_kernel(
    const float2* __restrict__ pkde, const int* __restrict__ tseg,
    const int* __restrict__ nseg, int nclasses, int Bp,
    float* __restrict__ out_lse) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Bp) return;
  const int jcount = class_jcount(nseg, class_of_row(tseg, nclasses, i));
  out_lse[i] = fold_kde(pkde, jcount, Bp, i);
}

// Plan-driven combines (sync-free scoring path): the same folds, but each
// padded row p writes its FINAL score to its source row rowmap[p]. Pad rows
// and rows at or past tseg[nclasses] write nothing, so the outputs
// (pre-filled with +inf by the caller) never see stale workspace content.
__global__ void grouped_rowmin_final_kernel(
    const float* __restrict__ pval, const int* __restrict__ pidx,
    const int* __restrict__ tseg, const int* __restrict__ nseg, int nclasses,
    int Bp, const int* __restrict__ rowmap, int out_rows,
    const float* __restrict__ btable, float* __restrict__ out_dsa,
    float* __restrict__ out_dist, int* __restrict__ out_idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Bp || i >= tseg[nclasses]) return;
  const int src = rowmap[i];
  if (src < 0 || src >= out_rows) return;
  const int jcount = class_jcount(nseg, class_of_row(tseg, nclasses, i));
  const MinIdx best = fold_rowmin(pval, pidx, jcount, Bp, i);
  if (jcount == 0) {
    // differs from grouped_rowmin_combine_kernel: the score is +inf
    out_dsa[src] = INFINITY;
    out_dist[src] = FLT_MAX;
    out_idx[src] = -1;
  } else if ((unsigned)best.i >= (unsigned)nseg[nclasses]) {
    // every distance was NaN (non-finite activations): no argmin to gather.
    // Only this kernel has the guard; the other two rowmin combines store
    // the fold's initial index.
    out_dsa[src] = NAN;
    out_dist[src] = NAN;
    out_idx[src] = -1;
  } else {
    const float dist = sqrtf(best.v);
    out_dsa[src] = dist / btable[best.i];
    out_dist[src] = dist;
    out_idx[src] = best.i;
  }
}

__global__ void grouped_kde_final_kernel(
    const float2* __restrict__ pkde, const int* __restrict__ tseg,
    const int* __restrict__ nseg, int nclasses, int Bp,
    const int* __restrict__ rowmap, int out_rows,
    const int* __restrict__ cls_fused,    // [C] 1: KDE class, 0: constant
    const float* __restrict__ cls_const,  // [C] KDE constant / the score
    float* __restrict__ out_lsa) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Bp || i >= tseg[nclasses]) return;
  const int src = rowmap[i];
  if (src < 0 || src >= out_rows) return;
  const int cls = class_of_row(tseg, nclasses, i);
  if (!cls_fused[cls]) {
    out_lsa[src] = cls_const[cls];
    return;
  }
  // differs from grouped_kde_combine_kernel: the negated, shifted score
  const float lse = fold_kde(pkde, class_jcount(nseg, cls), Bp, i);
  out_lsa[src] = -(lse + cls_const[cls]);
}

// ---------------------------------------------------------------------------
// Silhouette cluster sums (docs/kernels.md "Batched k-means"). X against
// itself: the tile at (row0, col0) holds the Gram block, and instead of
// writing sqrt(max(d^2, 0)) out, the epilogue adds it into the bin of its row
// that the column's label names, for every labeling of the pass at once. A
// pass serves problems p0 .. p0 + np - 1, whose bins seg[p0] .. seg[p0 + np]
// number at most SIL_BINS. A block owns one row block and a strip of
// SIL_STRIP consecutive column blocks, keeps the bins in LDS over the strip
// and writes one partial per strip; silhouette_fold_kernel adds the strips
// in ascending order.
//
// Epilogue layout. The accumulators hold a column per lane, the bins want a
// row per thread, so the tile goes through LDS in two 64-column passes: the
// two waves that own the pass's columns write their distances to
// T[128][SIL_TROW] (the dead staging buffer; the odd row stride keeps the
// row-per-lane reads conflict-free), then thread t scans row t & 127,
// columns (t >> 7) * 32 .. + 31 of the pass in ascending order, adding T into
// bins[t >> 7][slot][row]. slot[pl][col] is the pass-local bin of column col
// under problem p0 + pl, or -1 (column past N, label outside the problem).
// Every sum has one fixed order: columns ascending within a 32-column
// quarter, quarters of the low pass before the high pass, column blocks of
// the strip ascending, then quarter set 0 + quarter set 1, then the strips.
// The diagonal term is set to 0 exactly where row == column.
// ---------------------------------------------------------------------------

constexpr int SIL_BINS = 16;   // bins one Gram pass serves
constexpr int SIL_STRIP = 8;   // column blocks folded in LDS by one block
constexpr int SIL_TROW = 65;   // floats per row of the transposed pass tile

static_assert(BM * SIL_TROW <= 2 * BK * (BM + LDS_PAD),
              "the transposed pass tile reuses the staging buffer");

__launch_bounds__(256, 2) __global__ void silhouette_sums_kernel(
    const float* __restrict__ X,       // [N, K]
    const float* __restrict__ xnorm,   // [N]
    int N, int K,
    const int* __restrict__ labels,    // [P, N]
    const int* __restrict__ seg,       // [P+1]
    int p0, int np, int C,
    float* __restrict__ ppart) {       // [strips, N, SIL_BINS]
  __shared__ float lds[2 * BK * (BM + LDS_PAD)];
  __shared__ float bins[2][SIL_BINS][BM];
  __shared__ signed char slot[SIL_BINS][BN];

  const int t = threadIdx.x;
  const int lane = lane_id();
  const int wr = wave_id() >> 1;
  const int wc = wave_id() & 1;
  const int strip = blockIdx.x;
  const int row0 = blockIdx.y * BM;
  const int jb = (N + BN - 1) / BN;
  const int bj_end = min(jb, (strip + 1) * SIL_STRIP);
  const int bin0 = seg[p0];
  const int r = t & (BM - 1);
  const int q = t >> 7;

  for (int e = t; e < 2 * SIL_BINS * BM; e += blockDim.x)
    (&bins[0][0][0])[e] = 0.f;

  for (int bj = strip * SIL_STRIP; bj < bj_end; ++bj) {
    const int col0 = bj * BN;
    // the previous column block's scans ended in a barrier: slot is free
    for (int e = t; e < np * BN; e += blockDim.x) {
      const int pl = e / BN, c = e % BN;
      const int col = col0 + c;
      int s = -1;
      if (col < N) {
        const int b = seg[p0 + pl];
        const int k = seg[p0 + pl + 1] - b;
        const int lab = labels[(int64_t)(p0 + pl) * N + col];
        if (lab >= 0 && lab < k) s = b - bin0 + lab;
        if (s >= SIL_BINS || b + lab >= C) s = -1;
      }
      slot[pl][c] = (signed char)s;
    }
    // the main loop's barriers publish bins (first block) and slot
    const TileAcc acc = tile_mainloop_f32(X, N, X, N, K, row0, col0, lds,
                                          lds + BK * (BM + LDS_PAD));
    const int jl0 = col0 + wc * 64 + (lane & 31);
    const float bn0 = (jl0 < N) ? xnorm[jl0] : 0.f;
    const float bn1 = (jl0 + 32 < N) ? xnorm[jl0 + 32] : 0.f;
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      if (wc == h) {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
#pragma unroll
          for (int reg = 0; reg < 16; ++reg) {
            const int row_local = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
            const int block_row = wr * 64 + m * 32 + row_local;
            const int i = row0 + block_row;
            const float an = (i < N) ? xnorm[i] : 0.f;
            float d0 = sqrtf(fmaxf(an + bn0 - 2.f * acc.t[m][0][reg], 0.f));
            float d1 = sqrtf(fmaxf(an + bn1 - 2.f * acc.t[m][1][reg], 0.f));
            if (i == jl0) d0 = 0.f;
            if (i == jl0 + 32) d1 = 0.f;
            lds[block_row * SIL_TROW + (lane & 31)] = d0;
            lds[block_row * SIL_TROW + 32 + (lane & 31)] = d1;
          }
        }
      }
      __syncthreads();
#pragma unroll 4
      for (int jj = 0; jj < 32; ++jj) {
        const int cl = q * 32 + jj;
        const float d = lds[r * SIL_TROW + cl];
#pragma unroll 1
        for (int pl = 0; pl < np; ++pl) {
          const int s = slot[pl][h * 64 + cl];  // one address per wave
          if (s >= 0) bins[q][s][r] += d;
        }
      }
      __syncthreads();  // T, and after the last pass slot, may be rewritten
    }
  }

  for (int e = t; e < BM * SIL_BINS; e += blockDim.x) {
    const int rr = e / SIL_BINS, b = e % SIL_BINS;
    const int i = row0 + rr;
    if (i < N)
      ppart[((int64_t)strip * N + i) * SIL_BINS + b] =
          bins[0][b][rr] + bins[1][b][rr];
  }
}

// out[i, bin0 + b] = sum of the strips' partials of (row i, bin b), strips
// ascending; one thread per (row, bin of the pass).
__global__ void silhouette_fold_kernel(
    const float* __restrict__ ppart, int strips, int N, int bin0, int nbins,
    int C, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)N * SIL_BINS) return;
  const int i = (int)(e / SIL_BINS), b = (int)(e % SIL_BINS);
  if (b >= nbins || bin0 + b >= C) return;
  float s = 0.f;
  for (int st = 0; st < strips; ++st)
    s += ppart[((int64_t)st * N + i) * SIL_BINS + b];
  out[(int64_t)i * C + bin0 + b] = s;
}

// Row squared norms: one wave per row.
__global__ void rownorm_kernel(
    const float* __restrict__ X, int rows, int K, float* __restrict__ out) {
  const int row = blockIdx.x * (blockDim.x / WAVE) + wave_id();
  if (row >= rows) return;
  const float* p = X + (int64_t)row * K;
  float s = 0.f;
  for (int k = lane_id(); k < K; k += WAVE) {
    const float v = p[k];
    s += v * v;
  }
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
  if (lane_id() == 0) out[row] = s;
}

// ---- host-side launchers (called from bindings.cpp) ----

void launch_rownorm(const float* x, int rows, int k, float* out, hipStream_t s) {
  const int wpb = 4;
  rownorm_kernel<<<ceil_div(rows, wpb), wpb * WAVE, 0, s>>>(x, rows, k, out);
}

void launch_pairwise_full(const float* a, const float* b, const float* an,
                          const float* bn, int m, int n, int k, float* out,
                          hipStream_t s) {
  dim3 grid(ceil_div(n, BN), ceil_div(m, BM));
  pairwise_kernel<EPI_FULL><<<grid, 256, 0, s>>>(
      a, b, an, bn, m, n, k, out, nullptr, nullptr, nullptr);
}

void launch_pairwise_rowmin(const float* a, const float* b, const float* an,
                            const float* bn, int m, int n, int k,
                            float* pval, int* pidx, float* out_dist,
                            int64_t* out_idx, hipStream_t s) {
  const int jb = ceil_div(n, BN);
  dim3 grid(jb, ceil_div(m, BM));
  pairwise_kernel<EPI_ROWMIN><<<grid, 256, 0, s>>>(
      a, b, an, bn, m, n, k, nullptr, pval, pidx, nullptr);
  rowmin_combine_kernel<<<ceil_div(m, 256), 256, 0, s>>>(
      pval, pidx, jb, m, out_dist, out_idx);
}

void launch_pairwise_kde(const float* a, const float* b, const float* an,
                         const float* bn, int m, int n, int k, float2* pkde,
                         float* out_lse, hipStream_t s) {
  const int jb = ceil_div(n, BN);
  dim3 grid(jb, ceil_div(m, BM));
  pairwise_kernel<EPI_KDE><<<grid, 256, 0, s>>>(
      a, b, an, bn, m, n, k, nullptr, nullptr, nullptr, pkde);
  kde_combine_kernel<<<ceil_div(m, 256), 256, 0, s>>>(pkde, jb, m, out_lse);
}

void launch_grouped_rowmin(const float* a, const float* b, const float* an,
                           const float* bn, const int* tseg, const int* nseg,
                           int nclasses, int bp, int k, int jb_max,
                           float* pval, int* pidx, float* out_dist,
                           int64_t* out_idx, hipStream_t s) {
  dim3 grid(jb_max, ceil_div(bp, BM));
  grouped_pairwise_kernel<EPI_ROWMIN><<<grid, 256, 0, s>>>(
      a, b, an, bn, tseg, nseg, nclasses, bp, k, pval, pidx, nullptr);
  grouped_rowmin_combine_kernel<<<ceil_div(bp, 256), 256, 0, s>>>(
      pval, pidx, tseg, nseg, nclasses, bp, out_dist, out_idx);
}

void launch_grouped_kde(const float* a, const float* b, const float* an,
                        const float* bn, const int* tseg, const int* nseg,
                        int nclasses, int bp, int k, int jb_max, float2* pkde,
                        float* out_lse, hipStream_t s) {
  dim3 grid(jb_max, ceil_div(bp, BM));
  grouped_pairwise_kernel<EPI_KDE><<<grid, 256, 0, s>>>(
      a, b, an, bn, tseg, nseg, nclasses, bp, k, nullptr, nullptr, pkde);
  grouped_kde_combine_kernel<<<ceil_div(bp, 256), 256, 0, s>>>(
      pkde, tseg, nseg, nclasses, bp, out_lse);
}

// One silhouette pass: the cluster sums of problems p0 .. p0 + np - 1 (bins
// bin0 .. bin0 + nbins - 1 of the C columns of `out`, nbins <= SIL_BINS).
// ppart holds silhouette_strips(n) * n * SIL_BINS floats.
int silhouette_bins() { return SIL_BINS; }
int silhouette_strips(int n) { return ceil_div(ceil_div(n, BN), SIL_STRIP); }

void launch_silhouette_sums(const float* x, const float* xnorm, int n, int k,
                            const int* labels, const int* seg, int p0, int np,
                            int bin0, int nbins, int c, float* ppart,
                            float* out, hipStream_t s) {
  const int strips = silhouette_strips(n);
  dim3 grid(strips, ceil_div(n, BM));
  silhouette_sums_kernel<<<grid, 256, 0, s>>>(x, xnorm, n, k, labels, seg, p0,
                                              np, c, ppart);
  silhouette_fold_kernel<<<ceil_div((int64_t)n * SIL_BINS, 256), 256, 0, s>>>(
      ppart, strips, n, bin0, nbins, c, out);
}

// Dispatch of the bf16 row-min launchers. The pipelined kernel serves K a
// positive multiple of its K-tile and 16-byte-aligned operands (rows are then
// 16-byte aligned too); everything else, and everything while the generic
// kernel is forced, runs grouped_pairwise_bf16_kernel. The counter tells
// tests which kernel a call took.
static bool g_rowmin_force_generic = false;
static int64_t g_rowmin_pipelined_launches = 0;

void rowmin_bf16_force_generic(bool on) { g_rowmin_force_generic = on; }
int64_t rowmin_bf16_pipelined_launches() { return g_rowmin_pipelined_launches; }
int rowmin_bf16_pipeline_bk() { return PBK; }
int rowmin_bf16_pipeline_nbuf() { return PNBUF; }

static bool rowmin_bf16_use_pipeline(const short* a, const short* b, int k) {
  const bool ok = !g_rowmin_force_generic && k > 0 && k % PBK == 0 &&
                  ((reinterpret_cast<uintptr_t>(a) |
                    reinterpret_cast<uintptr_t>(b)) & 15) == 0;
  if (ok) ++g_rowmin_pipelined_launches;
  return ok;
}

void launch_grouped_rowmin_bf16(const short* a, const short* b,
                                const float* an, const float* bn,
                                const int* tseg, const int* nseg,
                                int nclasses, int bp, int k, int jb_max,
                                float* pval, int* pidx, float* out_dist,
                                int64_t* out_idx, hipStream_t s) {
  dim3 grid(jb_max, ceil_div(bp, BM));
  if (rowmin_bf16_use_pipeline(a, b, k))
    grouped_rowmin_bf16_pipe_kernel<false><<<grid, 256, 0, s>>>(
        a, b, an, bn, tseg, nseg, nullptr, 0, nclasses, bp, k, pval, pidx);
  else
    grouped_pairwise_bf16_kernel<EPI_ROWMIN, false><<<grid, 256, 0, s>>>(
        a, b, an, bn, tseg, nseg, nullptr, 0, nclasses, bp, k, pval, pidx,
        nullptr);
  grouped_rowmin_combine_kernel<<<ceil_div(bp, 256), 256, 0, s>>>(
      pval, pidx, tseg, nseg, nclasses, bp, out_dist, out_idx);
}

void launch_grouped_kde_bf16(const short* a, const short* b, const float* an,
                             const float* bn, const int* tseg,
                             const int* nseg, int nclasses, int bp, int k,
                             int jb_max, float2* pkde, float* out_lse,
                             hipStream_t s) {
  dim3 grid(jb_max, ceil_div(bp, BM));
  grouped_pairwise_bf16_kernel<EPI_KDE, false><<<grid, 256, 0, s>>>(
      a, b, an, bn, tseg, nseg, nullptr, 0, nclasses, bp, k, nullptr, nullptr,
      pkde);
  grouped_kde_combine_kernel<<<ceil_div(bp, 256), 256, 0, s>>>(
      pkde, tseg, nseg, nclasses, bp, out_lse);
}

// Sync-free path: A gathered through the segment plan, final DSA scores
// written per source row.
void launch_grouped_rowmin_plan(const short* a, int a_rows, const short* b,
                                const float* an, const float* bn,
                                const int* tseg, const int* nseg,
                                const int* rowmap, const float* btable,
                                int nclasses, int bp, int k, int jb_max,
                                float* pval, int* pidx, float* out_dsa,
                                float* out_dist, int* out_idx, hipStream_t s) {
  dim3 grid(jb_max, ceil_div(bp, BM));
  if (rowmin_bf16_use_pipeline(a, b, k))
    grouped_rowmin_bf16_pipe_kernel<true><<<grid, 256, 0, s>>>(
        a, b, an, bn, tseg, nseg, rowmap, a_rows, nclasses, bp, k, pval, pidx);
  else
    grouped_pairwise_bf16_kernel<EPI_ROWMIN, true><<<grid, 256, 0, s>>>(
        a, b, an, bn, tseg, nseg, rowmap, a_rows, nclasses, bp, k, pval, pidx,
        nullptr);
  grouped_rowmin_final_kernel<<<ceil_div(bp, 256), 256, 0, s>>>(
      pval, pidx, tseg, nseg, nclasses, bp, rowmap, a_rows, btable, out_dsa,
      out_dist, out_idx);
}

// Sync-free path: quadratic forms of the centred workspace `dc` against the
// groups' matrices, then the final Mahalanobis (logc == nullptr) or mixture
// NLL scores per source row. `slots` is the largest component count.
int grouped_gauss_max_slots() { return QUAD_MAX_SLOTS; }

void launch_grouped_gauss_plan(const float* dc, const float* mats,
                               const int* tseg, const int* comp_off,
                               const int* rowmap, int out_rows,
                               const float* logc, int ngroups, int bp, int d,
                               int slots, float* pquad, float* out,
                               hipStream_t s) {
  const int jb = ceil_div(d, BN);
  dim3 grid(jb, ceil_div(bp, BM), slots);
  grouped_quad_kernel<<<grid, 256, 0, s>>>(dc, mats, tseg, comp_off, ngroups,
                                           bp, d, pquad);
  grouped_gauss_final_kernel<<<ceil_div(bp, 256), 256, 0, s>>>(
      pquad, tseg, comp_off, ngroups, bp, jb, rowmap, out_rows, logc,
      logc != nullptr ? 1 : 0, out);
}

// Sync-free path: `a` is the whitened workspace (already in padded layout),
// final LSA scores written per source row.
void launch_grouped_kde_plan(const short* a, const short* b, const float* an,
                             const float* bn, const int* tseg,
                             const int* nseg, const int* rowmap, int out_rows,
                             const int* cls_fused, const float* cls_const,
                             int nclasses, int bp, int k, int jb_max,
                             float2* pkde, float* out_lsa, hipStream_t s) {
  dim3 grid(jb_max, ceil_div(bp, BM));
  grouped_pairwise_bf16_kernel<EPI_KDE, false><<<grid, 256, 0, s>>>(
      a, b, an, bn, tseg, nseg, nullptr, 0, nclasses, bp, k, nullptr, nullptr,
      pkde);
  grouped_kde_final_kernel<<<ceil_div(bp, 256), 256, 0, s>>>(
      pkde, tseg, nseg, nclasses, bp, rowmap, out_rows, cls_fused, cls_const,
      out_lsa);
}
