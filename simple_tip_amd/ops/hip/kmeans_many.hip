// Batched Lloyd iterations for gfx950 (CDNA4): P k-means problems that share
// the rows x [N, D] advance in lockstep (docs/kernels.md "Batched k-means").
// Their centres are stacked in centers [C, D]; problem p owns rows
// seg[p] .. seg[p+1] of it.
//
// Assign: the squared distances to all C centres come from one EPI_FULL
// launch of the pairwise tile core (pairwise.hip), so each is the value
// rowmin_l2 would see; lloyd_argmin_kernel takes the per-problem minimum with
// the same (value, index) combine.
//
// Update: lloyd_partial_kernel reads x once for all problems. A block owns 64
// feature columns of a chunk of KMEANS_MANY_CHUNK_ROWS rows and keeps the
// chunk's C x 64 sums in LDS, a private column per lane. Its four waves split
// the problems: a lane carries one problem of its wave, loads the row's label
// and turns it into the stacked centre index (or -1: problem inactive, label
// out of range), which the wave reads back lane by lane. lloyd_fold_kernel
// adds the chunks' partials in ascending order, divides by the count and
// writes the centre;
// lloyd_finish_kernel sums the centres' shifts per problem and clears
// `active` at or below tol. No float atomics: a sum's order is rows
// ascending within a chunk, then chunks ascending, whatever else the call
// holds. The counts are integer atomics, which commute.

#include "kmeans_many.h"
#include "tip_common.h"

#include <cfloat>

static_assert(KMEANS_MANY_MAX_PROBLEMS <= WAVE, "one lane per problem");

__global__ void lloyd_argmin_kernel(
    const float* __restrict__ d2,   // [N, C]
    const int* __restrict__ seg, int N, int C, int* __restrict__ labels,
    float* __restrict__ mind) {     // [P, N]
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int p = blockIdx.y;
  if (i >= N) return;
  const int b = max(seg[p], 0);
  const int e = min(seg[p + 1], C);
  MinIdx best{FLT_MAX, 0x7fffffff};
  for (int c = b; c < e; ++c)
    best = min_idx_combine(best, MinIdx{d2[(int64_t)i * C + c], c - b});
  labels[(int64_t)p * N + i] = best.i;
  mind[(int64_t)p * N + i] = sqrtf(best.v);
}

// Segment of problem p if it is active and well formed, else k = 0.
TIP_DEV void lloyd_segment(const int* __restrict__ seg,
                           const int* __restrict__ active, int p, int C,
                           int* base, int* k) {
  *base = 0;
  *k = 0;
  if (!active[p]) return;
  const int b = seg[p], n = seg[p + 1] - b;
  if (b < 0 || n <= 0 || n > KMEANS_MANY_MAX_K || b + n > C) return;
  *base = b;
  *k = n;
}

__global__ void lloyd_count_kernel(
    const int* __restrict__ labels, const int* __restrict__ seg,
    const int* __restrict__ active, int N, int C, int* __restrict__ counts) {
  __shared__ int hist[KMEANS_MANY_MAX_K];
  const int p = blockIdx.y;
  int base, k;
  lloyd_segment(seg, active, p, C, &base, &k);
  if (k == 0) return;  // block-uniform
  if (threadIdx.x < KMEANS_MANY_MAX_K) hist[threadIdx.x] = 0;
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) {
    const int lab = labels[(int64_t)p * N + i];
    if (lab >= 0 && lab < k) atomicAdd(&hist[lab], 1);
  }
  __syncthreads();
  if (threadIdx.x < k && hist[threadIdx.x] != 0)
    atomicAdd(&counts[base + threadIdx.x], hist[threadIdx.x]);
}

constexpr int LLOYD_WAVES = 4;  // waves of a block, each with its share of P

__launch_bounds__(LLOYD_WAVES * WAVE) __global__ void lloyd_partial_kernel(
    const float* __restrict__ x, const int* __restrict__ labels,
    const int* __restrict__ seg, const int* __restrict__ active, int N, int D,
    int P, int C, float* __restrict__ psum) {  // [chunks, C, D]
  extern __shared__ float acc[];               // [C][WAVE]
  const int lane = lane_id();
  const int w = wave_id();
  const int d = blockIdx.x * WAVE + lane;
  const bool dok = d < D;
  const int chunk = blockIdx.y;
  const int r0 = chunk * KMEANS_MANY_CHUNK_ROWS;
  const int r1 = min(N, r0 + KMEANS_MANY_CHUNK_ROWS);

  for (int c = w; c < C; c += LLOYD_WAVES) acc[c * WAVE + lane] = 0.f;
  __syncthreads();

  // this wave's problems: pw0 .. pw0 + pwn - 1, problem pw0 + l on lane l.
  // Problems own disjoint centres, so the waves never meet in acc.
  const int per = (P + LLOYD_WAVES - 1) / LLOYD_WAVES;
  const int pw0 = w * per;
  const int pwn = max(0, min(P, pw0 + per) - pw0);
  int base = 0, k = 0;
  if (lane < pwn) lloyd_segment(seg, active, pw0 + lane, C, &base, &k);

  constexpr int U = 4;  // rows in flight
  for (int r = r0; r < r1 && pwn > 0; r += U) {
    float v[U];
    int s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int rr = r + u;
      const bool ok = rr < r1;
      v[u] = (ok && dok) ? x[(int64_t)rr * D + d] : 0.f;
      const int lab =
          (ok && k > 0) ? labels[(int64_t)(pw0 + lane) * N + rr] : -1;
      s[u] = (lab >= 0 && lab < k) ? base + lab : -1;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      for (int p = 0; p < pwn; ++p) {
        const int sp = __builtin_amdgcn_readlane(s[u], p);  // wave-uniform
        if (sp >= 0) acc[sp * WAVE + lane] += v[u];
      }
    }
  }
  __syncthreads();
  if (dok)
    for (int c = w; c < C; c += LLOYD_WAVES)
      psum[((int64_t)chunk * C + c) * D + d] = acc[c * WAVE + lane];
}

// One block per stacked centre: fold, divide, write in place, and the
// centre's squared shift to pshift[c].
__global__ void lloyd_fold_kernel(
    const float* __restrict__ psum, const int* __restrict__ counts,
    const int* __restrict__ seg, const int* __restrict__ active, int chunks,
    int D, int P, int C, float* __restrict__ centers,
    float* __restrict__ pshift) {
  __shared__ float wsum[4];
  const int c = blockIdx.x;
  int p = -1;
  for (int q = 0; q < P; ++q)
    if (seg[q] <= c && c < seg[q + 1]) p = q;
  int base, k;
  if (p < 0) return;
  lloyd_segment(seg, active, p, C, &base, &k);
  if (k == 0) return;  // inactive: centre and pshift untouched
  const int cnt = counts[c];
  float local = 0.f;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    const float old = centers[(int64_t)c * D + d];
    float nw = old;
    if (cnt > 0) {
      float s = 0.f;
      for (int ch = 0; ch < chunks; ++ch)
        s += psum[((int64_t)ch * C + c) * D + d];
      nw = s / (float)cnt;
      centers[(int64_t)c * D + d] = nw;
    }
    const float diff = nw - old;
    local += diff * diff;
  }
  for (int off = 32; off >= 1; off >>= 1) local += __shfl_xor(local, off);
  if (lane_id() == 0) wsum[wave_id()] = local;
  __syncthreads();
  if (threadIdx.x == 0) pshift[c] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

__global__ void lloyd_finish_kernel(
    const float* __restrict__ pshift, const int* __restrict__ seg,
    int* __restrict__ active, int P, int C, double tol,
    float* __restrict__ shift) {
  const int p = threadIdx.x;
  if (p >= P) return;
  int base, k;
  lloyd_segment(seg, active, p, C, &base, &k);
  float s = 0.f;
  for (int c = 0; c < k; ++c) s += pshift[base + c];
  shift[p] = s;
  if (k > 0 && (double)s <= tol) active[p] = 0;
}

void launch_lloyd_argmin(const float* d2, const int* seg, int n, int c, int p,
                         int* labels, float* mind, hipStream_t s) {
  dim3 grid(ceil_div(n, 256), p);
  lloyd_argmin_kernel<<<grid, 256, 0, s>>>(d2, seg, n, c, labels, mind);
}

int lloyd_chunks(int n) { return ceil_div(n, KMEANS_MANY_CHUNK_ROWS); }

void launch_lloyd_update(const float* x, const int* labels, float* centers,
                         const int* seg, int* active, int n, int d, int p,
                         int c, double tol, float* psum, float* pshift,
                         int* counts, float* shift, hipStream_t s) {
  const int chunks = lloyd_chunks(n);
  (void)hipMemsetAsync(counts, 0, sizeof(int) * c, s);
  lloyd_count_kernel<<<dim3(ceil_div(n, 256), p), 256, 0, s>>>(
      labels, seg, active, n, c, counts);
  lloyd_partial_kernel<<<dim3(ceil_div(d, WAVE), chunks), LLOYD_WAVES * WAVE,
                         sizeof(float) * c * WAVE, s>>>(
      x, labels, seg, active, n, d, p, c, psum);
  lloyd_fold_kernel<<<c, 256, 0, s>>>(psum, counts, seg, active, chunks, d, p,
                                      c, centers, pshift);
  lloyd_finish_kernel<<<1, WAVE, 0, s>>>(pshift, seg, active, p, c, tol,
                                         shift);
}
