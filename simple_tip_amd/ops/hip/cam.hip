// Device-resident CAM greedy set cover.
//
// One persistent kernel runs the whole greedy loop. Each iteration:
// score[i] = popcount(profile[i] & uncovered) with a fused grid argmax
// (ties -> lowest row, np.argmax semantics), then block 0 records the
// winner and clears its columns from the uncovered mask in place. The host
// reads back the picked prefix once at the end; the O(N*W) popcount sweep —
// the reference's per-iteration numpy hot loop (prioritizers.py:16-59) —
// never leaves the device. The mask lives in global memory and is staged
// in LDS per block when it fits (W <= 2048 words); wider masks are swept
// straight from global memory by the same kernel.

#include "tip_common.h"

struct MaxIdxLL {
  long long v;
  int i;
};

TIP_DEV MaxIdxLL max_combine(MaxIdxLL a, MaxIdxLL b) {
  if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
  return a;
}

// Persistent multi-block CAM — the only path. Alternatives measured and
// rejected (profiles/r02_cam_ladder.md): a per-iteration two-kernel form
// (score + pick, since removed) was dispatch-bound at ~200 us/pick, and a
// single-block whole-loop kernel was sweep-bound on
// one CU (~340 us/pick). This kernel keeps CAM_NB blocks RESIDENT (1 block
// per CU is guaranteed co-residency on 256 CUs, so the software grid
// barrier cannot deadlock) and runs the whole greedy loop with two
// barriers per iteration: parallel sweep -> block partials -> barrier ->
// block 0 picks + updates the global uncovered mask -> barrier.
// Rows whose remaining coverage hits 0 are marked dead (uncovered only
// shrinks, so c==0 is permanent) and skip future sweeps.
constexpr int CAM_NB = 64;

TIP_DEV void cam_grid_barrier(int* ctr, int* round_) {
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_AGENT);
    const int target = (++(*round_)) * CAM_NB;
    // spin on relaxed LOADS: an RMW spin serializes all waiters on one
    // cacheline and cost ~100 us per barrier at 64 blocks
    while (__hip_atomic_load(ctr, __ATOMIC_ACQUIRE,
                             __HIP_MEMORY_SCOPE_AGENT) < target)
      __builtin_amdgcn_s_sleep(2);
  }
  __syncthreads();
}

__launch_bounds__(256) __global__ void cam_greedy_coop_kernel(
    const unsigned long long* __restrict__ words, int rows, int W,
    unsigned long long init_tail_mask, unsigned char* __restrict__ used,
    unsigned long long* __restrict__ uncovered,  // [W] global
    long long* __restrict__ part_val, int* __restrict__ part_idx,
    long long* __restrict__ order_out, int* __restrict__ n_out,
    int* __restrict__ barrier_ctr, int* __restrict__ win_slot) {
  __shared__ long long sv[4];
  __shared__ int si[4];
  constexpr int LDS_W = 2048;  // up to 128K profile bits staged in LDS
  __shared__ unsigned long long sunc[LDS_W];
  const bool use_lds = W <= LDS_W;
  const int tid = threadIdx.x;
  const int lane = lane_id();
  const int wid = wave_id();
  const int gthread = blockIdx.x * blockDim.x + tid;
  const int nthreads = CAM_NB * blockDim.x;
  int round_ = 0;
  // grid-stride: W may exceed the grid's 16384 threads (profiles wider than
  // 2^20 bits), and the buffer arrives uninitialised
  for (int w = gthread; w < W; w += nthreads)
    uncovered[w] = (w == W - 1) ? init_tail_mask : ~0ull;
  if (gthread == 0) {
    *n_out = 0;
    *win_slot = 0;
  }
  cam_grid_barrier(barrier_ctr, &round_);

  for (;;) {
    if (use_lds) {  // per-block copy: sweep reads hit LDS, not L2
      for (int w = tid; w < W; w += blockDim.x) sunc[w] = uncovered[w];
      __syncthreads();
    }
    const unsigned long long* unc = use_lds ? sunc : uncovered;
    MaxIdxLL best{-1, 0x7fffffff};
    for (int row = gthread; row < rows; row += nthreads) {
      if (used[row]) continue;
      long long c = 0;
      const unsigned long long* r = words + (int64_t)row * W;
      for (int w = 0; w < W; ++w) c += __popcll(r[w] & unc[w]);
      if (c == 0) {
        used[row] = 1;  // permanently dead: uncovered only shrinks
        continue;
      }
      best = max_combine(best, MaxIdxLL{c, row});
    }
    for (int off = 32; off >= 1; off >>= 1) {
      MaxIdxLL o{__shfl_xor(best.v, off), __shfl_xor(best.i, off)};
      best = max_combine(best, o);
    }
    if (lane == 0) {
      sv[wid] = best.v;
      si[wid] = best.i;
    }
    __syncthreads();
    if (tid == 0) {
      MaxIdxLL b{-1, 0x7fffffff};
      for (int w = 0; w < (int)(blockDim.x / WAVE); ++w)
        b = max_combine(b, MaxIdxLL{sv[w], si[w]});
      part_val[blockIdx.x] = b.v;
      part_idx[blockIdx.x] = b.i;
    }
    cam_grid_barrier(barrier_ctr, &round_);
    if (blockIdx.x == 0) {
      if (tid == 0) {
        MaxIdxLL b{-1, 0x7fffffff};
        for (int p = 0; p < CAM_NB; ++p)
          b = max_combine(b, MaxIdxLL{part_val[p], part_idx[p]});
        if (b.v > 0) {
          order_out[(*n_out)++] = b.i;
          used[b.i] = 1;
          *win_slot = b.i;
        } else {
          *win_slot = -1;
        }
      }
      __syncthreads();
      const int win = *win_slot;
      if (win >= 0) {
        const unsigned long long* r = words + (int64_t)win * W;
        for (int w = tid; w < W; w += blockDim.x) uncovered[w] &= ~r[w];
      }
    }
    cam_grid_barrier(barrier_ctr, &round_);
    if (*win_slot < 0 || *n_out >= rows) break;
  }
}

void launch_cam_greedy_coop(const unsigned long long* words, int rows, int W,
                            unsigned long long init_tail_mask,
                            unsigned char* used,
                            unsigned long long* uncovered, long long* part_val,
                            int* part_idx, long long* order_out, int* n_out,
                            int* barrier_ctr, int* win_slot, hipStream_t s) {
  cam_greedy_coop_kernel<<<CAM_NB, 256, 0, s>>>(
      words, rows, W, init_tail_mask, used, uncovered, part_val, part_idx,
      order_out, n_out, barrier_ctr, win_slot);
}
