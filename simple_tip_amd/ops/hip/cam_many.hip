// Batched CAM: the greedy set covers of up to CAM_MANY_MAX_PROBLEMS
// independent problems in one persistent launch (docs/kernels.md, "Batched
// CAM"; profiles/r13_cam_many.md).
//
// The grid is one block of 256 threads per CU, at most 256, divided by the
// host into one TEAM of consecutive blocks per problem (cam_many_teams). A
// team runs the greedy loop of cam.hip on its own problem: sweep -> block
// maxima -> team barrier -> the team's first block picks the winner and
// clears its columns from the uncovered mask -> team barrier. Teams share
// nothing and never wait for each other; a team that has finished exits.
//
// What differs from cam.hip's loop:
//  - gain[row] = popcount(row & uncovered) is kept in global memory. A row
//    whose gain is 0 is dead for good (the mask only shrinks), which is the
//    dead-row pruning; the picked row's own gain drops to 0 with its pick.
//  - after a pick the first block publishes newly = row[win] & uncovered as
//    (word, mask) pairs of its non-zero words. When the list is short
//    (L * CAM_MANY_INCR_DIV <= W, L <= CAM_MANY_LIST_CAP) the next sweep
//    only subtracts popcount(row[word] & mask) over the list from every live
//    gain, one row per thread; otherwise it recounts against the whole mask.
//  - full sweeps of wide profiles (W >= CAM_MANY_WIDE_WORDS) give a row to a
//    wave, lanes striding the words, so the loads coalesce.
//  - every wait is bounded (CAM_MANY_WAIT_TICKS): a block whose wait runs
//    out sets its problem's status word and leaves, its team-mates run into
//    the same bound, and the host raises instead of returning an order.
// All counts are integers, so the picks equal cam.hip's whatever the team
// size, the sweep form or the update form.

#include "cam_many.h"
#include "tip_common.h"

#include <algorithm>

namespace {

struct Best {
  int v;
  int i;
};

TIP_DEV Best best_combine(Best a, Best b) {
  if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
  return a;
}

TIP_DEV Best wave_best(Best b) {
  for (int off = 32; off >= 1; off >>= 1) {
    Best o{__shfl_xor(b.v, off), __shfl_xor(b.i, off)};
    b = best_combine(b, o);
  }
  return b;
}

TIP_DEV int wave_sum(int v) {
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// Words another block of the team writes during the launch are read with
// agent-scope atomics where the address is uniform: a vector load past the
// L1, never the scalar cache.
TIP_DEV int ld_agent(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

TIP_DEV void st_agent(int* p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Barrier of one team on its own monotonic counter: every wave releases its
// stores at agent scope, one lane arrives (release), polls relaxed and
// acquires once. Returns false when the wait ran out; the status word is
// then set and the caller leaves the kernel.
TIP_DEV bool team_barrier(int* ctr, int target, long long* status,
                          int* s_ok) {
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_AGENT);
    const long long t0 = wall_clock64();
    int ok = 1;
    while (ld_agent(ctr) < target) {
      if (wall_clock64() - t0 > CAM_MANY_WAIT_TICKS) {
        ok = 0;
        break;
      }
      __builtin_amdgcn_s_sleep(2);
    }
    if (!ok)
      __hip_atomic_store(status, 1ll, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    *s_ok = ok;
  }
  __syncthreads();
  return *s_ok != 0;
}

// Full recount of the team's rows against the mask `unc` (LDS or global).
template <bool WIDE>
TIP_DEV Best sweep_full(const CamManyDesc& d, const unsigned long long* unc,
                        int tb, bool first) {
  Best best{0, 0x7fffffff};
  const int W = d.W;
  if (WIDE) {  // a wave per row, lanes stride the words
    const int lane = lane_id();
    const int nwaves = d.team * (256 / WAVE);
    for (int row = tb * (256 / WAVE) + wave_id(); row < d.rows;
         row += nwaves) {
      if (!first && ld_agent(d.gain + row) == 0) continue;
      const unsigned long long* r = d.words + (int64_t)row * W;
      int c = 0;
#pragma unroll 4
      for (int w = lane; w < W; w += WAVE) c += __popcll(r[w] & unc[w]);
      c = wave_sum(c);
      if (lane == 0) d.gain[row] = c;
      if (c > 0) best = best_combine(best, Best{c, row});
    }
  } else {  // a thread per row
    const int nthreads = d.team * 256;
    for (int row = tb * 256 + threadIdx.x; row < d.rows; row += nthreads) {
      if (!first && d.gain[row] == 0) continue;
      const unsigned long long* r = d.words + (int64_t)row * W;
      int c = 0;
      for (int w = 0; w < W; ++w) c += __popcll(r[w] & unc[w]);
      d.gain[row] = c;
      if (c > 0) best = best_combine(best, Best{c, row});
    }
  }
  return best;
}

__launch_bounds__(256) __global__
    void cam_many_kernel(const CamManyDesc* __restrict__ table, int problems) {
  // the uncovered mask of a full sweep, or the (word, mask) list of an
  // incremental one
  __shared__ unsigned long long sbuf[CAM_MANY_LDS_WORDS];
  __shared__ int sv[256 / WAVE];
  __shared__ int si[256 / WAVE];
  __shared__ int s_ok, s_win, s_cnt;

  int p = -1;
  for (int q = 0; q < problems; ++q) {
    const int fb = table[q].first_block;
    if ((int)blockIdx.x >= fb && (int)blockIdx.x < fb + table[q].team) p = q;
  }
  if (p < 0) return;  // a block no team needs
  const CamManyDesc d = table[p];

  const int tid = threadIdx.x;
  const int lane = lane_id();
  const int wid = wave_id();
  const int tb = blockIdx.x - d.first_block;  // team-local block
  const int tthread = tb * 256 + tid;
  const int nthreads = d.team * 256;
  const int W = d.W;
  const bool use_lds = W <= CAM_MANY_LDS_WORDS;
  int* ctr = d.sync;
  int* win_slot = d.sync + 1;
  int* len_slot = d.sync + 2;
  int round_ = 0;

  for (int w = tthread; w < W; w += nthreads)
    d.uncovered[w] = (w == W - 1) ? d.tail_mask : ~0ull;
  if (!team_barrier(ctr, ++round_ * d.team, d.status, &s_ok)) return;

  for (int picks = 0;;) {
    // length of the last pick's list; 0 asks for a full sweep
    const int L = picks == 0 ? 0 : ld_agent(len_slot);
    Best best{0, 0x7fffffff};
    if (L > 0) {
      for (int i = tid; i < 2 * L; i += 256) sbuf[i] = d.list[i];
      __syncthreads();
      for (int row = tthread; row < d.rows; row += nthreads) {
        int g = d.gain[row];
        if (g == 0) continue;
        const unsigned long long* r = d.words + (int64_t)row * W;
        for (int i = 0; i < L; ++i)
          g -= __popcll(r[sbuf[2 * i]] & sbuf[2 * i + 1]);
        d.gain[row] = g;
        if (g > 0) best = best_combine(best, Best{g, row});
      }
    } else {
      if (use_lds) {  // per-block copy: sweep reads hit LDS, not L2
        for (int w = tid; w < W; w += 256) sbuf[w] = d.uncovered[w];
        __syncthreads();
      }
      const bool first = picks == 0;
      if (d.wide)
        best = use_lds ? sweep_full<true>(d, sbuf, tb, first)
                       : sweep_full<true>(d, d.uncovered, tb, first);
      else
        best = use_lds ? sweep_full<false>(d, sbuf, tb, first)
                       : sweep_full<false>(d, d.uncovered, tb, first);
    }
    best = wave_best(best);
    if (lane == 0) {
      sv[wid] = best.v;
      si[wid] = best.i;
    }
    __syncthreads();
    if (tid == 0) {
      Best b{0, 0x7fffffff};
      for (int w = 0; w < 256 / WAVE; ++w)
        b = best_combine(b, Best{sv[w], si[w]});
      d.part_val[tb] = b.v;
      d.part_idx[tb] = b.i;
    }
    if (!team_barrier(ctr, ++round_ * d.team, d.status, &s_ok)) return;

    if (tb == 0) {
      if (wid == 0) {
        Best b{0, 0x7fffffff};
        for (int q = lane; q < d.team; q += WAVE)
          b = best_combine(b, Best{d.part_val[q], d.part_idx[q]});
        b = wave_best(b);
        if (lane == 0) {
          s_win = b.v > 0 ? b.i : -1;
          s_cnt = 0;
        }
      }
      __syncthreads();
      const int win = s_win;
      if (win >= 0) {
        const unsigned long long* r = d.words + (int64_t)win * W;
        for (int w = tid; w < W; w += 256) {
          const unsigned long long u = d.uncovered[w];
          const unsigned long long newly = r[w] & u;
          if (newly) {
            d.uncovered[w] = u & ~newly;
            const int pos = atomicAdd(&s_cnt, 1);
            if (pos < d.list_cap) {
              d.list[2 * pos] = (unsigned long long)w;
              d.list[2 * pos + 1] = newly;
            }
          }
        }
        __syncthreads();
      }
      if (tid == 0) {
        if (win >= 0) {
          d.order[picks] = win;
          st_agent(len_slot, s_cnt <= d.list_cap ? s_cnt : 0);
        }
        st_agent(win_slot, win);
        *d.count = picks + (win >= 0 ? 1 : 0);
      }
    }
    if (!team_barrier(ctr, ++round_ * d.team, d.status, &s_ok)) return;
    if (ld_agent(win_slot) < 0 || ++picks >= d.rows) break;
  }
}

}  // namespace

std::vector<int> cam_many_teams(const std::vector<int64_t>& rows,
                                const std::vector<int64_t>& W, int grid) {
  const int P = (int)rows.size();
  std::vector<int> team(P, 1), cap(P, 1);
  unsigned long long total = 0;
  for (int p = 0; p < P; ++p) {
    // blocks the rows can occupy: 4 rows per block when a wave takes a row
    const int64_t per_block = W[p] >= CAM_MANY_WIDE_WORDS ? 256 / WAVE : 256;
    const int64_t need = (rows[p] + per_block - 1) / per_block;
    cap[p] = (int)std::max<int64_t>(
        1, std::min<int64_t>(need, CAM_MANY_TEAM_CAP));
    total += (unsigned long long)rows[p] * (unsigned long long)W[p];
  }
  int left = grid - P;
  if (left <= 0 || total == 0) return team;
  const unsigned long long spare = (unsigned long long)left;
  for (int p = 0; p < P; ++p) {
    const unsigned long long w =
        (unsigned long long)rows[p] * (unsigned long long)W[p];
    const int extra = (int)(spare * w / total);
    team[p] = std::min(cap[p], 1 + extra);
    left -= team[p] - 1;
  }
  // what rounding and the caps left over: one block at a time, in order
  for (bool moved = true; left > 0 && moved;) {
    moved = false;
    for (int p = 0; p < P && left > 0; ++p)
      if (team[p] < cap[p]) {
        ++team[p];
        --left;
        moved = true;
      }
  }
  return team;
}

int cam_many_grid() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                            dev) != hipSuccess)
    return 0;
  return std::min(cus, CAM_MANY_MAX_GRID);
}

void launch_cam_many(const CamManyDesc* table, int problems, int grid,
                     hipStream_t s) {
  cam_many_kernel<<<grid, 256, 0, s>>>(table, problems);
}
