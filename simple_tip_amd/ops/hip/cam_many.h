// Descriptors and constants of the batched CAM kernel (cam_many.hip), shared
// with bindings.cpp. Plain C++.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

constexpr int CAM_MANY_MAX_PROBLEMS = 32;  // problems (teams) per launch
constexpr int CAM_MANY_MAX_GRID = 256;     // one block of 256 threads per CU
constexpr int CAM_MANY_TEAM_CAP = 64;      // blocks per team (cam.hip's CAM_NB)
constexpr int CAM_MANY_LDS_WORDS = 2048;   // mask words / list pairs * 2 in LDS
// full sweeps give a row to a wave from this width on, to a thread below it
constexpr int CAM_MANY_WIDE_WORDS = 64;
// a pick whose `newly` mask has L non-zero words updates the gains from the
// list when L * CAM_MANY_INCR_DIV <= W and L <= CAM_MANY_LIST_CAP; a longer
// list means a full re-sweep
constexpr int CAM_MANY_INCR_DIV = 8;
constexpr int CAM_MANY_LIST_CAP = CAM_MANY_LDS_WORDS / 2;
// a team's polled words sit on a 128-byte line of their own
constexpr int CAM_MANY_SYNC_WORDS = 32;
// bound of every wait, in ticks of the 100 MHz constant-rate clock: 2 s
constexpr long long CAM_MANY_WAIT_TICKS = 200000000LL;

// One problem of a launch. Blocks first_block .. first_block + team - 1 are
// its team; every pointer is to that problem's own storage.
struct CamManyDesc {
  const unsigned long long* words;  // [rows, W], read where the caller has it
  unsigned long long* uncovered;    // [W], initialised by the kernel
  int* gain;                        // [rows] remaining coverage; 0 = dead row
  int* part_val;                    // [team] block maxima
  int* part_idx;                    // [team]
  unsigned long long* list;         // [2 * list_cap] (word, mask) of a pick
  long long* order;                 // [rows] picked prefix
  long long* count;                 // picks made
  long long* status;                // 0, or 1 once a bounded wait ran out
  int* sync;                        // [CAM_MANY_SYNC_WORDS], zeroed per call
  unsigned long long tail_mask;     // valid bits of word W - 1
  int rows, W;
  int first_block, team;
  int list_cap;                     // min(W / CAM_MANY_INCR_DIV, LIST_CAP)
  int wide;                         // W >= CAM_MANY_WIDE_WORDS
};

// Blocks per problem for a grid of `grid` blocks: one each, the rest in
// proportion to rows * W, never more than a problem's rows can occupy nor
// than CAM_MANY_TEAM_CAP. A function of the shapes and `grid` only.
std::vector<int> cam_many_teams(const std::vector<int64_t>& rows,
                                const std::vector<int64_t>& W, int grid);
// min(CAM_MANY_MAX_GRID, CUs of the current device); 0 if the query fails
int cam_many_grid();
void launch_cam_many(const CamManyDesc* table, int problems, int grid,
                     hipStream_t);
