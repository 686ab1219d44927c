// Host rules of the probed int8 scans (ivf_sq8.hip).  Below the slices: the query block and the tiles of the scan by list (DESIGN.md
// section 28; bench/ivf_sq8_lists_plan_check.cpp includes this file alone, too).
// The scan by query: the slice of candidate slots a workgroup serves.  The width
// of a candidate row and the query block are section 14's (ivf_candidate_width, ivf_query_block of list_common.hpp: both probed scans
// size the WS_IVF_CANDIDATES block the same way); the slice rule is this unit's own, because a slot here is a row of up to 128 KiB
// walked by a wave, not m bytes read by a lane.  Integer arithmetic only and no HIP header: bench/ivf_sq8_plan_check.cpp includes
// this file alone, with a host compiler.
#pragma once
#include <algorithm>
#include <cstdint>

#include "list_common.hpp"

namespace pvs {

constexpr int ISQ_THREADS = 1024;                           // sixteen waves, each walking whole stored rows
constexpr int ISQ_WAVES = ISQ_THREADS / 64;
constexpr int ISQ_MAX_PROBE = 1024;                         // one probe per thread of the workgroup
constexpr int64_t ISQ_MIN_SLICE = 64;                       // slots a workgroup serves at least when the host chooses: its LDS copy of
                                                            // the query is then at most 1/64 of the bytes it reads

struct IsqSlices {
  int64_t S;   // slots per workgroup: a multiple of 16, so every wave of a full slice walks the same number of rows
  int64_t G;   // workgroups per query: slice g serves [g S, min((g + 1) S, W))
};

// slice_rows > 0: that many slots, rounded up to a multiple of 16 (a test seam).  0: about two workgroups per compute unit over the
// query block, never fewer than ISQ_MIN_SLICE slots per workgroup.  W is a multiple of 64, W >= 64.
inline IsqSlices isq_slices(int num_cu, int64_t QB, int64_t W, int64_t slice_rows) {
  int64_t S;
  if (slice_rows > 0) {
    S = (slice_rows + ISQ_WAVES - 1) / ISQ_WAVES * ISQ_WAVES;
  } else {
    const int64_t want = (2 * (int64_t)num_cu + QB - 1) / QB;
    const int64_t G0 = std::max<int64_t>(1, std::min<int64_t>(want, W / ISQ_MIN_SLICE));
    S = ((W + G0 - 1) / G0 + ISQ_WAVES - 1) / ISQ_WAVES * ISQ_WAVES;
  }
  return {S, (W + S - 1) / S};
}

// ---- the scan by list: the probes of a query block are grouped by list, and a workgroup scores one tile of
// ISQL_ROWS consecutive stored rows of one list against the grouped pairs of that list, ISQL_PAIRS at a time, on the matrix pipe
constexpr int ISQL_ROWS = 128;                              // stored rows of a row tile: never across a list's end
constexpr int ISQL_PAIRS = 128;                             // grouped (query, probe) pairs of a query tile: never across a group's end
constexpr int64_t ISQL_PAIR_BYTES = 32;                     // grouping arrays per pair: two sort items of 8, base, gq, gbase of 4, rounded up
constexpr int64_t ISQL_GROUP_BYTES = (int64_t)32 << 20;     // budget of those arrays for one query block: 2^20 pairs
constexpr int64_t ISQL_MAX_PAIRS = ISQL_GROUP_BYTES / ISQL_PAIR_BYTES;

// row tiles of a list of len rows, query tiles of a group of n pairs: a list of length 0 has no tile
// (constexpr: the device code of ivf_sq8.hip calls them too)
constexpr int64_t isql_list_tiles(int64_t len) { return (len + ISQL_ROWS - 1) / ISQL_ROWS; }
constexpr int64_t isql_query_tiles(int64_t n) { return (n + ISQL_PAIRS - 1) / ISQL_PAIRS; }

struct IsqlPlan {
  int64_t W;           // slots of a candidate row (ivf_candidate_width)
  int64_t QB;          // queries of one block
  int64_t row_tiles;   // workgroups of the tile kernel: the sum of isql_list_tiles over the lists
  int64_t pairs;       // grouped pairs the block's arrays hold: QB nprobe
};

// query_block > 0: at most that many queries (a test seam).  The host rule under it: ivf_query_block(nq, W), capped so that QB nprobe
// pairs stay within ISQL_GROUP_BYTES.  h_list_off has passed offsets_first_break; nq >= 1; 1 <= nprobe <= min(nlist, ISQ_MAX_PROBE)
inline IsqlPlan isql_plan(const int64_t* h_list_off, int nlist, int nprobe, int64_t nq, int64_t query_block) {
  IsqlPlan p;
  p.W = ivf_candidate_width(h_list_off, nlist, nprobe);
  p.QB = std::min<int64_t>(ivf_query_block(nq, p.W), std::max<int64_t>(1, ISQL_MAX_PAIRS / nprobe));
  if (query_block > 0) p.QB = std::min(p.QB, query_block);
  p.row_tiles = 0;
  for (int l = 0; l < nlist; ++l) p.row_tiles += isql_list_tiles(h_list_off[l + 1] - h_list_off[l]);
  p.pairs = p.QB * nprobe;
  return p;
}

}  // namespace pvs
