// Host rule of the probed int8 scan (ivf_sq8.hip): the slice of candidate slots a workgroup serves.  The width
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

}  // namespace pvs
