// Subset search: the bit arithmetic of the allowed-set mask and the host rules around it.  Host and device
// share this file; nothing here needs a HIP header, so bench/subset_plan_check.cpp includes it alone, with a host compiler.
//   mask      ceil(N / 32) uint32 words, row i is bit (i & 31) of word (i >> 5); the bits beyond N in the last word are zero
//   window    the 64 mask bits of the columns col0 .. col0 + 63 for ANY col0: bit l is column col0 + l.  col0 % 32 != 0 makes the
//             window straddle three words; a word at or beyond `nwords` reads as zero (those columns do not exist)
//   chunks    the listed path takes the sorted ids in runs of subset_chunk_rows(...) positions
//   empty     a column panel [c0, c0 + cn) without an id is found by a binary search on the sorted host ids
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define PVS_HD __host__ __device__
#else
#define PVS_HD
#endif

namespace pvs {

constexpr int64_t SUBSET_STAGE_BYTES = (int64_t)256 << 20;   // gathered rows of one chunk; only a single row may be larger
constexpr int SUBSET_MAX_K = 1024;                           // one launch_topk page: a deeper list cannot merge across panels
constexpr int SUBSET_MAX_TILE = 32768;

PVS_HD inline int64_t subset_words(int64_t N) { return (N + 31) >> 5; }

PVS_HD inline uint32_t subset_word(const uint32_t* mask, int64_t nwords, int64_t w) { return w < nwords ? mask[w] : 0u; }

PVS_HD inline uint64_t subset_window64(const uint32_t* mask, int64_t nwords, int64_t col0) {
  const int64_t w = col0 >> 5;
  const int s = (int)(col0 & 31);
  const uint64_t lo = (uint64_t)subset_word(mask, nwords, w) | ((uint64_t)subset_word(mask, nwords, w + 1) << 32);
  if (s == 0) return lo;                                     // a shift by 64 below would be undefined
  return (lo >> s) | ((uint64_t)subset_word(mask, nwords, w + 2) << (64 - s));
}

// ---- host rules
// strictly ascending ids within [0, N): 0 = fine, otherwise the 1-based position of the first offender
inline int64_t subset_first_bad_id(const int64_t* ids, int64_t ns, int64_t N) {
  for (int64_t p = 0; p < ns; ++p)
    if (ids[p] < 0 || ids[p] >= N || (p > 0 && ids[p] <= ids[p - 1])) return p + 1;
  return 0;
}

// words[0 .. subset_words(N)) from valid ids
inline void subset_build_mask(const int64_t* ids, int64_t ns, int64_t N, uint32_t* words) {
  std::fill(words, words + subset_words(N), 0u);
  for (int64_t p = 0; p < ns; ++p) words[ids[p] >> 5] |= 1u << (ids[p] & 31);
}

// positions [first, last) of the ids that lie in the column panel [c0, c0 + cn); first == last: the panel holds none
inline void subset_panel_range(const int64_t* ids, int64_t ns, int64_t c0, int64_t cn, int64_t* first, int64_t* last) {
  *first = std::lower_bound(ids, ids + ns, c0) - ids;
  *last = std::lower_bound(ids, ids + ns, c0 + cn) - ids;
}
inline bool subset_panel_empty(const int64_t* ids, int64_t ns, int64_t c0, int64_t cn) {
  int64_t a, b;
  subset_panel_range(ids, ns, c0, cn, &a, &b);
  return a == b;
}

// rows of one staged chunk: what SUBSET_STAGE_BYTES hold, one row at least, all ns at most; tile > 0 caps it (a test seam)
inline int64_t subset_chunk_rows(int64_t ns, int64_t row_bytes, int tile) {
  int64_t rows = std::max<int64_t>(1, std::min<int64_t>(ns, SUBSET_STAGE_BYTES / std::max<int64_t>(row_bytes, 1)));
  if (tile > 0) rows = std::min<int64_t>(rows, tile);
  return rows;
}

// path 0: the listed path iff 4 ns <= N (bytes moved: three passes over a listed row against one pass over every row, one pass of margin)
inline bool subset_auto_listed(int64_t ns, int64_t N) { return ns <= N / 4; }   // == 4 ns <= N, without the product

}  // namespace pvs
