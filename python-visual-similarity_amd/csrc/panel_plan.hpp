// Score panels: the block sizes of every ranker's QT x NC score panel in WS_PANEL_OUT and the two loops around
// it.  The geometry is part of the result where a GEMM's split-K plan follows the panel shape (float64), so the rules are pinned value
// by value.  The host part needs no HIP header: bench/panel_plan_check.cpp includes this file alone, with a host compiler.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/pvsim.h"

namespace pvs {

void set_error(const char* fmt, ...);   // api.hip (bench/panel_plan_check.cpp brings its own)

constexpr int64_t PANEL_BUDGET_BYTES = (int64_t)1 << 30;   // 1 GiB of scores; only a single complete row may be larger
template <class T>
constexpr int64_t panel_elems() { return PANEL_BUDGET_BYTES / (int64_t)sizeof(T); }   // 2^28 floats, 2^27 doubles
constexpr int PANEL_PAGED_K = 1024;   // a deeper ranking pages through complete score rows (topk.hip)

// Blocks of QT queries x NC database rows over an nq x N problem (N >= 1); the last block of either axis may be short.
struct PanelPlan {
  int64_t nq, N, QT, NC;
  int64_t qn(int64_t q0) const { return std::min(QT, nq - q0); }
  int64_t cn(int64_t c0) const { return std::min(NC, N - c0); }
};
template <class T>
inline size_t panel_bytes(const PanelPlan& p) { return (size_t)p.QT * (size_t)p.NC * sizeof(T); }

// f32 / f16 GEMM + select, f32 kNN prefilter: 8192 x 32768 floats are the whole budget
inline PanelPlan panel_dense(int64_t nq, int64_t N) { return {nq, N, std::min<int64_t>(nq, 8192), std::min<int64_t>(N, 32768)}; }
// ADC and Int8 scans: 2^22 floats (16 MiB stay in the last-level cache between scan and select), 1024 queries, 4096 columns at least
inline PanelPlan panel_scan(int64_t nq, int64_t N) {
  const int64_t QT = std::min<int64_t>(nq, 1024);
  return {nq, N, QT, std::min<int64_t>(N, std::max<int64_t>(4096, ((int64_t)1 << 22) / QT))};
}
// complete rows: as many queries as `elems` scores hold, one query when a single row is larger than that
inline PanelPlan panel_full_rows(int64_t nq, int64_t N, int64_t elems) {
  return {nq, N, std::max<int64_t>(1, std::min<int64_t>(nq, elems / N)), N};
}
// Filtered top-k, panels of 32768 database rows: `same_operands` (Q == DB with one norm array) over a single column block within the
// budget is ONE symmetric launch for all queries; otherwise as many queries as the budget holds, 256 at least.
inline PanelPlan panel_filter(int64_t nq, int64_t N, bool same_operands) {
  const int64_t NC = std::min<int64_t>(N, 32768);
  const bool square = same_operands && N <= NC && nq * N <= panel_elems<float>();
  return {nq, N, square ? nq : std::min<int64_t>(nq, std::max<int64_t>(256, panel_elems<float>() / NC)), NC};
}
// Int8 threshold join, mask path (sq8_range.hip): the panel is one BIT per pair, so the column panels are eight times as wide as the
// dense rule's: 8192 x 262144 bits.  A mask row is `panel_mask_words` uint32 words (whole 128-column tiles of the GEMM), the rows are
// rounded up to whole 128-row tiles: 8192 x 8192 words = 256 MiB at most, a quarter of the budget.
constexpr int64_t PANEL_MASK_QT = 8192, PANEL_MASK_NC = 262144;
inline PanelPlan panel_mask(int64_t nq, int64_t N) { return {nq, N, std::min<int64_t>(nq, PANEL_MASK_QT), std::min<int64_t>(N, PANEL_MASK_NC)}; }
constexpr int64_t panel_mask_words(int64_t cols) { return 4 * ((cols + 127) / 128); }
inline size_t panel_mask_bytes(const PanelPlan& p) {
  return (size_t)((p.QT + 127) / 128 * 128) * (size_t)panel_mask_words(p.NC) * sizeof(uint32_t);
}
// A ranking of depth k: `bounded` (panel_dense or panel_scan) up to PANEL_PAGED_K, complete rows beyond -- which cannot continue the
// lists of an earlier call (merge) nor hold more than 2^28 scores: PVS_ERR_UNSUPPORTED, raised here for every ranker.
inline int panel_ranking_plan(PanelPlan (*bounded)(int64_t, int64_t), int64_t nq, int64_t N, int k, int merge, PanelPlan* plan) {
  if (k > PANEL_PAGED_K && (merge || N > panel_elems<float>())) {
    set_error("ranking depth %d needs a single panel", k);
    return PVS_ERR_UNSUPPORTED;
  }
  *plan = k > PANEL_PAGED_K ? panel_full_rows(nq, N, panel_elems<float>()) : bounded(nq, N);
  return PVS_OK;
}
// Query rows per upload of pvs_cosine_topk_f64: what one float64 panel holds, 2 GiB of rows at most.  DEFECT, kept: with
// the same operands it is all nq rows, uncapped, so the _dev form tiles them by panel_full_rows -- other blocks, other split-K plans.
inline int64_t host_f64_query_block(int64_t nq, int64_t N, int64_t L, bool same_operands) {
  if (same_operands) return nq;
  return std::max<int64_t>(1, std::min<int64_t>(nq, std::min<int64_t>(panel_elems<double>() / N, ((int64_t)256 << 20) / L)));
}

}  // namespace pvs

#ifdef __HIPCC__
#include "common.hpp"

namespace pvs {

// One query block: reserve WS_PANEL_OUT for a panel of T, then body(q0, qn, c0, cn, panel) per column block.  The reserve stands at
// the top of EVERY query block (two compares when large enough): what a site runs between query blocks may take the slot, a body must not.
// panel_query_block_sized: the same over a block of `bytes` bytes, for a site whose panel is not QT x NC elements of T or that keeps
// more than the panel in the block (the int8 threshold join: a bit mask, and its counters behind the panel).
template <class T, class Body>
inline int panel_query_block_sized(pvs_ctx* ctx, const PanelPlan& p, size_t bytes, int64_t q0, Body&& body) {
  T* panel = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_PANEL_OUT, bytes, &panel));
  for (int64_t c0 = 0; c0 < p.N; c0 += p.NC) PVS_TRY(body(q0, p.qn(q0), c0, p.cn(c0), panel));
  return PVS_OK;
}
template <class T, class Body>
inline int panel_query_block(pvs_ctx* ctx, const PanelPlan& p, int64_t q0, Body&& body) {
  return panel_query_block_sized<T>(ctx, p, panel_bytes<T>(p), q0, body);
}
// every query block in turn; a site with work between query blocks writes this loop itself around panel_query_block
template <class T, class Body>
inline int panel_for_each(pvs_ctx* ctx, const PanelPlan& p, Body&& body) {
  for (int64_t q0 = 0; q0 < p.nq; q0 += p.QT) PVS_TRY(panel_query_block<T>(ctx, p, q0, body));
  return PVS_OK;
}
// score(q0, qn, c0, cn, panel) fills the qn x cn panel (ld = cn); launch_topk continues the caller's lists over the column blocks
template <class Score>
inline int panel_topk(pvs_ctx* ctx, const PanelPlan& p, int k, int64_t col_offset, int merge, int64_t* d_idx, float* d_val, Score&& score) {
  return panel_for_each<float>(ctx, p, [&](int64_t q0, int64_t qn, int64_t c0, int64_t cn, float* panel) -> int {
    PVS_TRY(score(q0, qn, c0, cn, panel));
    return launch_topk(ctx, panel, qn, cn, cn, k, col_offset + c0, (merge || c0 > 0) ? 1 : 0, d_idx + q0 * k, d_val + q0 * k);
  });
}

}  // namespace pvs
#endif  // __HIPCC__
