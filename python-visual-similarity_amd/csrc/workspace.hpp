// Device scratch memory of a context: the slot names, the typed reserve, and the layout of a block that holds several buffers.
// Nothing here needs a HIP header, so a host-only program can include this file alone (bench/ws_layout_check.cpp does).
#pragma once
#include <cstddef>
#include <cstdint>

struct pvs_ctx;

namespace pvs {

// A context keeps 18 grow-only blocks of device memory (pvs_ctx::ws).  ws_reserve(ctx, slot, bytes, &p) hands out the slot's block,
// and when the block is too small it waits for the stream, FREES the block and allocates a larger one.  Hence the rule:
//
//   A pointer into a slot is dead once anything that may reserve the same slot has been called; re-reserve after such a call.
//
// Every function that reserves a slot is listed here; keep the table in step with `grep ws_reserve`.
//
//   WS_STAGE_IN       api.hip: pvs_vlad_encode, pvs_fisher_encode, pvs_cosine, pvs_cosine_topk, pvs_cosine_topk_f64 (host rows uploaded)
//   WS_SCRATCH        api.hip: pvs_vlad_encode_dev (labels), pvs_cosine_topk (norms | lists); cosine.hip: launch_cosine_f64 (norms);
//                     fisher.hip: launch_gmm_posterior, launch_gmm_em_step, launch_fisher (table | responsibilities | partials);
//                     learn.hip: launch_kmeans_step (twice), launch_label_sums, launch_gram, launch_seed_distances, launch_kmeanspp_run
//   WS_PANEL_OUT      api.hip: pvs_vlad_encode, pvs_fisher_encode, pvs_cosine (offsets | outputs of the host entry points),
//                     cosine_topk_impl (score row of one or two queries), pvs_kmeans_step_dev, pvs_gmm_em_step_dev, pvs_label_sums_dev,
//                     pvs_gram_dev, pvs_seed_distances_dev, pvs_seed_pick_dev, pvs_min_update_dev (statistics); panel_plan.hpp:
//                     panel_query_block (score panel, per query block) for cosine_topk_impl, pvs_cosine_topk_f64_dev, launch_cosine_topk_filtered,
//                     knn_f64_rows, pvs_l2_knn_dev, radius_impl, pvs_pq_scan_topk_dev, pvs_sq8_topk_dev, pvs_cosine_range_dev,
//                     pvs_cosine_topk_subset_dev, pvs_sq8_topk_subset_dev (and, through panel_query_block_sized, one block per call of
//                     pvs_sq8_range_dev in sq8_range.hip: float panel or bit mask | counters | row counts | row offsets; that entry
//                     reserves nothing else and tests/test_gpu_sq8_range.py runs it on poisoned and regrown blocks)
//   WS_PROJECTED     api.hip: project_if_needed (PCA rows), pvs_kmeanspp_run_dev; learn.hip: launch_label_sums (zero centres);
//                     filter.hip: launch_cosine_topk_filtered (rows and lists of the overflowing queries);
//                     range.hip: pvs_cosine_range_dev (candidate staging of the prefiltered path)
//                     subset.hip: pvs_cosine_topk_subset_dev, pvs_sq8_topk_subset_dev (gathered rows | factors of one chunk, listed path)
//   WS_AUX_ROWS       fisher.hip: materialise_f32 (RootSIFT rows); cosine.hip: launch_gemm_mfma, launch_gemm_f64 (split-K partials);
//                     learn.hip: launch_label_sums (squared rows), launch_gram (tile accumulator)
//   WS_FP16_ROWS      filter.hip: launch_cosine_topk_filtered; range.hip: pvs_cosine_range_dev (prefiltered path)
//   WS_LISTS          filter.hip: launch_cosine_topk_filtered; api.hip: pvs_cosine_topk_f64; vlad.hip: launch_assign;
//                     neighbors.hip: knn_f64_rows, pvs_l2_knn_dev; assign_topm.hip: pvs_kmeans_topm_dev (partial lists, splits > 1);
//                     range.hip: pvs_cosine_range_dev (norms of the fp16 rows | counters | row counts | row offsets),
//                     pvs_pair_components_dev (counters)
//   WS_NB_NORMS       neighbors.hip: pvs_l2_knn_dev, radius_impl
//   WS_NB_F64_ROWS    neighbors.hip: to_f64_copies
//   WS_DSIFT_TABLE    dsift.hip: pvs_dsift_dev
//   WS_SIFT_PYRAMID, WS_SIFT_TABLES, WS_SIFT_KEYPOINTS    sift.hip: pvs_sift_dev
//   WS_MATCH_TABLE    match.hip: upload_pairs, pvs_match_u8_dev
//   WS_VERIFY_POINTS, WS_VERIFY_SMALL    match.hip: pvs_verify_dev
//   WS_IVF_CANDIDATES ivf.hip: pvs_ivf_scan_topk_dev (candidate scores | candidate ids of one query block)
//                     ivf_sq8.hip: pvs_ivf_sq8_scan_topk_dev, pvs_ivf_sq8_scan_lists_topk_dev (the same layout)
//   WS_UPDATE         update.hip: pvs_keep_positions_dev (scan partials), pvs_compact_rows_dev in place (staging rows of one window),
//                     pvs_ivf_insert_dev (source of every merged row), pvs_ivf_remove_dev (stored keep mask | positions | scan partials);
//                     asmk_update.hip: pvs_asmk_invert_dev (two item arrays | digit counts | scan partials), pvs_asmk_remove_dev
//                     (survivor flags, scanned in place | scan partials); asmk_expand.hip: pvs_asmk_expand_dev (hit masks | chunk counts |
//                     chunk weight sums of one query block); ivf_sq8.hip: pvs_ivf_sq8_scan_lists_topk_dev, pvs_ivf_sq8_group_probes_dev
//                     (tile prefix | the grouping of one query block | the sort's items, digit counts and scan partials): a search
//                     calls no maintenance entry, so none of the users above is live in the same call
enum WsSlot : int {
  WS_STAGE_IN = 0, WS_SCRATCH = 1, WS_PANEL_OUT = 2, WS_PROJECTED = 3, WS_AUX_ROWS = 4, WS_FP16_ROWS = 5, WS_LISTS = 6, WS_NB_NORMS = 7,
  WS_NB_F64_ROWS = 8, WS_DSIFT_TABLE = 9, WS_SIFT_PYRAMID = 10, WS_SIFT_TABLES = 11, WS_SIFT_KEYPOINTS = 12, WS_MATCH_TABLE = 13,
  WS_VERIFY_POINTS = 14, WS_VERIFY_SMALL = 15, WS_IVF_CANDIDATES = 16, WS_UPDATE = 17
};

int ws_reserve(pvs_ctx* ctx, WsSlot which, size_t bytes, void** out);   // api.hip
template <class T>
inline int ws_reserve(pvs_ctx* ctx, WsSlot which, size_t bytes, T** out) {
  void* p = nullptr;
  const int rc = ws_reserve(ctx, which, bytes, &p);
  *out = static_cast<T*>(p);
  return rc;
}

constexpr size_t ws_round(size_t bytes, size_t align = 256) { return (bytes + align - 1) / align * align; }

// One buffer of a block: where it starts, and the typed pointer once the block's base is known.
template <class T>
struct WsPiece {
  size_t off = 0;
  T* operator()(void* base) const { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }
};

// Buffers of one block, in the order of the add() calls; each takes its bytes rounded up to ALIGN, so each starts on a multiple of it.
template <size_t ALIGN = 256>
class WsLayout {
  size_t end_ = 0;

 public:
  template <class T>
  WsPiece<T> add(size_t count) {
    const WsPiece<T> p{end_};
    end_ += ws_round(count * sizeof(T), ALIGN);
    return p;
  }
  size_t bytes() const { return end_; }
};

// ---- layouts that bench/ws_layout_check.cpp holds against their closed forms; the call sites build theirs through these functions.
// A braced list is evaluated left to right, so the pieces lie in the order of the struct's members.
// launch_cosine_topk_filtered, WS_LISTS: norms of the fp16 rows, counters, approximate lists, candidate lists, candidate counts
struct FilterListsLayout {
  WsPiece<float> invq, invdb;
  WsPiece<unsigned long long> stats;
  WsPiece<int64_t> aidx;
  WsPiece<float> aval;
  WsPiece<int64_t> cidx;
  WsPiece<float> cval;
  WsPiece<int> cnt;
  size_t bytes;
};
inline FilterListsLayout filter_lists_layout(size_t nq, size_t N, size_t QT, size_t k, size_t cap) {
  WsLayout<> l;
  return {l.add<float>(nq),       l.add<float>(N),          l.add<unsigned long long>(32), l.add<int64_t>(QT * k), l.add<float>(QT * k),
          l.add<int64_t>(QT * cap), l.add<float>(QT * cap), l.add<int>(QT),                l.bytes()};
}

// pvs_l2_knn_dev (float32), WS_LISTS: |y|^2 / 2 in f32, approximate lists, candidates, counts, keys, overflow counter
struct KnnF32Layout {
  WsPiece<float> hy;
  WsPiece<int64_t> aidx;
  WsPiece<float> aval;
  WsPiece<int64_t> cand;
  WsPiece<int> count;
  WsPiece<double> key;
  WsPiece<unsigned long long> ovf;
  size_t bytes;
};
inline KnnF32Layout knn_f32_layout(size_t N, size_t QT, size_t k, size_t cap) {
  WsLayout<> l;
  return {l.add<float>(N), l.add<int64_t>(QT * k), l.add<float>(QT * k), l.add<int64_t>(QT * cap), l.add<int>(QT), l.add<double>(QT * cap),
          l.add<unsigned long long>(32), l.bytes()};
}

// pvs_kmeanspp_run_dev, WS_PROJECTED: nblk = blocks of 4096 rows; `small` is the kernel's own 512 bytes of counters
struct KmeansppLayout {
  WsPiece<float> mind, dist, cand;
  WsPiece<double> block_sums, uniform;
  WsPiece<int64_t> indices;
  WsPiece<char> small;
  size_t bytes;
};
inline KmeansppLayout kmeanspp_layout(size_t total, size_t nblk, size_t D, size_t n_clusters, size_t trials) {
  WsLayout<> l;
  return {l.add<float>(total), l.add<float>(trials * total), l.add<float>(trials * D), l.add<double>(nblk),
          l.add<double>((n_clusters > 1 ? n_clusters - 1 : 1) * trials), l.add<int64_t>(n_clusters), l.add<char>(512), l.bytes()};
}

// pvs_sift_dev, WS_SIFT_KEYPOINTS (16-byte pieces): candidates, refined keypoints, three int tables of n_cand + 1, orientation bins
template <class Cand, class Kp>
struct SiftCandLayout {
  WsPiece<Cand> cand;
  WsPiece<Kp> kp;
  WsPiece<int> npeaks, nkeep, row_off;
  WsPiece<float> bins;
  size_t bytes;
};
template <class Cand, class Kp>
inline SiftCandLayout<Cand, Kp> sift_cand_layout(size_t n_cand, size_t max_peaks) {
  WsLayout<16> l;
  return {l.add<Cand>(n_cand), l.add<Kp>(n_cand), l.add<int>(n_cand + 1), l.add<int>(n_cand + 1), l.add<int>(n_cand + 1),
          l.add<float>(n_cand * max_peaks), l.bytes()};
}

// pvs_ivf_scan_topk_dev and pvs_ivf_sq8_scan_topk_dev, WS_IVF_CANDIDATES: one query block's candidate rows, QB queries x W slots each
struct IvfCandLayout {
  WsPiece<float> val;
  WsPiece<int32_t> id;
  size_t bytes;
};
inline IvfCandLayout ivf_cand_layout(size_t QB, size_t W) {
  WsLayout<> l;
  return {l.add<float>(QB * W), l.add<int32_t>(QB * W), l.bytes()};
}

// pvs_keep_positions_dev, WS_UPDATE: kept flags per tile, per block of `tile` tiles (at most `tile` blocks), and the total
struct UpdateScanLayout {
  WsPiece<int64_t> tile, block, top;
  size_t bytes;
};
inline UpdateScanLayout update_scan_layout(size_t ntiles, size_t tile) {
  WsLayout<> l;
  return {l.add<int64_t>(ntiles), l.add<int64_t>(tile), l.add<int64_t>(1), l.bytes()};
}

// pvs_compact_rows_dev in place, WS_UPDATE: the kept rows of one source window
constexpr size_t update_stage_bytes(size_t window_rows, size_t row_bytes) { return ws_round(window_rows * row_bytes); }

// pvs_ivf_remove_dev, WS_UPDATE: keep mask and positions in stored order, then the scan's partials
struct IvfRemoveLayout {
  WsPiece<uint8_t> keep;
  WsPiece<int64_t> pos, tile, block, top;
  size_t bytes;
};
inline IvfRemoveLayout ivf_remove_layout(size_t n, size_t ntiles, size_t tile) {
  WsLayout<> l;
  return {l.add<uint8_t>(n), l.add<int64_t>(n + 1), l.add<int64_t>(ntiles), l.add<int64_t>(tile), l.add<int64_t>(1), l.bytes()};
}

// pvs_asmk_invert_dev, WS_UPDATE: the (key, source slot) items of the radix sort in two arrays that the passes swap, the digit counts
// [257][ntiles] that one scan turns into positions, and that scan's partials (one per scan block of the counts)
struct AsmkInvertLayout {
  WsPiece<uint64_t> items_a, items_b;
  WsPiece<int32_t> counts, partials;
  size_t bytes;
};
inline AsmkInvertLayout asmk_invert_layout(size_t total, size_t ncounts, size_t nscanblocks) {
  WsLayout<> l;
  return {l.add<uint64_t>(total), l.add<uint64_t>(total), l.add<int32_t>(ncounts), l.add<int32_t>(nscanblocks), l.bytes()};
}

// pvs_asmk_remove_dev, WS_UPDATE: one survivor flag per stored entry and one more slot for the total, scanned in place, and the scan's partials
struct AsmkRemoveLayout {
  WsPiece<int32_t> spos, partials;
  size_t bytes;
};
inline AsmkRemoveLayout asmk_remove_layout(size_t entries, size_t nscanblocks) {
  WsLayout<> l;
  return {l.add<int32_t>(entries + 1), l.add<int32_t>(nscanblocks), l.bytes()};
}

// pvs_asmk_expand_dev, WS_UPDATE: for one block of `queries` queries the member hit mask of every word (chunks of 64 words), and per
// chunk the number of output entries (scanned in place into positions) and their weight sum
struct AsmkExpandLayout {
  WsPiece<uint32_t> mask;
  WsPiece<int32_t> cnt, wsum;
  size_t bytes;
};
inline AsmkExpandLayout asmk_expand_layout(size_t queries, size_t nchunks) {
  WsLayout<> l;
  return {l.add<uint32_t>(queries * nchunks * 64), l.add<int32_t>(queries * nchunks), l.add<int32_t>(queries * nchunks), l.bytes()};
}

// pvs_ivf_sq8_scan_lists_topk_dev and pvs_ivf_sq8_group_probes_dev, WS_UPDATE: the tile prefix of the lists; for one query block of
// `pairs` = queries x nprobe (query, probe) pairs the first slot of every pair, the live slots of every query, the group offsets of the
// lists, the query and the first slot of every grouped pair; then the sort's two item arrays, digit counts and scan partials
struct IvfSq8GroupLayout {
  WsPiece<int32_t> tile_off, base, total, goff, gq, gbase;
  WsPiece<uint64_t> items_a, items_b;
  WsPiece<int32_t> counts, partials;
  size_t bytes;
};
inline IvfSq8GroupLayout ivf_sq8_group_layout(size_t queries, size_t pairs, size_t nlist, size_t ncounts, size_t nscanblocks) {
  WsLayout<> l;
  return {l.add<int32_t>(nlist + 1), l.add<int32_t>(pairs),   l.add<int32_t>(queries), l.add<int32_t>(nlist + 1), l.add<int32_t>(pairs),
          l.add<int32_t>(pairs),     l.add<uint64_t>(pairs), l.add<uint64_t>(pairs),  l.add<int32_t>(ncounts),   l.add<int32_t>(nscanblocks),
          l.bytes()};
}

// pvs_kmeans_topm_dev with splits > 1, WS_LISTS: the partial lists [row][split][m], indices then values
struct TopmPartialLayout {
  WsPiece<int32_t> idx;
  WsPiece<float> val;
  size_t bytes;
};
inline TopmPartialLayout topm_partial_layout(size_t total, size_t splits, size_t m) {
  WsLayout<> l;
  return {l.add<int32_t>(total * splits * m), l.add<float>(total * splits * m), l.bytes()};
}

}  // namespace pvs
