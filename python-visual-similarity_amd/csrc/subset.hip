// Subset search: the k best among an allowed set S of rows, on the float32 and the int8 resident index.
//
//   pvs_subset_create / _destroy   the handle: sorted ids and a bitmask of the N rows on the device, the ids on the host too
//   pvs_cosine_topk_subset_dev     float32 rows, the score pvs_cosine_dev writes
//   pvs_sq8_topk_subset_dev        int8 code rows, ((float)acc * inv_q) * inv_d
//
// The result is the full ranking with the rows outside S deleted, cut to k; a score depends on its two rows and two factors alone, so
// both paths score with the project's own scorers (launch_cosine_f32, launch_sq8_scores) and the bits are rank's by construction.
//   mask path (1)    the panels of the unrestricted entry; a column panel without an id is skipped on the host (no launch), the others
//                    are scored, subset_mask_kernel writes -inf over the columns outside S, launch_topk merges as panel_topk does
//   listed path (2)  the sorted ids in chunks: rows (and factors) gathered into a staging block, scored, ranked by POSITION in the id
//                    list (positions ascend with indices, so ties resolve identically); subset_remap_kernel turns positions into ids
// No kernel here uses an atomic, and no list position is decided by one.
#include <algorithm>
#include <vector>

#include "panel_plan.hpp"
#include "subset_common.hpp"

struct pvs_subset {
  int64_t N = 0, ns = 0, nwords = 0;
  int64_t* d_ids = nullptr;      // [ns] ascending
  uint32_t* d_mask = nullptr;    // [nwords]
  std::vector<int64_t> h_ids;    // the host finds empty panels and cuts chunks from these
};

namespace pvs {

constexpr int SUB_SQ8_MAX_L = 131072;   // 127^2 L < 2^31, as sq8.hip
constexpr int SUB_THREADS = 256;          // four waves, each owning 64 consecutive columns
constexpr int SUB_MAX_ROW_BLOCKS = 1024;  // grid.y of the mask kernel; a workgroup strides over the rows

// panel[r][c] = -inf where column c0 + c is outside S.  A wave takes the 64 mask bits of its columns as one window (c0 need not be a
// multiple of 32: the window then straddles words); lane l owns bit l.  Rows and columns are guarded; plain vector stores.
__global__ __launch_bounds__(SUB_THREADS) void subset_mask_kernel(float* __restrict__ panel, int64_t rows, int64_t cols, int64_t ld,
                                                                  const uint32_t* __restrict__ mask, int64_t nwords, int64_t c0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t cb = ((int64_t)blockIdx.x * (SUB_THREADS / WAVE) + wave) * WAVE;   // first column of this wave
  if (cb >= cols) return;
  const uint64_t window = subset_window64(mask, nwords, c0 + cb);
  const int64_t c = cb + lane;
  if (c >= cols || ((window >> lane) & 1ull)) return;
  for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) panel[r * ld + c] = -INFINITY;
}

// idx[i] = ids[idx[i]]: list positions -> row indices of the full index; an unfilled slot (-1) stays -1
__global__ __launch_bounds__(SUB_THREADS) void subset_remap_kernel(int64_t* __restrict__ idx, int64_t n, const int64_t* __restrict__ ids,
                                                                   int64_t ns) {
  const int64_t i = (int64_t)blockIdx.x * SUB_THREADS + threadIdx.x;
  if (i >= n) return;
  const int64_t p = idx[i];
  idx[i] = (p >= 0 && p < ns) ? ids[p] : -1;
}

namespace {

int launch_subset_mask(pvs_ctx* ctx, float* panel, int64_t qn, int64_t cn, const pvs_subset* s, int64_t c0) {
  ScopedTimer tm(ctx, T_TOPK);
  const dim3 grid((unsigned)((cn + SUB_THREADS - 1) / SUB_THREADS), (unsigned)std::min<int64_t>(qn, SUB_MAX_ROW_BLOCKS));
  hipLaunchKernelGGL(subset_mask_kernel, grid, dim3(SUB_THREADS), 0, ctx->stream, panel, qn, cn, cn, s->d_mask, s->nwords, c0);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

// what both entries refuse before anything is launched
int subset_check(const char* fn, const pvs_subset* s, int64_t nq, int64_t N, int k, int path, int tile) {
  if (nq < 0 || nq > 0x7fffffffLL) PVS_FAIL(PVS_ERR_INVALID, "%s: need 0 <= nq < 2^31 (got %lld)", fn, (long long)nq);
  if (s->N != N) PVS_FAIL(PVS_ERR_INVALID, "%s: the subset was made for %lld rows, the index holds %lld", fn, (long long)s->N, (long long)N);
  if (k < 1 || k > s->ns) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= k <= |S| (k = %d, |S| = %lld)", fn, k, (long long)s->ns);
  if (k > SUBSET_MAX_K) PVS_FAIL(PVS_ERR_INVALID, "%s: a subset ranking holds at most %d entries (k = %d)", fn, SUBSET_MAX_K, k);
  if (path < 0 || path > 2) PVS_FAIL(PVS_ERR_INVALID, "%s: path must be 0, 1 or 2 (got %d)", fn, path);
  if (tile < 0 || tile > SUBSET_MAX_TILE) PVS_FAIL(PVS_ERR_INVALID, "%s: tile must be 0..%d (got %d)", fn, SUBSET_MAX_TILE, tile);
  return PVS_OK;
}

PanelPlan subset_plan(PanelPlan (*rule)(int64_t, int64_t), int64_t nq, int64_t cols, int tile) {
  return tile ? PanelPlan{nq, cols, std::min<int64_t>(nq, tile), std::min<int64_t>(cols, tile)} : rule(nq, cols);
}

// Mask path: score(q0, qn, c0, cn, panel) fills a panel of the resident rows c0 .. c0 + cn.  The loop is panel_topk's, except that a
// column panel without an id costs nothing, so "merge" is "this query block has ranked a panel before".
template <class Score>
int subset_mask_path(pvs_ctx* ctx, const PanelPlan& plan, const pvs_subset* s, int k, int64_t* d_idx, float* d_val, int64_t* stats,
                     Score&& score) {
  for (int64_t q0 = 0; q0 < plan.nq; q0 += plan.QT) {
    bool ranked = false;
    PVS_TRY(panel_query_block<float>(ctx, plan, q0, [&](int64_t, int64_t qn, int64_t c0, int64_t cn, float* panel) -> int {
      if (subset_panel_empty(s->h_ids.data(), s->ns, c0, cn)) {
        ++stats[2];
        return PVS_OK;
      }
      PVS_TRY(score(q0, qn, c0, cn, panel));
      PVS_TRY(launch_subset_mask(ctx, panel, qn, cn, s, c0));
      ++stats[1];
      const int merge = ranked ? 1 : 0;
      ranked = true;
      return launch_topk(ctx, panel, qn, cn, cn, k, c0, merge, d_idx + q0 * k, d_val + q0 * k);
    }));
  }
  return PVS_OK;
}

// Listed path: gather(p0, pn) brings the rows (and factors) of the ids at positions p0 .. p0 + pn into the staging block, then
// score(q0, qn, c0, cn, panel) fills a panel of the STAGED rows c0 .. c0 + cn.  Columns are positions in the id list.
template <class Gather, class Score>
int subset_listed_path(pvs_ctx* ctx, PanelPlan (*rule)(int64_t, int64_t), int64_t nq, const pvs_subset* s, int64_t chunk_rows, int k,
                       int tile, int64_t* d_idx, float* d_val, int64_t* stats, Gather&& gather, Score&& score) {
  for (int64_t p0 = 0; p0 < s->ns; p0 += chunk_rows) {
    const int64_t pn = std::min(chunk_rows, s->ns - p0);
    PVS_TRY(gather(p0, pn));
    ++stats[1];
    stats[3] += pn;
    PVS_TRY(panel_topk(ctx, subset_plan(rule, nq, pn, tile), k, p0, p0 > 0 ? 1 : 0, d_idx, d_val, score));
  }
  ScopedTimer tm(ctx, T_MISC);
  const int64_t n = nq * k;
  hipLaunchKernelGGL(subset_remap_kernel, dim3((unsigned)((n + SUB_THREADS - 1) / SUB_THREADS)), dim3(SUB_THREADS), 0, ctx->stream, d_idx, n,
                     s->d_ids, s->ns);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

// staging block of the listed path in WS_PROJECTED: the gathered rows (16 spare bytes, see the float32 entry), then their factors
struct SubsetStage {
  char* rows = nullptr;
  float* inv = nullptr;
};
int subset_stage(pvs_ctx* ctx, int64_t chunk_rows, int64_t row_bytes, SubsetStage* st) {
  WsLayout<> lay;
  const auto rows_p = lay.add<char>((size_t)chunk_rows * (size_t)row_bytes + 16);
  const auto inv_p = lay.add<float>((size_t)chunk_rows);
  char* base = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_PROJECTED, lay.bytes(), &base));
  st->rows = rows_p(base);
  st->inv = inv_p(base);
  return PVS_OK;
}

}  // namespace
}  // namespace pvs

using namespace pvs;

PVS_EXPORT int pvs_subset_create(pvs_ctx* ctx, const int64_t* h_ids, int64_t ns, int64_t N, pvs_subset** out) {
  PVS_NEED(ctx, "ctx");
  PVS_NEED(out, "out");
  *out = nullptr;
  if (N < 1 || N > 0x7fffffffLL) PVS_FAIL(PVS_ERR_INVALID, "pvs_subset_create: need 1 <= N < 2^31 (got %lld)", (long long)N);
  if (ns < 1 || ns > N) PVS_FAIL(PVS_ERR_INVALID, "pvs_subset_create: need 1 <= |S| <= N (|S| = %lld, N = %lld)", (long long)ns, (long long)N);
  PVS_NEED(h_ids, "ids");
  if (const int64_t bad = subset_first_bad_id(h_ids, ns, N))
    PVS_FAIL(PVS_ERR_INVALID, "pvs_subset_create: ids must ascend strictly within [0, %lld): entry %lld is %lld", (long long)N,
             (long long)(bad - 1), (long long)h_ids[bad - 1]);
  PVS_HIP(hipSetDevice(ctx->device));
  pvs_subset* s = new pvs_subset;
  s->N = N;
  s->ns = ns;
  s->nwords = subset_words(N);
  s->h_ids.assign(h_ids, h_ids + ns);
  std::vector<uint32_t> words((size_t)s->nwords);
  subset_build_mask(h_ids, ns, N, words.data());
  hipError_t e = hipMalloc(&s->d_ids, (size_t)ns * sizeof(int64_t));
  if (e == hipSuccess) e = hipMalloc(&s->d_mask, (size_t)s->nwords * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemcpyAsync(s->d_ids, h_ids, (size_t)ns * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(s->d_mask, words.data(), (size_t)s->nwords * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // the host arrays may go away after the call
  if (e != hipSuccess) {
    if (s->d_ids) (void)hipFree(s->d_ids);
    if (s->d_mask) (void)hipFree(s->d_mask);
    delete s;
    set_error("pvs_subset_create: allocation or upload failed: %s", hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? PVS_ERR_OOM : PVS_ERR_NO_DEVICE;
  }
  *out = s;
  return PVS_OK;
}

PVS_EXPORT int pvs_subset_destroy(pvs_ctx* ctx, pvs_subset* subset) {
  if (!subset) return PVS_OK;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);   // launches that read the ids or the mask may still be queued
  }
  if (subset->d_ids) (void)hipFree(subset->d_ids);
  if (subset->d_mask) (void)hipFree(subset->d_mask);
  delete subset;
  return PVS_OK;
}

PVS_EXPORT int pvs_cosine_topk_subset_dev(pvs_ctx* ctx, const float* d_Q, int64_t nq, const float* d_DB, int64_t N, int64_t L,
                                          const float* d_inv_q, const float* d_inv_db, const pvs_subset* subset, int k, int path, int tile,
                                          int64_t* d_idx, float* d_val, int64_t* h_stats) {
  PVS_NEED(ctx, "ctx");
  PVS_NEED(subset, "subset");
  if (h_stats) std::fill(h_stats, h_stats + 4, (int64_t)0);
  PVS_TRY(subset_check(__func__, subset, nq, N, k, path, tile));
  if (L < 1 || L > 0x7fffffffLL) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= L < 2^31", __func__);
  if (nq == 0) return PVS_OK;
  PVS_NEED(d_Q, "Q");
  PVS_NEED(d_DB, "DB");
  PVS_NEED(d_idx, "idx");
  PVS_NEED(d_val, "val");
  PVS_ALIGNED(d_Q, 4, "Q");
  PVS_ALIGNED(d_DB, 4, "DB");
  PVS_ALIGNED(d_idx, 8, "idx");
  PVS_ALIGNED(d_val, 4, "val");
  PVS_HIP(hipSetDevice(ctx->device));
  if (path == 0) path = subset_auto_listed(subset->ns, N) ? 2 : 1;
  int64_t stats[4] = {path, 0, 0, 0};
  int rc;
  if (path == 1) {
    rc = subset_mask_path(ctx, subset_plan(panel_dense, nq, N, tile), subset, k, d_idx, d_val, stats,
                          [&](int64_t q0, int64_t qn, int64_t c0, int64_t cn, float* panel) -> int {
                            return launch_cosine_f32(ctx, d_Q + q0 * L, qn, d_DB + c0 * L, cn, L, d_inv_q ? d_inv_q + q0 : nullptr,
                                                     d_inv_db ? d_inv_db + c0 : nullptr, panel, cn);
                          });
  } else {
    const int64_t row_bytes = L * (int64_t)sizeof(float);
    const int64_t chunk_rows = subset_chunk_rows(subset->ns, row_bytes, tile);
    SubsetStage st;
    PVS_TRY(subset_stage(ctx, chunk_rows, row_bytes, &st));
    // the staged rows start on 16 bytes exactly when the resident ones do, so launch_cosine_f32 takes the kernel class it takes for them
    float* rows = reinterpret_cast<float*>(st.rows + reinterpret_cast<uintptr_t>(d_DB) % 16);
    rc = subset_listed_path(
        ctx, panel_dense, nq, subset, chunk_rows, k, tile, d_idx, d_val, stats,
        [&](int64_t p0, int64_t pn) -> int {
          PVS_TRY(pvs_graph_gather_rows_dev(ctx, d_DB, N, row_bytes, subset->d_ids + p0, pn, rows));
          return d_inv_db ? pvs_graph_gather_rows_dev(ctx, d_inv_db, N, 4, subset->d_ids + p0, pn, st.inv) : PVS_OK;
        },
        [&](int64_t q0, int64_t qn, int64_t c0, int64_t cn, float* panel) -> int {
          return launch_cosine_f32(ctx, d_Q + q0 * L, qn, rows + c0 * L, cn, L, d_inv_q ? d_inv_q + q0 : nullptr,
                                   d_inv_db ? st.inv + c0 : nullptr, panel, cn);
        });
  }
  if (h_stats) std::copy(stats, stats + 4, h_stats);
  return rc;
}

PVS_EXPORT int pvs_sq8_topk_subset_dev(pvs_ctx* ctx, const int8_t* d_qcodes, const float* d_inv_q, int64_t nq, const int8_t* d_codes,
                                       const float* d_inv_db, int64_t N, int L, const pvs_subset* subset, int k, int path, int tile,
                                       int64_t* d_idx, float* d_val, int64_t* h_stats) {
  PVS_NEED(ctx, "ctx");
  PVS_NEED(subset, "subset");
  if (h_stats) std::fill(h_stats, h_stats + 4, (int64_t)0);
  PVS_TRY(subset_check(__func__, subset, nq, N, k, path, tile));
  if (L < 1 || L > SUB_SQ8_MAX_L) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= L <= %d (got %d)", __func__, SUB_SQ8_MAX_L, L);
  if (nq == 0) return PVS_OK;
  PVS_NEED(d_qcodes, "qcodes");
  PVS_NEED(d_inv_q, "inv_q");
  PVS_NEED(d_codes, "codes");
  PVS_NEED(d_inv_db, "inv_db");
  PVS_NEED(d_idx, "idx");
  PVS_NEED(d_val, "val");
  PVS_ALIGNED(d_qcodes, 16, "qcodes");
  PVS_ALIGNED(d_codes, 16, "codes");
  PVS_ALIGNED(d_inv_q, 4, "inv_q");
  PVS_ALIGNED(d_inv_db, 4, "inv_db");
  PVS_ALIGNED(d_idx, 8, "idx");
  PVS_ALIGNED(d_val, 4, "val");
  PVS_HIP(hipSetDevice(ctx->device));
  const int ld = PVS_SQ8_LD(L);
  const bool rows_scan = sq8_row_scan(ctx, nq);   // PVS_OPT_SQ8_PATH, as pvs_sq8_topk_dev reads it: the same bits either way
  if (path == 0) path = subset_auto_listed(subset->ns, N) ? 2 : 1;
  int64_t stats[4] = {path, 0, 0, 0};
  int rc;
  if (path == 1) {
    rc = subset_mask_path(ctx, subset_plan(panel_scan, nq, N, tile), subset, k, d_idx, d_val, stats,
                          [&](int64_t q0, int64_t qn, int64_t c0, int64_t cn, float* panel) -> int {
                            ScopedTimer t(ctx, T_GEMM);
                            return launch_sq8_scores(ctx, rows_scan, d_qcodes + q0 * ld, d_inv_q + q0, qn, d_codes + c0 * ld, d_inv_db + c0, cn, ld,
                                                     panel);
                          });
  } else {
    const int64_t chunk_rows = subset_chunk_rows(subset->ns, ld, tile);
    SubsetStage st;
    PVS_TRY(subset_stage(ctx, chunk_rows, ld, &st));
    int8_t* codes = reinterpret_cast<int8_t*>(st.rows);
    rc = subset_listed_path(
        ctx, panel_scan, nq, subset, chunk_rows, k, tile, d_idx, d_val, stats,
        [&](int64_t p0, int64_t pn) -> int {
          PVS_TRY(pvs_graph_gather_rows_dev(ctx, d_codes, N, ld, subset->d_ids + p0, pn, codes));
          return pvs_graph_gather_rows_dev(ctx, d_inv_db, N, 4, subset->d_ids + p0, pn, st.inv);
        },
        [&](int64_t q0, int64_t qn, int64_t c0, int64_t cn, float* panel) -> int {
          ScopedTimer t(ctx, T_GEMM);
          return launch_sq8_scores(ctx, rows_scan, d_qcodes + q0 * ld, d_inv_q + q0, qn, codes + c0 * ld, st.inv + c0, cn, ld, panel);
        });
  }
  if (h_stats) std::copy(stats, stats + 4, h_stats);
  return rc;
}
