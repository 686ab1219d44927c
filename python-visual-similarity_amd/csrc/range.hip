// Cosine threshold join and pair components: "everything at least this similar".
//
//   pvs_cosine_range_dev     every (query row, database row, score) with score >= t, in a defined order, into a COO list of a given
//                            capacity; PVS_RANGE_UPPER = the self-join, pairs j > i only.
//   pvs_pair_components_dev  the connected components of such a pair list: label = smallest member.
//
// The score is the float32 value pvs_cosine_dev writes: the exact path (1) scores QT x NC panels with that very launch and thresholds
// them where they lie (count per row -> one-workgroup scan that starts at the running total -> ordered emit; the panel stays in
// WS_PANEL_OUT between the three launches).  The prefiltered path (2) scores the panels with fp16 operands under the proven bound
// |s16 - s32| <= eps(L) of filter.hip, keeps every pair with s16 >= t - eps (ONE eps: the threshold does not move, unlike a k-th best),
// re-scores the kept pairs with the defined recurrence of the f32 GEMM and keeps s32 >= t.  Both paths emit a row block's hits in the
// same order, so the lists are equal entry by entry.  No output position is decided by an atomic.  The count / scan / emit kernels
// are in range_common.hpp: the int8 join of sq8_range.hip runs them too.
#include <algorithm>
#include <cmath>

#include "range_common.hpp"

namespace pvs {

constexpr int RNG_LIST_LD = 1024;    // a flat candidate list is compacted as rows of this many entries
constexpr int RNG_PASS = 16;         // pairs re-scored together by one workgroup
constexpr int RNG_SK = 32;           // k-values per chain slab staged in LDS
constexpr int RNG_THREADS = RNG_PASS * 32;
// path 0: the prefiltered path from this many query rows on, the exact path below (profiles/range_timing.jsonl at 8189 x 32768: the
// prefilter wins at 1024 queries, 4.1 against 7.3 ms, and in the self-join, 3.4 against 15.7 ms; one query loses, 1.16 against 0.93 ms)
constexpr int64_t RNG_AUTO_FILTER_ROWS = 1024;

// ---- exact scores of a flat pair list by the defined recurrence of the f32 GEMM (filter.hip's header): per pair the chain
// acc = fma(a[k], b[k], acc) over k in the order (8t+e, 8t+4+e), chains of 1024 k, sums added in order, then (0 + tot) * (inv_a * inv_b).
// The work split of filter_rescore_kernel: RNG_PASS pairs x 32 chain lanes, both operands through LDS in 32-k slabs with the next slab
// in flight; here every pair brings its own query row.
__global__ __launch_bounds__(RNG_THREADS) void range_rescore_pairs_kernel(const float* __restrict__ Q, const float* __restrict__ DB, int64_t L,
                                                                         const float* __restrict__ invq, const float* __restrict__ invdb,
                                                                         const int64_t* __restrict__ prow, const int64_t* __restrict__ pcol,
                                                                         int64_t npairs, float* __restrict__ out) {
  __shared__ float a_s[RNG_PASS][32][RNG_SK + 1];
  __shared__ float b_s[RNG_PASS][32][RNG_SK + 1];
  __shared__ float csum[RNG_PASS][32];
  const int tid = threadIdx.x;
  const int cand = tid >> 5, c = tid & 31;
  const int64_t p0 = (int64_t)blockIdx.x * RNG_PASS;
  const int npass = (int)min((int64_t)RNG_PASS, npairs - p0);
  const bool valid = cand < npass;
  const int64_t nchunks = (L + 1023) / 1024;
  // staging roles: every thread loads 8 float4 of the query slabs and 8 of the database slabs: slot u is pair 2u + (tid >> 8)
  float4 ra[8], rb[8];
  const float* arow[8];
  const float* brow[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int cd = 2 * u + (tid >> 8);
    arow[u] = brow[u] = nullptr;
    if (cd < npass) {
      arow[u] = Q + prow[p0 + cd] * L;
      brow[u] = DB + pcol[p0 + cd] * L;
    }
  }
  auto fetch = [&](int64_t r0, int s) {
    const int rem = tid & 255, cc = rem >> 3, w = rem & 7;
    const int64_t kk = (r0 + cc) * 1024 + (int64_t)s * RNG_SK + 4 * w;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const bool in = arow[u] != nullptr && kk < L;
      ra[u] = in ? *reinterpret_cast<const float4*>(arow[u] + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
      rb[u] = in ? *reinterpret_cast<const float4*>(brow[u] + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = tid + RNG_THREADS * u;
      const int cd = idx >> 8, rem = idx & 255, cc = rem >> 3, w = rem & 7;
      a_s[cd][cc][4 * w] = ra[u].x; a_s[cd][cc][4 * w + 1] = ra[u].y; a_s[cd][cc][4 * w + 2] = ra[u].z; a_s[cd][cc][4 * w + 3] = ra[u].w;
      b_s[cd][cc][4 * w] = rb[u].x; b_s[cd][cc][4 * w + 1] = rb[u].y; b_s[cd][cc][4 * w + 2] = rb[u].z; b_s[cd][cc][4 * w + 3] = rb[u].w;
    }
  };
  float tot = 0.f;
  for (int64_t r0 = 0; r0 < nchunks; r0 += 32) {
    float acc = 0.f;
    fetch(r0, 0);
    for (int s = 0; s < 1024 / RNG_SK; ++s) {
      __syncthreads();           // the previous slab has been consumed
      stash();
      __syncthreads();
      if (s + 1 < 1024 / RNG_SK) fetch(r0, s + 1);   // in flight during the chain below
#pragma unroll
      for (int b8 = 0; b8 < RNG_SK; b8 += 8)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc = fmaf(a_s[cand][c][b8 + e], b_s[cand][c][b8 + e], acc);
          acc = fmaf(a_s[cand][c][b8 + 4 + e], b_s[cand][c][b8 + 4 + e], acc);
        }
    }
    csum[cand][c] = acc;
    __syncthreads();
    if (c == 0) {
      const int lim = (int)min((int64_t)32, nchunks - r0);
      for (int cc = 0; cc < lim; ++cc) tot += csum[cand][cc];
    }
  }
  if (c == 0 && valid) {
    const float sa = invq[prow[p0 + cand]], sb = invdb[pcol[p0 + cand]];
    out[p0 + cand] = (0.f + tot) * (sa * sb);
  }
}

// ---- pair components: min-label hooking.  parent[x] <= x always and a parent lies in x's component, so chains end at a root.
__global__ void comp_check_kernel(const int64_t* __restrict__ a, const int64_t* __restrict__ b, int64_t E, int64_t N, int* __restrict__ bad) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x)
    if (a[e] < 0 || a[e] >= N || b[e] < 0 || b[e] >= N) *bad = 1;      // every writer stores the same value
}
__global__ void comp_init_kernel(int32_t* __restrict__ parent, int64_t N) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) parent[i] = (int32_t)i;
}
__device__ __forceinline__ int32_t comp_root(const int32_t* parent, int32_t x) {
  for (;;) {
    const int32_t p = __atomic_load_n(parent + x, __ATOMIC_RELAXED);
    if (p == x) return x;
    x = p;
  }
}
__global__ void comp_hook_kernel(const int64_t* __restrict__ a, const int64_t* __restrict__ b, int64_t E, int32_t* parent, int* __restrict__ changed) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const int32_t ra = comp_root(parent, (int32_t)a[e]), rb = comp_root(parent, (int32_t)b[e]);
    if (ra != rb) {
      atomicMin(parent + max(ra, rb), min(ra, rb));
      *changed = 1;
    }
  }
}
__global__ void comp_compress_kernel(int32_t* parent, int64_t N) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t r = comp_root(parent, (int32_t)i);
    if (r != (int32_t)i) __atomic_store_n(parent + i, r, __ATOMIC_RELAXED);
  }
}
// the integer histogram of the roots has one non-empty bin per component: count the nodes that are their own label
__global__ __launch_bounds__(256) void comp_count_roots_kernel(const int32_t* __restrict__ label, int64_t N, unsigned long long* __restrict__ count) {
  int n = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) n += label[i] == (int32_t)i;
  for (int m = 32; m >= 1; m >>= 1) n += __shfl_xor(n, m, 64);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(count, (unsigned long long)n);
}

namespace {

struct RangeJob {
  pvs_ctx* ctx;
  const float* Q;
  const float* DB;
  int64_t nq, N, L;
  const float* invq;
  const float* invdb;
  float thr;
  int upper;
  int64_t capacity;
  int64_t* d_row;
  int64_t* d_col;
  float* d_val;
  PanelPlan plan;
  int* counts;          // WS_LISTS
  int64_t* offsets;
  int64_t* totals;      // [0] output entries so far, [1] staged candidates of the current row block
  int64_t stats[6];
};

template <bool LIST>
int range_compact(RangeJob& j, const RangeSrc& src, int64_t* total, int64_t cap, int64_t* o_row, int64_t* o_col, float* o_val) {
  return range_compact<LIST>(j.ctx, j.counts, j.offsets, src, total, cap, o_row, o_col, o_val);   // range_common.hpp
}

bool tile_below_diagonal(const RangeJob& j, int64_t q0, int64_t c0, int64_t cn) { return range_tile_below_diagonal(j.upper, q0, c0, cn); }

// one row block by the exact path: f32 panels thresholded into the output
int range_exact_block(RangeJob& j, int64_t q0) {
  return panel_query_block<float>(j.ctx, j.plan, q0, [&](int64_t, int64_t qn, int64_t c0, int64_t cn, float* panel) -> int {
    if (tile_below_diagonal(j, q0, c0, cn)) {
      ++j.stats[4];
      return PVS_OK;
    }
    PVS_TRY(launch_cosine_f32(j.ctx, j.Q + q0 * j.L, qn, j.DB + c0 * j.L, cn, j.L, j.invq ? j.invq + q0 : nullptr,
                              j.invdb ? j.invdb + c0 : nullptr, panel, cn));
    ++j.stats[3];
    const RangeSrc src{panel, cn, qn, cn, q0, c0, nullptr, nullptr, 0, j.thr, j.upper};
    return range_compact<false>(j, src, j.totals, j.capacity, j.d_row, j.d_col, j.d_val);
  });
}

}  // namespace

}  // namespace pvs

using namespace pvs;

PVS_EXPORT int pvs_cosine_range_dev(pvs_ctx* ctx, const float* d_Q, int64_t nq, const float* d_DB, int64_t N, int64_t L,
                                    const float* d_inv_q, const float* d_inv_db, float threshold, int flags, int path, int tile,
                                    int64_t capacity, int64_t* d_row, int64_t* d_col, float* d_val, int64_t* h_total, int64_t* h_stats) {
  PVS_NEED(ctx, "ctx");
  PVS_NEED(h_total, "total");
  if (!std::isfinite(threshold)) PVS_FAIL(PVS_ERR_INVALID, "pvs_cosine_range_dev: the threshold must be finite");
  if (flags & ~PVS_RANGE_UPPER) PVS_FAIL(PVS_ERR_INVALID, "pvs_cosine_range_dev: unknown flags %d", flags);
  if (nq < 0 || N < 0 || nq > 0x7fffffffLL || N > 0x7fffffffLL) PVS_FAIL(PVS_ERR_INVALID, "pvs_cosine_range_dev: need 0 <= nq, N < 2^31");
  if ((flags & PVS_RANGE_UPPER) && nq != N)
    PVS_FAIL(PVS_ERR_INVALID, "pvs_cosine_range_dev: PVS_RANGE_UPPER joins a set with itself (nq = %lld, N = %lld)", (long long)nq, (long long)N);
  if (path < 0 || path > 2) PVS_FAIL(PVS_ERR_INVALID, "pvs_cosine_range_dev: path must be 0, 1 or 2 (got %d)", path);
  if (tile < 0 || tile > 32768) PVS_FAIL(PVS_ERR_INVALID, "pvs_cosine_range_dev: tile must be 0..32768 (got %d)", tile);
  if (capacity < 0 || capacity > PVS_RANGE_MAX_CAPACITY) PVS_FAIL(PVS_ERR_INVALID, "pvs_cosine_range_dev: capacity out of range");
  if (capacity > 0) {
    PVS_NEED(d_row, "row output");
    PVS_NEED(d_col, "col output");
    PVS_NEED(d_val, "val output");
  }
  *h_total = 0;
  if (h_stats) std::fill(h_stats, h_stats + 6, (int64_t)0);
  if (nq == 0 || N == 0) return PVS_OK;
  if (L < 1) PVS_FAIL(PVS_ERR_INVALID, "pvs_cosine_range_dev: L must be positive");
  PVS_NEED(d_Q, "Q");
  PVS_NEED(d_DB, "DB");
  PVS_HIP(hipSetDevice(ctx->device));

  RangeJob j{};
  j.ctx = ctx; j.Q = d_Q; j.DB = d_DB; j.nq = nq; j.N = N; j.L = L; j.invq = d_inv_q; j.invdb = d_inv_db;
  j.thr = threshold; j.upper = flags & PVS_RANGE_UPPER; j.capacity = capacity; j.d_row = d_row; j.d_col = d_col; j.d_val = d_val;
  j.plan = tile ? PanelPlan{nq, N, std::min<int64_t>(nq, tile), std::min<int64_t>(N, tile)} : panel_dense(nq, N);

  if (path == 0) path = nq >= RNG_AUTO_FILTER_ROWS ? 2 : 1;
  // path 2 qualifies as the filtered top-k does, and needs both norm arrays (the bound holds for normalised scores)
  bool filtered = path == 2 && d_inv_q && d_inv_db && L % 8 == 0 && L >= 8 && L <= (int64_t)8 * 1024 * 1024 &&
                  reinterpret_cast<uintptr_t>(d_Q) % 16 == 0 && reinterpret_cast<uintptr_t>(d_DB) % 16 == 0;
  const int64_t stage_cap = 2 * capacity + 4096;
  int64_t *srow = nullptr, *scol = nullptr;
  float* sval = nullptr;
  if (filtered) {
    WsLayout<> st;
    const auto srow_p = st.add<int64_t>((size_t)stage_cap), scol_p = st.add<int64_t>((size_t)stage_cap);
    const auto sval_p = st.add<float>((size_t)stage_cap);
    char* w3 = nullptr;
    if (ws_reserve(ctx, WS_PROJECTED, st.bytes(), &w3) != PVS_OK) {
      (void)hipGetLastError();   // no room for the staging list: the exact path needs none
      filtered = false;
    } else {
      srow = srow_p(w3); scol = scol_p(w3); sval = sval_p(w3);
    }
  }
  const bool same = filtered && d_Q == d_DB && nq == N && d_inv_q == d_inv_db;
  _Float16 *q16 = nullptr, *db16 = nullptr;
  if (filtered) {
    WsLayout<> l16;
    const auto q16_p = l16.add<_Float16>((size_t)nq * L), db16_p = l16.add<_Float16>(same ? 0 : (size_t)N * L);
    char* w5 = nullptr;
    if (ws_reserve(ctx, WS_FP16_ROWS, l16.bytes(), &w5) != PVS_OK) {
      (void)hipGetLastError();
      filtered = false;
    } else {
      q16 = q16_p(w5);
      db16 = same ? q16 : db16_p(w5);
    }
  }
  const int64_t list_rows = filtered ? (stage_cap + RNG_LIST_LD - 1) / RNG_LIST_LD : 0;
  const int64_t nrows = std::max<int64_t>(j.plan.QT, list_rows);
  WsLayout<> lay;
  const auto invq16_p = lay.add<float>(filtered ? (size_t)nq : 0), invd16_p = lay.add<float>(filtered && !same ? (size_t)N : 0);
  const auto fstats_p = lay.add<unsigned long long>(4);
  const auto totals_p = lay.add<int64_t>(2);
  const auto counts_p = lay.add<int>((size_t)nrows);
  const auto offsets_p = lay.add<int64_t>((size_t)nrows);
  char* w6 = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_LISTS, lay.bytes(), &w6));
  float* invq16 = invq16_p(w6);
  float* invd16 = same ? invq16 : invd16_p(w6);
  unsigned long long* fstats = fstats_p(w6);
  j.totals = totals_p(w6);
  j.counts = counts_p(w6);
  j.offsets = offsets_p(w6);
  PVS_HIP(hipMemsetAsync(fstats, 0, 32, ctx->stream));
  PVS_HIP(hipMemsetAsync(j.totals, 0, 16, ctx->stream));

  if (filtered) {
    PVS_TRY(launch_filter_rows_to_f16(ctx, d_Q, nq, L, d_inv_q, q16, invq16, fstats));
    if (!same) PVS_TRY(launch_filter_rows_to_f16(ctx, d_DB, N, L, d_inv_db, db16, invd16, fstats));
    unsigned long long bad = 0;
    PVS_HIP(hipMemcpyAsync(&bad, fstats, 8, hipMemcpyDeviceToHost, ctx->stream));
    PVS_HIP(hipStreamSynchronize(ctx->stream));
    if (bad) filtered = false;   // non-finite values or an extreme dynamic range: the exact path
  }

  if (!filtered) {
    for (int64_t q0 = 0; q0 < nq; q0 += j.plan.QT) PVS_TRY(range_exact_block(j, q0));
  } else {
    j.stats[0] = 1;
    // the largest float32 not above t - eps: s32 >= t  =>  s16 >= s32 - eps >= t - eps >= thr16
    const double lim = (double)threshold - filter_error_bound(L);
    float thr16 = (float)lim;
    if ((double)thr16 > lim) thr16 = std::nextafterf(thr16, -INFINITY);
    for (int64_t q0 = 0; q0 < nq; q0 += j.plan.QT) {
      PVS_HIP(hipMemsetAsync(j.totals + 1, 0, 8, ctx->stream));
      PVS_TRY(panel_query_block<float>(ctx, j.plan, q0, [&](int64_t, int64_t qn, int64_t c0, int64_t cn, float* panel) -> int {
        if (tile_below_diagonal(j, q0, c0, cn)) {
          ++j.stats[4];
          return PVS_OK;
        }
        PVS_TRY(launch_cosine_f16_bounded(ctx, q16 + q0 * L, qn, db16 + c0 * L, cn, L, invq16 + q0, invd16 + c0, panel, cn));
        ++j.stats[3];
        const RangeSrc src{panel, cn, qn, cn, q0, c0, nullptr, nullptr, 0, thr16, j.upper};
        return range_compact<false>(j, src, j.totals + 1, stage_cap, srow, scol, nullptr);
      }));
      int64_t ncand = 0;
      PVS_HIP(hipMemcpyAsync(&ncand, j.totals + 1, 8, hipMemcpyDeviceToHost, ctx->stream));
      PVS_HIP(hipStreamSynchronize(ctx->stream));
      if (ncand > stage_cap) {          // more candidates than the staging holds: this row block by the exact path
        ++j.stats[1];
        PVS_TRY(range_exact_block(j, q0));
        continue;
      }
      if (ncand == 0) continue;
      {
        ScopedTimer tm(ctx, T_RESCORE);
        hipLaunchKernelGGL(range_rescore_pairs_kernel, dim3((unsigned)((ncand + RNG_PASS - 1) / RNG_PASS)), dim3(RNG_THREADS), 0, ctx->stream,
                           d_Q, d_DB, L, d_inv_q, d_inv_db, srow, scol, ncand, sval);
        PVS_HIP(hipGetLastError());
      }
      j.stats[2] += ncand;
      const RangeSrc src{sval, RNG_LIST_LD, (ncand + RNG_LIST_LD - 1) / RNG_LIST_LD, RNG_LIST_LD, 0, 0, srow, scol, ncand, threshold, 0};
      PVS_TRY(range_compact<true>(j, src, j.totals, capacity, d_row, d_col, d_val));
    }
  }
  int64_t total = 0;
  PVS_HIP(hipMemcpyAsync(&total, j.totals, 8, hipMemcpyDeviceToHost, ctx->stream));
  PVS_HIP(hipStreamSynchronize(ctx->stream));
  *h_total = total;
  if (h_stats) std::copy(j.stats, j.stats + 6, h_stats);
  if (total > capacity)
    PVS_FAIL(PVS_ERR_CAPACITY, "threshold join: %lld pairs do not fit the output of %lld", (long long)total, (long long)capacity);
  return PVS_OK;
}

PVS_EXPORT int pvs_pair_components_dev(pvs_ctx* ctx, const int64_t* d_a, const int64_t* d_b, int64_t E, int64_t N, int32_t* d_label,
                                       int64_t* h_stats) {
  PVS_NEED(ctx, "ctx");
  if (E < 0 || N < 0 || N > 0x7fffffffLL) PVS_FAIL(PVS_ERR_INVALID, "pvs_pair_components_dev: need E >= 0 and 0 <= N < 2^31");
  if (E > 0 && N == 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_pair_components_dev: edges over an empty node set");
  if (h_stats) h_stats[0] = h_stats[1] = 0;
  if (N == 0) return PVS_OK;
  PVS_NEED(d_label, "labels");
  if (E > 0) {
    PVS_NEED(d_a, "pair rows");
    PVS_NEED(d_b, "pair columns");
  }
  PVS_HIP(hipSetDevice(ctx->device));
  WsLayout<> lay;
  const auto flags_p = lay.add<int>(2);
  const auto count_p = lay.add<unsigned long long>(1);
  char* w6 = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_LISTS, lay.bytes(), &w6));
  int* d_flags = flags_p(w6);                  // [0] a node id out of range, [1] this round hooked something
  unsigned long long* d_count = count_p(w6);
  const unsigned node_grid = (unsigned)std::min<int64_t>((N + 255) / 256, (int64_t)ctx->num_cu * 8);
  const unsigned edge_grid = (unsigned)std::min<int64_t>((std::max<int64_t>(E, 1) + 255) / 256, (int64_t)ctx->num_cu * 8);
  ScopedTimer tm(ctx, T_MISC);
  if (E > 0) {
    PVS_HIP(hipMemsetAsync(d_flags, 0, 8, ctx->stream));
    hipLaunchKernelGGL(comp_check_kernel, dim3(edge_grid), dim3(256), 0, ctx->stream, d_a, d_b, E, N, d_flags);
    int bad = 0;
    PVS_HIP(hipMemcpyAsync(&bad, d_flags, 4, hipMemcpyDeviceToHost, ctx->stream));
    PVS_HIP(hipStreamSynchronize(ctx->stream));
    if (bad) PVS_FAIL(PVS_ERR_INVALID, "pvs_pair_components_dev: a node id lies outside [0, %lld)", (long long)N);
  }
  hipLaunchKernelGGL(comp_init_kernel, dim3(node_grid), dim3(256), 0, ctx->stream, d_label, N);
  int64_t rounds = 0;
  for (int changed = E > 0; changed;) {
    if (rounds > N) PVS_FAIL(PVS_ERR_UNSUPPORTED, "pvs_pair_components_dev: no fixed point after %lld rounds", (long long)rounds);
    PVS_HIP(hipMemsetAsync(d_flags + 1, 0, 4, ctx->stream));
    hipLaunchKernelGGL(comp_hook_kernel, dim3(edge_grid), dim3(256), 0, ctx->stream, d_a, d_b, E, d_label, d_flags + 1);
    hipLaunchKernelGGL(comp_compress_kernel, dim3(node_grid), dim3(256), 0, ctx->stream, d_label, N);
    PVS_HIP(hipMemcpyAsync(&changed, d_flags + 1, 4, hipMemcpyDeviceToHost, ctx->stream));
    PVS_HIP(hipStreamSynchronize(ctx->stream));
    ++rounds;
  }
  unsigned long long comps = 0;
  PVS_HIP(hipMemsetAsync(d_count, 0, 8, ctx->stream));
  hipLaunchKernelGGL(comp_count_roots_kernel, dim3(node_grid), dim3(256), 0, ctx->stream, d_label, N, d_count);
  PVS_HIP(hipMemcpyAsync(&comps, d_count, 8, hipMemcpyDeviceToHost, ctx->stream));
  PVS_HIP(hipStreamSynchronize(ctx->stream));
  if (h_stats) {
    h_stats[0] = rounds;
    h_stats[1] = (int64_t)comps;
  }
  return PVS_OK;
}
