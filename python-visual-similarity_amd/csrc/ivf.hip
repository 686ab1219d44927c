// Inverted lists for the compact index: IVFADC of Jegou, Douze, Schmid (PAMI 2011) for an inner-product score.
//   pvs_ivf_assign_dev      rows -> nearest coarse centroid (int32) and the residual rows: nearest_codeword_kernel<int32_t> of
//                           pq_common.hpp on one sub-space of nlist codewords
//   pvs_ivf_coarse_dev      queries -> coarse terms q . c_l  [nq][nlist]: dot_table_kernel of pq_common.hpp on that sub-space (the
//                           probe list is pvs_topk_dev on the panel)
//   pvs_ivf_scan_topk_dev   tables x the codes of the probed lists -> candidate rows (score, original id) -> list-mode top-k (topk.hip)
// q . x ~ q . c_l + q . r: the table of a query does not depend on the list, so one table serves all its probes and a list adds one
// scalar, the coarse term, as the start of the sum.  Every sum is DEFINED (include/pvsim.h): float32, ascending index, a multiply and
// an add rounded separately; this unit is compiled with -ffp-contract=off like pq.hip, and tests/ivf_numpy.py restates it.  The
// scan shares its table copy, dword gather and segment plan with the flat scan of pq.hip (pq_common.hpp).
// From list_common.hpp: the block scan over the probed lists' lengths, the check of the host offsets.
#include <functional>

#include "list_common.hpp"
#include "pq_common.hpp"

namespace pvs {

constexpr int IVF_THREADS = 512;
constexpr int IVF_RPL = 4;                     // candidate slots per lane and tile
constexpr int IVF_TILE = IVF_THREADS * IVF_RPL;
constexpr int IVF_MAX_PROBE = 1024;
constexpr int IVF_SEG_ENTRIES = 36864;         // table entries per LDS segment: 144 KiB (the probe tables below take 12 KiB more)
constexpr int64_t IVF_MIN_SLICE = 1024;        // candidate slots a workgroup serves at least: a table copy is m * ksub * 4 bytes

// ------------------------------------------------------------------------------------------------- probed scan
// Workgroup (g, q) of a grid (G, queries of the block).  The candidate row of query q is the concatenation of its probed lists in
// probe order: probe j owns the slots [incl[j] - len[j], incl[j]), and slot p of it is stored row start[j] + p; the slots from
// incl[nprobe - 1] up to W are padding (id -1).  The workgroup serves the slice [g S, (g + 1) S) of that row, S a multiple of the
// tile, whatever lists it falls into: the host sizes G from the list lengths alone, and a query with one long probed list spreads
// over as many workgroups as a query with many short ones.  The table (or one segment of seg_m sub-spaces of it) is copied to LDS
// once per workgroup when it is one segment, once per tile and segment otherwise; a lane owns up to IVF_RPL slots of a tile, finds
// each slot's probe by a binary search of incl[] in LDS, reads the slot's codes `width` bytes at a time (the host's ScanPlan) and gathers
// tab[s][code[s]] for s ascending (walk_segment).  The running sum of a slot starts at its probe's coarse term and lives in a register across the segments.
// Every slot of [0, W) is written exactly once, by the lane that owns it: no atomics, no order-dependent writes.
__global__ __launch_bounds__(IVF_THREADS) void ivf_scan_kernel(const float* __restrict__ lut, int m, int ksub, int seg_m, int width,
                                                               const int64_t* __restrict__ probe, const float* __restrict__ pval,
                                                               int nprobe, const int64_t* __restrict__ list_off, int nlist,
                                                               const uint8_t* __restrict__ codes, const int32_t* __restrict__ ids,
                                                               const float* __restrict__ inv_q, const float* __restrict__ inv_db,
                                                               int64_t W, int64_t S, float* __restrict__ cval,
                                                               int32_t* __restrict__ cid) {
  extern __shared__ __attribute__((aligned(16))) float tab[];
  __shared__ int incl[IVF_MAX_PROBE];      // inclusive prefix sums of the probed lists' lengths (N < 2^31)
  __shared__ int start[IVF_MAX_PROBE];     // first stored row of each probed list
  __shared__ float cterm[IVF_MAX_PROBE];   // coarse term of each probe
  __shared__ int stmp[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q = blockIdx.y;
  const int64_t p0 = (int64_t)blockIdx.x * S, p1 = min(p0 + S, W);

  // ---- the probes of this query: two per lane
  {
    int len[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int j = 2 * tid + e;
      len[e] = 0;
      if (j < nprobe) {
        const int64_t l = probe[q * nprobe + j];
        const bool ok = l >= 0 && l < nlist;
        const int64_t a = ok ? list_off[l] : 0, b = ok ? list_off[l + 1] : 0;
        len[e] = (int)(b - a);
        start[j] = (int)a;
        cterm[j] = pval[q * nprobe + j];
      }
    }
    const int both = block_incl_scan(len[0] + len[1], stmp, lane, wave);
    if (2 * tid < nprobe) incl[2 * tid] = both - len[1];
    if (2 * tid + 1 < nprobe) incl[2 * tid + 1] = both;
  }
  __syncthreads();
  const int64_t total = incl[nprobe - 1];
  const int64_t live_end = min(p1, total);
  // ---- padding slots of this slice
  for (int64_t p = max(p0, total) + tid; p < p1; p += IVF_THREADS) {
    cval[q * W + p] = -INFINITY;
    cid[q * W + p] = -1;
  }
  if (p0 >= live_end) return;              // the whole workgroup leaves

  const int64_t tsize = (int64_t)m * ksub;
  const float* lq = lut + q * tsize;
  const bool one_seg = seg_m >= m;
  const float iq = inv_q ? inv_q[q] : 1.f;
  if (one_seg) {
    copy_table_segment<IVF_THREADS>(tab, lq, m * ksub, tid);
    __syncthreads();
  }

  for (int64_t t0 = p0; t0 < live_end; t0 += IVF_TILE) {
    int64_t row[IVF_RPL];
    float sum[IVF_RPL];
    bool live[IVF_RPL];
#pragma unroll
    for (int r = 0; r < IVF_RPL; ++r) {
      const int64_t p = t0 + (int64_t)r * IVF_THREADS + tid;
      live[r] = p < live_end;
      row[r] = 0;
      sum[r] = 0.f;
      if (live[r]) {
        // j = the number of probes that end at or before p: incl[j - 1] <= p < incl[j], so probe j is not empty
        int lo = 0, hi = nprobe - 1;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if ((int64_t)incl[mid] <= p) lo = mid + 1;
          else hi = mid;
        }
        const int64_t first = lo > 0 ? (int64_t)incl[lo - 1] : 0;
        row[r] = (int64_t)start[lo] + (p - first);
        sum[r] = cterm[lo];
      }
    }
    for (int s0 = 0; s0 < m; s0 += seg_m) {
      const int sn = min(seg_m, m - s0);
      if (!one_seg) {
        __syncthreads();   // the readers of the previous segment are done
        copy_table_segment<IVF_THREADS>(tab, lq + (int64_t)s0 * ksub, sn * ksub, tid);
        __syncthreads();
      }
      const uint8_t* cr[IVF_RPL];
#pragma unroll
      for (int r = 0; r < IVF_RPL; ++r) cr[r] = codes + row[r] * m + s0;
      walk_segment<IVF_RPL>(sum, cr, live, tab, ksub, sn, width);
    }
#pragma unroll
    for (int r = 0; r < IVF_RPL; ++r) {
      if (live[r]) {
        const int64_t p = t0 + (int64_t)r * IVF_THREADS + tid;
        cval[q * W + p] = __fmul_rn(__fmul_rn(sum[r], iq), inv_db ? inv_db[row[r]] : 1.f);
        cid[q * W + p] = ids[row[r]];
      }
    }
  }
}

}  // namespace pvs

using namespace pvs;

static int ivf_check_coarse(const char* fn, int d, int nlist) {
  if (d < 1 || d > (1 << 24)) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= d <= 2^24 (got %d)", fn, d);
  if (nlist < 1 || nlist > 65536) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= nlist <= 65536 (got %d)", fn, nlist);
  return PVS_OK;
}

PVS_EXPORT int pvs_ivf_assign_dev(pvs_ctx* ctx, const float* d_x, int64_t n, int d, const float* d_centroids, int nlist,
                                  int32_t* d_list, float* d_residual) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(ivf_check_coarse(__func__, d, nlist));
  if (n < 0 || n >= ((int64_t)1 << 31)) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_assign_dev: need 0 <= n < 2^31 (got %lld)", (long long)n);
  if (n == 0) return PVS_OK;
  PVS_NEED(d_x, "x");
  PVS_NEED(d_centroids, "centroids");
  PVS_NEED(d_list, "list");
  PVS_ALIGNED(d_x, 4, "x");
  PVS_ALIGNED(d_centroids, 4, "centroids");
  PVS_ALIGNED(d_list, 4, "list");
  if (d_residual) PVS_ALIGNED(d_residual, 4, "residual");
  if (d > NEAREST_LDS_FLOATS) PVS_FAIL(PVS_ERR_UNSUPPORTED, "pvs_ivf_assign_dev: d = %d exceeds %d", d, NEAREST_LDS_FLOATS);
  PVS_HIP(hipSetDevice(ctx->device));
  return launch_nearest_codeword<int32_t>(ctx, d_x, n, d_centroids, 1, nlist, d, d_list, d_residual);   // one sub-space of nlist codewords
}

PVS_EXPORT int pvs_ivf_coarse_dev(pvs_ctx* ctx, const float* d_q, int64_t nq, int d, const float* d_centroids, int nlist,
                                  float* d_coarse) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(ivf_check_coarse(__func__, d, nlist));
  if (nq < 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_coarse_dev: negative nq");
  if (nq == 0) return PVS_OK;
  PVS_NEED(d_q, "q");
  PVS_NEED(d_centroids, "centroids");
  PVS_NEED(d_coarse, "coarse");
  PVS_ALIGNED(d_q, 4, "q");
  PVS_ALIGNED(d_centroids, 4, "centroids");
  PVS_ALIGNED(d_coarse, 4, "coarse");
  PVS_HIP(hipSetDevice(ctx->device));
  return launch_dot_table(ctx, d_q, nq, d_centroids, 1, nlist, d, d_coarse);   // the table of one sub-space of nlist codewords
}

PVS_EXPORT int pvs_ivf_scan_topk_dev(pvs_ctx* ctx, const float* d_lut, int64_t nq, int m, int ksub, const int64_t* d_probe,
                                     const float* d_probe_val, int nprobe, const int64_t* d_list_off, const int64_t* h_list_off,
                                     int nlist, const uint8_t* d_codes, const int32_t* d_ids, const float* d_inv_q,
                                     const float* d_inv_db, int k, int64_t* d_idx, float* d_val) {
  PVS_NEED(ctx, "ctx");
  if (!scan_shape_ok(m, ksub))
    PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_scan_topk_dev: need 1 <= m <= 2^24 and 1 <= ksub <= 256 (got m=%d, ksub=%d)", m, ksub);
  if (nlist < 1 || nlist > 65536) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_scan_topk_dev: need 1 <= nlist <= 65536 (got %d)", nlist);
  if (nprobe < 1 || nprobe > std::min(nlist, IVF_MAX_PROBE))
    PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_scan_topk_dev: need 1 <= nprobe <= min(nlist, %d) (got nprobe=%d, nlist=%d)", IVF_MAX_PROBE, nprobe,
             nlist);
  if (k < 1 || k > 1024) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_scan_topk_dev: need 1 <= k <= 1024 (got %d)", k);
  if (nq < 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_scan_topk_dev: negative nq");
  PVS_NEED(h_list_off, "host list_off");
  const int64_t bad = offsets_first_break(h_list_off, nlist);
  if (bad == 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_scan_topk_dev: list_off[0] must be 0");
  if (bad > 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_scan_topk_dev: list_off must not decrease (list %d)", (int)(bad - 1));
  const int64_t N = h_list_off[nlist];
  if (N >= ((int64_t)1 << 31)) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_scan_topk_dev: need N < 2^31 (got %lld)", (long long)N);
  if (nq == 0) return PVS_OK;
  PVS_NEED(d_lut, "lut");
  PVS_NEED(d_probe, "probe");
  PVS_NEED(d_probe_val, "probe values");
  PVS_NEED(d_list_off, "list_off");
  if (N > 0) {
    PVS_NEED(d_codes, "codes");
    PVS_NEED(d_ids, "ids");
  }
  PVS_NEED(d_idx, "idx");
  PVS_NEED(d_val, "val");
  PVS_ALIGNED(d_lut, 4, "lut");
  PVS_ALIGNED(d_probe, 8, "probe");
  PVS_ALIGNED(d_probe_val, 4, "probe values");
  PVS_ALIGNED(d_list_off, 8, "list_off");
  PVS_ALIGNED(d_ids, 4, "ids");
  PVS_ALIGNED(d_idx, 8, "idx");
  PVS_ALIGNED(d_val, 4, "val");
  if (d_inv_q) PVS_ALIGNED(d_inv_q, 4, "inv_q");
  if (d_inv_db) PVS_ALIGNED(d_inv_db, 4, "inv_db");
  PVS_HIP(hipSetDevice(ctx->device));

  const int64_t W = ivf_candidate_width(h_list_off, nlist, nprobe);   // list_common.hpp, shared with ivf_sq8.hip
  // G workgroups per query: enough for two per compute unit over the query block, each with at least IVF_MIN_SLICE slots
  const int64_t QB = ivf_query_block(nq, W);
  const int64_t want = (2 * (int64_t)ctx->num_cu + QB - 1) / QB;
  const int64_t G0 = std::max<int64_t>(1, std::min<int64_t>(want, W / IVF_MIN_SLICE));
  const int64_t S = ((W + G0 - 1) / G0 + IVF_TILE - 1) / IVF_TILE * IVF_TILE;
  const int64_t G = (W + S - 1) / S;
  const IvfCandLayout lay = ivf_cand_layout((size_t)QB, (size_t)W);
  void* block = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_IVF_CANDIDATES, lay.bytes, &block));
  float* cval = lay.val(block);
  int32_t* cid = lay.id(block);

  const ScanPlan plan = scan_plan(m, ksub, IVF_SEG_ENTRIES, d_codes);
  const int64_t tsize = (int64_t)m * ksub;
  for (int64_t q0 = 0; q0 < nq; q0 += QB) {
    const int64_t qn = std::min(QB, nq - q0);
    {
      ScopedTimer t(ctx, T_GEMM);   // the scoring slot, as the flat scan
      PVS_TRY(launch_lds(ctx, ivf_scan_kernel, dim3((unsigned)G, (unsigned)qn), dim3(IVF_THREADS), plan.lds, d_lut + q0 * tsize, m, ksub,
                         plan.seg_m, plan.width, d_probe + q0 * nprobe, d_probe_val + q0 * nprobe, nprobe, d_list_off, nlist, d_codes, d_ids,
                         d_inv_q ? d_inv_q + q0 : nullptr, d_inv_db, W, S, cval, cid));
    }
    PVS_TRY(launch_topk_candidates(ctx, cid, cval, qn, W, k, d_idx + q0 * k, d_val + q0 * k));
  }
  return PVS_OK;
}
