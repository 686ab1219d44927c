// Inverted lists over the int8 code rows: the probed exact scan behind pvsim.IVFInt8Index.
//   pvs_ivf_sq8_scan_topk_dev   query codes x the code rows of the probed lists -> candidate rows (score, original id) -> list-mode
//                               top-k (topk.hip)
// All arithmetic is section 22's: acc = the int32 dot product of two code rows, score = ((float)acc * inv_q) * inv_d.  acc is an
// integer, so no slice size, wave assignment or order of summation changes a bit, and a score here is, bit for bit, the score
// pvs_sq8_topk_dev reports for the same pair.  Nothing is a multiply followed by an add: the unit needs no -ffp-contract=off.
// The storage, the candidate row and its padding are section 14's with m = ld (ivf.hip); the centroids are code rows themselves, so
// the list of a row and the probes of a query both come from pvs_sq8_topk_dev and this unit only scans.
// From list_common.hpp: the block scan over the probed lists' lengths, the check of the host offsets, W and the query block.  From
// ivf_sq8_plan.hpp: the slices.
#include "ivf_sq8_plan.hpp"
#include "list_common.hpp"

namespace pvs {
namespace {

using i32x4 = __attribute__((ext_vector_type(4))) int;

constexpr int ISQ_MAX_L = 131072;

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Workgroup (g, q) of a grid (G, queries of the block).  The candidate row of query q is the concatenation of its probed lists in
// probe order (section 14): probe j owns the slots [incl[j] - len[j], incl[j]), slot p of it is stored row start[j] + p, and the
// slots from incl[nprobe - 1] up to W are padding (-inf, -1).  The workgroup serves the slice [g S, (g + 1) S) of that row whatever
// lists it falls into.  The query's ld code bytes are copied to LDS once; then a WAVE owns a slot (a row is up to 128 KiB, not m
// bytes): wave w takes the slots p0 + w, p0 + w + 16, ..., finds the slot's probe by a binary search of incl[] in LDS (the same for
// all its lanes), walks the stored row with 16-byte loads, four in flight, and v_dot4 against the query's bytes at the same offsets
// (the inner loop of sq8_rows_kernel<1>), adds the 64 partial sums by shuffles, and lane 0 stores the slot.  Every slot of [0, W) is
// written exactly once: no atomics, no position that depends on timing.
__global__ __launch_bounds__(ISQ_THREADS) void ivf_sq8_scan_kernel(const int8_t* __restrict__ qc, const float* __restrict__ inv_q, int ld,
                                                                   const int64_t* __restrict__ probe, int nprobe,
                                                                   const int64_t* __restrict__ list_off, int nlist,
                                                                   const int8_t* __restrict__ codes, const float* __restrict__ inv_db,
                                                                   const int32_t* __restrict__ ids, int64_t W, int64_t S,
                                                                   float* __restrict__ cval, int32_t* __restrict__ cid) {
  extern __shared__ __attribute__((aligned(16))) int8_t s_qrow[];   // [ld]
  __shared__ int incl[ISQ_MAX_PROBE];      // inclusive prefix sums of the probed lists' lengths (N < 2^31)
  __shared__ int start[ISQ_MAX_PROBE];     // first stored row of each probed list
  __shared__ int stmp[ISQ_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q = blockIdx.y;
  const int64_t p0 = (int64_t)blockIdx.x * S, p1 = min(p0 + S, W);

  // ---- the probes of this query: one per thread
  {
    int len = 0;
    if (tid < nprobe) {
      const int64_t l = probe[q * nprobe + tid];
      const bool ok = l >= 0 && l < nlist;
      const int64_t a = ok ? list_off[l] : 0, b = ok ? list_off[l + 1] : 0;
      len = (int)(b - a);
      start[tid] = (int)a;
    }
    const int upto = block_incl_scan(len, stmp, lane, wave);
    if (tid < nprobe) incl[tid] = upto;
  }
  __syncthreads();
  const int64_t total = incl[nprobe - 1];
  const int64_t live_end = min(p1, total);
  // ---- padding slots of this slice
  for (int64_t p = max(p0, total) + tid; p < p1; p += ISQ_THREADS) {
    cval[q * W + p] = -INFINITY;
    cid[q * W + p] = -1;
  }
  if (p0 >= live_end) return;              // the whole workgroup leaves

  // ---- the query's code row
  const int nch = ld / 16;                 // 16-byte chunks of a row: a multiple of 4
  i32x4* s4 = reinterpret_cast<i32x4*>(s_qrow);
  {
    const i32x4* q4 = reinterpret_cast<const i32x4*>(qc + q * ld);
    for (int i = tid; i < nch; i += ISQ_THREADS) s4[i] = q4[i];
  }
  __syncthreads();
  const float iq = inv_q[q];

  auto dot16 = [&](const i32x4 d, int c, int a) {
    const i32x4 qv = s4[c];
    a = __builtin_amdgcn_sdot4(qv.x, d.x, a, false);
    a = __builtin_amdgcn_sdot4(qv.y, d.y, a, false);
    a = __builtin_amdgcn_sdot4(qv.z, d.z, a, false);
    a = __builtin_amdgcn_sdot4(qv.w, d.w, a, false);
    return a;
  };

  for (int64_t p = p0 + wave; p < live_end; p += ISQ_WAVES) {
    // j = the number of probes that end at or before p: incl[j - 1] <= p < incl[j], so probe j is not empty
    int lo = 0, hi = nprobe - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((int64_t)incl[mid] <= p) lo = mid + 1;
      else hi = mid;
    }
    const int64_t first = lo > 0 ? (int64_t)incl[lo - 1] : 0;
    const int64_t row = (int64_t)start[lo] + (p - first);
    const i32x4* d4 = reinterpret_cast<const i32x4*>(codes + row * ld);
    int acc = 0;
    int c = lane;
    for (; c + 192 < nch; c += 256) {
      const i32x4 v0 = d4[c], v1 = d4[c + 64], v2 = d4[c + 128], v3 = d4[c + 192];
      acc = dot16(v0, c, acc);
      acc = dot16(v1, c + 64, acc);
      acc = dot16(v2, c + 128, acc);
      acc = dot16(v3, c + 192, acc);
    }
    for (; c < nch; c += 64) acc = dot16(d4[c], c, acc);
    const int sum = wave_sum(acc);
    if (lane == 0) {
      cval[q * W + p] = ((float)sum * iq) * inv_db[row];
      cid[q * W + p] = ids[row];
    }
  }
}

}  // namespace
}  // namespace pvs

using namespace pvs;

// the checks both entries share: shapes, then the host offsets -> N
static int isq_check_lists(const char* fn, int nprobe, const int64_t* h_list_off, int nlist, int slice_rows, int64_t* N) {
  if (nlist < 1 || nlist > 65536) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= nlist <= 65536 (got %d)", fn, nlist);
  if (nprobe < 1 || nprobe > std::min(nlist, ISQ_MAX_PROBE))
    PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= nprobe <= min(nlist, %d) (got nprobe=%d, nlist=%d)", fn, ISQ_MAX_PROBE, nprobe, nlist);
  if (slice_rows < 0) PVS_FAIL(PVS_ERR_INVALID, "%s: negative slice_rows", fn);
  if (!h_list_off) PVS_FAIL(PVS_ERR_INVALID, "%s: null host list_off", fn);
  const int64_t bad = offsets_first_break(h_list_off, nlist);
  if (bad == 0) PVS_FAIL(PVS_ERR_INVALID, "%s: list_off[0] must be 0", fn);
  if (bad > 0) PVS_FAIL(PVS_ERR_INVALID, "%s: list_off must not decrease (list %d)", fn, (int)(bad - 1));
  *N = h_list_off[nlist];
  if (*N >= ((int64_t)1 << 31)) PVS_FAIL(PVS_ERR_INVALID, "%s: need N < 2^31 (got %lld)", fn, (long long)*N);
  return PVS_OK;
}

PVS_EXPORT int pvs_ivf_sq8_scan_plan(pvs_ctx* ctx, int64_t nq, int nprobe, const int64_t* h_list_off, int nlist, int slice_rows,
                                     int64_t* h_plan) {
  PVS_NEED(ctx, "ctx");
  PVS_NEED(h_plan, "plan");
  if (nq < 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_sq8_scan_plan: negative nq");
  int64_t N = 0;
  PVS_TRY(isq_check_lists(__func__, nprobe, h_list_off, nlist, slice_rows, &N));
  const int64_t W = ivf_candidate_width(h_list_off, nlist, nprobe);
  const int64_t QB = ivf_query_block(std::max<int64_t>(nq, 1), W);
  const IsqSlices sl = isq_slices(ctx->num_cu, QB, W, slice_rows);
  h_plan[0] = W, h_plan[1] = QB, h_plan[2] = sl.S, h_plan[3] = sl.G;
  return PVS_OK;
}

PVS_EXPORT int pvs_ivf_sq8_scan_topk_dev(pvs_ctx* ctx, const int8_t* d_qcodes, const float* d_inv_q, int64_t nq, int L,
                                         const int64_t* d_probe, int nprobe, const int64_t* d_list_off, const int64_t* h_list_off,
                                         int nlist, const int8_t* d_codes, const float* d_inv_db, const int32_t* d_ids, int k,
                                         int slice_rows, int64_t* d_idx, float* d_val) {
  PVS_NEED(ctx, "ctx");
  if (L < 1 || L > ISQ_MAX_L) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_sq8_scan_topk_dev: need 1 <= L <= %d (got %d)", ISQ_MAX_L, L);
  if (k < 1 || k > 1024) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_sq8_scan_topk_dev: need 1 <= k <= 1024 (got %d)", k);
  if (nq < 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_sq8_scan_topk_dev: negative nq");
  int64_t N = 0;
  PVS_TRY(isq_check_lists(__func__, nprobe, h_list_off, nlist, slice_rows, &N));
  if (nq == 0) return PVS_OK;
  PVS_NEED(d_qcodes, "qcodes");
  PVS_NEED(d_inv_q, "inv_q");
  PVS_NEED(d_probe, "probe");
  PVS_NEED(d_list_off, "list_off");
  if (N > 0) {
    PVS_NEED(d_codes, "codes");
    PVS_NEED(d_inv_db, "inv_db");
    PVS_NEED(d_ids, "ids");
  }
  PVS_NEED(d_idx, "idx");
  PVS_NEED(d_val, "val");
  PVS_ALIGNED(d_qcodes, 16, "qcodes");
  PVS_ALIGNED(d_codes, 16, "codes");
  PVS_ALIGNED(d_inv_q, 4, "inv_q");
  PVS_ALIGNED(d_inv_db, 4, "inv_db");
  PVS_ALIGNED(d_probe, 8, "probe");
  PVS_ALIGNED(d_list_off, 8, "list_off");
  PVS_ALIGNED(d_ids, 4, "ids");
  PVS_ALIGNED(d_idx, 8, "idx");
  PVS_ALIGNED(d_val, 4, "val");
  PVS_HIP(hipSetDevice(ctx->device));

  const int ld = PVS_SQ8_LD(L);
  const int64_t W = ivf_candidate_width(h_list_off, nlist, nprobe);
  const int64_t QB = ivf_query_block(nq, W);
  const IsqSlices sl = isq_slices(ctx->num_cu, QB, W, slice_rows);
  const IvfCandLayout lay = ivf_cand_layout((size_t)QB, (size_t)W);
  void* block = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_IVF_CANDIDATES, lay.bytes, &block));
  float* cval = lay.val(block);
  int32_t* cid = lay.id(block);

  for (int64_t q0 = 0; q0 < nq; q0 += QB) {
    const int64_t qn = std::min(QB, nq - q0);
    {
      ScopedTimer t(ctx, T_GEMM);   // the scoring slot, as the ADC scans
      PVS_TRY(launch_lds(ctx, ivf_sq8_scan_kernel, dim3((unsigned)sl.G, (unsigned)qn), dim3(ISQ_THREADS), (size_t)ld, d_qcodes + q0 * ld,
                         d_inv_q + q0, ld, d_probe + q0 * nprobe, nprobe, d_list_off, nlist, d_codes, d_inv_db, d_ids, W, sl.S, cval, cid));
    }
    PVS_TRY(launch_topk_candidates(ctx, cid, cval, qn, W, k, d_idx + q0 * k, d_val + q0 * k));
  }
  return PVS_OK;
}
