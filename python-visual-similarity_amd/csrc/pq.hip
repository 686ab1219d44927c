// Compact index: product-quantised encodings and asymmetric-distance search.
//   pvs_pq_encode_dev      rows -> uint8 codes (nearest_codeword_kernel<uint8_t> of pq_common.hpp)
//   pvs_pq_lut_dev         queries -> inner-product tables [nq][m][ksub] (dot_table_kernel of pq_common.hpp)
//   pvs_pq_scan_topk_dev   tables x codes -> score panel (table in LDS, one lane per row) -> the top-k kernels of topk.hip
//   pvs_rescore_rows_dev   exact cosine of each query with its candidate rows
// Every sum here is DEFINED (include/pvsim.h): float32, ascending index, a multiply and an add rounded separately.  The
// arithmetic goes through __fmul_rn / __fadd_rn / __fsub_rn and the Makefile compiles this unit with -ffp-contract=off (the
// intrinsics are plain inline `a * b` / `a + b` in the HIP headers: without the flag hipcc fuses them into an fma), so a
// NumPy restatement with np.float32 element operations gives the same bits (tests/pq_numpy.py).  The pieces the inverted lists
// (ivf.hip) use as well -- both kernels above, the table copy, the dword gather, the segment plan -- live in pq_common.hpp.
#include "panel_plan.hpp"
#include "pq_common.hpp"

struct pvs_pq {
  int m = 0, ksub = 0, dsub = 0;
  float* d_cb = nullptr;   // [m][ksub][dsub]
};

namespace pvs {

constexpr int PQ_SCAN_THREADS = 512;
constexpr int PQ_SCAN_QB = 4;                  // queries per workgroup: the code tile is fetched once for all of them
constexpr int PQ_SCAN_RPL = 4;                 // rows per lane at most
constexpr int PQ_SCAN_REG_DW = 16;             // code dwords a lane keeps per row in registers (m <= 64)
constexpr int PQ_SEG_ENTRIES = 40960;          // table entries per LDS segment: 160 KiB

// ------------------------------------------------------------------------------------------------- scan
// Workgroup = 512 lanes x rpl rows per lane (row = tile + r * 512 + lane: panel stores stay coalesced) x up to PQ_SCAN_QB
// queries.  Per query the table (or one segment of seg_m sub-spaces of it) is copied to LDS and every lane gathers
// tab[s][code[s]] for s ascending with ds_read_b32 on data-dependent addresses; the running sum of a row is one register and
// lives across the segments, so segmenting does not change the order of the additions.
// REG: m % 4 == 0, m <= 64, 4-byte aligned code rows: the lane keeps its rows' codes in registers across the query block (the
// table then fits one segment).  Otherwise the codes are read again per query (L1 / L2 hits: a tile is at most 2048 x m bytes),
// 4 bytes at a time when the launcher's ScanPlan allows (width >= 4), row by row.
template <bool REG, int RPL>
__global__ __launch_bounds__(PQ_SCAN_THREADS) void pq_scan_kernel(const float* __restrict__ lut, int nq, int m, int ksub, int seg_m,
                                                                  int width, const uint8_t* __restrict__ codes, int64_t N,
                                                                  const float* __restrict__ inv_q, const float* __restrict__ inv_db,
                                                                  float* __restrict__ panel, int64_t ld) {
  constexpr int rpl = RPL;
  extern __shared__ __attribute__((aligned(16))) float tab[];
  const int tid = threadIdx.x;
  const int64_t tile0 = (int64_t)blockIdx.x * PQ_SCAN_THREADS * rpl;
  const int q0 = blockIdx.y * PQ_SCAN_QB;
  const int qn = min(PQ_SCAN_QB, nq - q0);
  const int64_t tsize = (int64_t)m * ksub;

  uint32_t creg[REG ? RPL : 1][REG ? PQ_SCAN_REG_DW : 1];
  float idb[RPL];
  bool live[RPL];
  const uint8_t* crow[RPL];
#pragma unroll
  for (int r = 0; r < RPL; ++r) {
    const int64_t row = tile0 + (int64_t)r * PQ_SCAN_THREADS + tid;
    live[r] = row < N;
    crow[r] = codes + (live[r] ? row : 0) * m;
    idb[r] = (live[r] && inv_db) ? inv_db[row] : 1.f;
    if (REG) {
      const uint32_t* cr = reinterpret_cast<const uint32_t*>(crow[r]);
#pragma unroll
      for (int w = 0; w < PQ_SCAN_REG_DW; ++w) creg[r][w] = (live[r] && w * 4 < m) ? cr[w] : 0u;
    }
  }

  for (int qi = 0; qi < qn; ++qi) {
    const int64_t q = q0 + qi;
    const float* lq = lut + q * tsize;
    float sum[RPL];
#pragma unroll
    for (int r = 0; r < RPL; ++r) sum[r] = 0.f;
    for (int s0 = 0; s0 < m; s0 += seg_m) {
      const int sn = min(seg_m, m - s0);
      __syncthreads();   // the readers of the previous table are done
      copy_table_segment<PQ_SCAN_THREADS>(tab, lq + (int64_t)s0 * ksub, sn * ksub, tid);
      __syncthreads();
      if (REG) {
#pragma unroll
        for (int w = 0; w < PQ_SCAN_REG_DW; ++w) {
          if (w * 4 < m) {
            const float* t0 = tab + (w * 4) * ksub;
            // the byte offsets of a row's codes do not depend on the query, so the compiler would keep all 64 of them per row
            // across the query loop (256 registers and spills at four rows per lane): the empty asm makes it extract them here,
            // and the scheduling barrier keeps the gathers of one code dword together
            uint32_t u[RPL];
#pragma unroll
            for (int r = 0; r < RPL; ++r) {
              u[r] = creg[r][w];
              asm volatile("" : "+v"(u[r]));
            }
            gather_dword<RPL>(sum, u, t0, ksub);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      } else {
        // one row at a time, 4 bytes at most: the interleaved walk_segment is 3 times faster here with 16-byte loads (m = 128)
        // but 1.7 to 1.9 times slower with 4-byte loads (m = 68, 72; measured), so this path stays as it was
#pragma unroll
        for (int r = 0; r < RPL; ++r) {
          if (live[r]) {
            const uint8_t* cr = crow[r] + s0;
            float a = sum[r];
            int s = 0;
            if (width >= 4) {
              for (; s + 4 <= sn; s += 4) {
                const uint32_t u = *reinterpret_cast<const uint32_t*>(cr + s);
                a = __fadd_rn(a, tab[(s + 0) * ksub + (u & 255u)]);
                a = __fadd_rn(a, tab[(s + 1) * ksub + ((u >> 8) & 255u)]);
                a = __fadd_rn(a, tab[(s + 2) * ksub + ((u >> 16) & 255u)]);
                a = __fadd_rn(a, tab[(s + 3) * ksub + (u >> 24)]);
              }
            }
            for (; s < sn; ++s) a = __fadd_rn(a, tab[s * ksub + cr[s]]);
            sum[r] = a;
          }
        }
      }
    }
    const float iq = inv_q ? inv_q[q] : 1.f;
#pragma unroll
    for (int r = 0; r < RPL; ++r) {
      if (live[r]) panel[q * ld + tile0 + (int64_t)r * PQ_SCAN_THREADS + tid] = __fmul_rn(__fmul_rn(sum[r], iq), idb[r]);
    }
  }
}

// ------------------------------------------------------------------------------------------------- exact re-scoring
// One lane per (query, candidate): dot product in ascending t, then the two factors.  Slots with a negative index give -inf.
__global__ __launch_bounds__(256) void pq_rescore_kernel(const float* __restrict__ Q, int64_t nq, const float* __restrict__ X, int64_t N,
                                                         int64_t d, const float* __restrict__ inv_q, const float* __restrict__ inv_db,
                                                         const int64_t* __restrict__ cand, int64_t R, float* __restrict__ val) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nq * R) return;
  const int64_t q = e / R;
  const int64_t i = cand[e];
  if (i < 0 || i >= N) {
    val[e] = -INFINITY;
    return;
  }
  const float* a = Q + q * d;
  const float* b = X + i * d;
  float acc = 0.f;
  for (int64_t t = 0; t < d; ++t) acc = __fadd_rn(acc, __fmul_rn(a[t], b[t]));
  val[e] = __fmul_rn(__fmul_rn(acc, inv_q ? inv_q[q] : 1.f), inv_db ? inv_db[i] : 1.f);
}

}  // namespace pvs

using namespace pvs;

static int pq_check_shape(const char* fn, int m, int ksub, int dsub) {
  if (m < 1 || dsub < 1 || ksub < 1 || ksub > 256)
    PVS_FAIL(PVS_ERR_INVALID, "%s: need m >= 1, dsub >= 1 and 1 <= ksub <= 256 (got m=%d, ksub=%d, dsub=%d)", fn, m, ksub, dsub);
  if ((int64_t)m * dsub > (int64_t)1 << 24) PVS_FAIL(PVS_ERR_INVALID, "%s: m * dsub = %lld is too large", fn, (long long)m * dsub);
  return PVS_OK;
}

PVS_EXPORT int pvs_pq_create(pvs_ctx* ctx, const float* codebooks, int m, int ksub, int dsub, pvs_pq** out) {
  PVS_NEED(ctx, "ctx");
  PVS_NEED(codebooks, "codebooks");
  PVS_NEED(out, "out");
  PVS_TRY(pq_check_shape(__func__, m, ksub, dsub));
  if (dsub > NEAREST_LDS_FLOATS) PVS_FAIL(PVS_ERR_UNSUPPORTED, "pvs_pq_create: dsub = %d exceeds %d", dsub, NEAREST_LDS_FLOATS);
  PVS_HIP(hipSetDevice(ctx->device));
  const size_t bytes = (size_t)m * ksub * dsub * sizeof(float);
  float* d_cb = nullptr;
  PVS_HIP(hipMalloc(&d_cb, bytes));
  hipError_t e = hipMemcpyAsync(d_cb, codebooks, bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // the host array may go away after the call
  if (e != hipSuccess) {
    (void)hipFree(d_cb);
    PVS_FAIL(PVS_ERR_NO_DEVICE, "pvs_pq_create: upload failed: %s", hipGetErrorString(e));
  }
  pvs_pq* pq = new pvs_pq;
  pq->m = m;
  pq->ksub = ksub;
  pq->dsub = dsub;
  pq->d_cb = d_cb;
  *out = pq;
  return PVS_OK;
}

PVS_EXPORT int pvs_pq_destroy(pvs_ctx* ctx, pvs_pq* pq) {
  if (!pq) return PVS_OK;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);   // launches that read the table may still be queued
  }
  if (pq->d_cb) (void)hipFree(pq->d_cb);
  delete pq;
  return PVS_OK;
}

PVS_EXPORT int pvs_pq_encode_dev(pvs_ctx* ctx, const pvs_pq* pq, const float* d_x, int64_t n, uint8_t* d_codes) {
  PVS_NEED(ctx, "ctx");
  PVS_NEED(pq, "pq");
  if (n < 0 || n > ((int64_t)1 << 38)) PVS_FAIL(PVS_ERR_INVALID, "pvs_pq_encode_dev: bad n = %lld", (long long)n);
  if (n == 0) return PVS_OK;
  PVS_NEED(d_x, "x");
  PVS_NEED(d_codes, "codes");
  PVS_ALIGNED(d_x, 4, "x");
  if (pq->m > 65535) PVS_FAIL(PVS_ERR_UNSUPPORTED, "pvs_pq_encode_dev: m = %d exceeds 65535", pq->m);
  PVS_HIP(hipSetDevice(ctx->device));
  return launch_nearest_codeword<uint8_t>(ctx, d_x, n, pq->d_cb, pq->m, pq->ksub, pq->dsub, d_codes, nullptr);
}

PVS_EXPORT int pvs_pq_lut_dev(pvs_ctx* ctx, const pvs_pq* pq, const float* d_q, int64_t nq, float* d_lut) {
  PVS_NEED(ctx, "ctx");
  PVS_NEED(pq, "pq");
  if (nq < 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_pq_lut_dev: negative nq");
  if (nq == 0) return PVS_OK;
  PVS_NEED(d_q, "q");
  PVS_NEED(d_lut, "lut");
  PVS_ALIGNED(d_q, 4, "q");
  PVS_ALIGNED(d_lut, 4, "lut");
  PVS_HIP(hipSetDevice(ctx->device));
  return launch_dot_table(ctx, d_q, nq, pq->d_cb, pq->m, pq->ksub, pq->dsub, d_lut);
}

namespace pvs {
// one panel: scores of qn queries against cn rows into panel[qn][cn]
static int launch_pq_scan(pvs_ctx* ctx, const float* lut, int64_t qn, int m, int ksub, const uint8_t* codes, int64_t cn,
                          const float* inv_q, const float* inv_db, float* panel) {
  const ScanPlan plan = scan_plan(m, ksub, PQ_SEG_ENTRIES, codes);
  const bool reg = plan.width >= 4 && m <= 4 * PQ_SCAN_REG_DW;
  const int64_t qblocks = (qn + PQ_SCAN_QB - 1) / PQ_SCAN_QB;
  // four rows per lane quarter the table copies per row; one row per lane when that would leave compute units idle
  const int64_t big_tiles = (cn + (int64_t)PQ_SCAN_THREADS * PQ_SCAN_RPL - 1) / ((int64_t)PQ_SCAN_THREADS * PQ_SCAN_RPL);
  const int rpl = big_tiles * qblocks >= 2 * (int64_t)ctx->num_cu ? PQ_SCAN_RPL : 1;
  const int64_t tiles = (cn + (int64_t)PQ_SCAN_THREADS * rpl - 1) / ((int64_t)PQ_SCAN_THREADS * rpl);
  using scan_fn = void (*)(const float*, int, int, int, int, int, const uint8_t*, int64_t, const float*, const float*, float*, int64_t);
  const scan_fn kern = reg ? (rpl == 1 ? pq_scan_kernel<true, 1> : pq_scan_kernel<true, PQ_SCAN_RPL>)
                           : (rpl == 1 ? pq_scan_kernel<false, 1> : pq_scan_kernel<false, PQ_SCAN_RPL>);
  if (plan.lds > 48 * 1024) PVS_TRY(ensure_lds(ctx, reinterpret_cast<const void*>(kern), plan.lds));
  const dim3 grid((unsigned)tiles, (unsigned)qblocks);
  hipLaunchKernelGGL(kern, grid, dim3(PQ_SCAN_THREADS), plan.lds, ctx->stream, lut, (int)qn, m, ksub, plan.seg_m, plan.width, codes, cn, inv_q,
                     inv_db, panel, cn);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}
}  // namespace pvs

PVS_EXPORT int pvs_pq_scan_topk_dev(pvs_ctx* ctx, const float* d_lut, int64_t nq, int m, int ksub, const uint8_t* d_codes, int64_t N,
                                    const float* d_inv_q, const float* d_inv_db, int k, int64_t col_offset, int merge, int64_t* d_idx,
                                    float* d_val) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(pq_check_shape(__func__, m, ksub, 1));
  if (!scan_shape_ok(m, ksub)) PVS_FAIL(PVS_ERR_INVALID, "%s: (m, ksub) = (%d, %d) is out of range", __func__, m, ksub);
  if (nq < 0 || N < 0 || col_offset < 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_pq_scan_topk_dev: negative nq, N or col_offset");
  if (nq == 0) return PVS_OK;
  if (k < 1 || k > N) PVS_FAIL(PVS_ERR_INVALID, "pvs_pq_scan_topk_dev: need 1 <= k <= N (k = %d, N = %lld)", k, (long long)N);
  PVS_NEED(d_lut, "lut");
  PVS_NEED(d_codes, "codes");
  PVS_NEED(d_idx, "idx");
  PVS_NEED(d_val, "val");
  PVS_ALIGNED(d_lut, 4, "lut");
  PVS_ALIGNED(d_idx, 8, "idx");
  PVS_ALIGNED(d_val, 4, "val");
  if (d_inv_q) PVS_ALIGNED(d_inv_q, 4, "inv_q");
  if (d_inv_db) PVS_ALIGNED(d_inv_db, 4, "inv_db");
  PanelPlan plan;   // panel_plan.hpp: the scan rule, complete rows for k > 1024
  PVS_TRY(panel_ranking_plan(panel_scan, nq, N, k, merge, &plan));
  PVS_HIP(hipSetDevice(ctx->device));
  const int64_t tsize = (int64_t)m * ksub;
  return panel_topk(ctx, plan, k, col_offset, merge, d_idx, d_val, [&](int64_t q0, int64_t qn, int64_t c0, int64_t cn, float* panel) -> int {
    ScopedTimer t(ctx, T_GEMM);   // the scoring slot: the scan stands where the similarity GEMM stands in the dense path
    return launch_pq_scan(ctx, d_lut + q0 * tsize, qn, m, ksub, d_codes + c0 * m, cn, d_inv_q ? d_inv_q + q0 : nullptr,
                          d_inv_db ? d_inv_db + c0 : nullptr, panel);
  });
}

PVS_EXPORT int pvs_rescore_rows_dev(pvs_ctx* ctx, const float* d_Q, int64_t nq, const float* d_X, int64_t N, int64_t d,
                                    const float* d_inv_q, const float* d_inv_db, const int64_t* d_cand, int64_t R, float* d_val) {
  PVS_NEED(ctx, "ctx");
  if (nq < 0 || N < 0 || R < 0 || d < 1) PVS_FAIL(PVS_ERR_INVALID, "pvs_rescore_rows_dev: negative size or d < 1");
  if (nq == 0 || R == 0) return PVS_OK;
  if (nq * R > ((int64_t)1 << 38)) PVS_FAIL(PVS_ERR_INVALID, "pvs_rescore_rows_dev: nq * R is too large");
  PVS_NEED(d_Q, "Q");
  if (N > 0) PVS_NEED(d_X, "X");
  PVS_NEED(d_cand, "cand");
  PVS_NEED(d_val, "val");
  PVS_ALIGNED(d_Q, 4, "Q");
  PVS_ALIGNED(d_X, 4, "X");
  PVS_ALIGNED(d_cand, 8, "cand");
  PVS_ALIGNED(d_val, 4, "val");
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer t(ctx, T_RESCORE);
  hipLaunchKernelGGL(pq_rescore_kernel, dim3((unsigned)((nq * R + 255) / 256)), dim3(256), 0, ctx->stream, d_Q, nq, d_X, N, d, d_inv_q,
                     d_inv_db, d_cand, R, d_val);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}
