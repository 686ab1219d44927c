// Compact index: product-quantised encodings and asymmetric-distance search.
//   pvs_pq_encode_dev      rows -> uint8 codes (nearest codeword per sub-space, vector ALU, codewords in LDS)
//   pvs_pq_lut_dev         queries -> inner-product tables [nq][m][ksub]
//   pvs_pq_scan_topk_dev   tables x codes -> score panel (table in LDS, one lane per row) -> the top-k kernels of topk.hip
//   pvs_rescore_rows_dev   exact cosine of each query with its candidate rows
// Every sum here is DEFINED (include/pvsim.h): float32, ascending index, a multiply and an add rounded separately.  The
// arithmetic goes through __fmul_rn / __fadd_rn / __fsub_rn and the Makefile compiles this unit with -ffp-contract=off (the
// intrinsics are plain inline `a * b` / `a + b` in the HIP headers: without the flag hipcc fuses them into an fma), so a
// NumPy restatement with np.float32 element operations gives the same bits (tests/pq_numpy.py).
#include <algorithm>

#include "common.hpp"

struct pvs_pq {
  int m = 0, ksub = 0, dsub = 0;
  float* d_cb = nullptr;   // [m][ksub][dsub]
};

namespace pvs {

constexpr int PQ_ENC_THREADS = 256;
constexpr int PQ_ENC_LDS_FLOATS = 16384;       // codeword chunk of the encode kernel: 64 KiB
constexpr int PQ_SCAN_THREADS = 512;
constexpr int PQ_SCAN_QB = 4;                  // queries per workgroup: the code tile is fetched once for all of them
constexpr int PQ_SCAN_RPL = 4;                 // rows per lane at most
constexpr int PQ_SCAN_REG_DW = 16;             // code dwords a lane keeps per row in registers (m <= 64)
constexpr int PQ_SEG_ENTRIES = 40960;          // table entries per LDS segment: 160 KiB
constexpr int64_t PQ_PANEL_ELEMS = (int64_t)1 << 22;   // score panel: 16 MiB, stays in the last-level cache between scan and select
constexpr int64_t PQ_PANEL_MIN_COLS = 4096;
constexpr int64_t PQ_PANEL_QUERIES = 1024;

// ------------------------------------------------------------------------------------------------- encode
// One lane owns one row of one sub-space; the codewords of the sub-space pass through LDS in chunks of jc (all lanes read the
// same codeword element: an LDS broadcast).  acc_j = sum_t (x_t - c_jt)^2 in ascending t; strict < keeps the lowest j on ties.
__global__ __launch_bounds__(PQ_ENC_THREADS) void pq_encode_kernel(const float* __restrict__ x, int64_t n, int d,
                                                                   const float* __restrict__ cb, int m, int ksub, int dsub, int jc,
                                                                   uint8_t* __restrict__ codes) {
  extern __shared__ __attribute__((aligned(16))) float cw[];
  const int s = blockIdx.y;
  const int64_t row = (int64_t)blockIdx.x * PQ_ENC_THREADS + threadIdx.x;
  const bool live = row < n;
  const float* xr = x + (live ? row : 0) * (int64_t)d + (int64_t)s * dsub;
  const float* cs = cb + (int64_t)s * ksub * dsub;
  float best = 0.f;
  int bj = 0;
  for (int j0 = 0; j0 < ksub; j0 += jc) {
    const int jn = min(jc, ksub - j0);
    __syncthreads();
    for (int e = threadIdx.x; e < jn * dsub; e += PQ_ENC_THREADS) cw[e] = cs[(int64_t)j0 * dsub + e];
    __syncthreads();
    if (live) {
      for (int j = 0; j < jn; ++j) {
        const float* c = cw + j * dsub;
        float acc = 0.f;
        for (int t = 0; t < dsub; ++t) {
          const float df = __fsub_rn(xr[t], c[t]);
          acc = __fadd_rn(acc, __fmul_rn(df, df));
        }
        if (j0 + j == 0 || acc < best) {
          best = acc;
          bj = j0 + j;
        }
      }
    }
  }
  if (live) codes[row * m + s] = (uint8_t)bj;
}

// ------------------------------------------------------------------------------------------------- table
// lut[q][s][j] = sum_t q[s dsub + t] c[s][j][t], ascending t.  One thread per entry of one (sub-space, query).
__global__ __launch_bounds__(256) void pq_lut_kernel(const float* __restrict__ qv, int d, const float* __restrict__ cb, int m, int ksub,
                                                     int dsub, float* __restrict__ lut) {
  const int s = blockIdx.x;
  const int64_t q = blockIdx.y;
  const float* qs = qv + q * d + (int64_t)s * dsub;
  for (int j = threadIdx.x; j < ksub; j += 256) {
    const float* c = cb + ((int64_t)s * ksub + j) * dsub;
    float acc = 0.f;
    for (int t = 0; t < dsub; ++t) acc = __fadd_rn(acc, __fmul_rn(qs[t], c[t]));
    lut[(q * m + s) * ksub + j] = acc;
  }
}

// ------------------------------------------------------------------------------------------------- scan
// Workgroup = 512 lanes x rpl rows per lane (row = tile + r * 512 + lane: panel stores stay coalesced) x up to PQ_SCAN_QB
// queries.  Per query the table (or one segment of seg_m sub-spaces of it) is copied to LDS and every lane gathers
// tab[s][code[s]] for s ascending with ds_read_b32 on data-dependent addresses; the running sum of a row is one register and
// lives across the segments, so segmenting does not change the order of the additions.
// REG: m % 4 == 0, m <= 64, 4-byte aligned code rows: the lane keeps its rows' codes in registers across the query block (the
// table then fits one segment).  Otherwise the codes are read again per query (L1 / L2 hits: a tile is at most 2048 x m bytes).
template <bool REG, int RPL>
__global__ __launch_bounds__(PQ_SCAN_THREADS) void pq_scan_kernel(const float* __restrict__ lut, int nq, int m, int ksub, int seg_m,
                                                                  const uint8_t* __restrict__ codes, int64_t N,
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
#pragma unroll
  for (int r = 0; r < RPL; ++r) {
    const int64_t row = tile0 + (int64_t)r * PQ_SCAN_THREADS + tid;
    const bool live = row < N;
    idb[r] = (live && inv_db) ? inv_db[row] : 1.f;
    if (REG) {
      const uint32_t* cr = reinterpret_cast<const uint32_t*>(codes + (live ? row : 0) * m);
#pragma unroll
      for (int w = 0; w < PQ_SCAN_REG_DW; ++w) creg[r][w] = (live && w * 4 < m) ? cr[w] : 0u;
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
      const int cnt = sn * ksub;
      const float* src = lq + (int64_t)s0 * ksub;
      __syncthreads();   // the readers of the previous table are done
      if ((cnt & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* t4 = reinterpret_cast<float4*>(tab);
        for (int e = tid; e < (cnt >> 2); e += PQ_SCAN_THREADS) t4[e] = s4[e];
      } else {
        for (int e = tid; e < cnt; e += PQ_SCAN_THREADS) tab[e] = src[e];
      }
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
#pragma unroll
            for (int b = 0; b < 4; ++b) {
#pragma unroll
              for (int r = 0; r < RPL; ++r) sum[r] = __fadd_rn(sum[r], t0[b * ksub + ((u[r] >> (8 * b)) & 255u)]);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      } else {
        const bool dw = (m & 3) == 0 && (seg_m & 3) == 0 && (reinterpret_cast<uintptr_t>(codes) & 3) == 0;
#pragma unroll
        for (int r = 0; r < RPL; ++r) {
          const int64_t row = tile0 + (int64_t)r * PQ_SCAN_THREADS + tid;
          if (row < N) {
            const uint8_t* cr = codes + row * m + s0;
            float a = sum[r];
            int s = 0;
            if (dw) {
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
      const int64_t row = tile0 + (int64_t)r * PQ_SCAN_THREADS + tid;
      if (row < N) panel[q * ld + row] = __fmul_rn(__fmul_rn(sum[r], iq), idb[r]);
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

#define PQ_NEED(p, what) \
  if (!(p)) PVS_FAIL(PVS_ERR_INVALID, "%s: null %s", __func__, what)
#define PQ_ALIGNED(p, a, what) \
  if (reinterpret_cast<uintptr_t>(p) % (a)) PVS_FAIL(PVS_ERR_INVALID, "%s: %s must be %d-byte aligned", __func__, what, (int)(a))

static int pq_check_shape(const char* fn, int m, int ksub, int dsub) {
  if (m < 1 || dsub < 1 || ksub < 1 || ksub > 256)
    PVS_FAIL(PVS_ERR_INVALID, "%s: need m >= 1, dsub >= 1 and 1 <= ksub <= 256 (got m=%d, ksub=%d, dsub=%d)", fn, m, ksub, dsub);
  if ((int64_t)m * dsub > (int64_t)1 << 24) PVS_FAIL(PVS_ERR_INVALID, "%s: m * dsub = %lld is too large", fn, (long long)m * dsub);
  return PVS_OK;
}

PVS_EXPORT int pvs_pq_create(pvs_ctx* ctx, const float* codebooks, int m, int ksub, int dsub, pvs_pq** out) {
  PQ_NEED(ctx, "ctx");
  PQ_NEED(codebooks, "codebooks");
  PQ_NEED(out, "out");
  PVS_TRY(pq_check_shape(__func__, m, ksub, dsub));
  if (dsub > PQ_ENC_LDS_FLOATS) PVS_FAIL(PVS_ERR_UNSUPPORTED, "pvs_pq_create: dsub = %d exceeds %d", dsub, PQ_ENC_LDS_FLOATS);
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
  PQ_NEED(ctx, "ctx");
  PQ_NEED(pq, "pq");
  const int d = pq->m * pq->dsub;
  if (n < 0 || n > ((int64_t)1 << 38)) PVS_FAIL(PVS_ERR_INVALID, "pvs_pq_encode_dev: bad n = %lld", (long long)n);
  if (n == 0) return PVS_OK;
  PQ_NEED(d_x, "x");
  PQ_NEED(d_codes, "codes");
  PQ_ALIGNED(d_x, 4, "x");
  if (pq->m > 65535) PVS_FAIL(PVS_ERR_UNSUPPORTED, "pvs_pq_encode_dev: m = %d exceeds 65535", pq->m);
  PVS_HIP(hipSetDevice(ctx->device));
  const int jc = std::max(1, std::min(pq->ksub, PQ_ENC_LDS_FLOATS / pq->dsub));
  const size_t lds = (size_t)jc * pq->dsub * sizeof(float);
  ScopedTimer t(ctx, T_MISC);
  const dim3 grid((unsigned)((n + PQ_ENC_THREADS - 1) / PQ_ENC_THREADS), (unsigned)pq->m);
  hipLaunchKernelGGL(pq_encode_kernel, grid, dim3(PQ_ENC_THREADS), lds, ctx->stream, d_x, n, d, pq->d_cb, pq->m, pq->ksub, pq->dsub, jc,
                     d_codes);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

PVS_EXPORT int pvs_pq_lut_dev(pvs_ctx* ctx, const pvs_pq* pq, const float* d_q, int64_t nq, float* d_lut) {
  PQ_NEED(ctx, "ctx");
  PQ_NEED(pq, "pq");
  const int d = pq->m * pq->dsub;
  if (nq < 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_pq_lut_dev: negative nq");
  if (nq == 0) return PVS_OK;
  PQ_NEED(d_q, "q");
  PQ_NEED(d_lut, "lut");
  PQ_ALIGNED(d_q, 4, "q");
  PQ_ALIGNED(d_lut, 4, "lut");
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer t(ctx, T_MISC);
  for (int64_t q0 = 0; q0 < nq; q0 += 65535) {   // grid.y limit
    const int64_t qn = std::min<int64_t>(65535, nq - q0);
    hipLaunchKernelGGL(pq_lut_kernel, dim3((unsigned)pq->m, (unsigned)qn), dim3(256), 0, ctx->stream, d_q + q0 * d, d, pq->d_cb, pq->m,
                       pq->ksub, pq->dsub, d_lut + q0 * (int64_t)pq->m * pq->ksub);
    PVS_HIP(hipGetLastError());
  }
  return PVS_OK;
}

namespace pvs {
// one panel: scores of qn queries against cn rows into panel[qn][cn]
static int launch_pq_scan(pvs_ctx* ctx, const float* lut, int64_t qn, int m, int ksub, const uint8_t* codes, int64_t cn,
                          const float* inv_q, const float* inv_db, float* panel) {
  const int seg_m = std::max(1, PQ_SEG_ENTRIES / ksub);
  const size_t lds = (size_t)std::min(m, seg_m) * ksub * sizeof(float);
  const bool reg = (m & 3) == 0 && m <= 4 * PQ_SCAN_REG_DW && (reinterpret_cast<uintptr_t>(codes) & 3) == 0;
  const int64_t qblocks = (qn + PQ_SCAN_QB - 1) / PQ_SCAN_QB;
  // four rows per lane quarter the table copies per row; one row per lane when that would leave compute units idle
  const int64_t big_tiles = (cn + (int64_t)PQ_SCAN_THREADS * PQ_SCAN_RPL - 1) / ((int64_t)PQ_SCAN_THREADS * PQ_SCAN_RPL);
  const int rpl = big_tiles * qblocks >= 2 * (int64_t)ctx->num_cu ? PQ_SCAN_RPL : 1;
  const int64_t tiles = (cn + (int64_t)PQ_SCAN_THREADS * rpl - 1) / ((int64_t)PQ_SCAN_THREADS * rpl);
  using scan_fn = void (*)(const float*, int, int, int, int, const uint8_t*, int64_t, const float*, const float*, float*, int64_t);
  const scan_fn kern = reg ? (rpl == 1 ? pq_scan_kernel<true, 1> : pq_scan_kernel<true, PQ_SCAN_RPL>)
                           : (rpl == 1 ? pq_scan_kernel<false, 1> : pq_scan_kernel<false, PQ_SCAN_RPL>);
  if (lds > 48 * 1024) PVS_TRY(ensure_lds(ctx, reinterpret_cast<const void*>(kern), lds));
  const dim3 grid((unsigned)tiles, (unsigned)qblocks);
  hipLaunchKernelGGL(kern, grid, dim3(PQ_SCAN_THREADS), lds, ctx->stream, lut, (int)qn, m, ksub, seg_m, codes, cn, inv_q, inv_db, panel, cn);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}
}  // namespace pvs

PVS_EXPORT int pvs_pq_scan_topk_dev(pvs_ctx* ctx, const float* d_lut, int64_t nq, int m, int ksub, const uint8_t* d_codes, int64_t N,
                                    const float* d_inv_q, const float* d_inv_db, int k, int64_t col_offset, int merge, int64_t* d_idx,
                                    float* d_val) {
  PQ_NEED(ctx, "ctx");
  PVS_TRY(pq_check_shape(__func__, m, ksub, 1));
  if (nq < 0 || N < 0 || col_offset < 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_pq_scan_topk_dev: negative nq, N or col_offset");
  if (nq == 0) return PVS_OK;
  if (k < 1 || k > N) PVS_FAIL(PVS_ERR_INVALID, "pvs_pq_scan_topk_dev: need 1 <= k <= N (k = %d, N = %lld)", k, (long long)N);
  PQ_NEED(d_lut, "lut");
  PQ_NEED(d_codes, "codes");
  PQ_NEED(d_idx, "idx");
  PQ_NEED(d_val, "val");
  PQ_ALIGNED(d_lut, 4, "lut");
  PQ_ALIGNED(d_idx, 8, "idx");
  PQ_ALIGNED(d_val, 4, "val");
  if (d_inv_q) PQ_ALIGNED(d_inv_q, 4, "inv_q");
  if (d_inv_db) PQ_ALIGNED(d_inv_db, 4, "inv_db");
  // ranking deeper than 1024 pages through complete score rows (topk.hip), so the panel then spans all N columns
  const bool deep = k > 1024;
  if (deep && (merge || N > (int64_t)1 << 28)) PVS_FAIL(PVS_ERR_UNSUPPORTED, "ranking depth %d needs a single panel", k);
  PVS_HIP(hipSetDevice(ctx->device));
  const int64_t QT = deep ? std::max<int64_t>(1, std::min<int64_t>(nq, ((int64_t)1 << 28) / N)) : std::min<int64_t>(nq, PQ_PANEL_QUERIES);
  const int64_t NC = deep ? N : std::min<int64_t>(N, std::max<int64_t>(PQ_PANEL_MIN_COLS, PQ_PANEL_ELEMS / QT));
  float* panel = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_PANEL_OUT, (size_t)QT * NC * sizeof(float), &panel));
  const int64_t tsize = (int64_t)m * ksub;
  for (int64_t q0 = 0; q0 < nq; q0 += QT) {
    const int64_t qn = std::min(QT, nq - q0);
    for (int64_t c0 = 0; c0 < N; c0 += NC) {
      const int64_t cn = std::min(NC, N - c0);
      {
        ScopedTimer t(ctx, T_GEMM);   // the scoring slot: the scan stands where the similarity GEMM stands in the dense path
        PVS_TRY(launch_pq_scan(ctx, d_lut + q0 * tsize, qn, m, ksub, d_codes + c0 * m, cn, d_inv_q ? d_inv_q + q0 : nullptr,
                               d_inv_db ? d_inv_db + c0 : nullptr, panel));
      }
      PVS_TRY(launch_topk(ctx, panel, qn, cn, cn, k, col_offset + c0, (merge || c0 > 0) ? 1 : 0, d_idx + q0 * k, d_val + q0 * k));
    }
  }
  return PVS_OK;
}

PVS_EXPORT int pvs_rescore_rows_dev(pvs_ctx* ctx, const float* d_Q, int64_t nq, const float* d_X, int64_t N, int64_t d,
                                    const float* d_inv_q, const float* d_inv_db, const int64_t* d_cand, int64_t R, float* d_val) {
  PQ_NEED(ctx, "ctx");
  if (nq < 0 || N < 0 || R < 0 || d < 1) PVS_FAIL(PVS_ERR_INVALID, "pvs_rescore_rows_dev: negative size or d < 1");
  if (nq == 0 || R == 0) return PVS_OK;
  if (nq * R > ((int64_t)1 << 38)) PVS_FAIL(PVS_ERR_INVALID, "pvs_rescore_rows_dev: nq * R is too large");
  PQ_NEED(d_Q, "Q");
  if (N > 0) PQ_NEED(d_X, "X");
  PQ_NEED(d_cand, "cand");
  PQ_NEED(d_val, "val");
  PQ_ALIGNED(d_Q, 4, "Q");
  PQ_ALIGNED(d_X, 4, "X");
  PQ_ALIGNED(d_cand, 8, "cand");
  PQ_ALIGNED(d_val, 4, "val");
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer t(ctx, T_RESCORE);
  hipLaunchKernelGGL(pq_rescore_kernel, dim3((unsigned)((nq * R + 255) / 256)), dim3(256), 0, ctx->stream, d_Q, nq, d_X, N, d, d_inv_q,
                     d_inv_db, d_cand, R, d_val);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}
