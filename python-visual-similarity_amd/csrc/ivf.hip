// Inverted lists for the compact index: IVFADC of Jegou, Douze, Schmid (PAMI 2011) for an inner-product score.
//   pvs_ivf_assign_dev      rows -> nearest coarse centroid (int32) and the residual rows (vector ALU, centroids in LDS)
//   pvs_ivf_coarse_dev      queries -> coarse terms q . c_l  [nq][nlist]  (the probe list is pvs_topk_dev on that panel)
//   pvs_ivf_scan_topk_dev   tables x the codes of the probed lists -> candidate rows (score, original id) -> list-mode top-k (topk.hip)
// q . x ~ q . c_l + q . r: the table of a query does not depend on the list, so one table serves all its probes and a list adds one
// scalar, the coarse term, as the start of the sum.  Every sum is DEFINED (include/pvsim.h): float32, ascending index, a multiply and
// an add rounded separately; this unit is compiled with -ffp-contract=off like pq.hip, and tests/ivf_numpy.py restates it.
#include <algorithm>
#include <functional>
#include <vector>

#include "common.hpp"

namespace pvs {

constexpr int IVF_ASSIGN_THREADS = 256;
constexpr int IVF_ASSIGN_LDS_FLOATS = 16384;   // centroid chunk of the assignment kernel: 64 KiB
constexpr int IVF_THREADS = 512;
constexpr int IVF_RPL = 4;                     // candidate slots per lane and tile
constexpr int IVF_TILE = IVF_THREADS * IVF_RPL;
constexpr int IVF_MAX_PROBE = 1024;
constexpr int IVF_SEG_ENTRIES = 36864;         // table entries per LDS segment: 144 KiB (the probe tables below take 12 KiB more)
constexpr int64_t IVF_CAND_BYTES = (int64_t)64 << 20;   // candidate rows of one query block (8 bytes per slot)
constexpr int64_t IVF_MIN_SLICE = 1024;        // candidate slots a workgroup serves at least: a table copy is m * ksub * 4 bytes

// ------------------------------------------------------------------------------------------------- assignment + residual
// pq_encode_kernel with one sub-space and int32 labels: one lane owns one row, the centroids pass through LDS in chunks of jc (all
// lanes read the same element: a broadcast).  acc_l = sum_t (x_t - c_lt)^2, t ascending; strict < keeps the lowest l on ties.
__global__ __launch_bounds__(IVF_ASSIGN_THREADS) void ivf_assign_kernel(const float* __restrict__ x, int64_t n, int d,
                                                                        const float* __restrict__ cent, int nlist, int jc,
                                                                        int32_t* __restrict__ list, float* __restrict__ resid) {
  extern __shared__ __attribute__((aligned(16))) float cw[];
  const int64_t row = (int64_t)blockIdx.x * IVF_ASSIGN_THREADS + threadIdx.x;
  const bool live = row < n;
  const float* xr = x + (live ? row : 0) * (int64_t)d;
  float best = 0.f;
  int bl = 0;
  for (int j0 = 0; j0 < nlist; j0 += jc) {
    const int jn = min(jc, nlist - j0);
    __syncthreads();
    for (int e = threadIdx.x; e < jn * d; e += IVF_ASSIGN_THREADS) cw[e] = cent[(int64_t)j0 * d + e];
    __syncthreads();
    if (live) {
      for (int j = 0; j < jn; ++j) {
        const float* c = cw + j * d;
        float acc = 0.f;
        for (int t = 0; t < d; ++t) {
          const float df = __fsub_rn(xr[t], c[t]);
          acc = __fadd_rn(acc, __fmul_rn(df, df));
        }
        if (j0 + j == 0 || acc < best) {
          best = acc;
          bl = j0 + j;
        }
      }
    }
  }
  if (!live) return;
  list[row] = bl;
  if (resid) {
    const float* c = cent + (int64_t)bl * d;
    float* r = resid + row * (int64_t)d;
    for (int t = 0; t < d; ++t) r[t] = __fsub_rn(xr[t], c[t]);
  }
}

// ------------------------------------------------------------------------------------------------- coarse terms
// coarse[q][l] = sum_t q[t] c[l][t], ascending t.  One thread per entry; the query element is the same for every lane.
__global__ __launch_bounds__(256) void ivf_coarse_kernel(const float* __restrict__ qv, int d, const float* __restrict__ cent, int nlist,
                                                         float* __restrict__ coarse) {
  const int64_t q = blockIdx.y;
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= nlist) return;
  const float* qs = qv + q * d;
  const float* c = cent + (int64_t)l * d;
  float acc = 0.f;
  for (int t = 0; t < d; ++t) acc = __fadd_rn(acc, __fmul_rn(qs[t], c[t]));
  coarse[q * nlist + l] = acc;
}

// ------------------------------------------------------------------------------------------------- probed scan
// block-wide inclusive scan of one int per thread (512 threads); tmp: LDS int[8]
__device__ __forceinline__ int ivf_block_incl_scan(int v, int* tmp, int lane, int wave) {
  int incl = v;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const int o = __shfl_up(incl, s, 64);
    if (lane >= s) incl += o;
  }
  if (lane == 63) tmp[wave] = incl;
  __syncthreads();
  int off = 0;
  for (int w = 0; w < wave; ++w) off += tmp[w];
  __syncthreads();
  return incl + off;
}

// Workgroup (g, q) of a grid (G, queries of the block).  The candidate row of query q is the concatenation of its probed lists in
// probe order: probe j owns the slots [incl[j] - len[j], incl[j]), and slot p of it is stored row start[j] + p; the slots from
// incl[nprobe - 1] up to W are padding (id -1).  The workgroup serves the slice [g S, (g + 1) S) of that row, S a multiple of the
// tile, whatever lists it falls into: the host sizes G from the list lengths alone, and a query with one long probed list spreads
// over as many workgroups as a query with many short ones.  The table (or one segment of seg_m sub-spaces of it) is copied to LDS
// once per workgroup when it is one segment, once per tile and segment otherwise; a lane owns up to IVF_RPL slots of a tile, finds
// each slot's probe by a binary search of incl[] in LDS, reads the slot's codes 16 bytes at a time and gathers tab[s][code[s]]
// for s ascending.  The running sum of a slot starts at its probe's coarse term and lives in a register across the segments.
// Every slot of [0, W) is written exactly once, by the lane that owns it: no atomics, no order-dependent writes.
// vec: m % 16 == 0, 16-byte aligned codes and segments that start on a multiple of 16 sub-spaces.
__global__ __launch_bounds__(IVF_THREADS) void ivf_scan_kernel(const float* __restrict__ lut, int m, int ksub, int seg_m, int vec,
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
    const int both = ivf_block_incl_scan(len[0] + len[1], stmp, lane, wave);
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
  auto copy_segment = [&](int s0, int sn) {
    const int cnt = sn * ksub;
    const float* src = lq + (int64_t)s0 * ksub;
    if ((cnt & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
      const float4* s4 = reinterpret_cast<const float4*>(src);
      float4* t4 = reinterpret_cast<float4*>(tab);
      for (int e = tid; e < (cnt >> 2); e += IVF_THREADS) t4[e] = s4[e];
    } else {
      for (int e = tid; e < cnt; e += IVF_THREADS) tab[e] = src[e];
    }
  };
  if (one_seg) {
    copy_segment(0, m);
    __syncthreads();
  }
  const bool dw = (m & 3) == 0 && (one_seg || (seg_m & 3) == 0) && (reinterpret_cast<uintptr_t>(codes) & 3) == 0;

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
        copy_segment(s0, sn);
        __syncthreads();
      }
      const uint8_t* cr[IVF_RPL];
#pragma unroll
      for (int r = 0; r < IVF_RPL; ++r) cr[r] = codes + row[r] * m + s0;
      int s = 0;
      if (vec) {
        for (; s + 16 <= sn; s += 16) {
          uint4 u[IVF_RPL];
#pragma unroll
          for (int r = 0; r < IVF_RPL; ++r)
            u[r] = live[r] ? *reinterpret_cast<const uint4*>(cr[r] + s) : make_uint4(0u, 0u, 0u, 0u);
          const float* t0p = tab + s * ksub;
#pragma unroll
          for (int w = 0; w < 4; ++w) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
#pragma unroll
              for (int r = 0; r < IVF_RPL; ++r) {
                const uint32_t word = w == 0 ? u[r].x : w == 1 ? u[r].y : w == 2 ? u[r].z : u[r].w;
                sum[r] = __fadd_rn(sum[r], t0p[(4 * w + b) * ksub + ((word >> (8 * b)) & 255u)]);
              }
            }
          }
        }
      } else if (dw) {
        for (; s + 4 <= sn; s += 4) {
          uint32_t u[IVF_RPL];
#pragma unroll
          for (int r = 0; r < IVF_RPL; ++r) u[r] = live[r] ? *reinterpret_cast<const uint32_t*>(cr[r] + s) : 0u;
#pragma unroll
          for (int b = 0; b < 4; ++b) {
#pragma unroll
            for (int r = 0; r < IVF_RPL; ++r) sum[r] = __fadd_rn(sum[r], tab[(s + b) * ksub + ((u[r] >> (8 * b)) & 255u)]);
          }
        }
      }
      for (; s < sn; ++s) {
#pragma unroll
        for (int r = 0; r < IVF_RPL; ++r) {
          const uint32_t c = live[r] ? cr[r][s] : 0u;
          sum[r] = __fadd_rn(sum[r], tab[s * ksub + c]);
        }
      }
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

#define IVF_NEED(p, what) \
  if (!(p)) PVS_FAIL(PVS_ERR_INVALID, "%s: null %s", __func__, what)
#define IVF_ALIGNED(p, a, what) \
  if (reinterpret_cast<uintptr_t>(p) % (a)) PVS_FAIL(PVS_ERR_INVALID, "%s: %s must be %d-byte aligned", __func__, what, (int)(a))

static int ivf_check_coarse(const char* fn, int d, int nlist) {
  if (d < 1 || d > (1 << 24)) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= d <= 2^24 (got %d)", fn, d);
  if (nlist < 1 || nlist > 65536) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= nlist <= 65536 (got %d)", fn, nlist);
  return PVS_OK;
}

PVS_EXPORT int pvs_ivf_assign_dev(pvs_ctx* ctx, const float* d_x, int64_t n, int d, const float* d_centroids, int nlist,
                                  int32_t* d_list, float* d_residual) {
  IVF_NEED(ctx, "ctx");
  PVS_TRY(ivf_check_coarse(__func__, d, nlist));
  if (n < 0 || n >= ((int64_t)1 << 31)) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_assign_dev: need 0 <= n < 2^31 (got %lld)", (long long)n);
  if (n == 0) return PVS_OK;
  IVF_NEED(d_x, "x");
  IVF_NEED(d_centroids, "centroids");
  IVF_NEED(d_list, "list");
  IVF_ALIGNED(d_x, 4, "x");
  IVF_ALIGNED(d_centroids, 4, "centroids");
  IVF_ALIGNED(d_list, 4, "list");
  if (d_residual) IVF_ALIGNED(d_residual, 4, "residual");
  if (d > IVF_ASSIGN_LDS_FLOATS) PVS_FAIL(PVS_ERR_UNSUPPORTED, "pvs_ivf_assign_dev: d = %d exceeds %d", d, IVF_ASSIGN_LDS_FLOATS);
  PVS_HIP(hipSetDevice(ctx->device));
  const int jc = std::max(1, std::min(nlist, IVF_ASSIGN_LDS_FLOATS / d));
  const size_t lds = (size_t)jc * d * sizeof(float);
  ScopedTimer t(ctx, T_MISC);
  const dim3 grid((unsigned)((n + IVF_ASSIGN_THREADS - 1) / IVF_ASSIGN_THREADS));
  return launch_lds(ctx, ivf_assign_kernel, grid, dim3(IVF_ASSIGN_THREADS), lds, d_x, n, d, d_centroids, nlist, jc, d_list, d_residual);
}

PVS_EXPORT int pvs_ivf_coarse_dev(pvs_ctx* ctx, const float* d_q, int64_t nq, int d, const float* d_centroids, int nlist,
                                  float* d_coarse) {
  IVF_NEED(ctx, "ctx");
  PVS_TRY(ivf_check_coarse(__func__, d, nlist));
  if (nq < 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_coarse_dev: negative nq");
  if (nq == 0) return PVS_OK;
  IVF_NEED(d_q, "q");
  IVF_NEED(d_centroids, "centroids");
  IVF_NEED(d_coarse, "coarse");
  IVF_ALIGNED(d_q, 4, "q");
  IVF_ALIGNED(d_centroids, 4, "centroids");
  IVF_ALIGNED(d_coarse, 4, "coarse");
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer t(ctx, T_MISC);
  for (int64_t q0 = 0; q0 < nq; q0 += 65535) {   // grid.y limit
    const int64_t qn = std::min<int64_t>(65535, nq - q0);
    hipLaunchKernelGGL(ivf_coarse_kernel, dim3((unsigned)((nlist + 255) / 256), (unsigned)qn), dim3(256), 0, ctx->stream, d_q + q0 * d, d,
                       d_centroids, nlist, d_coarse + q0 * nlist);
    PVS_HIP(hipGetLastError());
  }
  return PVS_OK;
}

PVS_EXPORT int pvs_ivf_scan_topk_dev(pvs_ctx* ctx, const float* d_lut, int64_t nq, int m, int ksub, const int64_t* d_probe,
                                     const float* d_probe_val, int nprobe, const int64_t* d_list_off, const int64_t* h_list_off,
                                     int nlist, const uint8_t* d_codes, const int32_t* d_ids, const float* d_inv_q,
                                     const float* d_inv_db, int k, int64_t* d_idx, float* d_val) {
  IVF_NEED(ctx, "ctx");
  if (m < 1 || ksub < 1 || ksub > 256 || m > (1 << 24))
    PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_scan_topk_dev: need 1 <= m <= 2^24 and 1 <= ksub <= 256 (got m=%d, ksub=%d)", m, ksub);
  if (nlist < 1 || nlist > 65536) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_scan_topk_dev: need 1 <= nlist <= 65536 (got %d)", nlist);
  if (nprobe < 1 || nprobe > std::min(nlist, IVF_MAX_PROBE))
    PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_scan_topk_dev: need 1 <= nprobe <= min(nlist, %d) (got nprobe=%d, nlist=%d)", IVF_MAX_PROBE, nprobe,
             nlist);
  if (k < 1 || k > 1024) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_scan_topk_dev: need 1 <= k <= 1024 (got %d)", k);
  if (nq < 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_scan_topk_dev: negative nq");
  IVF_NEED(h_list_off, "host list_off");
  if (h_list_off[0] != 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_scan_topk_dev: list_off[0] must be 0");
  for (int l = 0; l < nlist; ++l)
    if (h_list_off[l + 1] < h_list_off[l]) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_scan_topk_dev: list_off must not decrease (list %d)", l);
  const int64_t N = h_list_off[nlist];
  if (N >= ((int64_t)1 << 31)) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_scan_topk_dev: need N < 2^31 (got %lld)", (long long)N);
  if (nq == 0) return PVS_OK;
  IVF_NEED(d_lut, "lut");
  IVF_NEED(d_probe, "probe");
  IVF_NEED(d_probe_val, "probe values");
  IVF_NEED(d_list_off, "list_off");
  if (N > 0) {
    IVF_NEED(d_codes, "codes");
    IVF_NEED(d_ids, "ids");
  }
  IVF_NEED(d_idx, "idx");
  IVF_NEED(d_val, "val");
  IVF_ALIGNED(d_lut, 4, "lut");
  IVF_ALIGNED(d_probe, 8, "probe");
  IVF_ALIGNED(d_probe_val, 4, "probe values");
  IVF_ALIGNED(d_list_off, 8, "list_off");
  IVF_ALIGNED(d_ids, 4, "ids");
  IVF_ALIGNED(d_idx, 8, "idx");
  IVF_ALIGNED(d_val, 4, "val");
  if (d_inv_q) IVF_ALIGNED(d_inv_q, 4, "inv_q");
  if (d_inv_db) IVF_ALIGNED(d_inv_db, 4, "inv_db");
  PVS_HIP(hipSetDevice(ctx->device));

  // W: no query's candidate row is longer than the nprobe longest lists together
  std::vector<int64_t> len(nlist);
  for (int l = 0; l < nlist; ++l) len[l] = h_list_off[l + 1] - h_list_off[l];
  std::nth_element(len.begin(), len.begin() + (nprobe - 1), len.end(), std::greater<int64_t>());
  int64_t W = 0;
  for (int j = 0; j < nprobe; ++j) W += len[j];
  W = std::max<int64_t>(64, (W + 63) / 64 * 64);
  // G workgroups per query: enough for two per compute unit over the query block, each with at least IVF_MIN_SLICE slots
  const int64_t QB = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nq, 65535), IVF_CAND_BYTES / (8 * W)));
  const int64_t want = (2 * (int64_t)ctx->num_cu + QB - 1) / QB;
  const int64_t G0 = std::max<int64_t>(1, std::min<int64_t>(want, W / IVF_MIN_SLICE));
  const int64_t S = ((W + G0 - 1) / G0 + IVF_TILE - 1) / IVF_TILE * IVF_TILE;
  const int64_t G = (W + S - 1) / S;
  const IvfCandLayout lay = ivf_cand_layout((size_t)QB, (size_t)W);
  void* block = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_IVF_CANDIDATES, lay.bytes, &block));
  float* cval = lay.val(block);
  int32_t* cid = lay.id(block);

  const int seg_m = std::max(1, IVF_SEG_ENTRIES / ksub);
  const size_t lds = (size_t)std::min(m, seg_m) * ksub * sizeof(float);
  const int vec = (m % 16 == 0) && (seg_m >= m || seg_m % 16 == 0) && (reinterpret_cast<uintptr_t>(d_codes) % 16 == 0);
  const int64_t tsize = (int64_t)m * ksub;
  for (int64_t q0 = 0; q0 < nq; q0 += QB) {
    const int64_t qn = std::min(QB, nq - q0);
    {
      ScopedTimer t(ctx, T_GEMM);   // the scoring slot, as the flat scan
      PVS_TRY(launch_lds(ctx, ivf_scan_kernel, dim3((unsigned)G, (unsigned)qn), dim3(IVF_THREADS), lds, d_lut + q0 * tsize, m, ksub, seg_m,
                         vec, d_probe + q0 * nprobe, d_probe_val + q0 * nprobe, nprobe, d_list_off, nlist, d_codes, d_ids,
                         d_inv_q ? d_inv_q + q0 : nullptr, d_inv_db, W, S, cval, cid));
    }
    PVS_TRY(launch_topk_candidates(ctx, cid, cval, qn, W, k, d_idx + q0 * k, d_val + q0 * k));
  }
  return PVS_OK;
}
