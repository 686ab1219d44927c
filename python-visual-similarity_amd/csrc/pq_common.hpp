// The quantiser core of the compact index, shared by pq.hip (flat scan) and ivf.hip (inverted lists, section 14);
// both units are compiled with -ffp-contract=off.  Every sum is DEFINED (include/pvsim.h): float32, ascending index, a multiply and
// an add rounded separately, so each piece below exists once and the NumPy twins (tests/pq_numpy.py, tests/ivf_numpy.py) see one order.
//   scan_plan, scan_shape_ok    host: segment size, LDS bytes and code-load width of a scan; the (m, ksub) range both scans accept
//   nearest_codeword_kernel     rows -> nearest codeword per sub-space (uint8 codes or int32 labels), optional residual
//   dot_table_kernel            queries -> inner products with every codeword [nq][m][ksub]
//   copy_table_segment          table segment -> LDS
//   gather_dword, walk_segment  tab[s][code[s]] for s ascending over R rows per lane, rows interleaved innermost (gather_dword: the
//                               flat scan's register path too; walk_segment: the probed scan; the flat scan's generic path walks
//                               row by row, where the interleaved walk measured slower on 4-byte loads)
// The host part needs no HIP header: bench/scan_plan_check.cpp includes this file alone, with a host compiler.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace pvs {

// A scan walks the table in LDS segments of seg_m sub-spaces (`entries` table entries at most; one segment when seg_m >= m) and reads
// a row's codes `width` bytes at a time: 16 or 4 when m, every segment start and the code base are multiples of it, single bytes
// otherwise.  This is the one place where the width is decided; the kernels take it as an argument.
struct ScanPlan {
  int seg_m;
  size_t lds;   // bytes of the table segment
  int width;    // 16, 4 or 1
};
inline ScanPlan scan_plan(int m, int ksub, int entries, const void* codes) {
  const int seg_m = std::max(1, entries / ksub);
  const auto fits = [&](int w) { return m % w == 0 && (seg_m >= m || seg_m % w == 0) && reinterpret_cast<uintptr_t>(codes) % w == 0; };
  return {seg_m, (size_t)std::min(m, seg_m) * ksub * sizeof(float), fits(16) ? 16 : fits(4) ? 4 : 1};
}

inline bool scan_shape_ok(int m, int ksub) { return m >= 1 && m <= (1 << 24) && ksub >= 1 && ksub <= 256; }

}  // namespace pvs

#ifdef __HIPCC__
#include "common.hpp"

namespace pvs {

constexpr int NEAREST_THREADS = 256;
constexpr int NEAREST_LDS_FLOATS = 16384;   // codeword chunk of the nearest-codeword kernel: 64 KiB
constexpr int TABLE_THREADS = 256;

// ------------------------------------------------------------------------------------------------- nearest codeword
// One lane owns one row of one sub-space (blockIdx.y); the codewords of the sub-space pass through LDS in chunks of jc (all lanes
// read the same codeword element: an LDS broadcast).  acc_j = sum_t (x_t - c_jt)^2 in ascending t; strict < keeps the lowest j on
// ties.  resid, when given, receives x - c of the winner, one subtraction per element.
template <class Label>
__global__ __launch_bounds__(NEAREST_THREADS) void nearest_codeword_kernel(const float* __restrict__ x, int64_t n, int d,
                                                                           const float* __restrict__ cb, int m, int ksub, int dsub, int jc,
                                                                           Label* __restrict__ out, float* __restrict__ resid) {
  extern __shared__ __attribute__((aligned(16))) float cw[];
  const int s = blockIdx.y;
  const int64_t row = (int64_t)blockIdx.x * NEAREST_THREADS + threadIdx.x;
  const bool live = row < n;
  const float* xr = x + (live ? row : 0) * (int64_t)d + (int64_t)s * dsub;
  const float* cs = cb + (int64_t)s * ksub * dsub;
  float best = 0.f;
  int bj = 0;
  for (int j0 = 0; j0 < ksub; j0 += jc) {
    const int jn = min(jc, ksub - j0);
    __syncthreads();
    for (int e = threadIdx.x; e < jn * dsub; e += NEAREST_THREADS) cw[e] = cs[(int64_t)j0 * dsub + e];
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
  if (!live) return;
  out[row * m + s] = (Label)bj;
  if (resid) {
    const float* c = cs + (int64_t)bj * dsub;
    float* r = resid + row * (int64_t)d + (int64_t)s * dsub;
    for (int t = 0; t < dsub; ++t) r[t] = __fsub_rn(xr[t], c[t]);
  }
}

template <class Label>
inline int launch_nearest_codeword(pvs_ctx* ctx, const float* x, int64_t n, const float* cb, int m, int ksub, int dsub, Label* out,
                                   float* resid) {
  const int jc = std::max(1, std::min(ksub, NEAREST_LDS_FLOATS / dsub));
  ScopedTimer t(ctx, T_MISC);
  const dim3 grid((unsigned)((n + NEAREST_THREADS - 1) / NEAREST_THREADS), (unsigned)m);
  return launch_lds(ctx, nearest_codeword_kernel<Label>, grid, dim3(NEAREST_THREADS), (size_t)jc * dsub * sizeof(float), x, n, m * dsub, cb,
                    m, ksub, dsub, jc, out, resid);
}

// ------------------------------------------------------------------------------------------------- table
// out[q][s][j] = sum_t q[s dsub + t] c[s][j][t], ascending t.  One thread per entry; blockIdx.x = (sub-space << jshift) | block of 256
// entries of it, 2^jshift >= the blocks a sub-space needs (a shift and a mask per block: a block is a few instructions at small dsub,
// and an integer division at its head cost 5 to 10 % of the table stage); blockIdx.y = query.
static __global__ __launch_bounds__(TABLE_THREADS) void dot_table_kernel(const float* __restrict__ qv, int d, const float* __restrict__ cb,
                                                                         int m, int ksub, int dsub, int jshift, float* __restrict__ out) {
  const int s = blockIdx.x >> jshift;
  const int j = (blockIdx.x & ((1u << jshift) - 1)) * TABLE_THREADS + threadIdx.x;
  if (j >= ksub) return;
  const int64_t q = blockIdx.y;
  const float* qs = qv + q * d + (int64_t)s * dsub;
  const float* c = cb + ((int64_t)s * ksub + j) * dsub;
  float acc = 0.f;
  for (int t = 0; t < dsub; ++t) acc = __fadd_rn(acc, __fmul_rn(qs[t], c[t]));
  out[(q * m + s) * ksub + j] = acc;
}

inline int launch_dot_table(pvs_ctx* ctx, const float* q, int64_t nq, const float* cb, int m, int ksub, int dsub, float* out) {
  const int d = m * dsub;
  int jshift = 0;
  while ((TABLE_THREADS << jshift) < ksub) ++jshift;
  ScopedTimer t(ctx, T_MISC);
  for (int64_t q0 = 0; q0 < nq; q0 += 65535) {   // grid.y limit
    const int64_t qn = std::min<int64_t>(65535, nq - q0);
    hipLaunchKernelGGL(dot_table_kernel, dim3((unsigned)m << jshift, (unsigned)qn), dim3(TABLE_THREADS), 0, ctx->stream, q + q0 * d, d,
                       cb, m, ksub, dsub, jshift, out + q0 * (int64_t)m * ksub);
    PVS_HIP(hipGetLastError());
  }
  return PVS_OK;
}

// ------------------------------------------------------------------------------------------------- scan pieces
// cnt table entries from src to LDS by a workgroup of THREADS lanes; the caller puts the barriers around it
template <int THREADS>
__device__ __forceinline__ void copy_table_segment(float* __restrict__ tab, const float* __restrict__ src, int cnt, int tid) {
  if ((cnt & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* t4 = reinterpret_cast<float4*>(tab);
    for (int e = tid; e < (cnt >> 2); e += THREADS) t4[e] = s4[e];
  } else {
    for (int e = tid; e < cnt; e += THREADS) tab[e] = src[e];
  }
}

// the four codes of one dword per row, b ascending, rows innermost; t0 = the table rows of the dword's first sub-space
template <int R>
__device__ __forceinline__ void gather_dword(float (&sum)[R], const uint32_t (&u)[R], const float* t0, int ksub) {
#pragma unroll
  for (int b = 0; b < 4; ++b) {
#pragma unroll
    for (int r = 0; r < R; ++r) sum[r] = __fadd_rn(sum[r], t0[b * ksub + ((u[r] >> (8 * b)) & 255u)]);
  }
}

// One segment of sn sub-spaces (table rows in tab) over R rows per lane: cr[r] = the row's codes at the segment's first sub-space,
// read `width` bytes at a time (a ScanPlan's), a dead row reads nothing and gathers entry 0.  s ascending per row.
template <int R>
__device__ __forceinline__ void walk_segment(float (&sum)[R], const uint8_t* const (&cr)[R], const bool (&live)[R], const float* tab,
                                             int ksub, int sn, int width) {
  int s = 0;
  if (width == 16) {
    for (; s + 16 <= sn; s += 16) {
      uint4 v[R];
#pragma unroll
      for (int r = 0; r < R; ++r) v[r] = live[r] ? *reinterpret_cast<const uint4*>(cr[r] + s) : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        uint32_t u[R];
#pragma unroll
        for (int r = 0; r < R; ++r) u[r] = w == 0 ? v[r].x : w == 1 ? v[r].y : w == 2 ? v[r].z : v[r].w;
        gather_dword<R>(sum, u, tab + (s + 4 * w) * ksub, ksub);
      }
    }
  }
  if (width >= 4) {
    for (; s + 4 <= sn; s += 4) {
      uint32_t u[R];
#pragma unroll
      for (int r = 0; r < R; ++r) u[r] = live[r] ? *reinterpret_cast<const uint32_t*>(cr[r] + s) : 0u;
      gather_dword<R>(sum, u, tab + s * ksub, ksub);
    }
  }
  for (; s < sn; ++s) {
#pragma unroll
    for (int r = 0; r < R; ++r) sum[r] = __fadd_rn(sum[r], tab[s * ksub + (live[r] ? cr[r][s] : 0u)]);
  }
}

}  // namespace pvs
#endif  // __HIPCC__
