// Int8 resident index: one signed byte per dimension, ranked by the cosine of the code rows.
//   pvs_sq8_encode_dev   float32 rows -> int8 codes [n][ld] (ld = 64 ceil(L / 64), zero padded) + 1 / sqrt(sum c^2) per row
//   pvs_sq8_topk_dev     query codes x database codes -> bounded score panel -> the top-k kernels of topk.hip, panel by panel
// The dot product of two code rows is an int32 (127^2 * 131072 < 2^31), so every tiling, split of the row and order of summation
// gives the same bits: the matrix path (v_mfma_i32_32x32x32_i8) and the row path (v_dot4 on 16-byte loads) agree exactly, and a
// NumPy restatement with int64 sums does too (tests/sq8_numpy.py).  The score is ((float)acc * inv_q) * inv_d: a conversion and
// two multiplies, each rounded on its own; nothing here is a multiply followed by an add, so the unit needs no -ffp-contract=off.
#include "panel_plan.hpp"

namespace pvs {
namespace {

using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x16 = __attribute__((ext_vector_type(16))) int;

constexpr int SQ_MAX_L = 131072;
constexpr int SQ_ENC_THREADS = 256;

constexpr int SQ_MM_THREADS = 256;   // four waves, 2 x 2, each owning 64 queries x 64 database rows
constexpr int SQ_MM_BQ = 128;        // queries of one workgroup
constexpr int SQ_MM_BD = 128;        // database rows of one workgroup
constexpr int SQ_MM_BK = 128;        // bytes of a row per k-block (four k-steps of 32)

constexpr int SQ_ROW_THREADS = 1024;             // sixteen waves, each walking whole database rows
constexpr int SQ_ROW_LDS = 128 * 1024;           // bytes of query codes per workgroup: 4 queries at L <= 32768, 1 at L = 131072
constexpr int SQ_ROW_MAX_Q = 4;                  // PVS_OPT_SQ8_PATH = 0 takes the row path up to this many queries

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------- encode
// c = (int8) rint((x / amax) * 127): an IEEE division, then a multiply, each rounded on its own; rint rounds half to even.
__device__ __forceinline__ int sq8_code(float x, float amax) { return (int)rintf((x / amax) * 127.0f); }

// Workgroups walk rows.  Pass one: amax (a maximum is exact in any order).  Pass two: a thread turns 16 consecutive elements into
// one 16-byte store, the padding bytes L .. ld included, and sums the squares of its codes (an integer: any order).
__global__ __launch_bounds__(SQ_ENC_THREADS) void sq8_encode_kernel(const float* __restrict__ x, int64_t n, int L, int ld, int vec,
                                                                    int8_t* __restrict__ codes, float* __restrict__ inv) {
  __shared__ float s_max[SQ_ENC_THREADS / WAVE];
  __shared__ int s_sum[SQ_ENC_THREADS / WAVE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
    const float* xr = x + row * L;
    float m = 0.f;
    if (vec) {
      const float4* x4 = reinterpret_cast<const float4*>(xr);
      for (int i = tid; i < L / 4; i += SQ_ENC_THREADS) {
        const float4 v = x4[i];
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
      }
    } else {
      for (int i = tid; i < L; i += SQ_ENC_THREADS) m = fmaxf(m, fabsf(xr[i]));
    }
    m = wave_max(m);
    if (lane == 0) s_max[wave] = m;
    __syncthreads();
    const float amax = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));

    int ss = 0;
    i32x4* out = reinterpret_cast<i32x4*>(codes + row * ld);
    for (int c = tid; c < ld / 16; c += SQ_ENC_THREADS) {
      const int t0 = c * 16;
      float v[16];
      if (vec && t0 + 16 <= L) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float4 f = *reinterpret_cast<const float4*>(xr + t0 + 4 * u);
          v[4 * u] = f.x, v[4 * u + 1] = f.y, v[4 * u + 2] = f.z, v[4 * u + 3] = f.w;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = t0 + e < L ? xr[t0 + e] : 0.f;
      }
      int w[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        unsigned pack = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int code = (amax == 0.f || t0 + 4 * u + e >= L) ? 0 : sq8_code(v[4 * u + e], amax);
          ss += code * code;
          pack |= (unsigned)(code & 255) << (8 * e);
        }
        w[u] = (int)pack;
      }
      out[c] = i32x4{w[0], w[1], w[2], w[3]};
    }
    ss = wave_sum(ss);
    if (lane == 0) s_sum[wave] = ss;
    __syncthreads();
    if (tid == 0) {
      const int total = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];   // at most 127^2 * 131072 < 2^31
      inv[row] = total == 0 ? 0.f : (float)(1.0 / sqrt((double)total));
    }
    __syncthreads();   // the next row writes s_max and s_sum again
  }
}

// ------------------------------------------------------------------------------------------------- matrix path
// panel[q][j] for 128 queries x 128 database rows per workgroup.  The query rows are the A operand of v_mfma_i32_32x32x32_i8 and the
// database rows its B operand, so a lane's 16 accumulators are 16 queries of ONE database row (column = lane & 31, row = (reg & 3) +
// 8 (reg >> 2) + 4 (lane >> 5)) and a panel store of one register covers 32 consecutive columns of two queries.  Both operands
// take byte 32 s + 16 (lane >> 5) + e of their row as element e of k-step s (the rule of match.hip), so the sum over the steps is
// the full dot product whatever order the instruction gives the 32 values of a step.  Rows past nq / N and bytes past ld are staged
// as zeros.  LDS rows are 128 bytes with the 16-byte chunk index xor-ed by (row & 7); the next k-block's global loads are issued
// before the current block is multiplied.
__global__ __launch_bounds__(SQ_MM_THREADS) void sq8_gemm_kernel(const int8_t* __restrict__ qc, const float* __restrict__ inv_q, int nq,
                                                                 const int8_t* __restrict__ dc, const float* __restrict__ inv_d, int64_t N,
                                                                 int ld, float* __restrict__ panel, int64_t ldp) {
  __shared__ __attribute__((aligned(16))) int8_t s_q[SQ_MM_BQ * SQ_MM_BK];
  __shared__ __attribute__((aligned(16))) int8_t s_d[SQ_MM_BD * SQ_MM_BK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int wq = wave & 1, wd = wave >> 1;
  const int64_t d0 = (int64_t)blockIdx.x * SQ_MM_BD;
  const int q0 = blockIdx.y * SQ_MM_BQ;

  // staging: thread -> 16-byte chunk (tid & 7) of rows (tid >> 3) + 32 u of both operands
  const int ch = tid & 7, srow = tid >> 3;
  i32x4 pre_q[4], pre_d[4];
  auto fetch = [&](int k0) {
    const bool in_k = k0 + 16 * ch < ld;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = srow + 32 * u;
      pre_q[u] = (in_k && q0 + row < nq) ? *reinterpret_cast<const i32x4*>(qc + (int64_t)(q0 + row) * ld + k0 + 16 * ch) : i32x4{0, 0, 0, 0};
      pre_d[u] = (in_k && d0 + row < N) ? *reinterpret_cast<const i32x4*>(dc + (d0 + row) * ld + k0 + 16 * ch) : i32x4{0, 0, 0, 0};
    }
  };

  i32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = i32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

  fetch(0);
  for (int k0 = 0; k0 < ld; k0 += SQ_MM_BK) {
    __syncthreads();                                     // every wave has multiplied the previous block
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = srow + 32 * u;
      const int off = row * SQ_MM_BK + ((ch ^ (row & 7)) << 4);
      *reinterpret_cast<i32x4*>(&s_q[off]) = pre_q[u];
      *reinterpret_cast<i32x4*>(&s_d[off]) = pre_d[u];
    }
    __syncthreads();
    if (k0 + SQ_MM_BK < ld) fetch(k0 + SQ_MM_BK);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      i32x4 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int qrow = wq * 64 + i * 32 + r, drow = wd * 64 + i * 32 + r;
        a[i] = *reinterpret_cast<const i32x4*>(&s_q[qrow * SQ_MM_BK + (((2 * s + h) ^ (qrow & 7)) << 4)]);
        b[i] = *reinterpret_cast<const i32x4*>(&s_d[drow * SQ_MM_BK + (((2 * s + h) ^ (drow & 7)) << 4)]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }

  // epilogue: convert, the query's factor, the row's factor
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t col = d0 + wd * 64 + j * 32 + r;
    if (col >= N) continue;
    const float idb = inv_d[col];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int q = q0 + wq * 64 + i * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        if (q < nq) panel[(int64_t)q * ldp + col] = ((float)acc[i][j][reg] * inv_q[q]) * idb;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------- row path
// One pass over the codes for up to QB queries whose codes sit in LDS.  A workgroup owns rows_per_wg consecutive database rows, a
// wave walks whole rows of them: 16 bytes per lane and load, four loads in flight, v_dot4 against each query's bytes at the same
// offsets.  The 64 partial sums of a row are added across the wave: integers, so the split changes nothing.
template <int QB>
__global__ __launch_bounds__(SQ_ROW_THREADS) void sq8_rows_kernel(const int8_t* __restrict__ qc, const float* __restrict__ inv_q, int nq,
                                                                  const int8_t* __restrict__ dc, const float* __restrict__ inv_d, int64_t N,
                                                                  int ld, int64_t rows_per_wg, float* __restrict__ panel, int64_t ldp) {
  extern __shared__ __attribute__((aligned(16))) int8_t s_qrows[];   // [QB][ld]
  i32x4* s4 = reinterpret_cast<i32x4*>(s_qrows);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.y * QB;
  const int qn = min(QB, nq - q0);
  const int nch = ld / 16;                         // 16-byte chunks of a row
  const i32x4* q4 = reinterpret_cast<const i32x4*>(qc + (int64_t)q0 * ld);
  for (int i = tid; i < QB * nch; i += SQ_ROW_THREADS) s4[i] = i < qn * nch ? q4[i] : i32x4{0, 0, 0, 0};
  __syncthreads();

  auto dot16 = [&](const i32x4 d, int c, int (&acc)[QB]) {
#pragma unroll
    for (int qi = 0; qi < QB; ++qi) {
      const i32x4 qv = s4[qi * nch + c];
      int a = acc[qi];
      a = __builtin_amdgcn_sdot4(qv.x, d.x, a, false);
      a = __builtin_amdgcn_sdot4(qv.y, d.y, a, false);
      a = __builtin_amdgcn_sdot4(qv.z, d.z, a, false);
      a = __builtin_amdgcn_sdot4(qv.w, d.w, a, false);
      acc[qi] = a;
    }
  };

  const int64_t row_begin = (int64_t)blockIdx.x * rows_per_wg;
  const int64_t row_end = row_begin + rows_per_wg < N ? row_begin + rows_per_wg : N;
  for (int64_t row = row_begin + wave; row < row_end; row += SQ_ROW_THREADS / WAVE) {
    const i32x4* d4 = reinterpret_cast<const i32x4*>(dc + row * ld);
    int acc[QB];
#pragma unroll
    for (int qi = 0; qi < QB; ++qi) acc[qi] = 0;
    int c = lane;
    for (; c + 192 < nch; c += 256) {
      const i32x4 v0 = d4[c], v1 = d4[c + 64], v2 = d4[c + 128], v3 = d4[c + 192];
      dot16(v0, c, acc);
      dot16(v1, c + 64, acc);
      dot16(v2, c + 128, acc);
      dot16(v3, c + 192, acc);
    }
    for (; c < nch; c += 64) dot16(d4[c], c, acc);
    const float idb = inv_d[row];
#pragma unroll
    for (int qi = 0; qi < QB; ++qi) {
      const int total = wave_sum(acc[qi]);
      if (lane == 0 && qi < qn) panel[(int64_t)(q0 + qi) * ldp + row] = ((float)total * inv_q[q0 + qi]) * idb;
    }
  }
}

template <int QB>
int launch_sq8_rows_qb(pvs_ctx* ctx, const int8_t* qc, const float* inv_q, int64_t qn, const int8_t* dc, const float* inv_d, int64_t cn,
                       int ld, float* panel) {
  constexpr int waves = SQ_ROW_THREADS / WAVE;
  // about two workgroups per compute unit, each amortising its copy of the query codes over its rows
  int64_t rows_per_wg = (cn + 2 * (int64_t)ctx->num_cu - 1) / (2 * (int64_t)ctx->num_cu);
  rows_per_wg = (rows_per_wg + waves - 1) / waves * waves;
  const int64_t wgs = (cn + rows_per_wg - 1) / rows_per_wg;
  const dim3 grid((unsigned)wgs, (unsigned)((qn + QB - 1) / QB));
  return launch_lds(ctx, sq8_rows_kernel<QB>, grid, dim3(SQ_ROW_THREADS), (size_t)QB * ld, qc, inv_q, (int)qn, dc, inv_d, cn, ld, rows_per_wg,
                    panel, cn);
}

}  // namespace

// PVS_OPT_SQ8_PATH: 1 the row scan, 2 the int8 GEMM, 0 the row scan up to SQ_ROW_MAX_Q queries of the call (subset.hip reads it too)
bool sq8_row_scan(const pvs_ctx* ctx, int64_t nq) {
  const int path = ctx->opt[PVS_OPT_SQ8_PATH];
  return path == 1 || (path == 0 && nq <= SQ_ROW_MAX_Q);
}

// one panel: scores of qn queries against cn rows into panel[qn][cn] (declared in common.hpp: subset.hip and the panel path of sq8_range.hip score their panels with it)
int launch_sq8_scores(pvs_ctx* ctx, bool rows, const int8_t* qc, const float* inv_q, int64_t qn, const int8_t* dc, const float* inv_d,
                      int64_t cn, int ld, float* panel) {
  if (rows) {
    const int fit = SQ_ROW_LDS / ld;             // queries whose codes fit the workgroup's LDS: >= 1 since ld <= 131072
    if (fit >= 4 && qn >= 3) return launch_sq8_rows_qb<4>(ctx, qc, inv_q, qn, dc, inv_d, cn, ld, panel);
    if (fit >= 2 && qn >= 2) return launch_sq8_rows_qb<2>(ctx, qc, inv_q, qn, dc, inv_d, cn, ld, panel);
    return launch_sq8_rows_qb<1>(ctx, qc, inv_q, qn, dc, inv_d, cn, ld, panel);
  }
  const dim3 grid((unsigned)((cn + SQ_MM_BD - 1) / SQ_MM_BD), (unsigned)((qn + SQ_MM_BQ - 1) / SQ_MM_BQ));
  hipLaunchKernelGGL(sq8_gemm_kernel, grid, dim3(SQ_MM_THREADS), 0, ctx->stream, qc, inv_q, (int)qn, dc, inv_d, cn, ld, panel, cn);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

}  // namespace pvs

using namespace pvs;

PVS_EXPORT int pvs_sq8_encode_dev(pvs_ctx* ctx, const float* d_x, int64_t n, int L, int8_t* d_codes, float* d_inv) {
  PVS_NEED(ctx, "ctx");
  if (n < 0 || n > ((int64_t)1 << 38)) PVS_FAIL(PVS_ERR_INVALID, "pvs_sq8_encode_dev: bad n = %lld", (long long)n);
  if (L < 1 || L > SQ_MAX_L) PVS_FAIL(PVS_ERR_INVALID, "pvs_sq8_encode_dev: need 1 <= L <= %d (got %d)", SQ_MAX_L, L);
  if (n == 0) return PVS_OK;
  PVS_NEED(d_x, "x");
  PVS_NEED(d_codes, "codes");
  PVS_NEED(d_inv, "inv");
  PVS_ALIGNED(d_x, 4, "x");
  PVS_ALIGNED(d_codes, 16, "codes");
  PVS_ALIGNED(d_inv, 4, "inv");
  PVS_HIP(hipSetDevice(ctx->device));
  const int ld = PVS_SQ8_LD(L);
  const int vec = (L % 4 == 0 && reinterpret_cast<uintptr_t>(d_x) % 16 == 0) ? 1 : 0;
  ScopedTimer t(ctx, T_MISC);
  hipLaunchKernelGGL(sq8_encode_kernel, dim3((unsigned)std::min<int64_t>(n, (int64_t)1 << 20)), dim3(SQ_ENC_THREADS), 0, ctx->stream, d_x, n, L,
                     ld, vec, d_codes, d_inv);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

PVS_EXPORT int pvs_sq8_topk_dev(pvs_ctx* ctx, const int8_t* d_qcodes, const float* d_inv_q, int64_t nq, const int8_t* d_codes,
                                const float* d_inv_db, int64_t N, int L, int k, int64_t col_offset, int merge, int64_t* d_idx,
                                float* d_val) {
  PVS_NEED(ctx, "ctx");
  if (L < 1 || L > SQ_MAX_L) PVS_FAIL(PVS_ERR_INVALID, "pvs_sq8_topk_dev: need 1 <= L <= %d (got %d)", SQ_MAX_L, L);
  if (nq < 0 || N < 0 || col_offset < 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_sq8_topk_dev: negative nq, N or col_offset");
  if (nq == 0) return PVS_OK;
  if (k < 1 || k > N) PVS_FAIL(PVS_ERR_INVALID, "pvs_sq8_topk_dev: need 1 <= k <= N (k = %d, N = %lld)", k, (long long)N);
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
  PanelPlan plan;   // panel_plan.hpp: the scan rule, as the ADC scan; complete rows for k > 1024
  PVS_TRY(panel_ranking_plan(panel_scan, nq, N, k, merge, &plan));
  PVS_HIP(hipSetDevice(ctx->device));
  const int ld = PVS_SQ8_LD(L);
  const bool rows = sq8_row_scan(ctx, nq);
  return panel_topk(ctx, plan, k, col_offset, merge, d_idx, d_val, [&](int64_t q0, int64_t qn, int64_t c0, int64_t cn, float* panel) -> int {
    ScopedTimer t(ctx, T_GEMM);   // the scoring slot, as the ADC scan
    return launch_sq8_scores(ctx, rows, d_qcodes + q0 * ld, d_inv_q + q0, qn, d_codes + c0 * ld, d_inv_db + c0, cn, ld, panel);
  });
}
