// Threshold join on the int8 code rows: "everything at least this similar" for an Int8Index.
//
//   pvs_sq8_range_dev   every (query row, database row, score) with score >= t, in the order and under the capacity protocol of
//                       pvs_cosine_range_dev (section 24); PVS_RANGE_UPPER = the self-join, pairs j > i with row i in the query role.
//
// The score is ((float)acc * inv_q[i]) * inv_d[j], the bits pvs_sq8_topk_dev reports for the pair: acc is an int32, so no tiling or
// order of summation changes it and there is nothing to prefilter or to re-score.  The score is NOT symmetric in its rows (two
// separately rounded products), so the self-join is defined by s(i, j) with i < j alone.
//   path 1, panel   launch_sq8_scores fills a float panel (row scan or GEMM, by PVS_OPT_SQ8_PATH), the count / scan / emit kernels of
//                   range_common.hpp threshold it where it lies.
//   path 2, mask    the GEMM of sq8.hip with another epilogue: the predicate of 32 consecutive columns of a query row is one ballot
//                   word, so a panel is one bit per pair.  Popcounts per row -> the same scan -> an emit that walks the words in
//                   order; the scores of the emitted pairs are then computed once, by the same expression on the same integer.
// Both paths keep panel, counters, row counts and row offsets in ONE block of WS_PANEL_OUT (panel_query_block_sized): its size does
// not change within a call, so the running total survives the reserve at the top of every row block.
#include <algorithm>
#include <cmath>

#include "range_common.hpp"

namespace pvs {
namespace {

using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x16 = __attribute__((ext_vector_type(16))) int;

constexpr int SQR_MAX_L = 131072;
constexpr int SQR_THREADS = 256;   // four waves, 2 x 2, each owning 64 queries x 64 database rows: the tile of sq8_gemm_kernel
constexpr int SQR_BQ = 128;
constexpr int SQR_BD = 128;
constexpr int SQR_BK = 128;

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// mask[q][w], q < 128 gridDim.y, w < words = 4 gridDim.x: bit b of word w of row q is the predicate of local pair (q, 32 w + b),
//   q < nq && col < N && s >= thr && (!upper || col0 + col > row0 + q),   s = ((float)acc * inv_q[q]) * inv_d[col].
// Operands and k-loop are those of sq8_gemm_kernel (byte 32 s + 16 (lane >> 5) + e of a row is element e of k-step s; rows past nq / N
// and bytes past ld are staged as zeros).  A lane's accumulator register holds query (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) of
// column lane & 31, so the ballot of one register is 32 consecutive columns of row R in its low half and of row R + 4 in its high
// half: lane 0 stores the low word, lane 32 the high one.  Every word of the 128 x 4 words of a workgroup is stored exactly once.
__global__ __launch_bounds__(SQR_THREADS) void sq8_range_gemm_kernel(const int8_t* __restrict__ qc, const float* __restrict__ inv_q, int nq,
                                                                     const int8_t* __restrict__ dc, const float* __restrict__ inv_d, int64_t N,
                                                                     int ld, float thr, int upper, int64_t row0, int64_t col0,
                                                                     uint32_t* __restrict__ mask, int64_t words) {
  __shared__ __attribute__((aligned(16))) int8_t s_q[SQR_BQ * SQR_BK];
  __shared__ __attribute__((aligned(16))) int8_t s_d[SQR_BD * SQR_BK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int wq = wave & 1, wd = wave >> 1;
  const int64_t d0 = (int64_t)blockIdx.x * SQR_BD;
  const int q0 = blockIdx.y * SQR_BQ;

  // the self-join: the largest column of the tile is not beyond its smallest row, so no pair j > i lies in it
  if (upper && col0 + d0 + SQR_BD <= row0 + q0 + 1) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = tid + SQR_THREADS * u;             // 128 rows x 4 words
      mask[(int64_t)(q0 + (idx >> 2)) * words + (int64_t)blockIdx.x * 4 + (idx & 3)] = 0u;
    }
    return;
  }

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
  for (int k0 = 0; k0 < ld; k0 += SQR_BK) {
    __syncthreads();                                     // every wave has multiplied the previous block
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = srow + 32 * u;
      const int off = row * SQR_BK + ((ch ^ (row & 7)) << 4);
      *reinterpret_cast<i32x4*>(&s_q[off]) = pre_q[u];
      *reinterpret_cast<i32x4*>(&s_d[off]) = pre_d[u];
    }
    __syncthreads();
    if (k0 + SQR_BK < ld) fetch(k0 + SQR_BK);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      i32x4 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int qrow = wq * 64 + i * 32 + r, drow = wd * 64 + i * 32 + r;
        a[i] = *reinterpret_cast<const i32x4*>(&s_q[qrow * SQR_BK + (((2 * s + h) ^ (qrow & 7)) << 4)]);
        b[i] = *reinterpret_cast<const i32x4*>(&s_d[drow * SQR_BK + (((2 * s + h) ^ (drow & 7)) << 4)]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }

  // epilogue: the score by the expression of sq8_gemm_kernel, the predicate, one ballot per register.  Every lane reaches every
  // ballot: a pair outside the problem votes false.
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t col = d0 + wd * 64 + j * 32 + r;
    const bool col_in = col < N;
    const float idb = col_in ? inv_d[col] : 0.f;
    const int64_t word = (int64_t)blockIdx.x * 4 + wd * 2 + j;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int q = q0 + wq * 64 + i * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        bool hit = false;
        if (col_in && q < nq) {
          const float s = ((float)acc[i][j][reg] * inv_q[q]) * idb;
          hit = s >= thr && (!upper || col0 + col > row0 + q);       // false for a NaN score
        }
        const unsigned long long vote = __ballot(hit);
        if (r == 0) mask[(int64_t)q * words + word] = h ? (uint32_t)(vote >> 32) : (uint32_t)vote;
      }
    }
  }
}

// one wave per row: the set bits of its words
__global__ __launch_bounds__(256) void mask_count_kernel(const uint32_t* __restrict__ mask, int64_t words, int64_t rows, int* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const uint32_t* m = mask + r * words;
  int n = 0;
  for (int64_t w = lane; w < words; w += 64) n += __popc(m[w]);
  n = wave_sum(n);
  if (lane == 0) counts[r] = n;
}

// one wave per row walks its words in order, 64 at a time: a lane's first position is the wave prefix of the popcounts, and it
// takes the bits of its word in ascending order.  Hit number k of row r goes to offsets[r] + k where that is below cap.
__global__ __launch_bounds__(256) void mask_emit_kernel(const uint32_t* __restrict__ mask, int64_t words, int64_t rows, int64_t row0, int64_t col0,
                                                        const int64_t* __restrict__ offsets, int64_t cap, int64_t* __restrict__ out_row,
                                                        int64_t* __restrict__ out_col) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const uint32_t* m = mask + r * words;
  int64_t base = offsets[r];
  for (int64_t w0 = 0; w0 < words && base < cap; w0 += 64) {
    uint32_t bits = w0 + lane < words ? m[w0 + lane] : 0u;
    const int pc = __popc(bits);
    int inc = pc;                                        // inclusive prefix over the lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(inc, d, 64);
      if (lane >= d) inc += up;
    }
    int64_t pos = base + (inc - pc);
    const int64_t c_first = col0 + (w0 + lane) * 32;
    while (bits && pos < cap) {
      const int b = __ffs((int)bits) - 1;
      out_row[pos] = row0 + r;
      out_col[pos] = c_first + b;
      bits &= bits - 1;
      ++pos;
    }
    base += __shfl(inc, 63, 64);
  }
}

// val[p] of the emitted pairs: one wave per pair walks both code rows in 16-byte loads on v_dot4 and sums across the wave.  The sum
// is the integer the GEMM held and the expression is the epilogue's, so the value is the one the predicate saw: val[p] >= thr.
__global__ __launch_bounds__(256) void sq8_pair_scores_kernel(const int8_t* __restrict__ qc, const float* __restrict__ inv_q,
                                                              const int8_t* __restrict__ dc, const float* __restrict__ inv_d, int ld,
                                                              const int64_t* __restrict__ prow, const int64_t* __restrict__ pcol, int64_t npairs,
                                                              float* __restrict__ val) {
  const int lane = threadIdx.x & 63;
  const int nch = ld / 16;
  for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < npairs; p += (int64_t)gridDim.x * 4) {
    const int64_t row = prow[p], col = pcol[p];
    const i32x4* q4 = reinterpret_cast<const i32x4*>(qc + row * ld);
    const i32x4* d4 = reinterpret_cast<const i32x4*>(dc + col * ld);
    int a = 0;
    for (int c = lane; c < nch; c += 64) {
      const i32x4 qv = q4[c], dv = d4[c];
      a = __builtin_amdgcn_sdot4(qv.x, dv.x, a, false);
      a = __builtin_amdgcn_sdot4(qv.y, dv.y, a, false);
      a = __builtin_amdgcn_sdot4(qv.z, dv.z, a, false);
      a = __builtin_amdgcn_sdot4(qv.w, dv.w, a, false);
    }
    const int total = wave_sum(a);
    if (lane == 0) val[p] = ((float)total * inv_q[row]) * inv_d[col];
  }
}

// the pieces of the block behind the panel: [0] output entries so far, row counts, row offsets
struct Sq8RangeTail {
  WsPiece<char> panel;
  WsPiece<int64_t> totals;
  WsPiece<int> counts;
  WsPiece<int64_t> offsets;
  size_t bytes;
};
Sq8RangeTail sq8_range_layout(size_t panel_bytes, size_t rows) {
  WsLayout<> l;
  return {l.add<char>(panel_bytes), l.add<int64_t>(2), l.add<int>(rows), l.add<int64_t>(rows), l.bytes()};
}

}  // namespace
}  // namespace pvs

using namespace pvs;

PVS_EXPORT int pvs_sq8_range_dev(pvs_ctx* ctx, const int8_t* d_qcodes, const float* d_inv_q, int64_t nq, const int8_t* d_codes,
                                 const float* d_inv_db, int64_t N, int L, float threshold, int flags, int path, int tile, int64_t capacity,
                                 int64_t* d_row, int64_t* d_col, float* d_val, int64_t* h_total, int64_t* h_stats) {
  PVS_NEED(ctx, "ctx");
  PVS_NEED(h_total, "total");
  if (!std::isfinite(threshold)) PVS_FAIL(PVS_ERR_INVALID, "pvs_sq8_range_dev: the threshold must be finite");
  if (flags & ~PVS_RANGE_UPPER) PVS_FAIL(PVS_ERR_INVALID, "pvs_sq8_range_dev: unknown flags %d", flags);
  if (nq < 0 || N < 0 || nq > 0x7fffffffLL || N > 0x7fffffffLL) PVS_FAIL(PVS_ERR_INVALID, "pvs_sq8_range_dev: need 0 <= nq, N < 2^31");
  if ((flags & PVS_RANGE_UPPER) && nq != N)
    PVS_FAIL(PVS_ERR_INVALID, "pvs_sq8_range_dev: PVS_RANGE_UPPER joins a set with itself (nq = %lld, N = %lld)", (long long)nq, (long long)N);
  if (path < 0 || path > 2) PVS_FAIL(PVS_ERR_INVALID, "pvs_sq8_range_dev: path must be 0, 1 or 2 (got %d)", path);
  if (tile < 0 || tile > 32768) PVS_FAIL(PVS_ERR_INVALID, "pvs_sq8_range_dev: tile must be 0..32768 (got %d)", tile);
  if (capacity < 0 || capacity > PVS_RANGE_MAX_CAPACITY) PVS_FAIL(PVS_ERR_INVALID, "pvs_sq8_range_dev: capacity out of range");
  if (L < 1 || L > SQR_MAX_L) PVS_FAIL(PVS_ERR_INVALID, "pvs_sq8_range_dev: need 1 <= L <= %d (got %d)", SQR_MAX_L, L);
  if (capacity > 0) {
    PVS_NEED(d_row, "row output");
    PVS_NEED(d_col, "col output");
    PVS_NEED(d_val, "val output");
    PVS_ALIGNED(d_row, 8, "row output");
    PVS_ALIGNED(d_col, 8, "col output");
    PVS_ALIGNED(d_val, 4, "val output");
  }
  *h_total = 0;
  if (h_stats) std::fill(h_stats, h_stats + 6, (int64_t)0);
  if (nq == 0 || N == 0) return PVS_OK;
  PVS_NEED(d_qcodes, "qcodes");
  PVS_NEED(d_inv_q, "inv_q");
  PVS_NEED(d_codes, "codes");
  PVS_NEED(d_inv_db, "inv_db");
  PVS_ALIGNED(d_qcodes, 16, "qcodes");
  PVS_ALIGNED(d_codes, 16, "codes");
  PVS_ALIGNED(d_inv_q, 4, "inv_q");
  PVS_ALIGNED(d_inv_db, 4, "inv_db");
  PVS_HIP(hipSetDevice(ctx->device));

  const int ld = PVS_SQ8_LD(L);
  const int upper = flags & PVS_RANGE_UPPER;
  const bool rows = sq8_row_scan(ctx, nq);
  // path 0: the panel is a few rows while the ranking takes the row scan; beyond, the mask (profiles/sq8_range_timing.jsonl)
  if (path == 0) path = rows ? 1 : 2;
  const bool use_mask = path == 2;
  const PanelPlan plan = tile ? PanelPlan{nq, N, std::min<int64_t>(nq, tile), std::min<int64_t>(N, tile)}
                              : (use_mask ? panel_mask(nq, N) : panel_dense(nq, N));
  const Sq8RangeTail lay = sq8_range_layout(use_mask ? panel_mask_bytes(plan) : panel_bytes<float>(plan), (size_t)plan.QT);
  int64_t stats[6] = {path, 0, 0, 0, 0, 0};
  int64_t* totals = nullptr;

  for (int64_t q0 = 0; q0 < nq; q0 += plan.QT) {
    PVS_TRY(panel_query_block_sized<char>(ctx, plan, lay.bytes, q0, [&](int64_t, int64_t qn, int64_t c0, int64_t cn, char* block) -> int {
      if (!totals) {                                     // the first tile of the call: the block keeps its place from here on
        totals = lay.totals(block);
        PVS_HIP(hipMemsetAsync(totals, 0, 16, ctx->stream));
      }
      if (range_tile_below_diagonal(upper, q0, c0, cn)) {
        ++stats[4];
        return PVS_OK;
      }
      ++stats[3];
      int* counts = lay.counts(block);
      int64_t* offsets = lay.offsets(block);
      if (!use_mask) {
        float* panel = reinterpret_cast<float*>(lay.panel(block));
        {
          ScopedTimer tm(ctx, T_GEMM);
          PVS_TRY(launch_sq8_scores(ctx, rows, d_qcodes + q0 * ld, d_inv_q + q0, qn, d_codes + c0 * ld, d_inv_db + c0, cn, ld, panel));
        }
        const RangeSrc src{panel, cn, qn, cn, q0, c0, nullptr, nullptr, 0, threshold, upper};
        return range_compact<false>(ctx, counts, offsets, src, totals, capacity, d_row, d_col, d_val);
      }
      uint32_t* mask = reinterpret_cast<uint32_t*>(lay.panel(block));
      const int64_t words = panel_mask_words(cn);
      {
        ScopedTimer tm(ctx, T_GEMM);
        const dim3 grid((unsigned)((cn + SQR_BD - 1) / SQR_BD), (unsigned)((qn + SQR_BQ - 1) / SQR_BQ));
        hipLaunchKernelGGL(sq8_range_gemm_kernel, grid, dim3(SQR_THREADS), 0, ctx->stream, d_qcodes + q0 * ld, d_inv_q + q0, (int)qn,
                           d_codes + c0 * ld, d_inv_db + c0, cn, ld, threshold, upper, q0, c0, mask, words);
      }
      ScopedTimer tm(ctx, T_TOPK);
      const unsigned grid = (unsigned)((qn + 3) / 4);
      hipLaunchKernelGGL(mask_count_kernel, dim3(grid), dim3(256), 0, ctx->stream, mask, words, qn, counts);
      hipLaunchKernelGGL(range_scan_kernel, dim3(1), dim3(RNG_SCAN_THREADS), 0, ctx->stream, counts, qn, offsets, totals);
      if (capacity > 0)
        hipLaunchKernelGGL(mask_emit_kernel, dim3(grid), dim3(256), 0, ctx->stream, mask, words, qn, q0, c0, offsets, capacity, d_row, d_col);
      PVS_HIP(hipGetLastError());
      return PVS_OK;
    }));
  }
  int64_t total = 0;
  PVS_HIP(hipMemcpyAsync(&total, totals, 8, hipMemcpyDeviceToHost, ctx->stream));
  PVS_HIP(hipStreamSynchronize(ctx->stream));
  const int64_t written = std::min(total, capacity);
  if (use_mask && written > 0) {
    {
      ScopedTimer tm(ctx, T_RESCORE);
      const unsigned grid = (unsigned)std::min<int64_t>((written + 3) / 4, (int64_t)ctx->num_cu * 32);
      hipLaunchKernelGGL(sq8_pair_scores_kernel, dim3(grid), dim3(256), 0, ctx->stream, d_qcodes, d_inv_q, d_codes, d_inv_db, ld, d_row, d_col,
                         written, d_val);
      PVS_HIP(hipGetLastError());
    }
    PVS_HIP(hipStreamSynchronize(ctx->stream));
    stats[2] = written;
  }
  *h_total = total;
  if (h_stats) std::copy(stats, stats + 6, h_stats);
  if (total > capacity)
    PVS_FAIL(PVS_ERR_CAPACITY, "threshold join: %lld pairs do not fit the output of %lld", (long long)total, (long long)capacity);
  return PVS_OK;
}
