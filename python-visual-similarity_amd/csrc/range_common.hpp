// The count / scan / emit compaction of the threshold joins (DESIGN.md sections 24 and 30): what range.hip (float32 rows) and
// sq8_range.hip (int8 code rows) both run over a score panel or a flat candidate list.  No output position is decided by an atomic:
// a row's hits are counted, one workgroup scans the counts from the running total on, and the same walk emits them.
#pragma once
#include "panel_plan.hpp"

namespace pvs {

constexpr int RNG_SCAN_THREADS = 1024;

// What the count and emit kernels walk.  PANEL: val[r * ld + c] is the score of (row0 + r, col0 + c), r < rows, c < cols.
// LIST: entry i = r * ld + c < n of a flat list (lrow[i], lcol[i], val[i]).
struct RangeSrc {
  const float* val;
  int64_t ld, rows, cols, row0, col0;
  const int64_t* lrow;
  const int64_t* lcol;
  int64_t n;
  float thr;
  int upper;
};

template <bool LIST>
__device__ __forceinline__ bool range_pred(const RangeSrc& s, int64_t r, int64_t c, float* v) {
  if (LIST) {
    const int64_t i = r * s.ld + c;
    if (c >= s.ld || i >= s.n) return false;
    *v = s.val[i];
    return *v >= s.thr;                                  // false for NaN
  }
  if (c >= s.cols) return false;
  *v = s.val[r * s.ld + c];
  return *v >= s.thr && (!s.upper || s.col0 + c > s.row0 + r);
}

// one wave per row: the number of hits of the row
template <bool LIST>
__global__ __launch_bounds__(256) void range_count_kernel(RangeSrc s, int* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= s.rows) return;
  const int64_t width = LIST ? s.ld : s.cols;
  int n = 0;
  for (int64_t c0 = 0; c0 < width; c0 += 64) {
    float v;
    n += __popcll(__ballot(range_pred<LIST>(s, r, c0 + lane, &v)));
  }
  if (lane == 0) counts[r] = n;
}

// one workgroup: offsets[r] = *total + (counts[0] + ... + counts[r - 1]), then *total += the sum.  Launches are serial in the stream,
// so the running total needs no atomic.  Static: each unit that includes this file holds its own copy.
static __global__ __launch_bounds__(RNG_SCAN_THREADS) void range_scan_kernel(const int* __restrict__ counts, int64_t n,
                                                                             int64_t* __restrict__ offsets, int64_t* __restrict__ total) {
  __shared__ int64_t part[RNG_SCAN_THREADS];
  const int tid = threadIdx.x;
  const int64_t base = *total;
  const int64_t per = (n + RNG_SCAN_THREADS - 1) / RNG_SCAN_THREADS;
  const int64_t lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
  int64_t sum = 0;
  for (int64_t i = lo; i < hi; ++i) sum += counts[i];
  part[tid] = sum;
  __syncthreads();
  for (int d = 1; d < RNG_SCAN_THREADS; d <<= 1) {       // inclusive scan of the per-thread sums
    const int64_t add = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  int64_t run = base + part[tid] - sum;
  for (int64_t i = lo; i < hi; ++i) {
    offsets[i] = run;
    run += counts[i];
  }
  if (tid == RNG_SCAN_THREADS - 1) *total = base + part[tid];
}

// the same walk as the count: hit number k of row r goes to offsets[r] + k where that is below cap
template <bool LIST>
__global__ __launch_bounds__(256) void range_emit_kernel(RangeSrc s, const int64_t* __restrict__ offsets, int64_t cap,
                                                         int64_t* __restrict__ out_row, int64_t* __restrict__ out_col,
                                                         float* __restrict__ out_val) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= s.rows) return;
  const int64_t width = LIST ? s.ld : s.cols;
  int64_t base = offsets[r];
  for (int64_t c0 = 0; c0 < width && base < cap; c0 += 64) {
    float v = 0.f;
    const bool pred = range_pred<LIST>(s, r, c0 + lane, &v);
    const unsigned long long mask = __ballot(pred);
    if (pred) {
      const int64_t pos = base + __popcll(mask & ((1ull << lane) - 1ull));
      if (pos < cap) {
        const int64_t i = r * s.ld + c0 + lane;
        out_row[pos] = LIST ? s.lrow[i] : s.row0 + r;
        out_col[pos] = LIST ? s.lcol[i] : s.col0 + c0 + lane;
        if (out_val) out_val[pos] = v;
      }
    }
    base += __popcll(mask);
  }
}

// count -> scan from *total on -> emit (cap == 0: count only).  counts and offsets hold src.rows entries.
template <bool LIST>
inline int range_compact(pvs_ctx* ctx, int* counts, int64_t* offsets, const RangeSrc& src, int64_t* total, int64_t cap, int64_t* o_row,
                         int64_t* o_col, float* o_val) {
  ScopedTimer tm(ctx, T_TOPK);
  const unsigned grid = (unsigned)((src.rows + 3) / 4);
  hipLaunchKernelGGL(range_count_kernel<LIST>, dim3(grid), dim3(256), 0, ctx->stream, src, counts);
  hipLaunchKernelGGL(range_scan_kernel, dim3(1), dim3(RNG_SCAN_THREADS), 0, ctx->stream, counts, src.rows, offsets, total);
  if (cap > 0) hipLaunchKernelGGL(range_emit_kernel<LIST>, dim3(grid), dim3(256), 0, ctx->stream, src, offsets, cap, o_row, o_col, o_val);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

// a tile of the self-join that lies wholly on or below the diagonal holds no pair j > i
inline bool range_tile_below_diagonal(int upper, int64_t q0, int64_t c0, int64_t cn) { return upper && c0 + cn <= q0 + 1; }

}  // namespace pvs
