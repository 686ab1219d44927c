// The stable LSD radix sort on keys below 65536 that asmk_update.hip (the inversion) and ivf_sq8.hip (section
// 28: the probes grouped by list) share, with the exclusive scan of int32 counts under it.  Integer counting and data movement only.
// The only atomics are adds to a digit histogram in LDS, whose sums do not depend on the order of arrival; every position comes from
// a scan or a ballot.  No kernel waits for another workgroup: the passes are separate launches ordered by the stream.
//
// The sort moves 8-byte items, (key << 32) | source slot, with key in [0, K), or K for a slot that is no entry: K's digit is 256 in
// every pass, behind every key.  One pass serves K <= 256, two serve K <= 65536.
// The kernels are static: each unit that includes this file holds its own copies, as with the templates of list_common.hpp.
#pragma once
#include <algorithm>

#include "list_common.hpp"

namespace pvs {

constexpr int AU_THREADS = 256;
constexpr int AU_WAVES = AU_THREADS / WAVE;
constexpr int AU_BINS = 257;                              // 256 digits and the one behind them
constexpr int AU_SCAN_PER = 8;
constexpr int AU_SCAN_BLOCK = AU_THREADS * AU_SCAN_PER;   // counts one workgroup scans

__device__ __forceinline__ int au_digit(uint32_t key, int K, int shift) { return key >= (uint32_t)K ? 256 : (int)((key >> shift) & 0xffu); }

// ------------------------------------------------------------------------------------------------- exclusive scan of int32 counts
static __global__ __launch_bounds__(AU_THREADS) void au_scan_sums_kernel(const int32_t* __restrict__ data, int64_t M, int32_t* __restrict__ partials) {
  __shared__ int tmp[AU_WAVES];
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * AU_SCAN_BLOCK + (int64_t)tid * AU_SCAN_PER;
  int mine = 0;
#pragma unroll
  for (int e = 0; e < AU_SCAN_PER; ++e) mine += i0 + e < M ? data[i0 + e] : 0;
  const int incl = block_incl_scan(mine, tmp, tid & 63, tid >> 6);
  if (tid == AU_THREADS - 1) partials[blockIdx.x] = incl;
}

// one workgroup: the partials become their exclusive prefixes, AU_THREADS at a time with a carry
static __global__ __launch_bounds__(AU_THREADS) void au_scan_partials_kernel(int32_t* __restrict__ partials, int nb) {
  __shared__ int tmp[AU_WAVES];
  __shared__ int chunk_total;
  const int tid = threadIdx.x;
  int carry = 0;
  for (int base = 0; base < nb; base += AU_THREADS) {
    const int v = base + tid < nb ? partials[base + tid] : 0;
    const int incl = block_incl_scan(v, tmp, tid & 63, tid >> 6);
    if (base + tid < nb) partials[base + tid] = carry + incl - v;
    if (tid == AU_THREADS - 1) chunk_total = incl;
    __syncthreads();
    carry += chunk_total;
    __syncthreads();
  }
}

static __global__ __launch_bounds__(AU_THREADS) void au_scan_apply_kernel(int32_t* __restrict__ data, int64_t M, const int32_t* __restrict__ partials) {
  __shared__ int tmp[AU_WAVES];
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * AU_SCAN_BLOCK + (int64_t)tid * AU_SCAN_PER;
  int v[AU_SCAN_PER], mine = 0;
#pragma unroll
  for (int e = 0; e < AU_SCAN_PER; ++e) {
    v[e] = i0 + e < M ? data[i0 + e] : 0;
    mine += v[e];
  }
  const int incl = block_incl_scan(mine, tmp, tid & 63, tid >> 6);
  int run = partials[blockIdx.x] + incl - mine;
#pragma unroll
  for (int e = 0; e < AU_SCAN_PER; ++e) {
    if (i0 + e < M) data[i0 + e] = run;
    run += v[e];
  }
}

// data[0 .. M) -> its exclusive prefix sums in place (the total stays below 2^31); partials: int32 [ceil(M / AU_SCAN_BLOCK)]
static int au_launch_scan(pvs_ctx* ctx, int32_t* data, int64_t M, int32_t* partials) {
  const int64_t nb = (M + AU_SCAN_BLOCK - 1) / AU_SCAN_BLOCK;
  hipLaunchKernelGGL(au_scan_sums_kernel, dim3((unsigned)nb), dim3(AU_THREADS), 0, ctx->stream, data, M, partials);
  hipLaunchKernelGGL(au_scan_partials_kernel, dim3(1), dim3(AU_THREADS), 0, ctx->stream, partials, (int)nb);
  hipLaunchKernelGGL(au_scan_apply_kernel, dim3((unsigned)nb), dim3(AU_THREADS), 0, ctx->stream, data, M, partials);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

// ------------------------------------------------------------------------------------------------- the passes
// counts[d][tile] = items of the tile whose digit is d
static __global__ __launch_bounds__(AU_THREADS) void au_digit_count_kernel(const uint64_t* __restrict__ items, int64_t total, int tile, int shift,
                                                                           int K, int ntiles, int32_t* __restrict__ counts) {
  __shared__ int hist[AU_BINS];
  const int tid = threadIdx.x;
  for (int d = tid; d < AU_BINS; d += AU_THREADS) hist[d] = 0;
  __syncthreads();
  const int64_t j0 = (int64_t)blockIdx.x * tile;
  for (int c = 0; c < tile; c += AU_THREADS) {
    const int64_t j = j0 + c + tid;
    if (j < total) atomicAdd(&hist[au_digit((uint32_t)(items[j] >> 32), K, shift)], 1);   // a count: the sum does not depend on the order
  }
  __syncthreads();
  for (int d = tid; d < AU_BINS; d += AU_THREADS) counts[(int64_t)d * ntiles + blockIdx.x] = hist[d];
}

// base[d][tile]: where the tile's first item of digit d goes.  The tile is walked 256 items at a time in order; inside a step a lane's
// rank among the lanes of its wave with the same digit comes from nine ballots, the waves before it from their counts in LDS.
static __global__ __launch_bounds__(AU_THREADS) void au_scatter_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, int64_t total,
                                                                       int tile, int shift, int K, int ntiles, const int32_t* __restrict__ base) {
  __shared__ int running[AU_BINS];
  __shared__ int wcnt[AU_WAVES][AU_BINS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int d = tid; d < AU_BINS; d += AU_THREADS) running[d] = base[(int64_t)d * ntiles + blockIdx.x];
  const int64_t j0 = (int64_t)blockIdx.x * tile;
  for (int c = 0; c < tile; c += AU_THREADS) {
    if (j0 + c >= total) break;                       // the same for every lane of the workgroup
    const int64_t j = j0 + c + tid;
    const bool valid = j < total;
    const uint64_t item = valid ? in[j] : 0;
    const int d = valid ? au_digit((uint32_t)(item >> 32), K, shift) : 0;
    for (int t = tid; t < AU_WAVES * AU_BINS; t += AU_THREADS) (&wcnt[0][0])[t] = 0;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 9; ++b) {
      const bool bit = (d >> b) & 1;
      const unsigned long long bal = __ballot(bit);
      peers &= bit ? bal : ~bal;
    }
    const int rank = __popcll(peers & ((1ull << lane) - 1ull)), cnt = __popcll(peers);
    __syncthreads();
    if (valid && rank == 0) wcnt[wave][d] = cnt;
    __syncthreads();
    if (valid) {
      int before = 0;
      for (int w = 0; w < wave; ++w) before += wcnt[w][d];
      const int64_t to = (int64_t)running[d] + before + rank;
      if (to >= 0 && to < total) out[to] = item;
    }
    __syncthreads();
    for (int dd = tid; dd < AU_BINS; dd += AU_THREADS) {
      int sum = 0;
#pragma unroll
      for (int w = 0; w < AU_WAVES; ++w) sum += wcnt[w][dd];
      running[dd] += sum;
    }
    __syncthreads();
  }
}

// off[w] = the first sorted item whose key is at least w, w = 0 .. K (key K: the slots that are no entries)
template <class T>
__global__ __launch_bounds__(AU_THREADS) void au_key_off_kernel(const uint64_t* __restrict__ items, int64_t total, int K, T* __restrict__ off) {
  const int w = blockIdx.x * AU_THREADS + threadIdx.x;
  if (w > K) return;
  int64_t lo = 0, hi = total;
  for (int it = 0; it < 32; ++it) {
    if (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((uint32_t)(items[mid] >> 32) < (uint32_t)w) lo = mid + 1;
      else hi = mid;
    }
  }
  off[w] = (T)lo;
}

// The `total` items of `a` sorted by key, stably, in tiles of `tile` items (ntiles of them): the passes swap a and b, *sorted is the
// array that holds the result.  counts: int32 [AU_BINS * ntiles]; partials: int32 [ceil(AU_BINS * ntiles / AU_SCAN_BLOCK)].
static int au_launch_sort(pvs_ctx* ctx, uint64_t* a, uint64_t* b, int64_t total, int64_t tile, int64_t ntiles, int K, int32_t* counts,
                          int32_t* partials, uint64_t** sorted) {
  const int64_t ncounts = (int64_t)AU_BINS * ntiles;
  const int passes = K <= 256 ? 1 : 2;
  for (int p = 0; p < passes; ++p) {
    hipLaunchKernelGGL(au_digit_count_kernel, dim3((unsigned)ntiles), dim3(AU_THREADS), 0, ctx->stream, a, total, (int)tile, 8 * p, K, (int)ntiles,
                       counts);
    PVS_HIP(hipGetLastError());
    PVS_TRY(au_launch_scan(ctx, counts, ncounts, partials));
    hipLaunchKernelGGL(au_scatter_kernel, dim3((unsigned)ntiles), dim3(AU_THREADS), 0, ctx->stream, a, b, total, (int)tile, 8 * p, K, (int)ntiles,
                       counts);
    PVS_HIP(hipGetLastError());
    std::swap(a, b);
  }
  *sorted = a;
  return PVS_OK;
}

}  // namespace pvs
