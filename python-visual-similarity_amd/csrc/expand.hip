// Query expansion and database-side augmentation: out[i] = w_self[i] self[i] + sum_j w[i][j] X[idx[i][j]],
// whole encoding rows gathered by index and summed in list order.  The definition (include/pvsim.h) rounds every multiply and every
// add separately, so this unit is compiled with -ffp-contract=off, like pq.hip.
//
// It is a bandwidth kernel: per output element it does r + 1 multiply-add pairs on r + 1 loaded elements.  One workgroup owns one
// output row and one chunk of COMBINE_CHUNK_BYTES of its columns; a lane owns 16 bytes of columns at a time (float4 / double2), or one
// element where the rows are not 16-byte aligned.  The list entries of the row are the same for every lane of the workgroup: they are
// read through the row index of the workgroup (blockIdx.x), so they sit in scalar registers, and skipping a slot is a uniform branch.
// The list is walked in batches of COMBINE_U slots: the row loads of a batch are all issued before the first of them is used, and the
// adds then run in ascending j, which keeps the summation order of the definition.
#include <algorithm>

#include "common.hpp"

namespace pvs {

constexpr int COMBINE_THREADS = 256;
constexpr int COMBINE_U = PVS_COMBINE_BATCH;              // list slots whose row loads are in flight together
constexpr int COMBINE_CHUNK_BYTES = PVS_COMBINE_CHUNK_BYTES;   // columns of one workgroup, in bytes of a row

// a lane's item: W elements of T that travel as one load / store
template <typename T, int W>
struct Item {
  T e[W];
};
template <>
struct alignas(16) Item<float, 4> {
  float e[4];
};
template <>
struct alignas(16) Item<double, 2> {
  double e[2];
};

__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ double mul_rn(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double add_rn(double a, double b) { return __dadd_rn(a, b); }

template <typename T, int W>
__device__ __forceinline__ void axpy_item(Item<T, W>& acc, T w, const Item<T, W>& v) {
#pragma unroll
  for (int e = 0; e < W; ++e) acc.e[e] = add_rn(acc.e[e], mul_rn(w, v.e[e]));
}

// grid: x = output row (fastest), y = column chunk.  `self` and `out` may be the same array (each item is read, then written, by the
// same lane), so neither is __restrict__; `out` does not overlap X (checked on the host).
template <typename T, int W>
__global__ __launch_bounds__(COMBINE_THREADS) void combine_rows_kernel(const T* __restrict__ X, int64_t N, int64_t L, const T* self,
                                                                       const T* __restrict__ w_self, const int64_t* __restrict__ idx,
                                                                       const T* __restrict__ w, int r, int64_t row0, int64_t chunk0,
                                                                       T* out) {
  using V = Item<T, W>;
  constexpr int64_t CHUNK = COMBINE_CHUNK_BYTES / (int64_t)sizeof(T);   // columns
  const int64_t row = row0 + blockIdx.x;
  const int64_t col0 = (chunk0 + blockIdx.y) * CHUNK;
  const int64_t col1 = col0 + CHUNK < L ? col0 + CHUNK : L;
  const int64_t* li = idx + row * r;       // wave-uniform: scalar loads
  const T* lw = w + row * r;
  const T ws = (self && w_self) ? w_self[row] : (T)1;

  for (int64_t col = col0 + (int64_t)threadIdx.x * W; col < col1; col += (int64_t)COMBINE_THREADS * W) {   // W divides L on the 16-byte path
    V acc;
#pragma unroll
    for (int e = 0; e < W; ++e) acc.e[e] = (T)0;
    if (self) axpy_item<T, W>(acc, ws, *reinterpret_cast<const V*>(self + row * L + col));
    int j = 0;
    for (; j + COMBINE_U <= r; j += COMBINE_U) {
      int64_t c[COMBINE_U];
      bool all = true;
#pragma unroll
      for (int u = 0; u < COMBINE_U; ++u) {
        c[u] = li[j + u];
        all = all && c[u] >= 0 && c[u] < N;
      }
      if (all) {                            // the usual case: COMBINE_U loads in flight, then the adds in order
        V v[COMBINE_U];
#pragma unroll
        for (int u = 0; u < COMBINE_U; ++u) v[u] = *reinterpret_cast<const V*>(X + c[u] * L + col);
#pragma unroll
        for (int u = 0; u < COMBINE_U; ++u) axpy_item<T, W>(acc, lw[j + u], v[u]);
      } else {                              // a batch with a skipped slot: slot by slot
        for (int u = 0; u < COMBINE_U; ++u)
          if (c[u] >= 0 && c[u] < N) axpy_item<T, W>(acc, lw[j + u], *reinterpret_cast<const V*>(X + c[u] * L + col));
      }
    }
    for (; j < r; ++j) {                    // the last r % COMBINE_U slots
      const int64_t c = li[j];
      if (c >= 0 && c < N) axpy_item<T, W>(acc, lw[j], *reinterpret_cast<const V*>(X + c * L + col));
    }
    *reinterpret_cast<V*>(out + row * L + col) = acc;
  }
}

template <typename T>
static int launch_combine(pvs_ctx* ctx, const T* X, int64_t N, int64_t L, const T* self, const T* w_self, const int64_t* idx, const T* w,
                          int64_t n, int r, T* out) {
  constexpr int W = 16 / (int)sizeof(T);
  auto aligned16 = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
  // rows of L elements start on 16-byte boundaries only if their byte length is a multiple of 16 and the matrices do
  const bool vec = L % W == 0 && aligned16(X) && aligned16(out) && aligned16(self);
  constexpr int64_t CHUNK = COMBINE_CHUNK_BYTES / (int64_t)sizeof(T);
  const int64_t chunks = (L + CHUNK - 1) / CHUNK;
  constexpr int64_t MAX_X = 1 << 23, MAX_Y = 65535;   // grid.x * 256 threads stays below 2^32
  ScopedTimer t(ctx, T_MISC);
  for (int64_t c0 = 0; c0 < chunks; c0 += MAX_Y)
    for (int64_t r0 = 0; r0 < n; r0 += MAX_X) {
      const dim3 grid((unsigned)std::min(MAX_X, n - r0), (unsigned)std::min(MAX_Y, chunks - c0));
      if (vec)
        hipLaunchKernelGGL((combine_rows_kernel<T, W>), grid, dim3(COMBINE_THREADS), 0, ctx->stream, X, N, L, self, w_self, idx, w, r, r0,
                           c0, out);
      else
        hipLaunchKernelGGL((combine_rows_kernel<T, 1>), grid, dim3(COMBINE_THREADS), 0, ctx->stream, X, N, L, self, w_self, idx, w, r, r0,
                           c0, out);
      PVS_HIP(hipGetLastError());
    }
  return PVS_OK;
}

}  // namespace pvs

using namespace pvs;

PVS_EXPORT int pvs_combine_rows_dev(pvs_ctx* ctx, const void* d_X, int64_t N, int64_t L, int is_f64, const void* d_self,
                                    const void* d_w_self, const int64_t* d_idx, const void* d_w, int64_t n, int r, void* d_out) {
  if (!ctx) PVS_FAIL(PVS_ERR_INVALID, "pvs_combine_rows_dev: null ctx");
  if (L < 1 || N < 0 || n < 0 || r < 0)
    PVS_FAIL(PVS_ERR_INVALID, "pvs_combine_rows_dev: need L >= 1, N >= 0, n >= 0, r >= 0 (got L=%lld, N=%lld, n=%lld, r=%d)", (long long)L,
             (long long)N, (long long)n, r);
  const int64_t sz = is_f64 ? 8 : 4;
  if (L > ((int64_t)1 << 40) || N > ((int64_t)1 << 40) || n > ((int64_t)1 << 40) || (double)L * (double)std::max(N, n) * sz > 9e18)
    PVS_FAIL(PVS_ERR_INVALID, "pvs_combine_rows_dev: the matrices are too large");
  if (n == 0) return PVS_OK;
  if (!d_out) PVS_FAIL(PVS_ERR_INVALID, "pvs_combine_rows_dev: null out");
  if (r > 0 && (!d_idx || !d_w)) PVS_FAIL(PVS_ERR_INVALID, "pvs_combine_rows_dev: null idx or w with r = %d", r);
  if (r > 0 && N > 0 && !d_X) PVS_FAIL(PVS_ERR_INVALID, "pvs_combine_rows_dev: null X");
  const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_out), o1 = o0 + (uintptr_t)(n * L * sz);
  const uintptr_t x0 = reinterpret_cast<uintptr_t>(d_X), x1 = x0 + (uintptr_t)(N * L * sz);
  if (d_X && N > 0 && o0 < x1 && x0 < o1) PVS_FAIL(PVS_ERR_INVALID, "pvs_combine_rows_dev: out overlaps X");
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_self);
  if (d_self && s0 != o0 && o0 < s0 + (uintptr_t)(n * L * sz) && s0 < o1)
    PVS_FAIL(PVS_ERR_INVALID, "pvs_combine_rows_dev: out overlaps self without being self");
  for (const void* p : {d_X, d_self, d_w_self, d_w, (const void*)d_out})
    if (reinterpret_cast<uintptr_t>(p) % sz) PVS_FAIL(PVS_ERR_INVALID, "pvs_combine_rows_dev: a matrix is not aligned to its element size");
  if (reinterpret_cast<uintptr_t>(d_idx) % 8) PVS_FAIL(PVS_ERR_INVALID, "pvs_combine_rows_dev: idx must be 8-byte aligned");
  PVS_HIP(hipSetDevice(ctx->device));
  if (is_f64)
    return launch_combine<double>(ctx, (const double*)d_X, N, L, (const double*)d_self, (const double*)d_w_self, d_idx, (const double*)d_w,
                                  n, r, (double*)d_out);
  return launch_combine<float>(ctx, (const float*)d_X, N, L, (const float*)d_self, (const float*)d_w_self, d_idx, (const float*)d_w, n, r,
                               (float*)d_out);
}
