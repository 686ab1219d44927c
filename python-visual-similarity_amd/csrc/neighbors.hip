// Exact Euclidean neighbour search and the sparse products of the spectral embedding (image clustering).
//
// The reference clusters encodings with sklearn (pyvisim/_utils.py:128-162): SpectralClustering builds kneighbors_graph(X, 10,
// include_self=True), DBSCAN asks radius_neighbors(X, eps).  Both are brute-force pairwise reductions in sklearn
// (sklearn/metrics/_pairwise_distances_reduction), float32 rows upcast to float64, and the value they rank or threshold is
//     d(i, j) = max(0, (|x_i|^2 + (-2 x_i . y_j)) + |y_j|^2)        (float64)
// Lists here use the same value and the total order (d ascending, index ascending): sklearn's heap rejects a value equal to its
// current worst, so among equal distances at the k-th place the lower index stays; a tie INSIDE the list is ordered by sklearn's
// unstable final sort, which these lists do not copy (tests allow a swap only between entries whose f64 gap is below the
// rounding of the dot products).
//
// k nearest neighbours, float32 rows ("prefilter with a proven margin, then re-score exactly", as filter.hip):
//   1. score panels (8192 queries x 32768 rows) with the exact f32 MFMA GEMM (gemm_mfma.hpp, unit inverse norms: raw x . y),
//   2. turn a panel into the approximate key  a(i, j) = x_i . y_j - fl32(|y_j|^2 / 2)   (larger = nearer; |x_i|^2 is constant
//      per row), keep the running approximate k best per query with the top-k kernels (topk.hip, merged across panels),
//   3. keep every column whose key is >= (the running approximate k-th best) - 2 E_i: the running k-th best can only be lower
//      than the final one, so the kept set is a superset of the exact k nearest, ties included,
//   4. re-score the kept pairs in float64 (a product of two f32 values is exact in f64; the sums run in f64) and rank them.
//   Error bound of a key (u = 2^-24, bounds taken with 2u to cover the rounding mode), for |y| <= ymax over the database:
//     f32 GEMM: chains of 1024 fma + L/1024 chain sums         <= (1025 + L/1024) 2u |x_i| ymax
//               (the generic tile kernel, L % 4 != 0 or unaligned rows: one chain of L fma <= (L + 1) 2u |x_i| ymax)
//     fl32(|y|^2 / 2) and the subtraction                        <= 2u (ymax^2 + |x_i| ymax)
//     products / partial sums flushed below the f32 normal range <= L 2^-124
//     the f64 re-score differs from exact arithmetic by          <= (L + 4) 2^-53 (|x_i|^2 + ymax^2 + 2 |x_i| ymax) / 2
//   E_i is their sum times 1.001; the margin is 2 E_i.  Rows whose largest norm^2 exceeds 2^100 (the f32 keys could overflow),
//   non-finite rows, k > 256, and query lists that overflow their candidate slots take a full float64 pass instead.
// k nearest neighbours, float64 rows (and the full float64 pass): f64 MFMA GEMM (gemm_f64.hpp) over complete rows, the panel
//   turned into -d(i, j) and ranked by the f64 ranking kernels of topk.hip; the columns within 2 E of the k-th are re-scored in
//   the same fixed order as above and ranked (E: the f64 rounding of the GEMM and of the re-score, see nb_key_error), so
//   identical rows tie exactly in both paths.  A query with more than its slots of candidates keeps the GEMM's ranking.
// radius neighbours: every pair is decided on the float64 value d(i, j) <= r (f32 rows converted exactly to f64 first), two
//   passes (count, then fill in index order) into CSR.
// CSR SpMM, float64: Y = alpha S X + X diag(beta) + gamma Z, one wave per row of S; the block operations of the eigensolver.
#include <algorithm>
#include <cmath>
#include <vector>

#include "panel_plan.hpp"

namespace pvs {

constexpr int NB_CAP_MAX = 1024;   // candidate slots per query (filtered kNN)
constexpr int NB_K_MAX = 256;      // largest k of the filtered kNN

// ---- |row|^2 in float64, one workgroup per row, fixed summation order
template <typename T>
__global__ __launch_bounds__(256) void nb_sqnorm_kernel(const T* __restrict__ x, int64_t rows, int64_t L, double* __restrict__ out) {
  __shared__ double red[4];
  const int64_t r = blockIdx.x;
  const T* xr = x + r * L;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < L; i += 256) {
    const double v = (double)xr[i];
    s = fma(v, v, s);
  }
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[r] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- largest value of a float64 array (one workgroup); NaN propagates as +inf
__global__ __launch_bounds__(256) void nb_max_kernel(const double* __restrict__ a, int64_t n, double* __restrict__ out) {
  __shared__ double red[4];
  double m = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const double v = a[i];
    m = (v == v) ? fmax(m, v) : INFINITY;
  }
  for (int s = 32; s >= 1; s >>= 1) m = fmax(m, __shfl_xor(m, s, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

__global__ __launch_bounds__(256) void nb_half_f32_kernel(const double* __restrict__ yn, int64_t n, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (float)(0.5 * yn[i]);
}

__global__ __launch_bounds__(256) void nb_f32_to_f64_kernel(const float* __restrict__ a, int64_t n, double* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = (double)a[i];
}

// ---- f32 panel of raw dot products -> approximate key  s - fl32(|y|^2 / 2)  (in place)
__global__ __launch_bounds__(256) void nb_key_f32_kernel(float* __restrict__ S, int64_t qn, int64_t cn, int64_t ld,
                                                         const float* __restrict__ hy) {
  const int64_t n = qn * cn;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / cn, j = e - i * cn;
    S[i * ld + j] = S[i * ld + j] - hy[j];
  }
}

// ---- f64 panel of raw dot products -> -d(i, j)  (in place; ranked descending by rank_f64)
__device__ __forceinline__ double nb_dist(double xn, double dot, double yn) { return fmax(0.0, (xn + (-2.0 * dot)) + yn); }

__global__ __launch_bounds__(256) void nb_negdist_f64_kernel(double* __restrict__ S, int64_t qn, int64_t cn, int64_t ld,
                                                             const double* __restrict__ xn, const double* __restrict__ yn) {
  const int64_t n = qn * cn;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / cn, j = e - i * cn;
    S[i * ld + j] = -nb_dist(xn[i], S[i * ld + j], yn[j]);
  }
}

__global__ __launch_bounds__(256) void nb_negate_kernel(const double* __restrict__ a, int64_t n, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = -a[i];
}

// ---- candidates of a query: columns with key >= (running approximate k-th best) - 2 E_q, in column order; one wave per query.
// float panels hold x.y - fl32(|y|^2 / 2) (f32 GEMM), double panels hold -d (f64 GEMM; E = the f64 rounding of the GEMM and of the
// re-score, both at most (L + 4) 2^-53 (|x|^2 + ymax^2 + 2 |x| ymax) to first order).
// count[q] may exceed cap (overflow: float panels redo everything in float64, double panels keep the GEMM's ranking).
// chain: the longest chain of f32 roundings a score goes through -- 1025 + L/1024 on the MFMA kernel (chains of 1024 fma, then
// the chain sums), L + 1 on the generic tile kernel that launch_cosine_f32 uses for L % 4 != 0 or unaligned rows (one fma chain)
template <typename T>
__device__ __forceinline__ double nb_key_error(double xnq, double ym2, int64_t L, double chain) {
  const double xq = sqrt(xnq), ym = sqrt(ym2), Ld = (double)L;
  const double f64 = (Ld + 4.0) * 0x1p-53 * (xnq + ym2 + 2.0 * xq * ym);
  if (sizeof(T) == 8) return 2.0 * f64 * 1.001;
  const double u2 = 1.1920928955078125e-7;   // 2^-23
  return (chain * u2 * xq * ym + u2 * (ym2 + xq * ym) + Ld * 0x1p-124 + 0.5 * f64) * 1.001;
}

template <typename T>
__global__ __launch_bounds__(256) void nb_collect_kernel(const T* __restrict__ S, int64_t qn, int64_t cn, int64_t ld,
                                                         const T* __restrict__ aval, int k, const double* __restrict__ xn,
                                                         const double* __restrict__ ymax2, int64_t L, double chain, int cap,
                                                         int64_t col_offset, int first, int64_t* __restrict__ cand,
                                                         int* __restrict__ count, unsigned long long* __restrict__ overflow) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= qn) return;
  const double E = nb_key_error<T>(xn[q], ymax2[0], L, chain);
  const T a_k = aval[q * k + k - 1];
  const T thr = (a_k == (T)-INFINITY) ? (T)-INFINITY : (T)((double)a_k - 2.0 * E);
  int base = first ? 0 : count[q];
  const int base0 = base;
  for (int64_t c0 = 0; c0 < cn; c0 += 64) {
    const int64_t c = c0 + lane;
    const bool pred = c < cn && S[q * ld + c] >= thr;
    const unsigned long long mask = __ballot(pred);
    if (pred) {
      const int slot = base + __popcll(mask & ((1ull << lane) - 1ull));
      if (slot < cap) cand[q * cap + slot] = col_offset + c;
    }
    base += __popcll(mask);
  }
  if (lane == 0) {
    count[q] = base;
    if (base > cap && base0 <= cap) atomicAdd(overflow, 1ull);
  }
}

// ---- exact re-score of the kept pairs: one wave per (query, slot), f64 sums (of the exact f32 products for float rows) in one
// fixed order, so the value depends on the two rows alone (identical rows tie exactly, whatever tile they sat in)
template <typename T>
__global__ __launch_bounds__(256) void nb_rescore_kernel(const T* __restrict__ Q, const T* __restrict__ X, int64_t qn, int64_t L,
                                                         const int64_t* __restrict__ cand, const int* __restrict__ count, int cap,
                                                         const double* __restrict__ xn, const double* __restrict__ yn,
                                                         double* __restrict__ key) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t q = w / cap;
  const int slot = (int)(w - q * cap);
  if (q >= qn || slot >= min(count[q], cap)) return;
  const int64_t j = cand[q * cap + slot];
  const T* a = Q + q * L;
  const T* b = X + j * L;
  double s = 0.0;
  for (int64_t i = lane; i < L; i += 64) s = fma((double)a[i], (double)b[i], s);
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  if (lane == 0) key[q * cap + slot] = nb_dist(xn[q], s, yn[j]);
}

// ---- rank the re-scored candidates of a query: position = number of candidates that are strictly better
__global__ __launch_bounds__(256) void nb_rank_kernel(const int64_t* __restrict__ cand, const double* __restrict__ key,
                                                      const int* __restrict__ count, int cap, int k, const int64_t* __restrict__ aidx,
                                                      const double* __restrict__ aval, int64_t* __restrict__ out_idx,
                                                      double* __restrict__ out_d) {
  __shared__ double ks[NB_CAP_MAX];
  __shared__ int64_t is[NB_CAP_MAX];
  const int64_t q = blockIdx.x;
  if (count[q] > cap) {               // (float panels: the call redoes everything; double panels: the GEMM's ranking of -d)
    if (aidx)
      for (int t = threadIdx.x; t < k; t += 256) {
        out_idx[q * k + t] = aidx[q * k + t];
        out_d[q * k + t] = -aval[q * k + t];
      }
    return;
  }
  const int c = count[q];
  for (int t = threadIdx.x; t < c; t += 256) {
    ks[t] = key[q * cap + t];
    is[t] = cand[q * cap + t];
  }
  __syncthreads();
  for (int t = threadIdx.x; t < c; t += 256) {
    const double v = ks[t];
    const int64_t id = is[t];
    int pos = 0;
    for (int o = 0; o < c; ++o) pos += (ks[o] < v || (ks[o] == v && is[o] < id)) ? 1 : 0;
    if (pos < k) {
      out_idx[q * k + pos] = id;
      out_d[q * k + pos] = v;
    }
  }
}

// ---- radius: per query the number of rows with d <= r (pass 1) / their indices in index order (pass 2); one wave per query
template <bool FILL>
__global__ __launch_bounds__(256) void nb_radius_kernel(const double* __restrict__ S, int64_t qn, int64_t cn, int64_t ld,
                                                        const double* __restrict__ xn, const double* __restrict__ yn, double r,
                                                        int64_t col_offset, int64_t* __restrict__ cursor,
                                                        int64_t* __restrict__ indices, double* __restrict__ sqd) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= qn) return;
  int64_t base = cursor[q];
  for (int64_t c0 = 0; c0 < cn; c0 += 64) {
    const int64_t c = c0 + lane;
    double d = 0.0;
    bool pred = false;
    if (c < cn) {
      d = nb_dist(xn[q], S[q * ld + c], yn[col_offset + c]);
      pred = d <= r;
    }
    const unsigned long long mask = __ballot(pred);
    if (FILL && pred) {
      const int64_t p = base + __popcll(mask & ((1ull << lane) - 1ull));
      indices[p] = col_offset + c;
      if (sqd) sqd[p] = d;
    }
    base += __popcll(mask);
  }
  if (lane == 0) cursor[q] = base;
}

__global__ __launch_bounds__(256) void nb_copy_i64_kernel(const int64_t* __restrict__ a, int64_t n, int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = a[i];
}

// ---- Y = alpha S X + X diag(beta) + gamma Z; one wave per row, lanes over the m columns
__global__ __launch_bounds__(256) void nb_spmm_kernel(int64_t n, const int64_t* __restrict__ indptr, const int64_t* __restrict__ indices,
                                                      const double* __restrict__ data, const double* __restrict__ X, int m, double alpha,
                                                      const double* __restrict__ beta, const double* __restrict__ Z, double gamma,
                                                      double* __restrict__ Y) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int64_t p0 = indptr[i], p1 = indptr[i + 1];
  for (int c = lane; c < m; c += 64) {
    double s = 0.0;
    for (int64_t p = p0; p < p1; ++p) s = fma(data[p], X[indices[p] * m + c], s);
    double y = alpha * s;
    if (beta) y = fma(beta[c], X[i * m + c], y);
    if (Z) y = fma(gamma, Z[i * m + c], y);
    Y[i * m + c] = y;
  }
}

__global__ __launch_bounds__(256) void nb_transpose_f64_kernel(const double* __restrict__ a, int64_t rows, int64_t cols,
                                                               double* __restrict__ out) {
  __shared__ double t[32][33];
  const int64_t r0 = (int64_t)blockIdx.y * 32, c0 = (int64_t)blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int y = ty; y < 32; y += 8)
    if (r0 + y < rows && c0 + tx < cols) t[y][tx] = a[(r0 + y) * cols + c0 + tx];
  __syncthreads();
  for (int y = ty; y < 32; y += 8)
    if (c0 + y < cols && r0 + tx < rows) out[(c0 + y) * rows + r0 + tx] = t[tx][y];
}

static unsigned nb_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 65536)); }

template <typename T>
static int nb_sqnorms(pvs_ctx* ctx, const T* x, int64_t rows, int64_t L, double* out) {
  if (rows <= 0) return PVS_OK;
  hipLaunchKernelGGL(nb_sqnorm_kernel<T>, dim3((unsigned)rows), dim3(256), 0, ctx->stream, x, rows, L, out);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

// float64 kNN over complete rows: f64 GEMM panel -> -d -> rank (approximate k-th) -> candidates within the margin -> re-score in
// the fixed order of nb_rescore_kernel -> rank.  The GEMM's split-K tail sums some tiles in another order, so its values alone
// could order two identical rows by rounding; the re-score makes the value a function of the two rows.
static int knn_f64_rows(pvs_ctx* ctx, const double* Q, int64_t nq, const double* X, int64_t N, int64_t L, const double* xn,
                        const double* yn, const double* d_ymax2, int k, int64_t* d_idx, double* d_dist) {
  const PanelPlan plan = panel_full_rows(nq, N, panel_elems<double>());
  const int64_t QT = plan.QT;
  const int cap = std::min(NB_CAP_MAX, std::max(256, 8 * k));
  const bool filt = k <= NB_K_MAX;
  char* w6 = nullptr;
  WsLayout<> lay;
  const auto aidx_p = lay.add<int64_t>((size_t)QT * k);
  const auto aval_p = lay.add<double>((size_t)QT * k);
  const auto cand_p = lay.add<int64_t>((size_t)QT * cap);
  const auto count_p = lay.add<int>((size_t)QT);
  const auto key_p = lay.add<double>((size_t)QT * cap);
  const auto ovf_p = lay.add<unsigned long long>(32);
  PVS_TRY(ws_reserve(ctx, WS_LISTS, lay.bytes(), &w6));
  int64_t* aidx = aidx_p(w6);
  double* aval = aval_p(w6);
  int64_t* cand = cand_p(w6);
  int* count = count_p(w6);
  double* key = key_p(w6);
  unsigned long long* ovf = ovf_p(w6);
  PVS_HIP(hipMemsetAsync(ovf, 0, 8, ctx->stream));
  return panel_for_each<double>(ctx, plan, [&](int64_t q0, int64_t qn, int64_t, int64_t, double* panel) -> int {
    PVS_TRY(launch_cosine_f64_dev(ctx, Q + q0 * L, qn, X, N, L, nullptr, nullptr, panel, N));
    {
      ScopedTimer tm(ctx, T_MISC);
      hipLaunchKernelGGL(nb_negdist_f64_kernel, dim3(nb_grid(qn * N)), dim3(256), 0, ctx->stream, panel, qn, N, N, xn + q0, yn);
      PVS_HIP(hipGetLastError());
    }
    if (!filt) {
      PVS_TRY(launch_rank_f64(ctx, panel, qn, N, N, k, d_idx + q0 * k, d_dist + q0 * k));
      ScopedTimer tm(ctx, T_MISC);
      hipLaunchKernelGGL(nb_negate_kernel, dim3(nb_grid(qn * k)), dim3(256), 0, ctx->stream, d_dist + q0 * k, qn * k, d_dist + q0 * k);
      PVS_HIP(hipGetLastError());
      return PVS_OK;
    }
    PVS_TRY(launch_rank_f64(ctx, panel, qn, N, N, k, aidx, aval));
    ScopedTimer tm(ctx, T_RESCORE);
    hipLaunchKernelGGL(nb_collect_kernel<double>, dim3((unsigned)((qn + 3) / 4)), dim3(256), 0, ctx->stream, panel, qn, N, N, aval, k,
                       xn + q0, d_ymax2, L, 0.0, cap, (int64_t)0, 1, cand, count, ovf);
    const int64_t waves = qn * cap;
    hipLaunchKernelGGL(nb_rescore_kernel<double>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, ctx->stream, Q + q0 * L, X, qn, L,
                       cand, count, cap, xn + q0, yn, key);
    hipLaunchKernelGGL(nb_rank_kernel, dim3((unsigned)qn), dim3(256), 0, ctx->stream, cand, key, count, cap, k, aidx, aval,
                       d_idx + q0 * k, d_dist + q0 * k);
    PVS_HIP(hipGetLastError());
    return PVS_OK;
  });
}

// float32 rows -> float64 copies in WS_NB_F64_ROWS (the full f64 pass); Q == X shares one copy
static int to_f64_copies(pvs_ctx* ctx, const float* Q, int64_t nq, const float* X, int64_t N, int64_t L, double** q64, double** x64) {
  const bool same = (Q == X && nq == N);
  WsLayout<> lay;
  const auto x_p = lay.add<double>((size_t)N * L), q_p = lay.add<double>(same ? 0 : (size_t)nq * L);
  char* w = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_NB_F64_ROWS, lay.bytes(), &w));
  *x64 = x_p(w);
  *q64 = same ? *x64 : q_p(w);
  ScopedTimer tm(ctx, T_MISC);
  hipLaunchKernelGGL(nb_f32_to_f64_kernel, dim3(nb_grid(N * L)), dim3(256), 0, ctx->stream, X, N * L, *x64);
  if (!same) hipLaunchKernelGGL(nb_f32_to_f64_kernel, dim3(nb_grid(nq * L)), dim3(256), 0, ctx->stream, Q, nq * L, *q64);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

static int nb_check(pvs_ctx* ctx, const void* Q, int64_t nq, const void* X, int64_t N, int64_t L) {
  if (!ctx) PVS_FAIL(PVS_ERR_INVALID, "null ctx");
  if (nq < 0 || N <= 0 || L <= 0) PVS_FAIL(PVS_ERR_INVALID, "neighbours: need nq >= 0, N > 0, L > 0");
  if (nq > 0 && (!Q || !X)) PVS_FAIL(PVS_ERR_INVALID, "neighbours: null rows");
  PVS_HIP(hipSetDevice(ctx->device));
  return PVS_OK;
}

}  // namespace pvs

using namespace pvs;

PVS_EXPORT int pvs_l2_knn_dev(pvs_ctx* ctx, const void* d_Q, int64_t nq, const void* d_X, int64_t N, int64_t L, int is_f64, int k,
                              int64_t* d_idx, double* d_sqdist, int64_t* h_stats) {
  if (h_stats) h_stats[0] = h_stats[1] = h_stats[2] = h_stats[3] = 0;
  PVS_TRY(nb_check(ctx, d_Q, nq, d_X, N, L));
  if (k < 1 || k > N) PVS_FAIL(PVS_ERR_INVALID, "n_neighbors = %d out of range 1..%lld", k, (long long)N);
  if (nq == 0) return PVS_OK;
  if (!d_idx || !d_sqdist) PVS_FAIL(PVS_ERR_INVALID, "pvs_l2_knn_dev: null output");
  const bool same = (d_Q == d_X && nq == N);
  // norms |x|^2 (queries) and |y|^2 (rows), f64, + the largest of both
  WsLayout<> nrm;
  const auto nrm_p = nrm.add<double>((size_t)(N + (same ? 0 : nq))), max_p = nrm.add<double>(32);
  char* w7 = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_NB_NORMS, nrm.bytes(), &w7));
  double* yn = nrm_p(w7);
  double* xn = same ? yn : yn + N;
  double* d_max = max_p(w7);
  if (is_f64) {
    const double* Q = static_cast<const double*>(d_Q);
    const double* X = static_cast<const double*>(d_X);
    PVS_TRY(nb_sqnorms(ctx, X, N, L, yn));
    if (!same) PVS_TRY(nb_sqnorms(ctx, Q, nq, L, xn));
    hipLaunchKernelGGL(nb_max_kernel, dim3(1), dim3(256), 0, ctx->stream, yn, N + (same ? 0 : nq), d_max);
    PVS_HIP(hipGetLastError());
    return knn_f64_rows(ctx, Q, nq, X, N, L, xn, yn, d_max, k, d_idx, d_sqdist);
  }
  const float* Q = static_cast<const float*>(d_Q);
  const float* X = static_cast<const float*>(d_X);
  PVS_TRY(nb_sqnorms(ctx, X, N, L, yn));
  if (!same) PVS_TRY(nb_sqnorms(ctx, Q, nq, L, xn));
  hipLaunchKernelGGL(nb_max_kernel, dim3(1), dim3(256), 0, ctx->stream, yn, N + (same ? 0 : nq), d_max);
  PVS_HIP(hipGetLastError());
  double h_max = 0.0;
  PVS_HIP(hipMemcpyAsync(&h_max, d_max, 8, hipMemcpyDeviceToHost, ctx->stream));
  PVS_HIP(hipStreamSynchronize(ctx->stream));
  bool filtered = k <= NB_K_MAX && std::isfinite(h_max) && h_max <= 0x1p100;
  if (filtered) {
    const int cap = std::min(NB_CAP_MAX, std::max(256, 8 * k));
    const PanelPlan plan = panel_dense(nq, N);
    // which f32 GEMM kernel launch_cosine_f32 picks for these panels (panel offsets keep the 16-B alignment of the bases)
    const bool mfma = L % 4 == 0 && reinterpret_cast<uintptr_t>(Q) % 16 == 0 && reinterpret_cast<uintptr_t>(X) % 16 == 0 &&
                      L <= (int64_t)8 * 1024 * 1024;
    const double chain = mfma ? 1025.0 + (double)L / 1024.0 : (double)L + 1.0;
    const KnnF32Layout lay = knn_f32_layout(N, plan.QT, k, cap);
    char* w6 = nullptr;
    PVS_TRY(ws_reserve(ctx, WS_LISTS, lay.bytes, &w6));
    float* hy = lay.hy(w6);
    int64_t* aidx = lay.aidx(w6);
    float* aval = lay.aval(w6);
    int64_t* cand = lay.cand(w6);
    int* count = lay.count(w6);
    double* key = lay.key(w6);
    unsigned long long* ovf = lay.ovf(w6);
    PVS_HIP(hipMemsetAsync(ovf, 0, 8, ctx->stream));
    hipLaunchKernelGGL(nb_half_f32_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, yn, N, hy);
    PVS_HIP(hipGetLastError());
    int64_t n_cand = 0;
    for (int64_t q0 = 0; q0 < nq; q0 += plan.QT) {
      const int64_t qn = plan.qn(q0);
      PVS_TRY(panel_query_block<float>(ctx, plan, q0, [&](int64_t, int64_t, int64_t c0, int64_t cn, float* panel) -> int {
        PVS_TRY(launch_cosine_f32(ctx, Q + q0 * L, qn, X + c0 * L, cn, L, nullptr, nullptr, panel, cn));
        {
          ScopedTimer tm(ctx, T_MISC);
          hipLaunchKernelGGL(nb_key_f32_kernel, dim3(nb_grid(qn * cn)), dim3(256), 0, ctx->stream, panel, qn, cn, cn, hy + c0);
          PVS_HIP(hipGetLastError());
        }
        PVS_TRY(launch_topk(ctx, panel, qn, cn, cn, k, c0, c0 > 0 ? 1 : 0, aidx, aval));
        {
          ScopedTimer tm(ctx, T_MISC);
          hipLaunchKernelGGL(nb_collect_kernel<float>, dim3((unsigned)((qn + 3) / 4)), dim3(256), 0, ctx->stream, panel, qn, cn, cn, aval, k,
                             xn + q0, d_max, L, chain, cap, c0, c0 == 0 ? 1 : 0, cand, count, ovf);
          PVS_HIP(hipGetLastError());
        }
        return PVS_OK;
      }));
      {
        ScopedTimer tm(ctx, T_RESCORE);
        const int64_t waves = qn * cap;
        hipLaunchKernelGGL(nb_rescore_kernel<float>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, ctx->stream, Q + q0 * L, X, qn, L,
                           cand, count, cap, xn + q0, yn, key);
        hipLaunchKernelGGL(nb_rank_kernel, dim3((unsigned)qn), dim3(256), 0, ctx->stream, cand, key, count, cap, k, (const int64_t*)nullptr,
                           (const double*)nullptr, d_idx + q0 * k, d_sqdist + q0 * k);
        PVS_HIP(hipGetLastError());
      }
      if (h_stats) {
        std::vector<int> hc((size_t)qn);
        PVS_HIP(hipMemcpyAsync(hc.data(), count, (size_t)qn * 4, hipMemcpyDeviceToHost, ctx->stream));
        PVS_HIP(hipStreamSynchronize(ctx->stream));
        for (int c : hc) n_cand += std::min(c, cap);
      }
    }
    unsigned long long h_ovf = 0;
    PVS_HIP(hipMemcpyAsync(&h_ovf, ovf, 8, hipMemcpyDeviceToHost, ctx->stream));
    PVS_HIP(hipStreamSynchronize(ctx->stream));
    if (h_stats) {
      h_stats[0] = 1;
      h_stats[1] = (int64_t)h_ovf;
      h_stats[2] = n_cand;
      h_stats[3] = cap;
    }
    if (h_ovf == 0) return PVS_OK;
  }
  // the full float64 pass (overflowing candidate lists, k > 256, very large or non-finite rows)
  double* q64 = nullptr;
  double* x64 = nullptr;
  PVS_TRY(to_f64_copies(ctx, Q, nq, X, N, L, &q64, &x64));
  return knn_f64_rows(ctx, q64, nq, x64, N, L, xn, yn, d_max, k, d_idx, d_sqdist);
}

// radius neighbours: pass 1 (fill == 0) writes the counts to d_out[nq]; pass 2 (fill != 0) takes d_indptr[nq + 1] and writes
// d_indices (and d_sqdist when not null) in index order.  Both passes run the same float64 panels.
static int radius_impl(pvs_ctx* ctx, const void* d_Q, int64_t nq, const void* d_X, int64_t N, int64_t L, int is_f64, double r,
                       int fill, const int64_t* d_indptr, int64_t* d_counts, int64_t* d_indices, double* d_sqdist) {
  PVS_TRY(nb_check(ctx, d_Q, nq, d_X, N, L));
  if (!(r >= 0.0)) PVS_FAIL(PVS_ERR_INVALID, "radius must be >= 0");
  if (nq == 0) return PVS_OK;
  const bool same = (d_Q == d_X && nq == N);
  const double* Q = static_cast<const double*>(d_Q);
  const double* X = static_cast<const double*>(d_X);
  double* q64 = nullptr;
  double* x64 = nullptr;
  if (!is_f64) {
    PVS_TRY(to_f64_copies(ctx, static_cast<const float*>(d_Q), nq, static_cast<const float*>(d_X), N, L, &q64, &x64));
    Q = q64;
    X = x64;
  }
  WsLayout<> nrm;
  const auto nrm_p = nrm.add<double>((size_t)(N + (same ? 0 : nq)));
  const auto cur_p = nrm.add<int64_t>((size_t)nq);
  char* w7 = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_NB_NORMS, nrm.bytes(), &w7));
  double* yn = nrm_p(w7);
  double* xn = same ? yn : yn + N;
  int64_t* cursor = cur_p(w7);
  PVS_TRY(nb_sqnorms(ctx, X, N, L, yn));
  if (!same) PVS_TRY(nb_sqnorms(ctx, Q, nq, L, xn));
  if (fill) {
    hipLaunchKernelGGL(nb_copy_i64_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream, d_indptr, nq, cursor);
    PVS_HIP(hipGetLastError());
  } else {
    PVS_HIP(hipMemsetAsync(cursor, 0, (size_t)nq * 8, ctx->stream));
  }
  PVS_TRY(panel_for_each<double>(ctx, panel_full_rows(nq, N, panel_elems<double>()),
                                 [&](int64_t q0, int64_t qn, int64_t, int64_t, double* panel) -> int {
    PVS_TRY(launch_cosine_f64_dev(ctx, Q + q0 * L, qn, X, N, L, nullptr, nullptr, panel, N));
    ScopedTimer tm(ctx, T_MISC);
    if (fill)
      hipLaunchKernelGGL(nb_radius_kernel<true>, dim3((unsigned)((qn + 3) / 4)), dim3(256), 0, ctx->stream, panel, qn, N, N, xn + q0, yn, r,
                         (int64_t)0, cursor + q0, d_indices, d_sqdist);
    else
      hipLaunchKernelGGL(nb_radius_kernel<false>, dim3((unsigned)((qn + 3) / 4)), dim3(256), 0, ctx->stream, panel, qn, N, N, xn + q0, yn,
                         r, (int64_t)0, cursor + q0, (int64_t*)nullptr, (double*)nullptr);
    PVS_HIP(hipGetLastError());
    return PVS_OK;
  }));
  if (!fill) PVS_HIP(hipMemcpyAsync(d_counts, cursor, (size_t)nq * 8, hipMemcpyDeviceToDevice, ctx->stream));
  return PVS_OK;
}

PVS_EXPORT int pvs_l2_radius_count_dev(pvs_ctx* ctx, const void* d_Q, int64_t nq, const void* d_X, int64_t N, int64_t L, int is_f64,
                                       double r_sq, int64_t* d_counts) {
  if (nq > 0 && !d_counts) PVS_FAIL(PVS_ERR_INVALID, "pvs_l2_radius_count_dev: null counts");
  return radius_impl(ctx, d_Q, nq, d_X, N, L, is_f64, r_sq, 0, nullptr, d_counts, nullptr, nullptr);
}

PVS_EXPORT int pvs_l2_radius_fill_dev(pvs_ctx* ctx, const void* d_Q, int64_t nq, const void* d_X, int64_t N, int64_t L, int is_f64,
                                      double r_sq, const int64_t* d_indptr, int64_t* d_indices, double* d_sqdist) {
  if (nq > 0 && (!d_indptr || !d_indices)) PVS_FAIL(PVS_ERR_INVALID, "pvs_l2_radius_fill_dev: null indptr / indices");
  return radius_impl(ctx, d_Q, nq, d_X, N, L, is_f64, r_sq, 1, d_indptr, nullptr, d_indices, d_sqdist);
}

PVS_EXPORT int pvs_csr_spmm_f64_dev(pvs_ctx* ctx, int64_t n, const int64_t* d_indptr, const int64_t* d_indices, const double* d_data,
                                    const double* d_X, int m, double alpha, const double* d_beta, const double* d_Z, double gamma,
                                    double* d_Y) {
  if (!ctx) PVS_FAIL(PVS_ERR_INVALID, "null ctx");
  if (n < 0 || m < 0) PVS_FAIL(PVS_ERR_INVALID, "spmm: negative size");
  if (n == 0 || m == 0) return PVS_OK;
  if (!d_indptr || !d_indices || !d_data || !d_X || !d_Y) PVS_FAIL(PVS_ERR_INVALID, "spmm: null operand");
  if (d_Y == d_X || (d_Z && d_Y == d_Z)) PVS_FAIL(PVS_ERR_INVALID, "spmm: Y must not alias X or Z");
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer tm(ctx, T_MISC);
  hipLaunchKernelGGL(nb_spmm_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, ctx->stream, n, d_indptr, d_indices, d_data, d_X, m,
                     alpha, d_beta, d_Z, gamma, d_Y);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

PVS_EXPORT int pvs_transpose_f64_dev(pvs_ctx* ctx, const double* d_src, int64_t rows, int64_t cols, double* d_dst) {
  if (!ctx) PVS_FAIL(PVS_ERR_INVALID, "null ctx");
  if (rows < 0 || cols < 0) PVS_FAIL(PVS_ERR_INVALID, "transpose: negative size");
  if (rows == 0 || cols == 0) return PVS_OK;
  if (!d_src || !d_dst || d_src == d_dst) PVS_FAIL(PVS_ERR_INVALID, "transpose: null or aliased operand");
  if ((rows + 31) / 32 > 65535) PVS_FAIL(PVS_ERR_UNSUPPORTED, "transpose: too many rows");
  PVS_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(nb_transpose_f64_kernel, dim3((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32)), dim3(256), 0, ctx->stream,
                     d_src, rows, cols, d_dst);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}
