// Diffusion re-ranking on the kNN graph of a resident index (definitions in include/pvsim.h).
//
// All graph and solver arithmetic is float64 with every multiply, add, subtract and divide rounded on its own, in the order the header
// states, so this unit is compiled with -ffp-contract=off, like pq.hip and expand.hip: a NumPy restatement gives the same bits.
//
// The graph is fixed-width rows (ELL): nbr int32 [N][kg] and s float64 [N][kg]; a slot that is not mutual holds s = +0 and adds
// nothing.  The four graph kernels (drop self + affinity, the mutual pass, degrees, normalised entries) are one lane per entry or per
// row; none of them is a throughput path.  The five maintenance kernels of a mutable graph (lists with the
// similarity kept, the merge of stored lists with candidates, damage flags, the remap through the keep positions, affinities from
// stored similarities) are of the same kind: integer work, comparisons and moves, every output element written once.
//
// The solver is conjugate gradients on (I - alpha S) x = y for C columns at once.  Vectors are [N][C], columns innermost, so the values
// of one neighbour for a tile of columns are one contiguous read.  One workgroup owns one block of 256 rows -- the block of the dot
// product's definition -- and CW columns; CW in {1, 4, 16, 64} is a template parameter.  A thread owns column tid % CW and the CW rows
// s + (256 / CW) m, m = 0 .. CW-1, with s = tid / CW.  Those rows are a complete subtree at the bottom of the block's fixed summation
// tree (v[0:h] += v[h:2h], h = 128 .. 1, pairs rows that differ in the HIGH bits first), so a thread reduces its own rows in
// registers: it walks m in bit-reversed order, which turns the subtree into an adjacent-pair tree, and keeps one partial per level
// (a binary counter).  What is left, 256 / CW partials per column, is the same rule over s and goes through 2 KiB of LDS.  With
// CW = 64 a wave owns a row: the row's nbr / s entries are wave-uniform and arrive as scalar loads (the row number goes through
// readfirstlane), as in combine_rows_kernel; with CW = 1 (one query, the serving case) the 256 lanes spread over 256 rows.  Every CW
// adds the same numbers in the same tree, so every CW gives the same bits.
//
// Per step: apply (Ap = p - alpha S p, block partials of p.Ap) -> one workgroup adds the partials in block order and forms a, retiring
// columns with p.Ap <= 0 -> update (x, r, block partials of r.r) -> one workgroup forms b, rr and the flags of the next step -> p.
// A column that does not step is not written.  The host reads one int (columns that still step) every check_every steps, only in
// order to stop launching.  From list_common.hpp: ranges_overlap.
#include <algorithm>

#include "list_common.hpp"

namespace pvs {

constexpr int DF_THREADS = PVS_DIFFUSE_DOT_BLOCK;   // 256: threads of a workgroup = rows of a dot-product block
constexpr int DF_U = 8;                             // graph slots whose gathers are in flight together
constexpr int DF_GAMMA_MAX = 8;
static_assert(DF_THREADS == 256, "the summation tree of the header is over blocks of 256 rows");

__device__ __forceinline__ double df_affinity(double v, int gamma) {
  const double sp = v > 0.0 ? v : 0.0;   // a NaN counts as 0
  if (gamma == 0) return 1.0;
  double a = sp;
  for (int g = 1; g < gamma; ++g) a = a * sp;
  return a;
}

static unsigned df_grid(int64_t n) { return (unsigned)((n + DF_THREADS - 1) / DF_THREADS); }

// ---------------------------------------------------------------------------------------------------------------- graph kernels
// one lane per output entry: lists idx / val [b][kg + 1] of rows row0 .. row0 + b - 1 -> nbr / a rows of the same numbers
template <typename T>
__global__ __launch_bounds__(DF_THREADS) void df_affinity_kernel(const int64_t* __restrict__ idx, const T* __restrict__ val, int64_t b,
                                                                 int kg, int64_t row0, int64_t N, int gamma, int32_t* __restrict__ nbr,
                                                                 double* __restrict__ a) {
  const int64_t e = (int64_t)blockIdx.x * DF_THREADS + threadIdx.x;
  if (e >= b * kg) return;
  const int64_t i = e / kg;
  const int t = (int)(e - i * kg);
  const int64_t* li = idx + i * (kg + 1);
  int drop = kg;                                  // the last slot where the row itself is absent
  for (int u = 0; u <= kg; ++u)
    if (li[u] == row0 + i) {
      drop = u;
      break;
    }
  const int src = t < drop ? t : t + 1;
  const int64_t j = li[src];
  const int64_t o = (row0 + i) * kg + t;
  nbr[o] = (j >= 0 && j < N) ? (int32_t)j : -1;
  a[o] = df_affinity((double)val[i * (kg + 1) + src], gamma);
}

// one lane per (row, slot): scan the partner's kg slots for the row
__global__ __launch_bounds__(DF_THREADS) void df_mutual_kernel(const int32_t* __restrict__ nbr, const double* __restrict__ a, int64_t N,
                                                               int kg, double* __restrict__ w) {
  const int64_t e = (int64_t)blockIdx.x * DF_THREADS + threadIdx.x;
  if (e >= N * kg) return;
  const int64_t i = e / kg;
  const int32_t j = nbr[e];
  double out = 0.0;
  if (j >= 0 && j < N) {
    const int32_t* lj = nbr + (int64_t)j * kg;
    for (int u = 0; u < kg; ++u)
      if (lj[u] == i) {
        const double mine = a[e], theirs = a[(int64_t)j * kg + u];
        out = theirs < mine ? theirs : mine;
        break;
      }
  }
  w[e] = out;
}

__global__ __launch_bounds__(DF_THREADS) void df_degree_kernel(const double* __restrict__ w, int64_t N, int kg, double* __restrict__ deg,
                                                               double* __restrict__ r) {
  const int64_t i = (int64_t)blockIdx.x * DF_THREADS + threadIdx.x;
  if (i >= N) return;
  double d = 0.0;
  for (int t = 0; t < kg; ++t) d = d + w[i * kg + t];
  deg[i] = d;
  r[i] = d > 0.0 ? 1.0 / sqrt(d) : 0.0;
}

__global__ __launch_bounds__(DF_THREADS) void df_normalise_kernel(const int32_t* __restrict__ nbr, const double* __restrict__ w,
                                                                  const double* __restrict__ r, int64_t N, int kg, double* __restrict__ s) {
  const int64_t e = (int64_t)blockIdx.x * DF_THREADS + threadIdx.x;
  if (e >= N * kg) return;
  const int64_t i = e / kg;
  const int32_t j = nbr[e];
  const double rj = (j >= 0 && j < N) ? r[j] : 0.0;
  s[e] = w[e] * (r[i] * rj);
}

// Y is zero already; one lane per list entry
template <typename T>
__global__ __launch_bounds__(DF_THREADS) void df_rhs_kernel(const int64_t* __restrict__ idx, const T* __restrict__ val, int64_t C, int kq,
                                                            int64_t N, int gamma, double* __restrict__ Y) {
  const int64_t e = (int64_t)blockIdx.x * DF_THREADS + threadIdx.x;
  if (e >= C * kq) return;
  const int64_t c = e / kq;
  const int64_t j = idx[e];
  if (j >= 0 && j < N) Y[j * C + c] = df_affinity((double)val[e], gamma);
}

// ---------------------------------------------------------------------------------------------------------------- graph maintenance
//   one lane per output entry: drop self as df_affinity_kernel, the similarity kept; a row's own number comes
// from ids where given.  A row whose own number leaves [0, N) writes nothing.
__global__ __launch_bounds__(DF_THREADS) void df_lists_kernel(const int64_t* __restrict__ idx, const float* __restrict__ val, int64_t b, int kg,
                                                              int64_t row0, const int64_t* __restrict__ ids, int64_t N,
                                                              int32_t* __restrict__ nbr, float* __restrict__ sim) {
  const int64_t e = (int64_t)blockIdx.x * DF_THREADS + threadIdx.x;
  if (e >= b * kg) return;
  const int64_t p = e / kg;
  const int t = (int)(e - p * kg);
  const int64_t own = ids ? ids[p] : row0 + p;
  if (own < 0 || own >= N) return;
  const int64_t* li = idx + p * (kg + 1);
  int drop = kg;
  for (int u = 0; u <= kg; ++u)
    if (li[u] == own) {
      drop = u;
      break;
    }
  const int src = t < drop ? t : t + 1;
  const int64_t j = li[src];
  const int64_t o = own * kg + t;
  nbr[o] = (j >= 0 && j < N) ? (int32_t)j : -1;
  sim[o] = val[p * (kg + 1) + src];
}

// the order of the lists: numbers before NaNs, larger before smaller (-0 and +0 tie), then the smaller id
__device__ __forceinline__ bool df_before(float xv, int64_t xid, float yv, int64_t yid) {
  const bool xn = xv != xv, yn = yv != yv;
  if (xn != yn) return yn;
  if (!xn) {
    if (xv > yv) return true;
    if (xv < yv) return false;
  }
  return xid < yid;
}

// one lane per row: a two-way merge of the stored list and the candidates, cut after kg entries; t entries out means at most t
// stored ones taken, so the stored list never runs out
__global__ __launch_bounds__(DF_THREADS) void df_merge_kernel(const int32_t* __restrict__ nbr, const float* __restrict__ sim,
                                                              const int64_t* __restrict__ cidx, const float* __restrict__ cval, int64_t rows,
                                                              int kg, int c, int64_t col_offset, int64_t N, int32_t* __restrict__ onbr,
                                                              float* __restrict__ osim) {
  const int64_t i = (int64_t)blockIdx.x * DF_THREADS + threadIdx.x;
  if (i >= rows) return;
  const int32_t* ln = nbr + i * kg;
  const float* ls = sim + i * kg;
  const int64_t* ci = cidx + i * c;
  const float* cv = cval + i * c;
  int p = 0, q = 0;
  for (int t = 0; t < kg; ++t) {
    while (q < c && ci[q] < 0) ++q;
    const int32_t sj = ln[p];
    const float sv = ls[p];
    int64_t cj = 0;
    float cs = 0.f;
    bool take = false;
    if (q < c) {
      cj = ci[q] + col_offset;
      cs = cv[q];
      take = df_before(cs, cj, sv, (int64_t)sj);
    }
    if (take) {
      onbr[i * kg + t] = (cj >= 0 && cj < N) ? (int32_t)cj : -1;
      osim[i * kg + t] = cs;
      ++q;
    } else {
      onbr[i * kg + t] = sj;
      osim[i * kg + t] = sv;
      ++p;
    }
  }
}

// one lane per row
__global__ __launch_bounds__(DF_THREADS) void df_damage_kernel(const int32_t* __restrict__ nbr, int64_t N, int kg,
                                                               const uint8_t* __restrict__ keep, uint8_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * DF_THREADS + threadIdx.x;
  if (i >= N) return;
  uint8_t f = 0;
  if (keep[i] != 0)
    for (int t = 0; t < kg; ++t) {
      const int32_t j = nbr[i * kg + t];
      if (j >= 0 && j < N && keep[j] == 0) {
        f = 1;
        break;
      }
    }
  flag[i] = f;
}

// one lane per entry; a lane reads the entry it writes, so out may be nbr itself
__global__ __launch_bounds__(DF_THREADS) void df_remap_kernel(const int32_t* nbr, int64_t N, int kg, const uint8_t* __restrict__ keep,
                                                              const int64_t* __restrict__ pos, int32_t* out) {
  const int64_t e = (int64_t)blockIdx.x * DF_THREADS + threadIdx.x;
  if (e >= N * kg) return;
  const int64_t i = e / kg;
  if (keep[i] == 0) return;
  const int32_t j = nbr[e];
  out[e] = (j >= 0 && j < N && keep[j] != 0) ? (int32_t)pos[j] : -1;
}

// one lane per 4-byte word of the output: out[p] = rows[ids[p]], zeros where the id leaves [0, n)
__global__ __launch_bounds__(DF_THREADS) void df_gather_rows_kernel(const uint32_t* __restrict__ rows, int64_t n, int64_t words,
                                                                    const int64_t* __restrict__ ids, int64_t b, uint32_t* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * DF_THREADS + threadIdx.x;
  if (e >= b * words) return;
  const int64_t p = e / words;
  const int64_t w = e - p * words;
  const int64_t i = ids[p];
  out[e] = (i >= 0 && i < n) ? rows[i * words + w] : 0u;
}

__global__ __launch_bounds__(DF_THREADS) void df_affinity_sim_kernel(const float* __restrict__ sim, int64_t n, int gamma,
                                                                     double* __restrict__ a) {
  const int64_t e = (int64_t)blockIdx.x * DF_THREADS + threadIdx.x;
  if (e >= n) return;
  a[e] = df_affinity((double)sim[e], gamma);
}

// ---------------------------------------------------------------------------------------------------------------- solver
constexpr int df_log2(int v) { return v <= 1 ? 0 : 1 + df_log2(v / 2); }

// the n-th leaf of a thread's subtree is its row m = n with the LOG bits reversed
template <int CW>
__device__ __forceinline__ int df_leaf_row(int n) {
  constexpr int LOG = df_log2(CW);
  if constexpr (LOG == 0) return 0;
  else return (int)(__brev((unsigned)n) >> (32 - LOG));
}

// an adjacent-pair tree over CW leaves pushed in ascending n: lvl[l] holds a finished subtree of 2^l leaves
template <int CW>
struct DfTree {
  static constexpr int LOG = df_log2(CW);
  double lvl[LOG > 0 ? LOG : 1];
  __device__ __forceinline__ void push(int n, double v, double& total) {
    bool carry = true;               // no early exit: the levels stay statically indexed, so lvl[] lives in registers
#pragma unroll
    for (int l = 0; l < LOG; ++l) {
      const bool bit = (n >> l) & 1;
      if (carry && bit) v = lvl[l] + v;
      if (carry && !bit) lvl[l] = v;
      carry = carry && bit;
    }
    if (carry) total = v;            // reached by the last leaf only
  }
};

// thread (s, cl) of a workgroup: rows blk * 256 + s + RP m, column chunk * CW + cl
template <int CW>
struct DfMap {
  static constexpr int RP = DF_THREADS / CW;
  int cl, s;
  __device__ __forceinline__ DfMap() {
    cl = (int)threadIdx.x % CW;
    s = (int)threadIdx.x / CW;
    if constexpr (CW == 64) s = __builtin_amdgcn_readfirstlane(s);   // a wave owns a row: the row number is uniform
  }
  __device__ __forceinline__ int64_t row(int n) const { return (int64_t)blockIdx.x * DF_THREADS + s + RP * df_leaf_row<CW>(n); }
};

// the upper levels of the block's tree, over s, and the store of the block's partial
template <int CW>
__device__ __forceinline__ void df_block_partial(const DfMap<CW>& mp, double total, double* red, double* __restrict__ part, int64_t C,
                                                 int64_t col, bool on) {
  constexpr int RP = DF_THREADS / CW;
  red[threadIdx.x] = total;
#pragma unroll
  for (int h = RP / 2; h >= 1; h >>= 1) {
    __syncthreads();
    if (mp.s < h) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + h * CW];
  }
  if (mp.s == 0 && on) part[(int64_t)blockIdx.x * C + col] = red[threadIdx.x];
}

// x = 0, r = p = y, block partials of y.y for every column
template <int CW>
__global__ __launch_bounds__(DF_THREADS) void df_init_kernel(const double* __restrict__ y, int64_t N, int64_t C, double* __restrict__ x,
                                                             double* __restrict__ r, double* __restrict__ p, double* __restrict__ part) {
  __shared__ double red[DF_THREADS];
  const DfMap<CW> mp;
  const int64_t col = (int64_t)blockIdx.y * CW + mp.cl;
  const bool on = col < C;
  DfTree<CW> tree;
  double total = 0.0;
  for (int n = 0; n < CW; ++n) {
    const int64_t i = mp.row(n);
    double prod = 0.0;
    if (i < N && on) {
      const double v = y[i * C + col];
      x[i * C + col] = 0.0;
      r[i * C + col] = v;
      p[i * C + col] = v;
      prod = v * v;
    }
    tree.push(n, prod, total);
  }
  df_block_partial<CW>(mp, total, red, part, C, col, on);
}

// Ap = p - alpha (S p) and the block partials of p.Ap, for the columns that step
template <int CW>
__global__ __launch_bounds__(DF_THREADS) void df_apply_kernel(const int32_t* __restrict__ nbr, const double* __restrict__ sv, int64_t N,
                                                              int kg, int64_t C, double alpha, const double* __restrict__ p,
                                                              const int* __restrict__ act, double* __restrict__ Ap,
                                                              double* __restrict__ part) {
  __shared__ double red[DF_THREADS];
  const DfMap<CW> mp;
  const int64_t col = (int64_t)blockIdx.y * CW + mp.cl;
  const bool on = col < C && act[col] != 0;
  if (!__syncthreads_or(on)) return;                     // no column of this chunk steps
  DfTree<CW> tree;
  double total = 0.0;
  for (int n = 0; n < CW; ++n) {
    const int64_t i = mp.row(n);
    double prod = 0.0;
    if (i < N && on) {
      const int32_t* li = nbr + i * kg;                  // CW = 64: wave-uniform, scalar loads
      const double* ls = sv + i * kg;
      double sum = 0.0;
      int t = 0;
      for (; t + DF_U <= kg; t += DF_U) {                // DF_U gathers in flight, consumed in slot order
        int32_t j[DF_U];
        double w[DF_U], v[DF_U];
#pragma unroll
        for (int u = 0; u < DF_U; ++u) {
          j[u] = li[t + u];
          w[u] = ls[t + u];
        }
#pragma unroll
        for (int u = 0; u < DF_U; ++u) v[u] = (uint32_t)j[u] < (uint32_t)N ? p[(int64_t)j[u] * C + col] : 0.0;
#pragma unroll
        for (int u = 0; u < DF_U; ++u) sum = sum + w[u] * v[u];
      }
      for (; t < kg; ++t) {
        const int32_t j = li[t];
        const double v = (uint32_t)j < (uint32_t)N ? p[(int64_t)j * C + col] : 0.0;
        sum = sum + ls[t] * v;
      }
      const double pi = p[i * C + col];
      const double ap = pi - alpha * sum;
      Ap[i * C + col] = ap;
      prod = pi * ap;
    }
    tree.push(n, prod, total);
  }
  df_block_partial<CW>(mp, total, red, part, C, col, on);
}

// x = x + a p, r = r - a Ap and the block partials of r.r, for the columns that step
template <int CW>
__global__ __launch_bounds__(DF_THREADS) void df_update_kernel(int64_t N, int64_t C, const double* __restrict__ a, const int* __restrict__ act,
                                                               const double* __restrict__ p, const double* __restrict__ Ap,
                                                               double* __restrict__ x, double* __restrict__ r, double* __restrict__ part) {
  __shared__ double red[DF_THREADS];
  const DfMap<CW> mp;
  const int64_t col = (int64_t)blockIdx.y * CW + mp.cl;
  const bool on = col < C && act[col] != 0;
  if (!__syncthreads_or(on)) return;
  const double av = on ? a[col] : 0.0;
  DfTree<CW> tree;
  double total = 0.0;
  for (int n = 0; n < CW; ++n) {
    const int64_t i = mp.row(n);
    double prod = 0.0;
    if (i < N && on) {
      const int64_t o = i * C + col;
      const double pv = p[o];
      x[o] = x[o] + av * pv;
      const double rv = r[o] - av * Ap[o];
      r[o] = rv;
      prod = rv * rv;
    }
    tree.push(n, prod, total);
  }
  df_block_partial<CW>(mp, total, red, part, C, col, on);
}

// p = r + b p for the columns that stepped
__global__ __launch_bounds__(DF_THREADS) void df_direction_kernel(int64_t N, int64_t C, const double* __restrict__ b, const int* __restrict__ upd,
                                                                  const double* __restrict__ r, double* __restrict__ p) {
  const int64_t e = (int64_t)blockIdx.x * DF_THREADS + threadIdx.x;
  if (e >= N * C) return;
  const int64_t col = e % C;
  if (upd[col] != 0) p[e] = r[e] + b[col] * p[e];
}

struct DfCols {          // per column, C entries each
  double *rr, *yy, *thr, *a, *b;
  int *act, *upd, *retired, *steps;
  int* remaining;        // one int: columns that take the next step
};

// One workgroup.  stage 0: rr = yy = sum, thr, first flags.  stage 1: p.Ap -> retire or a.  stage 2: rn -> b, rr, steps, next flags.
// The partials of a column are added from +0 in block order.
__global__ __launch_bounds__(DF_THREADS) void df_reduce_kernel(int stage, const double* __restrict__ part, int64_t nb, int64_t C, double tol,
                                                               DfCols st) {
  int remaining = 0;
  for (int64_t c0 = 0; c0 < C; c0 += DF_THREADS) {
    const int64_t col = c0 + threadIdx.x;
    bool next = false;
    if (col < C) {
      const bool on = stage == 0 || st.act[col] != 0;
      if (on) {
        double sum = 0.0;
        for (int64_t b = 0; b < nb; ++b) sum = sum + part[b * C + col];
        if (stage == 0) {
          st.rr[col] = sum;
          st.yy[col] = sum;
          st.thr[col] = (tol * tol) * sum;
          st.retired[col] = 0;
          st.steps[col] = 0;
          st.upd[col] = 0;
        } else if (stage == 1) {
          if (sum > 0.0) {                       // false for a NaN
            st.a[col] = st.rr[col] / sum;
          } else {
            st.retired[col] = 1;
            st.act[col] = 0;
          }
        } else {
          st.b[col] = sum / st.rr[col];
          st.rr[col] = sum;
          st.steps[col] = st.steps[col] + 1;
        }
      }
      if (stage != 1) {
        if (stage == 2) st.upd[col] = on ? 1 : 0;
        next = st.rr[col] > st.thr[col] && st.retired[col] == 0;
        st.act[col] = next ? 1 : 0;
      }
    }
    if (stage != 1) remaining += __syncthreads_count(next);
  }
  if (stage != 1 && threadIdx.x == 0) *st.remaining = remaining;
}

struct DfLayout {
  WsPiece<double> r, p, Ap, part, thr, a, b;
  WsPiece<int> act, upd, retired, remaining;
  size_t bytes;
};

static DfLayout df_layout(int64_t N, int64_t C) {
  const size_t nc = (size_t)N * (size_t)C, nb = (size_t)((N + DF_THREADS - 1) / DF_THREADS), c = (size_t)C;
  WsLayout<> l;
  DfLayout d;
  d.r = l.add<double>(nc);
  d.p = l.add<double>(nc);
  d.Ap = l.add<double>(nc);
  d.part = l.add<double>(nb * c);
  d.thr = l.add<double>(c);
  d.a = l.add<double>(c);
  d.b = l.add<double>(c);
  d.act = l.add<int>(c);
  d.upd = l.add<int>(c);
  d.retired = l.add<int>(c);
  d.remaining = l.add<int>(1);
  d.bytes = l.bytes();
  return d;
}

static int df_width(int64_t C, int width) { return width ? width : C == 1 ? 1 : C <= 4 ? 4 : C <= 16 ? 16 : 64; }

template <class F>
static int df_dispatch_width(int cw, F&& f) {
  switch (cw) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 16: return f(std::integral_constant<int, 16>{});
    default: return f(std::integral_constant<int, 64>{});
  }
}

static int df_check_graph_shape(const char* who, int64_t N, int kg) {
  if (N < 2 || N >= ((int64_t)1 << 31)) PVS_FAIL(PVS_ERR_INVALID, "%s: need 2 <= N < 2^31 (got N=%lld)", who, (long long)N);
  if (kg < 1 || kg > N - 1) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= kg <= N - 1 (got kg=%d, N=%lld)", who, kg, (long long)N);
  if ((double)N * kg > 4e11) PVS_FAIL(PVS_ERR_INVALID, "%s: the graph is too large", who);
  return PVS_OK;
}

}  // namespace pvs

using namespace pvs;

PVS_EXPORT int pvs_graph_affinity_dev(pvs_ctx* ctx, const int64_t* d_idx, const void* d_val, int val_f64, int64_t b, int kg, int64_t row0,
                                      int64_t N, int gamma, int32_t* d_nbr, double* d_a) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(df_check_graph_shape(__func__, N, kg));
  if (gamma < 0 || gamma > DF_GAMMA_MAX) PVS_FAIL(PVS_ERR_INVALID, "%s: gamma must be in 0..%d (got %d)", __func__, DF_GAMMA_MAX, gamma);
  if (b < 0 || row0 < 0 || row0 + b > N)
    PVS_FAIL(PVS_ERR_INVALID, "%s: rows [%lld, %lld) leave the index of %lld rows", __func__, (long long)row0, (long long)(row0 + b), (long long)N);
  if (b == 0) return PVS_OK;
  PVS_NEED(d_idx, "idx");
  PVS_NEED(d_val, "val");
  PVS_NEED(d_nbr, "nbr");
  PVS_NEED(d_a, "a");
  PVS_ALIGNED(d_idx, 8, "idx");
  PVS_ALIGNED(d_val, val_f64 ? 8 : 4, "val");
  PVS_ALIGNED(d_nbr, 4, "nbr");
  PVS_ALIGNED(d_a, 8, "a");
  const size_t in_n = (size_t)b * (kg + 1), out_n = (size_t)N * kg;
  const size_t val_bytes = in_n * (val_f64 ? 8 : 4);
  if (ranges_overlap(d_idx, in_n * 8, d_nbr, out_n * 4) || ranges_overlap(d_idx, in_n * 8, d_a, out_n * 8) ||
      ranges_overlap(d_val, val_bytes, d_nbr, out_n * 4) || ranges_overlap(d_val, val_bytes, d_a, out_n * 8))
    PVS_FAIL(PVS_ERR_INVALID, "%s: an output overlaps a list", __func__);
  if (ranges_overlap(d_nbr, out_n * 4, d_a, out_n * 8)) PVS_FAIL(PVS_ERR_INVALID, "%s: nbr overlaps a", __func__);
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer tm(ctx, T_MISC);
  if (val_f64)
    hipLaunchKernelGGL(df_affinity_kernel<double>, dim3(df_grid(b * kg)), dim3(DF_THREADS), 0, ctx->stream, d_idx, (const double*)d_val, b, kg,
                       row0, N, gamma, d_nbr, d_a);
  else
    hipLaunchKernelGGL(df_affinity_kernel<float>, dim3(df_grid(b * kg)), dim3(DF_THREADS), 0, ctx->stream, d_idx, (const float*)d_val, b, kg,
                       row0, N, gamma, d_nbr, d_a);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

PVS_EXPORT int pvs_graph_mutual_dev(pvs_ctx* ctx, const int32_t* d_nbr, const double* d_a, int64_t N, int kg, double* d_w) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(df_check_graph_shape(__func__, N, kg));
  PVS_NEED(d_nbr, "nbr");
  PVS_NEED(d_a, "a");
  PVS_NEED(d_w, "w");
  PVS_ALIGNED(d_nbr, 4, "nbr");
  PVS_ALIGNED(d_a, 8, "a");
  PVS_ALIGNED(d_w, 8, "w");
  const size_t n = (size_t)N * kg;
  if (ranges_overlap(d_w, n * 8, d_nbr, n * 4) || ranges_overlap(d_w, n * 8, d_a, n * 8)) PVS_FAIL(PVS_ERR_INVALID, "%s: w overlaps an input", __func__);
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer tm(ctx, T_MISC);
  hipLaunchKernelGGL(df_mutual_kernel, dim3(df_grid(N * kg)), dim3(DF_THREADS), 0, ctx->stream, d_nbr, d_a, N, kg, d_w);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

PVS_EXPORT int pvs_graph_degrees_dev(pvs_ctx* ctx, const double* d_w, int64_t N, int kg, double* d_deg, double* d_r) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(df_check_graph_shape(__func__, N, kg));
  PVS_NEED(d_w, "w");
  PVS_NEED(d_deg, "deg");
  PVS_NEED(d_r, "r");
  PVS_ALIGNED(d_w, 8, "w");
  PVS_ALIGNED(d_deg, 8, "deg");
  PVS_ALIGNED(d_r, 8, "r");
  const size_t n = (size_t)N * kg * 8, v = (size_t)N * 8;
  if (ranges_overlap(d_w, n, d_deg, v) || ranges_overlap(d_w, n, d_r, v) || ranges_overlap(d_deg, v, d_r, v))
    PVS_FAIL(PVS_ERR_INVALID, "%s: the arrays overlap", __func__);
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer tm(ctx, T_MISC);
  hipLaunchKernelGGL(df_degree_kernel, dim3(df_grid(N)), dim3(DF_THREADS), 0, ctx->stream, d_w, N, kg, d_deg, d_r);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

PVS_EXPORT int pvs_graph_normalise_dev(pvs_ctx* ctx, const int32_t* d_nbr, const double* d_w, const double* d_r, int64_t N, int kg,
                                       double* d_s) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(df_check_graph_shape(__func__, N, kg));
  PVS_NEED(d_nbr, "nbr");
  PVS_NEED(d_w, "w");
  PVS_NEED(d_r, "r");
  PVS_NEED(d_s, "s");
  PVS_ALIGNED(d_nbr, 4, "nbr");
  PVS_ALIGNED(d_w, 8, "w");
  PVS_ALIGNED(d_r, 8, "r");
  PVS_ALIGNED(d_s, 8, "s");
  const size_t n = (size_t)N * kg;
  if (ranges_overlap(d_s, n * 8, d_nbr, n * 4) || ranges_overlap(d_s, n * 8, d_r, (size_t)N * 8) || ranges_overlap(d_s, n * 8, d_w, n * 8))
    PVS_FAIL(PVS_ERR_INVALID, "%s: s overlaps an input", __func__);
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer tm(ctx, T_MISC);
  hipLaunchKernelGGL(df_normalise_kernel, dim3(df_grid(N * kg)), dim3(DF_THREADS), 0, ctx->stream, d_nbr, d_w, d_r, N, kg, d_s);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

// ---- graph maintenance
PVS_EXPORT int pvs_graph_lists_dev(pvs_ctx* ctx, const int64_t* d_idx, const float* d_val, int64_t b, int kg, int64_t row0,
                                   const int64_t* d_ids, int64_t N, int32_t* d_nbr, float* d_sim) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(df_check_graph_shape(__func__, N, kg));
  if (b < 0 || b > N) PVS_FAIL(PVS_ERR_INVALID, "%s: need 0 <= b <= N (got b=%lld, N=%lld)", __func__, (long long)b, (long long)N);
  if (!d_ids && (row0 < 0 || row0 + b > N))
    PVS_FAIL(PVS_ERR_INVALID, "%s: rows [%lld, %lld) leave the index of %lld rows", __func__, (long long)row0, (long long)(row0 + b), (long long)N);
  if (b == 0) return PVS_OK;
  PVS_NEED(d_idx, "idx");
  PVS_NEED(d_val, "val");
  PVS_NEED(d_nbr, "nbr");
  PVS_NEED(d_sim, "sim");
  PVS_ALIGNED(d_idx, 8, "idx");
  PVS_ALIGNED(d_val, 4, "val");
  PVS_ALIGNED(d_nbr, 4, "nbr");
  PVS_ALIGNED(d_sim, 4, "sim");
  PVS_ALIGNED(d_ids, 8, "ids");   // NULL passes
  const size_t in_n = (size_t)b * (kg + 1), out_b = (size_t)N * kg * 4;
  struct Range {
    const void* p;
    size_t n;
  } ins[] = {{d_idx, in_n * 8}, {d_val, in_n * 4}, {d_ids, d_ids ? (size_t)b * 8 : 0}};
  for (const Range& r : ins)
    if (r.n && (ranges_overlap(r.p, r.n, d_nbr, out_b) || ranges_overlap(r.p, r.n, d_sim, out_b)))
      PVS_FAIL(PVS_ERR_INVALID, "%s: an output overlaps an input", __func__);
  if (ranges_overlap(d_nbr, out_b, d_sim, out_b)) PVS_FAIL(PVS_ERR_INVALID, "%s: nbr overlaps sim", __func__);
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer tm(ctx, T_MISC);
  hipLaunchKernelGGL(df_lists_kernel, dim3(df_grid(b * kg)), dim3(DF_THREADS), 0, ctx->stream, d_idx, d_val, b, kg, row0, d_ids, N, d_nbr,
                     d_sim);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

PVS_EXPORT int pvs_graph_merge_dev(pvs_ctx* ctx, const int32_t* d_nbr, const float* d_sim, const int64_t* d_cidx, const float* d_cval,
                                   int64_t rows, int kg, int c, int64_t col_offset, int64_t N, int32_t* d_out_nbr, float* d_out_sim) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(df_check_graph_shape(__func__, N, kg));
  if (rows < 0 || rows > N) PVS_FAIL(PVS_ERR_INVALID, "%s: need 0 <= rows <= N (got rows=%lld, N=%lld)", __func__, (long long)rows, (long long)N);
  if (c < 1 || c > N) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= c <= N candidates per row (got c=%d)", __func__, c);
  if (col_offset < 0 || col_offset >= N)
    PVS_FAIL(PVS_ERR_INVALID, "%s: need 0 <= col_offset < N (got %lld, N=%lld)", __func__, (long long)col_offset, (long long)N);
  if (rows == 0) return PVS_OK;
  PVS_NEED(d_nbr, "nbr");
  PVS_NEED(d_sim, "sim");
  PVS_NEED(d_cidx, "cidx");
  PVS_NEED(d_cval, "cval");
  PVS_NEED(d_out_nbr, "out_nbr");
  PVS_NEED(d_out_sim, "out_sim");
  PVS_ALIGNED(d_nbr, 4, "nbr");
  PVS_ALIGNED(d_sim, 4, "sim");
  PVS_ALIGNED(d_cidx, 8, "cidx");
  PVS_ALIGNED(d_cval, 4, "cval");
  PVS_ALIGNED(d_out_nbr, 4, "out_nbr");
  PVS_ALIGNED(d_out_sim, 4, "out_sim");
  const size_t lb = (size_t)rows * kg * 4, cn = (size_t)rows * c;
  struct Range {
    const void* p;
    size_t n;
  } ins[] = {{d_nbr, lb}, {d_sim, lb}, {d_cidx, cn * 8}, {d_cval, cn * 4}};
  for (const Range& r : ins)
    if (ranges_overlap(r.p, r.n, d_out_nbr, lb) || ranges_overlap(r.p, r.n, d_out_sim, lb))
      PVS_FAIL(PVS_ERR_INVALID, "%s: an output overlaps an input", __func__);
  if (ranges_overlap(d_out_nbr, lb, d_out_sim, lb)) PVS_FAIL(PVS_ERR_INVALID, "%s: out_nbr overlaps out_sim", __func__);
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer tm(ctx, T_MISC);
  hipLaunchKernelGGL(df_merge_kernel, dim3(df_grid(rows)), dim3(DF_THREADS), 0, ctx->stream, d_nbr, d_sim, d_cidx, d_cval, rows, kg, c,
                     col_offset, N, d_out_nbr, d_out_sim);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

PVS_EXPORT int pvs_graph_damage_dev(pvs_ctx* ctx, const int32_t* d_nbr, int64_t N, int kg, const uint8_t* d_keep, uint8_t* d_flag) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(df_check_graph_shape(__func__, N, kg));
  PVS_NEED(d_nbr, "nbr");
  PVS_NEED(d_keep, "keep");
  PVS_NEED(d_flag, "flag");
  PVS_ALIGNED(d_nbr, 4, "nbr");
  if (ranges_overlap(d_flag, (size_t)N, d_nbr, (size_t)N * kg * 4) || ranges_overlap(d_flag, (size_t)N, d_keep, (size_t)N))
    PVS_FAIL(PVS_ERR_INVALID, "%s: flag overlaps an input", __func__);
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer tm(ctx, T_MISC);
  hipLaunchKernelGGL(df_damage_kernel, dim3(df_grid(N)), dim3(DF_THREADS), 0, ctx->stream, d_nbr, N, kg, d_keep, d_flag);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

PVS_EXPORT int pvs_graph_remap_dev(pvs_ctx* ctx, const int32_t* d_nbr, int64_t N, int kg, const uint8_t* d_keep, const int64_t* d_pos,
                                   int32_t* d_out) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(df_check_graph_shape(__func__, N, kg));
  PVS_NEED(d_nbr, "nbr");
  PVS_NEED(d_keep, "keep");
  PVS_NEED(d_pos, "pos");
  PVS_NEED(d_out, "out");
  PVS_ALIGNED(d_nbr, 4, "nbr");
  PVS_ALIGNED(d_pos, 8, "pos");
  PVS_ALIGNED(d_out, 4, "out");
  const size_t nb = (size_t)N * kg * 4;
  if ((d_out != d_nbr && ranges_overlap(d_out, nb, d_nbr, nb)) || ranges_overlap(d_out, nb, d_keep, (size_t)N) ||
      ranges_overlap(d_out, nb, d_pos, (size_t)(N + 1) * 8))
    PVS_FAIL(PVS_ERR_INVALID, "%s: out overlaps an input (only out == nbr is served in place)", __func__);
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer tm(ctx, T_MISC);
  hipLaunchKernelGGL(df_remap_kernel, dim3(df_grid(N * kg)), dim3(DF_THREADS), 0, ctx->stream, d_nbr, N, kg, d_keep, d_pos, d_out);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

PVS_EXPORT int pvs_graph_gather_rows_dev(pvs_ctx* ctx, const void* d_rows, int64_t n, int64_t row_bytes, const int64_t* d_ids, int64_t b,
                                         void* d_out) {
  PVS_NEED(ctx, "ctx");
  if (n < 1 || b < 0 || row_bytes < 4 || row_bytes % 4 != 0)
    PVS_FAIL(PVS_ERR_INVALID, "%s: need n >= 1, b >= 0 and rows of a multiple of 4 bytes (got n=%lld, b=%lld, row_bytes=%lld)", __func__,
             (long long)n, (long long)b, (long long)row_bytes);
  if ((double)n * (double)row_bytes > 9e18 || (double)b * (double)(row_bytes / 4) > 5e11)
    PVS_FAIL(PVS_ERR_INVALID, "%s: the rows are too large", __func__);
  if (b == 0) return PVS_OK;
  PVS_NEED(d_rows, "rows");
  PVS_NEED(d_ids, "ids");
  PVS_NEED(d_out, "out");
  PVS_ALIGNED(d_rows, 4, "rows");
  PVS_ALIGNED(d_ids, 8, "ids");
  PVS_ALIGNED(d_out, 4, "out");
  const size_t ob = (size_t)b * (size_t)row_bytes;
  if (ranges_overlap(d_out, ob, d_rows, (size_t)n * (size_t)row_bytes) || ranges_overlap(d_out, ob, d_ids, (size_t)b * 8))
    PVS_FAIL(PVS_ERR_INVALID, "%s: out overlaps an input", __func__);
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer tm(ctx, T_MISC);
  const int64_t words = row_bytes / 4;
  hipLaunchKernelGGL(df_gather_rows_kernel, dim3(df_grid(b * words)), dim3(DF_THREADS), 0, ctx->stream, (const uint32_t*)d_rows, n, words,
                     d_ids, b, (uint32_t*)d_out);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

PVS_EXPORT int pvs_graph_affinity_sim_dev(pvs_ctx* ctx, const float* d_sim, int64_t N, int kg, int gamma, double* d_a) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(df_check_graph_shape(__func__, N, kg));
  if (gamma < 0 || gamma > DF_GAMMA_MAX) PVS_FAIL(PVS_ERR_INVALID, "%s: gamma must be in 0..%d (got %d)", __func__, DF_GAMMA_MAX, gamma);
  PVS_NEED(d_sim, "sim");
  PVS_NEED(d_a, "a");
  PVS_ALIGNED(d_sim, 4, "sim");
  PVS_ALIGNED(d_a, 8, "a");
  const size_t n = (size_t)N * kg;
  if (ranges_overlap(d_a, n * 8, d_sim, n * 4)) PVS_FAIL(PVS_ERR_INVALID, "%s: a overlaps sim", __func__);
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer tm(ctx, T_MISC);
  hipLaunchKernelGGL(df_affinity_sim_kernel, dim3(df_grid((int64_t)n)), dim3(DF_THREADS), 0, ctx->stream, d_sim, (int64_t)n, gamma, d_a);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

PVS_EXPORT int pvs_diffuse_rhs_dev(pvs_ctx* ctx, const int64_t* d_idx, const void* d_val, int val_f64, int64_t C, int kq, int64_t N, int gamma,
                                   double* d_Y) {
  PVS_NEED(ctx, "ctx");
  if (N < 1 || N >= ((int64_t)1 << 31)) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= N < 2^31 (got %lld)", __func__, (long long)N);
  if (kq < 1 || kq > N) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= kq <= N (got kq=%d, N=%lld)", __func__, kq, (long long)N);
  if (gamma < 0 || gamma > DF_GAMMA_MAX) PVS_FAIL(PVS_ERR_INVALID, "%s: gamma must be in 0..%d (got %d)", __func__, DF_GAMMA_MAX, gamma);
  if (C < 0 || (double)C * (double)N > 1e15) PVS_FAIL(PVS_ERR_INVALID, "%s: need 0 <= C and N C <= 10^15 (got C=%lld)", __func__, (long long)C);
  if (C == 0) return PVS_OK;
  PVS_NEED(d_idx, "idx");
  PVS_NEED(d_val, "val");
  PVS_NEED(d_Y, "Y");
  PVS_ALIGNED(d_idx, 8, "idx");
  PVS_ALIGNED(d_val, val_f64 ? 8 : 4, "val");
  PVS_ALIGNED(d_Y, 8, "Y");
  const size_t yb = (size_t)N * (size_t)C * 8, lb = (size_t)C * kq * 8;
  if (ranges_overlap(d_Y, yb, d_idx, lb) || ranges_overlap(d_Y, yb, d_val, val_f64 ? lb : lb / 2)) PVS_FAIL(PVS_ERR_INVALID, "%s: Y overlaps a list", __func__);
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer tm(ctx, T_MISC);
  PVS_HIP(hipMemsetAsync(d_Y, 0, yb, ctx->stream));
  if (val_f64)
    hipLaunchKernelGGL(df_rhs_kernel<double>, dim3(df_grid(C * kq)), dim3(DF_THREADS), 0, ctx->stream, d_idx, (const double*)d_val, C, kq, N,
                       gamma, d_Y);
  else
    hipLaunchKernelGGL(df_rhs_kernel<float>, dim3(df_grid(C * kq)), dim3(DF_THREADS), 0, ctx->stream, d_idx, (const float*)d_val, C, kq, N,
                       gamma, d_Y);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

static int df_check_solve_shape(const char* who, int64_t N, int64_t C) {
  if (N < 1 || N >= ((int64_t)1 << 31)) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= N < 2^31 (got %lld)", who, (long long)N);
  if (C < 1 || C > PVS_DIFFUSE_MAX_COLUMNS)
    PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= C <= %d columns per call (got %lld)", who, PVS_DIFFUSE_MAX_COLUMNS, (long long)C);
  if ((double)N * (double)C > 1e15) PVS_FAIL(PVS_ERR_INVALID, "%s: the vectors are too large", who);
  return PVS_OK;
}

PVS_EXPORT int pvs_diffuse_workspace(int64_t N, int64_t C, size_t* bytes) {
  PVS_TRY(df_check_solve_shape(__func__, N, C));
  PVS_NEED(bytes, "bytes");
  *bytes = df_layout(N, C).bytes;
  return PVS_OK;
}

PVS_EXPORT int pvs_diffuse_cg_dev(pvs_ctx* ctx, const int32_t* d_nbr, const double* d_s, int64_t N, int kg, const double* d_Y, int64_t C,
                                  double alpha, double tol, int maxiter, int check_every, int width, void* d_work, size_t work_bytes,
                                  double* d_X, int32_t* d_steps, double* d_rr, double* d_yy) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(df_check_solve_shape(__func__, N, C));
  if (kg < 1 || kg > N - 1 || (double)N * kg > 4e11)
    PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= kg <= N - 1 (got kg=%d, N=%lld)", __func__, kg, (long long)N);
  if (!(alpha > 0.0 && alpha < 1.0)) PVS_FAIL(PVS_ERR_INVALID, "%s: alpha must lie in (0, 1) (got %g)", __func__, alpha);
  if (!(tol >= 0.0) || !std::isfinite(tol)) PVS_FAIL(PVS_ERR_INVALID, "%s: tol must be finite and >= 0 (got %g)", __func__, tol);
  if (maxiter < 0) PVS_FAIL(PVS_ERR_INVALID, "%s: maxiter must be >= 0 (got %d)", __func__, maxiter);
  if (check_every < 1) PVS_FAIL(PVS_ERR_INVALID, "%s: check_every must be >= 1 (got %d)", __func__, check_every);
  if (width != 0 && width != 1 && width != 4 && width != 16 && width != 64)
    PVS_FAIL(PVS_ERR_INVALID, "%s: width must be 0 (chosen from C), 1, 4, 16 or 64 (got %d)", __func__, width);
  PVS_NEED(d_nbr, "nbr");
  PVS_NEED(d_s, "s");
  PVS_NEED(d_Y, "Y");
  PVS_NEED(d_work, "work");
  PVS_NEED(d_X, "X");
  PVS_NEED(d_steps, "steps");
  PVS_NEED(d_rr, "rr");
  PVS_NEED(d_yy, "yy");
  PVS_ALIGNED(d_nbr, 4, "nbr");
  PVS_ALIGNED(d_s, 8, "s");
  PVS_ALIGNED(d_Y, 8, "Y");
  PVS_ALIGNED(d_work, 256, "work");
  PVS_ALIGNED(d_X, 8, "X");
  PVS_ALIGNED(d_steps, 4, "steps");
  PVS_ALIGNED(d_rr, 8, "rr");
  PVS_ALIGNED(d_yy, 8, "yy");
  const DfLayout lay = df_layout(N, C);
  if (work_bytes < lay.bytes)
    PVS_FAIL(PVS_ERR_INVALID, "%s: the work buffer holds %zu bytes, pvs_diffuse_workspace asks for %zu", __func__, work_bytes, lay.bytes);
  const size_t vb = (size_t)N * (size_t)C * 8, gb = (size_t)N * kg;
  struct Range {
    const void* p;
    size_t n;
    bool out;
  } ranges[] = {{d_nbr, gb * 4, false}, {d_s, gb * 8, false}, {d_Y, vb, false},          {d_work, lay.bytes, true},
                {d_X, vb, true},        {d_steps, (size_t)C * 4, true}, {d_rr, (size_t)C * 8, true}, {d_yy, (size_t)C * 8, true}};
  for (const Range& o : ranges)
    for (const Range& q : ranges)
      if (o.out && &o != &q && ranges_overlap(o.p, o.n, q.p, q.n)) PVS_FAIL(PVS_ERR_INVALID, "%s: an output or the work buffer overlaps another array", __func__);
  const int cw = df_width(C, width);
  const int64_t nb = (N + DF_THREADS - 1) / DF_THREADS, chunks = (C + cw - 1) / cw;
  if (chunks > 65535) PVS_FAIL(PVS_ERR_INVALID, "%s: %lld columns at width %d are more than 65535 column chunks", __func__, (long long)C, cw);
  PVS_HIP(hipSetDevice(ctx->device));
  double *r = lay.r(d_work), *p = lay.p(d_work), *Ap = lay.Ap(d_work), *part = lay.part(d_work);
  DfCols st{d_rr, d_yy, lay.thr(d_work), lay.a(d_work), lay.b(d_work), lay.act(d_work), lay.upd(d_work), lay.retired(d_work), d_steps,
            lay.remaining(d_work)};
  const dim3 grid((unsigned)nb, (unsigned)chunks), block(DF_THREADS);
  ScopedTimer tm(ctx, T_MISC);
  PVS_TRY(df_dispatch_width(cw, [&](auto w) -> int {
    constexpr int CW = decltype(w)::value;
    hipLaunchKernelGGL(df_init_kernel<CW>, grid, block, 0, ctx->stream, d_Y, N, C, d_X, r, p, part);
    hipLaunchKernelGGL(df_reduce_kernel, dim3(1), block, 0, ctx->stream, 0, part, nb, C, tol, st);
    PVS_HIP(hipGetLastError());
    for (int it = 0; it < maxiter; ++it) {
      if (it % check_every == 0) {                       // only in order to stop launching: no bit depends on it
        int remaining = 0;
        PVS_HIP(hipMemcpyAsync(&remaining, st.remaining, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        PVS_HIP(hipStreamSynchronize(ctx->stream));
        if (remaining == 0) break;
      }
      hipLaunchKernelGGL(df_apply_kernel<CW>, grid, block, 0, ctx->stream, d_nbr, d_s, N, kg, C, alpha, p, st.act, Ap, part);
      hipLaunchKernelGGL(df_reduce_kernel, dim3(1), block, 0, ctx->stream, 1, part, nb, C, tol, st);
      hipLaunchKernelGGL(df_update_kernel<CW>, grid, block, 0, ctx->stream, N, C, st.a, st.act, p, Ap, d_X, r, part);
      hipLaunchKernelGGL(df_reduce_kernel, dim3(1), block, 0, ctx->stream, 2, part, nb, C, tol, st);
      hipLaunchKernelGGL(df_direction_kernel, dim3(df_grid(N * C)), block, 0, ctx->stream, N, C, st.b, st.upd, r, p);
      PVS_HIP(hipGetLastError());
    }
    return (int)PVS_OK;
  }));
  return PVS_OK;
}

PVS_EXPORT int pvs_rank_f64_dev(pvs_ctx* ctx, const double* d_scores, int64_t nq, int64_t ncols, int64_t ld, int k, int64_t* d_idx,
                                double* d_val) {
  PVS_NEED(ctx, "ctx");
  if (nq < 0 || ncols < 1 || ld < ncols) PVS_FAIL(PVS_ERR_INVALID, "%s: need nq >= 0, ncols >= 1, ld >= ncols", __func__);
  if (k < 1 || k > ncols) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= k <= ncols (got k=%d, ncols=%lld)", __func__, k, (long long)ncols);
  if (nq == 0) return PVS_OK;
  PVS_NEED(d_scores, "scores");
  PVS_NEED(d_idx, "idx");
  PVS_NEED(d_val, "val");
  PVS_ALIGNED(d_scores, 8, "scores");
  PVS_ALIGNED(d_idx, 8, "idx");
  PVS_ALIGNED(d_val, 8, "val");
  const size_t sb = (size_t)nq * (size_t)ld * 8, lb = (size_t)nq * k * 8;
  if (ranges_overlap(d_scores, sb, d_idx, lb) || ranges_overlap(d_scores, sb, d_val, lb) || ranges_overlap(d_idx, lb, d_val, lb))
    PVS_FAIL(PVS_ERR_INVALID, "%s: the arrays overlap", __func__);
  PVS_HIP(hipSetDevice(ctx->device));
  return launch_rank_f64(ctx, d_scores, nq, ncols, ld, k, d_idx, d_val);
}
