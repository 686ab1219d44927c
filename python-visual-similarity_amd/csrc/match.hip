// Spatial re-ranking: 2-NN matching of uint8 descriptor rows on the int8 matrix pipe, the ratio / mutual
// filter with an ordered compaction, and the exhaustive float64 geometric verification.  Every entry point covers a whole list of
// image pairs with a fixed number of launches, enqueues on the context's stream and does not wait for it.
#include <climits>

#include "common.hpp"

namespace pvs {
namespace {

using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x16 = __attribute__((ext_vector_type(16))) int;

constexpr int MT_THREADS = 256;   // four waves, each owning 32 rows of the A image
constexpr int MT_QROWS = 128;     // A rows of one workgroup
constexpr int MT_BN = 128;        // B rows of one LDS block (16 KiB)
constexpr int MT_D = 128;         // bytes per row

struct MatchTile {                // one workgroup of the matcher: up to MT_QROWS rows of one pair's A image
  int64_t a_row0;                 // first A row (global)
  int64_t b_row0;                 // first row of the B image (global)
  int64_t out0;                   // output position of a_row0
  int32_t n_a;                    // A rows of this tile (1..MT_QROWS)
  int32_t n_b;                    // rows of the B image
};

struct PairRec {                  // one image pair of the filter and the verification
  int64_t out_a;                  // sum of nA over the earlier pairs: position of the pair's per-row results and of its matches
  int64_t out_b;                  // the same over nB (results of the transposed matching)
  int64_t fa0, fb0;               // first row of the two images (frames)
  int32_t n_a, n_b;
};

__device__ __forceinline__ int sumsq_s8x4(int v) {
  const int a = (int)(int8_t)(v & 0xff), b = (int)(int8_t)((v >> 8) & 0xff), c = (int)(int8_t)((v >> 16) & 0xff), d = v >> 24;
  return a * a + b * b + c * c + d * d;
}
__device__ __forceinline__ int sumsq_s8x16(i32x4 v) { return sumsq_s8x4(v.x) + sumsq_s8x4(v.y) + sumsq_s8x4(v.z) + sumsq_s8x4(v.w); }

__device__ __forceinline__ i32x4 load_recentred(const uint8_t* p) {   // 16 bytes, x ^ 0x80 = x - 128 as int8
  const i32x4 v = *reinterpret_cast<const i32x4*>(p);
  const int m = (int)0x80808080u;
  return i32x4{v.x ^ m, v.y ^ m, v.z ^ m, v.w ^ m};
}

// d(i, j) = |a_i|^2 + |b_j|^2 - 2 a_i . b_j on re-centred bytes, exact in int32.  The B rows of an LDS block are the A operand of
// v_mfma_i32_32x32x32_i8 and the wave's 32 A rows ("queries") its B operand, so a lane's 16 accumulators are 16 B rows of ONE query
// (column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)): the running (best, index, second) of a query lives in the
// registers of its two lanes, is updated in ascending j with strict comparisons (ties keep the lowest j) and the two halves are
// merged once at the end.  Both operands take byte 32 s + 16 (lane >> 5) + e of their row as element e of k-step s, so the sum over
// the four steps is the full dot product whatever order the instruction gives the 32 values of a step.
__global__ __launch_bounds__(MT_THREADS) void match_u8_kernel(const uint8_t* __restrict__ rows_a, const uint8_t* __restrict__ rows_b,
                                                              const MatchTile* __restrict__ tiles, int32_t* __restrict__ out_idx,
                                                              int32_t* __restrict__ out_d1, int32_t* __restrict__ out_d2) {
  __shared__ __attribute__((aligned(16))) uint8_t s_rows[MT_BN * MT_D];
  __shared__ __attribute__((aligned(16))) int s_norm[MT_BN];
  const MatchTile t = tiles[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int q = wave * 32 + r;
  const bool q_valid = q < t.n_a;
  const bool wave_active = wave * 32 < t.n_a;

  i32x4 qf[4];
  int na = 0;
  for (int s = 0; s < 4; ++s) {
    qf[s] = q_valid ? load_recentred(rows_a + (t.a_row0 + q) * MT_D + 32 * s + 16 * h) : i32x4{0, 0, 0, 0};
    na += sumsq_s8x16(qf[s]);
  }
  na += __shfl_xor(na, 32, 64);

  int best = INT_MAX, second = INT_MAX, bidx = -1;

  // staging: thread -> 16-byte chunk (tid & 7) of rows (tid >> 3) + 32 u; the next block is fetched while this one is scanned
  const int ch = tid & 7, srow = tid >> 3;
  i32x4 pre[4];
  auto fetch = [&](int b0) {
    for (int u = 0; u < 4; ++u) {
      const int row = b0 + srow + 32 * u;
      pre[u] = row < t.n_b ? load_recentred(rows_b + (t.b_row0 + row) * MT_D + 16 * ch) : i32x4{0, 0, 0, 0};
    }
  };
  if (t.n_b > 0) fetch(0);
  for (int b0 = 0; b0 < t.n_b; b0 += MT_BN) {
    __syncthreads();                                     // the previous block has been scanned by every wave
    for (int u = 0; u < 4; ++u) {
      const int row = srow + 32 * u;
      *reinterpret_cast<i32x4*>(&s_rows[row * MT_D + ((ch ^ (row & 7)) << 4)]) = pre[u];
      int n = sumsq_s8x16(pre[u]);
      n += __shfl_xor(n, 1, 64);
      n += __shfl_xor(n, 2, 64);
      n += __shfl_xor(n, 4, 64);
      if (ch == 0) s_norm[row] = (b0 + row < t.n_b) ? n : INT_MAX;      // a padded row (all zero) scores INT_MAX - 2 * 0
    }
    __syncthreads();
    if (b0 + MT_BN < t.n_b) fetch(b0 + MT_BN);
    if (!wave_active) continue;
    const int n_sub = min(MT_BN / 32, (t.n_b - b0 + 31) / 32);
    for (int sub = 0; sub < n_sub; ++sub) {
      i32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      const int row = sub * 32 + r;
      for (int s = 0; s < 4; ++s) {
        const i32x4 bf = *reinterpret_cast<const i32x4*>(&s_rows[row * MT_D + (((2 * s + h) ^ (row & 7)) << 4)]);
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(bf, qf[s], acc, 0, 0, 0);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int jl = sub * 32 + 8 * g + 4 * h;
        const i32x4 nb = *reinterpret_cast<const i32x4*>(&s_norm[jl]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int d = nb[e] - 2 * acc[4 * g + e];
          second = min(second, max(d, best));
          bidx = d < best ? b0 + jl + e : bidx;
          best = min(best, d);
        }
      }
    }
  }
  // the other half of the query's B rows sits 32 lanes away
  const int o_best = __shfl_xor(best, 32, 64), o_second = __shfl_xor(second, 32, 64), o_idx = __shfl_xor(bidx, 32, 64);
  const bool take = o_best < best || (o_best == best && (unsigned)o_idx < (unsigned)bidx);
  second = min(min(second, o_second), max(best, o_best));
  best = min(best, o_best);
  bidx = take ? o_idx : bidx;
  if (h == 0 && q_valid) {
    out_idx[t.out0 + q] = bidx;
    out_d1[t.out0 + q] = bidx < 0 ? INT_MAX : best + na;
    out_d2[t.out0 + q] = second == INT_MAX ? INT_MAX : second + na;
  }
}

// keep row i of a pair iff idx >= 0, (double)d1 < ratio_sq * (double)d2 and (mutual) the B row's own best A row is i; the kept rows
// are written in ascending i behind a per-workgroup running prefix (ballots and a four-entry wave table: no atomics)
__global__ __launch_bounds__(256) void match_filter_kernel(const PairRec* __restrict__ pairs, const int32_t* __restrict__ idx,
                                                           const int32_t* __restrict__ d1, const int32_t* __restrict__ d2,
                                                           const int32_t* __restrict__ idx_rev, double ratio_sq, int mutual,
                                                           int32_t* __restrict__ matches, int32_t* __restrict__ counts) {
  __shared__ int s_wave[4];
  const PairRec p = pairs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base = 0;
  for (int c0 = 0; c0 < p.n_a; c0 += 256) {
    const int i = c0 + tid;
    bool keep = false;
    int j = -1;
    if (i < p.n_a) {
      j = idx[p.out_a + i];
      if (j >= 0 && j < p.n_b) {          // anything else is not a result of the matcher: dropped, never followed
        keep = (double)d1[p.out_a + i] < ratio_sq * (double)d2[p.out_a + i];
        if (keep && mutual) keep = idx_rev[p.out_b + j] == i;
      }
    }
    const unsigned long long bal = __ballot(keep);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wave] = __popcll(bal);
    __syncthreads();
    int off = base, total = 0;
    for (int w = 0; w < 4; ++w) {
      if (w < wave) off += s_wave[w];
      total += s_wave[w];
    }
    if (keep) {
      matches[2 * (p.out_a + off + before)] = i;
      matches[2 * (p.out_a + off + before) + 1] = j;
    }
    base += total;
    __syncthreads();
  }
  if (tid == 0) counts[blockIdx.x] = base;
}

// ---------------------------------------------------------------------------------------------------------------- verification
struct VPoint {          // one match in float64: its two points and its similarity hypothesis sigma (cos phi, sin phi)
  double ax, ay, bx, by;
  double c, s;           // NaN when the match gives no hypothesis
};

constexpr double VF_DEG = 3.14159265358979323846 / 180.0;

__global__ __launch_bounds__(256) void verify_prepare_kernel(const PairRec* __restrict__ pairs, const float* __restrict__ frames_a,
                                                             const float* __restrict__ frames_b, const int32_t* __restrict__ matches,
                                                             const int32_t* __restrict__ counts, VPoint* __restrict__ pts) {
#pragma clang fp contract(off)
  const PairRec p = pairs[blockIdx.x];
  const int m = min(counts[blockIdx.x], p.n_a);      // a pair never has more matches than A rows
  const int g = blockIdx.y * 256 + threadIdx.x;
  if (g >= m) return;
  const int mi = matches[2 * (p.out_a + g)], mj = matches[2 * (p.out_a + g) + 1];
  VPoint v;
  if (mi < 0 || mi >= p.n_a || mj < 0 || mj >= p.n_b) {       // not a match of this pair: no point, no hypothesis, never an inlier
    v.ax = v.ay = v.bx = v.by = v.c = v.s = __builtin_nan("");
    pts[p.out_a + g] = v;
    return;
  }
  const float* fa = frames_a + (p.fa0 + mi) * 6;
  const float* fb = frames_b + (p.fb0 + mj) * 6;
  v.ax = (double)fa[0];
  v.ay = (double)fa[1];
  v.bx = (double)fb[0];
  v.by = (double)fb[1];
  const double sa = (double)fa[2], sb = (double)fb[2], ta = (double)fa[3], tb = (double)fb[3];
  const bool ok = isfinite(v.ax) && isfinite(v.ay) && isfinite(v.bx) && isfinite(v.by) && isfinite(sa) && isfinite(sb) && isfinite(ta) &&
                  isfinite(tb) && sa > 0.0;
  if (ok) {
    const double sigma = sb / sa, phi = (tb - ta) * VF_DEG;
    v.c = sigma * cos(phi);
    v.s = sigma * sin(phi);
  } else {
    v.c = v.s = __builtin_nan("");
  }
  pts[p.out_a + g] = v;
}

// r^2(h, g) <= tol^2 for every g, one hypothesis per thread; the g loop reads the same point in every lane
__global__ __launch_bounds__(256) void verify_count_kernel(const PairRec* __restrict__ pairs, const int32_t* __restrict__ counts,
                                                           const VPoint* __restrict__ pts, double tol_sq, int32_t* __restrict__ hyp_count) {
#pragma clang fp contract(off)
  const PairRec p = pairs[blockIdx.x];
  const int m = min(counts[blockIdx.x], p.n_a);      // a pair never has more matches than A rows
  const int h = blockIdx.y * 256 + threadIdx.x;
  if (h >= m) return;
  const VPoint* P = pts + p.out_a;
  const VPoint vh = P[h];
  int n = 0;
  if (vh.c == vh.c) {
    for (int g = 0; g < m; ++g) {
      const double dax = P[g].ax - vh.ax, day = P[g].ay - vh.ay, dbx = P[g].bx - vh.bx, dby = P[g].by - vh.by;
      const double rx = (vh.c * dax - vh.s * day) - dbx, ry = (vh.s * dax + vh.c * day) - dby;
      n += (rx * rx + ry * ry <= tol_sq) ? 1 : 0;
    }
  }
  hyp_count[p.out_a + h] = n;
}

// fixed-shape tree over the workgroup: the same bits on every run
template <int N>
__device__ void block_sum(double (&v)[N], double* s_red) {
  const int tid = threadIdx.x;
  for (int k = 0; k < N; ++k) {
    __syncthreads();
    s_red[tid] = v[k];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (tid < w) s_red[tid] += s_red[tid + w];
      __syncthreads();
    }
    v[k] = s_red[0];
  }
}

__global__ __launch_bounds__(256) void verify_refine_kernel(const PairRec* __restrict__ pairs, const int32_t* __restrict__ counts,
                                                            const VPoint* __restrict__ pts, const int32_t* __restrict__ hyp_count,
                                                            double tol_sq, int rounds, uint8_t* __restrict__ tmp_mask,
                                                            int32_t* __restrict__ out_inliers, double* __restrict__ out_models,
                                                            int32_t* __restrict__ out_best, uint8_t* __restrict__ out_mask) {
#pragma clang fp contract(off)
  __shared__ double s_red[256];
  __shared__ int s_cnt[256], s_arg[256];
  const PairRec p = pairs[blockIdx.x];
  const int m = min(counts[blockIdx.x], p.n_a);      // a pair never has more matches than A rows
  const int tid = threadIdx.x;
  const VPoint* P = pts + p.out_a;
  uint8_t* mask = out_mask + p.out_a;
  uint8_t* tmp = tmp_mask + p.out_a;

  // best hypothesis: largest count, lowest h
  int bc = -1, bh = INT_MAX;
  for (int h = tid; h < m; h += 256) {
    const int c = hyp_count[p.out_a + h];
    if (c > bc) {
      bc = c;
      bh = h;
    }
  }
  s_cnt[tid] = bc;
  s_arg[tid] = bh;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      const int c = s_cnt[tid + w], a = s_arg[tid + w];
      if (c > s_cnt[tid] || (c == s_cnt[tid] && a < s_arg[tid])) {
        s_cnt[tid] = c;
        s_arg[tid] = a;
      }
    }
    __syncthreads();
  }
  int count = s_cnt[0];
  const int best = s_arg[0];
  if (m <= 0 || count <= 0) {
    for (int g = tid; g < m; g += 256) mask[g] = 0;
    if (tid == 0) {
      out_inliers[blockIdx.x] = 0;
      out_best[blockIdx.x] = -1;
      for (int k = 0; k < 6; ++k) out_models[6 * blockIdx.x + k] = 0.0;
    }
    return;
  }
  const VPoint vb = P[best];
  // the model in the form  r = M (p_a - ca) - (p_b - cb)
  double M00 = vb.c, M01 = -vb.s, M10 = vb.s, M11 = vb.c, cax = vb.ax, cay = vb.ay, cbx = vb.bx, cby = vb.by;
  for (int g = tid; g < m; g += 256) {
    const double dax = P[g].ax - cax, day = P[g].ay - cay, dbx = P[g].bx - cbx, dby = P[g].by - cby;
    const double rx = (M00 * dax + M01 * day) - dbx, ry = (M10 * dax + M11 * day) - dby;
    mask[g] = (rx * rx + ry * ry <= tol_sq) ? 1 : 0;
  }
  for (int round = 0; round < rounds && count >= 3; ++round) {
    double s5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int g = tid; g < m; g += 256)
      if (mask[g]) {
        s5[0] += 1.0;
        s5[1] += P[g].ax;
        s5[2] += P[g].ay;
        s5[3] += P[g].bx;
        s5[4] += P[g].by;
      }
    block_sum(s5, s_red);
    const double n = s5[0], max_ = s5[1] / n, may = s5[2] / n, mbx = s5[3] / n, mby = s5[4] / n;
    double s7[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // Cxx Cxy Cyy | Bxx Bxy Byx Byy  (B = sum b~ a~^T)
    for (int g = tid; g < m; g += 256)
      if (mask[g]) {
        const double ax = P[g].ax - max_, ay = P[g].ay - may, bx = P[g].bx - mbx, by = P[g].by - mby;
        s7[0] += ax * ax;
        s7[1] += ax * ay;
        s7[2] += ay * ay;
        s7[3] += bx * ax;
        s7[4] += bx * ay;
        s7[5] += by * ax;
        s7[6] += by * ay;
      }
    block_sum(s7, s_red);
    const double det = s7[0] * s7[2] - s7[1] * s7[1], tr = s7[0] + s7[2];
    if (!(det > 1e-12 * (tr * tr))) break;
    const double N00 = (s7[3] * s7[2] - s7[4] * s7[1]) / det, N01 = (s7[4] * s7[0] - s7[3] * s7[1]) / det;
    const double N10 = (s7[5] * s7[2] - s7[6] * s7[1]) / det, N11 = (s7[6] * s7[0] - s7[5] * s7[1]) / det;
    double s2[2] = {0.0, 0.0};                            // new count | changed entries
    for (int g = tid; g < m; g += 256) {
      const double dax = P[g].ax - max_, day = P[g].ay - may, dbx = P[g].bx - mbx, dby = P[g].by - mby;
      const double rx = (N00 * dax + N01 * day) - dbx, ry = (N10 * dax + N11 * day) - dby;
      const uint8_t in = (rx * rx + ry * ry <= tol_sq) ? 1 : 0;
      tmp[g] = in;
      s2[0] += in;
      s2[1] += (in != mask[g]) ? 1.0 : 0.0;
    }
    block_sum(s2, s_red);
    const int new_count = (int)s2[0];
    if (new_count < count) break;
    for (int g = tid; g < m; g += 256) mask[g] = tmp[g];     // each thread copies the entries it wrote itself
    M00 = N00, M01 = N01, M10 = N10, M11 = N11;
    cax = max_, cay = may, cbx = mbx, cby = mby;
    count = new_count;
    if (s2[1] == 0.0) break;
  }
  if (tid == 0) {
    out_inliers[blockIdx.x] = count;
    out_best[blockIdx.x] = best;
    double* o = out_models + 6 * blockIdx.x;
    o[0] = M00;
    o[1] = M01;
    o[2] = cbx - (M00 * cax + M01 * cay);
    o[3] = M10;
    o[4] = M11;
    o[5] = cby - (M10 * cax + M11 * cay);
  }
}

// ---------------------------------------------------------------------------------------------------------------- host side
int check_csr(const char* who, const int64_t* off, int64_t n_images, const char* name) {
  if (n_images < 0) PVS_FAIL(PVS_ERR_INVALID, "%s: negative image count (%s)", who, name);
  if (!off) PVS_FAIL(PVS_ERR_INVALID, "%s: null offsets (%s)", who, name);
  if (off[0] < 0) PVS_FAIL(PVS_ERR_INVALID, "%s: negative first offset (%s)", who, name);
  for (int64_t i = 0; i < n_images; ++i) {
    if (off[i + 1] < off[i]) PVS_FAIL(PVS_ERR_INVALID, "%s: offsets of %s decrease at image %lld", who, name, (long long)i);
    if (off[i + 1] - off[i] > (int64_t)INT_MAX / 4) PVS_FAIL(PVS_ERR_INVALID, "%s: image %lld of %s has too many rows", who, (long long)i, name);
  }
  return PVS_OK;
}

int check_pairs(const char* who, const int32_t* h_pairs, int64_t n_pairs, int64_t n_images_a, int64_t n_images_b) {
  if (!h_pairs) PVS_FAIL(PVS_ERR_INVALID, "%s: null pair list", who);
  if (n_pairs > INT_MAX / 2) PVS_FAIL(PVS_ERR_INVALID, "%s: too many pairs", who);
  for (int64_t p = 0; p < n_pairs; ++p) {
    const int32_t ia = h_pairs[2 * p], ib = h_pairs[2 * p + 1];
    if (ia < 0 || ia >= n_images_a || ib < 0 || ib >= n_images_b)
      PVS_FAIL(PVS_ERR_INVALID, "%s: pair %lld = (%d, %d) is outside the %lld x %lld images", who, (long long)p, ia, ib, (long long)n_images_a,
               (long long)n_images_b);
  }
  return PVS_OK;
}

// the pair table of the filter and the verification, copied to the device behind the work already queued
int upload_pairs(pvs_ctx* ctx, const int64_t* h_off_a, const int64_t* h_off_b, const int32_t* h_pairs, int64_t n_pairs, PairRec** d_pairs,
                 int64_t* total_a, int* max_a) {
  std::vector<PairRec> recs((size_t)n_pairs);
  int64_t oa = 0, ob = 0;
  int mx = 0;
  for (int64_t p = 0; p < n_pairs; ++p) {
    const int32_t ia = h_pairs[2 * p], ib = h_pairs[2 * p + 1];
    PairRec& r = recs[(size_t)p];
    r.out_a = oa;
    r.out_b = ob;
    r.fa0 = h_off_a[ia];
    r.fb0 = h_off_b[ib];
    r.n_a = (int32_t)(h_off_a[ia + 1] - h_off_a[ia]);
    r.n_b = (int32_t)(h_off_b[ib + 1] - h_off_b[ib]);
    oa += r.n_a;
    ob += r.n_b;
    mx = std::max(mx, (int)r.n_a);
  }
  PVS_TRY(ws_reserve(ctx, WS_MATCH_TABLE, recs.size() * sizeof(PairRec), d_pairs));
  PVS_HIP(hipMemcpyAsync(*d_pairs, recs.data(), recs.size() * sizeof(PairRec), hipMemcpyHostToDevice, ctx->stream));
  *total_a = oa;
  *max_a = mx;
  return PVS_OK;
}

}  // namespace
}  // namespace pvs

using namespace pvs;

PVS_EXPORT int pvs_match_u8_dev(pvs_ctx* ctx, const void* d_rows_a, const int64_t* h_off_a, int64_t n_images_a, const void* d_rows_b,
                                const int64_t* h_off_b, int64_t n_images_b, const int32_t* h_pairs, int64_t n_pairs, int32_t* d_idx,
                                int32_t* d_d1, int32_t* d_d2) {
  static const char* who = "pvs_match_u8_dev";
  if (!ctx) PVS_FAIL(PVS_ERR_INVALID, "%s: null ctx", who);
  if (n_pairs < 0) PVS_FAIL(PVS_ERR_INVALID, "%s: negative pair count", who);
  if (n_pairs == 0) return PVS_OK;
  PVS_TRY(check_csr(who, h_off_a, n_images_a, "A"));
  PVS_TRY(check_csr(who, h_off_b, n_images_b, "B"));
  PVS_TRY(check_pairs(who, h_pairs, n_pairs, n_images_a, n_images_b));
  if (((uintptr_t)d_rows_a | (uintptr_t)d_rows_b) & 15) PVS_FAIL(PVS_ERR_INVALID, "%s: descriptor rows must be 16-byte aligned", who);
  std::vector<MatchTile> tiles;
  int64_t out = 0;
  for (int64_t p = 0; p < n_pairs; ++p) {
    const int32_t ia = h_pairs[2 * p], ib = h_pairs[2 * p + 1];
    const int64_t na = h_off_a[ia + 1] - h_off_a[ia], nb = h_off_b[ib + 1] - h_off_b[ib];
    for (int64_t a0 = 0; a0 < na; a0 += MT_QROWS)
      tiles.push_back(MatchTile{h_off_a[ia] + a0, h_off_b[ib], out + a0, (int32_t)std::min<int64_t>(MT_QROWS, na - a0), (int32_t)nb});
    out += na;
  }
  if (tiles.empty()) return PVS_OK;
  if (tiles.size() > (size_t)INT_MAX) PVS_FAIL(PVS_ERR_INVALID, "%s: too many row tiles", who);
  if (!d_rows_a || !d_idx || !d_d1 || !d_d2) PVS_FAIL(PVS_ERR_INVALID, "%s: null rows or outputs", who);
  bool any_b = false;
  for (const MatchTile& t : tiles) any_b |= t.n_b > 0;
  if (any_b && !d_rows_b) PVS_FAIL(PVS_ERR_INVALID, "%s: null B rows", who);
  PVS_HIP(hipSetDevice(ctx->device));
  MatchTile* d_tiles = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_MATCH_TABLE, tiles.size() * sizeof(MatchTile), &d_tiles));
  // pageable source: the runtime has copied it out of `tiles` when the call returns
  PVS_HIP(hipMemcpyAsync(d_tiles, tiles.data(), tiles.size() * sizeof(MatchTile), hipMemcpyHostToDevice, ctx->stream));
  ScopedTimer tm(ctx, T_MISC);
  hipLaunchKernelGGL(match_u8_kernel, dim3((unsigned)tiles.size()), dim3(MT_THREADS), 0, ctx->stream, static_cast<const uint8_t*>(d_rows_a),
                     static_cast<const uint8_t*>(d_rows_b), d_tiles, d_idx, d_d1, d_d2);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

PVS_EXPORT int pvs_match_filter_dev(pvs_ctx* ctx, const int64_t* h_off_a, int64_t n_images_a, const int64_t* h_off_b, int64_t n_images_b,
                                    const int32_t* h_pairs, int64_t n_pairs, const int32_t* d_idx, const int32_t* d_d1, const int32_t* d_d2,
                                    const int32_t* d_idx_rev, double ratio_sq, int mutual, int32_t* d_matches, int32_t* d_match_counts) {
  static const char* who = "pvs_match_filter_dev";
  if (!ctx) PVS_FAIL(PVS_ERR_INVALID, "%s: null ctx", who);
  if (n_pairs < 0) PVS_FAIL(PVS_ERR_INVALID, "%s: negative pair count", who);
  if (!(ratio_sq >= 0.0)) PVS_FAIL(PVS_ERR_INVALID, "%s: ratio_sq must be >= 0", who);
  if (n_pairs == 0) return PVS_OK;
  PVS_TRY(check_csr(who, h_off_a, n_images_a, "A"));
  PVS_TRY(check_csr(who, h_off_b, n_images_b, "B"));
  PVS_TRY(check_pairs(who, h_pairs, n_pairs, n_images_a, n_images_b));
  if (!d_match_counts) PVS_FAIL(PVS_ERR_INVALID, "%s: null match counts", who);
  PVS_HIP(hipSetDevice(ctx->device));
  PairRec* d_pairs = nullptr;
  int64_t total_a = 0;
  int max_a = 0;
  PVS_TRY(upload_pairs(ctx, h_off_a, h_off_b, h_pairs, n_pairs, &d_pairs, &total_a, &max_a));
  if (total_a > 0 && (!d_idx || !d_d1 || !d_d2 || !d_matches)) PVS_FAIL(PVS_ERR_INVALID, "%s: null results or matches", who);
  if (total_a > 0 && mutual && !d_idx_rev) PVS_FAIL(PVS_ERR_INVALID, "%s: the mutual check needs the transposed matching", who);
  ScopedTimer tm(ctx, T_MISC);
  hipLaunchKernelGGL(match_filter_kernel, dim3((unsigned)n_pairs), dim3(256), 0, ctx->stream, d_pairs, d_idx, d_d1, d_d2, d_idx_rev, ratio_sq,
                     mutual ? 1 : 0, d_matches, d_match_counts);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

PVS_EXPORT int pvs_verify_dev(pvs_ctx* ctx, const float* d_frames_a, const int64_t* h_off_a, int64_t n_images_a, const float* d_frames_b,
                              const int64_t* h_off_b, int64_t n_images_b, const int32_t* h_pairs, int64_t n_pairs, const int32_t* d_matches,
                              const int32_t* d_match_counts, double tol, int refine_rounds, int32_t* d_inliers, double* d_models,
                              int32_t* d_best, uint8_t* d_mask) {
  static const char* who = "pvs_verify_dev";
  if (!ctx) PVS_FAIL(PVS_ERR_INVALID, "%s: null ctx", who);
  if (n_pairs < 0) PVS_FAIL(PVS_ERR_INVALID, "%s: negative pair count", who);
  if (!(tol >= 0.0) || !std::isfinite(tol)) PVS_FAIL(PVS_ERR_INVALID, "%s: tol must be a finite number >= 0", who);
  if (refine_rounds < 0) PVS_FAIL(PVS_ERR_INVALID, "%s: negative refine_rounds", who);
  if (n_pairs == 0) return PVS_OK;
  PVS_TRY(check_csr(who, h_off_a, n_images_a, "A"));
  PVS_TRY(check_csr(who, h_off_b, n_images_b, "B"));
  PVS_TRY(check_pairs(who, h_pairs, n_pairs, n_images_a, n_images_b));
  if (!d_match_counts || !d_inliers || !d_models || !d_best) PVS_FAIL(PVS_ERR_INVALID, "%s: null counts or outputs", who);
  PVS_HIP(hipSetDevice(ctx->device));
  PairRec* d_pairs = nullptr;
  int64_t total_a = 0;
  int max_a = 0;
  PVS_TRY(upload_pairs(ctx, h_off_a, h_off_b, h_pairs, n_pairs, &d_pairs, &total_a, &max_a));
  if (total_a > 0 && (!d_frames_a || !d_frames_b || !d_matches || !d_mask)) PVS_FAIL(PVS_ERR_INVALID, "%s: null frames, matches or mask", who);
  VPoint* d_pts = nullptr;
  char* d_small = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_VERIFY_POINTS, (size_t)total_a * sizeof(VPoint), &d_pts));
  WsLayout<4> lay;
  const auto hyp_p = lay.add<int32_t>((size_t)total_a);
  const auto tmp_p = lay.add<uint8_t>((size_t)total_a);
  PVS_TRY(ws_reserve(ctx, WS_VERIFY_SMALL, lay.bytes(), &d_small));
  int32_t* d_hyp = hyp_p(d_small);
  const double tol_sq = tol * tol;
  if ((max_a + 255) / 256 > 65535) PVS_FAIL(PVS_ERR_UNSUPPORTED, "%s: an image with %d rows is beyond the exhaustive search", who, max_a);
  const unsigned chunks = (unsigned)((max_a + 255) / 256);
  ScopedTimer tm(ctx, T_MISC);
  for (int64_t p0 = 0; p0 < n_pairs; p0 += 65535) {      // grid.y carries the chunks, grid.x the pairs
    const unsigned np = (unsigned)std::min<int64_t>(65535, n_pairs - p0);
    if (chunks) {
      hipLaunchKernelGGL(verify_prepare_kernel, dim3(np, chunks), dim3(256), 0, ctx->stream, d_pairs + p0, d_frames_a, d_frames_b, d_matches,
                         d_match_counts + p0, d_pts);
      PVS_HIP(hipGetLastError());
      hipLaunchKernelGGL(verify_count_kernel, dim3(np, chunks), dim3(256), 0, ctx->stream, d_pairs + p0, d_match_counts + p0, d_pts, tol_sq, d_hyp);
      PVS_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(verify_refine_kernel, dim3(np), dim3(256), 0, ctx->stream, d_pairs + p0, d_match_counts + p0, d_pts, d_hyp, tol_sq,
                       refine_rounds, tmp_p(d_small), d_inliers + p0, d_models + 6 * p0, d_best + p0, d_mask);
    PVS_HIP(hipGetLastError());
  }
  return PVS_OK;
}
