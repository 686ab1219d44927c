// k-reciprocal re-ranking on the kNN lists of a resident index (definitions in include/pvsim.h).
//
// The lists are those of a mutable graph (section 20): nbr int32 [N][kg], sim float32 [N][kg].  All weights are float64 with every
// multiply, add and divide rounded on its own, in the order the header states, so this unit is compiled with -ffp-contract=off, like
// diffuse.hip: a NumPy restatement gives the same bits.  The set work is integer work and has no order to keep.
//
// One wave owns one row (or one query): a workgroup is 64 threads.  k1 <= 64, so lane t holds slot t of the reciprocal set and a set
// is one ballot.  The expansion E of a row is never stored: a lane owns one member j of B, counts |H(j)| and |H(j) & B| from the two
// 64-bit masks of row j, and the qualifying members are one more ballot; the member flag of a slot and the count of dropped members
// then scan the rows of the qualifying members, which the wave has just read (they sit in L1 / L2).  The same routine serves a
// database row (its list in global memory) and a query (its list in LDS).
//
// The weights and the local expansion are one lane per row or per entry, like the graph kernels of diffuse.hip: sums of at most
// kg + 1 terms in slot order.  The score is one workgroup of sixteen waves per query with the query's list and expanded vector in LDS,
// one wave per candidate: a lane takes a slot of the candidate's row, finds the id in the query's list, and the wave adds the 64
// terms of a chunk in lane order through readlane, so the sum keeps the slot order of the header.  Terms that do not count are +0
// and every term is >= +0, so adding them changes no bit.
//
// No atomics; every output element is written once.  From list_common.hpp: ByteRange, outputs_overlap.
#include <algorithm>

#include "list_common.hpp"

namespace pvs {

constexpr int KR_WAVE = 64;
constexpr int KR_THREADS = 256;                 // the lane-per-entry kernels
constexpr int KR_SCORE_THREADS = 1024;          // sixteen waves share a query's candidates: the latency of one query is what counts
constexpr int KR_SCORE_WAVES = KR_SCORE_THREADS / KR_WAVE;
constexpr int KR_MAX_K1 = PVS_KRR_MAX_K1;
constexpr int KR_MAX_KQ = PVS_KRR_MAX_KQ;
constexpr int KR_GAMMA_MAX = 8;
static_assert(KR_MAX_K1 == KR_WAVE, "a reciprocal set is one ballot of a wave");

// the affinity of the GRAPH block (diffuse.hip holds the same few lines)
__device__ __forceinline__ double kr_affinity(double v, int gamma) {
  const double sp = v > 0.0 ? v : 0.0;   // a NaN counts as 0
  if (gamma == 0) return 1.0;
  double a = sp;
  for (int g = 1; g < gamma; ++g) a = a * sp;
  return a;
}

__device__ __forceinline__ bool kr_valid(int32_t j, int64_t N) { return (uint32_t)j < (uint32_t)N; }   // N < 2^31
__device__ __forceinline__ uint64_t kr_clip(uint64_t m, int kg) { return kg >= 64 ? m : m & ((1ull << kg) - 1); }   // no bit names a slot >= kg
__device__ __forceinline__ uint64_t kr_below(int s) { return (1ull << s) - 1; }                          // s < 64
__device__ __forceinline__ int kr_low(uint64_t m) { return __builtin_ctzll(m); }

static unsigned kr_grid(int64_t n) { return (unsigned)((n + KR_THREADS - 1) / KR_THREADS); }

// ---------------------------------------------------------------------------------------------------------------- sets
// one wave per row: lane t looks for the row in the first k1 slots of its t-th neighbour
__global__ __launch_bounds__(KR_WAVE) void kr_sets_kernel(const int32_t* __restrict__ nbr, int64_t N, int kg, int k1,
                                                          uint64_t* __restrict__ mask1, uint64_t* __restrict__ maskh) {
  const int64_t i = blockIdx.x;
  const int t = (int)threadIdx.x;
  const int k1h = (k1 + 1) / 2;
  int u = kg;                                     // no back slot
  if (t < k1) {
    const int32_t j = nbr[i * kg + t];
    if (kr_valid(j, N)) {
      const int32_t* lj = nbr + (int64_t)j * kg;
      for (int s = 0; s < k1; ++s)
        if (lj[s] == (int32_t)i) {
          u = s;
          break;
        }
    }
  }
  const uint64_t m1 = __ballot(t < k1 && u < k1), mh = __ballot(t < k1h && u < k1h);
  if (t == 0) {
    mask1[i] = m1;
    maskh[i] = mh;
  }
}

// The scans below compare every element and leave no loop early: a wave that owns a whole row or query is bound by the latency of
// its loads, and a loop that may leave after any of them issues them one at a time.

// whether id m sits in a slot of H(g) other than g itself
__device__ __forceinline__ bool kr_in_h(int32_t g, int32_t m, const int32_t* __restrict__ nbr, const uint64_t* __restrict__ maskh, int kg) {
  const int32_t* lg = nbr + (int64_t)g * kg;
  bool hit = false;
  for (uint64_t c = kr_clip(maskh[g], kg); c; c &= c - 1) hit |= lg[kr_low(c)] == m;
  return hit;
}

// the first p < n with list[p] == m, or n
__device__ __forceinline__ int kr_first(const int32_t* list, int n, int32_t m) {
  int f = n;
  for (int p = n - 1; p >= 0; --p) f = list[p] == m ? p : f;
  return f;
}

// One wave, all 64 lanes.  list[0 .. n): the ids of the row's (or the query's) own list, -1 in the empty slots; self: the row's own
// id, -1 for a query; bmask: the slots < 64 of the list that are reciprocal.  Bl: 64 ints of LDS.  -> flags[t] = 1 iff list[t] is a
// member of E other than self and t is the first slot holding it; returns (in every lane) the number of members of E that are
// neither self nor in the list.
__device__ __forceinline__ int kr_members_wave(const int32_t* list, int n, int32_t self, uint64_t bmask, const int32_t* __restrict__ nbr,
                                               const uint64_t* __restrict__ maskh, int64_t N, int kg, int32_t* Bl, uint8_t* flags) {
  const int lane = (int)threadIdx.x;
  int32_t j = -1;                                 // this lane's member of B \ {self}
  if (lane < n && ((bmask >> lane) & 1)) {
    j = list[lane];
    if (!kr_valid(j, N) || j == self) j = -1;
  }
  Bl[lane] = j;
  __syncthreads();
  // rule 3: 3 |H(j) & B| > 2 |H(j)|, both counted over distinct ids; j itself is in both
  bool qualifies = false;
  uint64_t mh = 0;
  const int32_t* lj = nbr;
  if (j >= 0) {
    mh = kr_clip(maskh[j], kg);
    lj = nbr + (int64_t)j * kg;
    int in_h = 1, in_both = 1;
    for (uint64_t a = mh; a; a &= a - 1) {
      const int s = kr_low(a);
      const int32_t h = lj[s];
      if (!kr_valid(h, N) || h == j) continue;
      bool dup = false;
      for (uint64_t b = mh & kr_below(s); b; b &= b - 1) dup |= lj[kr_low(b)] == h;
      if (dup) continue;
      ++in_h;
      bool in_b = h == self;
      for (int b = 0; b < KR_WAVE; ++b) in_b |= Bl[b] == h;
      in_both += in_b ? 1 : 0;
    }
    qualifies = 3 * in_both > 2 * in_h;
  }
  const uint64_t qual = __ballot(qualifies);
  // departure 1: the members that sit in the list, at their first slot
  for (int t = lane; t < n; t += KR_WAVE) {
    const int32_t m = list[t];
    bool in = false;
    if (kr_valid(m, N) && m != self) {
      if (kr_first(list, t, m) == t) {
        for (int b = 0; b < KR_WAVE; ++b) in |= Bl[b] == m;
        if (!in)
          for (uint64_t e = qual; e; e &= e - 1) in |= kr_in_h(Bl[kr_low(e)], m, nbr, maskh, kg);
      }
    }
    flags[t] = in ? 1 : 0;
  }
  // ... and those that do not: an id counts where it comes first, over the qualifying lanes in lane order and their slots in order
  int cnt = 0;
  if (qualifies)
    for (uint64_t a = mh; a; a &= a - 1) {
      const int s = kr_low(a);
      const int32_t h = lj[s];
      if (!kr_valid(h, N) || h == j || h == self) continue;
      bool known = kr_first(list, n, h) < n;          // most ids are: the scan of the other rows is the rare case
      if (!known) {
        for (uint64_t b = mh & kr_below(s); b; b &= b - 1) known |= lj[kr_low(b)] == h;
        for (uint64_t e = qual & kr_below(lane); e; e &= e - 1) known |= kr_in_h(Bl[kr_low(e)], h, nbr, maskh, kg);
      }
      cnt += known ? 0 : 1;
    }
  for (int o = KR_WAVE / 2; o; o >>= 1) cnt += __shfl_xor(cnt, o);
  return cnt;
}

__global__ __launch_bounds__(KR_WAVE) void kr_members_kernel(const int32_t* __restrict__ nbr, const uint64_t* __restrict__ mask1,
                                                             const uint64_t* __restrict__ maskh, int64_t N, int kg, uint8_t* __restrict__ flags,
                                                             int32_t* __restrict__ dropped) {
  __shared__ int32_t Bl[KR_WAVE];
  const int64_t i = blockIdx.x;
  const int cnt = kr_members_wave(nbr + i * kg, kg, (int32_t)i, kr_clip(mask1[i], kg), nbr, maskh, N, kg, Bl, flags + i * kg);
  if (threadIdx.x == 0) dropped[i] = cnt;
}

// ---------------------------------------------------------------------------------------------------------------- weights
// one lane per row: the sum from +0, self (exactly 1) first, then the members in slot order
__global__ __launch_bounds__(KR_THREADS) void kr_weights_kernel(const float* __restrict__ sim, const uint8_t* __restrict__ flags, int64_t N,
                                                                int kg, int gamma, double* __restrict__ v, double* __restrict__ v0) {
  const int64_t i = (int64_t)blockIdx.x * KR_THREADS + threadIdx.x;
  if (i >= N) return;
  double sum = 0.0 + 1.0;
  for (int t = 0; t < kg; ++t)
    if (flags[i * kg + t] != 0) sum = sum + kr_affinity((double)sim[i * kg + t], gamma);
  v0[i] = 1.0 / sum;
  for (int t = 0; t < kg; ++t) v[i * kg + t] = flags[i * kg + t] != 0 ? kr_affinity((double)sim[i * kg + t], gamma) / sum : 0.0;
}

// V_j[m]: v0[j] when m = j, v[j][first slot holding m] when m sits in row j, +0 otherwise
__device__ __forceinline__ double kr_vec(int32_t j, int32_t m, const int32_t* __restrict__ nbr, const double* __restrict__ v,
                                         const double* __restrict__ v0, int kg) {
  if (m == j) return v0[j];
  const int f = kr_first(nbr + (int64_t)j * kg, kg, m);
  return f < kg ? v[(int64_t)j * kg + f] : 0.0;
}

// one lane per element of the support: slots 0 .. kg - 1 of row i, and kg for i itself
__global__ __launch_bounds__(KR_THREADS) void kr_expand_kernel(const int32_t* __restrict__ nbr, const double* __restrict__ v,
                                                               const double* __restrict__ v0, int64_t N, int kg, int k2, double* __restrict__ w,
                                                               double* __restrict__ w0) {
  const int64_t e = (int64_t)blockIdx.x * KR_THREADS + threadIdx.x;
  if (e >= N * (kg + 1)) return;
  const int64_t i = e / (kg + 1);
  const int s = (int)(e - i * (kg + 1));
  const int32_t* li = nbr + i * kg;
  const int32_t m = s == kg ? (int32_t)i : li[s];
  double out = 0.0;
  if (kr_valid(m, N)) {
    double acc = 0.0 + kr_vec((int32_t)i, m, nbr, v, v0, kg);
    for (int t = 0; t < k2 - 1; ++t) {
      const int32_t j = li[t];
      if (kr_valid(j, N)) acc = acc + kr_vec(j, m, nbr, v, v0, kg);
    }
    out = acc / (double)k2;
  }
  if (s == kg) w0[i] = out;
  else w[i * kg + s] = out;
}

__global__ __launch_bounds__(KR_THREADS) void kr_rowsum_kernel(const double* __restrict__ w, const double* __restrict__ w0, int64_t N, int kg,
                                                               double* __restrict__ ws) {
  const int64_t i = (int64_t)blockIdx.x * KR_THREADS + threadIdx.x;
  if (i >= N) return;
  double sum = 0.0 + w0[i];
  for (int t = 0; t < kg; ++t) sum = sum + w[i * kg + t];
  ws[i] = sum;
}

// ---------------------------------------------------------------------------------------------------------------- query
// the LDS of the two query kernels follows kq (<= KR_MAX_KQ, 21.5 KiB then), so a short list does not cost occupancy
extern __shared__ __align__(16) unsigned char kr_lds[];
static size_t kr_query_lds_bytes(int kq) { return (size_t)kq * (8 + 8 + 4 + 1) + KR_WAVE * 4; }   // vq, wl, ids, memb + Bl
static size_t kr_score_lds_bytes(int kq) { return (size_t)kq * (8 + 4); }                          // wl, ids

// one wave per query; its list, member flags and the two vectors live in LDS
__global__ __launch_bounds__(KR_WAVE) void kr_query_kernel(const int32_t* __restrict__ nbr, const float* __restrict__ sim,
                                                           const uint64_t* __restrict__ maskh, const double* __restrict__ v,
                                                           const double* __restrict__ v0, int64_t N, int kg, int k1, int k2, int gamma,
                                                           const int64_t* __restrict__ qidx, const float* __restrict__ qval, int kq,
                                                           double* __restrict__ wq, double* __restrict__ sq, int32_t* __restrict__ kept,
                                                           int32_t* __restrict__ dropped) {
  double* vq = reinterpret_cast<double*>(kr_lds);            // kr_query_lds_bytes(kq)
  double* wl = vq + kq;
  int32_t* ids = reinterpret_cast<int32_t*>(wl + kq);
  int32_t* Bl = ids + kq;
  uint8_t* memb = reinterpret_cast<uint8_t*>(Bl + KR_WAVE);
  const int64_t q = blockIdx.x;
  const int lane = (int)threadIdx.x;
  const int64_t* qi = qidx + q * kq;
  const float* qv = qval + q * kq;
  for (int t = lane; t < kq; t += KR_WAVE) {
    const int64_t g = qi[t];
    ids[t] = (g >= 0 && g < N) ? (int32_t)g : -1;
  }
  __syncthreads();
  bool rec = false;                               // the query would enter g's first k1: float32 against float32, false for a NaN
  if (lane < k1 && lane < kq) {
    const int32_t g = ids[lane];
    if (g >= 0 && kr_valid(nbr[(int64_t)g * kg + k1 - 1], N)) rec = qv[lane] >= sim[(int64_t)g * kg + k1 - 1];
  }
  const uint64_t bmask = __ballot(rec);
  const int cnt = kr_members_wave(ids, kq, -1, bmask, nbr, maskh, N, kg, Bl, memb);
  __syncthreads();
  double sum = 0.0;                               // every lane adds the same numbers in slot order
  int members = 0;
  for (int t = 0; t < kq; ++t)
    if (memb[t] != 0) {
      sum = sum + kr_affinity((double)qv[t], gamma);
      ++members;
    }
  for (int t = lane; t < kq; t += KR_WAVE) vq[t] = (memb[t] != 0 && sum > 0.0) ? kr_affinity((double)qv[t], gamma) / sum : 0.0;
  __syncthreads();
  const int src = k2 - 1 < kq ? k2 - 1 : kq;
  for (int t = lane; t < kq; t += KR_WAVE) {
    const int32_t m = ids[t];
    double out = 0.0;
    if (m >= 0) {
      double acc = 0.0 + vq[kr_first(ids, t, m)];       // t itself where no earlier slot holds m
      for (int p = 0; p < src; ++p) {
        const int32_t g = ids[p];
        if (g >= 0) acc = acc + kr_vec(g, m, nbr, v, v0, kg);
      }
      out = acc / (double)k2;
    }
    wl[t] = out;
    wq[q * kq + t] = out;
  }
  __syncthreads();
  double total = 0.0;
  for (int t = 0; t < kq; ++t) total = total + wl[t];
  if (lane == 0) {
    sq[q] = total;
    kept[q] = members;
    dropped[q] = cnt;
  }
}

// one workgroup of sixteen waves per query, one wave per candidate
__global__ __launch_bounds__(KR_SCORE_THREADS) void kr_score_kernel(const int32_t* __restrict__ nbr, const double* __restrict__ w,
                                                                    const double* __restrict__ w0, const double* __restrict__ ws, int64_t N, int kg,
                                                                    const int64_t* __restrict__ qidx, const float* __restrict__ qval,
                                                                    const double* __restrict__ wq, const double* __restrict__ sq, int kq, int kr,
                                                                    double one_minus_lam, double lam, double* __restrict__ scores) {
  double* wl = reinterpret_cast<double*>(kr_lds);            // kr_score_lds_bytes(kq)
  int32_t* ids = reinterpret_cast<int32_t*>(wl + kq);
  const int64_t q = blockIdx.x;
  const int lane = (int)threadIdx.x % KR_WAVE, wave = (int)threadIdx.x / KR_WAVE;
  for (int t = (int)threadIdx.x; t < kq; t += KR_SCORE_THREADS) {
    const int64_t g = qidx[q * kq + t];
    ids[t] = (g >= 0 && g < N) ? (int32_t)g : -1;
    wl[t] = wq[q * kq + t];
  }
  __syncthreads();
  const double sqv = sq[q];
  for (int r = wave; r < kr; r += KR_SCORE_WAVES) {          // r and c are the same in every lane of a wave
    const int32_t c = ids[r];
    double J = 0.0;
    if (c >= 0) {
      const int32_t* lc = nbr + (int64_t)c * kg;
      const double* wc = w + (int64_t)c * kg;
      const double a0 = wl[kr_first(ids, r, c)], b0 = w0[c];
      double m_sum = 0.0 + (b0 < a0 ? b0 : a0);
      for (int base = 0; base < kg; base += KR_WAVE) {
        const int s = base + lane;
        double term = 0.0;
        if (s < kg) {
          const int32_t m = lc[s];
          if (kr_valid(m, N) && m != c) {
            const int p = kr_first(ids, kq, m);
            if (p < kq && kr_first(lc, s, m) == s) {
              const double a = wl[p], b = wc[s];
              term = b < a ? b : a;
            }
          }
        }
        const int nn = kg - base < KR_WAVE ? kg - base : KR_WAVE;
        for (int l = 0; l < nn; ++l) m_sum = m_sum + __shfl(term, l);
      }
      const double den = (sqv + ws[c]) - m_sum;
      J = den > 0.0 ? m_sum / den : 0.0;
    }
    if (lane == 0) scores[q * kr + r] = one_minus_lam * J + lam * (double)qval[q * kq + r];
  }
}

static int kr_check_shape(const char* who, int64_t N, int kg) {
  if (N < 2 || N >= ((int64_t)1 << 31)) PVS_FAIL(PVS_ERR_INVALID, "%s: need 2 <= N < 2^31 (got N=%lld)", who, (long long)N);
  if (kg < 1 || kg > N - 1) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= kg <= N - 1 (got kg=%d, N=%lld)", who, kg, (long long)N);
  if ((double)N * kg > 4e11) PVS_FAIL(PVS_ERR_INVALID, "%s: the lists are too large", who);
  return PVS_OK;
}

static int kr_check_k1(const char* who, int kg, int k1) {
  if (k1 < 1 || k1 > kg || k1 > KR_MAX_K1) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= k1 <= min(kg, %d) (got k1=%d, kg=%d)", who, KR_MAX_K1, k1, kg);
  return PVS_OK;
}

static int kr_check_overlap(const char* who, const ByteRange* outs, int n_out, const ByteRange* ins, int n_in) {
  const int o = outputs_overlap(outs, n_out, ins, n_in);
  if (o == 1) PVS_FAIL(PVS_ERR_INVALID, "%s: an output overlaps an input", who);
  if (o == 2) PVS_FAIL(PVS_ERR_INVALID, "%s: two outputs overlap", who);
  return PVS_OK;
}

}  // namespace pvs

using namespace pvs;

PVS_EXPORT int pvs_krr_sets_dev(pvs_ctx* ctx, const int32_t* d_nbr, int64_t N, int kg, int k1, uint64_t* d_mask1, uint64_t* d_maskh) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(kr_check_shape(__func__, N, kg));
  PVS_TRY(kr_check_k1(__func__, kg, k1));
  PVS_NEED(d_nbr, "nbr");
  PVS_NEED(d_mask1, "mask1");
  PVS_NEED(d_maskh, "maskh");
  PVS_ALIGNED(d_nbr, 4, "nbr");
  PVS_ALIGNED(d_mask1, 8, "mask1");
  PVS_ALIGNED(d_maskh, 8, "maskh");
  const ByteRange ins[] = {{d_nbr, N * kg * 4}}, outs[] = {{d_mask1, N * 8}, {d_maskh, N * 8}};
  PVS_TRY(kr_check_overlap(__func__, outs, 2, ins, 1));
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer tm(ctx, T_MISC);
  hipLaunchKernelGGL(kr_sets_kernel, dim3((unsigned)N), dim3(KR_WAVE), 0, ctx->stream, d_nbr, N, kg, k1, d_mask1, d_maskh);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

PVS_EXPORT int pvs_krr_members_dev(pvs_ctx* ctx, const int32_t* d_nbr, const uint64_t* d_mask1, const uint64_t* d_maskh, int64_t N, int kg,
                                   uint8_t* d_members, int32_t* d_dropped) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(kr_check_shape(__func__, N, kg));
  PVS_NEED(d_nbr, "nbr");
  PVS_NEED(d_mask1, "mask1");
  PVS_NEED(d_maskh, "maskh");
  PVS_NEED(d_members, "members");
  PVS_NEED(d_dropped, "dropped");
  PVS_ALIGNED(d_nbr, 4, "nbr");
  PVS_ALIGNED(d_mask1, 8, "mask1");
  PVS_ALIGNED(d_maskh, 8, "maskh");
  PVS_ALIGNED(d_dropped, 4, "dropped");
  const ByteRange ins[] = {{d_nbr, N * kg * 4}, {d_mask1, N * 8}, {d_maskh, N * 8}}, outs[] = {{d_members, N * kg}, {d_dropped, N * 4}};
  PVS_TRY(kr_check_overlap(__func__, outs, 2, ins, 3));
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer tm(ctx, T_MISC);
  hipLaunchKernelGGL(kr_members_kernel, dim3((unsigned)N), dim3(KR_WAVE), 0, ctx->stream, d_nbr, d_mask1, d_maskh, N, kg, d_members, d_dropped);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

PVS_EXPORT int pvs_krr_weights_dev(pvs_ctx* ctx, const float* d_sim, const uint8_t* d_members, int64_t N, int kg, int gamma, double* d_v,
                                   double* d_v0) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(kr_check_shape(__func__, N, kg));
  if (gamma < 0 || gamma > KR_GAMMA_MAX) PVS_FAIL(PVS_ERR_INVALID, "%s: gamma must be in 0..%d (got %d)", __func__, KR_GAMMA_MAX, gamma);
  PVS_NEED(d_sim, "sim");
  PVS_NEED(d_members, "members");
  PVS_NEED(d_v, "v");
  PVS_NEED(d_v0, "v0");
  PVS_ALIGNED(d_sim, 4, "sim");
  PVS_ALIGNED(d_v, 8, "v");
  PVS_ALIGNED(d_v0, 8, "v0");
  const ByteRange ins[] = {{d_sim, N * kg * 4}, {d_members, N * kg}}, outs[] = {{d_v, N * kg * 8}, {d_v0, N * 8}};
  PVS_TRY(kr_check_overlap(__func__, outs, 2, ins, 2));
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer tm(ctx, T_MISC);
  hipLaunchKernelGGL(kr_weights_kernel, dim3(kr_grid(N)), dim3(KR_THREADS), 0, ctx->stream, d_sim, d_members, N, kg, gamma, d_v, d_v0);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

PVS_EXPORT int pvs_krr_expand_dev(pvs_ctx* ctx, const int32_t* d_nbr, const double* d_v, const double* d_v0, int64_t N, int kg, int k2,
                                  double* d_w, double* d_w0, double* d_ws) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(kr_check_shape(__func__, N, kg));
  if (k2 < 1 || k2 > kg + 1) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= k2 <= kg + 1 (got k2=%d, kg=%d)", __func__, k2, kg);
  PVS_NEED(d_nbr, "nbr");
  PVS_NEED(d_v, "v");
  PVS_NEED(d_v0, "v0");
  PVS_NEED(d_w, "w");
  PVS_NEED(d_w0, "w0");
  PVS_NEED(d_ws, "ws");
  PVS_ALIGNED(d_nbr, 4, "nbr");
  PVS_ALIGNED(d_v, 8, "v");
  PVS_ALIGNED(d_v0, 8, "v0");
  PVS_ALIGNED(d_w, 8, "w");
  PVS_ALIGNED(d_w0, 8, "w0");
  PVS_ALIGNED(d_ws, 8, "ws");
  const ByteRange ins[] = {{d_nbr, N * kg * 4}, {d_v, N * kg * 8}, {d_v0, N * 8}}, outs[] = {{d_w, N * kg * 8}, {d_w0, N * 8}, {d_ws, N * 8}};
  PVS_TRY(kr_check_overlap(__func__, outs, 3, ins, 3));
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer tm(ctx, T_MISC);
  hipLaunchKernelGGL(kr_expand_kernel, dim3(kr_grid(N * (kg + 1))), dim3(KR_THREADS), 0, ctx->stream, d_nbr, d_v, d_v0, N, kg, k2, d_w, d_w0);
  hipLaunchKernelGGL(kr_rowsum_kernel, dim3(kr_grid(N)), dim3(KR_THREADS), 0, ctx->stream, d_w, d_w0, N, kg, d_ws);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

PVS_EXPORT int pvs_krr_query_dev(pvs_ctx* ctx, const int32_t* d_nbr, const float* d_sim, const uint64_t* d_maskh, const double* d_v,
                                 const double* d_v0, int64_t N, int kg, int k1, int k2, int gamma, const int64_t* d_qidx, const float* d_qval,
                                 int64_t nq, int kq, double* d_wq, double* d_sq, int32_t* d_kept, int32_t* d_dropped) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(kr_check_shape(__func__, N, kg));
  PVS_TRY(kr_check_k1(__func__, kg, k1));
  if (k2 < 1 || k2 > kg + 1) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= k2 <= kg + 1 (got k2=%d, kg=%d)", __func__, k2, kg);
  if (gamma < 0 || gamma > KR_GAMMA_MAX) PVS_FAIL(PVS_ERR_INVALID, "%s: gamma must be in 0..%d (got %d)", __func__, KR_GAMMA_MAX, gamma);
  if (kq < 1 || kq > N || kq > KR_MAX_KQ) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= kq <= min(N, %d) (got kq=%d)", __func__, KR_MAX_KQ, kq);
  if (nq < 0 || nq >= ((int64_t)1 << 31)) PVS_FAIL(PVS_ERR_INVALID, "%s: need 0 <= nq < 2^31 (got %lld)", __func__, (long long)nq);
  if (nq == 0) return PVS_OK;
  PVS_NEED(d_nbr, "nbr");
  PVS_NEED(d_sim, "sim");
  PVS_NEED(d_maskh, "maskh");
  PVS_NEED(d_v, "v");
  PVS_NEED(d_v0, "v0");
  PVS_NEED(d_qidx, "qidx");
  PVS_NEED(d_qval, "qval");
  PVS_NEED(d_wq, "wq");
  PVS_NEED(d_sq, "sq");
  PVS_NEED(d_kept, "kept");
  PVS_NEED(d_dropped, "dropped");
  PVS_ALIGNED(d_nbr, 4, "nbr");
  PVS_ALIGNED(d_sim, 4, "sim");
  PVS_ALIGNED(d_maskh, 8, "maskh");
  PVS_ALIGNED(d_v, 8, "v");
  PVS_ALIGNED(d_v0, 8, "v0");
  PVS_ALIGNED(d_qidx, 8, "qidx");
  PVS_ALIGNED(d_qval, 4, "qval");
  PVS_ALIGNED(d_wq, 8, "wq");
  PVS_ALIGNED(d_sq, 8, "sq");
  PVS_ALIGNED(d_kept, 4, "kept");
  PVS_ALIGNED(d_dropped, 4, "dropped");
  const ByteRange ins[] = {{d_nbr, N * kg * 4}, {d_sim, N * kg * 4}, {d_maskh, N * 8},  {d_v, N * kg * 8},
                           {d_v0, N * 8},       {d_qidx, nq * kq * 8}, {d_qval, nq * kq * 4}},
                  outs[] = {{d_wq, nq * kq * 8}, {d_sq, nq * 8}, {d_kept, nq * 4}, {d_dropped, nq * 4}};
  PVS_TRY(kr_check_overlap(__func__, outs, 4, ins, 7));
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer tm(ctx, T_MISC);
  hipLaunchKernelGGL(kr_query_kernel, dim3((unsigned)nq), dim3(KR_WAVE), kr_query_lds_bytes(kq), ctx->stream, d_nbr, d_sim, d_maskh, d_v, d_v0, N, kg, k1, k2, gamma,
                     d_qidx, d_qval, kq, d_wq, d_sq, d_kept, d_dropped);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

PVS_EXPORT int pvs_krr_score_dev(pvs_ctx* ctx, const int32_t* d_nbr, const double* d_w, const double* d_w0, const double* d_ws, int64_t N,
                                 int kg, const int64_t* d_qidx, const float* d_qval, const double* d_wq, const double* d_sq, int64_t nq, int kq,
                                 int kr, double lam, double* d_scores) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(kr_check_shape(__func__, N, kg));
  if (kq < 1 || kq > N || kq > KR_MAX_KQ) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= kq <= min(N, %d) (got kq=%d)", __func__, KR_MAX_KQ, kq);
  if (kr < 1 || kr > kq) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= kr <= kq (got kr=%d, kq=%d)", __func__, kr, kq);
  if (!(lam >= 0.0 && lam <= 1.0)) PVS_FAIL(PVS_ERR_INVALID, "%s: lambda must lie in [0, 1] (got %g)", __func__, lam);
  if (nq < 0 || nq >= ((int64_t)1 << 31)) PVS_FAIL(PVS_ERR_INVALID, "%s: need 0 <= nq < 2^31 (got %lld)", __func__, (long long)nq);
  if (nq == 0) return PVS_OK;
  PVS_NEED(d_nbr, "nbr");
  PVS_NEED(d_w, "w");
  PVS_NEED(d_w0, "w0");
  PVS_NEED(d_ws, "ws");
  PVS_NEED(d_qidx, "qidx");
  PVS_NEED(d_qval, "qval");
  PVS_NEED(d_wq, "wq");
  PVS_NEED(d_sq, "sq");
  PVS_NEED(d_scores, "scores");
  PVS_ALIGNED(d_nbr, 4, "nbr");
  PVS_ALIGNED(d_w, 8, "w");
  PVS_ALIGNED(d_w0, 8, "w0");
  PVS_ALIGNED(d_ws, 8, "ws");
  PVS_ALIGNED(d_qidx, 8, "qidx");
  PVS_ALIGNED(d_qval, 4, "qval");
  PVS_ALIGNED(d_wq, 8, "wq");
  PVS_ALIGNED(d_sq, 8, "sq");
  PVS_ALIGNED(d_scores, 8, "scores");
  const ByteRange ins[] = {{d_nbr, N * kg * 4},   {d_w, N * kg * 8},     {d_w0, N * 8},        {d_ws, N * 8},
                           {d_qidx, nq * kq * 8}, {d_qval, nq * kq * 4}, {d_wq, nq * kq * 8}, {d_sq, nq * 8}},
                  outs[] = {{d_scores, nq * kr * 8}};
  PVS_TRY(kr_check_overlap(__func__, outs, 1, ins, 8));
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer tm(ctx, T_MISC);
  hipLaunchKernelGGL(kr_score_kernel, dim3((unsigned)nq), dim3(KR_SCORE_THREADS), kr_score_lds_bytes(kq), ctx->stream, d_nbr, d_w, d_w0, d_ws, N, kg, d_qidx, d_qval, d_wq,
                     d_sq, kq, kr, 1.0 - lam, lam, d_scores);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}
