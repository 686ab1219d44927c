// Local-descriptor retrieval: the aggregated selective match kernel with binary signatures, ASMK* of Tolias,
// Avrithis and Jegou (ICCV 2013), on top of Jegou's Hamming embedding.
//   pvs_asmk_aggregate_dev   rows + labels of a batch of images -> per image its entries (visual word, B-bit signature of the summed
//                            residual), words ascending
//   pvs_asmk_aggregate_ma_dev   the same with m labels per row (multiple assignment of a query's rows, pvs_kmeans_topm_dev)
//   pvs_asmk_score_dev       the entries of nq queries x an inverted file over words -> the score panel [nq][N]; the ranking is
//                            pvs_topk_dev on that panel
// Every value is DEFINED in include/pvsim.h: the residual sum is float32 in row order with separate roundings (this unit is compiled
// with -ffp-contract=off), the score is a sum of integers, exact in uint32, so the scan may be cut anywhere and may use atomics.
// tests/asmk_numpy.py restates both.  From list_common.hpp: the block scan, the lane searches, signatures, QueryOffsets, the score slice.
#include <algorithm>

#include "desc_load.hpp"
#include "list_common.hpp"

namespace pvs {

constexpr int ASMK_THREADS = 512;
constexpr int ASMK_WAVES = ASMK_THREADS / WAVE;
constexpr int ASMK_MAX_ROWS = 8192;            // rows of one image: 8192 keys of 8 bytes are 64 KiB of LDS
constexpr int ASMK_MAX_D = 128;
constexpr int ASMK_MAX_M = 8;                  // labels per row (pvs_asmk_aggregate_ma_dev)
constexpr int ASMK_MAX_KEYS = 16384;           // rows x labels of one image: 16384 keys of 4 bytes are 64 KiB, their heads 32 KiB
constexpr size_t ASMK_LDS_BUDGET = 160 * 1024 - 64;   // dynamic LDS of the aggregate kernel beside its static words

// ------------------------------------------------------------------------------------------------- aggregate
// One workgroup per image.  LDS: keys [npad] (label and row in one integer), heads uint16 [npad] (first position of every run of equal
// labels), then P transposed float [D][B] when there is a projection.  The keys are sorted by a bitonic network; the padding keys
// (all ones) sort last.  Wave v takes the runs v, v + 8, ...: lanes over t, rows in ascending j (the low part of the key).
//
// MA = false (pvs_asmk_aggregate_dev): one label per row, keys uint64 label << 32 | row, up to 8192 of them.
// MA = true (pvs_asmk_aggregate_ma_dev): m distinct labels per row, labels [row][m]; key i of the image is label << 13 | (i / m), a
// uint32 (row < 8192, label < 65536: 29 bits), up to 16384 of them = 64 KiB, heads 32 KiB.  A run of equal labels is then the rows
// that hold the word in any slot, ascending.  Where keys, heads and the transposed projection do not fit the 160 KiB together
// (p_lds == 0) the projection is read from global memory as it lies, [B][D]: 64 KiB at most, resident in L2.
template <bool MA>
struct AsmkKey {
  using type = unsigned long long;
  static constexpr int SHIFT = 32;
};
template <>
struct AsmkKey<true> {
  using type = uint32_t;
  static constexpr int SHIFT = 13;
};

template <int KIND, bool MA = false>
__global__ __launch_bounds__(ASMK_THREADS) void asmk_aggregate_kernel(const void* __restrict__ X, int D,
                                                                       const int64_t* __restrict__ offsets,
                                                                       const int32_t* __restrict__ labels,
                                                                       const float* __restrict__ cent, int K,
                                                                       const float* __restrict__ P, int B, int npad,
                                                                       int32_t* __restrict__ ent_word, uint32_t* __restrict__ ent_sig,
                                                                       int32_t* __restrict__ ent_count, int m, int p_lds) {
  using key_t = typename AsmkKey<MA>::type;
  constexpr int SHIFT = AsmkKey<MA>::SHIFT;
  constexpr key_t ROW_MASK = ((key_t)1 << SHIFT) - 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char asmk_lds[];
  __shared__ int stmp[ASMK_WAVES];
  key_t* keys = reinterpret_cast<key_t*>(asmk_lds);
  unsigned short* heads = reinterpret_cast<unsigned short*>(asmk_lds + (size_t)npad * sizeof(key_t));
  float* Pt = reinterpret_cast<float*>(asmk_lds + (size_t)npad * (sizeof(key_t) + 2));   // npad is a multiple of 64: 4-byte aligned
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t img = blockIdx.x;
  const int64_t r0 = offsets[img];
  const int mm = MA ? m : 1;
  const int n = (int)min((int64_t)npad, (offsets[img + 1] - r0) * mm);   // keys of the image; the host has checked n <= npad
  if (n <= 0) {
    if (tid == 0) ent_count[img] = 0;
    return;
  }
  const bool p_staged = P != nullptr && (!MA || p_lds != 0);
  if (p_staged)
    for (int i = tid; i < B * D; i += ASMK_THREADS) {
      const int t = i / D, u = i - t * D;
      Pt[u * B + t] = P[i];
    }
  // element (t, u) of the projection is pm[u * p_su + t * p_st]
  const bool p_t = !MA || p_staged;   // MA = false: always the transposed copy in LDS
  const float* pm = p_t ? Pt : P;
  const int p_su = p_t ? B : 1, p_st = p_t ? 1 : D;
  for (int i = tid; i < npad; i += ASMK_THREADS) {
    if constexpr (MA) keys[i] = i < n ? ((key_t)(unsigned)labels[r0 * mm + i] << SHIFT) | (key_t)(i / mm) : ~(key_t)0;
    else keys[i] = i < n ? ((key_t)(unsigned)labels[r0 + i] << SHIFT) | (unsigned)i : ~(key_t)0;
  }
  __syncthreads();
  for (int k = 2; k <= npad; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < npad; i += ASMK_THREADS) {
        const int o = i ^ j;
        if (o > i) {
          const key_t a = keys[i], b = keys[o];
          if ((a > b) == ((i & k) == 0)) {
            keys[i] = b;
            keys[o] = a;
          }
        }
      }
      __syncthreads();
    }

  // ---- run heads: thread `tid` owns the positions [tid per, (tid + 1) per)
  const int per = npad / ASMK_THREADS > 0 ? npad / ASMK_THREADS : 1;
  const int p_lo = tid * per, p_hi = min(p_lo + per, n);
  int mine = 0;
  for (int p = p_lo; p < p_hi; ++p) mine += (p == 0 || (keys[p] >> SHIFT) != (keys[p - 1] >> SHIFT)) ? 1 : 0;
  int E;
  int before = block_excl_scan<ASMK_WAVES, false>(mine, stmp, lane, wave, E);   // stmp is not written again
  for (int p = p_lo; p < p_hi; ++p)
    if (p == 0 || (keys[p] >> SHIFT) != (keys[p - 1] >> SHIFT)) heads[before++] = (unsigned short)p;
  __syncthreads();
  if (tid == 0) ent_count[img] = E;

  const int W = B >> 5;
  const bool two = D > 64;
  for (int e = wave; e < E; e += ASMK_WAVES) {
    const int p0 = heads[e], p1 = e + 1 < E ? (int)heads[e + 1] : n;
    const int w = (int)(keys[p0] >> SHIFT);
    const float* c = cent + (size_t)min(max(w, 0), K - 1) * D;
    const float c0 = lane < D ? c[lane] : 0.f, c1 = two && lane + 64 < D ? c[lane + 64] : 0.f;
    float v0 = 0.f, v1 = 0.f;
    for (int p = p0; p < p1; ++p) {
      const int64_t row = r0 + (int64_t)(unsigned)(keys[p] & ROW_MASK);
      float x0 = lane < D ? load1<KIND>(X, row, D, lane) : 0.f;
      float x1 = two && lane + 64 < D ? load1<KIND>(X, row, D, lane + 64) : 0.f;
      if (DescTraits<KIND>::rootsift) {
        const RootsiftRow<KIND> rr(wave_sum_xor(x0 + x1, 64));   // the row sum of materialise_kernel: lane-strided, then the butterfly
        x0 = rr(x0);
        x1 = rr(x1);
      }
      v0 = v0 + (x0 - c0);
      v1 = v1 + (x1 - c1);
    }
    float z0 = v0, z1 = v1;
    if (P != nullptr) {
      z0 = 0.f;
      z1 = 0.f;
      const int t0 = min(lane, B - 1), t1 = min(lane + 64, B - 1);   // lanes beyond B compute a value nobody reads
      const int d0 = min(D, 64);
      for (int u = 0; u < d0; ++u) {
        const float vu = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v0), u));
        z0 = z0 + pm[u * p_su + t0 * p_st] * vu;
        z1 = z1 + pm[u * p_su + t1 * p_st] * vu;
      }
      for (int u = 64; u < D; ++u) {
        const float vu = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v1), u - 64));
        z0 = z0 + pm[u * p_su + t0 * p_st] * vu;
        z1 = z1 + pm[u * p_su + t1 * p_st] * vu;
      }
    }
    const unsigned long long m0 = __ballot(z0 >= 0.f), m1 = __ballot(z1 >= 0.f);
    const int64_t slot = r0 * mm + e;
    if (lane == 0) ent_word[slot] = w;
    store_sig_ballots(ent_sig, slot, W, m0, m1, lane);
  }
}

// ------------------------------------------------------------------------------------------------- score
// Workgroup (g, q) of a grid (G, queries of the launch) serves query q and the images [g S, min((g + 1) S, N)).  acc[S] in LDS.
// A wave takes 64 of the query's entries at a time.  First every lane finds, by two searches of its own, the part of one entry's
// list that falls into the slice (the lists are sorted by image).  Then the wave walks the 64 parts: GW lanes per part and 64 / GW
// parts side by side, GW = 16, 32 or 64 by the longest part of the batch, with coalesced reads of id and signature, xor, popcount,
// a sel look-up and one LDS atomic add per entry.  After one barrier the slice is converted, scaled and stored.
template <int W>
__global__ __launch_bounds__(ASMK_THREADS) void asmk_score_kernel(QueryOffsets qo, const int32_t* __restrict__ q_word,
                                                                   const uint32_t* __restrict__ q_sig, int K,
                                                                   const int64_t* __restrict__ word_off,
                                                                   const int32_t* __restrict__ ent_img,
                                                                   const uint32_t* __restrict__ ent_sig, int N,
                                                                   const int32_t* __restrict__ wt, const int32_t* __restrict__ sel,
                                                                   const float* __restrict__ gamma_q,
                                                                   const float* __restrict__ gamma_db, int S,
                                                                   float* __restrict__ scores, int64_t ld) {
  extern __shared__ __attribute__((aligned(16))) unsigned int asmk_acc[];
  __shared__ unsigned int sel_s[W * 32 + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = blockIdx.y;
  const int s0 = blockIdx.x * S;
  const int sn = min(S, N - s0);
  for (int i = tid; i < sn; i += ASMK_THREADS) asmk_acc[i] = 0u;
  for (int i = tid; i <= W * 32; i += ASMK_THREADS) sel_s[i] = (unsigned)sel[i];
  __syncthreads();

  const int64_t e0 = qo.o[q], e1 = qo.o[q + 1];
  for (int64_t eb = e0 + (int64_t)wave * 64; eb < e1; eb += (int64_t)ASMK_WAVES * 64) {
    const int64_t e = eb + lane;
    int64_t lo = 0;
    int cnt = 0;
    unsigned wgt = 0u;
    if (e < e1) {
      const int w = q_word[e];
      if (w >= 0 && w < K) {
        wgt = (unsigned)wt[w];
        const int64_t a = word_off[w], b = word_off[w + 1];
        if (wgt != 0u && b > a) {
          lo = lower_bound_i32(ent_img, a, b, s0);
          // an image appears once per word: the slice holds at most sn entries of this list
          cnt = (int)(lower_bound_i32(ent_img, lo, min(b, lo + sn), s0 + sn) - lo);
        }
      }
    }
    int longest = cnt;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) longest = max(longest, __shfl_xor(longest, m, 64));
    const int gshift = longest <= 16 ? 4 : (longest <= 32 ? 5 : 6);
    const int GW = 1 << gshift, grp = lane >> gshift, gl = lane & (GW - 1), ngrp = 64 >> gshift;
    unsigned long long live = __ballot(cnt > 0);
    while (live) {
      int mine = -1;
      for (int g = 0; g < ngrp && live; ++g) {
        const int l = __builtin_ctzll(live);
        live &= live - 1;
        if (g == grp) mine = l;
      }
      const int src = mine < 0 ? lane : mine;
      const int64_t plo = shfl64(lo, src);
      const int pn = __shfl(cnt, src, 64);
      const unsigned pw = (unsigned)__shfl((int)wgt, src, 64);
      const int n = mine < 0 ? 0 : pn;
      if (n > 0) {
        uint32_t qs[W];
        load_sig<W>(q_sig + (eb + src) * W, qs);
        for (int t = gl; t < n; t += GW) {
          const int64_t p = plo + t;
          const unsigned i = (unsigned)(ent_img[p] - s0);
          uint32_t xs[W];
          load_sig<W>(ent_sig + p * W, xs);
          if (i < (unsigned)sn) atomicAdd(&asmk_acc[i], pw * sel_s[hamming<W>(xs, qs)]);
        }
      }
    }
  }
  __syncthreads();
  const float gq = gamma_q[qo.first + q];
  float* out = scores + (qo.first + q) * ld + s0;
  for (int i = tid; i < sn; i += ASMK_THREADS) out[i] = __fmul_rn(__fmul_rn((float)asmk_acc[i], gq), gamma_db[s0 + i]);
}

}  // namespace pvs

using namespace pvs;

static int asmk_check_bits(const char* fn, int bits) {
  if (!sig_bits_ok(bits)) PVS_FAIL(PVS_ERR_INVALID, "%s: bits must be 32, 64, 96 or 128 (got %d)", fn, bits);
  return PVS_OK;
}

// m = 0: one label per row (pvs_asmk_aggregate_dev); m >= 1: m labels per row (pvs_asmk_aggregate_ma_dev)
static int asmk_aggregate_impl(const char* fn, pvs_ctx* ctx, const pvs_codebook* cb, const void* d_desc, int desc_kind, const int64_t* d_offsets,
                               const int64_t* h_offsets, int64_t n_images, int64_t total_desc, const int32_t* d_labels, int m,
                               const float* d_proj, int bits, int32_t* d_ent_word, uint32_t* d_ent_sig, int32_t* d_ent_count) {
  const bool ma = m != 0;
  const int mm = ma ? m : 1;
  if (!ctx) PVS_FAIL(PVS_ERR_INVALID, "%s: null ctx", fn);
  if (!cb) PVS_FAIL(PVS_ERR_INVALID, "%s: null codebook", fn);
  PVS_TRY(asmk_check_bits(fn, bits));
  if (desc_kind != PVS_DESC_F32 && desc_kind != PVS_DESC_F32_ROOTSIFT && desc_kind != PVS_DESC_U8_ROOTSIFT)
    PVS_FAIL(PVS_ERR_INVALID, "%s: unknown descriptor kind %d", fn, desc_kind);
  const int D = cb->D, K = cb->K;
  if (D < 1 || D > ASMK_MAX_D) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= D <= %d (got %d)", fn, ASMK_MAX_D, D);
  if (!word_count_ok(K)) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= K <= 65536 (got %d)", fn, K);
  if (ma && (m < 1 || m > ASMK_MAX_M || m > K)) PVS_FAIL(PVS_ERR_INVALID, "%s: m must lie in 1..min(K, %d) (m = %d, K = %d)", fn, ASMK_MAX_M, m, K);
  if (!d_proj && bits != D) PVS_FAIL(PVS_ERR_INVALID, "%s: without a projection bits must equal D (bits=%d, D=%d)", fn, bits, D);
  if (n_images < 0 || total_desc < 0) PVS_FAIL(PVS_ERR_INVALID, "%s: negative sizes", fn);
  if (n_images >= ((int64_t)1 << 31)) PVS_FAIL(PVS_ERR_INVALID, "%s: need n_images < 2^31", fn);
  if (n_images == 0) return PVS_OK;
  if (!d_offsets) PVS_FAIL(PVS_ERR_INVALID, "%s: null offsets", fn);
  if (!h_offsets) PVS_FAIL(PVS_ERR_INVALID, "%s: null host offsets", fn);
  if (!d_ent_count) PVS_FAIL(PVS_ERR_INVALID, "%s: null entry counts", fn);
  if (h_offsets[0] != 0) PVS_FAIL(PVS_ERR_INVALID, "%s: offsets[0] must be 0", fn);
  int64_t longest = 0;
  for (int64_t i = 0; i < n_images; ++i) {
    const int64_t n = h_offsets[i + 1] - h_offsets[i];
    if (n < 0) PVS_FAIL(PVS_ERR_INVALID, "%s: offsets must not decrease (image %lld)", fn, (long long)i);
    longest = std::max(longest, n);
  }
  if (h_offsets[n_images] != total_desc)
    PVS_FAIL(PVS_ERR_INVALID, "%s: offsets end at %lld but total_desc is %lld", fn, (long long)h_offsets[n_images], (long long)total_desc);
  if (longest > ASMK_MAX_ROWS) PVS_FAIL(PVS_ERR_UNSUPPORTED, "%s: an image of %lld rows exceeds %d", fn, (long long)longest, ASMK_MAX_ROWS);
  if (ma && longest * m > ASMK_MAX_KEYS)
    PVS_FAIL(PVS_ERR_UNSUPPORTED, "%s: an image of %lld rows x %d labels exceeds %d keys", fn, (long long)longest, m, ASMK_MAX_KEYS);
  if (total_desc > 0 && (!d_desc || !d_labels || !d_ent_word || !d_ent_sig)) PVS_FAIL(PVS_ERR_INVALID, "%s: null descriptors, labels or entry arrays", fn);
  if (reinterpret_cast<uintptr_t>(d_offsets) % 8) PVS_FAIL(PVS_ERR_INVALID, "%s: offsets must be 8-byte aligned", fn);
  if (reinterpret_cast<uintptr_t>(d_labels) % 4 || reinterpret_cast<uintptr_t>(d_ent_word) % 4 || reinterpret_cast<uintptr_t>(d_ent_sig) % 4 ||
      reinterpret_cast<uintptr_t>(d_ent_count) % 4 || reinterpret_cast<uintptr_t>(d_proj) % 4 ||
      (desc_kind != PVS_DESC_U8_ROOTSIFT && reinterpret_cast<uintptr_t>(d_desc) % 4))
    PVS_FAIL(PVS_ERR_INVALID, "%s: labels, entry arrays, projection and float descriptors must be 4-byte aligned", fn);
  PVS_HIP(hipSetDevice(ctx->device));
  int npad = 64;
  while (npad < longest * mm) npad <<= 1;
  const size_t key_bytes = ma ? 4 : 8, proj_bytes = d_proj ? (size_t)bits * D * sizeof(float) : 0;
  size_t lds = (size_t)npad * (key_bytes + 2) + proj_bytes;
  // keys, heads and the projection's transposed copy share the 160 KiB with the kernel's few static bytes
  const int p_lds = lds <= ASMK_LDS_BUDGET ? 1 : 0;
  if (ma && !p_lds) lds -= proj_bytes;
  ScopedTimer t(ctx, T_AGGREGATE);
  return dispatch_desc_kind(desc_kind, [&](auto k) -> int {
    constexpr int KIND = decltype(k)::value;
    if (ma)
      return launch_lds(ctx, asmk_aggregate_kernel<KIND, true>, dim3((unsigned)n_images), dim3(ASMK_THREADS), lds, d_desc, D, d_offsets,
                        d_labels, (const float*)cb->d_cent, K, d_proj, bits, npad, d_ent_word, d_ent_sig, d_ent_count, m, p_lds);
    return launch_lds(ctx, asmk_aggregate_kernel<KIND, false>, dim3((unsigned)n_images), dim3(ASMK_THREADS), lds, d_desc, D, d_offsets,
                      d_labels, (const float*)cb->d_cent, K, d_proj, bits, npad, d_ent_word, d_ent_sig, d_ent_count, 1, 1);
  });
}

PVS_EXPORT int pvs_asmk_aggregate_dev(pvs_ctx* ctx, const pvs_codebook* cb, const void* d_desc, int desc_kind, const int64_t* d_offsets,
                                      const int64_t* h_offsets, int64_t n_images, int64_t total_desc, const int32_t* d_labels,
                                      const float* d_proj, int bits, int32_t* d_ent_word, uint32_t* d_ent_sig, int32_t* d_ent_count) {
  return asmk_aggregate_impl("pvs_asmk_aggregate_dev", ctx, cb, d_desc, desc_kind, d_offsets, h_offsets, n_images, total_desc, d_labels, 0, d_proj,
                             bits, d_ent_word, d_ent_sig, d_ent_count);
}

PVS_EXPORT int pvs_asmk_aggregate_ma_dev(pvs_ctx* ctx, const pvs_codebook* cb, const void* d_desc, int desc_kind, const int64_t* d_offsets,
                                         const int64_t* h_offsets, int64_t n_images, int64_t total_desc, const int32_t* d_labels, int m,
                                         const float* d_proj, int bits, int32_t* d_ent_word, uint32_t* d_ent_sig, int32_t* d_ent_count) {
  if (m == 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_aggregate_ma_dev: m must lie in 1..min(K, %d) (m = 0)", ASMK_MAX_M);
  return asmk_aggregate_impl("pvs_asmk_aggregate_ma_dev", ctx, cb, d_desc, desc_kind, d_offsets, h_offsets, n_images, total_desc, d_labels, m,
                             d_proj, bits, d_ent_word, d_ent_sig, d_ent_count);
}

PVS_EXPORT int pvs_asmk_score_dev(pvs_ctx* ctx, int64_t nq, const int64_t* h_q_off, const int32_t* d_q_word, const uint32_t* d_q_sig,
                                  int bits, int K, const int64_t* d_word_off, const int32_t* d_ent_img, const uint32_t* d_ent_sig,
                                  int64_t N, const int32_t* d_wt, const int32_t* d_sel, const float* d_gamma_q, const float* d_gamma_db,
                                  int slice_images, float* d_scores, int64_t ld) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(asmk_check_bits(__func__, bits));
  if (!word_count_ok(K)) PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_score_dev: need 1 <= K <= 65536 (got %d)", K);
  if (nq < 0 || N < 0 || N >= ((int64_t)1 << 31)) PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_score_dev: need nq >= 0 and 0 <= N < 2^31");
  if (ld < N) PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_score_dev: ld = %lld is below N = %lld", (long long)ld, (long long)N);
  if (slice_images != 0 && (slice_images < 64 || slice_images > ASMK_MAX_SLICE || slice_images % 64))
    PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_score_dev: slice_images must be 0 or a multiple of 64 in 64..%d (got %d)", ASMK_MAX_SLICE, slice_images);
  if (nq == 0 || N == 0) return PVS_OK;
  const int W = bits / 32;
  PVS_TRY(check_query_and_file(__func__, nq, h_q_off, d_q_word, d_q_sig, W, d_word_off, d_ent_img, d_ent_sig, true, d_wt));
  PVS_NEED(d_sel, "selectivity table");
  PVS_NEED(d_gamma_q, "query normalisers");
  PVS_NEED(d_gamma_db, "database normalisers");
  PVS_NEED(d_scores, "scores");
  PVS_ALIGNED(d_sel, 4, "selectivity table");
  PVS_ALIGNED(d_gamma_q, 4, "query normalisers");
  PVS_ALIGNED(d_gamma_db, 4, "database normalisers");
  PVS_ALIGNED(d_scores, 4, "scores");
  PVS_HIP(hipSetDevice(ctx->device));

  for (int64_t q0 = 0; q0 < nq; q0 += LIST_QUERY_BLOCK) {
    const int64_t qn = std::min<int64_t>(LIST_QUERY_BLOCK, nq - q0);
    const int64_t S = score_slice(ctx->num_cu, qn, N, slice_images), G = (N + S - 1) / S;
    const QueryOffsets qo = query_offsets(h_q_off, q0, qn);
    ScopedTimer t(ctx, T_GEMM);   // the scoring slot, as the scans of the compact index
    const dim3 grid((unsigned)G, (unsigned)qn), block(ASMK_THREADS);
    const size_t lds = (size_t)S * sizeof(unsigned int);
    PVS_TRY(dispatch_sig_words(W, [&](auto w) -> int {
      return launch_lds(ctx, asmk_score_kernel<decltype(w)::value>, grid, block, lds, qo, d_q_word, d_q_sig, K, d_word_off, d_ent_img, d_ent_sig,
                        (int)N, d_wt, d_sel, d_gamma_q, d_gamma_db, (int)S, d_scores, ld);
    }));
  }
  return PVS_OK;
}
