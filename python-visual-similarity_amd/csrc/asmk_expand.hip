// ASMK query expansion: the entries of a query are refined by the entries of a few reliable database images, the
// MEMBERS, read out of the word-major inverted file by binary searches (Tolias, Jegou, Pattern Recognition 2014).
//   pvs_asmk_expand_dev   query entries + members + votes x the inverted file -> the expanded entries, ordered by word, their count and
//                         their weight sum
// Every value is DEFINED in include/pvsim.h; all arithmetic is integer; tests/asmk_expand_numpy.py restates it.
//
// A wave owns a CHUNK of 64 consecutive words of one query; a workgroup of four waves owns a tile of consecutive chunks.  Three launches
// per block of 128 queries, ordered by the stream:
//   mark   one lane per word: is it a query word (one search of the query's words), and which members hold it (R searches of its list;
//          the members ascend, so the lower bound carries forward).  64 searches run side by side, as in asmk_score_kernel.  The hit mask
//          of every word goes to the workspace, and per chunk the number of output entries and their weight sum.
//   scan   one workgroup per query: the chunk counts become their exclusive prefixes; count and sum of the query are written.
//   emit   the output words of a chunk are popped from a ballot in ascending order; the position of each is the chunk's prefix plus its
//          rank.  Lane r finds member r's entry in the word's list; then the hits are walked one by one, wave-uniform (signature, gate,
//          vote), with the lanes over the bits: lane l tallies the bits l and l + 64.  The result bits come from two ballots.
// No position is decided by an atomic (there is none), no workgroup waits for another, every written element is written once.  The cut
// into tiles assigns chunks to workgroups and nothing else: every tile_words gives the same bytes.
#include <algorithm>

#include "common.hpp"

namespace pvs {

constexpr int AX_THREADS = 256;
constexpr int AX_WAVES = AX_THREADS / WAVE;
constexpr int AX_QUERY_BLOCK = 128;   // queries of one launch: their entry offsets travel as kernel arguments
constexpr int AX_MAX_R = 32;          // members of a query: one bit each in a word's hit mask
constexpr int AX_TILE_MAX = 4096;     // words of a tile

struct AxQueryOffsets {
  int64_t o[AX_QUERY_BLOCK + 1];   // entry offsets of the launch's queries
  int64_t first;                   // global index of its first query
};

// the first p in [a, b) with v[p] >= key, b without one; v ascending in [a, b)
__device__ __forceinline__ int64_t ax_lower_bound(const int32_t* __restrict__ v, int64_t a, int64_t b, int key) {
  while (a < b) {
    const int64_t m = a + ((b - a) >> 1);
    if (v[m] < key) a = m + 1;
    else b = m;
  }
  return a;
}

__device__ __forceinline__ int64_t ax_shfl64(int64_t v, int src) {
  const int lo = __shfl((int)(v & 0xffffffff), src, WAVE), hi = __shfl((int)(v >> 32), src, WAVE);
  return ((int64_t)hi << 32) | (unsigned)lo;
}

template <int W>
__device__ __forceinline__ void ax_load_sig(const uint32_t* __restrict__ p, uint32_t (&s)[W]) {
  if constexpr (W == 4) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    s[0] = v.x, s[1] = v.y, s[2] = v.z, s[3] = v.w;
  } else if constexpr (W == 2) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    s[0] = v.x, s[1] = v.y;
  } else {
#pragma unroll
    for (int i = 0; i < W; ++i) s[i] = p[i];
  }
}

// the bits `lane` and `lane + 64` of a signature, as 0 / 1; a lane beyond the signature's bits gets a value nobody reads
template <int W>
__device__ __forceinline__ void ax_lane_bits(const uint32_t (&s)[W], int lane, int& b0, int& b1) {
  uint32_t x0 = s[0], x1 = 0u;
  if constexpr (W >= 2) x0 = lane >= 32 ? s[1] : s[0];
  if constexpr (W >= 3) x1 = s[2];
  if constexpr (W == 4) x1 = lane >= 32 ? s[3] : s[2];
  b0 = (int)((x0 >> (lane & 31)) & 1u);
  b1 = (int)((x1 >> (lane & 31)) & 1u);
}

__device__ __forceinline__ bool ax_is_output(bool in_range, bool is_query_word, uint32_t hits, int min_support) {
  return in_range && (is_query_word || (min_support >= 1 && __popc(hits) >= min_support));
}

// ------------------------------------------------------------------------------------------------- mark
// grid (tiles, queries of the launch).  mask [query][nchunks * 64], cnt and wsum [query][nchunks].
__global__ __launch_bounds__(AX_THREADS) void ax_mark_kernel(AxQueryOffsets qo, const int32_t* __restrict__ q_word, int K,
                                                             const int64_t* __restrict__ word_off, const int32_t* __restrict__ ent_img,
                                                             int R, const int32_t* __restrict__ members, const int32_t* __restrict__ wt,
                                                             int min_support, int tile_chunks, int nchunks, uint32_t* __restrict__ mask,
                                                             int32_t* __restrict__ cnt, int32_t* __restrict__ wsum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.y;
  const int64_t e0 = qo.o[q], e1 = qo.o[q + 1];
  const int32_t* mem = members + (qo.first + q) * R;
  const int c_lo = blockIdx.x * tile_chunks, c_hi = min(c_lo + tile_chunks, nchunks);
  for (int c = c_lo + wave; c < c_hi; c += AX_WAVES) {
    const int w = c * 64 + lane;
    uint32_t hits = 0u;
    bool isq = false;
    int weight = 0;
    if (w < K) {
      const int64_t p = ax_lower_bound(q_word, e0, e1, w);
      isq = p < e1 && q_word[p] == w;
      weight = wt[w];
      int64_t a = word_off[w];
      const int64_t b = word_off[w + 1];
      for (int r = 0; r < R; ++r) {
        const int id = mem[r];        // the same address in every lane
        if (id < 0) break;            // the padding: wave-uniform
        if (a < b) {
          a = ax_lower_bound(ent_img, a, b, id);
          if (a < b && ent_img[a] == id) hits |= 1u << r;
        }
      }
    }
    const bool out = ax_is_output(w < K, isq, hits, min_support);
    const unsigned long long em = __ballot(out);
    int ws = out ? 1023 * weight : 0;   // 64 x 1023 x 1023 < 2^31
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) ws += __shfl_xor(ws, m, WAVE);
    const int64_t slot = (int64_t)q * nchunks + c;
    mask[slot * 64 + lane] = hits;
    if (lane == 0) {
      cnt[slot] = __popcll(em);
      wsum[slot] = ws;
    }
  }
}

// ------------------------------------------------------------------------------------------------- scan
// one workgroup per query: cnt[q][.] -> exclusive prefixes in place; the totals go to out_count / out_sum
__global__ __launch_bounds__(AX_THREADS) void ax_scan_kernel(int64_t first, int nchunks, int32_t* __restrict__ cnt,
                                                             const int32_t* __restrict__ wsum, int32_t* __restrict__ out_count,
                                                             int64_t* __restrict__ out_sum) {
  __shared__ int tmp[AX_WAVES];
  __shared__ long long stmp[AX_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = blockIdx.x;
  int32_t* c = cnt + (int64_t)q * nchunks;
  const int32_t* s = wsum + (int64_t)q * nchunks;
  int carry = 0;
  long long sum = 0;
  for (int base = 0; base < nchunks; base += AX_THREADS) {   // nchunks is a launch argument: the same trip count in every thread
    const bool live = base + tid < nchunks;
    const int v = live ? c[base + tid] : 0;
    sum += live ? (long long)s[base + tid] : 0ll;
    int incl = v;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const int o = __shfl_up(incl, d, WAVE);
      if (lane >= d) incl += o;
    }
    if (lane == WAVE - 1) tmp[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < AX_WAVES; ++w) {
      if (w < wave) before += tmp[w];
      total += tmp[w];
    }
    __syncthreads();
    if (live) c[base + tid] = carry + before + incl - v;
    carry += total;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, WAVE);
  if (lane == 0) stmp[wave] = sum;
  __syncthreads();
  if (tid == 0) {
    long long all = 0;
    for (int w = 0; w < AX_WAVES; ++w) all += stmp[w];
    out_count[first + q] = carry;
    out_sum[first + q] = all;
  }
}

// ------------------------------------------------------------------------------------------------- emit
template <int W>
__global__ __launch_bounds__(AX_THREADS) void ax_emit_kernel(AxQueryOffsets qo, const int32_t* __restrict__ q_word,
                                                             const uint32_t* __restrict__ q_sig, int K,
                                                             const int64_t* __restrict__ word_off, const int32_t* __restrict__ ent_img,
                                                             const uint32_t* __restrict__ ent_sig, int R,
                                                             const int32_t* __restrict__ members, const int32_t* __restrict__ votes,
                                                             int query_vote, int h_max, int min_support, int tile_chunks, int nchunks,
                                                             const uint32_t* __restrict__ mask, const int32_t* __restrict__ cnt, int cap,
                                                             int32_t* __restrict__ out_word, uint32_t* __restrict__ out_sig) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.y;
  const int64_t e0 = qo.o[q], e1 = qo.o[q + 1];
  const int64_t row = (qo.first + q) * (int64_t)cap;
  int my_id = -1, my_vote = 0;        // lane r holds member r
  if (lane < R) {
    my_id = members[(qo.first + q) * R + lane];
    my_vote = votes[(qo.first + q) * R + lane];
  }
  const int c_lo = blockIdx.x * tile_chunks, c_hi = min(c_lo + tile_chunks, nchunks);
  for (int c = c_lo + wave; c < c_hi; c += AX_WAVES) {
    const int64_t slot = (int64_t)q * nchunks + c;
    const int base = cnt[slot];
    if (base >= cap) continue;        // wave-uniform: nothing of this chunk is stored
    const int w = c * 64 + lane;
    uint32_t hits = 0u;
    int64_t qpos = -1;
    if (w < K) {
      hits = mask[slot * 64 + lane];
      const int64_t p = ax_lower_bound(q_word, e0, e1, w);
      if (p < e1 && q_word[p] == w) qpos = p;
    }
    unsigned long long em = __ballot(ax_is_output(w < K, qpos >= 0, hits, min_support));
    for (int pos = base; em != 0ull && pos < cap; ++pos) {
      const int l = __builtin_ctzll(em);
      em &= em - 1ull;
      const int ww = c * 64 + l;
      const uint32_t h = (uint32_t)__shfl((int)hits, l, WAVE);
      const int64_t qp = ax_shfl64(qpos, l);
      const bool isq = qp >= 0;
      // lane r < 32: where member r stands in list ww, -1 if it does not
      int64_t hp = -1;
      if (lane < AX_MAX_R && ((h >> lane) & 1u) && my_id >= 0) {
        const int64_t a = word_off[ww], b = word_off[ww + 1];
        const int64_t p = ax_lower_bound(ent_img, a, b, my_id);
        if (p < b && ent_img[p] == my_id) hp = p;
      }
      uint32_t qs[W];
#pragma unroll
      for (int i = 0; i < W; ++i) qs[i] = 0u;
      int qb0 = 0, qb1 = 0, t0 = 0, t1 = 0;
      if (isq) {
        ax_load_sig<W>(q_sig + qp * W, qs);
        ax_lane_bits<W>(qs, lane, qb0, qb1);
        t0 = query_vote * (2 * qb0 - 1);
        t1 = query_vote * (2 * qb1 - 1);
      }
      for (uint32_t hh = h; hh != 0u; hh &= hh - 1u) {
        const int r = __builtin_ctz(hh);
        const int64_t p = ax_shfl64(hp, r);
        if (p < 0) continue;          // only where the members break their precondition
        uint32_t s[W];
        ax_load_sig<W>(ent_sig + p * W, s);
        if (isq) {                    // the gate: against the ORIGINAL query signature
          int hd = 0;
#pragma unroll
          for (int i = 0; i < W; ++i) hd += __popc(s[i] ^ qs[i]);
          if (hd > h_max) continue;
        }
        const int v = __shfl(my_vote, r, WAVE);
        int b0, b1;
        ax_lane_bits<W>(s, lane, b0, b1);
        t0 += v * (2 * b0 - 1);
        t1 += v * (2 * b1 - 1);
      }
      const bool r0 = isq ? (t0 > 0 || (t0 == 0 && qb0 != 0)) : t0 >= 0;
      const bool r1 = isq ? (t1 > 0 || (t1 == 0 && qb1 != 0)) : t1 >= 0;
      const unsigned long long m0 = __ballot(r0), m1 = __ballot(r1);
      if (lane == 0) out_word[row + pos] = ww;
      if (lane < W) {
        const unsigned long long mk = lane < 2 ? m0 : m1;
        out_sig[(row + pos) * W + lane] = (unsigned)(lane & 1 ? mk >> 32 : mk);
      }
    }
  }
}

}  // namespace pvs

using namespace pvs;

PVS_EXPORT int pvs_asmk_expand_dev(pvs_ctx* ctx, int64_t nq, const int64_t* h_q_off, const int32_t* d_q_word, const uint32_t* d_q_sig,
                                   int bits, int K, const int64_t* d_word_off, const int32_t* d_ent_img, const uint32_t* d_ent_sig,
                                   int64_t N, int R, const int32_t* d_members, const int32_t* d_votes, int query_vote, int h_max,
                                   int min_support, const int32_t* d_wt, int tile_words, int cap, int32_t* d_out_word,
                                   uint32_t* d_out_sig, int32_t* d_out_count, int64_t* d_out_sum) {
  PVS_NEED(ctx, "ctx");
  if (bits != 32 && bits != 64 && bits != 96 && bits != 128)
    PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_expand_dev: bits must be 32, 64, 96 or 128 (got %d)", bits);
  if (K < 1 || K > 65536) PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_expand_dev: need 1 <= K <= 65536 (got %d)", K);
  if (nq < 0 || N < 0 || N >= ((int64_t)1 << 31)) PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_expand_dev: need nq >= 0 and 0 <= N < 2^31");
  if (R < 0 || R > AX_MAX_R) PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_expand_dev: R must lie in 0..%d (got %d)", AX_MAX_R, R);
  if (query_vote < 0 || query_vote > 65535) PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_expand_dev: query_vote must lie in 0..65535 (got %d)", query_vote);
  if (h_max < 0 || h_max > bits) PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_expand_dev: h_max must lie in 0..bits (got %d)", h_max);
  if (min_support < 0 || min_support > AX_MAX_R + 1)
    PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_expand_dev: min_support must lie in 0..%d (got %d)", AX_MAX_R + 1, min_support);
  if (tile_words != 0 && (tile_words < 64 || tile_words > AX_TILE_MAX || tile_words % 64))
    PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_expand_dev: tile_words must be 0 or a multiple of 64 in 64..%d (got %d)", AX_TILE_MAX, tile_words);
  if (cap < 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_expand_dev: cap must not be negative (got %d)", cap);
  if (nq == 0) return PVS_OK;
  PVS_NEED(h_q_off, "host query offsets");
  for (int64_t q = 0; q < nq; ++q)
    if (h_q_off[q] < 0 || h_q_off[q + 1] < h_q_off[q])
      PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_expand_dev: query offsets must be non-negative and must not decrease (query %lld)", (long long)q);
  if (h_q_off[nq] > h_q_off[0]) {
    PVS_NEED(d_q_word, "query words");
    PVS_NEED(d_q_sig, "query signatures");
  }
  if (R > 0) {
    PVS_NEED(d_members, "members");
    PVS_NEED(d_votes, "votes");
  }
  if (cap > 0) {
    PVS_NEED(d_out_word, "out words");
    PVS_NEED(d_out_sig, "out signatures");
  }
  PVS_NEED(d_word_off, "word offsets");
  PVS_NEED(d_wt, "word weights");
  PVS_NEED(d_out_count, "out counts");
  PVS_NEED(d_out_sum, "out sums");
  const int W = bits / 32;
  const int sig_align = W == 4 ? 16 : (W == 2 ? 8 : 4);
  PVS_ALIGNED(d_q_word, 4, "query words");
  PVS_ALIGNED(d_q_sig, sig_align, "query signatures");
  PVS_ALIGNED(d_word_off, 8, "word offsets");
  PVS_ALIGNED(d_ent_img, 4, "entry images");
  PVS_ALIGNED(d_ent_sig, sig_align, "entry signatures");
  PVS_ALIGNED(d_members, 4, "members");
  PVS_ALIGNED(d_votes, 4, "votes");
  PVS_ALIGNED(d_wt, 4, "word weights");
  PVS_ALIGNED(d_out_word, 4, "out words");
  PVS_ALIGNED(d_out_sig, sig_align, "out signatures");
  PVS_ALIGNED(d_out_count, 4, "out counts");
  PVS_ALIGNED(d_out_sum, 8, "out sums");
  PVS_HIP(hipSetDevice(ctx->device));

  const int nchunks = (K + 63) / 64;
  const int64_t qb = std::min<int64_t>(AX_QUERY_BLOCK, nq);
  const AsmkExpandLayout lay = asmk_expand_layout((size_t)qb, (size_t)nchunks);
  void* block = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_UPDATE, lay.bytes, &block));
  uint32_t* mask = lay.mask(block);
  int32_t *cnt = lay.cnt(block), *wsum = lay.wsum(block);

  ScopedTimer t(ctx, T_MISC);   // slot 6, with the maintenance of section 18
  for (int64_t q0 = 0; q0 < nq; q0 += AX_QUERY_BLOCK) {
    const int64_t qn = std::min<int64_t>(AX_QUERY_BLOCK, nq - q0);
    int tile_chunks = tile_words / 64;
    if (tile_chunks == 0) {
      // about eight workgroups per compute unit over the query block, every wave of a workgroup with a chunk where the words allow
      const int64_t want = (int64_t)ctx->num_cu * 8;
      tile_chunks = (int)std::min<int64_t>(AX_TILE_MAX / 64, std::max<int64_t>(AX_WAVES, ((int64_t)nchunks * qn + want - 1) / want));
    }
    const int ntiles = (nchunks + tile_chunks - 1) / tile_chunks;
    AxQueryOffsets qo;
    for (int64_t q = 0; q <= AX_QUERY_BLOCK; ++q) qo.o[q] = h_q_off[q0 + std::min(q, qn)];
    qo.first = q0;
    const dim3 grid((unsigned)ntiles, (unsigned)qn), blk(AX_THREADS);
    hipLaunchKernelGGL(ax_mark_kernel, grid, blk, 0, ctx->stream, qo, d_q_word, K, d_word_off, d_ent_img, R, d_members, d_wt, min_support,
                       tile_chunks, nchunks, mask, cnt, wsum);
    PVS_HIP(hipGetLastError());
    hipLaunchKernelGGL(ax_scan_kernel, dim3((unsigned)qn), blk, 0, ctx->stream, q0, nchunks, cnt, wsum, d_out_count, d_out_sum);
    PVS_HIP(hipGetLastError());
    if (cap == 0) continue;
#define PVS_AX_EMIT(WORDS)                                                                                                              \
  hipLaunchKernelGGL(ax_emit_kernel<WORDS>, grid, blk, 0, ctx->stream, qo, d_q_word, d_q_sig, K, d_word_off, d_ent_img, d_ent_sig, R,   \
                     d_members, d_votes, query_vote, h_max, min_support, tile_chunks, nchunks, mask, cnt, cap, d_out_word, d_out_sig)
    switch (W) {
      case 1: PVS_AX_EMIT(1); break;
      case 2: PVS_AX_EMIT(2); break;
      case 3: PVS_AX_EMIT(3); break;
      default: PVS_AX_EMIT(4); break;
    }
#undef PVS_AX_EMIT
    PVS_HIP(hipGetLastError());
  }
  return PVS_OK;
}
