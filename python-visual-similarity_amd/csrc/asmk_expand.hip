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
// From list_common.hpp: the block scan, the lane searches, signatures, QueryOffsets, the tile rule.
#include <algorithm>

#include "list_common.hpp"

namespace pvs {

constexpr int AX_THREADS = 256;
constexpr int AX_WAVES = AX_THREADS / WAVE;
static_assert(AX_WAVES == AX_TILE_MIN_CHUNKS, "the tile rule gives every wave of a workgroup a chunk");
constexpr int AX_MAX_R = 32;          // members of a query: one bit each in a word's hit mask

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
__global__ __launch_bounds__(AX_THREADS) void ax_mark_kernel(QueryOffsets qo, const int32_t* __restrict__ q_word, int K,
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
      const int64_t p = lower_bound_i32(q_word, e0, e1, w);
      isq = p < e1 && q_word[p] == w;
      weight = wt[w];
      int64_t a = word_off[w];
      const int64_t b = word_off[w + 1];
      for (int r = 0; r < R; ++r) {
        const int id = mem[r];        // the same address in every lane
        if (id < 0) break;            // the padding: wave-uniform
        if (a < b) {
          a = lower_bound_i32(ent_img, a, b, id);
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
    int total;
    const int before = block_excl_scan<AX_WAVES>(v, tmp, lane, wave, total);
    if (live) c[base + tid] = carry + before;
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
__global__ __launch_bounds__(AX_THREADS) void ax_emit_kernel(QueryOffsets qo, const int32_t* __restrict__ q_word,
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
      const int64_t p = lower_bound_i32(q_word, e0, e1, w);
      if (p < e1 && q_word[p] == w) qpos = p;
    }
    unsigned long long em = __ballot(ax_is_output(w < K, qpos >= 0, hits, min_support));
    for (int pos = base; em != 0ull && pos < cap; ++pos) {
      const int l = __builtin_ctzll(em);
      em &= em - 1ull;
      const int ww = c * 64 + l;
      const uint32_t h = (uint32_t)__shfl((int)hits, l, WAVE);
      const int64_t qp = shfl64(qpos, l);
      const bool isq = qp >= 0;
      // lane r < 32: where member r stands in list ww, -1 if it does not
      int64_t hp = -1;
      if (lane < AX_MAX_R && ((h >> lane) & 1u) && my_id >= 0) {
        const int64_t a = word_off[ww], b = word_off[ww + 1];
        const int64_t p = lower_bound_i32(ent_img, a, b, my_id);
        if (p < b && ent_img[p] == my_id) hp = p;
      }
      uint32_t qs[W];
#pragma unroll
      for (int i = 0; i < W; ++i) qs[i] = 0u;
      int qb0 = 0, qb1 = 0, t0 = 0, t1 = 0;
      if (isq) {
        load_sig<W>(q_sig + qp * W, qs);
        ax_lane_bits<W>(qs, lane, qb0, qb1);
        t0 = query_vote * (2 * qb0 - 1);
        t1 = query_vote * (2 * qb1 - 1);
      }
      for (uint32_t hh = h; hh != 0u; hh &= hh - 1u) {
        const int r = __builtin_ctz(hh);
        const int64_t p = shfl64(hp, r);
        if (p < 0) continue;          // only where the members break their precondition
        uint32_t s[W];
        load_sig<W>(ent_sig + p * W, s);
        if (isq && hamming<W>(s, qs) > h_max) continue;   // the gate: against the ORIGINAL query signature
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
      store_sig_ballots(out_sig, row + pos, W, m0, m1, lane);
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
  if (!sig_bits_ok(bits)) PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_expand_dev: bits must be 32, 64, 96 or 128 (got %d)", bits);
  if (!word_count_ok(K)) PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_expand_dev: need 1 <= K <= 65536 (got %d)", K);
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
  const int W = bits / 32;
  PVS_TRY(check_query_and_file(__func__, nq, h_q_off, d_q_word, d_q_sig, W, d_word_off, d_ent_img, d_ent_sig, false, d_wt));
  if (R > 0) {
    PVS_NEED(d_members, "members");
    PVS_NEED(d_votes, "votes");
  }
  if (cap > 0) {
    PVS_NEED(d_out_word, "out words");
    PVS_NEED(d_out_sig, "out signatures");
  }
  PVS_NEED(d_out_count, "out counts");
  PVS_NEED(d_out_sum, "out sums");
  PVS_ALIGNED(d_members, 4, "members");
  PVS_ALIGNED(d_votes, 4, "votes");
  PVS_ALIGNED(d_out_word, 4, "out words");
  PVS_ALIGNED(d_out_sig, sig_align(W), "out signatures");
  PVS_ALIGNED(d_out_count, 4, "out counts");
  PVS_ALIGNED(d_out_sum, 8, "out sums");
  PVS_HIP(hipSetDevice(ctx->device));

  const int nchunks = (K + 63) / 64;
  const int64_t qb = std::min<int64_t>(LIST_QUERY_BLOCK, nq);
  const AsmkExpandLayout lay = asmk_expand_layout((size_t)qb, (size_t)nchunks);
  void* block = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_UPDATE, lay.bytes, &block));
  uint32_t* mask = lay.mask(block);
  int32_t *cnt = lay.cnt(block), *wsum = lay.wsum(block);

  ScopedTimer t(ctx, T_MISC);   // slot 6, with the maintenance of section 18
  for (int64_t q0 = 0; q0 < nq; q0 += LIST_QUERY_BLOCK) {
    const int64_t qn = std::min<int64_t>(LIST_QUERY_BLOCK, nq - q0);
    const int tile_chunks = expand_tile_chunks(ctx->num_cu, nchunks, qn, tile_words);
    const int ntiles = (nchunks + tile_chunks - 1) / tile_chunks;
    const QueryOffsets qo = query_offsets(h_q_off, q0, qn);
    const dim3 grid((unsigned)ntiles, (unsigned)qn), blk(AX_THREADS);
    hipLaunchKernelGGL(ax_mark_kernel, grid, blk, 0, ctx->stream, qo, d_q_word, K, d_word_off, d_ent_img, R, d_members, d_wt, min_support,
                       tile_chunks, nchunks, mask, cnt, wsum);
    PVS_HIP(hipGetLastError());
    hipLaunchKernelGGL(ax_scan_kernel, dim3((unsigned)qn), blk, 0, ctx->stream, q0, nchunks, cnt, wsum, d_out_count, d_out_sum);
    PVS_HIP(hipGetLastError());
    if (cap == 0) continue;
    PVS_TRY(dispatch_sig_words(W, [&](auto w) -> int {
      hipLaunchKernelGGL(ax_emit_kernel<decltype(w)::value>, grid, blk, 0, ctx->stream, qo, d_q_word, d_q_sig, K, d_word_off, d_ent_img,
                         d_ent_sig, R, d_members, d_votes, query_vote, h_max, min_support, tile_chunks, nchunks, mask, cnt, cap, d_out_word,
                         d_out_sig);
      PVS_HIP(hipGetLastError());
      return PVS_OK;
    }));
  }
  return PVS_OK;
}
