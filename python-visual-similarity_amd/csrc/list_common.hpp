// The list core, shared by the units that scan, search and maintain inverted lists: ivf.hip (section 14),
// update.hip (15), asmk.hip (17), asmk_update.hip (18), asmk_expand.hip (19); diffuse.hip takes ranges_overlap.  The vocabulary is the
// same in all of them: offset arrays, signatures of 1-4 words, block scans, the query offsets of a launch.  Integer arithmetic and
// data movement only, by rule: some of these units are compiled with -ffp-contract=off and some are not, and a header without
// floating point means the same in both.
//   ranges_overlap, outputs_overlap          host: byte ranges of device arrays
//   offsets_first_break, query_offsets_first_break   host: where a host offset array breaks its rule
//   sig_bits_ok, sig_align, word_count_ok    host: the signature widths and vocabulary sizes every entry point accepts
//   score_slice, expand_tile_chunks, invert_tile, flat_grid   host: launch shapes
//   ivf_candidate_width, ivf_query_block     host: the candidate rows of a probed scan (ivf.hip, ivf_sq8.hip)
//   wave_incl_scan, block_incl_scan, block_excl_scan   one int per thread, wave totals through LDS; the exclusive form also returns the block total
//   lower_bound_i32, last_le, shfl64         searches of a lane, a 64-bit shuffle
//   load_sig, move_sig, hamming, store_sig_ballots   signatures
//   QueryOffsets, query_offsets              the entry offsets of up to 128 queries as one kernel argument
//   dispatch_sig_words                       f(std::integral_constant<int, W>) for W = bits / 32
//   check_query_and_file                     the arguments pvs_asmk_score_dev and pvs_asmk_expand_dev share
//   sum_offsets_kernel, remap_offsets_kernel   the two offset kernels of an insert and a remove (templates: only a unit that launches one holds it)
// The host part needs no HIP header: bench/list_common_check.cpp includes this file alone, with a host compiler.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

namespace pvs {

// ------------------------------------------------------------------------------------------------- byte ranges
// a null or empty range overlaps nothing
inline bool ranges_overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a && b && a_bytes > 0 && b_bytes > 0 && a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

struct ByteRange {
  const void* p;
  int64_t bytes;
};

// 1: an output overlaps an input; 2: two outputs overlap (and no output an input); 0: neither
inline int outputs_overlap(const ByteRange* outs, int n_out, const ByteRange* ins, int n_in) {
  for (int o = 0; o < n_out; ++o)
    for (int i = 0; i < n_in; ++i)
      if (ranges_overlap(outs[o].p, outs[o].bytes, ins[i].p, ins[i].bytes)) return 1;
  for (int o = 0; o < n_out; ++o)
    for (int p = o + 1; p < n_out; ++p)
      if (ranges_overlap(outs[o].p, outs[o].bytes, outs[p].p, outs[p].bytes)) return 2;
  return 0;
}

// ------------------------------------------------------------------------------------------------- host offset arrays
// h[0 .. count] must start at 0 and never decrease.  -> the first index that breaks this: 0 when h[0] != 0, i >= 1 when
// h[i] < h[i - 1]; -1 when none does
inline int64_t offsets_first_break(const int64_t* h, int64_t count) {
  if (h[0] != 0) return 0;
  for (int64_t l = 0; l < count; ++l)
    if (h[l + 1] < h[l]) return l + 1;
  return -1;
}

// h[0 .. nq] must be non-negative and never decrease.  -> the first query q with h[q] < 0 or h[q + 1] < h[q]; -1 when there is none
inline int64_t query_offsets_first_break(const int64_t* h, int64_t nq) {
  for (int64_t q = 0; q < nq; ++q)
    if (h[q] < 0 || h[q + 1] < h[q]) return q;
  return -1;
}

// ------------------------------------------------------------------------------------------------- shapes
inline bool sig_bits_ok(int bits) { return bits == 32 || bits == 64 || bits == 96 || bits == 128; }
// bytes a signature of W words must be aligned to: load_sig and move_sig read it as one vector where W is 2 or 4
inline int sig_align(int W) { return W == 4 ? 16 : (W == 2 ? 8 : 4); }
inline bool word_count_ok(int K) { return K >= 1 && K <= 65536; }

// ------------------------------------------------------------------------------------------------- launch shapes
constexpr int ASMK_MAX_SLICE = 32768;          // uint32 accumulators of one score workgroup: 128 KiB
constexpr int64_t ASMK_MIN_SLICE = 1024;       // images a score workgroup serves at least when the host chooses (the rule of section 14)
constexpr int AX_TILE_MAX = 4096;              // words of an expand tile
constexpr int AX_TILE_MIN_CHUNKS = 4;          // one chunk of 64 words per wave of an expand workgroup
constexpr int AU_TILE_DEFAULT = 4096;          // entries of an invert tile
constexpr int AU_TILE_MAX = 65536;
constexpr int64_t AU_MAX_TILES = 65536;

constexpr int64_t IVF_CAND_BYTES = (int64_t)64 << 20;   // candidate rows of one query block of a probed scan (8 bytes per slot)

// W of a probed scan: no query's candidate row is longer than the nprobe longest lists together; rounded up to 64, at least 64.
// h_list_off[0 .. nlist] has passed offsets_first_break; 1 <= nprobe <= nlist
inline int64_t ivf_candidate_width(const int64_t* h_list_off, int nlist, int nprobe) {
  std::vector<int64_t> len(nlist);
  for (int l = 0; l < nlist; ++l) len[l] = h_list_off[l + 1] - h_list_off[l];
  std::nth_element(len.begin(), len.begin() + (nprobe - 1), len.end(), std::greater<int64_t>());
  int64_t W = 0;
  for (int j = 0; j < nprobe; ++j) W += len[j];
  return std::max<int64_t>(64, (W + 63) / 64 * 64);
}

// queries whose candidate rows of W slots share the workspace block: all of them up to grid.y, within IVF_CAND_BYTES, at least one
inline int64_t ivf_query_block(int64_t nq, int64_t W) {
  return std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nq, 65535), IVF_CAND_BYTES / (8 * W)));
}

// images per workgroup of the score: slice_images, or (0) about two workgroups per compute unit over the query block and no slice
// below ASMK_MIN_SLICE images
inline int64_t score_slice(int num_cu, int64_t qn, int64_t N, int slice_images) {
  if (slice_images != 0) return slice_images;
  const int64_t want = (2 * (int64_t)num_cu + qn - 1) / qn;
  const int64_t G0 = std::max<int64_t>(1, std::min<int64_t>(want, N / ASMK_MIN_SLICE));
  return std::min<int64_t>(ASMK_MAX_SLICE, ((N + G0 - 1) / G0 + 63) / 64 * 64);
}

// chunks per workgroup of the expansion: tile_words / 64, or (0) about eight workgroups per compute unit over the query block, every
// wave of a workgroup with a chunk where the words allow
inline int expand_tile_chunks(int num_cu, int nchunks, int64_t qn, int tile_words) {
  if (tile_words / 64 != 0) return tile_words / 64;
  const int64_t want = (int64_t)num_cu * 8;
  return (int)std::min<int64_t>(AX_TILE_MAX / 64, std::max<int64_t>(AX_TILE_MIN_CHUNKS, ((int64_t)nchunks * qn + want - 1) / want));
}

// entries per tile of the inversion: tile_entries rounded up to 256 and clamped to 256..AU_TILE_MAX (0: the default), raised so that
// at most AU_MAX_TILES tiles cover `total`
inline int64_t invert_tile(int tile_entries, int64_t total) {
  const int64_t tile =
      tile_entries == 0 ? AU_TILE_DEFAULT : std::min<int64_t>(std::max<int64_t>(((int64_t)tile_entries + 255) / 256 * 256, 256), AU_TILE_MAX);
  const int64_t need = ((total + AU_MAX_TILES - 1) / AU_MAX_TILES + 255) / 256 * 256;   // need <= 32768
  return std::max(tile, need);
}

// workgroups of a grid-stride kernel over n items, per_block to a workgroup's pass: never more than eight per compute unit
inline unsigned flat_grid(int num_cu, int64_t n, int64_t per_block = 256) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per_block - 1) / per_block, (int64_t)num_cu * 8));
}

}  // namespace pvs

#ifdef __HIPCC__
#include "common.hpp"

namespace pvs {

// ------------------------------------------------------------------------------------------------- block scan
__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int s = 1; s < WAVE; s <<= 1) {
    const int o = __shfl_up(v, s, WAVE);
    if (lane >= s) v += o;
  }
  return v;
}

// block-wide inclusive scan of one int per thread; tmp: LDS int[waves of the block]; the caller may reuse tmp after the call
__device__ __forceinline__ int block_incl_scan(int v, int* tmp, int lane, int wave) {
  const int incl = wave_incl_scan(v, lane);
  if (lane == WAVE - 1) tmp[wave] = incl;
  __syncthreads();
  int off = 0;
  for (int w = 0; w < wave; ++w) off += tmp[w];
  __syncthreads();
  return incl + off;
}

// the exclusive form for a block of WAVES waves: -> the sum of v over the threads before this one, and the sum over the whole block
// in `total`.  A caller that never writes tmp again may pass REUSE_TMP = false and save the barrier behind the reads.
template <int WAVES, bool REUSE_TMP = true>
__device__ __forceinline__ int block_excl_scan(int v, int* tmp, int lane, int wave, int& total) {
  const int incl = wave_incl_scan(v, lane);
  if (lane == WAVE - 1) tmp[wave] = incl;
  __syncthreads();
  int before = incl - v;
  total = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    if (w < wave) before += tmp[w];
    total += tmp[w];
  }
  if (REUSE_TMP) __syncthreads();
  return before;
}

// ------------------------------------------------------------------------------------------------- searches
// the first p in [a, b) with v[p] >= key, b without one; v ascending in [a, b).  One lane's own search: 64 of them run side by side,
// so the dependent loads of a search are paid once per 64 searches.
__device__ __forceinline__ int64_t lower_bound_i32(const int32_t* __restrict__ v, int64_t a, int64_t b, int key) {
  while (a < b) {
    const int64_t m = a + ((b - a) >> 1);
    if (v[m] < key) a = m + 1;
    else b = m;
  }
  return a;
}

// the last i in [0, n - 1] with off(i) <= s; off non-decreasing with off(0) <= s.  `steps` >= log2(n) bounds the loop.
template <class Off>
__device__ __forceinline__ int last_le(Off&& off, int n, int64_t s, int steps) {
  int lo = 0, hi = n - 1;
  for (int it = 0; it < steps; ++it) {
    if (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (off(mid) <= s) lo = mid;
      else hi = mid - 1;
    }
  }
  return lo;
}

__device__ __forceinline__ int64_t shfl64(int64_t v, int src) {
  const int lo = __shfl((int)(v & 0xffffffff), src, WAVE), hi = __shfl((int)(v >> 32), src, WAVE);
  return ((int64_t)hi << 32) | (unsigned)lo;
}

// ------------------------------------------------------------------------------------------------- signatures
typedef uint32_t sig32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t sig32x2 __attribute__((ext_vector_type(2)));

// a signature of W words as one load where W is 2 or 4 (the entry points check sig_align)
template <int W>
__device__ __forceinline__ void load_sig(const uint32_t* __restrict__ p, uint32_t (&s)[W]) {
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

// one load and one store of the signature's full width
template <int W>
__device__ __forceinline__ void move_sig(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst) {
  if constexpr (W == 4) {
    *reinterpret_cast<sig32x4*>(dst) = *reinterpret_cast<const sig32x4*>(src);
  } else if constexpr (W == 2) {
    *reinterpret_cast<sig32x2*>(dst) = *reinterpret_cast<const sig32x2*>(src);
  } else {
    uint32_t v[W];
#pragma unroll
    for (int t = 0; t < W; ++t) v[t] = src[t];
#pragma unroll
    for (int t = 0; t < W; ++t) dst[t] = v[t];
  }
}

template <int W>
__device__ __forceinline__ int hamming(const uint32_t (&a)[W], const uint32_t (&b)[W]) {
  int h = 0;
#pragma unroll
  for (int u = 0; u < W; ++u) h += __popc(a[u] ^ b[u]);
  return h;
}

// signature `slot` of sig [.][W] from two ballots, m0 its bits 0..63 and m1 its bits 64..127: lane t < W stores word t (and only
// those lanes form the address)
__device__ __forceinline__ void store_sig_ballots(uint32_t* __restrict__ sig, int64_t slot, int W, unsigned long long m0,
                                                  unsigned long long m1, int lane) {
  if (lane < W) {
    const unsigned long long mk = lane < 2 ? m0 : m1;
    sig[slot * W + lane] = (unsigned)(lane & 1 ? mk >> 32 : mk);
  }
}

// f(std::integral_constant<int, W>{}) for W = bits / 32
template <class F>
inline int dispatch_sig_words(int W, F&& f) {
  switch (W) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    default: return f(std::integral_constant<int, 4>{});
  }
}

// ------------------------------------------------------------------------------------------------- query blocks
constexpr int LIST_QUERY_BLOCK = 128;   // queries of one launch: their entry offsets travel as kernel arguments

struct QueryOffsets {
  int64_t o[LIST_QUERY_BLOCK + 1];   // entry offsets of the launch's queries
  int64_t first;                     // global index of its first query
};

// the queries [q0, q0 + qn) of host offsets h_q_off, qn <= LIST_QUERY_BLOCK; the slots behind them repeat the last offset
inline QueryOffsets query_offsets(const int64_t* h_q_off, int64_t q0, int64_t qn) {
  QueryOffsets qo;
  for (int64_t q = 0; q <= LIST_QUERY_BLOCK; ++q) qo.o[q] = h_q_off[q0 + std::min(q, qn)];
  qo.first = q0;
  return qo;
}

// What pvs_asmk_score_dev and pvs_asmk_expand_dev both take: the entries of nq > 0 queries (host offsets, device words and signatures of
// W words) and an inverted file with its weights.  The file's entries may be absent where `need_entries` is false (a file of no entries).
inline int check_query_and_file(const char* fn, int64_t nq, const int64_t* h_q_off, const int32_t* d_q_word, const uint32_t* d_q_sig, int W,
                                const int64_t* d_word_off, const int32_t* d_ent_img, const uint32_t* d_ent_sig, bool need_entries,
                                const int32_t* d_wt) {
  const auto need = [&](const void* p, const char* what) -> int {
    if (!p) PVS_FAIL(PVS_ERR_INVALID, "%s: null %s", fn, what);
    return PVS_OK;
  };
  const auto aligned = [&](const void* p, int a, const char* what) -> int {
    if (reinterpret_cast<uintptr_t>(p) % a) PVS_FAIL(PVS_ERR_INVALID, "%s: %s must be %d-byte aligned", fn, what, a);
    return PVS_OK;
  };
  PVS_TRY(need(h_q_off, "host query offsets"));
  const int64_t bad = query_offsets_first_break(h_q_off, nq);
  if (bad >= 0) PVS_FAIL(PVS_ERR_INVALID, "%s: query offsets must be non-negative and must not decrease (query %lld)", fn, (long long)bad);
  if (h_q_off[nq] > h_q_off[0]) {
    PVS_TRY(need(d_q_word, "query words"));
    PVS_TRY(need(d_q_sig, "query signatures"));
  }
  PVS_TRY(need(d_word_off, "word offsets"));
  if (need_entries) {
    PVS_TRY(need(d_ent_img, "entry images"));
    PVS_TRY(need(d_ent_sig, "entry signatures"));
  }
  PVS_TRY(need(d_wt, "word weights"));
  PVS_TRY(aligned(d_q_word, 4, "query words"));
  PVS_TRY(aligned(d_q_sig, sig_align(W), "query signatures"));
  PVS_TRY(aligned(d_word_off, 8, "word offsets"));
  PVS_TRY(aligned(d_ent_img, 4, "entry images"));
  PVS_TRY(aligned(d_ent_sig, sig_align(W), "entry signatures"));
  PVS_TRY(aligned(d_wt, 4, "word weights"));
  return PVS_OK;
}

// ------------------------------------------------------------------------------------------------- offset kernels
// the offsets of two files over the same lists, merged
template <class T>
__global__ void sum_offsets_kernel(const T* __restrict__ a, const T* __restrict__ b, int count, T* __restrict__ out) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l < count) out[l] = a[l] + b[l];
}

// the offsets of a thinned file: spos[e] = the survivors before stored position e, e = 0 .. n
template <class T>
__global__ void remap_offsets_kernel(const int64_t* __restrict__ off, const T* __restrict__ spos, int64_t n, int count,
                                            int64_t* __restrict__ out) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l < count) out[l] = spos[min(max(off[l], (int64_t)0), n)];
}

}  // namespace pvs
#endif  // __HIPCC__
