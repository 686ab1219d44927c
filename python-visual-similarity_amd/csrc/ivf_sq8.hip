// Inverted lists over the int8 code rows: the probed exact scan behind pvsim.IVFInt8Index.
//   pvs_ivf_sq8_scan_topk_dev   query codes x the code rows of the probed lists -> candidate rows (score, original id) -> list-mode
//                               top-k (topk.hip)
// All arithmetic is section 22's: acc = the int32 dot product of two code rows, score = ((float)acc * inv_q) * inv_d.  acc is an
// integer, so no slice size, wave assignment or order of summation changes a bit, and a score here is, bit for bit, the score
// pvs_sq8_topk_dev reports for the same pair.  Nothing is a multiply followed by an add: the unit needs no -ffp-contract=off.
// The storage, the candidate row and its padding are section 14's with m = ld (ivf.hip); the centroids are code rows themselves, so
// the list of a row and the probes of a query both come from pvs_sq8_topk_dev and this unit only scans.
//   pvs_ivf_sq8_scan_lists_topk_dev   the same candidate rows, filled by list: the (query, probe) pairs of a
//                               query block grouped by list, every row tile of a probed list scored against its group on the int8
//                               matrix pipe; for batches of queries
//   pvs_ivf_sq8_group_probes_dev      the grouping alone
// From list_common.hpp: the block scan over the probed lists' lengths, the check of the host offsets, W and the query block.  From
// ivf_sq8_plan.hpp: the slices, the query block and the tiles of the scan by list.  From radix_sort.hpp: the stable sort of the pairs.
#include "ivf_sq8_plan.hpp"
#include "list_common.hpp"
#include "radix_sort.hpp"

namespace pvs {
namespace {

using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x16 = __attribute__((ext_vector_type(16))) int;

constexpr int ISQ_MAX_L = 131072;

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Workgroup (g, q) of a grid (G, queries of the block).  The candidate row of query q is the concatenation of its probed lists in
// probe order (section 14): probe j owns the slots [incl[j] - len[j], incl[j]), slot p of it is stored row start[j] + p, and the
// slots from incl[nprobe - 1] up to W are padding (-inf, -1).  The workgroup serves the slice [g S, (g + 1) S) of that row whatever
// lists it falls into.  The query's ld code bytes are copied to LDS once; then a WAVE owns a slot (a row is up to 128 KiB, not m
// bytes): wave w takes the slots p0 + w, p0 + w + 16, ..., finds the slot's probe by a binary search of incl[] in LDS (the same for
// all its lanes), walks the stored row with 16-byte loads, four in flight, and v_dot4 against the query's bytes at the same offsets
// (the inner loop of sq8_rows_kernel<1>), adds the 64 partial sums by shuffles, and lane 0 stores the slot.  Every slot of [0, W) is
// written exactly once: no atomics, no position that depends on timing.
__global__ __launch_bounds__(ISQ_THREADS) void ivf_sq8_scan_kernel(const int8_t* __restrict__ qc, const float* __restrict__ inv_q, int ld,
                                                                   const int64_t* __restrict__ probe, int nprobe,
                                                                   const int64_t* __restrict__ list_off, int nlist,
                                                                   const int8_t* __restrict__ codes, const float* __restrict__ inv_db,
                                                                   const int32_t* __restrict__ ids, int64_t W, int64_t S,
                                                                   float* __restrict__ cval, int32_t* __restrict__ cid) {
  extern __shared__ __attribute__((aligned(16))) int8_t s_qrow[];   // [ld]
  __shared__ int incl[ISQ_MAX_PROBE];      // inclusive prefix sums of the probed lists' lengths (N < 2^31)
  __shared__ int start[ISQ_MAX_PROBE];     // first stored row of each probed list
  __shared__ int stmp[ISQ_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q = blockIdx.y;
  const int64_t p0 = (int64_t)blockIdx.x * S, p1 = min(p0 + S, W);

  // ---- the probes of this query: one per thread
  {
    int len = 0;
    if (tid < nprobe) {
      const int64_t l = probe[q * nprobe + tid];
      const bool ok = l >= 0 && l < nlist;
      const int64_t a = ok ? list_off[l] : 0, b = ok ? list_off[l + 1] : 0;
      len = (int)(b - a);
      start[tid] = (int)a;
    }
    const int upto = block_incl_scan(len, stmp, lane, wave);
    if (tid < nprobe) incl[tid] = upto;
  }
  __syncthreads();
  const int64_t total = incl[nprobe - 1];
  const int64_t live_end = min(p1, total);
  // ---- padding slots of this slice
  for (int64_t p = max(p0, total) + tid; p < p1; p += ISQ_THREADS) {
    cval[q * W + p] = -INFINITY;
    cid[q * W + p] = -1;
  }
  if (p0 >= live_end) return;              // the whole workgroup leaves

  // ---- the query's code row
  const int nch = ld / 16;                 // 16-byte chunks of a row: a multiple of 4
  i32x4* s4 = reinterpret_cast<i32x4*>(s_qrow);
  {
    const i32x4* q4 = reinterpret_cast<const i32x4*>(qc + q * ld);
    for (int i = tid; i < nch; i += ISQ_THREADS) s4[i] = q4[i];
  }
  __syncthreads();
  const float iq = inv_q[q];

  auto dot16 = [&](const i32x4 d, int c, int a) {
    const i32x4 qv = s4[c];
    a = __builtin_amdgcn_sdot4(qv.x, d.x, a, false);
    a = __builtin_amdgcn_sdot4(qv.y, d.y, a, false);
    a = __builtin_amdgcn_sdot4(qv.z, d.z, a, false);
    a = __builtin_amdgcn_sdot4(qv.w, d.w, a, false);
    return a;
  };

  for (int64_t p = p0 + wave; p < live_end; p += ISQ_WAVES) {
    // j = the number of probes that end at or before p: incl[j - 1] <= p < incl[j], so probe j is not empty
    int lo = 0, hi = nprobe - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((int64_t)incl[mid] <= p) lo = mid + 1;
      else hi = mid;
    }
    const int64_t first = lo > 0 ? (int64_t)incl[lo - 1] : 0;
    const int64_t row = (int64_t)start[lo] + (p - first);
    const i32x4* d4 = reinterpret_cast<const i32x4*>(codes + row * ld);
    int acc = 0;
    int c = lane;
    for (; c + 192 < nch; c += 256) {
      const i32x4 v0 = d4[c], v1 = d4[c + 64], v2 = d4[c + 128], v3 = d4[c + 192];
      acc = dot16(v0, c, acc);
      acc = dot16(v1, c + 64, acc);
      acc = dot16(v2, c + 128, acc);
      acc = dot16(v3, c + 192, acc);
    }
    for (; c < nch; c += 64) acc = dot16(d4[c], c, acc);
    const int sum = wave_sum(acc);
    if (lane == 0) {
      cval[q * W + p] = ((float)sum * iq) * inv_db[row];
      cid[q * W + p] = ids[row];
    }
  }
}

// ------------------------------------------------------------------------------------------------- the scan by list (section 28)
constexpr int ISQL_THREADS = 256;   // four waves, 2 x 2, each owning 64 grouped pairs x 64 stored rows
constexpr int ISQL_BK = 128;        // bytes of a row per k-block (four k-steps of 32)

// Step one of ivf_sq8_scan_kernel without the scan.  Workgroup q, one thread per probe: base[q][j] = the first slot of probe j in the
// candidate row = the lengths of the probes before it, total[q] = the live slots, and the sort item of the pair, (list << 32) | (q
// nprobe + j), with list = nlist for a probe outside [0, nlist).  With a candidate block the padding slots [total[q], W) are written
// here: the tile kernel writes every live slot, so each slot of [0, W) is written exactly once.
__global__ __launch_bounds__(ISQ_THREADS) void isql_base_kernel(const int64_t* __restrict__ probe, int nprobe, const int64_t* __restrict__ list_off,
                                                                int nlist, int64_t W, int32_t* __restrict__ base, int32_t* __restrict__ total,
                                                                uint64_t* __restrict__ items, float* __restrict__ cval, int32_t* __restrict__ cid) {
  __shared__ int stmp[ISQ_WAVES];
  __shared__ int s_total;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q = blockIdx.x;
  int len = 0;
  uint32_t key = (uint32_t)nlist;
  if (tid < nprobe) {
    const int64_t l = probe[q * nprobe + tid];
    if (l >= 0 && l < nlist) {
      len = (int)(list_off[l + 1] - list_off[l]);
      key = (uint32_t)l;
    }
  }
  const int upto = block_incl_scan(len, stmp, lane, wave);
  if (tid < nprobe) {
    const int64_t s = q * nprobe + tid;
    base[s] = upto - len;
    items[s] = ((uint64_t)key << 32) | (uint64_t)(uint32_t)s;
  }
  if (tid == nprobe - 1) {
    total[q] = upto;
    s_total = upto;
  }
  if (!cval) return;                       // the same for every thread
  __syncthreads();
  for (int64_t p = (int64_t)s_total + tid; p < W; p += ISQ_THREADS) {
    cval[q * W + p] = -INFINITY;
    cid[q * W + p] = -1;
  }
}

// tile_off[l] = the row tiles of the lists before l, l = 0 .. nlist: one workgroup, ISQ_THREADS lists at a time with a carry
__global__ __launch_bounds__(ISQ_THREADS) void isql_tile_off_kernel(const int64_t* __restrict__ list_off, int nlist, int32_t* __restrict__ tile_off) {
  __shared__ int stmp[ISQ_WAVES];
  __shared__ int chunk_total;
  const int tid = threadIdx.x;
  int carry = 0;
  for (int l0 = 0; l0 < nlist; l0 += ISQ_THREADS) {
    const int l = l0 + tid;
    const int v = l < nlist ? (int)isql_list_tiles(max(list_off[l + 1] - list_off[l], (int64_t)0)) : 0;
    const int incl = block_incl_scan(v, stmp, tid & 63, tid >> 6);
    if (l < nlist) tile_off[l] = carry + incl - v;
    if (tid == ISQ_THREADS - 1) chunk_total = incl;
    __syncthreads();
    carry += chunk_total;
    __syncthreads();
  }
  if (tid == 0) tile_off[nlist] = carry;
}

// the sorted items -> the query and the first slot of every grouped pair; the items behind goff[nlist] are no pairs of a list
__global__ __launch_bounds__(AU_THREADS) void isql_pairs_kernel(const uint64_t* __restrict__ items, int64_t pairs, int nprobe, int nlist,
                                                                const int32_t* __restrict__ base, int32_t* __restrict__ gq,
                                                                int32_t* __restrict__ gbase) {
  for (int64_t p = (int64_t)blockIdx.x * AU_THREADS + threadIdx.x; p < pairs; p += (int64_t)gridDim.x * AU_THREADS) {
    const uint64_t item = items[p];
    if ((uint32_t)(item >> 32) >= (uint32_t)nlist) continue;
    const int64_t s = (int64_t)(uint32_t)item;
    if (s >= pairs) continue;
    gq[p] = (int32_t)(s / nprobe);
    gbase[p] = base[s];
  }
}

// Workgroup t scores one row tile: ISQL_ROWS consecutive stored rows of ONE list l (tile_off[l] <= t < tile_off[l + 1], found by a
// search of the tile prefix), against the grouped pairs [goff[l], goff[l + 1]) of that list, ISQL_PAIRS at a time.  The loop is
// sq8_gemm_kernel's (sq8.hip): the gathered query rows are the A operand of v_mfma_i32_32x32x32_i8 and the stored rows its B operand,
// both take byte 32 s + 16 (lane >> 5) + e of their row as element e of k-step s, k-blocks of 128 bytes go through LDS rows whose
// 16-byte chunk index is xor-ed by (row & 7), and the next k-block's global loads are issued before the current block is multiplied.
// Three maskings: a tile row past the list's end is the next list's row (storage is contiguous) and a pair past the group's end is
// the next list's pair; both are staged as zeros and never stored; bytes past ld are zeros.  A lane's 16 accumulators are 16 pairs
// of one stored row, so the 32 lanes of a half wave store one register into 32 consecutive slots of one candidate row:
//   slot = q W + gbase + (row - list start), 64-bit, written by exactly this workgroup and this pair.
__global__ __launch_bounds__(ISQL_THREADS) void ivf_sq8_tile_kernel(const int8_t* __restrict__ qc, const float* __restrict__ inv_q, int qn, int ld,
                                                                    const int64_t* __restrict__ list_off, int nlist,
                                                                    const int32_t* __restrict__ tile_off, const int32_t* __restrict__ goff,
                                                                    const int32_t* __restrict__ gq, const int32_t* __restrict__ gbase,
                                                                    const int8_t* __restrict__ codes, const float* __restrict__ inv_db,
                                                                    const int32_t* __restrict__ ids, int64_t N, int64_t W,
                                                                    float* __restrict__ cval, int32_t* __restrict__ cid) {
  __shared__ __attribute__((aligned(16))) int8_t s_q[ISQL_PAIRS * ISQL_BK];
  __shared__ __attribute__((aligned(16))) int8_t s_d[ISQL_ROWS * ISQL_BK];
  __shared__ int s_pq[ISQL_PAIRS];         // the query of each pair of the query tile, -1 past the group's end
  __shared__ int s_pb[ISQL_PAIRS];         // its first slot
  __shared__ float s_piq[ISQL_PAIRS];      // its query's factor
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int wq = wave & 1, wd = wave >> 1;
  const int t = blockIdx.x;
  const int l = last_le([&](int i) { return (int64_t)tile_off[i]; }, nlist, t, 17);   // nlist <= 2^16
  const int g0 = goff[l], g1 = goff[l + 1];
  if (g0 >= g1) return;                    // no query of the block probes this list: the whole workgroup leaves
  const int64_t first = list_off[l], end = min(list_off[l + 1], N);
  const int64_t d0 = first + (int64_t)(t - tile_off[l]) * ISQL_ROWS;
  if (d0 < 0 || d0 >= end) return;         // device offsets that disagree with the host's: nothing is read out of bounds

  // staging: thread -> 16-byte chunk (tid & 7) of rows (tid >> 3) + 32 u of both operands
  const int ch = tid & 7, srow = tid >> 3;
  const int8_t* drow[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) drow[u] = d0 + srow + 32 * u < end ? codes + (d0 + srow + 32 * u) * ld + 16 * ch : nullptr;

  for (int p0 = g0; p0 < g1; p0 += ISQL_PAIRS) {
    if (tid < ISQL_PAIRS) {
      int q = -1, b = 0;
      float iq = 0.f;
      if (p0 + tid < g1) {
        q = gq[p0 + tid];
        b = gbase[p0 + tid];
        if (q < 0 || q >= qn || b < 0) q = -1;
        else iq = inv_q[q];
      }
      s_pq[tid] = q, s_pb[tid] = b, s_piq[tid] = iq;
    }
    const int8_t* arow[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int p = p0 + srow + 32 * u;
      const int q = p < g1 ? gq[p] : -1;
      arow[u] = q >= 0 && q < qn ? qc + (int64_t)q * ld + 16 * ch : nullptr;
    }
    i32x4 pre_q[4], pre_d[4];
    auto fetch = [&](int k0) {
      const bool in_k = k0 + 16 * ch < ld;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        pre_q[u] = (in_k && arow[u]) ? *reinterpret_cast<const i32x4*>(arow[u] + k0) : i32x4{0, 0, 0, 0};
        pre_d[u] = (in_k && drow[u]) ? *reinterpret_cast<const i32x4*>(drow[u] + k0) : i32x4{0, 0, 0, 0};
      }
    };

    i32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = i32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

    fetch(0);
    for (int k0 = 0; k0 < ld; k0 += ISQL_BK) {
      __syncthreads();                                     // every wave has multiplied the previous block
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int row = srow + 32 * u;
        const int off = row * ISQL_BK + ((ch ^ (row & 7)) << 4);
        *reinterpret_cast<i32x4*>(&s_q[off]) = pre_q[u];
        *reinterpret_cast<i32x4*>(&s_d[off]) = pre_d[u];
      }
      __syncthreads();
      if (k0 + ISQL_BK < ld) fetch(k0 + ISQL_BK);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        i32x4 a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int qrow = wq * 64 + i * 32 + r, row = wd * 64 + i * 32 + r;
          a[i] = *reinterpret_cast<const i32x4*>(&s_q[qrow * ISQL_BK + (((2 * s + h) ^ (qrow & 7)) << 4)]);
          b[i] = *reinterpret_cast<const i32x4*>(&s_d[row * ISQL_BK + (((2 * s + h) ^ (row & 7)) << 4)]);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }

    // epilogue: convert, the query's factor, the row's factor; column = stored row, register = grouped pair
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t row = d0 + wd * 64 + j * 32 + r;
      if (row >= end) continue;
      const float idb = inv_db[row];
      const int32_t id = ids[row];
      const int64_t in_list = row - first;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int pr = wq * 64 + i * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
          const int q = s_pq[pr];
          const int64_t p = (int64_t)s_pb[pr] + in_list;
          if (q < 0 || p >= W) continue;
          cval[(int64_t)q * W + p] = ((float)acc[i][j][reg] * s_piq[pr]) * idb;
          cid[(int64_t)q * W + p] = id;
        }
      }
    }
    __syncthreads();                                       // the pair tables and the last block are read: the next query tile may write
  }
}

// the sort geometry of `pairs` items: the tile of the inversion (list_common.hpp) and the sizes of its counts
struct IsqlSort {
  int64_t tile, ntiles, ncounts, nscan;
};
inline IsqlSort isql_sort(int64_t pairs) {
  const int64_t tile = invert_tile(0, pairs), ntiles = (pairs + tile - 1) / tile, ncounts = (int64_t)AU_BINS * ntiles;
  return {tile, ntiles, ncounts, (ncounts + AU_SCAN_BLOCK - 1) / AU_SCAN_BLOCK};
}

// The grouping of one query block, enqueued: base, total (and the padding of the candidate rows where cval is given), then the pairs
// sorted by list, stably, so in (list ascending, query ascending) order, goff, gq and gbase.
int isql_group(pvs_ctx* ctx, const int64_t* d_probe, int64_t qn, int nprobe, const int64_t* d_list_off, int nlist, int64_t W, float* cval,
               int32_t* cid, int32_t* base, int32_t* total, int32_t* goff, int32_t* gq, int32_t* gbase, uint64_t* items_a, uint64_t* items_b,
               int32_t* counts, int32_t* partials) {
  const int64_t pairs = qn * nprobe;
  const IsqlSort so = isql_sort(pairs);
  hipLaunchKernelGGL(isql_base_kernel, dim3((unsigned)qn), dim3(ISQ_THREADS), 0, ctx->stream, d_probe, nprobe, d_list_off, nlist, W, base, total,
                     items_a, cval, cid);
  PVS_HIP(hipGetLastError());
  uint64_t* sorted = nullptr;
  PVS_TRY(au_launch_sort(ctx, items_a, items_b, pairs, so.tile, so.ntiles, nlist, counts, partials, &sorted));
  hipLaunchKernelGGL(au_key_off_kernel<int32_t>, dim3((nlist + 1 + AU_THREADS - 1) / AU_THREADS), dim3(AU_THREADS), 0, ctx->stream, sorted, pairs,
                     nlist, goff);
  hipLaunchKernelGGL(isql_pairs_kernel, dim3(flat_grid(ctx->num_cu, pairs)), dim3(AU_THREADS), 0, ctx->stream, sorted, pairs, nprobe, nlist, base, gq,
                     gbase);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

}  // namespace
}  // namespace pvs

using namespace pvs;

// the checks both entries share: shapes, then the host offsets -> N
static int isq_check_lists(const char* fn, int nprobe, const int64_t* h_list_off, int nlist, int slice_rows, int64_t* N) {
  if (nlist < 1 || nlist > 65536) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= nlist <= 65536 (got %d)", fn, nlist);
  if (nprobe < 1 || nprobe > std::min(nlist, ISQ_MAX_PROBE))
    PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= nprobe <= min(nlist, %d) (got nprobe=%d, nlist=%d)", fn, ISQ_MAX_PROBE, nprobe, nlist);
  if (slice_rows < 0) PVS_FAIL(PVS_ERR_INVALID, "%s: negative slice_rows", fn);
  if (!h_list_off) PVS_FAIL(PVS_ERR_INVALID, "%s: null host list_off", fn);
  const int64_t bad = offsets_first_break(h_list_off, nlist);
  if (bad == 0) PVS_FAIL(PVS_ERR_INVALID, "%s: list_off[0] must be 0", fn);
  if (bad > 0) PVS_FAIL(PVS_ERR_INVALID, "%s: list_off must not decrease (list %d)", fn, (int)(bad - 1));
  *N = h_list_off[nlist];
  if (*N >= ((int64_t)1 << 31)) PVS_FAIL(PVS_ERR_INVALID, "%s: need N < 2^31 (got %lld)", fn, (long long)*N);
  return PVS_OK;
}

PVS_EXPORT int pvs_ivf_sq8_scan_plan(pvs_ctx* ctx, int64_t nq, int nprobe, const int64_t* h_list_off, int nlist, int slice_rows,
                                     int64_t* h_plan) {
  PVS_NEED(ctx, "ctx");
  PVS_NEED(h_plan, "plan");
  if (nq < 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_sq8_scan_plan: negative nq");
  int64_t N = 0;
  PVS_TRY(isq_check_lists(__func__, nprobe, h_list_off, nlist, slice_rows, &N));
  const int64_t W = ivf_candidate_width(h_list_off, nlist, nprobe);
  const int64_t QB = ivf_query_block(std::max<int64_t>(nq, 1), W);
  const IsqSlices sl = isq_slices(ctx->num_cu, QB, W, slice_rows);
  h_plan[0] = W, h_plan[1] = QB, h_plan[2] = sl.S, h_plan[3] = sl.G;
  return PVS_OK;
}

PVS_EXPORT int pvs_ivf_sq8_scan_topk_dev(pvs_ctx* ctx, const int8_t* d_qcodes, const float* d_inv_q, int64_t nq, int L,
                                         const int64_t* d_probe, int nprobe, const int64_t* d_list_off, const int64_t* h_list_off,
                                         int nlist, const int8_t* d_codes, const float* d_inv_db, const int32_t* d_ids, int k,
                                         int slice_rows, int64_t* d_idx, float* d_val) {
  PVS_NEED(ctx, "ctx");
  if (L < 1 || L > ISQ_MAX_L) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_sq8_scan_topk_dev: need 1 <= L <= %d (got %d)", ISQ_MAX_L, L);
  if (k < 1 || k > 1024) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_sq8_scan_topk_dev: need 1 <= k <= 1024 (got %d)", k);
  if (nq < 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_sq8_scan_topk_dev: negative nq");
  int64_t N = 0;
  PVS_TRY(isq_check_lists(__func__, nprobe, h_list_off, nlist, slice_rows, &N));
  if (nq == 0) return PVS_OK;
  PVS_NEED(d_qcodes, "qcodes");
  PVS_NEED(d_inv_q, "inv_q");
  PVS_NEED(d_probe, "probe");
  PVS_NEED(d_list_off, "list_off");
  if (N > 0) {
    PVS_NEED(d_codes, "codes");
    PVS_NEED(d_inv_db, "inv_db");
    PVS_NEED(d_ids, "ids");
  }
  PVS_NEED(d_idx, "idx");
  PVS_NEED(d_val, "val");
  PVS_ALIGNED(d_qcodes, 16, "qcodes");
  PVS_ALIGNED(d_codes, 16, "codes");
  PVS_ALIGNED(d_inv_q, 4, "inv_q");
  PVS_ALIGNED(d_inv_db, 4, "inv_db");
  PVS_ALIGNED(d_probe, 8, "probe");
  PVS_ALIGNED(d_list_off, 8, "list_off");
  PVS_ALIGNED(d_ids, 4, "ids");
  PVS_ALIGNED(d_idx, 8, "idx");
  PVS_ALIGNED(d_val, 4, "val");
  PVS_HIP(hipSetDevice(ctx->device));

  const int ld = PVS_SQ8_LD(L);
  const int64_t W = ivf_candidate_width(h_list_off, nlist, nprobe);
  const int64_t QB = ivf_query_block(nq, W);
  const IsqSlices sl = isq_slices(ctx->num_cu, QB, W, slice_rows);
  const IvfCandLayout lay = ivf_cand_layout((size_t)QB, (size_t)W);
  void* block = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_IVF_CANDIDATES, lay.bytes, &block));
  float* cval = lay.val(block);
  int32_t* cid = lay.id(block);

  for (int64_t q0 = 0; q0 < nq; q0 += QB) {
    const int64_t qn = std::min(QB, nq - q0);
    {
      ScopedTimer t(ctx, T_GEMM);   // the scoring slot, as the ADC scans
      PVS_TRY(launch_lds(ctx, ivf_sq8_scan_kernel, dim3((unsigned)sl.G, (unsigned)qn), dim3(ISQ_THREADS), (size_t)ld, d_qcodes + q0 * ld,
                         d_inv_q + q0, ld, d_probe + q0 * nprobe, nprobe, d_list_off, nlist, d_codes, d_inv_db, d_ids, W, sl.S, cval, cid));
    }
    PVS_TRY(launch_topk_candidates(ctx, cid, cval, qn, W, k, d_idx + q0 * k, d_val + q0 * k));
  }
  return PVS_OK;
}

// ------------------------------------------------------------------------------------------------- the scan by list: entry points
PVS_EXPORT int pvs_ivf_sq8_group_probes_dev(pvs_ctx* ctx, const int64_t* d_probe, int64_t qn, int nprobe, const int64_t* d_list_off, int nlist,
                                            int32_t* d_base, int32_t* d_total, int32_t* d_goff, int32_t* d_gq, int32_t* d_gbase) {
  PVS_NEED(ctx, "ctx");
  if (nlist < 1 || nlist > 65536) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_sq8_group_probes_dev: need 1 <= nlist <= 65536 (got %d)", nlist);
  if (nprobe < 1 || nprobe > std::min(nlist, ISQ_MAX_PROBE))
    PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_sq8_group_probes_dev: need 1 <= nprobe <= min(nlist, %d) (got nprobe=%d, nlist=%d)", ISQ_MAX_PROBE, nprobe,
             nlist);
  if (qn < 0 || qn > 65535 || qn * nprobe > ISQL_MAX_PAIRS)
    PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_sq8_group_probes_dev: need 0 <= qn <= 65535 and qn nprobe <= %lld, one query block (got qn=%lld, nprobe=%d)",
             (long long)ISQL_MAX_PAIRS, (long long)qn, nprobe);
  PVS_NEED(d_goff, "goff");
  PVS_ALIGNED(d_goff, 4, "goff");
  PVS_HIP(hipSetDevice(ctx->device));
  if (qn == 0) {
    PVS_HIP(hipMemsetAsync(d_goff, 0, (size_t)(nlist + 1) * 4, ctx->stream));
    return PVS_OK;
  }
  PVS_NEED(d_probe, "probe");
  PVS_NEED(d_list_off, "list_off");
  PVS_NEED(d_base, "base");
  PVS_NEED(d_total, "total");
  PVS_NEED(d_gq, "gq");
  PVS_NEED(d_gbase, "gbase");
  PVS_ALIGNED(d_probe, 8, "probe");
  PVS_ALIGNED(d_list_off, 8, "list_off");
  PVS_ALIGNED(d_base, 4, "base");
  PVS_ALIGNED(d_total, 4, "total");
  PVS_ALIGNED(d_gq, 4, "gq");
  PVS_ALIGNED(d_gbase, 4, "gbase");
  const int64_t pairs = qn * nprobe;
  const IsqlSort so = isql_sort(pairs);
  const IvfSq8GroupLayout lay = ivf_sq8_group_layout((size_t)qn, (size_t)pairs, (size_t)nlist, (size_t)so.ncounts, (size_t)so.nscan);
  void* block = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_UPDATE, lay.bytes, &block));
  ScopedTimer t(ctx, T_MISC);
  return isql_group(ctx, d_probe, qn, nprobe, d_list_off, nlist, 0, nullptr, nullptr, d_base, d_total, d_goff, d_gq, d_gbase, lay.items_a(block),
                    lay.items_b(block), lay.counts(block), lay.partials(block));
}

PVS_EXPORT int pvs_ivf_sq8_scan_lists_plan(pvs_ctx* ctx, int64_t nq, int nprobe, const int64_t* h_list_off, int nlist, int query_block,
                                           int64_t* h_plan) {
  PVS_NEED(ctx, "ctx");
  PVS_NEED(h_plan, "plan");
  if (nq < 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_sq8_scan_lists_plan: negative nq");
  int64_t N = 0;
  PVS_TRY(isq_check_lists(__func__, nprobe, h_list_off, nlist, 0, &N));
  if (query_block < 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_sq8_scan_lists_plan: negative query_block");
  const IsqlPlan p = isql_plan(h_list_off, nlist, nprobe, std::max<int64_t>(nq, 1), query_block);
  h_plan[0] = p.W, h_plan[1] = p.QB, h_plan[2] = p.row_tiles, h_plan[3] = p.pairs;
  return PVS_OK;
}

PVS_EXPORT int pvs_ivf_sq8_scan_lists_topk_dev(pvs_ctx* ctx, const int8_t* d_qcodes, const float* d_inv_q, int64_t nq, int L,
                                               const int64_t* d_probe, int nprobe, const int64_t* d_list_off, const int64_t* h_list_off,
                                               int nlist, const int8_t* d_codes, const float* d_inv_db, const int32_t* d_ids, int k,
                                               int query_block, int64_t* d_idx, float* d_val) {
  PVS_NEED(ctx, "ctx");
  if (L < 1 || L > ISQ_MAX_L) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_sq8_scan_lists_topk_dev: need 1 <= L <= %d (got %d)", ISQ_MAX_L, L);
  if (k < 1 || k > 1024) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_sq8_scan_lists_topk_dev: need 1 <= k <= 1024 (got %d)", k);
  if (nq < 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_sq8_scan_lists_topk_dev: negative nq");
  int64_t N = 0;
  PVS_TRY(isq_check_lists(__func__, nprobe, h_list_off, nlist, 0, &N));
  if (query_block < 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_sq8_scan_lists_topk_dev: negative query_block");
  if (nq == 0) return PVS_OK;
  PVS_NEED(d_qcodes, "qcodes");
  PVS_NEED(d_inv_q, "inv_q");
  PVS_NEED(d_probe, "probe");
  PVS_NEED(d_list_off, "list_off");
  if (N > 0) {
    PVS_NEED(d_codes, "codes");
    PVS_NEED(d_inv_db, "inv_db");
    PVS_NEED(d_ids, "ids");
  }
  PVS_NEED(d_idx, "idx");
  PVS_NEED(d_val, "val");
  PVS_ALIGNED(d_qcodes, 16, "qcodes");
  PVS_ALIGNED(d_codes, 16, "codes");
  PVS_ALIGNED(d_inv_q, 4, "inv_q");
  PVS_ALIGNED(d_inv_db, 4, "inv_db");
  PVS_ALIGNED(d_probe, 8, "probe");
  PVS_ALIGNED(d_list_off, 8, "list_off");
  PVS_ALIGNED(d_ids, 4, "ids");
  PVS_ALIGNED(d_idx, 8, "idx");
  PVS_ALIGNED(d_val, 4, "val");
  PVS_HIP(hipSetDevice(ctx->device));

  const int ld = PVS_SQ8_LD(L);
  const IsqlPlan plan = isql_plan(h_list_off, nlist, nprobe, nq, query_block);
  const int64_t W = plan.W, QB = plan.QB;
  const IvfCandLayout lay = ivf_cand_layout((size_t)QB, (size_t)W);
  void* block = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_IVF_CANDIDATES, lay.bytes, &block));
  float* cval = lay.val(block);
  int32_t* cid = lay.id(block);
  const IsqlSort so = isql_sort(plan.pairs);
  const IvfSq8GroupLayout gl = ivf_sq8_group_layout((size_t)QB, (size_t)plan.pairs, (size_t)nlist, (size_t)so.ncounts, (size_t)so.nscan);
  void* gblock = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_UPDATE, gl.bytes, &gblock));
  int32_t *tile_off = gl.tile_off(gblock), *goff = gl.goff(gblock), *gq = gl.gq(gblock), *gbase = gl.gbase(gblock);

  if (plan.row_tiles > 0) {
    ScopedTimer t(ctx, T_MISC);
    hipLaunchKernelGGL(isql_tile_off_kernel, dim3(1), dim3(ISQ_THREADS), 0, ctx->stream, d_list_off, nlist, tile_off);
    PVS_HIP(hipGetLastError());
  }
  for (int64_t q0 = 0; q0 < nq; q0 += QB) {
    const int64_t qn = std::min(QB, nq - q0);
    {
      ScopedTimer t(ctx, T_MISC);
      PVS_TRY(isql_group(ctx, d_probe + q0 * nprobe, qn, nprobe, d_list_off, nlist, W, cval, cid, gl.base(gblock), gl.total(gblock), goff, gq, gbase,
                         gl.items_a(gblock), gl.items_b(gblock), gl.counts(gblock), gl.partials(gblock)));
    }
    if (plan.row_tiles > 0) {
      ScopedTimer t(ctx, T_GEMM);   // the scoring slot, as the scan by query
      hipLaunchKernelGGL(ivf_sq8_tile_kernel, dim3((unsigned)plan.row_tiles), dim3(ISQL_THREADS), 0, ctx->stream, d_qcodes + q0 * ld, d_inv_q + q0,
                         (int)qn, ld, d_list_off, nlist, tile_off, goff, gq, gbase, d_codes, d_inv_db, d_ids, N, W, cval, cid);
      PVS_HIP(hipGetLastError());
    }
    PVS_TRY(launch_topk_candidates(ctx, cid, cval, qn, W, k, d_idx + q0 * k, d_val + q0 * k));
  }
  return PVS_OK;
}
