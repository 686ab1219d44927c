// Index maintenance: rows join and leave a resident index without a rebuild from the host.
//   pvs_keep_mask_dev        r removed indices -> uint8 keep mask of n entries (fill with 1, scatter 0)
//   pvs_keep_positions_dev   keep mask -> pos[i] = kept entries before i, pos[n] = the total: a three-level scan, four launches
//   pvs_compact_rows_dev     out[pos[i]] = rows[i] for kept i; out-of-place in one pass, in place window by window through a
//                            bounded staging block (WS_UPDATE)
//   pvs_ivf_insert_dev       stored arrays of n rows + b new rows -> the merged storage in (list, original index) order
//   pvs_ivf_remove_dev       keep mask by original index -> compacted stored arrays, remapped ids, new list offsets
//   pvs_copy_dev             device-to-device copy on the context's stream
// Everything here is data movement and integer counting: no floating-point arithmetic, no atomics, and every output element is
// written by exactly one lane, so the results do not depend on scheduling.  tests/update_numpy.py restates each entry point.
//
// The movers are bandwidth kernels.  A row of row_bytes moves as row_bytes / V units of V bytes, V the widest of 16, 8, 4, 2, 1
// that divides the row length and both base addresses; a lane owns one unit at a time and keeps MOVE_U of them in flight.  The
// only indirection is one keep byte and one position (or one source index) per unit, read from arrays that neighbouring lanes share.
// From list_common.hpp: the block scan, the two offset kernels, the grid rule, the overlap and offset checks.
#include <algorithm>

#include "list_common.hpp"

namespace pvs {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_TILE = PVS_SCAN_TILE;                 // flags one workgroup counts
constexpr int SCAN_PER_LANE = SCAN_TILE / SCAN_THREADS;  // 8: one 8-byte load where the mask is 8-byte aligned
static_assert(SCAN_PER_LANE == 8, "a lane reads its flags as one 8-byte word");
constexpr int64_t SCAN_MAX_N = (int64_t)1 << 31;         // tiles <= 2^20, tile blocks <= 512 <= SCAN_TILE: three levels suffice
constexpr int MOVE_THREADS = 256;
constexpr int MOVE_U = 4;                                // units a lane keeps in flight
constexpr int64_t UPDATE_STAGE_BYTES = (int64_t)64 << 20;   // staging block of the in-place compaction
constexpr int64_t MOVE_MAX_ROW_BYTES = (int64_t)1 << 30;

// ------------------------------------------------------------------------------------------------- keep positions
// the 8 flags of a lane as bits 0..7 (bit e: keep[i0 + e] != 0); entries at or beyond n count as 0
__device__ __forceinline__ unsigned load_flags(const uint8_t* __restrict__ keep, int64_t i0, int64_t n, bool aligned8) {
  unsigned bits = 0;
  if (i0 + SCAN_PER_LANE <= n && aligned8) {
    const uint64_t w = *reinterpret_cast<const uint64_t*>(keep + i0);
#pragma unroll
    for (int e = 0; e < SCAN_PER_LANE; ++e) bits |= ((w >> (8 * e)) & 0xffu) ? (1u << e) : 0u;
  } else {
#pragma unroll
    for (int e = 0; e < SCAN_PER_LANE; ++e)
      if (i0 + e < n && keep[i0 + e]) bits |= 1u << e;
  }
  return bits;
}

// level 1: kept flags of each tile
__global__ __launch_bounds__(SCAN_THREADS) void scan_tile_count_kernel(const uint8_t* __restrict__ keep, int64_t n, bool aligned8,
                                                                       int64_t* __restrict__ tile_sum) {
  __shared__ int tmp[4];
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)tid * SCAN_PER_LANE;
  const int c = __popc(load_flags(keep, i0, n, aligned8));
  const int incl = block_incl_scan(c, tmp, tid & 63, tid >> 6);
  if (tid == SCAN_THREADS - 1) tile_sum[blockIdx.x] = incl;
}

// levels 2 and 3: `count` sums, SCAN_TILE per workgroup -> their exclusive prefixes within the workgroup's block (in place) and the
// block's total
__global__ __launch_bounds__(SCAN_THREADS) void scan_sums_kernel(int64_t* __restrict__ sums, int64_t count, int64_t* __restrict__ block_sum) {
  __shared__ int64_t wtot[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)tid * SCAN_PER_LANE;
  int64_t v[SCAN_PER_LANE], mine = 0;
#pragma unroll
  for (int e = 0; e < SCAN_PER_LANE; ++e) {
    v[e] = i0 + e < count ? sums[i0 + e] : 0;
    mine += v[e];
  }
  int64_t incl = mine;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const int64_t o = __shfl_up(incl, s, 64);
    if (lane >= s) incl += o;
  }
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  int64_t off = 0;
  for (int w = 0; w < wave; ++w) off += wtot[w];
  int64_t run = off + incl - mine;
#pragma unroll
  for (int e = 0; e < SCAN_PER_LANE; ++e) {
    if (i0 + e < count) sums[i0 + e] = run;
    run += v[e];
  }
  if (tid == SCAN_THREADS - 1) block_sum[blockIdx.x] = off + incl;
}

// level 1 again, now with the prefixes of the levels above: pos[i] for the tile's entries, and pos[n] from the last tile
__global__ __launch_bounds__(SCAN_THREADS) void scan_final_kernel(const uint8_t* __restrict__ keep, int64_t n, bool aligned8,
                                                                  const int64_t* __restrict__ tile_ex, const int64_t* __restrict__ block_ex,
                                                                  int64_t* __restrict__ pos) {
  __shared__ int tmp[4];
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)tid * SCAN_PER_LANE;
  const unsigned bits = load_flags(keep, i0, n, aligned8);
  const int c = __popc(bits);
  const int incl = block_incl_scan(c, tmp, tid & 63, tid >> 6);
  int64_t run = block_ex[blockIdx.x / SCAN_TILE] + tile_ex[blockIdx.x] + (incl - c);
#pragma unroll
  for (int e = 0; e < SCAN_PER_LANE; ++e) {
    if (i0 + e < n) pos[i0 + e] = run;
    run += (bits >> e) & 1u;
    if (i0 + e + 1 == n) pos[n] = run;
  }
}

struct ScanPartials {
  int64_t *tile, *block, *top;   // tile sums [ntiles], block sums [SCAN_TILE], the total [1]
};

// pos[0 .. n] from keep[0 .. n): four launches for any 1 <= n <= SCAN_MAX_N
static int launch_keep_positions(pvs_ctx* ctx, const uint8_t* keep, int64_t n, int64_t* pos, const ScanPartials& p) {
  const int64_t ntiles = (n + SCAN_TILE - 1) / SCAN_TILE, nblocks = (ntiles + SCAN_TILE - 1) / SCAN_TILE;
  const bool aligned8 = reinterpret_cast<uintptr_t>(keep) % 8 == 0;
  ScopedTimer t(ctx, T_MISC);
  hipLaunchKernelGGL(scan_tile_count_kernel, dim3((unsigned)ntiles), dim3(SCAN_THREADS), 0, ctx->stream, keep, n, aligned8, p.tile);
  hipLaunchKernelGGL(scan_sums_kernel, dim3((unsigned)nblocks), dim3(SCAN_THREADS), 0, ctx->stream, p.tile, ntiles, p.block);
  hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(SCAN_THREADS), 0, ctx->stream, p.block, nblocks, p.top);
  hipLaunchKernelGGL(scan_final_kernel, dim3((unsigned)ntiles), dim3(SCAN_THREADS), 0, ctx->stream, keep, n, aligned8, p.tile, p.block, pos);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

__global__ void scatter_zero_kernel(const int64_t* __restrict__ removed, int64_t r, int64_t n, uint8_t* __restrict__ keep) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < r; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = removed[j];
    if (i >= 0 && i < n) keep[i] = 0;
  }
}

// ------------------------------------------------------------------------------------------------- row movers
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // 16- and 8-byte units as plain vectors: the per-lane arrays below stay in registers
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// Unit u of a launch is column unit u % upr of row row0 + u / upr; a kept row goes to row pos[row] - *pos_base of dst.  src and dst do
// not overlap (the in-place compaction gathers into the staging block).  total < 2^31, so the index arithmetic is 32-bit.
template <typename V>
__global__ __launch_bounds__(MOVE_THREADS) void move_rows_kernel(const char* __restrict__ src, char* __restrict__ dst,
                                                                 const uint8_t* __restrict__ keep, const int64_t* __restrict__ pos,
                                                                 const int64_t* __restrict__ pos_base, int64_t row0, uint32_t upr,
                                                                 uint32_t total, int64_t row_bytes) {
  const int64_t base = pos_base ? *pos_base : 0;
  const uint32_t stride = gridDim.x * MOVE_THREADS;
  for (uint32_t u0 = blockIdx.x * MOVE_THREADS + threadIdx.x; u0 < total; u0 += MOVE_U * stride) {
    V v[MOVE_U];
    int64_t to[MOVE_U];
    bool ok[MOVE_U];
#pragma unroll
    for (int e = 0; e < MOVE_U; ++e) {
      const uint32_t u = u0 + e * stride;
      ok[e] = false;
      if (u < total) {
        const uint32_t r = u / upr, c = u - r * upr;
        const int64_t row = row0 + r;
        if (keep[row]) {
          ok[e] = true;
          to[e] = (pos[row] - base) * row_bytes + (int64_t)c * sizeof(V);
          v[e] = *reinterpret_cast<const V*>(src + row * row_bytes + (int64_t)c * sizeof(V));
        }
      }
    }
#pragma unroll
    for (int e = 0; e < MOVE_U; ++e)
      if (ok[e]) *reinterpret_cast<V*>(dst + to[e]) = v[e];
  }
}

// the staged rows of window [a, b) back to their place: pos[b] - pos[a] rows from the start of the staging block to row pos[a] of out
template <typename V>
__global__ __launch_bounds__(MOVE_THREADS) void unstage_rows_kernel(const char* __restrict__ stage, char* __restrict__ out,
                                                                    const int64_t* __restrict__ pos, int64_t a, int64_t b, int64_t row_bytes) {
  const int64_t pa = pos[a];
  const int64_t units = (pos[b] - pa) * row_bytes / (int64_t)sizeof(V);
  const V* s = reinterpret_cast<const V*>(stage);
  V* d = reinterpret_cast<V*>(out + pa * row_bytes);
  const int64_t stride = (int64_t)gridDim.x * MOVE_THREADS;
  for (int64_t u = (int64_t)blockIdx.x * MOVE_THREADS + threadIdx.x; u < units; u += stride) d[u] = s[u];
}

// out row j0 + u / upr = row srcmap[j] of `old` (srcmap[j] < n_old) or row srcmap[j] - n_old of `fresh`
template <typename V>
__global__ __launch_bounds__(MOVE_THREADS) void gather_rows2_kernel(const char* __restrict__ old, const char* __restrict__ fresh,
                                                                    int64_t n_old, const int32_t* __restrict__ srcmap, int64_t j0,
                                                                    uint32_t upr, uint32_t total, int64_t row_bytes, char* __restrict__ dst) {
  const uint32_t stride = gridDim.x * MOVE_THREADS;
  for (uint32_t u0 = blockIdx.x * MOVE_THREADS + threadIdx.x; u0 < total; u0 += MOVE_U * stride) {
    V v[MOVE_U];
#pragma unroll
    for (int e = 0; e < MOVE_U; ++e) {
      const uint32_t u = u0 + e * stride;
      if (u < total) {
        const uint32_t r = u / upr, c = u - r * upr;
        const int64_t s = srcmap[j0 + r];
        const char* from = s < n_old ? old + s * row_bytes : fresh + (s - n_old) * row_bytes;
        v[e] = *reinterpret_cast<const V*>(from + (int64_t)c * sizeof(V));
      }
    }
#pragma unroll
    for (int e = 0; e < MOVE_U; ++e) {
      const uint32_t u = u0 + e * stride;
      if (u < total) *reinterpret_cast<V*>(dst + (j0 + u / upr) * row_bytes + (int64_t)(u % upr) * sizeof(V)) = v[e];
    }
  }
}

// the widest unit that divides the row length and every base address
static int move_width(int64_t row_bytes, std::initializer_list<const void*> bases) {
  uintptr_t bits = (uintptr_t)row_bytes;
  for (const void* p : bases) bits |= reinterpret_cast<uintptr_t>(p);
  for (int w = 16; w > 1; w >>= 1)
    if (bits % w == 0) return w;
  return 1;
}

static unsigned move_grid(const pvs_ctx* ctx, int64_t units) {
  return flat_grid(ctx->num_cu, units, (int64_t)MOVE_THREADS * MOVE_U);
}

// f(V{}) for the unit type of `width` bytes
template <class F>
static int dispatch_width(int width, F&& f) {
  switch (width) {
    case 16: return f(u32x4{});
    case 8: return f(u32x2{});
    case 4: return f(uint32_t{});
    case 2: return f(uint16_t{});
    default: return f(uint8_t{});
  }
}

// rows [a, b) of src -> their positions (less *pos_base) in dst, in launches of fewer than 2^31 units
static int launch_move_rows(pvs_ctx* ctx, const void* src, void* dst, const uint8_t* keep, const int64_t* pos, const int64_t* pos_base,
                            int64_t a, int64_t b, int64_t row_bytes) {
  const int width = move_width(row_bytes, {src, (const void*)dst});
  const int64_t upr = row_bytes / width;
  const int64_t rows_per_launch = std::max<int64_t>(1, (((int64_t)1 << 31) - 1) / upr);
  return dispatch_width(width, [&](auto v) -> int {
    using V = decltype(v);
    for (int64_t r0 = a; r0 < b; r0 += rows_per_launch) {
      const int64_t rn = std::min(rows_per_launch, b - r0);
      hipLaunchKernelGGL((move_rows_kernel<V>), dim3(move_grid(ctx, rn * upr)), dim3(MOVE_THREADS), 0, ctx->stream,
                         static_cast<const char*>(src), static_cast<char*>(dst), keep, pos, pos_base, r0, (uint32_t)upr,
                         (uint32_t)(rn * upr), row_bytes);
      PVS_HIP(hipGetLastError());
    }
    return PVS_OK;
  });
}

// ------------------------------------------------------------------------------------------------- inverted lists
// One lane per merged stored row j: its list is the last l with out_off[l] <= j (a list that starts at j and is not empty); inside the
// list the old rows come first, then the new rows of the list in arrival order.  Writes the source of the row's code (srcmap), its
// id and its norm.
__global__ __launch_bounds__(256) void ivf_insert_plan_kernel(const int64_t* __restrict__ out_off, const int64_t* __restrict__ list_off,
                                                              const int64_t* __restrict__ new_off, int nlist,
                                                              const int32_t* __restrict__ ids, const float* __restrict__ inv,
                                                              const int32_t* __restrict__ perm, const float* __restrict__ new_inv, int64_t n,
                                                              int64_t b, int64_t total, int32_t* __restrict__ srcmap, int32_t* __restrict__ out_ids,
                                                              float* __restrict__ out_inv) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (int64_t)gridDim.x * blockDim.x) {
    int lo = 0, hi = nlist - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (out_off[mid] <= j) lo = mid;
      else hi = mid - 1;
    }
    const int64_t r = j - out_off[lo], first = list_off[lo], old_len = list_off[lo + 1] - first;
    if (r < old_len) {
      const int64_t s = first + r;
      srcmap[j] = (int32_t)s;
      out_ids[j] = ids[s];
      out_inv[j] = inv[s];
    } else {
      const int64_t p = min(max((int64_t)perm[new_off[lo] + (r - old_len)], (int64_t)0), b - 1);   // a permutation of 0 .. b-1 (precondition)
      srcmap[j] = (int32_t)(n + p);
      out_ids[j] = (int32_t)(n + p);
      out_inv[j] = new_inv[p];
    }
  }
}

__global__ void ivf_stored_keep_kernel(const int32_t* __restrict__ ids, const uint8_t* __restrict__ keep, int64_t n,
                                       uint8_t* __restrict__ skeep) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
  {
    const int64_t id = ids[i];
    skeep[i] = id >= 0 && id < n && keep[id] ? 1 : 0;   // an id outside [0, n) breaks a precondition: the row is dropped, nothing is read out of bounds
  }
}

__global__ void ivf_remap_kernel(const int32_t* __restrict__ ids, const float* __restrict__ inv, const uint8_t* __restrict__ skeep,
                                 const int64_t* __restrict__ spos, const int64_t* __restrict__ pos_orig, int64_t n,
                                 int32_t* __restrict__ out_ids, float* __restrict__ out_inv) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    if (skeep[i]) {
      const int64_t p = spos[i];
      out_ids[p] = (int32_t)pos_orig[ids[i]];
      out_inv[p] = inv[i];
    }
}

static int check_offsets(const char* fn, const char* what, const int64_t* h, int nlist) {
  const int64_t bad = offsets_first_break(h, nlist);
  if (bad == 0) PVS_FAIL(PVS_ERR_INVALID, "%s: %s[0] must be 0", fn, what);
  if (bad > 0) PVS_FAIL(PVS_ERR_INVALID, "%s: %s must not decrease (list %d)", fn, what, (int)(bad - 1));
  return PVS_OK;
}

}  // namespace pvs

using namespace pvs;

PVS_EXPORT int pvs_copy_dev(pvs_ctx* ctx, void* d_dst, const void* d_src, size_t bytes) {
  PVS_NEED(ctx, "ctx");
  if (bytes == 0) return PVS_OK;
  PVS_NEED(d_dst, "dst");
  PVS_NEED(d_src, "src");
  if (ranges_overlap(d_dst, (int64_t)bytes, d_src, (int64_t)bytes)) PVS_FAIL(PVS_ERR_INVALID, "pvs_copy_dev: dst overlaps src");
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer t(ctx, T_MISC);
  PVS_HIP(hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  return PVS_OK;
}

PVS_EXPORT int pvs_keep_mask_dev(pvs_ctx* ctx, const int64_t* d_removed, int64_t r, int64_t n, uint8_t* d_keep) {
  PVS_NEED(ctx, "ctx");
  if (n < 0 || r < 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_keep_mask_dev: need n >= 0 and r >= 0 (got n=%lld, r=%lld)", (long long)n, (long long)r);
  if (n == 0) return PVS_OK;
  PVS_NEED(d_keep, "keep");
  if (r > 0) {
    PVS_NEED(d_removed, "removed");
    PVS_ALIGNED(d_removed, 8, "removed");
    if (ranges_overlap(d_removed, r * 8, d_keep, n)) PVS_FAIL(PVS_ERR_INVALID, "pvs_keep_mask_dev: keep overlaps removed");
  }
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer t(ctx, T_MISC);
  PVS_HIP(hipMemsetAsync(d_keep, 1, (size_t)n, ctx->stream));
  if (r > 0) {
    hipLaunchKernelGGL(scatter_zero_kernel, dim3(flat_grid(ctx->num_cu, r)), dim3(256), 0, ctx->stream, d_removed, r, n, d_keep);
    PVS_HIP(hipGetLastError());
  }
  return PVS_OK;
}

PVS_EXPORT int pvs_keep_positions_dev(pvs_ctx* ctx, const uint8_t* d_keep, int64_t n, int64_t* d_pos) {
  PVS_NEED(ctx, "ctx");
  if (n < 0 || n > SCAN_MAX_N) PVS_FAIL(PVS_ERR_INVALID, "pvs_keep_positions_dev: need 0 <= n <= 2^31 (got %lld)", (long long)n);
  PVS_NEED(d_pos, "pos");
  PVS_ALIGNED(d_pos, 8, "pos");
  PVS_HIP(hipSetDevice(ctx->device));
  if (n == 0) {
    PVS_HIP(hipMemsetAsync(d_pos, 0, 8, ctx->stream));
    return PVS_OK;
  }
  PVS_NEED(d_keep, "keep");
  if (ranges_overlap(d_keep, n, d_pos, (n + 1) * 8)) PVS_FAIL(PVS_ERR_INVALID, "pvs_keep_positions_dev: pos overlaps keep");
  const UpdateScanLayout lay = update_scan_layout((size_t)((n + SCAN_TILE - 1) / SCAN_TILE), SCAN_TILE);
  void* block = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_UPDATE, lay.bytes, &block));
  return launch_keep_positions(ctx, d_keep, n, d_pos, {lay.tile(block), lay.block(block), lay.top(block)});
}

PVS_EXPORT int pvs_compact_rows_dev(pvs_ctx* ctx, const void* d_rows, int64_t n, int64_t row_bytes, const uint8_t* d_keep,
                                    const int64_t* d_pos, int64_t first, void* d_out) {
  PVS_NEED(ctx, "ctx");
  if (n < 0 || row_bytes < 1 || first < 0)
    PVS_FAIL(PVS_ERR_INVALID, "pvs_compact_rows_dev: need n >= 0, row_bytes >= 1, first >= 0 (got n=%lld, row_bytes=%lld, first=%lld)",
             (long long)n, (long long)row_bytes, (long long)first);
  if (row_bytes > MOVE_MAX_ROW_BYTES) PVS_FAIL(PVS_ERR_UNSUPPORTED, "pvs_compact_rows_dev: rows of more than 2^30 bytes");
  if ((double)n * (double)row_bytes > 9e18) PVS_FAIL(PVS_ERR_INVALID, "pvs_compact_rows_dev: the matrix is too large");
  if (n == 0) return PVS_OK;
  PVS_NEED(d_rows, "rows");
  PVS_NEED(d_keep, "keep");
  PVS_NEED(d_pos, "pos");
  PVS_NEED(d_out, "out");
  PVS_ALIGNED(d_pos, 8, "pos");
  const bool in_place = d_out == d_rows;
  if (!in_place && ranges_overlap(d_rows, n * row_bytes, d_out, n * row_bytes))
    PVS_FAIL(PVS_ERR_INVALID, "pvs_compact_rows_dev: out overlaps rows without being rows");
  if (ranges_overlap(d_keep, n, d_out, n * row_bytes) || ranges_overlap(d_pos, (n + 1) * 8, d_out, n * row_bytes))
    PVS_FAIL(PVS_ERR_INVALID, "pvs_compact_rows_dev: out overlaps keep or pos");
  PVS_HIP(hipSetDevice(ctx->device));
  if (!in_place) {
    ScopedTimer t(ctx, T_MISC);
    return launch_move_rows(ctx, d_rows, d_out, d_keep, d_pos, nullptr, 0, n, row_bytes);
  }
  if (first >= n) return PVS_OK;
  // Window [a, b) of source rows: its kept rows go to the staging block, then to rows [pos[a], pos[b]) of the matrix.  pos[b] <= b,
  // so the write stays below the next window's first source row, and every row it overwrites was read by this window or an earlier
  // one; the launches are ordered by the stream.
  const int64_t budget = std::max<int64_t>(1, UPDATE_STAGE_BYTES / row_bytes);
  const int cap = ctx->opt[PVS_OPT_UPDATE_WINDOW_ROWS];
  const int64_t W = cap > 0 && cap < budget ? cap : budget;
  char* stage = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_UPDATE, update_stage_bytes((size_t)std::min(W, n - first), (size_t)row_bytes), &stage));
  const int width = move_width(row_bytes, {d_rows, (const void*)stage});
  ScopedTimer t(ctx, T_MISC);
  for (int64_t a = first; a < n; a += W) {
    const int64_t b = std::min(n, a + W);
    PVS_TRY(launch_move_rows(ctx, d_rows, stage, d_keep, d_pos, d_pos + a, a, b, row_bytes));
    PVS_TRY(dispatch_width(width, [&](auto v) -> int {
      using V = decltype(v);
      hipLaunchKernelGGL((unstage_rows_kernel<V>), dim3(move_grid(ctx, (b - a) * row_bytes / width)), dim3(MOVE_THREADS), 0, ctx->stream,
                         stage, static_cast<char*>(d_out), d_pos, a, b, row_bytes);
      PVS_HIP(hipGetLastError());
      return PVS_OK;
    }));
  }
  return PVS_OK;
}

static int ivf_update_check(const char* fn, int m, int nlist) {
  if (m < 1 || m > (1 << 24)) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= m <= 2^24 (got %d)", fn, m);
  if (nlist < 1 || nlist > 65536) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= nlist <= 65536 (got %d)", fn, nlist);
  return PVS_OK;
}

PVS_EXPORT int pvs_ivf_insert_dev(pvs_ctx* ctx, int m, int nlist, const uint8_t* d_codes, const float* d_inv_db, const int32_t* d_ids,
                                  const int64_t* d_list_off, const int64_t* h_list_off, const uint8_t* d_new_codes,
                                  const float* d_new_inv, const int64_t* d_new_off, const int64_t* h_new_off, const int32_t* d_perm,
                                  uint8_t* d_out_codes, float* d_out_inv, int32_t* d_out_ids, int64_t* d_out_list_off) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(ivf_update_check(__func__, m, nlist));
  PVS_NEED(h_list_off, "host list_off");
  PVS_NEED(h_new_off, "host new_off");
  PVS_TRY(check_offsets(__func__, "list_off", h_list_off, nlist));
  PVS_TRY(check_offsets(__func__, "new_off", h_new_off, nlist));
  const int64_t n = h_list_off[nlist], b = h_new_off[nlist], total = n + b;
  if (total >= ((int64_t)1 << 31)) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_insert_dev: need n + b < 2^31 (got %lld)", (long long)total);
  PVS_NEED(d_list_off, "list_off");
  PVS_NEED(d_new_off, "new_off");
  PVS_NEED(d_out_list_off, "out list_off");
  PVS_ALIGNED(d_list_off, 8, "list_off");
  PVS_ALIGNED(d_new_off, 8, "new_off");
  PVS_ALIGNED(d_out_list_off, 8, "out list_off");
  if (n > 0) {
    PVS_NEED(d_codes, "codes");
    PVS_NEED(d_inv_db, "inv_db");
    PVS_NEED(d_ids, "ids");
  }
  if (b > 0) {
    PVS_NEED(d_new_codes, "new codes");
    PVS_NEED(d_new_inv, "new inv_db");
    PVS_NEED(d_perm, "perm");
  }
  if (total > 0) {
    PVS_NEED(d_out_codes, "out codes");
    PVS_NEED(d_out_inv, "out inv_db");
    PVS_NEED(d_out_ids, "out ids");
  }
  for (const void* p : {(const void*)d_inv_db, (const void*)d_ids, (const void*)d_new_inv, (const void*)d_perm, (const void*)d_out_inv,
                        (const void*)d_out_ids})
    if (reinterpret_cast<uintptr_t>(p) % 4) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_insert_dev: norms, ids and perm must be 4-byte aligned");
  if (ranges_overlap(d_out_codes, total * m, d_codes, n * m) || ranges_overlap(d_out_codes, total * m, d_new_codes, b * m) ||
      ranges_overlap(d_out_inv, total * 4, d_inv_db, n * 4) || ranges_overlap(d_out_inv, total * 4, d_new_inv, b * 4) ||
      ranges_overlap(d_out_ids, total * 4, d_ids, n * 4) || ranges_overlap(d_out_ids, total * 4, d_perm, b * 4) ||
      ranges_overlap(d_out_list_off, (nlist + 1) * 8, d_list_off, (nlist + 1) * 8) ||
      ranges_overlap(d_out_list_off, (nlist + 1) * 8, d_new_off, (nlist + 1) * 8))
    PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_insert_dev: an output overlaps an input");
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer t(ctx, T_MISC);
  hipLaunchKernelGGL(sum_offsets_kernel<int64_t>, dim3((nlist + 1 + 255) / 256), dim3(256), 0, ctx->stream, d_list_off, d_new_off, nlist + 1,
                     d_out_list_off);
  PVS_HIP(hipGetLastError());
  if (total == 0) return PVS_OK;
  int32_t* srcmap = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_UPDATE, (size_t)total * sizeof(int32_t), &srcmap));
  hipLaunchKernelGGL(ivf_insert_plan_kernel, dim3(flat_grid(ctx->num_cu, total)), dim3(256), 0, ctx->stream, d_out_list_off, d_list_off, d_new_off,
                     nlist, d_ids, d_inv_db, d_perm, d_new_inv, n, b, total, srcmap, d_out_ids, d_out_inv);
  PVS_HIP(hipGetLastError());
  const int width = move_width(m, {(const void*)(n > 0 ? d_codes : nullptr), (const void*)(b > 0 ? d_new_codes : nullptr), (const void*)d_out_codes});
  const int64_t upr = m / width;
  const int64_t rows_per_launch = std::max<int64_t>(1, (((int64_t)1 << 31) - 1) / upr);
  return dispatch_width(width, [&](auto v) -> int {
    using V = decltype(v);
    for (int64_t j0 = 0; j0 < total; j0 += rows_per_launch) {
      const int64_t rn = std::min(rows_per_launch, total - j0);
      hipLaunchKernelGGL((gather_rows2_kernel<V>), dim3(move_grid(ctx, rn * upr)), dim3(MOVE_THREADS), 0, ctx->stream,
                         reinterpret_cast<const char*>(d_codes), reinterpret_cast<const char*>(d_new_codes), n, srcmap, j0, (uint32_t)upr,
                         (uint32_t)(rn * upr), (int64_t)m, reinterpret_cast<char*>(d_out_codes));
      PVS_HIP(hipGetLastError());
    }
    return PVS_OK;
  });
}

PVS_EXPORT int pvs_ivf_remove_dev(pvs_ctx* ctx, int m, int nlist, int64_t n, const uint8_t* d_codes, const float* d_inv_db,
                                  const int32_t* d_ids, const int64_t* d_list_off, const uint8_t* d_keep, const int64_t* d_pos,
                                  uint8_t* d_out_codes, float* d_out_inv, int32_t* d_out_ids, int64_t* d_out_list_off) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(ivf_update_check(__func__, m, nlist));
  if (n < 0 || n >= ((int64_t)1 << 31)) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_remove_dev: need 0 <= n < 2^31 (got %lld)", (long long)n);
  PVS_NEED(d_list_off, "list_off");
  PVS_NEED(d_out_list_off, "out list_off");
  PVS_ALIGNED(d_list_off, 8, "list_off");
  PVS_ALIGNED(d_out_list_off, 8, "out list_off");
  PVS_HIP(hipSetDevice(ctx->device));
  if (n == 0) {
    PVS_HIP(hipMemsetAsync(d_out_list_off, 0, (size_t)(nlist + 1) * 8, ctx->stream));
    return PVS_OK;
  }
  PVS_NEED(d_codes, "codes");
  PVS_NEED(d_inv_db, "inv_db");
  PVS_NEED(d_ids, "ids");
  PVS_NEED(d_keep, "keep");
  PVS_NEED(d_pos, "pos");
  PVS_NEED(d_out_codes, "out codes");
  PVS_NEED(d_out_inv, "out inv_db");
  PVS_NEED(d_out_ids, "out ids");
  PVS_ALIGNED(d_pos, 8, "pos");
  for (const void* p : {(const void*)d_inv_db, (const void*)d_ids, (const void*)d_out_inv, (const void*)d_out_ids})
    if (reinterpret_cast<uintptr_t>(p) % 4) PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_remove_dev: norms and ids must be 4-byte aligned");
  if (ranges_overlap(d_out_codes, n * m, d_codes, n * m) || ranges_overlap(d_out_inv, n * 4, d_inv_db, n * 4) ||
      ranges_overlap(d_out_ids, n * 4, d_ids, n * 4) || ranges_overlap(d_out_list_off, (nlist + 1) * 8, d_list_off, (nlist + 1) * 8))
    PVS_FAIL(PVS_ERR_INVALID, "pvs_ivf_remove_dev: an output overlaps an input");
  const IvfRemoveLayout lay = ivf_remove_layout((size_t)n, (size_t)((n + SCAN_TILE - 1) / SCAN_TILE), SCAN_TILE);
  void* block = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_UPDATE, lay.bytes, &block));
  uint8_t* skeep = lay.keep(block);
  int64_t* spos = lay.pos(block);
  {
    ScopedTimer t(ctx, T_MISC);
    hipLaunchKernelGGL(ivf_stored_keep_kernel, dim3(flat_grid(ctx->num_cu, n)), dim3(256), 0, ctx->stream, d_ids, d_keep, n, skeep);
    PVS_HIP(hipGetLastError());
  }
  PVS_TRY(launch_keep_positions(ctx, skeep, n, spos, {lay.tile(block), lay.block(block), lay.top(block)}));
  ScopedTimer t(ctx, T_MISC);
  hipLaunchKernelGGL(ivf_remap_kernel, dim3(flat_grid(ctx->num_cu, n)), dim3(256), 0, ctx->stream, d_ids, d_inv_db, skeep, spos, d_pos, n, d_out_ids,
                     d_out_inv);
  hipLaunchKernelGGL(remap_offsets_kernel<int64_t>, dim3((nlist + 1 + 255) / 256), dim3(256), 0, ctx->stream, d_list_off, spos, n, nlist + 1,
                     d_out_list_off);
  PVS_HIP(hipGetLastError());
  return launch_move_rows(ctx, d_codes, d_out_codes, skeep, spos, nullptr, 0, n, m);
}
