// Top-m nearest centroids of descriptor rows ("multiple assignment"): pvs_kmeans_topm_dev.
//
// The values are DEFINED in include/pvsim.h: v_j = fmaf(-2, dot_j, |c_j|^2) with dot_j the float32 fma chain of the exact assignment
// kernel (assign_kernel, vlad.hip), a NaN or +inf v_j counted as +inf, and the list of a row is its first m centroids in the order
// (v ascending, j ascending).  That order is total, so the list does not depend on how the vocabulary or the rows are cut.
//
//   topm_kernel (A)   workgroup (row block, split): 256 rows x a contiguous range of centroid blocks.  The block is staged in LDS and
//                     the tile is formed by the MFMA sequence of assign_kernel (same operand roles, same k order: the same bits).
//                     Every lane keeps a sorted list of MC >= m (v, j) pairs in registers for its row; a value is compared with the
//                     list's worst first and inserted only when it wins.  The two half-waves of a row merge their lists at the end.
//                     splits == 1: the lists are the result.  Otherwise they go to the workspace as [row][split][m].
//   topm_merge_kernel (B)   one wave per row: the splits x m candidates are dealt over the lanes, every lane keeps its own list, and a
//                     butterfly over the lanes merges them by (v, j).
// No global atomics; no kernel uses scratch (csrc/resource_usage.py assign_topm.hip).
//
// assign_kernel itself is left as it is: the fragment code below repeats its load / MFMA sequence as functions (as shared functions
// they would change its register allocation, the experience written down in assign_prefilter.hpp); RootSIFT is desc_load.hpp's.
#include <algorithm>

#include "assign_prefilter.hpp"

namespace pvs {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TOPM_DCHUNK = 128;       // dims resident in LDS / registers at a time (ASSIGN_DCHUNK of vlad.hip)
constexpr int TOPM_MAX_M = 8;
constexpr int TOPM_SENTINEL = 0x7fffffff;   // index of an empty list slot: loses against every centroid, padded ones included

struct TopmArgs {
  const void* X;
  int64_t total;
  int D, ld;
  const float* Cpad;    // [K_pad][D_pad], zero padded
  const float* cnorm;   // [K_pad], +inf on padded clusters
  int K_pad, D_pad;
  int m, splits;
  int32_t* out_idx;     // splits == 1: [total][m] labels; otherwise the partial lists [total][splits][m]
  float* out_val;       // the same shape; may be null when splits == 1
};

// (v, j) order of the header: v ascending, then j ascending
__device__ __forceinline__ bool topm_before(float v, int j, float lv, int lj) { return v < lv || (v == lv && j < lj); }

template <int MC>
struct TopmList {
  float v[MC];
  int j[MC];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int q = 0; q < MC; ++q) {
      v[q] = INFINITY;
      j[q] = TOPM_SENTINEL;
    }
  }
  // nv is already a number or +inf (never NaN)
  __device__ __forceinline__ void offer(float nv, int nj) {
    if (topm_before(nv, nj, v[MC - 1], j[MC - 1])) {
      v[MC - 1] = nv;
      j[MC - 1] = nj;
#pragma unroll
      for (int q = MC - 1; q > 0; --q) {
        const bool sw = topm_before(v[q], j[q], v[q - 1], j[q - 1]);
        const float tv = v[q - 1];
        const int tj = j[q - 1];
        v[q - 1] = sw ? v[q] : tv;
        j[q - 1] = sw ? j[q] : tj;
        v[q] = sw ? tv : v[q];
        j[q] = sw ? tj : j[q];
      }
    }
  }
  // the lists of lane and lane ^ MASK merged; both lanes end with the same list
  template <int MASK>
  __device__ __forceinline__ void merge_xor() {
    float ov[MC];
    int oj[MC];
#pragma unroll
    for (int q = 0; q < MC; ++q) {
      ov[q] = __shfl_xor(v[q], MASK, 64);
      oj[q] = __shfl_xor(j[q], MASK, 64);
    }
#pragma unroll
    for (int q = 0; q < MC; ++q) offer(ov[q], oj[q]);
  }
};

// ---- fragment code: the sequence of assign_kernel (vlad.hip).  Operand roles: MFMA "A" = centroids (row i = cluster within a 32-tile,
// from LDS), "B" = descriptors (col j = lane & 31, from registers); lane (., h = lane >> 5) feeds dims 8t + 4h .. 8t + 4h + 3 to the
// four k-steps of step t, so the chain of a (row, centroid) runs over dims (8t + e, 8t + 4 + e), e = 0..3, t ascending.
template <int KIND, bool VEC>
__device__ __forceinline__ void topm_row_fragment(const TopmArgs& a, int64_t row, bool rvalid, int dc, int nt, int h, float4 (&xb)[16]) {
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    xb[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < nt) {
      const int d = dc + 8 * t + 4 * h;
      if constexpr (VEC) {
        if (rvalid && d < a.D) xb[t] = load4<KIND>(a.X, row, a.ld, d);
      } else {
        if (rvalid) {
          if (d + 0 < a.D) xb[t].x = load1<KIND>(a.X, row, a.ld, d + 0);
          if (d + 1 < a.D) xb[t].y = load1<KIND>(a.X, row, a.ld, d + 1);
          if (d + 2 < a.D) xb[t].z = load1<KIND>(a.X, row, a.ld, d + 2);
          if (d + 3 < a.D) xb[t].w = load1<KIND>(a.X, row, a.ld, d + 3);
        }
      }
    }
  }
  if constexpr (DescTraits<KIND>::rootsift) {
    // the host guarantees D <= 128 (one slab) for the RootSIFT kinds
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t) s += (xb[t].x + xb[t].y) + (xb[t].z + xb[t].w);
    s += __shfl_xor(s, 32, 64);
    const RootsiftRow<KIND> rr(s);
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      xb[t].x = rr(xb[t].x);
      xb[t].y = rr(xb[t].y);
      xb[t].z = rr(xb[t].z);
      xb[t].w = rr(xb[t].w);
    }
  }
}

template <int NT>
__device__ __forceinline__ void topm_mfma_tiles(const float* lds_c, int stride, int j, int h, int nt, const float4 (&xb)[16], f32x16 (&acc)[NT]) {
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    if (t < nt) {
#pragma unroll
      for (int tile = 0; tile < NT; ++tile) {
        const float4 c4 = *reinterpret_cast<const float4*>(lds_c + (32 * tile + j) * stride + 8 * t + 4 * h);
        acc[tile] = __builtin_amdgcn_mfma_f32_32x32x2f32(c4.x, xb[t].x, acc[tile], 0, 0, 0);
        acc[tile] = __builtin_amdgcn_mfma_f32_32x32x2f32(c4.y, xb[t].y, acc[tile], 0, 0, 0);
        acc[tile] = __builtin_amdgcn_mfma_f32_32x32x2f32(c4.z, xb[t].z, acc[tile], 0, 0, 0);
        acc[tile] = __builtin_amdgcn_mfma_f32_32x32x2f32(c4.w, xb[t].w, acc[tile], 0, 0, 0);
      }
    }
  }
}

// =============================================================================================== kernel A
// grid = row blocks x splits (blockIdx.x = row block * splits + split); split s takes the centroid blocks [s nb / splits, (s + 1) nb / splits)
template <int NT, int KIND, bool VEC, int MC>
__global__ __launch_bounds__(ASSIGN_THREADS, 2) void topm_kernel(TopmArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int CB = 32 * NT;
  const int cw_max = a.D_pad < TOPM_DCHUNK ? a.D_pad : TOPM_DCHUNK;
  const int stride = cw_max + 4;  // +16 B per row: ds_read_b128 of 16 consecutive rows is conflict-free
  float* lds_c = reinterpret_cast<float*>(smem);
  float* lds_n = lds_c + CB * stride;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int ncb = a.K_pad / CB;
  const int nsc = (a.D_pad + TOPM_DCHUNK - 1) / TOPM_DCHUNK;
  const int64_t rb = (int64_t)blockIdx.x / a.splits;
  const int split = (int)((int64_t)blockIdx.x - rb * a.splits);
  const int cb_lo = (int)((int64_t)split * ncb / a.splits), cb_hi = (int)((int64_t)(split + 1) * ncb / a.splits);

  const int64_t row = rb * ASSIGN_ROWS + wave * 32 + j;
  const bool rvalid = row < a.total;

  TopmList<MC> best;
  best.clear();

  float4 xb[16];
  if (nsc == 1) topm_row_fragment<KIND, VEC>(a, row, rvalid, 0, cw_max >> 3, h, xb);   // one slab: the row stays in registers

  // The accumulators of G tiles are live at a time (a 256-centroid block is two groups of four): 128 accumulator registers beside
  // the 64 of the row and the list do not fit 256.  One slab (D <= 128): the block is staged once for both groups.  More slabs: every
  // (group, slab) stages its slab of the whole block again -- twice the LDS traffic on the rare wide-row path.
  constexpr int G = NT < 4 ? NT : 4;
  for (int cb = cb_lo; cb < cb_hi; ++cb) {
    for (int g0 = 0; g0 < NT; g0 += G) {
      f32x16 acc[G];
#pragma unroll
      for (int t = 0; t < G; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

      for (int sc = 0; sc < nsc; ++sc) {
        const int dc = sc * TOPM_DCHUNK;
        const int cw = min(TOPM_DCHUNK, a.D_pad - dc);
        if (g0 == 0 || nsc > 1) {
          __syncthreads();   // the readers of what the LDS held are done
          const int c4n = cw >> 2;
          for (int idx = threadIdx.x; idx < CB * c4n; idx += ASSIGN_THREADS) {
            const int r = idx / c4n, c4 = idx - r * c4n;
            const float4 v = *reinterpret_cast<const float4*>(a.Cpad + (int64_t)(cb * CB + r) * a.D_pad + dc + 4 * c4);
            *reinterpret_cast<float4*>(lds_c + r * stride + 4 * c4) = v;
          }
          for (int idx = threadIdx.x; idx < CB; idx += ASSIGN_THREADS) lds_n[idx] = a.cnorm[cb * CB + idx];
          __syncthreads();
        }
        if (nsc > 1) topm_row_fragment<KIND, VEC>(a, row, rvalid, dc, cw >> 3, h, xb);
        topm_mfma_tiles<G>(lds_c + 32 * g0 * stride, stride, j, h, cw >> 3, xb, acc);
      }

      // ---- the lane's 16 G values in ascending centroid order
#pragma unroll
      for (int tile = 0; tile < G; ++tile) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int r0 = 32 * (g0 + tile) + 8 * g + 4 * h;  // C/D layout: row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
          const float4 cn = *reinterpret_cast<const float4*>(lds_n + r0);
          const float cnv[4] = {cn.x, cn.y, cn.z, cn.w};
          const int kb = cb * CB + r0;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float v = fmaf(-2.f, acc[tile][4 * g + e], cnv[e]);
            v = v < INFINITY ? v : INFINITY;   // NaN and +inf count as +inf
            best.offer(v, kb + e);
          }
        }
      }
    }
  }

  // the two half-waves hold interleaved centroid subsets of the same row
  best.template merge_xor<32>();
  if (h == 0 && rvalid) {
    const int64_t o = a.splits == 1 ? row * a.m : (row * a.splits + split) * a.m;
#pragma unroll
    for (int q = 0; q < MC; ++q)
      if (q < a.m) {
        a.out_idx[o + q] = best.j[q];
        if (a.out_val != nullptr) a.out_val[o + q] = best.v[q];
      }
  }
}

// =============================================================================================== kernel B
constexpr int TOPM_MERGE_THREADS = 256;

template <int MC>
__global__ __launch_bounds__(TOPM_MERGE_THREADS) void topm_merge_kernel(const int32_t* __restrict__ part_idx, const float* __restrict__ part_val,
                                                                         int64_t total, int per_row /* splits * m */, int m,
                                                                         int32_t* __restrict__ labels, float* __restrict__ val) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (TOPM_MERGE_THREADS / 64) + (threadIdx.x >> 6);
  if (row >= total) return;   // whole waves leave
  TopmList<MC> best;
  best.clear();
  const int64_t base = row * per_row;
  for (int i = lane; i < per_row; i += 64) best.offer(part_val[base + i], part_idx[base + i]);
  best.template merge_xor<32>();
  best.template merge_xor<16>();
  best.template merge_xor<8>();
  best.template merge_xor<4>();
  best.template merge_xor<2>();
  best.template merge_xor<1>();
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < MC; ++q)
      if (q < m) {
        labels[row * m + q] = best.j[q];
        if (val != nullptr) val[row * m + q] = best.v[q];
      }
  }
}

template <int NT, int KIND, int MC>
static int launch_topm_mc(pvs_ctx* ctx, const TopmArgs& a, bool vec, size_t lds, unsigned grid) {
  auto kv = topm_kernel<NT, KIND, true, MC>;
  auto ks = topm_kernel<NT, KIND, false, MC>;
  return launch_lds(ctx, vec ? kv : ks, dim3(grid), dim3(ASSIGN_THREADS), lds, a);
}

template <int NT, int KIND>
static int launch_topm_nt(pvs_ctx* ctx, const TopmArgs& a, int mc, bool vec, size_t lds, unsigned grid) {
  switch (mc) {
    case 2: return launch_topm_mc<NT, KIND, 2>(ctx, a, vec, lds, grid);
    case 5: return launch_topm_mc<NT, KIND, 5>(ctx, a, vec, lds, grid);
    default: return launch_topm_mc<NT, KIND, 8>(ctx, a, vec, lds, grid);
  }
}

}  // namespace pvs

using namespace pvs;

PVS_EXPORT int pvs_kmeans_topm_dev(pvs_ctx* ctx, const pvs_codebook* cb, const void* d_desc, int desc_kind, int64_t total_desc, int m,
                                   int splits, int32_t* d_labels, float* d_val) {
  PVS_NEED(ctx, "ctx");
  PVS_NEED(cb, "codebook");
  if (desc_kind != PVS_DESC_F32 && desc_kind != PVS_DESC_F32_ROOTSIFT && desc_kind != PVS_DESC_U8_ROOTSIFT)
    PVS_FAIL(PVS_ERR_INVALID, "pvs_kmeans_topm_dev: unknown descriptor kind %d", desc_kind);
  if (total_desc < 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_kmeans_topm_dev: negative descriptor count");
  if (m < 1 || m > TOPM_MAX_M || m > cb->K)
    PVS_FAIL(PVS_ERR_INVALID, "pvs_kmeans_topm_dev: m must lie in 1..min(K, %d) (m = %d, K = %d)", TOPM_MAX_M, m, cb->K);
  if (total_desc >= ((int64_t)1 << 32)) PVS_FAIL(PVS_ERR_UNSUPPORTED, "pvs_kmeans_topm_dev: %lld rows in one call", (long long)total_desc);
  if (total_desc == 0) return PVS_OK;
  PVS_NEED(d_desc, "descriptors");
  PVS_NEED(d_labels, "labels");
  PVS_ALIGNED(d_labels, 4, "labels");
  if (d_val) PVS_ALIGNED(d_val, 4, "values");
  if (desc_kind != PVS_DESC_U8_ROOTSIFT) PVS_ALIGNED(d_desc, 4, "descriptors");
  if (desc_kind != PVS_DESC_F32 && cb->D > TOPM_DCHUNK)
    PVS_FAIL(PVS_ERR_UNSUPPORTED, "fused RootSIFT needs D <= %d (got %d)", TOPM_DCHUNK, cb->D);
  PVS_HIP(hipSetDevice(ctx->device));

  // a table padded to whole 256-centroid blocks is walked in such blocks; a smaller one (K <= 128) in blocks of 32
  const int nt = cb->K_pad % 256 == 0 ? 8 : 1;
  if (cb->K_pad % 32 != 0 || cb->D_pad % 8 != 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_kmeans_topm_dev: unexpected codebook padding");
  const int64_t nblocks = (total_desc + ASSIGN_ROWS - 1) / ASSIGN_ROWS;
  const int max_splits = std::max(1, cb->K_pad / 256);
  int64_t sp = splits;
  if (splits == 0) sp = (2 * (int64_t)ctx->num_cu + nblocks - 1) / nblocks;   // about two workgroups per CU over the launch; large batches get 1
  sp = std::min<int64_t>(std::max<int64_t>(sp, 1), max_splits);
  if (nblocks * sp >= ((int64_t)1 << 31)) PVS_FAIL(PVS_ERR_UNSUPPORTED, "pvs_kmeans_topm_dev: %lld workgroups in one launch", (long long)(nblocks * sp));

  const int ld = cb->D;
  const int esz = desc_kind == PVS_DESC_U8_ROOTSIFT ? 1 : 4;
  // vector path: rows and 4-element groups are 16-B (f32) / 4-B (u8) aligned
  const bool vec = (cb->D % 4 == 0) && (ld % 4 == 0) && ((reinterpret_cast<uintptr_t>(d_desc) % (4 * esz)) == 0);
  const int cw = cb->D_pad < TOPM_DCHUNK ? cb->D_pad : TOPM_DCHUNK;
  const size_t lds = (size_t)(32 * nt) * (cw + 4) * 4 + (size_t)(32 * nt) * 4;
  // list slots of the instantiation: the smallest of 2, 5, 8 that holds m (a one-slot list made the compiler turn the insertion into
  // selects and overlap the two tile groups, which spilled)
  const int mc = m <= 2 ? 2 : (m <= 5 ? 5 : 8);

  ScopedTimer tm(ctx, T_ASSIGN);
  TopmArgs a{d_desc, total_desc, cb->D, ld, cb->d_cpad, cb->d_cnorm, cb->K_pad, cb->D_pad, m, (int)sp, d_labels, d_val};
  int32_t* part_idx = nullptr;
  float* part_val = nullptr;
  if (sp > 1) {
    const TopmPartialLayout lay = topm_partial_layout((size_t)total_desc, (size_t)sp, (size_t)m);
    char* ws = nullptr;
    PVS_TRY(ws_reserve(ctx, WS_LISTS, lay.bytes, &ws));
    part_idx = lay.idx(ws);
    part_val = lay.val(ws);
    a.out_idx = part_idx;
    a.out_val = part_val;
  }
  const unsigned grid = (unsigned)(nblocks * sp);
  PVS_TRY(dispatch_desc_kind(desc_kind, [&](auto k) -> int {
    constexpr int KIND = decltype(k)::value;
    return nt == 8 ? launch_topm_nt<8, KIND>(ctx, a, mc, vec, lds, grid) : launch_topm_nt<1, KIND>(ctx, a, mc, vec, lds, grid);
  }));
  if (sp > 1) {
    const unsigned g2 = (unsigned)((total_desc + TOPM_MERGE_THREADS / 64 - 1) / (TOPM_MERGE_THREADS / 64));
    const int per_row = (int)sp * m;
#define PVS_TOPM_MERGE(MCV) \
  hipLaunchKernelGGL(topm_merge_kernel<MCV>, dim3(g2), dim3(TOPM_MERGE_THREADS), 0, ctx->stream, part_idx, part_val, total_desc, per_row, m, d_labels, d_val)
    switch (mc) {
      case 2: PVS_TOPM_MERGE(2); break;
      case 5: PVS_TOPM_MERGE(5); break;
      default: PVS_TOPM_MERGE(8); break;
    }
#undef PVS_TOPM_MERGE
    PVS_HIP(hipGetLastError());
  }
  return PVS_OK;
}
