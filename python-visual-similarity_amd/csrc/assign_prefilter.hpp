// What the two kernels of the K1 prefilter (assign16_kernel in vlad.hip: v_mfma_f32_32x32x16_f16; assign16x_kernel in assign16x.hip:
// v_mfma_f32_16x16x32_f16) must agree on, defined once: their arguments, the sqrt table of uint8 rows, the proven margin and what
// happens to a row that is settled or not.  The row statistics, the float-row scale, the -|c|^2/2 fragments and the cross-lane merge
// are still written out in each kernel: as shared functions they changed the register allocation of assign16_kernel.
//
// The exact kernel (assign_kernel) runs at the f32 MFMA rate (vector-FMA speed).  Most descriptors have a clear nearest centre,
// so a first pass evaluates  v16 = |c|^2 - 2 x.c  on the f16 MFMA with both operands split into two fp16 halves
// (x = xh + xl, c = ch + cl after a power-of-two scaling into the fp16 range; products ch.xh + ch.xl + cl.xh, fp32
// accumulate: 3 MFMAs at 16x the f32 rate) under a proven error bound, and settles every descriptor whose best v16 is
// more than 2 eps below all others -- there the exact kernel's strict-'<' argmin is the same cluster.  The remaining
// descriptors (near ties, non-finite values) are listed per workgroup and labelled by the exact kernel itself in a second
// launch, so the labels are those of the exact kernel for every input.
#pragma once

#include "common.hpp"
#include "desc_load.hpp"

namespace pvs {

typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));

constexpr int ASSIGN_THREADS = 512;                      // 8 waves, 2 per SIMD
constexpr int ASSIGN_ROWS = (ASSIGN_THREADS / 64) * 32;  // 256 descriptors per workgroup step

struct Assign16Args {
  const void* X;
  int64_t total;
  int D, ld;
  const _Float16* C16;  // [2][K_pad][D_pad16]  hi | lo
  const float* cnorm;   // [K_pad], +inf on padded clusters
  int K_pad, D_pad16;
  int c_shift;
  float cmax;
  const _Float16* cnk;  // [K_pad][4]: three exact fp16 pieces of -|c|^2/2 2^(c_shift - cn_e1) (padded clusters: -65504, 0, 0), 0
  int cn_e1, K;
  int32_t* labels;
  int64_t* amb_rows;             // [gridDim][cap]: descriptors left to the exact kernel, one list per workgroup
  unsigned long long* amb_count; // [gridDim]
  int64_t cap;
  float2* rowstat;               // uint8 rows: (row sum + 1e-7, its reciprocal) per descriptor for the aggregate pass, or null
  unsigned long long* stamps;    // diagnostic build (DIAG) only: [16] cycle totals over all workgroups, see pvs_fused_profile
  int nprod;                     // fp16 products per (row, cluster): 3 (product path), 2 or 1 (measurement variants)
  int shape16;                   // != 0: assign16x_kernel (v_mfma_f32_16x16x32_f16) where its shape qualifies (measurement variant)
};

// the 16 x 16 x 32 kernel for the shape the benchmarks use (assign16x.hip); lds and grid as for assign16_kernel<8, ...>
int launch_assign16x(pvs_ctx* ctx, const Assign16Args& p, int kind, size_t lds, int grid);

// uint8 rows through the table: sqrt(raw) for raw = 0..255 as an fp16 pair (hi | lo << 16).  RootSIFT's element is sqrt(raw) / sqrt(d)
// with ONE factor per row, so the prefilter works on T = sqrt(raw) -- a table lookup and two byte permutes per element, no arithmetic
// at all -- and the row's factor sqrt(d) moves into the -|c|^2/2 step:  x.c - |c|^2/2 = (T.c - |c|^2 sqrt(d) / 2) / sqrt(d).
__device__ __forceinline__ void pf_fill_sqrt_table(uint32_t* lds_t) {
  if (threadIdx.x < 256) {
    const float sv = sqrtf((float)threadIdx.x);
    const _Float16 hi = (_Float16)sv, lo = (_Float16)(sv - (float)hi);
    lds_t[threadIdx.x] = (uint32_t)__builtin_bit_cast(unsigned short, hi) | ((uint32_t)__builtin_bit_cast(unsigned short, lo) << 16);
  }
}
// the eight raw bytes xw[0], xw[1] of a row as one hi and one lo fragment
__device__ __forceinline__ void pf_u8_fragment(const uint32_t* lds_t, const uint32_t* xw, f16x8_t* xh, f16x8_t* xl) {
  uint32_t hw[4], lw[4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int pq = 0; pq < 2; ++pq) {
      const uint32_t w = xw[i];
      const uint32_t e0 = lds_t[(w >> (16 * pq)) & 0xffu], e1 = lds_t[(w >> (16 * pq + 8)) & 0xffu];
      hw[2 * i + pq] = __builtin_amdgcn_perm(e1, e0, 0x05040100u);   // hi(e0) | hi(e1) << 16
      lw[2 * i + pq] = __builtin_amdgcn_perm(e1, e0, 0x07060302u);   // lo(e0) | lo(e1) << 16
    }
  *xh = __builtin_bit_cast(f16x8_t, make_uint4(hw[0], hw[1], hw[2], hw[3]));
  *xl = __builtin_bit_cast(f16x8_t, make_uint4(lw[0], lw[1], lw[2], lw[3]));
}

// The proven margin.  With x, c the row and the centre as the exact kernel sees them and dot16 what the fp16 products give,
//   |dot16 - dot32| <= [ 2 2^-22 (operand split) + 2^-22 (dropped cl.xl) + 400 2^-23 (fp32 accumulation of 384 products)
//                       + 128 2^-24 (the exact kernel's own accumulation) + 1e-9 (flush below the fp16 normal range)
//                       + conv_err + drop_err ] |x||c|
//   eps = 2 |dot16 - dot32| + 2^-22 (|c|^2 + 2 |x||c|)   (the final fma of both kernels)
// conv_err = 2^-21: the approximate RootSIFT elements (y' = v_sqrt(raw / d), see the row scale in assign16_kernel).
// drop_err: NP fp16 products per (row, cluster), 3 = ch.xh + ch.xl + cl.xh (the product path), 2 = cl.xh dropped, 1 = ch.xh only; a
// dropped correction product is |cl| <= 2^-11 |c| or |xl| <= 2^-11 |x| element by element, so fewer products widen the margin and
// leave more rows to the exact kernel -- the labels stay the exact kernel's.
// Table rows (LUT): everything in units of 1 / sqrt(d) (|T| |c| instead of |x| |c|; |c|^2 sqrt(d) instead of |c|^2); the -|c|^2/2 term
// additionally carries the dropped third piece of sqrt(d) (2^-22) and six accumulation roundings (6 2^-24): 6e-7 instead of 2.4e-7.
template <int KIND, int NP, bool LUT>
__device__ __forceinline__ float prefilter_eps(float nx, float cmax, float lut_sd, float sqrt_d) {
  const float xc = nx * cmax;
  constexpr float conv_err = DescTraits<KIND>::rootsift ? 4.8e-7f : 0.f;
  const float cc = LUT ? cmax * cmax * lut_sd : cmax * cmax;
  constexpr float drop_err = (3 - NP) * 4.9e-4f;
  return 2.f * (4.8e-7f + 2.4e-7f + 4.8e-5f + 7.7e-6f + 1e-9f + conv_err + drop_err) * xc * (1.f + sqrt_d * 1e-9f) + (LUT ? 6.0e-7f : 2.4e-7f) * (cc + 2.f * xc);
}

// The end of a row's tail.  A settled row (exactly one cluster within the margin, the minimum itself; everything finite; a real, not a
// padded cluster) gets its label; the rest goes on the workgroup's list: one LDS atomic per wave (ballot + prefix count).  `leader`:
// this lane speaks for the row and the row exists.  Every lane of the wave must call this.
__device__ __forceinline__ void pf_label_or_list(const Assign16Args& a, bool settled, bool leader, int64_t row, int bidx, int lane,
                                                 unsigned int* s_count, int64_t* my_rows) {
  const bool amb = leader && !settled;
  const unsigned long long amask = __ballot(amb);
  unsigned int base = 0;
  if (amask != 0ull) {
    if (lane == 0) base = atomicAdd(s_count, (unsigned int)__popcll(amask));
    base = __shfl(base, 0, 64);
  }
  if (leader) {
    if (settled) a.labels[row] = bidx;
    else my_rows[base + __popcll(amask & ((1ull << lane) - 1ull))] = row;
  }
}

}  // namespace pvs
