/*
 * pvsim_diag.h -- DIAGNOSTIC entry points of libpvsim_hip.so.  Not part of the product ABI (include/pvsim.h): nothing in the
 * package's encode / similarity / retrieval path calls them; they exist for tests/tools/{assign,fused}_profile.py, which read
 * in-kernel cycle stamps of specially built kernel variants.  The product kernels carry no stamps.  The suite also reads the plan
 * of the last GEMM and poisons recycled device memory through them.
 */
#ifndef PVSIM_DIAG_H
#define PVSIM_DIAG_H

#include "pvsim.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic build of the fused VLAD encode (in-kernel cycle stamps of one wave per workgroup; the product kernel carries
 * none).  enable != 0: following fused launches run the stamped kernel and add into 16 counters; out16 (optional) receives and
 * resets them: [0..6] shader cycles in P0 / A / reduce / exact re-evaluation / K2 / epilogue / image switch summed over the
 * workgroups, [8] stages, [9] stages with a re-evaluation, [10] re-evaluation entries, [11] rows the margin did not settle. */
int pvs_fused_profile(pvs_ctx* ctx, int enable, int64_t* out16);

/* Which launches the last similarity GEMM of this context made (host bookkeeping, written where the launches are made; nothing
 * on the device).  Tests use it to assert that a case ran the plan it is named for (PVS_OPT_GEMM_SLOTS pins the plans).
 *   out12[0]  model (pvs_gemm_model)                out12[6]  n_tail: list entries handed to the split-K tail
 *   out12[1]  tiles_m   (generic: 64-row blocks)    out12[7]  split used by the tail = min(plan split, nparts); 1 without one
 *   out12[2]  tiles_n                               out12[8]  nparts: partial images per tail tile (0 without a tail)
 *   out12[3]  1: symmetric form (upper triangle)    out12[9]  tail ran unsplit (pvs_gemm_tail_unsplit), 0 otherwise
 *   out12[4]  1: dual form (panel + transpose)      out12[10] 1: the main launch was the 8-phase fp16 kernel
 *   out12[5]  n_main: list entries run whole        out12[11] 1: the launch added into the output (a later segment of long rows)
 * All -1 before the first GEMM. */
typedef enum {
  PVS_GEMM_MODEL_EXACT_F32 = 0,   /* 128 x 128, v_mfma_f32_32x32x2_f32, chains of 1024 k */
  PVS_GEMM_MODEL_F16_256 = 1,     /* fp16 operands, 256 x 256, single-level accumulation */
  PVS_GEMM_MODEL_F16_BOUNDED = 2, /* fp16 operands, 128 x 128, chains of 1024 k (prefilter) */
  PVS_GEMM_MODEL_F64 = 3,         /* 128 x 128 on the f64 matrix pipe */
  PVS_GEMM_MODEL_F16_2LVL = 4,    /* fp16 operands, 256 x 128 two-level kernel, whole tiles only (prefilter) */
  PVS_GEMM_MODEL_GENERIC = 5      /* 64 x 64 tiled fallback, any length and alignment (f32 and f64) */
} pvs_gemm_model;
typedef enum {
  PVS_GEMM_TAIL_UNSPLIT_BYTES = 1,     /* the partial images would exceed 1 GiB */
  PVS_GEMM_TAIL_UNSPLIT_ONE_SLICE = 2  /* a single k-tile: nothing to split (f64) */
} pvs_gemm_tail_unsplit;
int pvs_gemm_last_plan(pvs_ctx* ctx, int32_t out12[12]);

/* Device memory that a context hands out again without clearing it (tests/test_gpu_recycled_memory.py).  pvs_diag_poison queues on
 * the context's stream a memset with `byte` (0..255) of the WHOLE capacity of every allocated workspace slot (what & 1) and / or of
 * every block now waiting in the table block cache (what & 2); it allocates nothing and frees nothing.  pvs_diag_ws_bytes reports
 * the capacity of the 18 workspace slots in the order of pvs::WsSlot (csrc/workspace.hpp), 0 for a slot never reserved. */
int pvs_diag_poison(pvs_ctx* ctx, int byte, int what);
int pvs_diag_ws_bytes(pvs_ctx* ctx, size_t out18[18]);

#ifdef __cplusplus
}
#endif
#endif /* PVSIM_DIAG_H */
