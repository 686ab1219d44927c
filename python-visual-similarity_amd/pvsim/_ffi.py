"""ctypes binding of libpvsim_hip.so (C-ABI: include/pvsim.h).

The library is the product: there is no CPU fallback.  Loading fails loudly (ImportError) if the shared
object has not been built, and creating a Context fails loudly (RuntimeError) if no MI355X is visible.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

from ._errors import CapacityError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PVSIM_LIB", os.path.join(_HERE, "libpvsim_hip.so"))

# pvs_status -> Python exception (same exception classes as the reference raises)
PVS_OK, PVS_ERR_INVALID, PVS_ERR_NO_DEVICE, PVS_ERR_OOM, PVS_ERR_UNSUPPORTED, PVS_ERR_DIM, PVS_ERR_CAPACITY = range(7)
_EXC = {PVS_ERR_INVALID: ValueError, PVS_ERR_NO_DEVICE: RuntimeError, PVS_ERR_OOM: MemoryError,
        PVS_ERR_UNSUPPORTED: NotImplementedError, PVS_ERR_DIM: RuntimeError, PVS_ERR_CAPACITY: CapacityError}

DESC_F32, DESC_F32_ROOTSIFT, DESC_U8_ROOTSIFT = 0, 1, 2
OPT_ASSIGN_PREFILTER, OPT_VLAD_PATH, OPT_TOPK_SELECT_ONLY, OPT_AGG_VARIANT, OPT_FISHER_SCALE = 0, 1, 2, 3, 4      # pvs_option
OPT_TRAIN_BATCH_CHUNKS = 5        # 0: training batches from the byte budgets; 1..1024: at most that many chunks per batch
PIX_U8_RGB, PIX_U8_GRAY, PIX_F32_RGB, PIX_F32_GRAY = 0, 1, 2, 3          # pvs_pixel_kind
DSIFT_U8, DSIFT_F32, DSIFT_F32_RAW, DSIFT_F32_QUANT = 0, 1, 2, 3                         # pvs_dsift_out
OPT_UPDATE_WINDOW_ROWS = 6        # 0: windows of the in-place row compaction from the staging byte budget; 1..2^20: at most that many rows
OPT_SQ8_PATH = 7                  # pvs_sq8_topk_dev: 0 chooses by the number of queries, 1 the row scan, 2 the int8 GEMM; same bits
OPT_GEMM_SLOTS = 8                # 0: the similarity GEMMs plan for the chip's workgroup slots; 1..4096: for that many (tests pin every launch plan)
GEMM_EXACT_F32, GEMM_F16_256, GEMM_F16_BOUNDED, GEMM_F64, GEMM_F16_2LVL, GEMM_GENERIC = range(6)      # pvs_gemm_model (include/pvsim_diag.h)
GEMM_TAIL_UNSPLIT_BYTES, GEMM_TAIL_UNSPLIT_ONE_SLICE = 1, 2                                           # pvs_gemm_tail_unsplit
GEMM_PLAN_FIELDS = ("model", "tiles_m", "tiles_n", "symm", "dual", "n_main", "n_tail", "split", "nparts", "tail_unsplit",
                    "main_8ph", "accumulate")
WS_SLOTS = ("WS_STAGE_IN", "WS_SCRATCH", "WS_PANEL_OUT", "WS_PROJECTED", "WS_AUX_ROWS", "WS_FP16_ROWS", "WS_LISTS", "WS_NB_NORMS",
            "WS_NB_F64_ROWS", "WS_DSIFT_TABLE", "WS_SIFT_PYRAMID", "WS_SIFT_TABLES", "WS_SIFT_KEYPOINTS", "WS_MATCH_TABLE",
            "WS_VERIFY_POINTS", "WS_VERIFY_SMALL", "WS_IVF_CANDIDATES", "WS_UPDATE")     # pvs::WsSlot (csrc/workspace.hpp), in order
POISON_WORKSPACE, POISON_TABLE_CACHE = 1, 2                                              # pvs_diag_poison `what` bits
SQ8_PATH_AUTO, SQ8_PATH_ROWS, SQ8_PATH_MATRIX = 0, 1, 2
SQ8_MAX_L = 131072                # 127^2 * L < 2^31
RANGE_UPPER = 1                   # PVS_RANGE_UPPER: the self-join, pairs j > i only
RANGE_PATH_AUTO, RANGE_PATH_EXACT, RANGE_PATH_FILTERED = 0, 1, 2      # pvs_cosine_range_dev: same triples on every path
RANGE_MAX_CAPACITY = 1 << 40      # PVS_RANGE_MAX_CAPACITY
SQ8_RANGE_PATH_AUTO, SQ8_RANGE_PATH_PANEL, SQ8_RANGE_PATH_MASK = 0, 1, 2      # pvs_sq8_range_dev: same triples on every path
SUBSET_PATH_AUTO, SUBSET_PATH_MASK, SUBSET_PATH_LISTED = 0, 1, 2      # pvs_*_topk_subset_dev: same lists on every path
SUBSET_MAX_K = 1024               # a subset ranking is one page of the top-k kernels
SCAN_TILE = 2048                # PVS_SCAN_TILE of include/pvsim.h
COMBINE_CHUNK_BYTES, COMBINE_BATCH = 8192, 8     # PVS_COMBINE_CHUNK_BYTES, PVS_COMBINE_BATCH of include/pvsim.h
DIFFUSE_DOT_BLOCK, DIFFUSE_MAX_COLUMNS = 256, 65536   # PVS_DIFFUSE_DOT_BLOCK, PVS_DIFFUSE_MAX_COLUMNS of include/pvsim.h
KRR_MAX_K1, KRR_MAX_KQ = 64, 1024                     # PVS_KRR_MAX_K1, PVS_KRR_MAX_KQ of include/pvsim.h
VLAD_PATH_AUTO, VLAD_PATH_GATHER, VLAD_PATH_STREAM, VLAD_PATH_FUSED = 0, 1, 2, 3
TIMER_NAMES = ("assign", "aggregate", "cosine_gemm", "topk", "fisher_posterior", "fisher_moments", "misc", "rescore")


class NormParams(C.Structure):
    _fields_ = [("power_norm_weight", C.c_double), ("norm_order", C.c_double), ("epsilon", C.c_double)]


_vp, _i64, _int, _sz = C.c_void_p, C.c_int64, C.c_int, C.c_size_t
_pp = C.POINTER(C.c_void_p)
_np = C.POINTER(NormParams)

# name -> argtypes  (restype is int everywhere except where noted)
SIGNATURES = {
    "pvs_version": [],
    "pvs_last_error": [],
    "pvs_device_count": [C.POINTER(C.c_int)],
    "pvs_init": [_int, _vp, _pp],
    "pvs_destroy": [_vp],
    "pvs_sync": [_vp],
    "pvs_stream": [_vp],
    "pvs_device_name": [_vp, C.c_char_p, _sz],
    "pvs_set_option": [_vp, _int, _int],
    "pvs_get_option": [_vp, _int, C.POINTER(C.c_int)],
    "pvs_malloc": [_vp, _sz, _pp],
    "pvs_free": [_vp, _vp],
    "pvs_memcpy_h2d": [_vp, _vp, _vp, _sz],
    "pvs_memcpy_d2h": [_vp, _vp, _vp, _sz],
    "pvs_memset": [_vp, _vp, _int, _sz],
    "pvs_fill_dev": [_vp, _vp, _i64, _int, C.c_uint64],
    "pvs_stream_wait": [_vp, _vp],
    "pvs_comm_unique_id": [_vp],
    "pvs_comm_init": [_vp, _int, _int, _vp, _pp],
    "pvs_comm_destroy": [_vp],
    "pvs_comm_library": [],
    "pvs_allgather_dev": [_vp, _vp, _vp, _sz],
    "pvs_alltoall_dev": [_vp, _vp, _vp, _sz],
    "pvs_sendrecv_dev": [_vp, _int, _vp, _vp, _vp, _vp, _vp],
    "pvs_allreduce_max_f64": [_vp, _vp, _int],
    "pvs_comm_barrier": [_vp],
    "pvs_codebook_create": [_vp, _vp, _int, _int, _pp],
    "pvs_codebook_destroy": [_vp, _vp],
    "pvs_gmm_create": [_vp, _vp, _vp, _vp, _int, _int, _pp],
    "pvs_gmm_destroy": [_vp, _vp],
    "pvs_pca_create": [_vp, _vp, _vp, _int, _int, _pp],
    "pvs_pca_destroy": [_vp, _vp],
    "pvs_vlad_encode": [_vp, _vp, _vp, _vp, _int, _vp, _i64, _np, _vp, _vp],
    "pvs_vlad_encode_dev": [_vp, _vp, _vp, _vp, _int, _vp, _i64, _i64, _np, _vp, _vp, _vp],
    "pvs_kmeans_predict_dev": [_vp, _vp, _vp, _int, _i64, _vp],
    "pvs_kmeans_topm_dev": [_vp, _vp, _vp, _int, _i64, _int, _int, _vp, _vp],
    "pvs_fisher_encode": [_vp, _vp, _vp, _vp, _int, _vp, _i64, _np, _vp],
    "pvs_fisher_encode_dev": [_vp, _vp, _vp, _vp, _int, _vp, _i64, _i64, _np, _vp, _int],
    "pvs_gmm_predict_proba_dev": [_vp, _vp, _vp, _int, _i64, _vp],
    "pvs_pca_transform_dev": [_vp, _vp, _vp, _int, _i64, _vp],
    "pvs_cosine": [_vp, _vp, _i64, _vp, _i64, _i64, _int, _vp],
    "pvs_row_inv_norms_dev": [_vp, _vp, _i64, _i64, _vp],
    "pvs_cosine_dev": [_vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _i64],
    "pvs_cosine_dual_dev": [_vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _i64],
    "pvs_topk_dev": [_vp, _vp, _i64, _i64, _i64, _int, _i64, _int, _vp, _vp],
    "pvs_cosine_topk_dev": [_vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _int, _i64, _int, _vp, _vp],
    "pvs_cosine_topk_filtered_dev": [_vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _int, _vp, _vp, _vp],
    "pvs_f32_to_f16_dev": [_vp, _vp, _i64, _vp],
    "pvs_cosine_f16_dev": [_vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _i64],
    "pvs_cosine_topk_f16_dev": [_vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _int, _i64, _int, _vp, _vp],
    "pvs_cosine_topk": [_vp, _vp, _i64, _vp, _i64, _i64, _int, _vp, _vp],
    "pvs_cosine_topk_f64": [_vp, _vp, _i64, _vp, _i64, _i64, _int, _vp, _vp],
    "pvs_row_inv_norms_f64_dev": [_vp, _vp, _i64, _i64, _vp],
    "pvs_cosine_f64_dev": [_vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _i64],
    "pvs_cosine_topk_f64_dev": [_vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _int, _vp, _vp],
    "pvs_topk_merge_dev": [_vp, _vp, _vp, _int, _i64, _int, _vp, _vp],
    "pvs_materialise_dev": [_vp, _vp, _int, _int, _i64, _vp],
    "pvs_kmeans_step_dev": [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp],
    "pvs_gmm_em_step_dev": [_vp, _vp, _vp, _i64, _vp],
    "pvs_label_sums_dev": [_vp, _vp, _int, _i64, _vp, _int, _int, _vp],
    "pvs_gram_dev": [_vp, _vp, _int, _i64, _vp],
    "pvs_seed_distances_dev": [_vp, _vp, _int, _i64, _vp, _int, _vp, _vp, _vp, _int],
    "pvs_seed_pick_dev": [_vp, _vp, _int, _i64, _vp, _vp, _vp, _vp, _int, _vp, _vp],
    "pvs_min_update_dev": [_vp, _vp, _vp, _i64, _vp],
    "pvs_kmeanspp_run_dev": [_vp, _vp, _int, _i64, _int, _int, _vp, _vp],
    "pvs_l2_knn_dev": [_vp, _vp, _i64, _vp, _i64, _i64, _int, _int, _vp, _vp, _vp],
    "pvs_l2_radius_count_dev": [_vp, _vp, _i64, _vp, _i64, _i64, _int, C.c_double, _vp],
    "pvs_l2_radius_fill_dev": [_vp, _vp, _i64, _vp, _i64, _i64, _int, C.c_double, _vp, _vp, _vp],
    "pvs_csr_spmm_f64_dev": [_vp, _i64, _vp, _vp, _vp, _vp, _int, C.c_double, _vp, _vp, C.c_double, _vp],
    "pvs_transpose_f64_dev": [_vp, _vp, _i64, _i64, _vp],
    "pvs_dsift_count": [_int, _int, _int, _vp, _int, _vp],
    "pvs_dsift_frames": [_int, _int, _int, _vp, _int, _vp, _i64],
    "pvs_dsift_dev": [_vp, _vp, _int, _vp, _vp, _i64, _int, _vp, _int, C.c_double, _int, _vp, _i64, _vp],
    "pvs_sift_workspace": [_int, _int, _int, _int, C.POINTER(_sz), C.POINTER(_i64)],
    "pvs_sift_dev": [_vp, _vp, _int, _vp, _vp, _i64, _int, _int, C.c_double, C.c_double, C.c_double, _int, _int, _vp, _i64, _vp,
                     _vp, C.POINTER(_i64)],
    "pvs_match_u8_dev": [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp],
    "pvs_match_filter_dev": [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, C.c_double, _int, _vp, _vp],
    "pvs_verify_dev": [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, C.c_double, _int, _vp, _vp, _vp, _vp],
    "pvs_pq_create": [_vp, _vp, _int, _int, _int, _pp],
    "pvs_pq_destroy": [_vp, _vp],
    "pvs_pq_encode_dev": [_vp, _vp, _vp, _i64, _vp],
    "pvs_pq_lut_dev": [_vp, _vp, _vp, _i64, _vp],
    "pvs_pq_scan_topk_dev": [_vp, _vp, _i64, _int, _int, _vp, _i64, _vp, _vp, _int, _i64, _int, _vp, _vp],
    "pvs_rescore_rows_dev": [_vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp],
    "pvs_ivf_assign_dev": [_vp, _vp, _i64, _int, _vp, _int, _vp, _vp],
    "pvs_ivf_coarse_dev": [_vp, _vp, _i64, _int, _vp, _int, _vp],
    "pvs_ivf_scan_topk_dev": [_vp, _vp, _i64, _int, _int, _vp, _vp, _int, _vp, _vp, _int, _vp, _vp, _vp, _vp, _int, _vp, _vp],
    "pvs_combine_rows_dev": [_vp, _vp, _i64, _i64, _int, _vp, _vp, _vp, _vp, _i64, _int, _vp],
    "pvs_keep_mask_dev": [_vp, _vp, _i64, _i64, _vp],
    "pvs_keep_positions_dev": [_vp, _vp, _i64, _vp],
    "pvs_compact_rows_dev": [_vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp],
    "pvs_ivf_insert_dev": [_vp, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "pvs_ivf_remove_dev": [_vp, _int, _int, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "pvs_copy_dev": [_vp, _vp, _vp, _sz],
    "pvs_graph_affinity_dev": [_vp, _vp, _vp, _int, _i64, _int, _i64, _i64, _int, _vp, _vp],
    "pvs_graph_mutual_dev": [_vp, _vp, _vp, _i64, _int, _vp],
    "pvs_graph_degrees_dev": [_vp, _vp, _i64, _int, _vp, _vp],
    "pvs_graph_normalise_dev": [_vp, _vp, _vp, _vp, _i64, _int, _vp],
    "pvs_diffuse_rhs_dev": [_vp, _vp, _vp, _int, _i64, _int, _i64, _int, _vp],
    "pvs_diffuse_workspace": [_i64, _i64, C.POINTER(_sz)],
    "pvs_diffuse_cg_dev": [_vp, _vp, _vp, _i64, _int, _vp, _i64, C.c_double, C.c_double, _int, _int, _int, _vp, _sz, _vp, _vp, _vp, _vp],
    "pvs_rank_f64_dev": [_vp, _vp, _i64, _i64, _i64, _int, _vp, _vp],
    "pvs_graph_lists_dev": [_vp, _vp, _vp, _i64, _int, _i64, _vp, _i64, _vp, _vp],
    "pvs_graph_merge_dev": [_vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _i64, _i64, _vp, _vp],
    "pvs_graph_damage_dev": [_vp, _vp, _i64, _int, _vp, _vp],
    "pvs_graph_remap_dev": [_vp, _vp, _i64, _int, _vp, _vp, _vp],
    "pvs_graph_gather_rows_dev": [_vp, _vp, _i64, _i64, _vp, _i64, _vp],
    "pvs_graph_affinity_sim_dev": [_vp, _vp, _i64, _int, _int, _vp],
    "pvs_krr_sets_dev": [_vp, _vp, _i64, _int, _int, _vp, _vp],
    "pvs_krr_members_dev": [_vp, _vp, _vp, _vp, _i64, _int, _vp, _vp],
    "pvs_krr_weights_dev": [_vp, _vp, _vp, _i64, _int, _int, _vp, _vp],
    "pvs_krr_expand_dev": [_vp, _vp, _vp, _vp, _i64, _int, _int, _vp, _vp, _vp],
    "pvs_krr_query_dev": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _int, _int, _vp, _vp, _i64, _int, _vp, _vp, _vp, _vp],
    "pvs_krr_score_dev": [_vp, _vp, _vp, _vp, _vp, _i64, _int, _vp, _vp, _vp, _vp, _i64, _int, _int, C.c_double, _vp],
    "pvs_asmk_aggregate_dev": [_vp, _vp, _vp, _int, _vp, _vp, _i64, _i64, _vp, _vp, _int, _vp, _vp, _vp],
    "pvs_asmk_aggregate_ma_dev": [_vp, _vp, _vp, _int, _vp, _vp, _i64, _i64, _vp, _int, _vp, _int, _vp, _vp, _vp],
    "pvs_asmk_score_dev": [_vp, _i64, _vp, _vp, _vp, _int, _int, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _int, _vp, _i64],
    "pvs_asmk_invert_dev": [_vp, _int, _int, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _int, _vp, _vp, _vp],
    "pvs_asmk_weight_sums_dev": [_vp, _int, _vp, _vp, _i64, _vp, _vp, _vp, _vp],
    "pvs_asmk_insert_dev": [_vp, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "pvs_asmk_remove_dev": [_vp, _int, _int, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "pvs_asmk_expand_dev": [_vp, _i64, _vp, _vp, _vp, _int, _int, _vp, _vp, _vp, _i64, _int, _vp, _vp, _int, _int, _int, _vp, _int, _int,
                            _vp, _vp, _vp, _vp],
    "pvs_sq8_encode_dev": [_vp, _vp, _i64, _int, _vp, _vp],
    "pvs_sq8_topk_dev": [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _int, _int, _i64, _int, _vp, _vp],
    "pvs_sq8_range_dev": [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _int, C.c_float, _int, _int, _int, _i64, _vp, _vp, _vp, _vp, _vp],
    "pvs_cosine_range_dev": [_vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp, C.c_float, _int, _int, _int, _i64, _vp, _vp, _vp, _vp, _vp],
    "pvs_pair_components_dev": [_vp, _vp, _vp, _i64, _i64, _vp, _vp],
    "pvs_subset_create": [_vp, _vp, _i64, _i64, _pp],
    "pvs_subset_destroy": [_vp, _vp],
    "pvs_cosine_topk_subset_dev": [_vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _int, _int, _int, _vp, _vp, _vp],
    "pvs_sq8_topk_subset_dev": [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _int, _vp, _int, _int, _int, _vp, _vp, _vp],
    "pvs_ivf_sq8_scan_topk_dev": [_vp, _vp, _vp, _i64, _int, _vp, _int, _vp, _vp, _int, _vp, _vp, _vp, _int, _int, _vp, _vp],
    "pvs_ivf_sq8_scan_plan": [_vp, _i64, _int, _vp, _int, _int, _vp],
    "pvs_ivf_sq8_group_probes_dev": [_vp, _vp, _i64, _int, _vp, _int, _vp, _vp, _vp, _vp, _vp],
    "pvs_ivf_sq8_scan_lists_topk_dev": [_vp, _vp, _vp, _i64, _int, _vp, _int, _vp, _vp, _int, _vp, _vp, _vp, _int, _int, _vp, _vp],
    "pvs_ivf_sq8_scan_lists_plan": [_vp, _i64, _int, _vp, _int, _int, _vp],
    "pvs_fused_profile": [_vp, _int, _vp],
    "pvs_gemm_last_plan": [_vp, _vp],
    "pvs_diag_poison": [_vp, _int, _int],
    "pvs_diag_ws_bytes": [_vp, _vp],
    "pvs_timers_enable": [_vp, _int],
    "pvs_timers_reset": [_vp],
    "pvs_timers_read": [_vp, _int, C.POINTER(C.c_double), C.POINTER(C.c_int64)],
}

_lib = None
_lock = threading.Lock()


def mapped_hip_runtimes() -> list[str]:
    """Paths of the HIP runtime images (libamdhip64) mapped into this process."""
    found = []
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                path = line.rsplit(None, 1)[-1] if "/" in line else ""
                if "libamdhip64" in os.path.basename(path) and path not in found:
                    found.append(path)
    except OSError:
        pass
    return found


def _one_hip_runtime() -> None:
    """One HIP runtime per process, whatever the import order.

    libpvsim_hip.so needs `libamdhip64.so.7`.  A PyTorch-ROCm wheel ships its own copy under torch/lib with that same
    SONAME, and two runtimes in one process each open the device on their own (the second one then sees no GPU).  The
    dynamic linker binds a DT_NEEDED entry to an already mapped object of that SONAME, so all that is needed is that the
    FIRST runtime mapped is the one everybody else will ask for: if none is mapped yet and torch is installed, map
    torch's copy now (a later `import torch` finds the same file); without torch the system runtime under /opt/rocm is
    used.  pvs_init refuses to run when it finds two runtimes mapped."""
    if mapped_hip_runtimes():
        return
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    for loc in (spec.submodule_search_locations if spec and spec.submodule_search_locations else []):
        cand = os.path.join(loc, "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
            return


def lib():
    """The loaded shared library (loads on first use; raises ImportError if it is not built)."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise ImportError(
                        f"{LIB_PATH} not found: build the HIP library first "
                        "(python -c 'import __graft_entry__ as g; g.build()' or make -C python-visual-similarity_amd/csrc). "
                        "pvsim has no CPU fallback.")
                _one_hip_runtime()
                l = C.CDLL(LIB_PATH)
                for name, args in SIGNATURES.items():
                    fn = getattr(l, name)          # AttributeError here = header / library mismatch
                    fn.argtypes = args
                    fn.restype = C.c_int
                l.pvs_last_error.restype = C.c_char_p
                l.pvs_comm_library.restype = C.c_char_p
                l.pvs_stream.restype = C.c_void_p
                _lib = l
    return _lib


def check(status: int) -> None:
    if status != PVS_OK:
        msg = lib().pvs_last_error().decode("utf-8", "replace")
        raise _EXC.get(status, RuntimeError)(msg)


def ptr(a) -> C.c_void_p:
    """Host pointer of a C-contiguous ndarray, raw int device pointer, or None."""
    if a is None:
        return C.c_void_p(None)
    if isinstance(a, np.ndarray):
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError("array must be C-contiguous")
        return C.c_void_p(a.ctypes.data)
    return C.c_void_p(int(a))


def norm_params(power, norm_order, epsilon) -> NormParams:
    return NormParams(float(power), float(norm_order), float(epsilon))
