/*
 * pvsim.h -- C-ABI of libpvsim_hip.so: the MI355X (gfx950) hot path of an image-similarity engine
 * that is a drop-in for pyvisim's VLADEncoder / FisherVectorEncoder / cosine_similarity / eval top-k.
 *
 * The reference (MechaCritter/Python-Visual-Similarity, pure Python) has no FFI layer; its extension
 * points are Python objects.  This header is therefore the NEW boundary that sits
 * directly beneath those Python methods; each entry point names the reference code it replaces
 * (paths relative to the reference root).  The Python package `pvsim` binds it with ctypes
 * (python-visual-similarity_amd/pvsim/_ffi.py); INTEGRATION.md shows the binding a pyvisim maintainer
 * would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only; no C++/torch types.
 *   - every function returns a pvs_status (0 = ok).  pvs_last_error() returns a thread-local message.
 *     No exception or abort crosses the ABI.
 *   - the library never owns host memory: outputs are caller-allocated, C-contiguous.
 *   - device tables live behind opaque handles with explicit create/destroy.
 *   - one pvs_ctx = one device + one HIP stream.  Entry points ending in `_dev` take DEVICE pointers
 *     (e.g. torch.Tensor.data_ptr(), or pvs_malloc memory), enqueue on the context's stream and return
 *     without synchronising; all others take HOST pointers and block until the result is in host memory.
 *   - there is no CPU fallback: without a GPU every compute entry point fails with PVS_ERR_NO_DEVICE.
 */
#ifndef PVSIM_H
#define PVSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PVS_VERSION 103 /* 0.1.3 */

typedef enum {
  PVS_OK = 0,
  PVS_ERR_INVALID = 1,     /* bad argument                      -> ValueError   */
  PVS_ERR_NO_DEVICE = 2,   /* no HIP device / HIP runtime error -> RuntimeError */
  PVS_ERR_OOM = 3,         /* device allocation failed          -> MemoryError  */
  PVS_ERR_UNSUPPORTED = 4, /* shape / option not implemented    -> NotImplementedError */
  PVS_ERR_DIM = 5,         /* dimension mismatch                -> RuntimeError (as the reference raises) */
  PVS_ERR_CAPACITY = 6     /* a data-dependent output does not fit; the true size was returned -> pvsim.CapacityError */
} pvs_status;

/* How descriptor rows are stored, and whether the RootSIFT tail
 * (pyvisim/features/_features.py:112-114: d /= sum(d)+1e-7; d = sqrt(d)) is fused into the load. */
typedef enum {
  PVS_DESC_F32 = 0,          /* float32 rows used as they are                                */
  PVS_DESC_F32_ROOTSIFT = 1, /* float32 raw SIFT rows (0..255), RootSIFT applied on the fly  */
  PVS_DESC_U8_ROOTSIFT = 2   /* uint8  raw SIFT rows, RootSIFT applied on the fly (4x fewer HBM bytes) */
} pvs_desc_kind;

/* Behaviour switches of a context (pvs_set_option).  The defaults are the product path; the other values exist so that
 * tests and benchmarks can pin one of several implementations that must agree bit for bit. */
typedef enum {
  PVS_OPT_ASSIGN_PREFILTER = 0, /* 1 (default): fp16 MFMA prefilter (three products) + exact pass on near ties; 0: exact f32 MFMA kernel   */
                                /* only; 2 / 3: measurement variants with two / one fp16 product(s) and the wider margin that goes with them; */
                                /* 4: three products on v_mfma_f32_16x16x32_f16 (D = 128, 128 < K <= 256: measurement variant, same lists)   */
  PVS_OPT_VLAD_PATH = 1,        /* 0 (default) and 1: assign + gather aggregate (two reads of the descriptors); 2: assign +        */
                                /* streaming aggregate; 3: fused one-read kernel (D = 128, 128 < K <= 256; error otherwise)        */
  PVS_OPT_TOPK_SELECT_ONLY = 2, /* top-k kernel for k <= 16: 0 (default) threshold filter on panels of >= 4096 columns, k rounds         */
                                /* otherwise; 1: always the radix-select kernel; 2: always the rounds; 3: always the threshold filter  */
  PVS_OPT_AGG_VARIANT = 3,      /* gather aggregate at D <= 128: 0 (default) chosen by rows per cluster; 1: eight waves per SIMD,     */
                                /* batches of 4 rows (short images); 2: five waves, batches of 8 (long images).  Same bits.         */
  PVS_OPT_FISHER_SCALE = 4,     /* division of a Fisher row by its norm: 0 (default) and 1: a second pass over the rows; 2: inside the      */
                                /* moments kernel (one workgroup per image; 1.6 % less time, 1.7 x the bytes beyond L2 at configs[2]).     */
                                /* Same bits.                                                                                             */
  PVS_OPT_TRAIN_BATCH_CHUNKS = 5, /* rows per batch of the training passes (Lloyd step, label sums, Gram, EM step): 0 (default) from the  */
                                /* workspace byte budgets; v in 1..1024: at most v chunks per batch (chunk = 4096 rows in the Lloyd step  */
                                /* and the label sums, 8192 in the Gram pass, 2048 in the EM step), so that a test reaches the seam       */
                                /* between two batches at a few thousand rows.  Same sums: chunks are added in chunk order either way.    */
  PVS_OPT_UPDATE_WINDOW_ROWS = 6, /* source rows per window of the in-place pvs_compact_rows_dev: 0 (default) what the staging byte budget  */
                                /* holds; v in 1..2^20: at most v rows, so that a test reaches a window seam with a few hundred rows.      */
                                /* Same bytes: the windows move the rows, they compute nothing.                                          */
  PVS_OPT_SQ8_PATH = 7,         /* pvs_sq8_topk_dev: 0 (default) the row scan for up to 4 queries, the int8 GEMM beyond; 1: always the row   */
                                /* scan; 2: always the GEMM.  Same bits: the dot product of two code rows is an integer.                  */
  PVS_OPT_GEMM_SLOTS = 8,       /* workgroup slots the similarity GEMMs plan their launches for: 0 (default) what the chip has (CUs x       */
                                /* workgroups per CU); v in 1..4096: plan as if it had v, so that a test reaches every launch plan (whole   */
                                /* tiles, full rounds + split-K tail, every tile split, the 256 x 128 two-level kernel) with a few tiles.   */
                                /* It moves the cut of the tile list into launches, never the arithmetic of a score.                      */
  PVS_OPT_COUNT_ = 9
} pvs_option;

typedef struct pvs_ctx pvs_ctx;
typedef struct pvs_codebook pvs_codebook; /* KMeans.cluster_centers_ (K,D) f32 + ||c||^2                */
typedef struct pvs_gmm pvs_gmm;           /* GaussianMixture weights_/means_/covariances_ ('diag')     */
typedef struct pvs_pca pvs_pca;           /* PCA components_ (C,Din) + mean_                            */
typedef struct pvs_comm pvs_comm;         /* one rank of the multi-GPU exchange (RCCL communicator bound to a context)  */

/* Normalisation knobs shared by both encoders -- the constructor kwargs of
 * VLADEncoder (pyvisim/encoders/vlad.py:42-53) and FisherVectorEncoder (fisher_vector.py:41-51). */
typedef struct {
  double power_norm_weight; /* p in sign(v)|v|^p ; VLAD default 1, Fisher default 0.5 */
  double norm_order;        /* ord of np.linalg.norm: 1, 2, any p > 0, or +INFINITY   */
  double epsilon;           /* added to the norm before dividing (default 1e-9)       */
} pvs_norm_params;

/* ---------------------------------------------------------------- context / errors */
int pvs_version(void);
const char* pvs_last_error(void);
int pvs_device_count(int* count);
/* stream == NULL: the context creates and owns a stream.  Otherwise `stream` is a hipStream_t the
 * caller owns (e.g. torch.cuda.current_stream().cuda_stream) and all work is enqueued there. */
int pvs_init(int device_id, void* stream, pvs_ctx** out);
int pvs_destroy(pvs_ctx* ctx);
int pvs_sync(pvs_ctx* ctx);
void* pvs_stream(pvs_ctx* ctx);
int pvs_device_name(pvs_ctx* ctx, char* buf, size_t buflen);
int pvs_set_option(pvs_ctx* ctx, int option, int value);
int pvs_get_option(pvs_ctx* ctx, int option, int* value);

/* plain device memory for hosts that do not use torch */
int pvs_malloc(pvs_ctx* ctx, size_t bytes, void** dptr);
int pvs_free(pvs_ctx* ctx, void* dptr);
int pvs_memcpy_h2d(pvs_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int pvs_memcpy_d2h(pvs_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int pvs_memset(pvs_ctx* ctx, void* dst_dev, int value, size_t bytes);

/* 4- or 8-byte pattern fill of device memory on the context's stream (list buffers: -1 indices, -inf scores). */
int pvs_fill_dev(pvs_ctx* ctx, void* dst_dev, int64_t n_elems, int elem_bytes, uint64_t pattern);
/* Stream ordering between two contexts of one process (e.g. compute and exchange): work queued on `waiter` after this
 * call starts only when everything queued on `signal` before this call has finished.  No host synchronisation. */
int pvs_stream_wait(pvs_ctx* waiter, pvs_ctx* signal);

/* ---------------------------------------------------------------- tables (host pointers in) */
/* replaces reading KMeans.cluster_centers_ per image (vlad.py:96) */
int pvs_codebook_create(pvs_ctx* ctx, const float* centroids /*[K*D]*/, int K, int D, pvs_codebook** out);
int pvs_codebook_destroy(pvs_ctx* ctx, pvs_codebook* cb);
/* replaces reading weights_/means_/covariances_ per image (fisher_vector.py:95-97); fp64 in, as sklearn stores */
int pvs_gmm_create(pvs_ctx* ctx, const double* weights /*[K]*/, const double* means /*[K*D]*/,
                   const double* covariances /*[K*D]*/, int K, int D, pvs_gmm** out);
int pvs_gmm_destroy(pvs_ctx* ctx, pvs_gmm* g);
/* replaces PCA.transform (vlad.py:89-90, fisher_vector.py:91-92) */
int pvs_pca_create(pvs_ctx* ctx, const float* components /*[C*Din]*/, const float* mean /*[Din]*/,
                   int n_components, int d_in, pvs_pca** out);
int pvs_pca_destroy(pvs_ctx* ctx, pvs_pca* p);

/* ---------------------------------------------------------------- VLAD: vlad.py:81-115
 * desc: packed rows of all images [offsets[n_images]][D_in]; offsets: int64[n_images+1] (CSR style).
 * pca may be NULL.  out: float32 [n_images][K*D] (k-major, flatten=True layout).  An image with zero
 * descriptors yields a zero row (the reference aborts the batch, vlad.py:92-93 -- fenced quirk).
 * out_labels (optional): int32 [total descriptors], the KMeans.predict labels (vlad.py:95).
 * out_inv_norm (optional, _dev only): float32 [n_images], 1/||row||_2 (1 for zero rows) for the cosine step.
 * The host forms validate the offsets (offsets[0] == 0, non-decreasing).  pvs_vlad_encode_dev never synchronises, so it
 * cannot: d_offsets[0] == 0, non-decreasing, d_offsets[n_images] == total_desc are PRECONDITIONS of that entry point
 * (pvs_fisher_encode_dev copies the offsets to the host for batching and does check them). */
int pvs_vlad_encode(pvs_ctx* ctx, const pvs_codebook* cb, const pvs_pca* pca, const void* desc,
                    int desc_kind, const int64_t* offsets, int64_t n_images, const pvs_norm_params* prm,
                    float* out, int32_t* out_labels);
int pvs_vlad_encode_dev(pvs_ctx* ctx, const pvs_codebook* cb, const pvs_pca* pca, const void* d_desc,
                        int desc_kind, const int64_t* d_offsets, int64_t n_images, int64_t total_desc,
                        const pvs_norm_params* prm, float* d_out, int32_t* d_labels, float* d_inv_norm);
/* KMeans.predict alone (vlad.py:95 -> sklearn _k_means_lloyd.pyx:168-218) */
int pvs_kmeans_predict_dev(pvs_ctx* ctx, const pvs_codebook* cb, const void* d_desc, int desc_kind,
                           int64_t total_desc, int32_t* d_labels);

/* ---------------------------------------------------------------- Fisher: fisher_vector.py:83-135
 * out: [n_images][K + 2*K*D]  laid out [d_pi | d_mu (k-major) | d_sigma].  The host form returns
 * float64 (the reference's dtype); the device form writes float32 or float64 (out_f64 != 0). */
int pvs_fisher_encode(pvs_ctx* ctx, const pvs_gmm* g, const pvs_pca* pca, const void* desc, int desc_kind,
                      const int64_t* offsets, int64_t n_images, const pvs_norm_params* prm, double* out);
int pvs_fisher_encode_dev(pvs_ctx* ctx, const pvs_gmm* g, const pvs_pca* pca, const void* d_desc,
                          int desc_kind, const int64_t* d_offsets, int64_t n_images, int64_t total_desc,
                          const pvs_norm_params* prm, void* d_out, int out_f64);
/* GaussianMixture.predict_proba alone (fisher_vector.py:99), float64 [total][K] */
int pvs_gmm_predict_proba_dev(pvs_ctx* ctx, const pvs_gmm* g, const void* d_desc, int desc_kind,
                              int64_t total_desc, double* d_resp);
/* PCA.transform alone: float32 [total][C] */
int pvs_pca_transform_dev(pvs_ctx* ctx, const pvs_pca* p, const void* d_desc, int desc_kind,
                          int64_t total_desc, float* d_out);

/* ---------------------------------------------------------------- cosine: pyvisim/_utils.py:312-330
 * (-> sklearn.metrics.pairwise.cosine_similarity): rows L2-normalised (zero rows stay zero), A.B^T.
 * is_f64 != 0: operands and output are float64 (the reference's dtype rule: fp32 iff both fp32). */
int pvs_cosine(pvs_ctx* ctx, const void* A, int64_t M, const void* B, int64_t N, int64_t L, int is_f64,
               void* out /*[M*N]*/);
int pvs_row_inv_norms_dev(pvs_ctx* ctx, const float* d_x, int64_t rows, int64_t L, float* d_inv);
/* out[i*ldo + j] = (A_i . B_j) * inv_a[i] * inv_b[j]; inv_* may be NULL (treated as 1). */
int pvs_cosine_dev(pvs_ctx* ctx, const float* d_A, int64_t M, const float* d_B, int64_t N, int64_t L,
                   const float* d_inv_a, const float* d_inv_b, float* d_out, int64_t ldo);

/* Same, and additionally the transposed panel out_t[j*ldt + i] = out[i*ldo + j] (bit-identical): one GEMM then serves
 * the row queries AND the column queries of a block pair (symmetric multi-GPU scheme, pvsim/distributed.py). */
int pvs_cosine_dual_dev(pvs_ctx* ctx, const float* d_A, int64_t M, const float* d_B, int64_t N, int64_t L,
                        const float* d_inv_a, const float* d_inv_b, float* d_out, int64_t ldo, float* d_out_t, int64_t ldt);

/* ---------------------------------------------------------------- top-k: pyvisim/eval.py:37-43,75-80,131-132
 * per query row: np.argsort(-scores)[:k].  Order is (score desc, index asc); NaN scores rank last, after -inf; -0 and +0 tie.
 * Returned values: a zero score comes back as +0.0 whatever its sign was, and every NaN as the canonical quiet NaN (0x7fc00000,
 * float64: 0x7ff8000000000000) whatever its sign and payload were; slots that cannot be filled are idx = -1, val = -inf.
 * pvs_topk_dev consumes a score panel [nq][ncols] (row stride ld) whose column 0 has global index
 * col_offset; with merge != 0 the panel is merged into the running lists already in d_idx/d_val.
 * d_idx: int64 [nq*k], d_val: float32 [nq*k]. */
int pvs_topk_dev(pvs_ctx* ctx, const float* d_scores, int64_t nq, int64_t ncols, int64_t ld, int k,
                 int64_t col_offset, int merge, int64_t* d_idx, float* d_val);
/* cosine + top-k without materialising the full nq x N matrix (tiled through a workspace panel). */
int pvs_cosine_topk_dev(pvs_ctx* ctx, const float* d_Q, int64_t nq, const float* d_DB, int64_t N, int64_t L,
                        const float* d_inv_q, const float* d_inv_db, int k, int64_t col_offset, int merge,
                        int64_t* d_idx, float* d_val);
/* fp16 operands (BASELINE configs[4]: the 1M x 1M similarity on fp16 encodings): fp32 rows are converted once
 * (round-to-nearest-even; keep the intra-normalised VLAD values and pass the fp32 1/||row|| factors, do not
 * pre-divide -- that would push elements into fp16 subnormals), then v_mfma_f32_32x32x16_f16 with fp32 accumulate. */
int pvs_f32_to_f16_dev(pvs_ctx* ctx, const float* d_src, int64_t n, void* d_dst_f16);
int pvs_cosine_f16_dev(pvs_ctx* ctx, const void* d_A16, int64_t M, const void* d_B16, int64_t N, int64_t L,
                       const float* d_inv_a, const float* d_inv_b, float* d_out, int64_t ldo);
int pvs_cosine_topk_f16_dev(pvs_ctx* ctx, const void* d_Q16, int64_t nq, const void* d_DB16, int64_t N, int64_t L,
                            const float* d_inv_q, const float* d_inv_db, int k, int64_t col_offset, int merge,
                            int64_t* d_idx, float* d_val);
int pvs_cosine_topk(pvs_ctx* ctx, const float* Q, int64_t nq, const float* DB, int64_t N, int64_t L, int k,
                    int64_t* out_idx, float* out_val);
/* float64 operands (Fisher encodings): the reference scores and ranks in float64 unless BOTH operands are float32
 * (pyvisim/_utils.py:312-330 -> sklearn cosine_similarity; eval.py:37-43,75-80,131-132 argsort that array).  The GEMM runs
 * on the f64 matrix pipe (v_mfma_f64_16x16x4_f64, fixed k order, upper triangle + mirror when Q == DB); rows must be 16-B
 * aligned with an even L for that path (anything else takes a vector-ALU tile kernel).  out_val float64 [nq][k], same order
 * as the fp32 entry points (score descending, index ascending, NaN last); any 1 <= k <= N (deep rankings page through the
 * complete score rows, as top_k_map(k=None) needs).
 * pvs_cosine_topk_f64: host pointers, the database is uploaded once per call.  The _dev forms take device pointers and the
 * 1/||row|| factors (pvs_row_inv_norms_f64_dev; NULL = 1), keep everything resident and do not synchronise. */
int pvs_cosine_topk_f64(pvs_ctx* ctx, const double* Q, int64_t nq, const double* DB, int64_t N, int64_t L, int k,
                        int64_t* out_idx, double* out_val);
int pvs_row_inv_norms_f64_dev(pvs_ctx* ctx, const double* d_x, int64_t rows, int64_t L, double* d_inv);
int pvs_cosine_f64_dev(pvs_ctx* ctx, const double* d_A, int64_t M, const double* d_B, int64_t N, int64_t L,
                       const double* d_inv_a, const double* d_inv_b, double* d_out, int64_t ldo);
int pvs_cosine_topk_f64_dev(pvs_ctx* ctx, const double* d_Q, int64_t nq, const double* d_DB, int64_t N, int64_t L,
                            const double* d_inv_q, const double* d_inv_db, int k, int64_t* d_idx, double* d_val);
/* The same lists as pvs_cosine_topk_dev(col_offset 0, merge 0) -- bit-identical indices AND scores -- computed faster:
 * all pairs are scored with fp16 operands under a proven error bound, the columns within twice that bound of each query's
 * approximate k-th best are re-scored with the exact fp32 recurrence of the f32 GEMM kernel, and those are ranked.
 * Inputs that do not qualify (k > 128, rows not 16-B aligned or L % 8 != 0, non-finite values, or scores so crowded that more
 * than a tenth of the queries overflow their candidate slots) silently take the plain exact path.  h_stats (optional, int64[4]): [0] 1 if the filter ran, [1] queries redone by the exact path
 * (more candidates than slots), [2] candidates re-scored, [3] candidate slots per query. */
int pvs_cosine_topk_filtered_dev(pvs_ctx* ctx, const float* d_Q, int64_t nq, const float* d_DB, int64_t N, int64_t L,
                                 const float* d_inv_q, const float* d_inv_db, int k, int64_t* d_idx, float* d_val,
                                 int64_t* h_stats);
/* merges per-rank top-k lists (multi-GPU: each rank scored its own DB shard): lists [n_lists][nq][k]. */
int pvs_topk_merge_dev(pvs_ctx* ctx, const int64_t* d_idx_lists, const float* d_val_lists, int n_lists,
                       int64_t nq, int k, int64_t* d_idx, float* d_val);

/* ---------------------------------------------------------------- multi-GPU exchange (one process per GPU, RCCL over xGMI)
 * The path shards by image (images are independent: pyvisim/encoders/vlad.py:87-113; global index = block offset + local
 * index, the insertion order of pyvisim/eval.py:28); the pairwise step needs ONE exchange of the encoding blocks, plus one
 * all-to-all of k-candidate lists in the symmetric block-pair scheme (pvsim/distributed.py).  librccl is resolved at
 * pvs_comm_init (an image already mapped in the process is preferred); collectives are enqueued on the context's stream.
 * Bootstrap: rank 0 calls pvs_comm_unique_id and hands the 128 bytes to the other ranks by any host channel. */
#define PVS_UNIQUE_ID_BYTES 128
int pvs_comm_unique_id(void* out_id /*[128]*/);
int pvs_comm_init(pvs_ctx* ctx, int nranks, int rank, const void* unique_id /*[128]*/, pvs_comm** out);
int pvs_comm_destroy(pvs_comm* comm);
const char* pvs_comm_library(void);   /* which librccl image was bound ("" before the first pvs_comm_init) */
/* recv[r * bytes_per_rank ...] = rank r's send block, for every r */
int pvs_allgather_dev(pvs_comm* comm, const void* d_send, void* d_recv, size_t bytes_per_rank);
/* recv[p * bytes_per_rank ...] = the block rank p addressed to this rank (its send[this rank]) */
int pvs_alltoall_dev(pvs_comm* comm, const void* d_send, void* d_recv, size_t bytes_per_rank);
/* batched point-to-point: op i sends send_bytes[i] bytes to and receives recv_bytes[i] bytes from peers[i] (either may be 0) */
int pvs_sendrecv_dev(pvs_comm* comm, int n_ops, const int* peers, const void* const* d_send, const size_t* send_bytes,
                     void* const* d_recv, const size_t* recv_bytes);
/* element-wise maximum over the ranks of up to 64 host doubles (timing: slowest rank); synchronises the stream */
int pvs_allreduce_max_f64(pvs_comm* comm, double* h_inout, int count);
int pvs_comm_barrier(pvs_comm* comm);

/* ---------------------------------------------------------------- vocabulary training
 * Replaces the sklearn fits inside ImageEncoderBase.learn (pyvisim/encoders/_base_encoder.py:311-342: PCA.fit ->
 * KMeans.fit for VLAD / GaussianMixture(covariance_type="diag").fit for Fisher).  Each entry is ONE pass over the
 * stacked descriptors on the device; the K x D sized parameter update and the loop control stay with the caller
 * (pvsim/learn.py).  d_x are plain fp32 rows (n, D), ld = D: make them with pvs_materialise_dev. */
/* any descriptor kind -> plain fp32 rows (RootSIFT applied for the *_ROOTSIFT kinds). */
int pvs_materialise_dev(pvs_ctx* ctx, const void* d_desc, int desc_kind, int D, int64_t total_desc, float* d_out);
/* One Lloyd pass (sklearn/cluster/_kmeans.py:_kmeans_single_lloyd body): labels as KMeans.predict with the centres of
 * `cb`; h_stats[K*D + K + 2] = [sum over members of (x - c_k) (K*D) | member counts (K) | inertia | number of labels that
 * differ from d_prev_labels (0 if NULL)].  d_sqdist (optional, f32[n]) receives |x_i - c_label|^2. */
int pvs_kmeans_step_dev(pvs_ctx* ctx, const pvs_codebook* cb, const float* d_x, int64_t total_desc, int32_t* d_labels,
                        const int32_t* d_prev_labels, double* h_stats, float* d_sqdist);
/* One EM pass (sklearn/mixture/_base.py:_e_step + _gaussian_mixture.py:_estimate_gaussian_parameters, fp64):
 * h_stats[K + 2*K*D + 1] = [sum_i gamma_ik (K) | per k: sum_i gamma_ik x_i (D), sum_i gamma_ik x_i**2 (D) | sum_i log p(x_i)].
 * K <= 256. */
int pvs_gmm_em_step_dev(pvs_ctx* ctx, const pvs_gmm* gmm, const float* d_x, int64_t total_desc, double* h_stats);
/* h_out[K*D]: per label k the sum of x_i (square = 0) or of x_i**2 squared in fp32 (square = 1) over the descriptors with
 * d_labels[i] == k -- the hard-assignment moments GaussianMixture starts from (sklearn/mixture/_base.py, init_params="kmeans"). */
int pvs_label_sums_dev(pvs_ctx* ctx, const float* d_x, int D, int64_t total_desc, const int32_t* d_labels, int K, int square,
                       double* h_out);
/* h_out[D + D*D] = [sum_i x_i | sum_i x_i x_i^T] in fp64 (sklearn/decomposition/_pca.py covariance_eigh solver input). */
int pvs_gram_dev(pvs_ctx* ctx, const float* d_x, int D, int64_t total_desc, double* h_out);
/* k-means++ seeding (sklearn/cluster/_kmeans.py:_kmeans_plusplus): for n_cand <= 8 candidate centres (host, f32[n_cand][D])
 * d_dist[j][i] = |x_i - cand_j|^2 and h_pot[j] = sum_i min(d_mind[i], d_dist[j][i]) (d_mind NULL = +inf).  cand_on_device != 0:
 * `cand` is a device pointer (e.g. pvs_seed_pick_dev's d_cand). */
int pvs_seed_distances_dev(pvs_ctx* ctx, const float* d_x, int D, int64_t total_desc, const float* cand, int n_cand,
                           const float* d_mind, float* d_dist, double* h_pot, int cand_on_device);
/* The candidate draw of a seeding step on the device: candidate c is the first position of block h_blocks[c] (4096 entries of
 * d_mind) where the running fp64 sum, started at h_base[c], reaches h_target[c] -- searchsorted(cumsum(d_mind), r) with the
 * block chosen by the caller from pvs_min_update_dev's block sums.  Writes the rows to d_cand[c] and the indices to h_idx. */
int pvs_seed_pick_dev(pvs_ctx* ctx, const float* d_x, int D, int64_t total_desc, const float* d_mind, const int64_t* h_blocks,
                      const double* h_base, const double* h_target, int n_cand, float* d_cand, int64_t* h_idx);
/* d_mind = min(d_mind, d_dist) (d_dist NULL = keep) and h_block_sums[ceil(n/4096)] = fp64 sums of d_mind per 4096 entries. */
int pvs_min_update_dev(pvs_ctx* ctx, float* d_mind, const float* d_dist, int64_t total_desc, double* h_block_sums);

/* The whole greedy k-means++ run (sklearn/cluster/_kmeans.py:_kmeans_plusplus) from a given first centre, without a host round
 * trip per step: for c = 1 .. n_clusters-1 the targets u * pot, the candidate draws (pvs_seed_pick_dev's arithmetic, the block of a
 * draw found on the device), the candidates' distances and potentials, the best candidate and the running-minimum update are
 * enqueued back to back; one synchronisation at the end.  trials <= 8 (2 + log K for K < 404).  h_uniform: (n_clusters-1) x trials
 * numbers in [0, 1) from the caller's random stream, in draw order.  h_indices[n_clusters]: [0] = the first centre (in), the
 * others out.  The same indices as the stepwise entry points give with the same numbers. */
int pvs_kmeanspp_run_dev(pvs_ctx* ctx, const float* d_x, int D, int64_t total_desc, int n_clusters, int trials,
                         const double* h_uniform, int64_t* h_indices);

/* ---------------------------------------------------------------- image clustering: pyvisim/_utils.py:128-162
 * (cluster_and_return_labels -> sklearn SpectralClustering / DBSCAN).  Their cost is an exact Euclidean neighbour search over the
 * encodings, brute force as sklearn does it: float32 rows are upcast to float64 (sklearn/metrics/_pairwise_distances_reduction),
 * and the value ranked or thresholded is  d = max(0, (|x|^2 + (-2 x.y)) + |y|^2)  in float64.  is_f64 != 0: rows are double,
 * otherwise float.  Rows are C-contiguous [n][L].  Q == X with nq == N is the self graph; the GEMM computes only the
 * upper triangle when one panel covers the whole problem (nq <= 8192 and N <= 32768 for float32 rows).
 *
 * pvs_l2_knn_dev: per query the k rows with the smallest d, order (d ascending, index ascending); d_idx int64 [nq][k],
 * d_sqdist float64 [nq][k] = d.  float32 rows: f32 MFMA prefilter with a proven margin + float64 re-score (neighbors.hip);
 * float64 rows, k > 256 or candidate lists that overflow: a full float64 pass.  Synchronises the stream (it reads the largest row
 * norm).  h_stats (optional, int64[4]): [0] 1 if the prefilter ran, [1] queries that overflowed their candidate slots (the call
 * then redid everything in float64), [2] candidates re-scored, [3] candidate slots per query. */
int pvs_l2_knn_dev(pvs_ctx* ctx, const void* d_Q, int64_t nq, const void* d_X, int64_t N, int64_t L, int is_f64, int k,
                   int64_t* d_idx, double* d_sqdist, int64_t* h_stats);
/* Radius neighbours (DBSCAN): all rows with d <= r_sq, decided in float64.  Pass 1 writes the counts (int64 [nq]); the caller
 * forms indptr (int64 [nq + 1], exclusive prefix sum) and pass 2 writes d_indices (int64) and optionally d_sqdist (float64) in
 * index order per query (CSR). */
int pvs_l2_radius_count_dev(pvs_ctx* ctx, const void* d_Q, int64_t nq, const void* d_X, int64_t N, int64_t L, int is_f64,
                            double r_sq, int64_t* d_counts);
int pvs_l2_radius_fill_dev(pvs_ctx* ctx, const void* d_Q, int64_t nq, const void* d_X, int64_t N, int64_t L, int is_f64,
                           double r_sq, const int64_t* d_indptr, int64_t* d_indices, double* d_sqdist);
/* Y = alpha S X + X diag(beta) + gamma Z, float64, for the block eigensolver of the spectral embedding.  S: n x n CSR (indptr int64
 * [n + 1], indices int64, data float64); X, Z, Y: [n][m] row-major; d_beta [m] may be NULL (0), d_Z may be NULL (0).  Y must not
 * alias X or Z. */
int pvs_csr_spmm_f64_dev(pvs_ctx* ctx, int64_t n, const int64_t* d_indptr, const int64_t* d_indices, const double* d_data,
                         const double* d_X, int m, double alpha, const double* d_beta, const double* d_Z, double gamma, double* d_Y);
/* dst[c][r] = src[r][c], float64 (block Gram matrices through pvs_cosine_f64_dev with unit inverse norms). */
int pvs_transpose_f64_dev(pvs_ctx* ctx, const double* d_src, int64_t rows, int64_t cols, double* d_dst);

/* ---------------------------------------------------------------- dense SIFT: pixels -> local descriptors
 * SIFT descriptors on a regular grid at fixed bin sizes, no detector and no orientation assignment (the dense descriptor of the
 * Fisher-vector / VLAD literature; the reference extracts keypoint SIFT with OpenCV on the CPU, pyvisim/features/_features.py:54-115).
 * Per bin size s (pixels): gray = 0.299 R + 0.587 G + 0.114 B; separable Gaussian, sigma = s/6, radius ceil(4 sigma), replicated
 * borders; central-difference gradient (one-sided at the borders); magnitude split linearly between the two nearest of 8
 * orientation planes; 4 x 4 spatial bins with centres s apart and the triangular window w(d) = 1 - |d|/s; then
 * L2-normalise, clamp at 0.2, renormalise.  Descriptor origins x0 = s - 1 + a*step <= W - 4s (likewise y0); rows are ordered by
 * (size, y0, x0), elements by (j*4 + i)*8 + o; the frame of a row is (x0 + 1.5 s, y0 + 1.5 s, s).
 * pvs_dsift_count / pvs_dsift_frames are host arithmetic (no device needed): rows of one H x W image and their frames float32 [n][3]. */
typedef enum {
  PVS_PIX_U8_RGB = 0,  /* uint8 [H][W][3]   */
  PVS_PIX_U8_GRAY = 1, /* uint8 [H][W]      */
  PVS_PIX_F32_RGB = 2, /* float32 [H][W][3], 0..255 */
  PVS_PIX_F32_GRAY = 3 /* float32 [H][W],    0..255 */
} pvs_pixel_kind;
typedef enum {
  PVS_DSIFT_U8 = 0,     /* uint8 rows min(255, floor(512 v + 0.5)): OpenCV's scale, feeds PVS_DESC_U8_ROOTSIFT */
  PVS_DSIFT_F32 = 1,    /* float32 rows v (normalised, clamped, renormalised) */
  PVS_DSIFT_F32_RAW = 2, /* float32 accumulators before normalisation */
  PVS_DSIFT_F32_QUANT = 3 /* the integers of PVS_DSIFT_U8 stored as float32 (plain SIFT rows for PVS_DESC_F32) */
} pvs_dsift_out;
int pvs_dsift_count(int H, int W, int step, const int32_t* sizes, int n_sizes, int64_t* count);
int pvs_dsift_frames(int H, int W, int step, const int32_t* sizes, int n_sizes, float* frames /*[capacity][3]*/, int64_t capacity);
/* A batch of images of mixed sizes in one device buffer.  h_hw: HOST int32 [n_images][2] = (H, W); h_pix_offsets: HOST int64
 * [n_images], the first element of each image in d_pixels counted in elements of the pixel type (NULL: images packed back to back).
 * d_out: [out_rows][128] of the output kind (16-byte aligned); d_row_offsets: DEVICE int64 [n_images + 1], written by the call
 * (CSR over the rows, the `d_offsets` of the encode entry points).  A row whose norm is <= contrast_threshold is all zeros.  An
 * image too small for a size contributes no rows for it.  Bin sizes whose tile does not fit the LDS (s > 18) -> PVS_ERR_UNSUPPORTED.
 * n_images == 0 is a no-op: nothing is written, d_row_offsets included.  step may be any positive int (beyond the image: one origin
 * per axis).  Enqueues on the context's stream and does not wait for it. */
int pvs_dsift_dev(pvs_ctx* ctx, const void* d_pixels, int pixel_kind, const int32_t* h_hw, const int64_t* h_pix_offsets,
                  int64_t n_images, int step, const int32_t* sizes, int n_sizes, double contrast_threshold, int out_kind,
                  void* d_out, int64_t out_rows, int64_t* d_row_offsets);

/* ---------------------------------------------------------------- keypoint SIFT: pixels -> detected, oriented descriptors
 * Lowe's scale-space SIFT (IJCV 2004) with OpenCV's parameter names and defaults -- not a bit-for-bit clone of cv2.SIFT.  Gray and
 * pixel kinds as for dense SIFT; first octave = the 2x bilinearly enlarged image when `upsample`; octaves while min(H_o, W_o) >= 16;
 * n_octave_layers + 3 Gaussian images per octave by incremental blur (radius ceil(4 sigma), replicated borders); strict 3 x 3 x 3
 * extrema of the DoG above 0.5 * contrast_threshold / n_octave_layers * 255, five pixels off the border; up to five steps of the 3-D
 * quadratic; |interpolated value| >= 255 * contrast_threshold / n_octave_layers; edge test with edge_threshold; 36-bin orientation
 * histogram, one row per peak >= 0.8 max; 4 x 4 x 8 descriptor in the rotated frame, then the tail of dense SIFT.  Rows are ordered
 * by (image, octave, layer, y, x of the integer extremum, orientation peak ascending); frames are float32
 * (x, y, size = diameter, angle in degrees from +x towards +y, |response|, octave) in input-image coordinates.  nfeatures > 0 keeps
 * the nfeatures strongest rows of each image by |response| (ties by row order), in the same order.
 * pvs_sift_workspace is host arithmetic: bytes of one image's Gaussian pyramid and a (very loose) upper bound of its rows.
 * pvs_sift_dev: arguments as pvs_dsift_dev; the row count is data dependent, so the call writes at most capacity_rows rows (and
 * frames, when d_frames is not NULL) but always the true CSR d_row_offsets (DEVICE int64 [n_images + 1]) and *h_total_rows (HOST).
 * If the total exceeds the capacity it returns PVS_ERR_CAPACITY with both valid: the rows below the capacity are written, nothing
 * beyond it; call again with a larger buffer.  Unlike the other _dev entry points this one WAITS for the stream (it returns the
 * total).  Batches are processed in chunks whose pyramids stay under 256 MiB; a row's bits and place do not depend on the batch.
 * n_images == 0 is a no-op: nothing is written, *h_total_rows included. */
int pvs_sift_workspace(int H, int W, int n_octave_layers, int upsample, size_t* bytes, int64_t* max_rows);
int pvs_sift_dev(pvs_ctx* ctx, const void* d_pixels, int pixel_kind, const int32_t* h_hw, const int64_t* h_pix_offsets,
                 int64_t n_images, int nfeatures, int n_octave_layers, double contrast_threshold, double edge_threshold, double sigma,
                 int upsample, int out_kind, void* d_rows, int64_t capacity_rows, float* d_frames /*[capacity_rows][6] or NULL*/,
                 int64_t* d_row_offsets, int64_t* h_total_rows);

/* ---------------------------------------------------------------- spatial re-ranking: local matching + geometric verification
 * The second stage of instance retrieval (Lowe 2004 section 7; Philbin et al. 2007): match the local descriptors of a query against
 * each image of a shortlist, fit a transform to the matches, count the inliers.  The operands are what pvs_sift_dev / pvs_dsift_dev
 * leave on the device: uint8 rows [rows][128] (PVS_DSIFT_U8, 16-byte aligned), float32 frames [rows][6] and the HOST int64 CSR
 * offsets [n_images + 1] over the images of a set.  h_pairs: HOST int32 [n_pairs][2] = (image of set A, image of set B); repeats are
 * allowed and the two sets may be one buffer.  The per-row results and the matches of pair p start at entry sum_{q<p} nA(q); one
 * call covers every pair with a fixed number of launches.  n_pairs == 0 is a no-op.  All three enqueue on the context's stream and
 * do not wait for it; what is written for a pair does not depend on the other pairs of the call.
 *
 * pvs_match_u8_dev: for row i of the A image  d_d1 = min_j |a_i - b_j|^2 over the rows of the B image (exact int32, at most
 * 128 * 255^2), d_idx = that j (local to the image; ties: the lowest j), d_d2 = the smallest distance over j != d_idx (it may equal
 * d_d1).  A B image with one row: d_d2 = INT32_MAX; with none: d_idx = -1, d_d1 = d_d2 = INT32_MAX.  An A image without rows writes
 * nothing.  Dot products of the bytes re-centred by 128 on v_mfma_i32_32x32x32_i8; no rounding anywhere. */
int pvs_match_u8_dev(pvs_ctx* ctx, const void* d_rows_a, const int64_t* h_off_a, int64_t n_images_a, const void* d_rows_b,
                     const int64_t* h_off_b, int64_t n_images_b, const int32_t* h_pairs, int64_t n_pairs, int32_t* d_idx, int32_t* d_d1,
                     int32_t* d_d2);
/* Lowe's ratio test, the mutual check and the compaction.  Row i of pair p is kept iff d_idx >= 0, (double)d1 < ratio_sq * (double)d2
 * (one float64 product and comparison; ratio_sq >= 0 comes from the caller) and, with mutual != 0, d_idx_rev[row d_idx of the B image]
 * == i, where d_idx_rev is the d_idx of pvs_match_u8_dev called with A and B exchanged and the pair list transposed (entries at
 * sum_{q<p} nB(q); NULL without mutual).  d_matches: int32 [sum nA][2] = (i, j) in ascending i from the pair's first entry;
 * d_match_counts: int32 [n_pairs].  The order comes from a prefix sum, not from atomics. */
int pvs_match_filter_dev(pvs_ctx* ctx, const int64_t* h_off_a, int64_t n_images_a, const int64_t* h_off_b, int64_t n_images_b,
                         const int32_t* h_pairs, int64_t n_pairs, const int32_t* d_idx, const int32_t* d_d1, const int32_t* d_d2,
                         const int32_t* d_idx_rev, double ratio_sq, int mutual, int32_t* d_matches, int32_t* d_match_counts);
/* Exhaustive verification in float64.  A match g joins frame (x, y, size, angle) of A to one of B.  Match h is a hypothesis:
 * sigma = size_b / size_a, phi = (angle_b - angle_a) pi / 180, A_h = sigma [[cos phi, -sin phi], [sin phi, cos phi]] anchored at its
 * own points, r^2(h, g) = |A_h (p_a(g) - p_a(h)) - (p_b(g) - p_b(h))|^2; g is an inlier iff r^2 <= tol^2 (tol in pixels of the B image).
 * Non-finite frames or size_a <= 0 give a hypothesis that counts 0.  The best hypothesis h* has the largest count (ties: the lowest
 * h).  Then up to refine_rounds rounds on the inlier set S (|S| >= 3): centre both point sets on their means over S, C = sum a~ a~^T,
 * stop if det C <= 1e-12 (tr C)^2, M = (sum b~ a~^T) C^-1, recount with r = M (p_a - mean_a) - (p_b - mean_b); the new model and set
 * are adopted unless the count fell; stop when it fell or the set did not change.  Per pair: d_inliers int32, d_models float64 [6] =
 * (M00, M01, t_x, M10, M11, t_y) with p_b ~ M p_a + t, d_best = h*, d_mask uint8 per match (at the pair's first entry; the entries
 * beyond the pair's match count are not written).  No matches or no valid hypothesis: count 0, a zero model, h* = -1. */
int pvs_verify_dev(pvs_ctx* ctx, const float* d_frames_a, const int64_t* h_off_a, int64_t n_images_a, const float* d_frames_b,
                   const int64_t* h_off_b, int64_t n_images_b, const int32_t* h_pairs, int64_t n_pairs, const int32_t* d_matches,
                   const int32_t* d_match_counts, double tol, int refine_rounds, int32_t* d_inliers, double* d_models, int32_t* d_best,
                   uint8_t* d_mask);

/* ---------------------------------------------------------------- compact index: product quantisation + ADC search
 * Jegou, Douze, Schmid, Perez (CVPR 2010; PAMI 2012): an encoding (optionally projected to d dimensions first) is cut into m
 * sub-vectors of dsub dimensions (d = m dsub), each replaced by the index of its nearest of ksub <= 256 codewords; a query is
 * scored against the codes through a per-query table (asymmetric distance computation), and a short list may be re-scored exactly.
 * ALL arithmetic below is float32 with separate roundings -- a multiply, then an add, never an fma -- in the stated order, so that
 * a restatement with float32 element operations gives the same bits.
 *   quantiser  codebooks float32 [m][ksub][dsub].
 *   encode     the code of row x in sub-space s is the j that minimises acc_j; acc_j starts at +0 and, for t = 0 .. dsub-1 ascending,
 *              acc_j = acc_j + (x[s dsub + t] - c[s][j][t])^2.  Ties go to the lowest j.  Codes are uint8 [n][m].
 *   table      lut[q][s][j] starts at +0 and adds q[s dsub + t] * c[s][j][t] for t ascending: an inner-product table, because the
 *              engine's score is a cosine.
 *   score      sum starts at +0 and adds lut[q][s][code[i][s]] for s = 0 .. m-1 ascending; score = (sum * inv_q[q]) * inv_db[i]
 *              (the convention of pvs_cosine_dev).  inv_db[i] is 1/||row i|| of the unquantised row, stored when the index is built
 *              (4 bytes per image).  A NULL inv_* pointer means 1.
 *   ranking    (score descending, global index ascending), NaN last: the rule of pvs_topk_dev.
 * n == 0 and nq == 0 are no-ops.  The _dev entry points enqueue on the context's stream and do not wait for it. */
typedef struct pvs_pq pvs_pq;             /* product quantiser: codebooks [m][ksub][dsub] f32 on the device */
int pvs_pq_create(pvs_ctx* ctx, const float* codebooks /*[m][ksub][dsub]*/, int m, int ksub, int dsub, pvs_pq** out);
int pvs_pq_destroy(pvs_ctx* ctx, pvs_pq* pq);
/* d_x float32 [n][m dsub] -> d_codes uint8 [n][m] */
int pvs_pq_encode_dev(pvs_ctx* ctx, const pvs_pq* pq, const float* d_x, int64_t n, uint8_t* d_codes);
/* d_q float32 [nq][m dsub] -> d_lut float32 [nq][m][ksub] */
int pvs_pq_lut_dev(pvs_ctx* ctx, const pvs_pq* pq, const float* d_q, int64_t nq, float* d_lut);
/* Scores of nq tables against N code rows and their ranking, with the semantics of pvs_cosine_topk_dev: row 0 has global index
 * col_offset; merge != 0 merges into the running lists already in d_idx / d_val; 1 <= k <= N (k > 1024 needs merge == 0 and
 * N <= 2^28, as there).  The nq x N score matrix never exists: scores pass through a bounded workspace panel into the top-k
 * kernels.  d_idx int64 [nq][k], d_val float32 [nq][k].  Every code must be < ksub (a precondition: it is not checked). */
int pvs_pq_scan_topk_dev(pvs_ctx* ctx, const float* d_lut, int64_t nq, int m, int ksub, const uint8_t* d_codes, int64_t N,
                         const float* d_inv_q, const float* d_inv_db, int k, int64_t col_offset, int merge, int64_t* d_idx,
                         float* d_val);
/* The exact cosine of each query with its R candidate rows, gathered by index: d_val[q][r] = ((sum_t Q[q][t] * X[c][t], t ascending,
 * separate roundings) * inv_q[q]) * inv_db[c] with c = d_cand[q][r]; c < 0 (an unfilled list slot) or c >= N gives -inf. */
int pvs_rescore_rows_dev(pvs_ctx* ctx, const float* d_Q, int64_t nq, const float* d_X, int64_t N, int64_t d, const float* d_inv_q,
                         const float* d_inv_db, const int64_t* d_cand /*[nq][R]*/, int64_t R, float* d_val /*[nq][R]*/);

/* ---------------------------------------------------------------- inverted lists for the compact index
 * IVFADC (Jegou, Douze, Schmid, PAMI 2011) for an inner-product score: a coarse quantiser cuts the database into nlist inverted
 * lists, a row is product-quantised as its residual to its list's centroid, and a query scans only its nprobe best lists.
 * q . x ~ q . c_l + q . r: the table of a query is the one of section 12 against the residual codebooks and does not depend on
 * the list; the list adds one scalar.  Arithmetic as above: float32, separate roundings, the stated order.
 *   coarse quantiser  centroids C float32 [nlist][d], 1 <= nlist <= 65536.
 *   assignment  the list of row x is the l that minimises acc_l; acc_l starts at +0 and, for t ascending,
 *               acc_l = acc_l + (x[t] - C[l][t])^2.  Ties go to the lowest l (the encode rule with m = 1, without its ksub limit).
 *   residual    r[t] = x[t] - C[l][t], one subtraction.  Codes are the section 12 codes of r.
 *   storage     rows sorted by (list, original index): list_off int64 [nlist + 1], ids int32 [N] (N < 2^31), codes uint8 [N][m] and
 *               inv_db float32 [N] in stored order (1/||x|| of the unquantised row).  Empty lists are legal.
 *   coarse term coarse[q][l] starts at +0 and adds q[t] * C[l][t] for t ascending.
 *   probes      the first nprobe entries of the ranking of coarse[q][.] by (value descending, l ascending): pvs_topk_dev on that
 *               panel.  1 <= nprobe <= min(nlist, 1024).
 *   score       of stored row i of probed list l: sum starts at coarse[q][l] and adds lut[q][s][code[i][s]] for s ascending;
 *               score = (sum * inv_q[q]) * inv_db[i].  A NULL inv_* pointer means 1.
 *   ranking     over the union of the probed lists, by (score descending, ORIGINAL index ascending), NaN last; when the probed
 *               lists hold fewer than k rows the remaining slots are idx = -1, val = -inf.  1 <= k <= 1024.
 * n == 0 and nq == 0 are no-ops.  The entry points enqueue on the context's stream and do not wait for it. */
/* d_x float32 [n][d] -> d_list int32 [n] and, unless NULL, d_residual float32 [n][d] (may not overlap d_x).  d <= 16384. */
int pvs_ivf_assign_dev(pvs_ctx* ctx, const float* d_x, int64_t n, int d, const float* d_centroids /*[nlist][d]*/, int nlist,
                       int32_t* d_list, float* d_residual);
/* d_q float32 [nq][d] -> d_coarse float32 [nq][nlist] */
int pvs_ivf_coarse_dev(pvs_ctx* ctx, const float* d_q, int64_t nq, int d, const float* d_centroids /*[nlist][d]*/, int nlist,
                       float* d_coarse);
/* d_probe int64 [nq][nprobe] and d_probe_val float32 [nq][nprobe] are the lists pvs_topk_dev gave for the coarse panel (a probe
 * outside [0, nlist) counts as an empty list).  h_list_off is a HOST copy of d_list_off: all sizing is done from it, so nothing
 * inside the call waits for the device; the two must agree.  Scores pass through a bounded workspace of candidate rows into the
 * top-k kernels.  d_idx int64 [nq][k], d_val float32 [nq][k].  Every code must be < ksub and the ids of the probed rows distinct
 * (preconditions: not checked). */
int pvs_ivf_scan_topk_dev(pvs_ctx* ctx, const float* d_lut, int64_t nq, int m, int ksub, const int64_t* d_probe,
                          const float* d_probe_val, int nprobe, const int64_t* d_list_off, const int64_t* h_list_off, int nlist,
                          const uint8_t* d_codes, const int32_t* d_ids, const float* d_inv_q, const float* d_inv_db, int k,
                          int64_t* d_idx, float* d_val);

/* ---------------------------------------------------------------- query expansion, database-side augmentation
 * Chum et al. (ICCV 2007), Arandjelovic & Zisserman (CVPR 2012), Radenovic et al. (PAMI 2018): the query, or every database row, is
 * replaced by a weighted sum of itself and the rows its first ranking found.  The device's part is that sum over whole rows, gathered
 * by index.  T is float32 (is_f64 == 0) or float64; ALL arithmetic is in T with separate roundings -- a multiply, then an add, never
 * an fma -- in the stated order, so that a restatement with element operations in T gives the same bits.
 *   X       T [N][L], the rows to gather from.
 *   self    T [n][L] or NULL; w_self T [n], NULL = 1 (read only together with self).
 *   idx     int64 [n][r]; w T [n][r].
 *   out     T [n][L].  For each row i and column t: acc = +0; with self, acc = acc + w_self[i] * self[i][t]; then for j = 0 .. r-1
 *           ascending, with c = idx[i][j]: if 0 <= c < N, acc = acc + w[i][j] * X[c][t], otherwise the slot is skipped (unfilled list
 *           slots may be passed as -1); out[i][t] = acc.
 * n == 0 is a no-op; r == 0 gives the self term alone (+0 without one).  d_out may be d_self itself (each element is read and then
 * written by the same lane); any other overlap of the two, and any overlap of [d_out, d_out + n L) with [d_X, d_X + N L), is
 * PVS_ERR_INVALID, found on the host before anything is launched, as are L < 1, N < 0, n < 0, r < 0 and a missing pointer that is
 * needed (d_out; d_idx and d_w when r > 0; d_X when r > 0 and N > 0).  Matrices need the alignment of their elements only; rows whose
 * byte length is a multiple of 16 in 16-byte aligned matrices move as 16-byte loads.  Needs no workspace; enqueues on the context's
 * stream and does not wait for it; timed on slot 6. */
#define PVS_COMBINE_CHUNK_BYTES 8192   /* bytes of an output row that one workgroup owns (2048 float32 / 1024 float64 columns) */
#define PVS_COMBINE_BATCH 8            /* list slots whose row loads are in flight together */
int pvs_combine_rows_dev(pvs_ctx* ctx, const void* d_X, int64_t N, int64_t L, int is_f64,
                         const void* d_self /*[n][L] or NULL*/, const void* d_w_self /*[n], NULL = 1*/,
                         const int64_t* d_idx /*[n][r]*/, const void* d_w /*[n][r]*/, int64_t n, int r,
                         void* d_out /*[n][L]*/);

/* ---------------------------------------------------------------- index maintenance: add and remove rows without a rebuild
 * An index is an ordered sequence of (path, row); the ORIGINAL INDEX of a row is its position in that sequence.
 *   add      new rows are appended in the order given and get the original indices N, N + 1, ...
 *   remove   the named rows leave, the others keep their relative order: the original index of a surviving row falls by the number
 *            of removed rows that stood before it.
 *   invariant  after any sequence of adds and removes every array of the index equals, byte for byte, the one an index built from
 *            scratch from the surviving rows in surviving order with the same tables (projection, codebooks, coarse centroids)
 *            holds.  Updates retrain nothing.
 * The entry points below are data movement and integer counting: no floating-point arithmetic, no atomics, every output element
 * written once.  They enqueue on the context's stream and do not wait for it; n == 0 is a no-op except where stated.
 *
 *   keep mask      uint8 [n]; entry i != 0 means row i stays.
 *   keep positions pos int64 [n + 1]: pos[i] = the number of j < i with keep[j] != 0, pos[n] = the number of kept rows.  A scan over
 *                  tiles of PVS_SCAN_TILE flags in three levels and four launches for any n <= 2^31.
 *   compaction     out[pos[i]] = rows[i] for every kept i, rows of row_bytes >= 1 bytes each.  Bytes of out past row pos[n] - 1 are
 *                  not defined.  Rows move 16 bytes at a time where row_bytes and both base addresses are multiples of 16, and 8, 4, 2
 *                  or 1 byte at a time otherwise: every row length and alignment is served. */
#define PVS_SCAN_TILE 2048             /* flags of one scan tile; PVS_SCAN_TILE tiles make one block of the second level */
/* d_keep[i] = 1 for i < n, then 0 at every d_removed[j], j < r (int64; an index outside [0, n) is skipped, repeats are harmless). */
int pvs_keep_mask_dev(pvs_ctx* ctx, const int64_t* d_removed, int64_t r, int64_t n, uint8_t* d_keep);
/* d_pos int64 [n + 1]; n == 0 writes pos[0] = 0.  0 <= n <= 2^31.  Uses the workspace for the partial sums. */
int pvs_keep_positions_dev(pvs_ctx* ctx, const uint8_t* d_keep, int64_t n, int64_t* d_pos);
/* d_pos as pvs_keep_positions_dev gives it for d_keep.  d_out disjoint from d_rows: one pass over the rows.  d_out == d_rows: in
 * place.  The rows before `first` are not touched; `first` must not exceed the index of the first removed row (0 is always valid; it
 * only saves traffic, and is ignored out of place).  The rest moves window by window: the kept rows of source rows [a, b) are
 * gathered into a staging block of the workspace (at most 64 MiB, or one row; PVS_OPT_UPDATE_WINDOW_ROWS caps the window), then
 * written to rows [pos[a], pos[b]).  pos[b] <= b, so a window never writes at or beyond the next window's first source row, and
 * the launches are ordered by the stream: extra device memory does not depend on n.  Any other overlap of d_out with d_rows, and
 * any overlap of d_out with d_keep or d_pos, is PVS_ERR_INVALID, found on the host before anything is launched. */
int pvs_compact_rows_dev(pvs_ctx* ctx, const void* d_rows, int64_t n, int64_t row_bytes, const uint8_t* d_keep, const int64_t* d_pos,
                         int64_t first, void* d_out);
/* Inverted-list insert (storage of section 14).  The n stored rows (d_codes uint8 [n][m], d_inv_db float32 [n], d_ids int32 [n],
 * list_off int64 [nlist + 1], in (list, original index) order) and b new rows in ARRIVAL order (d_new_codes [b][m], d_new_inv [b];
 * new row p gets the id n + p) are merged into the d_out_* arrays of n + b rows, again in (list, original index) order: the rows of
 * list l are its old rows followed by its new rows in arrival order, because every new id exceeds every old one.  The caller
 * supplies, from the b list numbers: new_off int64 [nlist + 1], the cumulative count of new rows per list (new_off[0] = 0,
 * new_off[nlist] = b), and d_perm int32 [b], the new rows sorted by (list, arrival).  h_list_off and h_new_off are HOST copies of
 * d_list_off and d_new_off: all sizing comes from them and nothing inside the call waits for the device; they must agree.
 * d_out_list_off[l] = list_off[l] + new_off[l].  n + b < 2^31.  Every output must be disjoint from every input (PVS_ERR_INVALID).
 * n + b == 0 writes the offsets only. */
int pvs_ivf_insert_dev(pvs_ctx* ctx, int m, int nlist, const uint8_t* d_codes, const float* d_inv_db, const int32_t* d_ids,
                       const int64_t* d_list_off, const int64_t* h_list_off, const uint8_t* d_new_codes, const float* d_new_inv,
                       const int64_t* d_new_off, const int64_t* h_new_off, const int32_t* d_perm, uint8_t* d_out_codes,
                       float* d_out_inv, int32_t* d_out_ids, int64_t* d_out_list_off);
/* Inverted-list remove.  d_keep uint8 [n] and d_pos int64 [n + 1] are indexed by ORIGINAL index.  Stored row i survives iff
 * keep[ids[i]] != 0, its new id is pos[ids[i]], and the survivors keep their stored order: codes, norms and ids are compacted into
 * the d_out_* arrays (disjoint from the inputs), and d_out_list_off[l] = the number of surviving stored rows before list_off[l].
 * n < 2^31; n == 0 writes zero offsets. */
int pvs_ivf_remove_dev(pvs_ctx* ctx, int m, int nlist, int64_t n, const uint8_t* d_codes, const float* d_inv_db, const int32_t* d_ids,
                       const int64_t* d_list_off, const uint8_t* d_keep, const int64_t* d_pos, uint8_t* d_out_codes, float* d_out_inv,
                       int32_t* d_out_ids, int64_t* d_out_list_off);
/* bytes from d_src to d_dst on the context's stream (growing a buffer); overlapping ranges are PVS_ERR_INVALID. */
int pvs_copy_dev(pvs_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);

/* ---------------------------------------------------------------- diffusion re-ranking on the kNN graph
 * Zhou et al. (NIPS 2003), Iscen et al. (CVPR 2017): the query's first results are spread over the neighbour graph of the whole
 * database by solving (I - alpha S) f = y, and the database is ranked by f.  ALL arithmetic below is float64; every multiply, add,
 * subtract and divide is rounded on its own (never an fma), in the stated order, so that a restatement with element operations gives
 * the same bits.  A float32 similarity is upcast exactly.  N < 2^31 everywhere.
 *
 * GRAPH, from the rankings of every row against the index to depth kg + 1, 1 <= kg <= N - 1, integer 0 <= gamma <= 8:
 *   drop self  from the list of row i the first slot that holds i leaves, or the last slot where there is none: nbr int32 [N][kg]
 *              (an index outside [0, N) is stored as -1 and never counts) and sim [N][kg].
 *   affinity   a[i][t] = max(sim[i][t], 0) multiplied by itself gamma - 1 times, left to right (gamma = 0: 1; a NaN counts as 0).
 *   mutual     w[i][t] = min(a[i][t], a[j][u]) with j = nbr[i][t] and u the FIRST slot of row j that holds i; +0 without such a
 *              slot.  The min is taken at both ends, so W is symmetric to the bit.
 *   degrees    deg[i] = +0, then + w[i][t] for t ascending.  r[i] = 1 / sqrt(deg[i]), correctly rounded both, and 0 where deg[i] = 0.
 *   entries    s[i][t] = w[i][t] * (r[i] * r[j]): the product of the two r first, so S is symmetric to the bit.
 * The graph is nbr plus s in fixed-width rows; there is no CSR and no transpose.
 *
 * RIGHT-HAND SIDE, from the rankings idx / val [C][kq] of C queries, 1 <= kq <= N: Y float64 [N][C] (columns innermost) is zero
 * except Y[idx[c][j]][c] = the affinity of val[c][j] (the same product); slots outside [0, N) are skipped.
 *
 * SOLVE (I - alpha S) x = y per column by conjugate gradients, 0 < alpha < 1:
 *   x = 0; r = y; p = y; rr = dot(r, r); yy = rr; thr = (tol * tol) * yy
 *   up to maxiter times:
 *     column c takes the step iff rr[c] > thr[c] (false for a NaN) and it has not been retired
 *     Ap[i] = p[i] - alpha * (sum_t s[i][t] * p[nbr[i][t]])    the sum from +0, t ascending; a slot with nbr outside [0, N) reads +0
 *     pAp = dot(p, Ap); pAp <= 0 (or a NaN) retires the column for good, before anything of it is written
 *     a = rr / pAp; x = x + a * p; r = r - a * Ap; rn = dot(r, r); b = rn / rr; p = r + b * p; rr = rn
 *   a column that does not step is not written at all.
 *   dot(u, v) of a column: the N products u[i] * v[i], padded with +0 to a multiple of PVS_DIFFUSE_DOT_BLOCK rows; inside each block
 *   of that many consecutive rows the fixed tree  v[0:h] += v[h:2h]  for h = 128, 64, .., 1; the block results added from +0 in
 *   ascending block order.
 * So a column's result depends on that column alone: neither the number of columns of a call, nor the kernel's column width, nor how
 * often the host looks at the flags changes a bit.
 *
 * Every entry point checks its arguments on the host before anything is launched (PVS_ERR_INVALID: sizes out of the ranges above,
 * a missing pointer, arrays that overlap, a work buffer that is too small), enqueues on the context's stream, and is timed on slot 6. */
#define PVS_DIFFUSE_DOT_BLOCK 256
#define PVS_DIFFUSE_MAX_COLUMNS 65536  /* columns of one pvs_diffuse_cg_dev call */
/* Lists of rows row0 .. row0 + b - 1: d_idx int64 [b][kg + 1], d_val float32 or float64 [b][kg + 1] (val_f64) -> rows row0 .. of
 * d_nbr int32 [N][kg] and d_a float64 [N][kg] (drop self + affinity). */
int pvs_graph_affinity_dev(pvs_ctx* ctx, const int64_t* d_idx, const void* d_val, int val_f64, int64_t b, int kg, int64_t row0,
                           int64_t N, int gamma, int32_t* d_nbr, double* d_a);
/* d_w float64 [N][kg] (the mutual pass: one lane per entry scans the partner's kg slots) */
int pvs_graph_mutual_dev(pvs_ctx* ctx, const int32_t* d_nbr, const double* d_a, int64_t N, int kg, double* d_w);
/* d_deg, d_r float64 [N] */
int pvs_graph_degrees_dev(pvs_ctx* ctx, const double* d_w, int64_t N, int kg, double* d_deg, double* d_r);
/* d_s float64 [N][kg] */
int pvs_graph_normalise_dev(pvs_ctx* ctx, const int32_t* d_nbr, const double* d_w, const double* d_r, int64_t N, int kg, double* d_s);
/* d_idx int64 [C][kq], d_val float32 or float64 [C][kq] -> d_Y float64 [N][C], zeroed here first.  C == 0 is a no-op. */
int pvs_diffuse_rhs_dev(pvs_ctx* ctx, const int64_t* d_idx, const void* d_val, int val_f64, int64_t C, int kq, int64_t N, int gamma,
                        double* d_Y);
/* Host arithmetic: bytes of the work buffer of one pvs_diffuse_cg_dev call over C columns (three vectors of N C, the block partials,
 * a few numbers per column). */
int pvs_diffuse_workspace(int64_t N, int64_t C, size_t* bytes);
/* d_Y, d_X float64 [N][C]; d_steps int32 [C], d_rr, d_yy float64 [C]: steps taken, the last rr and yy of every column.  d_work: at
 * least pvs_diffuse_workspace(N, C) bytes, 256-byte aligned, the caller's; no workspace slot of the context is used.  width: the
 * kernel's column width, 0 (chosen from C), 1, 4, 16 or 64 -- every width gives the same bits.  The host reads one int (columns that
 * still step) before the first step and then every check_every >= 1 steps, and stops launching when it is 0; it waits for the
 * stream only there.  maxiter == 0 gives x = 0 and rr = yy. */
int pvs_diffuse_cg_dev(pvs_ctx* ctx, const int32_t* d_nbr, const double* d_s, int64_t N, int kg, const double* d_Y, int64_t C,
                       double alpha, double tol, int maxiter, int check_every, int width, void* d_work, size_t work_bytes,
                       double* d_X, int32_t* d_steps, double* d_rr, double* d_yy);
/* The float64 ranking kernels behind every float64 top-k: d_scores [nq][ld], the first ncols columns of a row ranked by (score
 * descending, column ascending, NaN last; -0 ranks and returns as +0) to depth 1 <= k <= ncols -> d_idx int64 [nq][k], d_val
 * float64 [nq][k].  Timed on slot 3. */
int pvs_rank_f64_dev(pvs_ctx* ctx, const double* d_scores, int64_t nq, int64_t ncols, int64_t ld, int k, int64_t* d_idx, double* d_val);

/* ---------------------------------------------------------------- graph maintenance after add / remove
 * A MUTABLE graph keeps, beside nbr and s, the forward similarities sim float32 [N][kg]: the values the ranking returned, in list
 * order.  The LIST of row i is the first kg rows j != i of row i's ranking, in the order of the top-k block above: score descending,
 * index ascending, NaN after every number, -0 and +0 tie.  drop self on a ranking to depth kg + 1 gives exactly that list.  After an
 * add or a remove every list is brought to the one a ranking of the updated index gives, by the entry points below; a, w, deg, r and s
 * are then derived again from sim by the rules of the GRAPH block.  float32 similarities only: see DESIGN.md for why a float64 score is
 * not a function of its two rows alone.
 *   lists     drop self with the similarity kept: row p of the rankings belongs to row own = row0 + p, or ids[p] where an id array is
 *             given.  The first slot holding own leaves, or the last slot where there is none; the other kg slots go, in order, to
 *             row own of nbr (an index outside [0, N) is stored as -1) and of sim (the value as it stands).  A row whose own lies
 *             outside [0, N) is not written.
 *   merge     per row, the stored list (kg entries, in list order) and c candidates (idx int64 [rows][c] relative to col_offset, val
 *             float32, in list order; a candidate with idx < 0 is skipped, the others get the id idx + col_offset) are merged: entry x
 *             comes before entry y iff x is a number and y a NaN, or both are numbers and x > y, or they tie (both NaN, or equal as
 *             numbers) and the id of x is smaller; where neither comes before the other the stored entry goes first.  The first kg
 *             entries of the merged sequence are written, ids as int32, values moved as they stand.  1 <= c.
 *   damage    flag[i] = 1 iff keep[i] != 0 and some slot of row i names a row j in [0, N) with keep[j] == 0; 0 otherwise.
 *   remap     out[i][t] = pos[nbr[i][t]] where keep[i] != 0, nbr[i][t] lies in [0, N) and keep[nbr[i][t]] != 0; -1 in the other slots
 *             of a kept row; the rows with keep[i] == 0 are not written.  pos is monotone, so a list that named no removed row stays
 *             in list order.  d_out may be d_nbr itself.
 *   gather    out[p] = rows[ids[p]], rows of row_bytes bytes (a multiple of 4) moved as they stand; a row whose id lies outside [0, n)
 *             is written as zeros.  It puts the damaged rows side by side, so that they can be ranked as one block of queries.
 *   affinity  a[i][t] = the affinity of the GRAPH block of float64(sim[i][t]): the same product, the same bits as
 *             pvs_graph_affinity_dev gives for the same value.
 * Integer work, comparisons and data movement (and the affinity's products); one lane per row or per entry, every output element
 * written once, no atomics.  Arguments are checked on the host before anything is launched, as in the block above; zero rows are a
 * no-op.  Enqueued on the context's stream, timed on slot 6. */
/* d_idx int64 [b][kg + 1], d_val float32 [b][kg + 1]; d_ids int64 [b] or NULL (then own = row0 + p, and row0 + b <= N is required;
 * with d_ids, row0 is ignored) -> rows `own` of d_nbr int32 [N][kg] and d_sim float32 [N][kg]. */
int pvs_graph_lists_dev(pvs_ctx* ctx, const int64_t* d_idx, const float* d_val, int64_t b, int kg, int64_t row0, const int64_t* d_ids,
                        int64_t N, int32_t* d_nbr, float* d_sim);
/* d_nbr int32 / d_sim float32 [rows][kg] (the stored rows), d_cidx int64 / d_cval float32 [rows][c] -> d_out_nbr int32 / d_out_sim
 * float32 [rows][kg], disjoint from every input.  An id outside [0, N) is stored as -1.  2 <= N < 2^31, 1 <= kg <= N - 1. */
int pvs_graph_merge_dev(pvs_ctx* ctx, const int32_t* d_nbr, const float* d_sim, const int64_t* d_cidx, const float* d_cval, int64_t rows,
                        int kg, int c, int64_t col_offset, int64_t N, int32_t* d_out_nbr, float* d_out_sim);
/* d_nbr int32 [N][kg], d_keep uint8 [N] -> d_flag uint8 [N] */
int pvs_graph_damage_dev(pvs_ctx* ctx, const int32_t* d_nbr, int64_t N, int kg, const uint8_t* d_keep, uint8_t* d_flag);
/* d_keep uint8 [N], d_pos int64 [N + 1] (pvs_keep_mask_dev / pvs_keep_positions_dev) -> d_out int32 [N][kg], old numbering of rows */
int pvs_graph_remap_dev(pvs_ctx* ctx, const int32_t* d_nbr, int64_t N, int kg, const uint8_t* d_keep, const int64_t* d_pos, int32_t* d_out);
/* d_rows [n][row_bytes], d_ids int64 [b] -> d_out [b][row_bytes], disjoint from both.  n >= 1; b == 0 is a no-op. */
int pvs_graph_gather_rows_dev(pvs_ctx* ctx, const void* d_rows, int64_t n, int64_t row_bytes, const int64_t* d_ids, int64_t b, void* d_out);
/* d_sim float32 [N][kg] -> d_a float64 [N][kg]; integer 0 <= gamma <= 8 */
int pvs_graph_affinity_sim_dev(pvs_ctx* ctx, const float* d_sim, int64_t N, int kg, int gamma, double* d_a);

/* ---------------------------------------------------------------- k-reciprocal re-ranking on the kNN lists
 * Zhong, Zheng, Cao, Li (CVPR 2017): a database image near the query whose own neighbourhood does not share the query's is demoted
 * by the Jaccard distance of k-reciprocal neighbourhoods.  The LISTS are those of the block above: nbr int32 [N][kg] (a slot outside
 * [0, N) holds -1 and takes part in nothing) and sim float32 [N][kg].  ALL weights are float64; every multiply, add and divide is
 * rounded on its own, in the stated order.  1 <= k1 <= min(kg, 64), k1h = (k1 + 1) / 2, 1 <= k2 <= kg + 1, integer 0 <= gamma <= 8.
 * The two DEPARTURES from the paper (truncation, weights) are what makes the result a function of the lists alone, to the bit.
 *
 *   back slot  u(i, t), with j = nbr[i][t]: the FIRST slot of row j that holds i, or none.
 *   sets       R_k(i) = { t < k : u(i, t) exists and u(i, t) < k }.  mask1[i] holds R_k1(i), maskh[i] holds R_k1h(i), bit t for slot t.
 *              B(i) = {i} + { nbr[i][t] : t in R_k1(i) };  H(j) = {j} + { nbr[j][t] : t in R_k1h(j) }.
 *   expansion  E(i) = B(i) + every H(j) with j in B(i) \ {i} and 3 |H(j) & B(i)| > 2 |H(j)|: the paper's rule, tested against the
 *              unexpanded B, so the order of j is immaterial.  Sets of ids: an id that sits in two slots counts once.
 *   members    DEPARTURE 1: a member m of E(i) keeps a weight only if m = i or m sits in a slot of row i.  members[i][t] = 1 iff
 *              nbr[i][t] is a member other than i and t is the first slot of row i that holds it, 0 otherwise; dropped[i] = the
 *              number of members that are neither i nor in row i.  Every sparse vector lives on {i} + nbr[i][.]: kg + 1 wide.
 *   weights    DEPARTURE 2: the weight of a member is the affinity of the GRAPH block of float64(sim[i][t]), of i itself exactly 1.
 *              sum = +0, then + 1, then + the members' affinities for t ascending; v0[i] = 1 / sum, v[i][t] = affinity / sum, +0
 *              in the slots that are not members.
 *   V_j[m]     v0[j] when m = j; v[j][s] with s the first slot of row j that holds m; +0 otherwise.
 *   expand     for m = i (w0[i]) and for m = nbr[i][t] (w[i][t]; +0 where the slot holds -1): acc = +0, then + V_j[m] for j = i,
 *              nbr[i][0], .., nbr[i][k2 - 2] in that order, -1 slots skipped; the result is acc / float64(k2).  The sources are the
 *              unexpanded V of all rows.  ws[i] = +0, then + w0[i], then + w[i][t] for t ascending.  k2 = 1 gives w = v to the bit.
 *
 * QUERY, from its ranking qidx int64 / qval float32 [kq] against the index, 1 <= kq <= min(N, PVS_KRR_MAX_KQ); an id outside [0, N)
 * is an empty slot.  The query is not a database row and has no self entry.
 *   B(q)       slot t < min(k1, kq) with g = qidx[t] is reciprocal iff slot k1 - 1 of row g does not hold -1 and
 *              qval[t] >= sim[g][k1 - 1], compared as float32 (false for a NaN): the query would enter g's first k1.
 *   E(q)       the expansion rule with the database's H; the members outside the query's own list are dropped and counted; a member
 *              keeps its weight at the first slot of the list that holds it.
 *   weights    sum = +0, then + the affinity of qval[t] over the member slots, t ascending; vq[t] = affinity / sum in the member
 *              slots, +0 elsewhere, and +0 everywhere where the sum is not > 0.
 *   expand     wq[t], m = qidx[t]: acc = +0, then + vq[first slot holding m], then + V_g[m] for g = qidx[0 .. k2 - 2] (those < kq,
 *              empty slots skipped); wq[t] = acc / float64(k2), +0 in an empty slot.  sq = +0, then + wq[t] for t ascending.
 * SCORE of candidate r < kr <= kq, c = qidx[r]:
 *   m_sum      +0, then + min(wq[pos(c)], w0[c]), then for the slots s of row c ascending + min(wq[pos(m)], w[c][s]) with
 *              m = nbr[c][s] -- only where m is an id other than c that row c holds at no earlier slot and that the query's list
 *              holds; pos(m) is the first slot of the query's list that holds m.  min(a, b) is b where b < a, else a.
 *   J          m_sum / ((sq + ws[c]) - m_sum), +0 where that denominator is not > 0 and for an empty slot c.
 *   score      (1 - lambda) * J + lambda * float64(qval[r]), 0 <= lambda <= 1: 1 - lambda is formed in float64 on the host, the
 *              two products are formed first and then added.
 * The candidates are then ranked by pvs_rank_f64_dev on [nq][kr]: score descending, position in the first ranking ascending, NaN
 * last.  lambda = 1 gives back the first ranking.
 *
 * One wave per row or per query for the sets; one workgroup per query and one wave per candidate for the score.  No atomics, every
 * output element written once.  Arguments are checked on the host before anything is launched (PVS_ERR_INVALID: sizes out of the
 * ranges above, a missing or misaligned pointer, arrays that overlap); zero queries are a no-op.  The masks handed to members and
 * query must be those pvs_krr_sets_dev gave for the same nbr; whatever they hold, no read leaves the arrays.  Enqueued on the
 * context's stream, timed on slot 6. */
#define PVS_KRR_MAX_K1 64
#define PVS_KRR_MAX_KQ 1024  /* depth of a query's first ranking: its list and vectors live in LDS */
/* d_nbr int32 [N][kg] -> d_mask1, d_maskh uint64 [N] */
int pvs_krr_sets_dev(pvs_ctx* ctx, const int32_t* d_nbr, int64_t N, int kg, int k1, uint64_t* d_mask1, uint64_t* d_maskh);
/* -> d_members uint8 [N][kg], d_dropped int32 [N] */
int pvs_krr_members_dev(pvs_ctx* ctx, const int32_t* d_nbr, const uint64_t* d_mask1, const uint64_t* d_maskh, int64_t N, int kg,
                        uint8_t* d_members, int32_t* d_dropped);
/* d_sim float32 [N][kg], d_members uint8 [N][kg] -> d_v float64 [N][kg], d_v0 float64 [N] */
int pvs_krr_weights_dev(pvs_ctx* ctx, const float* d_sim, const uint8_t* d_members, int64_t N, int kg, int gamma, double* d_v, double* d_v0);
/* -> d_w float64 [N][kg], d_w0, d_ws float64 [N] */
int pvs_krr_expand_dev(pvs_ctx* ctx, const int32_t* d_nbr, const double* d_v, const double* d_v0, int64_t N, int kg, int k2, double* d_w,
                       double* d_w0, double* d_ws);
/* d_qidx int64 [nq][kq], d_qval float32 [nq][kq] -> d_wq float64 [nq][kq], d_sq float64 [nq], d_kept int32 [nq] (the members that sit
 * in the query's list) and d_dropped int32 [nq] (those that do not) */
int pvs_krr_query_dev(pvs_ctx* ctx, const int32_t* d_nbr, const float* d_sim, const uint64_t* d_maskh, const double* d_v, const double* d_v0,
                      int64_t N, int kg, int k1, int k2, int gamma, const int64_t* d_qidx, const float* d_qval, int64_t nq, int kq,
                      double* d_wq, double* d_sq, int32_t* d_kept, int32_t* d_dropped);
/* -> d_scores float64 [nq][kr] */
int pvs_krr_score_dev(pvs_ctx* ctx, const int32_t* d_nbr, const double* d_w, const double* d_w0, const double* d_ws, int64_t N, int kg,
                      const int64_t* d_qidx, const float* d_qval, const double* d_wq, const double* d_sq, int64_t nq, int kq, int kr,
                      double lam, double* d_scores);

/* ---------------------------------------------------------------- local-descriptor retrieval: ASMK* 
 * The aggregated selective match kernel with binary signatures (Tolias, Avrithis, Jegou, ICCV 2013; Hamming embedding: Jegou,
 * Douze, Schmid, ECCV 2008): a large vocabulary, per image and visual word ONE B-bit signature of the summed residual, an inverted
 * file over words, and a score that sums a selectivity function of the Hamming distance over the words two images share.
 *
 * ENTRIES of an image with descriptor rows x_j (j in CSR order, any pvs_desc_kind; x_j[t] is the value the encoders use: the
 * RootSIFT kinds give what pvs_materialise_dev gives) and labels l_j (pvs_kmeans_predict_dev) against centroids c [K][D]:
 *   the entries are the image's distinct labels in ascending order.  For the entry of word w:
 *   V[t]   starts at +0 and adds (x_j[t] - c_w[t]) for j ascending over the rows with l_j = w: one float32 subtraction and one
 *          float32 addition, each rounded on its own.
 *   z[t]   with a projection P float32 [B][D]: starts at +0 and adds P[t][u] * V[u] for u ascending, a multiply then an add, never
 *          an fma.  Without one (P NULL, which needs B == D): z = V.
 *   bits   bit t of the signature is 1 iff z[t] >= 0 (a NaN gives 0).  A sum that starts at +0 never ends at -0, so a row that sits
 *          on its centroid gives all ones.  Bit t lies in uint32 word t / 32 at position t % 32.
 *   limits B in {32, 64, 96, 128}, 1 <= D <= 128, 1 <= K <= 65536.  An image of more than 8192 rows is PVS_ERR_UNSUPPORTED; an
 *          image of 0 rows has 0 entries.
 *
 * INTEGER WEIGHTS, computed by the caller in float64:
 *   sel    int32 [B + 1]: with u = 1 - 2 h / B, sel[h] = rint(1023 u^alpha) where u > tau, 0 otherwise (alpha > 0, 0 <= tau < 1).
 *   wt     int32 [K]: 0 for a word no database image holds, otherwise clip(rint(64 ln(N / df_w)), 1, 1023) with df_w the number of
 *          database images that hold w; 64 for every held word when idf is off.
 *   gamma  gamma(X) = float32(1 / sqrt(float64(sum over the entries of X of 1023 wt[w]))), 0 for an image without entries (or
 *          whose sum is 0).  With it an image scores 1 against itself.
 *
 * SCORE of query Q against image X:
 *   acc    = sum over the words w that Q and X share of wt[w] * sel[popcount(sig_Q(w) xor sig_X(w))], in uint32, exact: the caller
 *            refuses a query whose sum of 1023 wt[w] reaches 2^32 (4104 entries are always safe).  Integer sums do not depend on
 *            the order, so the scan may be cut anywhere and every cut gives the same bits.
 *   score  = (float32(acc) * gamma(Q)) * gamma(X): the conversion rounds to nearest even, the two multiplies are rounded separately.
 *
 * STORAGE: entries sorted by (word, image): word_off int64 [K + 1], ent_img int32 [E] (ascending inside a word, each image at most
 * once per word), ent_sig uint32 [E][B / 32], gamma_db float32 [N].
 * The entry points enqueue on the context's stream and do not wait for it. */
/* cb gives c, K and D.  d_offsets int64 [n_images + 1] are the CSR offsets of the rows (offsets[0] = 0) and h_offsets their HOST
 * copy: all checks and sizing come from it; the two must agree.  d_labels int32 [total_desc], every label in [0, K) (a
 * precondition).  d_proj float32 [bits][D] or NULL.  Image i writes its entries to the slots offsets[i] .. offsets[i] + count[i] - 1
 * of d_ent_word int32 [total_desc] and d_ent_sig uint32 [total_desc][bits / 32], and count[i] to d_ent_count int32 [n_images]: an
 * image cannot have more entries than rows, so there is no capacity protocol.  Slots beyond count[i] are left unwritten.  Timed on
 * slot 1. */
int pvs_asmk_aggregate_dev(pvs_ctx* ctx, const pvs_codebook* cb, const void* d_desc, int desc_kind, const int64_t* d_offsets,
                           const int64_t* h_offsets, int64_t n_images, int64_t total_desc, const int32_t* d_labels,
                           const float* d_proj, int bits, int32_t* d_ent_word, uint32_t* d_ent_sig, int32_t* d_ent_count);

/* MULTIPLE ASSIGNMENT of a query's rows (the paper assigns every query row to its 5 nearest words; the database stays single
 * assignment).
 *
 * TOP-M LIST of a row.  For a row x (the value the encoders use; for the RootSIFT kinds, what pvs_materialise_dev gives) and
 * centroid j < K:
 *   dot_j  the float32 fma chain of the exact assignment kernel: it starts at +0 and runs over the dims in the order
 *          (8t + e, 8t + 4 + e), e = 0..3, t ascending.
 *   v_j    = fmaf(-2, dot_j, |c_j|^2), with |c_j|^2 the sequential float32 sum the codebook stores.  |x|^2 is not added.  A v_j that
 *          is NaN or +inf counts as +inf.
 *   list   the first m centroids in the order (v ascending, j ascending), 1 <= m <= min(K, 8).  The order is total, so the list does
 *          not depend on how the vocabulary or the rows are cut.  Column 0 is the label of pvs_kmeans_predict_dev for every input
 *          that entry point accepts, an all-NaN row included (label 0).  Padded rows of the table (index >= K) never appear.
 * The same descriptor kinds, D range and alignment rules (vector and scalar load path) as pvs_kmeans_predict_dev.  d_labels int32
 * [total_desc][m]; d_val float32 [total_desc][m] (the v of every label) or NULL.  A workgroup takes 256 rows and a contiguous
 * range of the table's 256-centroid blocks: splits = 0 leaves the number of ranges to the host (about two workgroups per compute
 * unit over the launch, at least one block per range, so a large batch gets 1), any other value is clamped to 1..(K_pad / 256),
 * K_pad = K rounded up to 256 (1 range where K <= 128) -- every value gives the same bits.  No global atomics.  m outside
 * 1..min(K, 8) is PVS_ERR_INVALID; total_desc == 0 is a no-op.  Enqueues on the context's stream and never waits.  Timed on slot 0. */
int pvs_kmeans_topm_dev(pvs_ctx* ctx, const pvs_codebook* cb, const void* d_desc, int desc_kind, int64_t total_desc, int m, int splits,
                        int32_t* d_labels, float* d_val);
/* ENTRIES with m labels per row: d_labels int32 [total_desc][m], the m labels of a row distinct and in [0, K) (preconditions;
 * pvs_kmeans_topm_dev gives such lists).  The entries of an image are the distinct labels over all its rows and slots, ascending.
 * V of word w adds (x_j - c_w) for j ascending over the rows that hold w in any slot; z, bits and storage as above.  Image i
 * writes to the slots m offsets[i] .. of d_ent_word int32 [m total_desc] and d_ent_sig uint32 [m total_desc][bits / 32].  Limits:
 * at most 8192 rows and rows * m <= 16384 keys per image (a 2000-row query fits at m = 8), 1 <= m <= min(K, 8); more is
 * PVS_ERR_UNSUPPORTED.  At m = 1 the outputs are those of pvs_asmk_aggregate_dev.  Timed on slot 1. */
int pvs_asmk_aggregate_ma_dev(pvs_ctx* ctx, const pvs_codebook* cb, const void* d_desc, int desc_kind, const int64_t* d_offsets,
                              const int64_t* h_offsets, int64_t n_images, int64_t total_desc, const int32_t* d_labels, int m,
                              const float* d_proj, int bits, int32_t* d_ent_word, uint32_t* d_ent_sig, int32_t* d_ent_count);
/* Query q holds the entries h_q_off[q] .. h_q_off[q + 1] - 1 of d_q_word int32 / d_q_sig uint32 [.][bits / 32] (h_q_off: HOST int64
 * [nq + 1], non-decreasing); a query word outside [0, K) is skipped.  d_word_off, d_ent_img, d_ent_sig, d_gamma_db: the storage
 * above for N < 2^31 images; d_wt int32 [K], d_sel int32 [bits + 1], d_gamma_q float32 [nq].  Signature arrays are 16-byte aligned
 * at bits = 128, 8-byte at 64, 4-byte otherwise.  d_scores float32 [nq][ld], ld >= N: every column < N of every row is written
 * exactly once, with +0 where nothing is shared; columns >= N are untouched.  A workgroup serves one query and a slice of
 * consecutive images: slice_images = 0 leaves the slice to the host (about two workgroups per compute unit, no slice below 1024
 * images), otherwise it is a multiple of 64 in 64..32768 -- every value gives the same bits.  No global atomics, no float atomics.
 * The ranking is pvs_topk_dev on the panel.  Timed on slot 2. */
int pvs_asmk_score_dev(pvs_ctx* ctx, int64_t nq, const int64_t* h_q_off, const int32_t* d_q_word, const uint32_t* d_q_sig, int bits,
                       int K, const int64_t* d_word_off, const int32_t* d_ent_img, const uint32_t* d_ent_sig, int64_t N,
                       const int32_t* d_wt, const int32_t* d_sel, const float* d_gamma_q, const float* d_gamma_db, int slice_images,
                       float* d_scores, int64_t ld);

/* ---------------------------------------------------------------- ASMK maintenance: inversion on the device, list insert and remove
 * With weights that belong to the vocabulary and not to the indexed set (a FROZEN index), gamma(X) depends on X's own entries alone,
 * and adding or removing images is what section 15 calls an update: data movement, with the arrays of a from-scratch build of the
 * surviving images as the result, byte for byte.  The entry points below are integer counting and data movement: no floating
 * point; integer atomics only on counters in LDS whose result does not depend on the order of arrival, never to decide a position;
 * no kernel waits for another workgroup; every output element is written exactly once.  They enqueue on the context's stream and
 * never wait for the device: all sizing comes from the host copies of the offsets.  They serve fewer than 2^31 entries (slots for
 * the inversion); more is PVS_ERR_UNSUPPORTED, found on the host.  1 <= K <= 65536, bits in {32, 64, 96, 128}, W = bits / 32.
 * Signature arrays are 16-byte aligned at W = 4, 8-byte at W = 2, 4-byte otherwise, and move as one load of that width per entry.
 * Timed on slot 6. */
/* IMAGE-MAJOR ENTRIES -> INVERTED FILE.  The inputs are what pvs_asmk_aggregate_dev leaves behind: d_offsets int64 [n_images + 1]
 * with its HOST copy h_offsets (total = h_offsets[n_images]), d_ent_count int32 [n_images], d_ent_word int32 [total], d_ent_sig
 * uint32 [total][W].  The entries of image i are the slots offsets[i] .. offsets[i] + count[i] - 1 (count clamped to the image's
 * slots); slots beyond are unwritten memory and are never read as entries.  An entry whose word lies outside [0, K) is dropped.
 * Outputs, all sized by total: d_word_off int64 [K + 1], d_out_img int32 [total], d_out_sig uint32 [total][W].  word_off[K] = E is
 * the number of defined output entries; the entry (image i, word w) stands at word_off[w] + #{i' < i holding w} and carries the id
 * img_base + i (img_base + n_images <= 2^31 - 1).  Elements at and beyond E are not written.  A stable least-significant-digit
 * radix sort on the word, 8-bit digits (one pass for K <= 256, otherwise two); a slot that is no entry carries a digit behind
 * every word.  Each pass: digit counts per tile, one exclusive scan over [digit][tile], a scatter in which a lane's rank inside its
 * tile comes from wave ballots and per-wave counts in LDS.  tile_entries = 0 leaves the tile to the host; other values are a
 * multiple of 256 in 256..65536 (clamped, and raised where total needs more than 65536 tiles) -- every value gives the same bytes.
 * total == 0 writes zero offsets.  Uses the workspace (16 bytes per slot and the counts). */
int pvs_asmk_invert_dev(pvs_ctx* ctx, int K, int bits, const int64_t* d_offsets, const int64_t* h_offsets, int64_t n_images,
                        const int32_t* d_ent_count, const int32_t* d_ent_word, const uint32_t* d_ent_sig, int64_t img_base,
                        int tile_entries, int64_t* d_word_off, int32_t* d_out_img, uint32_t* d_out_sig);
/* d_sums int64 [n_images]: sums[i] = the sum over image i's entries (same slot layout) of 1023 wt[w], d_wt int32 [K]; a word outside
 * [0, K) adds 0.  One wave per image.  gamma is float32(1 / sqrt(float64(sums[i]))) on the host, 0 where the sum is 0. */
int pvs_asmk_weight_sums_dev(pvs_ctx* ctx, int K, const int64_t* d_offsets, const int64_t* h_offsets, int64_t n_images,
                             const int32_t* d_ent_count, const int32_t* d_ent_word, const int32_t* d_wt, int64_t* d_sums);
/* LIST INSERT.  A stored file (d_word_off with its HOST copy h_word_off, d_ent_img, d_ent_sig; E = h_word_off[K] entries) and a
 * batch inverted by pvs_asmk_invert_dev (d_new_off / h_new_off, d_new_img, d_new_sig; b = h_new_off[K]) are merged into the
 * d_out_* arrays of E + b entries: out_word_off[w] = word_off[w] + new_off[w], and list w is its old entries followed by its new
 * ones.  Precondition: every new id exceeds every stored id, so the result is sorted by (word, image).  One lane per merged entry
 * finds its word by a binary search of the summed offsets.  E + b < 2^31.  Any overlap of an output with an input is
 * PVS_ERR_INVALID.  E + b == 0 writes the offsets only. */
int pvs_asmk_insert_dev(pvs_ctx* ctx, int K, int bits, const int64_t* d_word_off, const int64_t* h_word_off, const int32_t* d_ent_img,
                        const uint32_t* d_ent_sig, const int64_t* d_new_off, const int64_t* h_new_off, const int32_t* d_new_img,
                        const uint32_t* d_new_sig, int64_t* d_out_word_off, int32_t* d_out_img, uint32_t* d_out_sig);
/* LIST REMOVE.  d_keep uint8 [N] and d_pos int64 [N + 1] by image id (pvs_keep_mask_dev / pvs_keep_positions_dev).  A stored entry e
 * survives iff keep[ent_img[e]] != 0 (an id outside [0, N) breaks a precondition: the entry is dropped), its new id is
 * pos[ent_img[e]], and the survivors keep their stored order.  out_word_off[w] = the number of survivors before word_off[w].
 * h_word_off is the HOST copy of d_word_off (E = h_word_off[K] < 2^31).  Outputs, sized by E, are disjoint from the inputs
 * (PVS_ERR_INVALID).  E == 0 writes zero offsets.  Uses the workspace (4 bytes per entry). */
int pvs_asmk_remove_dev(pvs_ctx* ctx, int K, int bits, int64_t N, const int64_t* d_word_off, const int64_t* h_word_off,
                        const int32_t* d_ent_img, const uint32_t* d_ent_sig, const uint8_t* d_keep, const int64_t* d_pos,
                        int64_t* d_out_word_off, int32_t* d_out_img, uint32_t* d_out_sig);

/* ---------------------------------------------------------------- ASMK query expansion: majority-vote signatures and new words
 * Query expansion on the entries themselves (Tolias, Jegou, "Visual query expansion with or without geometry: refining local
 * descriptors by feature aggregation", Pattern Recognition 2014): the signatures of the query's words are refined by the signatures
 * that reliable results, the MEMBERS, store for the same words, and words that enough members agree on are added.  The members'
 * entries are read out of the word-major file: every list is sorted by image, so "does member i hold word w, and with which
 * signature" is one binary search.  All arithmetic is integer; nothing depends on any order of summation.
 *
 * INPUTS per query q: its entries as pvs_asmk_score_dev takes them (words strictly ascending, signatures q_w);
 *   members[q][0 .. R)  int32 image ids in [0, N), strictly ascending, then -1 padding up to R (0 <= R <= 32): the members are the
 *                       ids before the first negative value;
 *   votes[q][0 .. R)    int32 in 1..1023, votes[q][r] belongs to members[q][r];
 * and, shared by the call, query_vote in 0..65535, h_max in 0..B, min_support in 0..33.
 *
 * DEFINITION.  For each word w in [0, K), ascending: M(w) is the set of members r whose id stands in list w, s_r the signature
 * stored there.
 *   w is a query word with signature q_w:
 *     the voters are the members r in M(w) with popcount(s_r xor q_w) <= h_max: the gate always uses the ORIGINAL query signature;
 *     for each bit t: tally[t] = query_vote (2 q_w[t] - 1) + sum over the voters of votes[r] (2 s_r[t] - 1), in int32
 *     (|tally| <= 65535 + 32 * 1023);
 *     the new bit is 1 if tally > 0, 0 if tally < 0 and q_w[t] if tally = 0;
 *     w is always an output entry.
 *   w is not a query word:
 *     w is an output entry iff min_support >= 1 and |M(w)| >= min_support;
 *     the tally runs over all of M(w), with no gate and no query term;
 *     the bit is 1 iff tally >= 0: the z >= 0 rule of the signatures.
 * Query words outside [0, K) are dropped from the output (the score skips them anyway).
 *
 * OUTPUT per query: the entries ascending by word; count, the true number of entries; sum, the int64 sum of 1023 wt[w] over the
 * output entries (what gamma(Q) and the caller's 2^32 check need).  With R = 0 the output equals the query's in-range entries;
 * with min_support = 0 no word is added. */
/* Query block as for the score: nq, HOST h_q_off int64 [nq + 1], d_q_word, d_q_sig, bits.  File: K, d_word_off, d_ent_img,
 * d_ent_sig, N < 2^31.  d_members and d_votes int32 [nq][R] (may be NULL at R = 0).  d_wt int32 [K].
 * Outputs: d_out_word int32 [nq][cap], d_out_sig uint32 [nq][cap][bits / 32], d_out_count int32 [nq], d_out_sum int64 [nq].
 * CAPACITY: count and sum are always the true values; output entry j of query q goes to position j of its row iff j < cap; nothing
 * at or beyond min(count, cap) of a row is touched.  cap = min(K, |Q| + R * 8192) always suffices (an image holds at most 8192
 * entries); cap = 0 gives counts and sums alone (the two output arrays may then be NULL).
 * DETERMINISM: a wave owns 64 consecutive words of one query, a workgroup a tile of tile_words words.  tile_words = 0 leaves the cut
 * to the host (about eight workgroups per compute unit over the query block); other values are a multiple of 64 in 64..4096 --
 * every value gives the same bytes, since the position of an entry comes from a count per 64 words and one scan per query.  No
 * output position is decided by an atomic (the kernels hold none), no workgroup waits for another, every written element is
 * written once.
 * CHECKS on the host, PVS_ERR_INVALID: bits, K, N, R, query_vote, h_max, min_support, tile_words, cap < 0, decreasing offsets,
 * NULL arrays, and the alignment of pvs_asmk_score_dev (signature arrays, d_out_sig included: 16 bytes at bits = 128, 8 at 64, 4
 * otherwise).  BROKEN PRECONDITIONS on the device side: a member id >= N stands in no list, so it is never in M(w) and changes
 * nothing; a member list that does not ascend strictly (before its padding) gives unspecified members of M(w), but count, sum and
 * positions stay consistent with each other and no read or write leaves its array; votes outside 1..1023 are used as they are.
 * The query offsets travel as kernel arguments, 128 queries per launch: more queries mean more launches (three per 128 queries:
 * mark, scan, emit), all enqueued by the one call.  Uses the workspace (256 + 8 bytes per 64 words and query of a block, 34 MB at
 * K = 65536 and 128 queries).  Enqueues on the context's stream and never waits for it.  Timed on slot 6. */
int pvs_asmk_expand_dev(pvs_ctx* ctx, int64_t nq, const int64_t* h_q_off, const int32_t* d_q_word, const uint32_t* d_q_sig, int bits,
                        int K, const int64_t* d_word_off, const int32_t* d_ent_img, const uint32_t* d_ent_sig, int64_t N, int R,
                        const int32_t* d_members, const int32_t* d_votes, int query_vote, int h_max, int min_support,
                        const int32_t* d_wt, int tile_words, int cap, int32_t* d_out_word, uint32_t* d_out_sig,
                        int32_t* d_out_count, int64_t* d_out_sum);

/* ---------------------------------------------------------------- int8 resident index: one signed byte per dimension
 * A scalar-quantised copy of float32 rows, a quarter of their size, ranked by the cosine of the CODE rows.  Every sum is an integer,
 * so no tiling, split of a row or order of summation changes a bit, and a restatement with int64 sums gives the same bytes.
 *   code row    x float32 [L], 1 <= L <= 131072, every element finite (a PRECONDITION of the entry point: it is not checked).
 *               amax = max_t |x[t]|.  amax == 0 gives all-zero codes.  Otherwise c[t] = (int8) rint((x[t] / amax) * 127.0f): an IEEE
 *               float32 division, then a float32 multiply, each rounded on its own; rint rounds half to even.  |x / amax| <= 1, so
 *               |c| <= 127 and -128 never occurs.  No reciprocal is formed: a subnormal amax is no special case.
 *   storage     int8 [N][ld], ld = PVS_SQ8_LD(L) = 64 ceil(L / 64); bytes L .. ld of every row are zero, so they add nothing to any
 *               sum; every row starts on 64 bytes and a k-step of the matrix instruction never straddles a row end.
 *   row factor  ss = sum_t c[t]^2 as an integer; inv = ss == 0 ? 0.0f : (float)(1.0 / sqrt((double)ss)): float64 square root and
 *               division, then one rounding to float32.  One float32 per row.  The quantisation scale amax / 127 cancels in a
 *               cosine of the codes and is not stored.
 *   score       acc = sum_t cq[t] * cd[t] in int32, exact because 127^2 * 131072 = 2 114 060 288 < 2^31 (this bounds L);
 *               score = ((float)acc * inv_q) * inv_d: the int32 -> float32 conversion rounds to nearest even, then two multiplies,
 *               each rounded on its own.  The queries are quantised by the same rule.
 *   ranking     (score descending, global index ascending): the rule of pvs_topk_dev.  (float)acc merges neighbouring integers
 *               above 2^24, so ties happen and the index decides them.
 * n == 0 and nq == 0 are no-ops.  Both entry points enqueue on the context's stream and do not wait for it. */
#define PVS_SQ8_LD(L) (64 * (((L) + 63) / 64))
/* d_x float32 [n][L] -> d_codes int8 [n][ld] (16-byte aligned; the padding bytes are written too, as zeros) and d_inv float32 [n].
 * Nothing past row n of either output is touched.  Timed on slot 6. */
int pvs_sq8_encode_dev(pvs_ctx* ctx, const float* d_x, int64_t n, int L, int8_t* d_codes, float* d_inv);
/* Scores of nq code rows against N code rows (both [.][ld], 16-byte aligned, with their row factors) and their ranking, with the
 * semantics of pvs_pq_scan_topk_dev and pvs_cosine_topk_dev: row 0 has global index col_offset; merge != 0 merges into the running
 * lists already in d_idx / d_val; 1 <= k <= N (k > 1024 needs merge == 0 and N <= 2^28, as there).  The nq x N score matrix never
 * exists: scores pass through a bounded workspace panel into the top-k kernels, panel by panel.  d_idx int64 [nq][k], d_val float32
 * [nq][k].  Two device paths sit behind the entry, chosen by PVS_OPT_SQ8_PATH: a tiled int8 GEMM on v_mfma_i32_32x32x32_i8 and a
 * one-pass row scan on v_dot4 for a handful of queries; they give the same bits.  Timed on slots 2 (scores) and 3 (ranking). */
int pvs_sq8_topk_dev(pvs_ctx* ctx, const int8_t* d_qcodes, const float* d_inv_q, int64_t nq, const int8_t* d_codes,
                     const float* d_inv_db, int64_t N, int L, int k, int64_t col_offset, int merge, int64_t* d_idx, float* d_val);

/* ---------------------------------------------------------------- threshold join and pair components
 * "Everything at least this similar": the pairs (i, j) of query row i and database row j whose score reaches a threshold, and the
 * connected components of such a pair list.
 *   score       s(i, j) is the float32 value pvs_cosine_dev writes for query row i and database row j with the same inverse-norm
 *               arrays (NULL = 1): the defined recurrence of the f32 GEMM, whatever the path, the tile size or the capacity.
 *   hit         s(i, j) >= threshold, compared in float32.  A NaN score is never a hit; -0 >= 0 holds; the returned score bits are
 *               the stored ones, not canonicalised.
 *   self-join   PVS_RANGE_UPPER: the caller promises that Q and DB hold the same rows (nq == N); only j > i is emitted.  s(i, j) and
 *               s(j, i) are the same bits: fma(a, b, c) and inv_a * inv_b are symmetric in the operands.
 * flags: PVS_RANGE_UPPER = 1.  path: 0 auto, 1 exact f32 panels, 2 fp16 prefilter + exact re-score (silently 1 where it
 * does not qualify).  tile: 0 = the plan's geometry; 1..32768 = row blocks and column panels of that many rows (test seams).
 * Writes min(total, capacity) triples, *h_total = total; total > capacity -> PVS_ERR_CAPACITY with both valid, nothing
 * written at or beyond capacity (capacity 0 with NULL outputs = count only).  Synchronises.
 * Order on the device: row blocks ascending, within a row block column panels ascending, within a tile (row, col) ascending.
 * h_stats (optional, int64[6]): [0] 1 if the prefilter ran, [1] row blocks redone by the exact path, [2] candidates re-scored,
 * [3] tiles scored, [4] tiles skipped below the diagonal, [5] 0.
 * path 0 is path 2 from 1024 query rows on and path 1 below (the measurement behind the rule: DESIGN.md section 24).  Path 2 qualifies
 * as pvs_cosine_topk_filtered_dev does (16-byte aligned rows, L % 8 == 0, finite values) and needs both norm arrays.
 * PVS_ERR_INVALID, before anything is launched: a non-finite threshold, unknown flags, PVS_RANGE_UPPER with nq != N, path outside
 * 0..2, tile outside 0..32768, capacity outside 0..PVS_RANGE_MAX_CAPACITY, a missing pointer that will be written, L < 1, nq or N
 * beyond 2^31 - 1.  nq == 0 or N == 0 is a no-op with total 0.  Timed on slots 2 (scores), 3 (count, scan, emit), 6 (fp16 rows), 7. */
#define PVS_RANGE_UPPER 1
#define PVS_RANGE_MAX_CAPACITY ((int64_t)1 << 40)
int pvs_cosine_range_dev(pvs_ctx* ctx, const float* d_Q, int64_t nq, const float* d_DB, int64_t N, int64_t L,
                         const float* d_inv_q, const float* d_inv_db, float threshold, int flags, int path, int tile,
                         int64_t capacity, int64_t* d_row, int64_t* d_col, float* d_val, int64_t* h_total, int64_t* h_stats);
/* The threshold join on int8 code rows: d_qcodes int8 [nq][ld] and d_codes int8 [N][ld], ld = PVS_SQ8_LD(L),
 * 16-byte aligned, with their row factors, as pvs_sq8_topk_dev takes them.
 *   score       s(i, j) = ((float)acc * inv_q[i]) * inv_d[j], acc the int32 dot product of the two code rows: the bits pvs_sq8_topk_dev
 *               reports for the pair, on every path, tile size and capacity.  No prefilter, no re-score: acc is an integer.
 *   hit         s(i, j) >= threshold compared in float32; a NaN score (a factor may be anything) is never a hit; a zero row has
 *               factor 0 and scores +0 against everything, so it hits iff threshold <= 0.
 *   self-join   PVS_RANGE_UPPER (nq == N, the same codes and factors on both sides): for i < j the pair is a hit iff s(i, j) >= threshold
 *               with row i in the QUERY role, and s(i, j) is the value emitted.  The score is NOT symmetric: (a * x) * y and
 *               (a * y) * x are two separately rounded products and differ in about a third of the pairs.  A pair with
 *               s(i, j) < threshold <= s(j, i) is not emitted.
 * path: 0 auto, 1 panel (the float panels of pvs_sq8_topk_dev, row scan or GEMM by PVS_OPT_SQ8_PATH, thresholded where they lie),
 * 2 mask (the int8 GEMM writes one bit per pair; popcount, scan, ordered emit; the scores of the emitted pairs are computed once
 * at the end, from the same integer by the same expression).  Path 0 is path 1 while pvs_sq8_topk_dev takes the row scan (at most
 * 4 queries under the default PVS_OPT_SQ8_PATH) and path 2 beyond.  tile: 0 = the plan's geometry (panel: 8192 x 32768; mask:
 * 8192 x 262144); 1..32768 = row blocks and column panels of that many rows (test seams; any value, no multiple of 32 or 128 needed).
 * Order, capacity protocol, flags and synchronisation are those of pvs_cosine_range_dev: row blocks ascending, column panels
 * ascending, (row, col) ascending within a tile; min(total, capacity) triples written, *h_total = total, PVS_ERR_CAPACITY when
 * total > capacity with nothing written at or beyond the capacity; capacity 0 with NULL outputs counts.  No position is decided by
 * an atomic.  h_stats (optional, int64[6]): [0] the path taken (1 or 2), [2] pairs scored by the pair kernel, [3] tiles scored,
 * [4] tiles skipped below the diagonal, [1] and [5] 0.
 * PVS_ERR_INVALID, before anything is launched: a non-finite threshold, unknown flags, PVS_RANGE_UPPER with nq != N, path outside
 * 0..2, tile outside 0..32768, capacity outside 0..PVS_RANGE_MAX_CAPACITY, L outside 1..131072, nq or N beyond 2^31 - 1, a missing
 * or misaligned pointer that will be used.  nq == 0 or N == 0 is a no-op with total 0.  Timed on slots 2 (scores), 3 (count, scan,
 * emit) and 7 (pair scores). */
int pvs_sq8_range_dev(pvs_ctx* ctx, const int8_t* d_qcodes, const float* d_inv_q, int64_t nq, const int8_t* d_codes,
                      const float* d_inv_db, int64_t N, int L, float threshold, int flags, int path, int tile, int64_t capacity,
                      int64_t* d_row, int64_t* d_col, float* d_val, int64_t* h_total, int64_t* h_stats);
/* Connected components of an undirected pair list over N nodes: d_label[i] (int32) = the smallest node index of i's component.
 * E == 0 gives the identity.  N < 2^31.  h_stats (optional, int64[2]): [0] rounds, [1] components.  A node id outside [0, N) is
 * PVS_ERR_INVALID (checked on the device before the first round).  Synchronises. */
int pvs_pair_components_dev(pvs_ctx* ctx, const int64_t* d_a, const int64_t* d_b, int64_t E, int64_t N, int32_t* d_label,
                            int64_t* h_stats);

/* ---------------------------------------------------------------- subset search: the k best among an allowed set
 * S is a set of row indices of an index with N rows, 1 <= |S| <= N.  The subset ranking of a query is the full ranking of the index
 * with the rows outside S deleted, cut to k, 1 <= k <= |S|: (score descending, index ascending), indices in the numbering of the full
 * index, and the score bits those of the unrestricted entry for that pair -- the float32 value pvs_cosine_dev writes, or
 * ((float)acc * inv_q) * inv_d on code rows.  A score depends on its two rows and two factors alone, so the result does not depend on
 * the path, the tile, the chunk or how S was given; a row outside S never appears; S = all rows gives the unrestricted lists.
 *   handle      h_ids is a HOST array of ns ids, strictly ascending within [0, N), N < 2^31; it is checked on the host before anything
 *               is allocated (PVS_ERR_INVALID).  The handle owns the ids on the device, a bitmask of ceil(N / 32) uint32 words on the
 *               device (row i is bit i & 31 of word i >> 5, built on the host; the bits beyond N are zero) and a host copy of the ids.
 *               pvs_subset_create waits for the upload; pvs_subset_destroy waits for the stream.
 *   path        0 auto (the listed path iff 4 ns <= N), 1 mask, 2 listed.
 *               mask: the panels of the unrestricted entry (tile > 0: tile x tile blocks, a test seam); a column panel that holds no
 *               id is skipped on the host, the others are scored by the unrestricted entry's scorer, the columns outside S are set to
 *               -inf and the panel is ranked.  listed: the ids in chunks of at most 256 MiB of rows (tile > 0: at most tile rows);
 *               rows and factors are gathered into the workspace, scored by the same scorer, ranked by position in the id list and
 *               the positions are replaced by the ids at the end.
 *   outputs     d_idx int64 [nq][k], d_val float32 [nq][k]; k <= |S| makes every entry a row of S with its score.
 *   h_stats     optional int64[4]: [0] the path taken (1 or 2), [1] panels scored (mask: per query block and column panel) or chunks
 *               gathered (listed), [2] column panels skipped (mask, per query block), [3] rows gathered (listed: ns).
 * PVS_ERR_INVALID, before anything is launched: k < 1, k > ns, k > 1024, a handle made for another N, path outside 0..2, tile
 * outside 0..32768.  nq == 0 is a no-op.  Both entries enqueue on the context's stream and do not wait for it.  The int8 entry reads
 * PVS_OPT_SQ8_PATH as pvs_sq8_topk_dev does.  Timed on slots 2 (scores), 3 (mask, ranking), 6 (gather, positions -> ids). */
typedef struct pvs_subset pvs_subset;
int pvs_subset_create(pvs_ctx* ctx, const int64_t* h_ids, int64_t ns, int64_t N, pvs_subset** out);
int pvs_subset_destroy(pvs_ctx* ctx, pvs_subset* subset);
int pvs_cosine_topk_subset_dev(pvs_ctx* ctx, const float* d_Q, int64_t nq, const float* d_DB, int64_t N, int64_t L,
                               const float* d_inv_q, const float* d_inv_db, const pvs_subset* subset, int k, int path, int tile,
                               int64_t* d_idx, float* d_val, int64_t* h_stats);
int pvs_sq8_topk_subset_dev(pvs_ctx* ctx, const int8_t* d_qcodes, const float* d_inv_q, int64_t nq, const int8_t* d_codes,
                            const float* d_inv_db, int64_t N, int L, const pvs_subset* subset, int k, int path, int tile,
                            int64_t* d_idx, float* d_val, int64_t* h_stats);

/* ---------------------------------------------------------------- inverted lists over the int8 code rows
 * Sub-linear search with the int8 score itself: the code rows of section 22 cut into nlist inverted lists, a query scores the rows
 * of its nprobe best lists only.  All arithmetic is section 22's (code row, ld, inv, the int32 acc, ((float)acc * inv_q) * inv_d):
 * no new floating-point rule, and every reported score is, bit for bit, the one pvs_sq8_topk_dev reports for that pair.
 *   centroids   are code rows: cent_codes int8 [nlist][ld] and cent_inv float32 [nlist], 1 <= nlist <= 65536, made from float32
 *               centroid rows by pvs_sq8_encode_dev.
 *   list        of a database row: the first entry of the ranking of the row's codes against the centroid codes by (score
 *               descending, list number ascending): pvs_sq8_topk_dev with k = 1.
 *   probes      of a query: the first nprobe entries of the same ranking, 1 <= nprobe <= min(nlist, 1024).
 *   storage     section 14's with m = ld: codes int8 [N][ld], inv float32 [N] and ids int32 [N] in (list, original index) order,
 *               list_off int64 [nlist + 1] on the device with a host copy.  N < 2^31.  Empty lists are legal.
 *   candidates  of a query: the concatenation of its probed lists in probe order, padded to W as pvs_ivf_scan_topk_dev computes W: the
 *               sum of the nprobe longest lists, rounded up to 64, at least 64.  A live slot holds (score, original id), a padding
 *               slot (-inf, -1).  A probe outside [0, nlist) counts as an empty list.  Distinct probes are a precondition.
 *   result      the first k candidates by (score descending, original id ascending), -0 and +0 tied, 1 <= k <= 1024; slots beyond
 *               the live candidates are idx = -1, val = -inf.
 * With nprobe = nlist every row is a candidate exactly once and the two orders coincide: the lists equal those of pvs_sq8_topk_dev
 * on the same rows byte for byte.  acc is an integer, so no slice size, wave assignment or summation order changes a bit. */
/* d_qcodes int8 [nq][ld] and d_codes int8 [N][ld] are 16-byte aligned; d_probe int64 [nq][nprobe] as pvs_sq8_topk_dev gave it
 * against the centroid codes.  h_list_off is a HOST copy of d_list_off: all sizing is done from it, so nothing inside the call waits
 * for the device; the two must agree.  slice_rows: candidate slots per workgroup, a test seam: 0 lets the host choose (about two
 * workgroups per compute unit over the query block, at least 64 slots each), any other value is rounded up to a multiple of 16; the
 * result does not depend on it.  d_idx int64 [nq][k], d_val float32 [nq][k].  PVS_ERR_INVALID, before anything is launched: L
 * outside 1..131072, nlist, nprobe or k out of range, negative nq or slice_rows, host offsets that do not start at 0 or that
 * decrease, N >= 2^31, a missing or misaligned pointer.  nq == 0 is a no-op; N == 0 writes only (-1, -inf).  Enqueues on the
 * context's stream and does not wait for it.  Timed on slots 2 (the scan) and 3 (the ranking). */
int pvs_ivf_sq8_scan_topk_dev(pvs_ctx* ctx, const int8_t* d_qcodes, const float* d_inv_q, int64_t nq, int L, const int64_t* d_probe,
                              int nprobe, const int64_t* d_list_off, const int64_t* h_list_off, int nlist, const int8_t* d_codes,
                              const float* d_inv_db, const int32_t* d_ids, int k, int slice_rows, int64_t* d_idx, float* d_val);
/* What the entry above will do for nq queries on this context's device, from the host offsets alone (no device work): h_plan int64
 * [4] = W, the queries of one block, the slots per workgroup S (a multiple of 16), the workgroups per query ceil(W / S).  The same
 * checks of nprobe, nlist, slice_rows and the offsets. */
int pvs_ivf_sq8_scan_plan(pvs_ctx* ctx, int64_t nq, int nprobe, const int64_t* h_list_off, int nlist, int slice_rows, int64_t* h_plan);

/* ---------------------------------------------------------------- the same search scanned by list
 * For batches of queries.  Every definition above stays: the candidate rows, W, the padding and the result are those of
 * pvs_ivf_sq8_scan_topk_dev, and the lists are the same bytes for every input; only who computes which slot differs.  The (query,
 * probe) pairs of a block of queries are grouped by list, and every tile of 128 consecutive stored rows of a list is scored against
 * the grouped pairs of that list, 128 at a time, on the int8 matrix pipe: a probed row is read once per query block, not once per query.
 *   base[q][j]  the first slot of probe j in the candidate row of query q: the lengths of the probed lists before it in probe order,
 *               a probe outside [0, nlist) counting as length 0.  total[q]: the live slots of the row.
 *   grouping    the pairs (q, j) whose probe lies in [0, nlist), in (list ascending, query ascending) order: a stable sort of the
 *               pairs in (q, j) order on the list number.  goff[l] .. goff[l + 1] are the pairs of list l, gq[p] the query of grouped
 *               pair p and gbase[p] its base[q][j].  P = goff[nlist] pairs; gq and gbase behind P are not written. */
/* The grouping of one query block alone: d_probe int64 [qn][nprobe] -> d_base int32 [qn][nprobe], d_total int32 [qn], d_goff int32
 * [nlist + 1], d_gq and d_gbase int32 [qn nprobe].  0 <= qn <= 65535 and qn nprobe <= 2^20 (one query block); nlist and nprobe as
 * above; N < 2^31 is a precondition.  qn == 0 writes goff = 0 only.  No position is decided by an atomic.  Enqueues on the context's
 * stream; nothing is copied to the host and the stream is not waited for.  Timed on slot 6. */
int pvs_ivf_sq8_group_probes_dev(pvs_ctx* ctx, const int64_t* d_probe, int64_t qn, int nprobe, const int64_t* d_list_off, int nlist,
                                 int32_t* d_base, int32_t* d_total, int32_t* d_goff, int32_t* d_gq, int32_t* d_gbase);
/* The arguments, checks and results of pvs_ivf_sq8_scan_topk_dev, with query_block in the place of slice_rows: the queries grouped
 * at a time, a test seam: 0 lets the host choose (the query block of the scan above, capped so that query_block nprobe <= 2^20 pairs,
 * 32 MiB of grouping arrays), a positive value means at most that many; negative is PVS_ERR_INVALID; the result does not depend
 * on it.  Timed on slots 6 (the grouping), 2 (the tiles) and 3 (the ranking). */
int pvs_ivf_sq8_scan_lists_topk_dev(pvs_ctx* ctx, const int8_t* d_qcodes, const float* d_inv_q, int64_t nq, int L, const int64_t* d_probe,
                                    int nprobe, const int64_t* d_list_off, const int64_t* h_list_off, int nlist, const int8_t* d_codes,
                                    const float* d_inv_db, const int32_t* d_ids, int k, int query_block, int64_t* d_idx, float* d_val);
/* h_plan int64 [4] = W, the queries of one block, the row tiles (workgroups of the tile kernel: the sum over the lists of
 * ceil(length / 128)), the pairs one block's grouping arrays hold (query block x nprobe).  No device work. */
int pvs_ivf_sq8_scan_lists_plan(pvs_ctx* ctx, int64_t nq, int nprobe, const int64_t* h_list_off, int nlist, int query_block,
                                int64_t* h_plan);

/* ---------------------------------------------------------------- measurement hooks (bench.py) */
/* Enable per-kernel-family HIP-event timing on the context's stream. which: 0 assign, 1 aggregate,
 * 2 cosine gemm (and the ADC scan of the compact index, which stands in its place), 3 top-k, 4 fisher posterior, 5 fisher moments, 6 norms/misc, 7 exact re-scoring (filtered top-k). */
#define PVS_TIMER_SLOTS 8
int pvs_timers_enable(pvs_ctx* ctx, int on);
int pvs_timers_reset(pvs_ctx* ctx);
int pvs_timers_read(pvs_ctx* ctx, int which, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* PVSIM_H */
