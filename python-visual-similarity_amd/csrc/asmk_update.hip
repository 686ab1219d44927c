// ASMK maintenance: the inverted file is made, extended and thinned on the device.
//   pvs_asmk_invert_dev       image-major entries in slots -> the inverted file: a stable LSD radix sort on the word
//   pvs_asmk_weight_sums_dev  per image the sum of 1023 wt[w] over its entries: one wave per image
//   pvs_asmk_insert_dev       a stored file + an inverted batch -> the merged file: one lane per merged entry
//   pvs_asmk_remove_dev       keep mask and positions by image id -> the compacted file with renumbered ids
// Integer counting and data movement only.  The only atomics are adds to a digit histogram in LDS, whose sums do not depend on the
// order of arrival; every position comes from a scan or a ballot.  No kernel waits for another workgroup: the passes are separate
// launches ordered by the stream.  Every loop is bounded by a launch argument.  tests/asmk_update_numpy.py restates each entry point.
//
// The sort (radix_sort.hpp, shared with ivf_sq8.hip) moves 8-byte items, (key << 32) | source slot, with key = the word, or K for a
// slot that is no entry: K's digit is 256 in every pass, behind every word.  The signatures move once, in the final gather, as one
// load and one store of their full width.
// From list_common.hpp: the block scan, last_le, move_sig, the two offset kernels, the tile and grid rules, the overlap and offset checks.
// From radix_sort.hpp: the exclusive scan of int32 counts, the sort passes, the offsets of the sorted keys.
#include <algorithm>

#include "list_common.hpp"
#include "radix_sort.hpp"

namespace pvs {

constexpr int64_t AU_MAX_ENTRIES = ((int64_t)1 << 31) - 1;

// ------------------------------------------------------------------------------------------------- inversion
// one item per slot: the key is the word of an entry, K for a slot beyond the image's count or a word outside [0, K)
__global__ __launch_bounds__(AU_THREADS) void au_items_kernel(const int64_t* __restrict__ offsets, int n, int steps,
                                                              const int32_t* __restrict__ count, const int32_t* __restrict__ word, int K,
                                                              int64_t total, uint64_t* __restrict__ items) {
  for (int64_t s = (int64_t)blockIdx.x * AU_THREADS + threadIdx.x; s < total; s += (int64_t)gridDim.x * AU_THREADS) {
    const int i = last_le([&](int t) { return offsets[t]; }, n, s, steps);
    const int64_t first = offsets[i], rows = offsets[i + 1] - first;
    const int64_t c = min(max((int64_t)count[i], (int64_t)0), rows);
    uint32_t key = (uint32_t)K;
    if (s - first < c) {
      const int32_t w = word[s];
      if (w >= 0 && w < K) key = (uint32_t)w;
    }
    items[s] = ((uint64_t)key << 32) | (uint64_t)(uint32_t)s;
  }
}

template <int W>
__global__ __launch_bounds__(AU_THREADS) void au_gather_kernel(const uint64_t* __restrict__ items, int64_t total, int K,
                                                               const int64_t* __restrict__ offsets, int n, int steps,
                                                               const uint32_t* __restrict__ sig, int64_t img_base, int32_t* __restrict__ out_img,
                                                               uint32_t* __restrict__ out_sig) {
  for (int64_t j = (int64_t)blockIdx.x * AU_THREADS + threadIdx.x; j < total; j += (int64_t)gridDim.x * AU_THREADS) {
    const uint64_t item = items[j];
    if ((uint32_t)(item >> 32) >= (uint32_t)K) continue;
    const int64_t s = (int64_t)(uint32_t)item;
    if (s >= total) continue;
    out_img[j] = (int32_t)(img_base + last_le([&](int t) { return offsets[t]; }, n, s, steps));
    move_sig<W>(sig + s * W, out_sig + j * W);
  }
}

// ------------------------------------------------------------------------------------------------- weight sums
// one wave per image; `rounds` = ceil(the longest image / 64) bounds the loop
__global__ __launch_bounds__(AU_THREADS) void au_weight_sums_kernel(const int64_t* __restrict__ offsets, int64_t n, int rounds,
                                                                    const int32_t* __restrict__ count, const int32_t* __restrict__ word,
                                                                    const int32_t* __restrict__ wt, int K, int64_t* __restrict__ sums) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * AU_WAVES + (threadIdx.x >> 6);
  if (i >= n) return;
  const int64_t first = offsets[i];
  const int64_t c = min(max((int64_t)count[i], (int64_t)0), offsets[i + 1] - first);
  int64_t acc = 0;
  for (int r = 0; r < rounds; ++r) {
    const int64_t t = (int64_t)r * WAVE + lane;
    if (t < c) {
      const int32_t w = word[first + t];
      if (w >= 0 && w < K) acc += (int64_t)1023 * wt[w];
    }
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) acc += __shfl_down(acc, s, WAVE);
  if (lane == 0) sums[i] = acc;
}

// ------------------------------------------------------------------------------------------------- insert and remove
// One lane per merged entry j: its word is the last w with word_off[w] + new_off[w] <= j; inside the list the old entries come first.
template <int W>
__global__ __launch_bounds__(AU_THREADS) void au_insert_kernel(const int64_t* __restrict__ word_off, const int64_t* __restrict__ new_off, int K,
                                                               const int32_t* __restrict__ img, const uint32_t* __restrict__ sig,
                                                               const int32_t* __restrict__ new_img, const uint32_t* __restrict__ new_sig,
                                                               int64_t E, int64_t b, int32_t* __restrict__ out_img,
                                                               uint32_t* __restrict__ out_sig) {
  const int64_t total = E + b;
  for (int64_t j = (int64_t)blockIdx.x * AU_THREADS + threadIdx.x; j < total; j += (int64_t)gridDim.x * AU_THREADS) {
    const int lo = last_le([&](int w) { return word_off[w] + new_off[w]; }, K, j, 17);   // K <= 2^16
    const int64_t first = word_off[lo], old_len = word_off[lo + 1] - first, r = j - (first + new_off[lo]);
    if (r < old_len) {
      const int64_t s = first + r;
      if (s < 0 || s >= E) continue;                  // the device offsets disagree with the host's: a broken precondition, nothing is read out of bounds
      out_img[j] = img[s];
      move_sig<W>(sig + s * W, out_sig + j * W);
    } else {
      const int64_t s = new_off[lo] + (r - old_len);
      if (s < 0 || s >= b) continue;
      out_img[j] = new_img[s];
      move_sig<W>(new_sig + s * W, out_sig + j * W);
    }
  }
}

// flag[e] = 1 where the stored entry e survives; flag[E] = 0, so that the scan leaves the number of survivors there
__global__ __launch_bounds__(AU_THREADS) void au_survivor_flags_kernel(const int32_t* __restrict__ img, const uint8_t* __restrict__ keep, int64_t N,
                                                                       int64_t E, int32_t* __restrict__ flag) {
  for (int64_t e = (int64_t)blockIdx.x * AU_THREADS + threadIdx.x; e <= E; e += (int64_t)gridDim.x * AU_THREADS) {
    int f = 0;
    if (e < E) {
      const int64_t id = img[e];
      f = id >= 0 && id < N && keep[id] ? 1 : 0;
    }
    flag[e] = f;
  }
}

template <int W>
__global__ __launch_bounds__(AU_THREADS) void au_remove_kernel(const int32_t* __restrict__ img, const uint32_t* __restrict__ sig,
                                                               const uint8_t* __restrict__ keep, const int64_t* __restrict__ pos,
                                                               const int32_t* __restrict__ spos, int64_t N, int64_t E,
                                                               int32_t* __restrict__ out_img, uint32_t* __restrict__ out_sig) {
  for (int64_t e = (int64_t)blockIdx.x * AU_THREADS + threadIdx.x; e < E; e += (int64_t)gridDim.x * AU_THREADS) {
    const int64_t id = img[e];
    if (id < 0 || id >= N || !keep[id]) continue;
    const int64_t p = spos[e];
    if (p < 0 || p >= E) continue;
    out_img[p] = (int32_t)pos[id];
    move_sig<W>(sig + e * W, out_sig + p * W);
  }
}

static int au_log2_steps(int64_t n) {
  int s = 1;
  while (((int64_t)1 << s) < n) ++s;
  return s;
}

static int au_check_shape(const char* fn, int K, int bits) {
  if (!word_count_ok(K)) PVS_FAIL(PVS_ERR_INVALID, "%s: need 1 <= K <= 65536 (got %d)", fn, K);
  if (!sig_bits_ok(bits)) PVS_FAIL(PVS_ERR_INVALID, "%s: bits must be 32, 64, 96 or 128 (got %d)", fn, bits);
  return PVS_OK;
}

static int au_check_offsets(const char* fn, const char* what, const int64_t* h, int64_t count) {
  const int64_t bad = offsets_first_break(h, count);
  if (bad == 0) PVS_FAIL(PVS_ERR_INVALID, "%s: %s[0] must be 0", fn, what);
  if (bad > 0) PVS_FAIL(PVS_ERR_INVALID, "%s: %s must not decrease (at %lld)", fn, what, (long long)(bad - 1));
  return PVS_OK;
}

}  // namespace pvs

using namespace pvs;

PVS_EXPORT int pvs_asmk_invert_dev(pvs_ctx* ctx, int K, int bits, const int64_t* d_offsets, const int64_t* h_offsets, int64_t n_images,
                                   const int32_t* d_ent_count, const int32_t* d_ent_word, const uint32_t* d_ent_sig, int64_t img_base,
                                   int tile_entries, int64_t* d_word_off, int32_t* d_out_img, uint32_t* d_out_sig) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(au_check_shape(__func__, K, bits));
  if (n_images < 0 || img_base < 0 || img_base + n_images > AU_MAX_ENTRIES)
    PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_invert_dev: need n_images >= 0, img_base >= 0 and img_base + n_images < 2^31 (got %lld, %lld)",
             (long long)n_images, (long long)img_base);
  if (tile_entries < 0) PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_invert_dev: tile_entries must not be negative (got %d)", tile_entries);
  PVS_NEED(h_offsets, "host offsets");
  PVS_TRY(au_check_offsets(__func__, "offsets", h_offsets, n_images));
  const int64_t total = h_offsets[n_images];
  if (total > AU_MAX_ENTRIES) PVS_FAIL(PVS_ERR_UNSUPPORTED, "pvs_asmk_invert_dev: %lld slots, the inversion serves fewer than 2^31", (long long)total);
  PVS_NEED(d_word_off, "word_off");
  PVS_ALIGNED(d_word_off, 8, "word_off");
  PVS_HIP(hipSetDevice(ctx->device));
  if (total == 0) {
    PVS_HIP(hipMemsetAsync(d_word_off, 0, (size_t)(K + 1) * 8, ctx->stream));
    return PVS_OK;
  }
  const int W = bits / 32;
  PVS_NEED(d_offsets, "offsets");
  PVS_NEED(d_ent_count, "ent_count");
  PVS_NEED(d_ent_word, "ent_word");
  PVS_NEED(d_ent_sig, "ent_sig");
  PVS_NEED(d_out_img, "out img");
  PVS_NEED(d_out_sig, "out sig");
  PVS_ALIGNED(d_offsets, 8, "offsets");
  PVS_ALIGNED(d_ent_count, 4, "ent_count");
  PVS_ALIGNED(d_ent_word, 4, "ent_word");
  PVS_ALIGNED(d_out_img, 4, "out img");
  PVS_ALIGNED(d_ent_sig, sig_align(W), "ent_sig");
  PVS_ALIGNED(d_out_sig, sig_align(W), "out sig");
  if (ranges_overlap(d_out_sig, total * W * 4, d_ent_sig, total * W * 4) || ranges_overlap(d_out_img, total * 4, d_ent_word, total * 4) ||
      ranges_overlap(d_out_img, total * 4, d_ent_sig, total * W * 4) || ranges_overlap(d_out_sig, total * W * 4, d_ent_word, total * 4) ||
      ranges_overlap(d_word_off, (int64_t)(K + 1) * 8, d_offsets, (n_images + 1) * 8))
    PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_invert_dev: an output overlaps an input");

  const int64_t tile = invert_tile(tile_entries, total);
  const int64_t ntiles = (total + tile - 1) / tile, ncounts = (int64_t)AU_BINS * ntiles;
  const AsmkInvertLayout lay = asmk_invert_layout((size_t)total, (size_t)ncounts, (size_t)((ncounts + AU_SCAN_BLOCK - 1) / AU_SCAN_BLOCK));
  void* block = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_UPDATE, lay.bytes, &block));
  uint64_t *src = lay.items_a(block), *dst = lay.items_b(block);
  int32_t *counts = lay.counts(block), *partials = lay.partials(block);
  const int n = (int)n_images, steps = au_log2_steps(n_images);

  ScopedTimer t(ctx, T_MISC);
  hipLaunchKernelGGL(au_items_kernel, dim3(flat_grid(ctx->num_cu, total)), dim3(AU_THREADS), 0, ctx->stream, d_offsets, n, steps, d_ent_count, d_ent_word, K,
                     total, src);
  PVS_HIP(hipGetLastError());
  PVS_TRY(au_launch_sort(ctx, src, dst, total, tile, ntiles, K, counts, partials, &src));
  hipLaunchKernelGGL(au_key_off_kernel<int64_t>, dim3((K + 1 + AU_THREADS - 1) / AU_THREADS), dim3(AU_THREADS), 0, ctx->stream, src, total, K, d_word_off);
  PVS_HIP(hipGetLastError());
  return dispatch_sig_words(W, [&](auto w) -> int {
    hipLaunchKernelGGL((au_gather_kernel<decltype(w)::value>), dim3(flat_grid(ctx->num_cu, total)), dim3(AU_THREADS), 0, ctx->stream, src, total, K,
                       d_offsets, n, steps, d_ent_sig, img_base, d_out_img, d_out_sig);
    PVS_HIP(hipGetLastError());
    return PVS_OK;
  });
}

PVS_EXPORT int pvs_asmk_weight_sums_dev(pvs_ctx* ctx, int K, const int64_t* d_offsets, const int64_t* h_offsets, int64_t n_images,
                                        const int32_t* d_ent_count, const int32_t* d_ent_word, const int32_t* d_wt, int64_t* d_sums) {
  PVS_NEED(ctx, "ctx");
  if (!word_count_ok(K)) PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_weight_sums_dev: need 1 <= K <= 65536 (got %d)", K);
  if (n_images < 0 || n_images > AU_MAX_ENTRIES) PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_weight_sums_dev: need 0 <= n_images < 2^31 (got %lld)", (long long)n_images);
  PVS_NEED(h_offsets, "host offsets");
  PVS_TRY(au_check_offsets(__func__, "offsets", h_offsets, n_images));
  if (n_images == 0) return PVS_OK;
  PVS_NEED(d_offsets, "offsets");
  PVS_NEED(d_ent_count, "ent_count");
  PVS_NEED(d_wt, "wt");
  PVS_NEED(d_sums, "sums");
  PVS_ALIGNED(d_offsets, 8, "offsets");
  PVS_ALIGNED(d_sums, 8, "sums");
  PVS_ALIGNED(d_ent_count, 4, "ent_count");
  PVS_ALIGNED(d_ent_word, 4, "ent_word");
  PVS_ALIGNED(d_wt, 4, "wt");
  int64_t longest = 0;
  for (int64_t i = 0; i < n_images; ++i) longest = std::max(longest, h_offsets[i + 1] - h_offsets[i]);
  if (longest > AU_MAX_ENTRIES) PVS_FAIL(PVS_ERR_UNSUPPORTED, "pvs_asmk_weight_sums_dev: an image of %lld slots", (long long)longest);
  if (longest > 0) PVS_NEED(d_ent_word, "ent_word");
  if (ranges_overlap(d_sums, n_images * 8, d_offsets, (n_images + 1) * 8) || ranges_overlap(d_sums, n_images * 8, d_ent_count, n_images * 4) ||
      ranges_overlap(d_sums, n_images * 8, d_wt, (int64_t)K * 4) || ranges_overlap(d_sums, n_images * 8, d_ent_word, h_offsets[n_images] * 4))
    PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_weight_sums_dev: sums overlaps an input");
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer t(ctx, T_MISC);
  hipLaunchKernelGGL(au_weight_sums_kernel, dim3((unsigned)((n_images + AU_WAVES - 1) / AU_WAVES)), dim3(AU_THREADS), 0, ctx->stream, d_offsets,
                     n_images, (int)((longest + WAVE - 1) / WAVE), d_ent_count, d_ent_word, d_wt, K, d_sums);
  PVS_HIP(hipGetLastError());
  return PVS_OK;
}

PVS_EXPORT int pvs_asmk_insert_dev(pvs_ctx* ctx, int K, int bits, const int64_t* d_word_off, const int64_t* h_word_off, const int32_t* d_ent_img,
                                   const uint32_t* d_ent_sig, const int64_t* d_new_off, const int64_t* h_new_off, const int32_t* d_new_img,
                                   const uint32_t* d_new_sig, int64_t* d_out_word_off, int32_t* d_out_img, uint32_t* d_out_sig) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(au_check_shape(__func__, K, bits));
  PVS_NEED(h_word_off, "host word_off");
  PVS_NEED(h_new_off, "host new_off");
  PVS_TRY(au_check_offsets(__func__, "word_off", h_word_off, K));
  PVS_TRY(au_check_offsets(__func__, "new_off", h_new_off, K));
  const int64_t E = h_word_off[K], b = h_new_off[K], total = E + b;
  if (E > AU_MAX_ENTRIES || b > AU_MAX_ENTRIES || total > AU_MAX_ENTRIES)
    PVS_FAIL(PVS_ERR_UNSUPPORTED, "pvs_asmk_insert_dev: %lld + %lld entries, list maintenance serves fewer than 2^31", (long long)E, (long long)b);
  const int W = bits / 32;
  PVS_NEED(d_word_off, "word_off");
  PVS_NEED(d_new_off, "new_off");
  PVS_NEED(d_out_word_off, "out word_off");
  PVS_ALIGNED(d_word_off, 8, "word_off");
  PVS_ALIGNED(d_new_off, 8, "new_off");
  PVS_ALIGNED(d_out_word_off, 8, "out word_off");
  if (E > 0) {
    PVS_NEED(d_ent_img, "ent_img");
    PVS_NEED(d_ent_sig, "ent_sig");
  }
  if (b > 0) {
    PVS_NEED(d_new_img, "new img");
    PVS_NEED(d_new_sig, "new sig");
  }
  if (total > 0) {
    PVS_NEED(d_out_img, "out img");
    PVS_NEED(d_out_sig, "out sig");
  }
  for (const void* p : {(const void*)d_ent_img, (const void*)d_new_img, (const void*)d_out_img})
    if (reinterpret_cast<uintptr_t>(p) % 4) PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_insert_dev: ids must be 4-byte aligned");
  for (const void* p : {(const void*)d_ent_sig, (const void*)d_new_sig, (const void*)d_out_sig})
    if (reinterpret_cast<uintptr_t>(p) % sig_align(W))
      PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_insert_dev: signatures must be %d-byte aligned", sig_align(W));
  const int64_t off_bytes = (int64_t)(K + 1) * 8, sw = (int64_t)W * 4;
  const ByteRange ins[] = {{d_word_off, off_bytes}, {d_new_off, off_bytes}, {d_ent_img, E * 4}, {d_ent_sig, E * sw}, {d_new_img, b * 4},
                           {d_new_sig, b * sw}},
                  outs[] = {{d_out_word_off, off_bytes}, {d_out_img, total * 4}, {d_out_sig, total * sw}};
  const int clash = outputs_overlap(outs, 3, ins, 6);
  if (clash == 1) PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_insert_dev: an output overlaps an input");
  if (clash == 2) PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_insert_dev: two outputs overlap");
  PVS_HIP(hipSetDevice(ctx->device));
  ScopedTimer t(ctx, T_MISC);
  hipLaunchKernelGGL(sum_offsets_kernel<int64_t>, dim3((K + 1 + 255) / 256), dim3(256), 0, ctx->stream, d_word_off, d_new_off, K + 1, d_out_word_off);
  PVS_HIP(hipGetLastError());
  if (total == 0) return PVS_OK;
  return dispatch_sig_words(W, [&](auto w) -> int {
    hipLaunchKernelGGL((au_insert_kernel<decltype(w)::value>), dim3(flat_grid(ctx->num_cu, total)), dim3(AU_THREADS), 0, ctx->stream, d_word_off, d_new_off,
                       K, d_ent_img, d_ent_sig, d_new_img, d_new_sig, E, b, d_out_img, d_out_sig);
    PVS_HIP(hipGetLastError());
    return PVS_OK;
  });
}

PVS_EXPORT int pvs_asmk_remove_dev(pvs_ctx* ctx, int K, int bits, int64_t N, const int64_t* d_word_off, const int64_t* h_word_off,
                                   const int32_t* d_ent_img, const uint32_t* d_ent_sig, const uint8_t* d_keep, const int64_t* d_pos,
                                   int64_t* d_out_word_off, int32_t* d_out_img, uint32_t* d_out_sig) {
  PVS_NEED(ctx, "ctx");
  PVS_TRY(au_check_shape(__func__, K, bits));
  if (N < 0 || N > AU_MAX_ENTRIES) PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_remove_dev: need 0 <= N < 2^31 (got %lld)", (long long)N);
  PVS_NEED(h_word_off, "host word_off");
  PVS_TRY(au_check_offsets(__func__, "word_off", h_word_off, K));
  const int64_t E = h_word_off[K];
  if (E > AU_MAX_ENTRIES) PVS_FAIL(PVS_ERR_UNSUPPORTED, "pvs_asmk_remove_dev: %lld entries, list maintenance serves fewer than 2^31", (long long)E);
  const int W = bits / 32;
  PVS_NEED(d_out_word_off, "out word_off");
  PVS_ALIGNED(d_out_word_off, 8, "out word_off");
  PVS_HIP(hipSetDevice(ctx->device));
  if (E == 0) {
    PVS_HIP(hipMemsetAsync(d_out_word_off, 0, (size_t)(K + 1) * 8, ctx->stream));
    return PVS_OK;
  }
  PVS_NEED(d_word_off, "word_off");
  PVS_NEED(d_ent_img, "ent_img");
  PVS_NEED(d_ent_sig, "ent_sig");
  PVS_NEED(d_keep, "keep");
  PVS_NEED(d_pos, "pos");
  PVS_NEED(d_out_img, "out img");
  PVS_NEED(d_out_sig, "out sig");
  PVS_ALIGNED(d_word_off, 8, "word_off");
  PVS_ALIGNED(d_pos, 8, "pos");
  PVS_ALIGNED(d_ent_img, 4, "ent_img");
  PVS_ALIGNED(d_out_img, 4, "out img");
  PVS_ALIGNED(d_ent_sig, sig_align(W), "ent_sig");
  PVS_ALIGNED(d_out_sig, sig_align(W), "out sig");
  const int64_t off_bytes = (int64_t)(K + 1) * 8, sw = (int64_t)W * 4;
  const ByteRange ins[] = {{d_word_off, off_bytes}, {d_ent_img, E * 4}, {d_ent_sig, E * sw}, {d_keep, N}, {d_pos, (N + 1) * 8}},
                  outs[] = {{d_out_word_off, off_bytes}, {d_out_img, E * 4}, {d_out_sig, E * sw}};
  const int clash = outputs_overlap(outs, 3, ins, 5);
  if (clash == 1) PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_remove_dev: an output overlaps an input");
  if (clash == 2) PVS_FAIL(PVS_ERR_INVALID, "pvs_asmk_remove_dev: two outputs overlap");
  const int64_t M = E + 1;
  const AsmkRemoveLayout lay = asmk_remove_layout((size_t)E, (size_t)((M + AU_SCAN_BLOCK - 1) / AU_SCAN_BLOCK));
  void* block = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_UPDATE, lay.bytes, &block));
  int32_t *spos = lay.spos(block), *partials = lay.partials(block);
  ScopedTimer t(ctx, T_MISC);
  hipLaunchKernelGGL(au_survivor_flags_kernel, dim3(flat_grid(ctx->num_cu, M)), dim3(AU_THREADS), 0, ctx->stream, d_ent_img, d_keep, N, E, spos);
  PVS_HIP(hipGetLastError());
  PVS_TRY(au_launch_scan(ctx, spos, M, partials));
  hipLaunchKernelGGL(remap_offsets_kernel<int32_t>, dim3((K + 1 + 255) / 256), dim3(256), 0, ctx->stream, d_word_off, spos, E, K + 1, d_out_word_off);
  PVS_HIP(hipGetLastError());
  return dispatch_sig_words(W, [&](auto w) -> int {
    hipLaunchKernelGGL((au_remove_kernel<decltype(w)::value>), dim3(flat_grid(ctx->num_cu, E)), dim3(AU_THREADS), 0, ctx->stream, d_ent_img, d_ent_sig, d_keep,
                       d_pos, spos, N, E, d_out_img, d_out_sig);
    PVS_HIP(hipGetLastError());
    return PVS_OK;
  });
}
