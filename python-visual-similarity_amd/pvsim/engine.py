"""Thin object layer over the C-ABI: one Context = one MI355X + one HIP stream; device tables behind
handles.  Everything here marshals pointers and sizes -- no arithmetic happens in Python."""
from __future__ import annotations

import ctypes as C
import os
import sys
import threading

import numpy as np

from . import _ffi
from ._ffi import DESC_F32, DESC_F32_ROOTSIFT, DESC_U8_ROOTSIFT, check, norm_params, ptr

__all__ = ["Context", "default_context", "pack_descriptors", "dsift_count", "dsift_frames", "sift_workspace", "diffuse_workspace", "DESC_F32", "DESC_F32_ROOTSIFT", "DESC_U8_ROOTSIFT"]


def pack_descriptors(desc_list, dim: int, dtype=np.float32):
    """list of (n_i, D) arrays -> (packed (sum n_i, D) C-contiguous, offsets int64 (N+1,))."""
    counts = [0 if d is None else int(d.shape[0]) for d in desc_list]
    offsets = np.zeros(len(desc_list) + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    packed = np.empty((int(offsets[-1]), dim), dtype=dtype)
    for d, o in zip(desc_list, offsets[:-1]):
        if d is not None and d.shape[0]:
            if d.shape[1] != dim:
                raise RuntimeError(f"descriptor dimension {d.shape[1]} does not match the model input dimension {dim}")
            packed[o:o + d.shape[0]] = d
    return packed, offsets


def dsift_count(h: int, w: int, step: int, sizes) -> int:
    """pvs_dsift_count: descriptor rows of one h x w image (host arithmetic, no device)."""
    sizes = np.ascontiguousarray(sizes, dtype=np.int32).reshape(-1)
    n = C.c_int64()
    check(_ffi.lib().pvs_dsift_count(int(h), int(w), int(step), ptr(sizes) if sizes.size else None, sizes.size, C.byref(n)))
    return int(n.value)


def dsift_frames(h: int, w: int, step: int, sizes) -> np.ndarray:
    """pvs_dsift_frames: (n, 3) float32 rows (x centre, y centre, bin size), in descriptor order."""
    sizes = np.ascontiguousarray(sizes, dtype=np.int32).reshape(-1)
    out = np.empty((dsift_count(h, w, step, sizes), 3), dtype=np.float32)
    check(_ffi.lib().pvs_dsift_frames(int(h), int(w), int(step), ptr(sizes), sizes.size, ptr(out), out.shape[0]))
    return out


def sift_workspace(h: int, w: int, n_octave_layers: int = 3, upsample: bool = True):
    """pvs_sift_workspace: (bytes of one h x w image's Gaussian pyramid, loose upper bound of its rows); host arithmetic."""
    nbytes, rows = C.c_size_t(), C.c_int64()
    check(_ffi.lib().pvs_sift_workspace(int(h), int(w), int(n_octave_layers), int(bool(upsample)), C.byref(nbytes), C.byref(rows)))
    return int(nbytes.value), int(rows.value)


def diffuse_workspace(n: int, columns: int) -> int:
    """pvs_diffuse_workspace: bytes of the work buffer of one pvs_diffuse_cg_dev call over `columns` columns; host arithmetic."""
    nbytes = C.c_size_t()
    check(_ffi.lib().pvs_diffuse_workspace(int(n), int(columns), C.byref(nbytes)))
    return int(nbytes.value)


class _Handle:
    _destroy = None

    def __init__(self, ctx: "Context", handle):
        self.ctx, self.handle = ctx, handle

    def close(self):
        if self.handle is not None and self.ctx.handle is not None:
            getattr(_ffi.lib(), self._destroy)(self.ctx.handle, self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Codebook(_Handle):
    _destroy = "pvs_codebook_destroy"
    K = D = 0


class GMM(_Handle):
    _destroy = "pvs_gmm_destroy"
    K = D = 0


class PCATable(_Handle):
    _destroy = "pvs_pca_destroy"
    C = Din = 0


class PQTable(_Handle):
    _destroy = "pvs_pq_destroy"
    m = ksub = dsub = 0


class SubsetHandle(_Handle):
    _destroy = "pvs_subset_destroy"
    n = size = 0


class DeviceBuffer:
    """A block of device memory owned by a Context (pvs_malloc / pvs_free); .ptr is the raw device address."""

    def __init__(self, ctx: "Context", nbytes: int):
        self._ctx, self.nbytes, self.ptr = ctx, int(nbytes), 0
        self._cap = max(int(nbytes), 16)
        hit = ctx._take_cached(self._cap)
        if hit is not None:                      # a block this context released earlier: no hipMalloc / hipFree on the hot path
            self.ptr, self._cap = hit
            return
        p = C.c_void_p()
        check(_ffi.lib().pvs_malloc(ctx.handle, self._cap, C.byref(p)))
        self.ptr = int(p.value)

    @classmethod
    def view(cls, ctx: "Context", dptr: int, nbytes: int) -> "DeviceBuffer":
        """Non-owning view of device memory allocated elsewhere (e.g. torch.Tensor.data_ptr()); free() is a no-op."""
        b = cls.__new__(cls)
        b._ctx, b.nbytes, b.ptr, b._borrowed = ctx, int(nbytes), int(dptr), True
        return b

    def upload(self, a: np.ndarray, offset: int = 0):
        a = np.ascontiguousarray(a)
        if offset + a.nbytes > self.nbytes:
            raise ValueError("upload past the end of the device buffer")
        check(_ffi.lib().pvs_memcpy_h2d(self._ctx.handle, C.c_void_p(self.ptr + offset), ptr(a), a.nbytes))
        return self

    def download(self, shape, dtype, offset: int = 0) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        if offset + out.nbytes > self.nbytes:
            raise ValueError("download past the end of the device buffer")
        check(_ffi.lib().pvs_memcpy_d2h(self._ctx.handle, ptr(out), C.c_void_p(self.ptr + offset), out.nbytes))
        return out

    def fill_bytes(self, value: int):
        check(_ffi.lib().pvs_memset(self._ctx.handle, C.c_void_p(self.ptr), int(value), self.nbytes))
        return self

    def free(self):
        if self.ptr and not getattr(self, "_borrowed", False) and self._ctx.handle is not None:
            if not self._ctx._give_cached(self.ptr, getattr(self, "_cap", self.nbytes)):
                _ffi.lib().pvs_free(self._ctx.handle, C.c_void_p(self.ptr))
        self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _Scratch:
    """The device temporaries of one `with ctx.scratch() as tmp:` block.  `tmp(nbytes)` and `tmp.upload(array)` hand out DeviceBuffers
    that are freed when the block ends, however it ends; `tmp.keep(buf)` takes one out of the block: it is the caller's from then on."""

    def __init__(self, ctx):
        self.ctx, self._bufs = ctx, []

    def __call__(self, nbytes: int) -> DeviceBuffer:
        self._bufs.append(self.ctx.buffer(nbytes))
        return self._bufs[-1]

    def upload(self, a) -> DeviceBuffer:
        a = np.ascontiguousarray(a)
        buf = self(a.nbytes)
        return buf.upload(a) if a.nbytes else buf

    def keep(self, buf):
        self._bufs = [b for b in self._bufs if b is not buf]
        return buf

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        bufs, self._bufs = self._bufs, []
        for b in bufs:
            b.free()


class Context:
    """One device + one stream.  `stream` may be a raw hipStream_t (int), e.g.
    torch.cuda.current_stream().cuda_stream, so that work interleaves with torch in order."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self.handle = None
        h = C.c_void_p()
        check(_ffi.lib().pvs_init(int(device), C.c_void_p(stream), C.byref(h)))
        self.handle = h
        self.device = int(device)
        self._cache = []          # released DeviceBuffers kept for reuse: [(capacity, ptr)], bounded (training loops allocate the same sizes over and over; hipFree synchronises the device)

    _CACHE_BLOCKS, _CACHE_BYTES = 24, 2 << 30

    def _take_cached(self, nbytes):
        best = None
        for i, (cap, p) in enumerate(self._cache):
            if nbytes <= cap <= 2 * nbytes + 4096 and (best is None or cap < self._cache[best][0]):
                best = i
        if best is None:
            return None
        cap, p = self._cache.pop(best)
        return p, cap

    def _give_cached(self, p, cap):
        if len(self._cache) >= self._CACHE_BLOCKS or cap + sum(c for c, _ in self._cache) > self._CACHE_BYTES:
            return False
        self._cache.append((int(cap), int(p)))
        return True

    def trim(self):
        """Return the cached device blocks to the driver."""
        while self._cache:
            _, p = self._cache.pop()
            if self.handle is not None:
                _ffi.lib().pvs_free(self.handle, C.c_void_p(p))

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if self.handle is not None:
            self.trim()
            _ffi.lib().pvs_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sync(self):
        check(_ffi.lib().pvs_sync(self.handle))

    @property
    def stream(self) -> int:
        return int(_ffi.lib().pvs_stream(self.handle) or 0)

    def set_option(self, option: int, value: int) -> None:
        """pvs_set_option: pins one of several implementations that must agree bit for bit (tests, benchmarks)."""
        check(_ffi.lib().pvs_set_option(self.handle, int(option), int(value)))

    def get_option(self, option: int) -> int:
        v = C.c_int()
        check(_ffi.lib().pvs_get_option(self.handle, int(option), C.byref(v)))
        return int(v.value)

    def option(self, option: int, value: int):
        """Context manager: `with ctx.option(OPT_ASSIGN_PREFILTER, 0): ...` restores the previous value on exit."""
        ctx = self

        class _Scoped:
            def __enter__(self_inner):
                self_inner.old = ctx.get_option(option)
                ctx.set_option(option, value)

            def __exit__(self_inner, *exc):
                ctx.set_option(option, self_inner.old)

        return _Scoped()

    def gemm_last_plan(self) -> dict:
        """pvs_gemm_last_plan (diagnostic): the launches of this context's last similarity GEMM, by the names of
        _ffi.GEMM_PLAN_FIELDS; every value is -1 before the first one."""
        out = (C.c_int32 * 12)()
        check(_ffi.lib().pvs_gemm_last_plan(self.handle, out))
        return dict(zip(_ffi.GEMM_PLAN_FIELDS, (int(v) for v in out)))

    def diag_poison(self, byte: int, what: int = _ffi.POISON_WORKSPACE | _ffi.POISON_TABLE_CACHE) -> None:
        """pvs_diag_poison (diagnostic): fill the whole capacity of every workspace slot (what & 1) and / or of every block
        in the table block cache (what & 2) with `byte`, on this context's stream."""
        check(_ffi.lib().pvs_diag_poison(self.handle, int(byte), int(what)))

    def diag_ws_bytes(self) -> dict:
        """pvs_diag_ws_bytes (diagnostic): capacity of every workspace slot by the names of _ffi.WS_SLOTS; 0 = never reserved."""
        out = (C.c_size_t * len(_ffi.WS_SLOTS))()
        check(_ffi.lib().pvs_diag_ws_bytes(self.handle, out))
        return dict(zip(_ffi.WS_SLOTS, (int(v) for v in out)))

    def fill_dev(self, d_ptr: int, n_elems: int, dtype: str, value) -> None:
        """4- or 8-byte pattern fill on this context's stream (dtype: float32 / int32 / int64 / float64)."""
        a = np.array([value], dtype=dtype)
        if a.itemsize not in (4, 8):
            raise ValueError("fill_dev: 4- or 8-byte element types only")
        pattern = int(a.view(np.uint32 if a.itemsize == 4 else np.uint64)[0])
        check(_ffi.lib().pvs_fill_dev(self.handle, ptr(d_ptr), int(n_elems), a.itemsize, C.c_uint64(pattern)))

    def wait_for(self, other: "Context") -> None:
        """Work queued on THIS context after the call waits for everything `other` has queued so far (no host sync)."""
        check(_ffi.lib().pvs_stream_wait(self.handle, other.handle))

    def device_name(self) -> str:
        buf = C.create_string_buffer(256)
        check(_ffi.lib().pvs_device_name(self.handle, buf, 256))
        return buf.value.decode()

    # ------------------------------------------------------------------ tables
    def codebook(self, centroids) -> Codebook:
        c = np.ascontiguousarray(centroids, dtype=np.float32)
        if c.ndim != 2:
            raise ValueError("centroids must be (K, D)")
        h = C.c_void_p()
        check(_ffi.lib().pvs_codebook_create(self.handle, ptr(c), c.shape[0], c.shape[1], C.byref(h)))
        cb = Codebook(self, h)
        cb.K, cb.D = c.shape
        return cb

    def gmm(self, weights, means, covariances) -> GMM:
        w = np.ascontiguousarray(weights, dtype=np.float64)
        m = np.ascontiguousarray(means, dtype=np.float64)
        v = np.ascontiguousarray(covariances, dtype=np.float64)
        if m.ndim != 2 or v.shape != m.shape or w.shape != (m.shape[0],):
            raise ValueError("GMM tables must be weights (K,), means (K, D), diagonal covariances (K, D)")
        h = C.c_void_p()
        check(_ffi.lib().pvs_gmm_create(self.handle, ptr(w), ptr(m), ptr(v), m.shape[0], m.shape[1], C.byref(h)))
        g = GMM(self, h)
        g.K, g.D = m.shape
        return g

    def pca(self, components, mean) -> PCATable:
        comp = np.ascontiguousarray(components, dtype=np.float32)
        mu = np.ascontiguousarray(mean, dtype=np.float32).reshape(-1)
        if comp.ndim != 2 or mu.shape[0] != comp.shape[1]:
            raise ValueError("PCA tables must be components (C, Din), mean (Din,)")
        h = C.c_void_p()
        check(_ffi.lib().pvs_pca_create(self.handle, ptr(comp), ptr(mu), comp.shape[0], comp.shape[1], C.byref(h)))
        p = PCATable(self, h)
        p.C, p.Din = comp.shape
        return p

    def pq(self, codebooks) -> PQTable:
        """Product quantiser table from codebooks (m, ksub, dsub) float32."""
        c = np.ascontiguousarray(codebooks, dtype=np.float32)
        if c.ndim != 3:
            raise ValueError("codebooks must be (m, ksub, dsub)")
        h = C.c_void_p()
        check(_ffi.lib().pvs_pq_create(self.handle, ptr(c), c.shape[0], c.shape[1], c.shape[2], C.byref(h)))
        t = PQTable(self, h)
        t.m, t.ksub, t.dsub = c.shape
        return t

    # ------------------------------------------------------------------ encoders (host arrays)
    @staticmethod
    def _check_desc(packed, kind, dim):
        want = np.uint8 if kind == DESC_U8_ROOTSIFT else np.float32
        packed = np.ascontiguousarray(packed, dtype=want)
        if packed.ndim != 2 or packed.shape[1] != dim:
            raise RuntimeError(f"descriptors must be (n, {dim}), got {packed.shape}")
        return packed

    def vlad_encode(self, cb: Codebook, packed, offsets, kind=DESC_F32, power=1.0, norm_order=2, epsilon=1e-9,
                    pca: PCATable | None = None, return_labels=False):
        d_in = pca.Din if pca is not None else cb.D
        packed = self._check_desc(packed, kind, d_in)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = offsets.shape[0] - 1
        if offsets[-1] != packed.shape[0]:
            raise ValueError("offsets[-1] must equal the number of descriptor rows")
        out = np.empty((n, cb.K * cb.D), dtype=np.float32)
        labels = np.empty(packed.shape[0], dtype=np.int32) if return_labels else None
        prm = norm_params(power, norm_order, epsilon)
        check(_ffi.lib().pvs_vlad_encode(self.handle, cb.handle, pca.handle if pca else None, ptr(packed), kind,
                                         ptr(offsets), n, C.byref(prm), ptr(out), ptr(labels)))
        return (out, labels) if return_labels else out

    def fisher_encode(self, g: GMM, packed, offsets, kind=DESC_F32, power=0.5, norm_order=2, epsilon=1e-9,
                      pca: PCATable | None = None):
        d_in = pca.Din if pca is not None else g.D
        packed = self._check_desc(packed, kind, d_in)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = offsets.shape[0] - 1
        if offsets[-1] != packed.shape[0]:
            raise ValueError("offsets[-1] must equal the number of descriptor rows")
        out = np.empty((n, g.K + 2 * g.K * g.D), dtype=np.float64)
        prm = norm_params(power, norm_order, epsilon)
        # the device entry takes at most 65535 images per launch: batch here
        step = 32768
        for s in range(0, n, step):
            e = min(n, s + step)
            sub_off = offsets[s:e + 1] - offsets[s]
            sub = packed[offsets[s]:offsets[e]]
            check(_ffi.lib().pvs_fisher_encode(self.handle, g.handle, pca.handle if pca else None, ptr(sub), kind,
                                               ptr(np.ascontiguousarray(sub_off)), e - s, C.byref(prm), ptr(out[s:e])))
        return out

    # ------------------------------------------------------------------ similarity (host arrays)
    def cosine(self, a, b):
        a, b = np.asarray(a), np.asarray(b)
        f64 = not (a.dtype == np.float32 and b.dtype == np.float32)
        dt = np.float64 if f64 else np.float32
        a = np.ascontiguousarray(a, dtype=dt)
        b = np.ascontiguousarray(b, dtype=dt)
        if a.shape[1] != b.shape[1]:
            raise ValueError(f"Incompatible dimension for X and Y matrices: X.shape[1] == {a.shape[1]} "
                             f"while Y.shape[1] == {b.shape[1]}")
        out = np.empty((a.shape[0], b.shape[0]), dtype=dt)
        same = a is b or (a.ctypes.data == b.ctypes.data and a.shape == b.shape)
        check(_ffi.lib().pvs_cosine(self.handle, ptr(a), a.shape[0], ptr(a if same else b), b.shape[0], a.shape[1],
                                    int(f64), ptr(out)))
        return out

    def cosine_topk(self, q, db, k: int):
        q = np.ascontiguousarray(q, dtype=np.float32)
        db = np.ascontiguousarray(db, dtype=np.float32)
        if q.shape[1] != db.shape[1]:
            raise ValueError("query and database dimensions differ")
        idx = np.empty((q.shape[0], k), dtype=np.int64)
        val = np.empty((q.shape[0], k), dtype=np.float32)
        same = q.ctypes.data == db.ctypes.data and q.shape == db.shape
        check(_ffi.lib().pvs_cosine_topk(self.handle, ptr(q), q.shape[0], ptr(q if same else db), db.shape[0],
                                         q.shape[1], int(k), ptr(idx), ptr(val)))
        return idx, val

    def cosine_topk_f64(self, q, db, k: int):
        """float64 scores and ranking (the reference's dtype whenever an operand is not float32, e.g. Fisher encodings)."""
        q = np.ascontiguousarray(q, dtype=np.float64)
        db = np.ascontiguousarray(db, dtype=np.float64)
        if q.shape[1] != db.shape[1]:
            raise ValueError("query and database dimensions differ")
        idx = np.empty((q.shape[0], k), dtype=np.int64)
        val = np.empty((q.shape[0], k), dtype=np.float64)
        check(_ffi.lib().pvs_cosine_topk_f64(self.handle, ptr(q), q.shape[0], ptr(db), db.shape[0], q.shape[1], int(k),
                                             ptr(idx), ptr(val)))
        return idx, val

    # ------------------------------------------------------------------ device-pointer forms
    # All pointer arguments are raw device addresses (int), e.g. torch.Tensor.data_ptr().
    def vlad_encode_dev(self, cb, d_desc, kind, d_offsets, n_images, total_desc, d_out, power=1.0, norm_order=2,
                        epsilon=1e-9, pca=None, d_labels=None, d_inv_norm=None):
        prm = norm_params(power, norm_order, epsilon)
        check(_ffi.lib().pvs_vlad_encode_dev(self.handle, cb.handle, pca.handle if pca else None, ptr(d_desc), kind,
                                             ptr(d_offsets), n_images, total_desc, C.byref(prm), ptr(d_out),
                                             ptr(d_labels), ptr(d_inv_norm)))

    def fisher_encode_dev(self, g, d_desc, kind, d_offsets, n_images, total_desc, d_out, out_f64, power=0.5,
                          norm_order=2, epsilon=1e-9, pca=None):
        prm = norm_params(power, norm_order, epsilon)
        check(_ffi.lib().pvs_fisher_encode_dev(self.handle, g.handle, pca.handle if pca else None, ptr(d_desc), kind,
                                               ptr(d_offsets), n_images, total_desc, C.byref(prm), ptr(d_out),
                                               int(out_f64)))

    def kmeans_predict_dev(self, cb, d_desc, kind, total_desc, d_labels):
        check(_ffi.lib().pvs_kmeans_predict_dev(self.handle, cb.handle, ptr(d_desc), kind, total_desc, ptr(d_labels)))

    def kmeans_topm_dev(self, cb, d_desc, kind, total_desc, m, d_labels, d_val=None, splits=0):
        """pvs_kmeans_topm_dev: the m nearest centroids of every row by (v ascending, index ascending) -> d_labels int32 (total, m)
        and, when given, their v in d_val float32 (total, m).  splits = 0 leaves the cut of the vocabulary to the host."""
        check(_ffi.lib().pvs_kmeans_topm_dev(self.handle, cb.handle, ptr(d_desc), int(kind), int(total_desc), int(m), int(splits),
                                             ptr(d_labels), ptr(d_val)))

    def gmm_predict_proba_dev(self, g, d_desc, kind, total_desc, d_resp):
        check(_ffi.lib().pvs_gmm_predict_proba_dev(self.handle, g.handle, ptr(d_desc), kind, total_desc, ptr(d_resp)))

    def pca_transform_dev(self, p, d_desc, kind, total_desc, d_out):
        check(_ffi.lib().pvs_pca_transform_dev(self.handle, p.handle, ptr(d_desc), kind, total_desc, ptr(d_out)))

    def row_inv_norms_dev(self, d_x, rows, L, d_inv):
        check(_ffi.lib().pvs_row_inv_norms_dev(self.handle, ptr(d_x), rows, L, ptr(d_inv)))

    def cosine_dev(self, d_a, M, d_b, N, L, d_inva, d_invb, d_out, ldo):
        check(_ffi.lib().pvs_cosine_dev(self.handle, ptr(d_a), M, ptr(d_b), N, L, ptr(d_inva), ptr(d_invb), ptr(d_out), ldo))

    def cosine_dual_dev(self, d_a, M, d_b, N, L, d_inva, d_invb, d_out, ldo, d_out_t, ldt):
        check(_ffi.lib().pvs_cosine_dual_dev(self.handle, ptr(d_a), M, ptr(d_b), N, L, ptr(d_inva), ptr(d_invb), ptr(d_out),
                                             ldo, ptr(d_out_t), ldt))

    def topk_dev(self, d_scores, nq, ncols, ld, k, col_offset, merge, d_idx, d_val):
        check(_ffi.lib().pvs_topk_dev(self.handle, ptr(d_scores), nq, ncols, ld, k, col_offset, int(merge), ptr(d_idx),
                                      ptr(d_val)))

    def cosine_topk_dev(self, d_q, nq, d_db, N, L, d_invq, d_invdb, k, col_offset, merge, d_idx, d_val):
        check(_ffi.lib().pvs_cosine_topk_dev(self.handle, ptr(d_q), nq, ptr(d_db), N, L, ptr(d_invq), ptr(d_invdb), k,
                                             col_offset, int(merge), ptr(d_idx), ptr(d_val)))

    def cosine_topk_filtered_dev(self, d_q, nq, d_db, N, L, d_invq, d_invdb, k, d_idx, d_val):
        """Same lists as cosine_topk_dev (bit-identical), via the fp16 prefilter + exact re-scoring.
        -> dict(filtered, redone_exact, candidates, slots)"""
        st = (C.c_int64 * 4)()
        check(_ffi.lib().pvs_cosine_topk_filtered_dev(self.handle, ptr(d_q), nq, ptr(d_db), N, L, ptr(d_invq), ptr(d_invdb), k,
                                                      ptr(d_idx), ptr(d_val), st))
        return {"filtered": bool(st[0]), "redone_exact": int(st[1]), "candidates": int(st[2]), "slots": int(st[3])}

    # compact index
    def pq_encode_dev(self, pq, d_x, n, d_codes):
        check(_ffi.lib().pvs_pq_encode_dev(self.handle, pq.handle, ptr(d_x), n, ptr(d_codes)))

    def pq_lut_dev(self, pq, d_q, nq, d_lut):
        check(_ffi.lib().pvs_pq_lut_dev(self.handle, pq.handle, ptr(d_q), nq, ptr(d_lut)))

    def pq_scan_topk_dev(self, d_lut, nq, m, ksub, d_codes, N, d_invq, d_invdb, k, col_offset, merge, d_idx, d_val):
        check(_ffi.lib().pvs_pq_scan_topk_dev(self.handle, ptr(d_lut), nq, m, ksub, ptr(d_codes), N, ptr(d_invq), ptr(d_invdb), k,
                                              col_offset, int(merge), ptr(d_idx), ptr(d_val)))

    def rescore_rows_dev(self, d_q, nq, d_x, N, d, d_invq, d_invdb, d_cand, R, d_val):
        check(_ffi.lib().pvs_rescore_rows_dev(self.handle, ptr(d_q), nq, ptr(d_x), N, d, ptr(d_invq), ptr(d_invdb), ptr(d_cand), R,
                                              ptr(d_val)))

    # int8 resident index
    def sq8_encode_dev(self, d_x, n, L, d_codes, d_inv):
        """pvs_sq8_encode_dev: float32 rows (n, L) -> int8 codes (n, 64 ceil(L / 64)), zero padded, and 1 / sqrt(sum c^2) per row"""
        check(_ffi.lib().pvs_sq8_encode_dev(self.handle, ptr(d_x), int(n), int(L), ptr(d_codes), ptr(d_inv)))

    def sq8_topk_dev(self, d_qcodes, d_invq, nq, d_codes, d_invdb, N, L, k, col_offset, merge, d_idx, d_val):
        check(_ffi.lib().pvs_sq8_topk_dev(self.handle, ptr(d_qcodes), ptr(d_invq), int(nq), ptr(d_codes), ptr(d_invdb), int(N), int(L),
                                          int(k), int(col_offset), int(merge), ptr(d_idx), ptr(d_val)))

    # threshold join and pair components
    def cosine_range_dev(self, d_q, nq, d_db, N, L, d_invq, d_invdb, threshold, capacity, d_row, d_col, d_val, flags=0, path=0, tile=0):
        """pvs_cosine_range_dev: every (row, col, score) with score >= threshold into the COO outputs int64 / int64 / float32 of
        `capacity` entries, in the device order of the header.  Waits for the stream.
        -> (total, dict(filtered, redone_exact, rescored, tiles, tiles_skipped)); raises CapacityError (args[1] = the total, args[2] =
        the dict) when the total exceeds the capacity: the entries below the capacity are written then, nothing beyond."""
        total, st = C.c_int64(0), (C.c_int64 * 6)()
        status = _ffi.lib().pvs_cosine_range_dev(self.handle, ptr(d_q), int(nq), ptr(d_db), int(N), int(L), ptr(d_invq), ptr(d_invdb),
                                                 float(threshold), int(flags), int(path), int(tile), int(capacity), ptr(d_row),
                                                 ptr(d_col), ptr(d_val), C.byref(total), st)
        stats = {"filtered": bool(st[0]), "redone_exact": int(st[1]), "rescored": int(st[2]), "tiles": int(st[3]),
                 "tiles_skipped": int(st[4])}
        if status == _ffi.PVS_ERR_CAPACITY:
            raise _ffi.CapacityError(_ffi.lib().pvs_last_error().decode("utf-8", "replace"), int(total.value), stats)
        check(status)
        return int(total.value), stats

    def sq8_range_dev(self, d_qcodes, d_invq, nq, d_codes, d_invdb, N, L, threshold, capacity, d_row, d_col, d_val, flags=0, path=0, tile=0):
        """pvs_sq8_range_dev: every (row, col, score) of the int8 code rows with score >= threshold into the COO outputs int64 / int64 /
        float32 of `capacity` entries, in the device order of the header.  Waits for the stream.
        -> (total, dict(path, pairs_scored, tiles, tiles_skipped)); raises CapacityError (args[1] = the total, args[2] = the dict) when
        the total exceeds the capacity: the entries below the capacity are written then, nothing beyond."""
        total, st = C.c_int64(0), (C.c_int64 * 6)()
        status = _ffi.lib().pvs_sq8_range_dev(self.handle, ptr(d_qcodes), ptr(d_invq), int(nq), ptr(d_codes), ptr(d_invdb), int(N), int(L),
                                              float(threshold), int(flags), int(path), int(tile), int(capacity), ptr(d_row), ptr(d_col),
                                              ptr(d_val), C.byref(total), st)
        stats = {"path": ("auto", "panel", "mask")[int(st[0])] if 0 <= int(st[0]) <= 2 else int(st[0]), "pairs_scored": int(st[2]),
                 "tiles": int(st[3]), "tiles_skipped": int(st[4])}
        if status == _ffi.PVS_ERR_CAPACITY:
            raise _ffi.CapacityError(_ffi.lib().pvs_last_error().decode("utf-8", "replace"), int(total.value), stats)
        check(status)
        return int(total.value), stats

    # subset search
    def subset_create(self, ids: np.ndarray, n: int) -> SubsetHandle:
        """pvs_subset_create: ids int64, strictly ascending within [0, n) (checked there: ValueError) -> the handle that owns the ids
        and the bitmask on the device"""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        h = C.c_void_p()
        check(_ffi.lib().pvs_subset_create(self.handle, ptr(ids), int(ids.size), int(n), C.byref(h)))
        s = SubsetHandle(self, h)
        s.n, s.size = int(n), int(ids.size)
        return s

    @staticmethod
    def _subset_stats(st) -> dict:
        return {"path": ("auto", "mask", "listed")[int(st[0])] if 0 <= int(st[0]) <= 2 else int(st[0]), "scored": int(st[1]),
                "panels_skipped": int(st[2]), "rows_gathered": int(st[3])}

    def cosine_topk_subset_dev(self, d_q, nq, d_db, N, L, d_invq, d_invdb, subset, k, d_idx, d_val, path=0, tile=0) -> dict:
        """pvs_cosine_topk_subset_dev -> dict(path, scored, panels_skipped, rows_gathered)"""
        st = (C.c_int64 * 4)()
        check(_ffi.lib().pvs_cosine_topk_subset_dev(self.handle, ptr(d_q), int(nq), ptr(d_db), int(N), int(L), ptr(d_invq), ptr(d_invdb),
                                                    subset.handle, int(k), int(path), int(tile), ptr(d_idx), ptr(d_val), st))
        return self._subset_stats(st)

    def sq8_topk_subset_dev(self, d_qcodes, d_invq, nq, d_codes, d_invdb, N, L, subset, k, d_idx, d_val, path=0, tile=0) -> dict:
        """pvs_sq8_topk_subset_dev -> dict(path, scored, panels_skipped, rows_gathered)"""
        st = (C.c_int64 * 4)()
        check(_ffi.lib().pvs_sq8_topk_subset_dev(self.handle, ptr(d_qcodes), ptr(d_invq), int(nq), ptr(d_codes), ptr(d_invdb), int(N), int(L),
                                                 subset.handle, int(k), int(path), int(tile), ptr(d_idx), ptr(d_val), st))
        return self._subset_stats(st)

    def pair_components_dev(self, d_a, d_b, E, N, d_label):
        """pvs_pair_components_dev: int64 pair arrays of E entries over N nodes -> d_label int32 (N,), the smallest member of every
        node's component.  Waits for the stream.  -> dict(rounds, components)"""
        st = (C.c_int64 * 2)()
        check(_ffi.lib().pvs_pair_components_dev(self.handle, ptr(d_a), ptr(d_b), int(E), int(N), ptr(d_label), st))
        return {"rounds": int(st[0]), "components": int(st[1])}

    # inverted lists of the compact index
    def ivf_assign_dev(self, d_x, n, d, d_centroids, nlist, d_list, d_residual):
        check(_ffi.lib().pvs_ivf_assign_dev(self.handle, ptr(d_x), n, d, ptr(d_centroids), nlist, ptr(d_list), ptr(d_residual)))

    def ivf_coarse_dev(self, d_q, nq, d, d_centroids, nlist, d_coarse):
        check(_ffi.lib().pvs_ivf_coarse_dev(self.handle, ptr(d_q), nq, d, ptr(d_centroids), nlist, ptr(d_coarse)))

    def ivf_scan_topk_dev(self, d_lut, nq, m, ksub, d_probe, d_probe_val, nprobe, d_list_off, h_list_off, nlist, d_codes, d_ids,
                          d_invq, d_invdb, k, d_idx, d_val):
        """h_list_off: the host copy of the list offsets, a C-contiguous int64 array of nlist + 1 entries"""
        h = np.ascontiguousarray(h_list_off, dtype=np.int64)
        if h.shape != (nlist + 1,):
            raise ValueError(f"h_list_off must have nlist + 1 = {nlist + 1} entries, got shape {h.shape}")
        check(_ffi.lib().pvs_ivf_scan_topk_dev(self.handle, ptr(d_lut), nq, m, ksub, ptr(d_probe), ptr(d_probe_val), nprobe,
                                               ptr(d_list_off), ptr(h), nlist, ptr(d_codes), ptr(d_ids), ptr(d_invq), ptr(d_invdb), k,
                                               ptr(d_idx), ptr(d_val)))

    # inverted lists over the int8 code rows
    def ivf_sq8_scan_topk_dev(self, d_qcodes, d_invq, nq, L, d_probe, nprobe, d_list_off, h_list_off, nlist, d_codes, d_invdb, d_ids, k,
                              d_idx, d_val, slice_rows=0):
        """pvs_ivf_sq8_scan_topk_dev; h_list_off: the host copy of the list offsets, a C-contiguous int64 array of nlist + 1 entries;
        slice_rows: candidate slots per workgroup (0: the host's rule), a test seam that never changes the result"""
        h = np.ascontiguousarray(h_list_off, dtype=np.int64)
        if h.shape != (nlist + 1,):
            raise ValueError(f"h_list_off must have nlist + 1 = {nlist + 1} entries, got shape {h.shape}")
        check(_ffi.lib().pvs_ivf_sq8_scan_topk_dev(self.handle, ptr(d_qcodes), ptr(d_invq), int(nq), int(L), ptr(d_probe), int(nprobe),
                                                   ptr(d_list_off), ptr(h), int(nlist), ptr(d_codes), ptr(d_invdb), ptr(d_ids), int(k),
                                                   int(slice_rows), ptr(d_idx), ptr(d_val)))

    def ivf_sq8_scan_plan(self, nq, nprobe, h_list_off, nlist, slice_rows=0) -> dict:
        """pvs_ivf_sq8_scan_plan -> dict(W, query_block, slice_rows, slices): how the scan above is cut, from the host offsets alone"""
        h = np.ascontiguousarray(h_list_off, dtype=np.int64)
        if h.shape != (nlist + 1,):
            raise ValueError(f"h_list_off must have nlist + 1 = {nlist + 1} entries, got shape {h.shape}")
        out = (C.c_int64 * 4)()
        check(_ffi.lib().pvs_ivf_sq8_scan_plan(self.handle, int(nq), int(nprobe), ptr(h), int(nlist), int(slice_rows), out))
        return {"W": int(out[0]), "query_block": int(out[1]), "slice_rows": int(out[2]), "slices": int(out[3])}

    # the same candidate rows filled by list, for batches of queries
    def ivf_sq8_group_probes_dev(self, d_probe, qn, nprobe, d_list_off, nlist, d_base, d_total, d_goff, d_gq, d_gbase):
        """pvs_ivf_sq8_group_probes_dev: the probes int64 (qn, nprobe) of one query block -> base int32 (qn, nprobe), total int32 (qn,),
        goff int32 (nlist + 1,), and gq, gbase int32 (qn nprobe,) of which the first goff[nlist] entries are written"""
        check(_ffi.lib().pvs_ivf_sq8_group_probes_dev(self.handle, ptr(d_probe), int(qn), int(nprobe), ptr(d_list_off), int(nlist),
                                                      ptr(d_base), ptr(d_total), ptr(d_goff), ptr(d_gq), ptr(d_gbase)))

    def ivf_sq8_scan_lists_topk_dev(self, d_qcodes, d_invq, nq, L, d_probe, nprobe, d_list_off, h_list_off, nlist, d_codes, d_invdb, d_ids,
                                    k, d_idx, d_val, query_block=0):
        """pvs_ivf_sq8_scan_lists_topk_dev: the arguments of ivf_sq8_scan_topk_dev; query_block: queries grouped at a time (0: the
        host's rule), a test seam that never changes the result"""
        h = np.ascontiguousarray(h_list_off, dtype=np.int64)
        if h.shape != (nlist + 1,):
            raise ValueError(f"h_list_off must have nlist + 1 = {nlist + 1} entries, got shape {h.shape}")
        check(_ffi.lib().pvs_ivf_sq8_scan_lists_topk_dev(self.handle, ptr(d_qcodes), ptr(d_invq), int(nq), int(L), ptr(d_probe), int(nprobe),
                                                         ptr(d_list_off), ptr(h), int(nlist), ptr(d_codes), ptr(d_invdb), ptr(d_ids),
                                                         int(k), int(query_block), ptr(d_idx), ptr(d_val)))

    def ivf_sq8_scan_lists_plan(self, nq, nprobe, h_list_off, nlist, query_block=0) -> dict:
        """pvs_ivf_sq8_scan_lists_plan -> dict(W, query_block, row_tiles, pairs): how the scan by list is cut, from the host offsets alone"""
        h = np.ascontiguousarray(h_list_off, dtype=np.int64)
        if h.shape != (nlist + 1,):
            raise ValueError(f"h_list_off must have nlist + 1 = {nlist + 1} entries, got shape {h.shape}")
        out = (C.c_int64 * 4)()
        check(_ffi.lib().pvs_ivf_sq8_scan_lists_plan(self.handle, int(nq), int(nprobe), ptr(h), int(nlist), int(query_block), out))
        return {"W": int(out[0]), "query_block": int(out[1]), "row_tiles": int(out[2]), "pairs": int(out[3])}

    # query expansion / database-side augmentation
    COMBINE_CHUNK_BYTES, COMBINE_BATCH = _ffi.COMBINE_CHUNK_BYTES, _ffi.COMBINE_BATCH

    def combine_rows_dev(self, d_x, N, L, is_f64, d_self, d_w_self, d_idx, d_w, n, r, d_out):
        """pvs_combine_rows_dev: out[i] = w_self[i] self[i] + sum_j w[i][j] X[idx[i][j]] in list order, slots outside [0, N) skipped"""
        check(_ffi.lib().pvs_combine_rows_dev(self.handle, ptr(d_x), N, L, int(bool(is_f64)), ptr(d_self), ptr(d_w_self), ptr(d_idx),
                                              ptr(d_w), n, r, ptr(d_out)))

    # diffusion re-ranking
    def graph_affinity_dev(self, d_idx, d_val, val_f64, b, kg, row0, N, gamma, d_nbr, d_a):
        """pvs_graph_affinity_dev: lists (b, kg + 1) of rows row0.. -> rows row0.. of nbr int32 (N, kg) and a float64 (N, kg)"""
        check(_ffi.lib().pvs_graph_affinity_dev(self.handle, ptr(d_idx), ptr(d_val), int(bool(val_f64)), int(b), int(kg), int(row0), int(N),
                                                int(gamma), ptr(d_nbr), ptr(d_a)))

    def graph_mutual_dev(self, d_nbr, d_a, N, kg, d_w):
        """pvs_graph_mutual_dev: w = min of the two affinities where both rows list each other, +0 elsewhere"""
        check(_ffi.lib().pvs_graph_mutual_dev(self.handle, ptr(d_nbr), ptr(d_a), int(N), int(kg), ptr(d_w)))

    def graph_degrees_dev(self, d_w, N, kg, d_deg, d_r):
        """pvs_graph_degrees_dev: deg = sum of a row's w in slot order, r = 1 / sqrt(deg) (0 where deg = 0)"""
        check(_ffi.lib().pvs_graph_degrees_dev(self.handle, ptr(d_w), int(N), int(kg), ptr(d_deg), ptr(d_r)))

    def graph_normalise_dev(self, d_nbr, d_w, d_r, N, kg, d_s):
        """pvs_graph_normalise_dev: s[i][t] = w[i][t] * (r[i] * r[nbr[i][t]])"""
        check(_ffi.lib().pvs_graph_normalise_dev(self.handle, ptr(d_nbr), ptr(d_w), ptr(d_r), int(N), int(kg), ptr(d_s)))

    def diffuse_rhs_dev(self, d_idx, d_val, val_f64, C_, kq, N, gamma, d_y):
        """pvs_diffuse_rhs_dev: query lists (C, kq) -> Y float64 (N, C), zero except the affinities of the list entries"""
        check(_ffi.lib().pvs_diffuse_rhs_dev(self.handle, ptr(d_idx), ptr(d_val), int(bool(val_f64)), int(C_), int(kq), int(N), int(gamma),
                                             ptr(d_y)))

    def diffuse_cg_dev(self, d_nbr, d_s, N, kg, d_y, C_, alpha, tol, maxiter, check_every, width, d_work, work_bytes, d_x, d_steps, d_rr,
                       d_yy):
        """pvs_diffuse_cg_dev: conjugate gradients on (I - alpha S) x = y for C columns (N, C); steps int32, rr, yy per column"""
        check(_ffi.lib().pvs_diffuse_cg_dev(self.handle, ptr(d_nbr), ptr(d_s), int(N), int(kg), ptr(d_y), int(C_), float(alpha), float(tol),
                                            int(maxiter), int(check_every), int(width), ptr(d_work), int(work_bytes), ptr(d_x), ptr(d_steps),
                                            ptr(d_rr), ptr(d_yy)))

    def rank_f64_dev(self, d_scores, nq, ncols, ld, k, d_idx, d_val):
        """pvs_rank_f64_dev: rows of float64 scores -> the k best columns by (score descending, column ascending, NaN last)"""
        check(_ffi.lib().pvs_rank_f64_dev(self.handle, ptr(d_scores), int(nq), int(ncols), int(ld), int(k), ptr(d_idx), ptr(d_val)))

    # graph maintenance after add / remove
    def graph_lists_dev(self, d_idx, d_val, b, kg, row0, N, d_nbr, d_sim, d_ids=None):
        """pvs_graph_lists_dev: float32 lists (b, kg + 1) of rows row0.. (or of the rows d_ids int64 (b,) names) -> those rows of nbr
        int32 (N, kg) and sim float32 (N, kg): drop self, the similarity kept"""
        check(_ffi.lib().pvs_graph_lists_dev(self.handle, ptr(d_idx), ptr(d_val), int(b), int(kg), int(row0), ptr(d_ids), int(N), ptr(d_nbr),
                                             ptr(d_sim)))

    def graph_merge_dev(self, d_nbr, d_sim, d_cidx, d_cval, rows, kg, c, col_offset, N, d_out_nbr, d_out_sim):
        """pvs_graph_merge_dev: stored lists (rows, kg) + candidates (rows, c) with ids cidx + col_offset -> the first kg of both"""
        check(_ffi.lib().pvs_graph_merge_dev(self.handle, ptr(d_nbr), ptr(d_sim), ptr(d_cidx), ptr(d_cval), int(rows), int(kg), int(c),
                                             int(col_offset), int(N), ptr(d_out_nbr), ptr(d_out_sim)))

    def graph_damage_dev(self, d_nbr, N, kg, d_keep, d_flag):
        """pvs_graph_damage_dev: flag uint8 (N,) = 1 for a kept row that lists a removed one"""
        check(_ffi.lib().pvs_graph_damage_dev(self.handle, ptr(d_nbr), int(N), int(kg), ptr(d_keep), ptr(d_flag)))

    def graph_remap_dev(self, d_nbr, N, kg, d_keep, d_pos, d_out):
        """pvs_graph_remap_dev: the slots of the kept rows through pos (-1 for a removed neighbour); d_out may be d_nbr"""
        check(_ffi.lib().pvs_graph_remap_dev(self.handle, ptr(d_nbr), int(N), int(kg), ptr(d_keep), ptr(d_pos), ptr(d_out)))

    def graph_gather_rows_dev(self, d_rows, n, row_bytes, d_ids, b, d_out):
        """pvs_graph_gather_rows_dev: out[p] = rows[ids[p]] for the b int64 ids (zeros for an id outside [0, n))"""
        check(_ffi.lib().pvs_graph_gather_rows_dev(self.handle, ptr(d_rows), int(n), int(row_bytes), ptr(d_ids), int(b), ptr(d_out)))

    def graph_affinity_sim_dev(self, d_sim, N, kg, gamma, d_a):
        """pvs_graph_affinity_sim_dev: a float64 (N, kg) from the stored float32 similarities, the product of graph_affinity_dev"""
        check(_ffi.lib().pvs_graph_affinity_sim_dev(self.handle, ptr(d_sim), int(N), int(kg), int(gamma), ptr(d_a)))

    # k-reciprocal re-ranking
    def krr_sets_dev(self, d_nbr, N, kg, k1, d_mask1, d_maskh):
        """pvs_krr_sets_dev: nbr int32 (N, kg) -> the reciprocal slots of every row at k1 and at (k1 + 1) // 2, two uint64 (N,)"""
        check(_ffi.lib().pvs_krr_sets_dev(self.handle, ptr(d_nbr), int(N), int(kg), int(k1), ptr(d_mask1), ptr(d_maskh)))

    def krr_members_dev(self, d_nbr, d_mask1, d_maskh, N, kg, d_members, d_dropped):
        """pvs_krr_members_dev: the members of the expanded set that sit in the row's own list, uint8 (N, kg), and the count of those
        that do not, int32 (N,)"""
        check(_ffi.lib().pvs_krr_members_dev(self.handle, ptr(d_nbr), ptr(d_mask1), ptr(d_maskh), int(N), int(kg), ptr(d_members),
                                             ptr(d_dropped)))

    def krr_weights_dev(self, d_sim, d_members, N, kg, gamma, d_v, d_v0):
        """pvs_krr_weights_dev: v float64 (N, kg) and v0 (N,): the members' affinities and the self weight 1 over their sum"""
        check(_ffi.lib().pvs_krr_weights_dev(self.handle, ptr(d_sim), ptr(d_members), int(N), int(kg), int(gamma), ptr(d_v), ptr(d_v0)))

    def krr_expand_dev(self, d_nbr, d_v, d_v0, N, kg, k2, d_w, d_w0, d_ws):
        """pvs_krr_expand_dev: the mean of V over a row and its first k2 - 1 neighbours on the row's support: w (N, kg), w0, ws (N,)"""
        check(_ffi.lib().pvs_krr_expand_dev(self.handle, ptr(d_nbr), ptr(d_v), ptr(d_v0), int(N), int(kg), int(k2), ptr(d_w), ptr(d_w0),
                                            ptr(d_ws)))

    def krr_query_dev(self, d_nbr, d_sim, d_maskh, d_v, d_v0, N, kg, k1, k2, gamma, d_qidx, d_qval, nq, kq, d_wq, d_sq, d_kept, d_dropped):
        """pvs_krr_query_dev: float32 query lists (nq, kq) -> the queries' expanded vectors wq float64 (nq, kq), their sums sq (nq,),
        the members kept and the members dropped, int32 (nq,) both"""
        check(_ffi.lib().pvs_krr_query_dev(self.handle, ptr(d_nbr), ptr(d_sim), ptr(d_maskh), ptr(d_v), ptr(d_v0), int(N), int(kg), int(k1),
                                           int(k2), int(gamma), ptr(d_qidx), ptr(d_qval), int(nq), int(kq), ptr(d_wq), ptr(d_sq),
                                           ptr(d_kept), ptr(d_dropped)))

    def krr_score_dev(self, d_nbr, d_w, d_w0, d_ws, N, kg, d_qidx, d_qval, d_wq, d_sq, nq, kq, kr, lam, d_scores):
        """pvs_krr_score_dev: (1 - lam) Jaccard + lam cosine of the first kr candidates of every query -> float64 (nq, kr)"""
        check(_ffi.lib().pvs_krr_score_dev(self.handle, ptr(d_nbr), ptr(d_w), ptr(d_w0), ptr(d_ws), int(N), int(kg), ptr(d_qidx), ptr(d_qval),
                                           ptr(d_wq), ptr(d_sq), int(nq), int(kq), int(kr), float(lam), ptr(d_scores)))

    # local-descriptor retrieval, ASMK* 
    def asmk_aggregate_dev(self, cb, d_desc, kind, d_offsets, h_offsets, n_images, total_desc, d_labels, d_proj, bits, d_ent_word,
                           d_ent_sig, d_ent_count):
        """pvs_asmk_aggregate_dev: rows + labels -> per image its (word, signature) entries in the slots offsets[i] .. and their
        count.  h_offsets: the host copy of the CSR offsets, int64 (n_images + 1,)"""
        h = np.ascontiguousarray(h_offsets, dtype=np.int64)
        if h.shape != (int(n_images) + 1,):
            raise ValueError(f"h_offsets must have n_images + 1 = {int(n_images) + 1} entries, got shape {h.shape}")
        check(_ffi.lib().pvs_asmk_aggregate_dev(self.handle, cb.handle, ptr(d_desc), int(kind), ptr(d_offsets), ptr(h), int(n_images),
                                                int(total_desc), ptr(d_labels), ptr(d_proj), int(bits), ptr(d_ent_word), ptr(d_ent_sig),
                                                ptr(d_ent_count)))

    def asmk_aggregate_ma_dev(self, cb, d_desc, kind, d_offsets, h_offsets, n_images, total_desc, d_labels, m, d_proj, bits, d_ent_word,
                              d_ent_sig, d_ent_count):
        """pvs_asmk_aggregate_ma_dev: rows + m distinct labels per row (d_labels int32 (total, m)) -> per image its entries in the
        slots m * offsets[i] .. of arrays sized m * total_desc, and their count"""
        h = np.ascontiguousarray(h_offsets, dtype=np.int64)
        if h.shape != (int(n_images) + 1,):
            raise ValueError(f"h_offsets must have n_images + 1 = {int(n_images) + 1} entries, got shape {h.shape}")
        check(_ffi.lib().pvs_asmk_aggregate_ma_dev(self.handle, cb.handle, ptr(d_desc), int(kind), ptr(d_offsets), ptr(h), int(n_images),
                                                   int(total_desc), ptr(d_labels), int(m), ptr(d_proj), int(bits), ptr(d_ent_word),
                                                   ptr(d_ent_sig), ptr(d_ent_count)))

    def asmk_score_dev(self, nq, h_q_off, d_q_word, d_q_sig, bits, K, d_word_off, d_ent_img, d_ent_sig, N, d_wt, d_sel, d_gamma_q,
                       d_gamma_db, d_scores, ld, slice_images=0):
        """pvs_asmk_score_dev: the entries of nq queries x the inverted file -> the score panel (nq, ld), columns < N written.
        h_q_off: host int64 (nq + 1,), the entry offsets of the queries"""
        h = np.ascontiguousarray(h_q_off, dtype=np.int64)
        if h.shape != (int(nq) + 1,):
            raise ValueError(f"h_q_off must have nq + 1 = {int(nq) + 1} entries, got shape {h.shape}")
        check(_ffi.lib().pvs_asmk_score_dev(self.handle, int(nq), ptr(h), ptr(d_q_word), ptr(d_q_sig), int(bits), int(K), ptr(d_word_off),
                                            ptr(d_ent_img), ptr(d_ent_sig), int(N), ptr(d_wt), ptr(d_sel), ptr(d_gamma_q),
                                            ptr(d_gamma_db), int(slice_images), ptr(d_scores), int(ld)))

    # ASMK maintenance
    def asmk_invert_dev(self, K, bits, d_offsets, h_offsets, n_images, d_ent_count, d_ent_word, d_ent_sig, img_base, d_word_off,
                        d_out_img, d_out_sig, tile_entries=0):
        """pvs_asmk_invert_dev: the slots pvs_asmk_aggregate_dev filled -> word_off int64 (K + 1,), and ent_img / ent_sig sorted by
        (word, image) in arrays sized by the slots; image i carries img_base + i.  h_offsets: host int64 (n_images + 1,)"""
        h = np.ascontiguousarray(h_offsets, dtype=np.int64)
        if h.shape != (int(n_images) + 1,):
            raise ValueError(f"h_offsets must have n_images + 1 = {int(n_images) + 1} entries, got shape {h.shape}")
        check(_ffi.lib().pvs_asmk_invert_dev(self.handle, int(K), int(bits), ptr(d_offsets), ptr(h), int(n_images), ptr(d_ent_count),
                                             ptr(d_ent_word), ptr(d_ent_sig), int(img_base), int(tile_entries), ptr(d_word_off),
                                             ptr(d_out_img), ptr(d_out_sig)))

    def asmk_weight_sums_dev(self, K, d_offsets, h_offsets, n_images, d_ent_count, d_ent_word, d_wt, d_sums):
        """pvs_asmk_weight_sums_dev: sums int64 (n_images,), the sum of 1023 wt[w] over each image's entries in the same slots"""
        h = np.ascontiguousarray(h_offsets, dtype=np.int64)
        if h.shape != (int(n_images) + 1,):
            raise ValueError(f"h_offsets must have n_images + 1 = {int(n_images) + 1} entries, got shape {h.shape}")
        check(_ffi.lib().pvs_asmk_weight_sums_dev(self.handle, int(K), ptr(d_offsets), ptr(h), int(n_images), ptr(d_ent_count),
                                                  ptr(d_ent_word), ptr(d_wt), ptr(d_sums)))

    def asmk_insert_dev(self, K, bits, d_word_off, h_word_off, d_ent_img, d_ent_sig, d_new_off, h_new_off, d_new_img, d_new_sig,
                        d_out_word_off, d_out_img, d_out_sig):
        """pvs_asmk_insert_dev: a stored file + an inverted batch of larger ids -> the merged file in distinct buffers.  h_word_off,
        h_new_off: the host copies of the two offset arrays, int64 (K + 1,)"""
        h, hn = np.ascontiguousarray(h_word_off, dtype=np.int64), np.ascontiguousarray(h_new_off, dtype=np.int64)
        if h.shape != (int(K) + 1,) or hn.shape != (int(K) + 1,):
            raise ValueError(f"h_word_off and h_new_off must have K + 1 = {int(K) + 1} entries, got shapes {h.shape}, {hn.shape}")
        check(_ffi.lib().pvs_asmk_insert_dev(self.handle, int(K), int(bits), ptr(d_word_off), ptr(h), ptr(d_ent_img), ptr(d_ent_sig),
                                             ptr(d_new_off), ptr(hn), ptr(d_new_img), ptr(d_new_sig), ptr(d_out_word_off), ptr(d_out_img),
                                             ptr(d_out_sig)))

    def asmk_remove_dev(self, K, bits, N, d_word_off, h_word_off, d_ent_img, d_ent_sig, d_keep, d_pos, d_out_word_off, d_out_img,
                        d_out_sig):
        """pvs_asmk_remove_dev: keep uint8 (N,) and pos int64 (N + 1,) by image id -> the surviving entries, renumbered, in distinct
        buffers.  h_word_off: the host copy of the offsets, int64 (K + 1,)"""
        h = np.ascontiguousarray(h_word_off, dtype=np.int64)
        if h.shape != (int(K) + 1,):
            raise ValueError(f"h_word_off must have K + 1 = {int(K) + 1} entries, got shape {h.shape}")
        check(_ffi.lib().pvs_asmk_remove_dev(self.handle, int(K), int(bits), int(N), ptr(d_word_off), ptr(h), ptr(d_ent_img),
                                             ptr(d_ent_sig), ptr(d_keep), ptr(d_pos), ptr(d_out_word_off), ptr(d_out_img), ptr(d_out_sig)))

    # ASMK query expansion
    def asmk_expand_dev(self, nq, h_q_off, d_q_word, d_q_sig, bits, K, d_word_off, d_ent_img, d_ent_sig, N, R, d_members, d_votes,
                        query_vote, h_max, min_support, d_wt, cap, d_out_word, d_out_sig, d_out_count, d_out_sum, tile_words=0):
        """pvs_asmk_expand_dev: the entries of nq queries, refined and extended by the entries of their members (int32 (nq, R) ids
        ascending, -1 padded, with votes) -> out_word int32 (nq, cap), out_sig uint32 (nq, cap, bits / 32), the true count int32
        (nq,) and weight sum int64 (nq,).  h_q_off: host int64 (nq + 1,)"""
        h = np.ascontiguousarray(h_q_off, dtype=np.int64)
        if h.shape != (int(nq) + 1,):
            raise ValueError(f"h_q_off must have nq + 1 = {int(nq) + 1} entries, got shape {h.shape}")
        check(_ffi.lib().pvs_asmk_expand_dev(self.handle, int(nq), ptr(h), ptr(d_q_word), ptr(d_q_sig), int(bits), int(K), ptr(d_word_off),
                                             ptr(d_ent_img), ptr(d_ent_sig), int(N), int(R), ptr(d_members), ptr(d_votes), int(query_vote),
                                             int(h_max), int(min_support), ptr(d_wt), int(tile_words), int(cap), ptr(d_out_word),
                                             ptr(d_out_sig), ptr(d_out_count), ptr(d_out_sum)))

    # index maintenance
    SCAN_TILE = _ffi.SCAN_TILE

    def copy_dev(self, d_dst, d_src, nbytes):
        check(_ffi.lib().pvs_copy_dev(self.handle, ptr(d_dst), ptr(d_src), int(nbytes)))

    def keep_mask_dev(self, d_removed, r, n, d_keep):
        """pvs_keep_mask_dev: keep[i] = 1 for i < n, then 0 at the r int64 indices of d_removed"""
        check(_ffi.lib().pvs_keep_mask_dev(self.handle, ptr(d_removed), int(r), int(n), ptr(d_keep)))

    def keep_positions_dev(self, d_keep, n, d_pos):
        """pvs_keep_positions_dev: pos int64 (n + 1,), pos[i] = kept entries before i, pos[n] = the total"""
        check(_ffi.lib().pvs_keep_positions_dev(self.handle, ptr(d_keep), int(n), ptr(d_pos)))

    def compact_rows_dev(self, d_rows, n, row_bytes, d_keep, d_pos, d_out, first=0):
        """pvs_compact_rows_dev: out[pos[i]] = rows[i] for kept i; d_out == d_rows compacts in place, leaving rows [0, first) alone"""
        check(_ffi.lib().pvs_compact_rows_dev(self.handle, ptr(d_rows), int(n), int(row_bytes), ptr(d_keep), ptr(d_pos), int(first),
                                              ptr(d_out)))

    def ivf_insert_dev(self, m, nlist, d_codes, d_inv, d_ids, d_list_off, h_list_off, d_new_codes, d_new_inv, d_new_off, h_new_off,
                       d_perm, d_out_codes, d_out_inv, d_out_ids, d_out_list_off):
        """h_list_off, h_new_off: the host copies of the two offset arrays, C-contiguous int64 of nlist + 1 entries"""
        h, hn = np.ascontiguousarray(h_list_off, dtype=np.int64), np.ascontiguousarray(h_new_off, dtype=np.int64)
        if h.shape != (nlist + 1,) or hn.shape != (nlist + 1,):
            raise ValueError(f"h_list_off and h_new_off must have nlist + 1 = {nlist + 1} entries, got shapes {h.shape}, {hn.shape}")
        check(_ffi.lib().pvs_ivf_insert_dev(self.handle, int(m), int(nlist), ptr(d_codes), ptr(d_inv), ptr(d_ids), ptr(d_list_off), ptr(h),
                                            ptr(d_new_codes), ptr(d_new_inv), ptr(d_new_off), ptr(hn), ptr(d_perm), ptr(d_out_codes),
                                            ptr(d_out_inv), ptr(d_out_ids), ptr(d_out_list_off)))

    def ivf_remove_dev(self, m, nlist, n, d_codes, d_inv, d_ids, d_list_off, d_keep, d_pos, d_out_codes, d_out_inv, d_out_ids,
                       d_out_list_off):
        check(_ffi.lib().pvs_ivf_remove_dev(self.handle, int(m), int(nlist), int(n), ptr(d_codes), ptr(d_inv), ptr(d_ids), ptr(d_list_off),
                                            ptr(d_keep), ptr(d_pos), ptr(d_out_codes), ptr(d_out_inv), ptr(d_out_ids),
                                            ptr(d_out_list_off)))

    def f32_to_f16_dev(self, d_src, n, d_dst):
        check(_ffi.lib().pvs_f32_to_f16_dev(self.handle, ptr(d_src), n, ptr(d_dst)))

    def cosine_f16_dev(self, d_a, M, d_b, N, L, d_inva, d_invb, d_out, ldo):
        check(_ffi.lib().pvs_cosine_f16_dev(self.handle, ptr(d_a), M, ptr(d_b), N, L, ptr(d_inva), ptr(d_invb), ptr(d_out), ldo))

    def cosine_topk_f16_dev(self, d_q, nq, d_db, N, L, d_invq, d_invdb, k, col_offset, merge, d_idx, d_val):
        check(_ffi.lib().pvs_cosine_topk_f16_dev(self.handle, ptr(d_q), nq, ptr(d_db), N, L, ptr(d_invq), ptr(d_invdb), k,
                                                 col_offset, int(merge), ptr(d_idx), ptr(d_val)))

    def row_inv_norms_f64_dev(self, d_x, rows, L, d_inv):
        check(_ffi.lib().pvs_row_inv_norms_f64_dev(self.handle, ptr(d_x), rows, L, ptr(d_inv)))

    def cosine_f64_dev(self, d_a, M, d_b, N, L, d_inva, d_invb, d_out, ldo):
        """float64 operands and scores on the f64 matrix pipe (the reference's dtype for Fisher encodings)"""
        check(_ffi.lib().pvs_cosine_f64_dev(self.handle, ptr(d_a), M, ptr(d_b), N, L, ptr(d_inva), ptr(d_invb), ptr(d_out), ldo))

    def cosine_topk_f64_dev(self, d_q, nq, d_db, N, L, d_invq, d_invdb, k, d_idx, d_val):
        """float64 scores + ranking, everything resident: d_idx int64 [nq][k], d_val float64 [nq][k]"""
        check(_ffi.lib().pvs_cosine_topk_f64_dev(self.handle, ptr(d_q), nq, ptr(d_db), N, L, ptr(d_invq), ptr(d_invdb), int(k),
                                                 ptr(d_idx), ptr(d_val)))

    def topk_merge_dev(self, d_idx_lists, d_val_lists, n_lists, nq, k, d_idx, d_val):
        check(_ffi.lib().pvs_topk_merge_dev(self.handle, ptr(d_idx_lists), ptr(d_val_lists), n_lists, nq, k, ptr(d_idx),
                                            ptr(d_val)))

    # ------------------------------------------------------------------ image clustering (neighbors.hip)
    def l2_knn_dev(self, d_q, nq, d_x, N, L, is_f64, k, d_idx, d_sqdist, stats=False):
        """Exact Euclidean k nearest rows: d_idx int64 [nq][k], d_sqdist float64 [nq][k] (squared distances, sklearn's
        float64 value and order).  Synchronises.  stats=True -> dict(filtered, overflowed, candidates, slots) (one more host
        synchronisation per query tile to count the candidates); otherwise None."""
        st = (C.c_int64 * 4)() if stats else None
        check(_ffi.lib().pvs_l2_knn_dev(self.handle, ptr(d_q), nq, ptr(d_x), N, L, int(is_f64), int(k), ptr(d_idx),
                                        ptr(d_sqdist), st))
        if not stats:
            return None
        return {"filtered": bool(st[0]), "overflowed": int(st[1]), "candidates": int(st[2]), "slots": int(st[3])}

    def l2_radius_count_dev(self, d_q, nq, d_x, N, L, is_f64, r_sq, d_counts):
        check(_ffi.lib().pvs_l2_radius_count_dev(self.handle, ptr(d_q), nq, ptr(d_x), N, L, int(is_f64), float(r_sq),
                                                 ptr(d_counts)))

    def l2_radius_fill_dev(self, d_q, nq, d_x, N, L, is_f64, r_sq, d_indptr, d_indices, d_sqdist=None):
        check(_ffi.lib().pvs_l2_radius_fill_dev(self.handle, ptr(d_q), nq, ptr(d_x), N, L, int(is_f64), float(r_sq),
                                                ptr(d_indptr), ptr(d_indices), ptr(d_sqdist)))

    def csr_spmm_f64_dev(self, n, d_indptr, d_indices, d_data, d_x, m, d_y, alpha=1.0, d_beta=None, d_z=None, gamma=0.0):
        """Y = alpha S X + X diag(beta) + gamma Z (float64; S n x n CSR, X / Z / Y (n, m))"""
        check(_ffi.lib().pvs_csr_spmm_f64_dev(self.handle, n, ptr(d_indptr), ptr(d_indices), ptr(d_data), ptr(d_x), int(m),
                                              float(alpha), ptr(d_beta), ptr(d_z), float(gamma), ptr(d_y)))

    def transpose_f64_dev(self, d_src, rows, cols, d_dst):
        check(_ffi.lib().pvs_transpose_f64_dev(self.handle, ptr(d_src), rows, cols, ptr(d_dst)))

    # ------------------------------------------------------------------ dense SIFT (dsift.hip)
    @staticmethod
    def _image_args(hw, pix_offsets):
        hw = np.ascontiguousarray(hw, dtype=np.int32).reshape(-1, 2)
        return hw, None if pix_offsets is None else np.ascontiguousarray(pix_offsets, dtype=np.int64)

    def dsift_dev(self, d_pixels, pixel_kind, hw, pix_offsets, step, sizes, contrast_threshold, out_kind, d_out, out_rows,
                  d_row_offsets):
        """pvs_dsift_dev: hw host int32 (B, 2), pix_offsets host int64 (B,) or None, sizes host int32; everything else device."""
        hw, po = self._image_args(hw, pix_offsets)
        sizes = np.ascontiguousarray(sizes, dtype=np.int32)
        check(_ffi.lib().pvs_dsift_dev(self.handle, ptr(d_pixels), int(pixel_kind), ptr(hw), ptr(po), hw.shape[0], int(step),
                                       ptr(sizes), sizes.shape[0], float(contrast_threshold), int(out_kind), ptr(d_out),
                                       int(out_rows), ptr(d_row_offsets)))

    # ------------------------------------------------------------------ keypoint SIFT (sift.hip)
    def sift_dev(self, d_pixels, pixel_kind, hw, pix_offsets, nfeatures, n_octave_layers, contrast_threshold, edge_threshold, sigma,
                 upsample, out_kind, d_rows, capacity_rows, d_frames, d_row_offsets) -> int:
        """pvs_sift_dev: hw host int32 (B, 2), pix_offsets host int64 (B,) or None; rows, frames (or None) and row offsets on the
        device.  Waits for the stream.  -> total rows; raises CapacityError (args[1] = the total) when they exceed capacity_rows."""
        hw, po = self._image_args(hw, pix_offsets)
        total = C.c_int64(0)
        status = _ffi.lib().pvs_sift_dev(self.handle, ptr(d_pixels), int(pixel_kind), ptr(hw), ptr(po), hw.shape[0], int(nfeatures),
                                         int(n_octave_layers), float(contrast_threshold), float(edge_threshold), float(sigma),
                                         int(bool(upsample)), int(out_kind), ptr(d_rows), int(capacity_rows), ptr(d_frames),
                                         ptr(d_row_offsets), C.byref(total))
        if status == _ffi.PVS_ERR_CAPACITY:
            raise _ffi.CapacityError(_ffi.lib().pvs_last_error().decode("utf-8", "replace"), int(total.value))
        check(status)
        return int(total.value)

    # ------------------------------------------------------------------ spatial re-ranking (match.hip)
    @staticmethod
    def _pair_args(off_a, off_b, pairs):
        off_a = np.ascontiguousarray(off_a, dtype=np.int64).reshape(-1)
        off_b = np.ascontiguousarray(off_b, dtype=np.int64).reshape(-1)
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        if off_a.size < 1 or off_b.size < 1:
            raise ValueError("CSR offsets need at least one entry")
        return off_a, off_b, pairs

    def match_u8_dev(self, d_rows_a, off_a, d_rows_b, off_b, pairs, d_idx, d_d1, d_d2):
        """pvs_match_u8_dev: uint8 rows on the device, host int64 CSR offsets, host int32 pairs (P, 2); int32 results per A row."""
        off_a, off_b, pairs = self._pair_args(off_a, off_b, pairs)
        check(_ffi.lib().pvs_match_u8_dev(self.handle, ptr(d_rows_a), ptr(off_a), off_a.size - 1, ptr(d_rows_b), ptr(off_b),
                                          off_b.size - 1, ptr(pairs), pairs.shape[0], ptr(d_idx), ptr(d_d1), ptr(d_d2)))

    def match_filter_dev(self, off_a, off_b, pairs, d_idx, d_d1, d_d2, d_idx_rev, ratio_sq, mutual, d_matches, d_match_counts):
        """pvs_match_filter_dev: ratio test (d1 < ratio_sq d2 in float64), mutual check against the transposed matching, compaction."""
        off_a, off_b, pairs = self._pair_args(off_a, off_b, pairs)
        check(_ffi.lib().pvs_match_filter_dev(self.handle, ptr(off_a), off_a.size - 1, ptr(off_b), off_b.size - 1, ptr(pairs),
                                              pairs.shape[0], ptr(d_idx), ptr(d_d1), ptr(d_d2), ptr(d_idx_rev), float(ratio_sq),
                                              int(bool(mutual)), ptr(d_matches), ptr(d_match_counts)))

    def verify_dev(self, d_frames_a, off_a, d_frames_b, off_b, pairs, d_matches, d_match_counts, tol, refine_rounds, d_inliers,
                   d_models, d_best, d_mask):
        """pvs_verify_dev: exhaustive similarity hypotheses + affine refinement in float64, one result per pair."""
        off_a, off_b, pairs = self._pair_args(off_a, off_b, pairs)
        check(_ffi.lib().pvs_verify_dev(self.handle, ptr(d_frames_a), ptr(off_a), off_a.size - 1, ptr(d_frames_b), ptr(off_b),
                                        off_b.size - 1, ptr(pairs), pairs.shape[0], ptr(d_matches), ptr(d_match_counts), float(tol),
                                        int(refine_rounds), ptr(d_inliers), ptr(d_models), ptr(d_best), ptr(d_mask)))

    # ------------------------------------------------------------------ vocabulary training (one device pass each)
    def buffer(self, nbytes: int) -> "DeviceBuffer":
        return DeviceBuffer(self, nbytes)

    def scratch(self) -> _Scratch:
        """`with ctx.scratch() as tmp:` -- device temporaries that are freed when the block ends (see _Scratch)"""
        return _Scratch(self)

    def materialise_dev(self, d_desc, kind, D, total_desc, d_out):
        check(_ffi.lib().pvs_materialise_dev(self.handle, ptr(d_desc), kind, D, total_desc, ptr(d_out)))

    def kmeans_step_dev(self, cb, d_x, total_desc, d_labels, d_prev_labels=None, d_sqdist=None):
        """-> (residual sums (K, D) f64, counts (K,) f64, inertia, changed labels)"""
        K, D = cb.K, cb.D
        st = np.empty(K * D + K + 2, dtype=np.float64)
        check(_ffi.lib().pvs_kmeans_step_dev(self.handle, cb.handle, ptr(d_x), total_desc, ptr(d_labels), ptr(d_prev_labels),
                                             ptr(st), ptr(d_sqdist)))
        return st[:K * D].reshape(K, D), st[K * D:K * D + K], float(st[K * D + K]), int(st[K * D + K + 1])

    def gmm_em_step_dev(self, g, d_x, total_desc):
        """-> (s0 (K,), s1 (K, D), s2 (K, D), sum_i log p(x_i)), all fp64"""
        K, D = g.K, g.D
        st = np.empty(K + 2 * K * D + 1, dtype=np.float64)
        check(_ffi.lib().pvs_gmm_em_step_dev(self.handle, g.handle, ptr(d_x), total_desc, ptr(st)))
        s12 = st[K:K + 2 * K * D].reshape(K, 2, D)
        return st[:K], s12[:, 0, :], s12[:, 1, :], float(st[-1])

    def gram_dev(self, d_x, D, total_desc):
        """-> (sum_i x_i (D,), sum_i x_i x_i^T (D, D)) in fp64"""
        out = np.empty(D + D * D, dtype=np.float64)
        check(_ffi.lib().pvs_gram_dev(self.handle, ptr(d_x), D, total_desc, ptr(out)))
        return out[:D], out[D:].reshape(D, D)

    def label_sums_dev(self, d_x, D, total_desc, d_labels, K, square=False):
        out = np.empty((K, D), dtype=np.float64)
        check(_ffi.lib().pvs_label_sums_dev(self.handle, ptr(d_x), D, total_desc, ptr(d_labels), K, int(square), ptr(out)))
        return out

    def seed_distances_dev(self, d_x, D, total_desc, cand, d_mind, d_dist, n_cand=None):
        """cand: host (n_cand, D) array, or a raw device pointer (int) together with n_cand"""
        on_dev = not isinstance(cand, np.ndarray)
        if not on_dev:
            cand = np.ascontiguousarray(cand, dtype=np.float32).reshape(-1, D)
            n_cand = cand.shape[0]
        pot = np.empty(n_cand, dtype=np.float64)
        check(_ffi.lib().pvs_seed_distances_dev(self.handle, ptr(d_x), D, total_desc, ptr(cand), n_cand, ptr(d_mind),
                                                ptr(d_dist), ptr(pot), int(on_dev)))
        return pot

    def seed_pick_dev(self, d_x, D, total_desc, d_mind, blocks, base, target, d_cand):
        blocks = np.ascontiguousarray(blocks, dtype=np.int64)
        base = np.ascontiguousarray(base, dtype=np.float64)
        target = np.ascontiguousarray(target, dtype=np.float64)
        idx = np.empty(len(blocks), dtype=np.int64)
        check(_ffi.lib().pvs_seed_pick_dev(self.handle, ptr(d_x), D, total_desc, ptr(d_mind), ptr(blocks), ptr(base), ptr(target),
                                           len(blocks), ptr(d_cand), ptr(idx)))
        return idx

    def min_update_dev(self, d_mind, d_dist, total_desc):
        bs = np.empty((total_desc + 4095) // 4096, dtype=np.float64)
        check(_ffi.lib().pvs_min_update_dev(self.handle, ptr(d_mind), ptr(d_dist), total_desc, ptr(bs)))
        return bs

    def kmeanspp_run_dev(self, d_x, D, total_desc, n_clusters, trials, uniform, first_index):
        """pvs_kmeanspp_run_dev: the greedy k-means++ run on the device (trials <= 8) -> indices (n_clusters,) int64."""
        u = np.ascontiguousarray(uniform, dtype=np.float64).reshape(-1)
        if u.size < max(n_clusters - 1, 0) * trials:
            raise ValueError("need (n_clusters - 1) x trials uniform numbers")
        idx = np.full(n_clusters, -1, dtype=np.int64)
        idx[0] = first_index
        if u.size == 0:
            u = np.zeros(1)
        check(_ffi.lib().pvs_kmeanspp_run_dev(self.handle, ptr(d_x), D, total_desc, n_clusters, trials, ptr(u), ptr(idx)))
        return idx

    def fused_profile(self, enable=True, raw=False):
        """pvs_fused_profile: (re)start or stop the stamped diagnostic builds of the VLAD encode kernels -> the 16 counters so far
        (fused path: the names below; two-kernel path with raw=True: the prefilter's phase cycles, see tests/tools/assign_profile.py)."""
        out = np.zeros(16, dtype=np.int64)
        check(_ffi.lib().pvs_fused_profile(self.handle, int(enable), ptr(out)))
        if raw:
            return out
        names = ("P0", "A", "reduce", "reevaluate", "K2", "epilogue", "image_switch", "_", "stages", "stages_reevaluated", "entries", "rows_unsettled")
        return {n: int(v) for n, v in zip(names, out) if n != "_"}

    # ------------------------------------------------------------------ timers
    def timers_enable(self, on=True):
        check(_ffi.lib().pvs_timers_enable(self.handle, int(on)))

    def timers_reset(self):
        check(_ffi.lib().pvs_timers_reset(self.handle))

    def timers(self) -> dict:
        out = {}
        for i, name in enumerate(_ffi.TIMER_NAMES):
            ms, cnt = C.c_double(), C.c_int64()
            check(_ffi.lib().pvs_timers_read(self.handle, i, C.byref(ms), C.byref(cnt)))
            out[name] = (ms.value, cnt.value)
        return out


_default = None
_default_lock = threading.Lock()


def default_context() -> Context:
    """Process-wide context on device LOCAL_RANK (0 if unset); created on first use."""
    global _default
    if _default is None or _default.handle is None:
        with _default_lock:
            if _default is None or _default.handle is None:
                _default = Context(int(os.environ.get("PVSIM_DEVICE", os.environ.get("LOCAL_RANK", "0"))))
    return _default
