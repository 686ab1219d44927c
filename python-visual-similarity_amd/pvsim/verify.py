"""Spatial re-ranking: local-descriptor matching and geometric verification on the MI355X.

The second stage of instance retrieval (Lowe 2004 section 7; Philbin et al. 2007, "fast spatial matching"): take the shortlist a
global descriptor gives, match the local descriptors of the query against each candidate, fit a transform to the matches and
re-order the shortlist by the number of inliers.

    index = LocalFeatureIndex.from_images(paths)                 # uint8 rows + frames of the database, resident on the device
    verifier = SpatialVerifier()
    hits = eval.retrieve_top_k_similar(query, encodings, encoder, k=100)
    ranked = eval.rerank_spatial(query, hits, index, verifier)   # [(path, similarity, inliers)]

Three device stages (csrc/match.hip) serve a whole shortlist with one call each: exact 2-NN matching of uint8 rows on the int8
matrix pipe, the ratio / mutual filter, and an exhaustive, deterministic float64 verification (every match is a similarity
hypothesis from its two frames; least-squares affine refinement).  `match` is the OpenCV-free counterpart of
`BFMatcher.knnMatch(k=2)` plus Lowe's ratio test for two host arrays.  No arithmetic happens in Python."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

__all__ = ["LocalFeatureIndex", "SpatialVerifier", "Verification", "match", "DEFAULT_TOL"]

# Absolute distance in pixels of the B (candidate) image.  Chosen with the NumPy twin (tests/match_numpy.py) on planted
# similarities (scale 1.37, rotation 33 degrees, position noise sigma 0.7 px, 2 % size and 1.5 degree angle noise, up to 60 %
# outliers): a hypothesis comes from ONE match, so its scale / angle noise grows with the distance from its anchor (2 % and 1.5
# degrees are ~10 px at 300 px); 12 px lets the best hypothesis collect most of the planted set while random matches stay in the
# single digits, and the refinement then fits the whole set.
DEFAULT_TOL = 12.0

Verification = namedtuple("Verification", "inliers model matches frames_a frames_b mask best")
Verification.__doc__ = """Result of verifying one image pair: inliers (int), model (2, 3) float64 with p_b ~ model @ (x_a, y_a, 1),
matches (m, 2) int32 rows (i in A, j in B), frames_a / frames_b (m, 6) float32 the matched frames, mask (m,) bool the inliers,
best the index of the winning hypothesis (-1: none)."""


def _check_ratio(ratio):
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float, np.integer, np.floating)) or not (0.0 < float(ratio) <= 1.0):
        raise ValueError(f"ratio must be a number in (0, 1], got {ratio!r}")
    return float(ratio)


def _check_bool(name, v):
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError(f"{name} must be a bool, got {v!r}")
    return bool(v)


def _u8_rows(name, a):
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 2 or a.shape[1] != 128:
        raise ValueError(f"{name} must be a (n, 128) uint8 array, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


class LocalFeatureIndex:
    """uint8 descriptor rows (n, 128), frames (x, y, size, angle, response, octave) and the CSR offsets of a set of images, resident
    on the device, with a path <-> position map.

    Matching is Euclidean on the raw uint8 rows of either extractor (KeypointSIFT and KeypointRootSIFT write the same rows).
    Matching in Hellinger / RootSIFT space is out of scope: it would need its own quantisation definition of the square-rooted
    rows; the ratio test on raw rows is Lowe's original."""

    def __init__(self, ctx, rows, frames, offsets, paths):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        paths = list(paths)
        if offsets.size != len(paths) + 1:
            raise ValueError(f"{len(paths)} paths need {len(paths) + 1} offsets, got {offsets.size}")
        if len(set(paths)) != len(paths):
            raise ValueError("paths must be unique")
        self.ctx, self.rows, self.frames, self.offsets, self.paths = ctx, rows, frames, offsets, paths
        self._pos = {p: i for i, p in enumerate(paths)}
        self._host_frames = None

    # -------------------------------------------------------------------------------------------------- construction
    @classmethod
    def from_arrays(cls, rows_list, frames_list, paths=None, ctx=None) -> "LocalFeatureIndex":
        """From host arrays: per image (n_i, 128) uint8 rows and (n_i, 6) float32 frames."""
        from .engine import default_context
        ctx = ctx if ctx is not None else default_context()
        rows_list = [_u8_rows("rows", r) for r in rows_list]
        frames_list = [np.ascontiguousarray(f, dtype=np.float32).reshape(-1, 6) for f in frames_list]
        if len(rows_list) != len(frames_list) or any(len(r) != len(f) for r, f in zip(rows_list, frames_list)):
            raise ValueError("rows and frames must pair up image by image and row by row")
        paths = list(range(len(rows_list))) if paths is None else list(paths)
        off = np.zeros(len(rows_list) + 1, np.int64)
        np.cumsum([len(r) for r in rows_list], out=off[1:])
        total = int(off[-1])
        rows = ctx.buffer(max(total, 1) * 128)
        frames = ctx.buffer(max(total, 1) * 24)
        if total:
            rows.upload(np.concatenate(rows_list))
            frames.upload(np.concatenate(frames_list))
        return cls(ctx, rows, frames, off, paths)

    @classmethod
    def from_images(cls, images_or_paths, extractor=None, batch: int = 16, paths=None, ctx=None) -> "LocalFeatureIndex":
        """Extract `batch` images at a time with `extractor.device_descriptors(..., out_kind=DSIFT_U8, frames=True)` (default
        KeypointRootSIFT(nfeatures=2000)) and keep everything on the device.  Items may be images (ndarray) or paths; `paths`
        names the images (default: the path strings, or 0..N-1)."""
        from ._ffi import DSIFT_U8
        from .encoders._base_encoder import _image_chunks
        from .features import KeypointRootSIFT
        if isinstance(batch, bool) or int(batch) != batch or batch < 1:
            raise ValueError(f"batch must be a positive integer, got {batch!r}")
        items = list(images_or_paths)
        if not items:
            raise ValueError("need at least one image")
        if paths is None:
            paths = [it if isinstance(it, str) else i for i, it in enumerate(items)]
        paths = list(paths)
        if len(paths) != len(items):
            raise ValueError(f"{len(items)} images but {len(paths)} paths")
        extractor = extractor if extractor is not None else KeypointRootSIFT(nfeatures=2000)
        if not hasattr(extractor, "device_descriptors"):
            raise ValueError("the extractor must provide device_descriptors(..., frames=True) (KeypointSIFT / KeypointRootSIFT)")
        ctx = ctx if ctx is not None else extractor.context
        parts, counts = [], []
        try:
            for s in range(0, len(items), int(batch)):
                chunk = [_load(it) for it in items[s:s + int(batch)]]
                for run in _image_chunks(chunk, int(batch), float("inf")):      # gray and colour runs: one kind per launch
                    got = extractor.device_descriptors(run, ctx, DSIFT_U8, frames=True)
                    got[1].free()
                    parts.append((got[0], got[6], int(got[3])))
                    counts.extend(np.diff(got[5]).tolist())
            off = np.zeros(len(items) + 1, np.int64)
            np.cumsum(counts, out=off[1:])
            total = int(off[-1])
            rows, frames = ctx.buffer(max(total, 1) * 128), ctx.buffer(max(total, 1) * 24)
        except Exception:
            for r, f, _ in parts:
                r.free()
                f.free()
            raise
        at = 0
        for r, f, n in parts:                 # gather the batches into one block each (device -> device through the host API)
            if n:
                rows.upload(r.download((n, 128), np.uint8), at * 128)
                frames.upload(f.download((n, 6), np.float32), at * 24)
            at += n
            r.free()
            f.free()
        return cls(ctx, rows, frames, off, paths)

    # -------------------------------------------------------------------------------------------------- access
    def __len__(self) -> int:
        return len(self.paths)

    def __contains__(self, path) -> bool:
        return path in self._pos

    def position(self, path) -> int:
        """Position of `path`; KeyError if the index does not hold it."""
        return self._pos[path]

    @property
    def total_rows(self) -> int:
        return int(self.offsets[-1])

    def count(self, path) -> int:
        i = self._pos[path]
        return int(self.offsets[i + 1] - self.offsets[i])

    def rows_of(self, path) -> np.ndarray:
        """(n, 128) uint8 rows of one image (downloaded)."""
        i = self._pos[path]
        lo, hi = int(self.offsets[i]), int(self.offsets[i + 1])
        return self.rows.download((hi - lo, 128), np.uint8, lo * 128) if hi > lo else np.zeros((0, 128), np.uint8)

    def host_frames(self) -> np.ndarray:
        """(total, 6) float32 frames of all images (downloaded once, then kept)."""
        if self._host_frames is None:
            n = self.total_rows
            self._host_frames = self.frames.download((n, 6), np.float32) if n else np.zeros((0, 6), np.float32)
        return self._host_frames

    def frames_of(self, path) -> np.ndarray:
        """(n, 6) float32 frames of one image: x, y, size, angle, response, octave."""
        i = self._pos[path]
        return self.host_frames()[int(self.offsets[i]):int(self.offsets[i + 1])]

    # -------------------------------------------------------------------------------------------------- updates
    def add(self, other, rows_list=None, frames_list=None) -> "LocalFeatureIndex":
        """Append images: `add(other)` with a LocalFeatureIndex copies its rows and frames on the device and takes its paths;
        `add(paths, rows_list, frames_list)` takes host arrays as `from_arrays` does.  A path the index already holds is a
        ValueError before anything changes; an empty batch is a no-op.  Together with an ASMKIndex: `local.add(new); asmk.add(new)`."""
        if isinstance(other, LocalFeatureIndex):
            if rows_list is not None or frames_list is not None:
                raise ValueError("add takes a LocalFeatureIndex alone, or paths with rows_list and frames_list")
            paths, off, host = list(other.paths), other.offsets, None
        else:
            if rows_list is None or frames_list is None:
                raise ValueError("add takes a LocalFeatureIndex alone, or paths with rows_list and frames_list")
            paths = list(other)
            rows_list = [_u8_rows("rows", r) for r in rows_list]
            frames_list = [np.ascontiguousarray(f, dtype=np.float32).reshape(-1, 6) for f in frames_list]
            if len(rows_list) != len(frames_list) or any(len(r) != len(f) for r, f in zip(rows_list, frames_list)):
                raise ValueError("rows and frames must pair up image by image and row by row")
            if len(rows_list) != len(paths):
                raise ValueError(f"{len(paths)} paths but {len(rows_list)} arrays of rows")
            off = np.zeros(len(paths) + 1, np.int64)
            np.cumsum([len(r) for r in rows_list], out=off[1:])
            host = (rows_list, frames_list)
        have = set(self.paths)
        for p in paths:
            if p in have:
                raise ValueError(f"{p!r} is already in the index (or named twice)")
            have.add(p)
        if not paths:
            return self
        ctx, total, more = self.ctx, self.total_rows, int(off[-1])
        if more:
            rows, frames = ctx.buffer((total + more) * 128), ctx.buffer((total + more) * 24)
            ctx.copy_dev(rows.ptr, self.rows.ptr, total * 128)
            ctx.copy_dev(frames.ptr, self.frames.ptr, total * 24)
            if host is None:
                ctx.copy_dev(rows.ptr + total * 128, other.rows.ptr, more * 128)
                ctx.copy_dev(frames.ptr + total * 24, other.frames.ptr, more * 24)
            else:
                rows.upload(np.concatenate(host[0]), total * 128)
                frames.upload(np.concatenate(host[1]), total * 24)
            ctx.sync()
            self.rows.free()
            self.frames.free()
            self.rows, self.frames = rows, frames
        self.offsets = np.concatenate([self.offsets, total + np.asarray(off[1:], np.int64)])
        self.paths = self.paths + paths
        self._pos = {p: i for i, p in enumerate(self.paths)}
        self._host_frames = None
        return self

    def remove(self, paths) -> "LocalFeatureIndex":
        """Drop the named images; the survivors keep their order.  Rows and frames are compacted in place on the device.  An unknown
        path is a KeyError, a path named twice a ValueError, both before anything changes; an empty list is a no-op."""
        gone = []
        for p in list(paths):
            if p not in self._pos:
                raise KeyError(p)
            gone.append(self._pos[p])
        if len(set(gone)) != len(gone):
            raise ValueError("a path is named twice")
        if not gone:
            return self
        gone = sorted(gone)
        ctx, total, off = self.ctx, self.total_rows, self.offsets
        removed = np.concatenate([np.arange(off[i], off[i + 1], dtype=np.int64) for i in gone])
        if len(removed):
            with ctx.scratch() as tmp:
                d_removed, d_keep, d_pos = tmp.upload(removed), tmp(total), tmp((total + 1) * 8)
                ctx.keep_mask_dev(d_removed.ptr, len(removed), total, d_keep.ptr)
                ctx.keep_positions_dev(d_keep.ptr, total, d_pos.ptr)
                ctx.compact_rows_dev(self.rows.ptr, total, 128, d_keep.ptr, d_pos.ptr, self.rows.ptr, first=int(removed[0]))
                ctx.compact_rows_dev(self.frames.ptr, total, 24, d_keep.ptr, d_pos.ptr, self.frames.ptr, first=int(removed[0]))
                ctx.sync()
        dead = set(gone)
        counts = [int(off[i + 1] - off[i]) for i in range(len(self.paths)) if i not in dead]
        self.paths = [p for i, p in enumerate(self.paths) if i not in dead]
        self.offsets = np.zeros(len(self.paths) + 1, np.int64)
        np.cumsum(counts, out=self.offsets[1:])
        self._pos = {p: i for i, p in enumerate(self.paths)}
        self._host_frames = None
        return self

    def close(self):
        for b in (self.rows, self.frames):
            if b is not None:
                b.free()
        self.rows = self.frames = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __repr__(self):
        return f"LocalFeatureIndex(images={len(self)}, rows={self.total_rows})"


def _load(item):
    if isinstance(item, str):
        from .encoders._base_encoder import _read_rgb
        return _read_rgb(item)
    return item


def _match_stage(ctx, rows_a, off_a, rows_b, off_b, pairs, ratio, mutual):
    """Stages 1 + 2 for a pair list -> dict of device buffers (idx, d1, d2, matches, counts) and the per-pair entry offsets."""
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    na = (off_a[1:] - off_a[:-1])[pairs[:, 0]] if len(pairs) else np.zeros(0, np.int64)
    nb = (off_b[1:] - off_b[:-1])[pairs[:, 1]] if len(pairs) else np.zeros(0, np.int64)
    out_a = np.zeros(len(pairs) + 1, np.int64)
    np.cumsum(na, out=out_a[1:])
    ta, tb = int(out_a[-1]), int(nb.sum())
    b = {k: ctx.buffer(max(ta, 1) * 4) for k in ("idx", "d1", "d2")}
    b["matches"] = ctx.buffer(max(ta, 1) * 8)
    b["counts"] = ctx.buffer(max(len(pairs), 1) * 4)
    rev = [ctx.buffer(max(tb, 1) * 4) for _ in range(3)] if mutual else []
    try:
        ctx.match_u8_dev(rows_a, off_a, rows_b, off_b, pairs, b["idx"].ptr, b["d1"].ptr, b["d2"].ptr)
        if mutual:
            ctx.match_u8_dev(rows_b, off_b, rows_a, off_a, pairs[:, ::-1], rev[0].ptr, rev[1].ptr, rev[2].ptr)
        ctx.match_filter_dev(off_a, off_b, pairs, b["idx"].ptr, b["d1"].ptr, b["d2"].ptr, rev[0].ptr if mutual else None,
                             float(ratio) * float(ratio), mutual, b["matches"].ptr, b["counts"].ptr)
        if rev:
            ctx.sync()                      # the transposed results go back to the context's cache: their reader must be done
    except Exception:
        for x in b.values():
            x.free()
        raise
    finally:
        for x in rev:
            x.free()
    return b, pairs, out_a


def match(rows_a, rows_b, ratio: float = 0.8, mutual: bool = True, ctx=None):
    """Match two host arrays of (n, 128) uint8 descriptors: nearest and second nearest row of `rows_b` for every row of `rows_a`
    (exact squared Euclidean distances), Lowe's ratio test d1 < ratio^2 d2 and, with `mutual`, the cross check.
    -> (matches (m, 2) int32 (i, j) in ascending i, d1 (m,) int32, d2 (m,) int32)."""
    from .engine import default_context
    ratio, mutual = _check_ratio(ratio), _check_bool("mutual", mutual)
    a, b = _u8_rows("rows_a", rows_a), _u8_rows("rows_b", rows_b)
    ctx = ctx if ctx is not None else default_context()
    off_a, off_b = np.array([0, len(a)], np.int64), np.array([0, len(b)], np.int64)
    if len(a) == 0:
        return np.zeros((0, 2), np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32)
    da, db = ctx.buffer(max(a.nbytes, 1)), ctx.buffer(max(b.nbytes, 1))
    bufs = {}
    try:
        da.upload(a)
        if len(b):
            db.upload(b)
        bufs, _, _ = _match_stage(ctx, da.ptr, off_a, db.ptr, off_b, [[0, 0]], ratio, mutual)
        m = int(bufs["counts"].download((1,), np.int32)[0])
        matches = bufs["matches"].download((len(a), 2), np.int32)[:m].copy()
        d1 = bufs["d1"].download((len(a),), np.int32)[matches[:, 0]]
        d2 = bufs["d2"].download((len(a),), np.int32)[matches[:, 0]]
        return matches, d1, d2
    finally:
        for x in (da, db, *bufs.values()):
            x.free()


class SpatialVerifier:
    """Match + verify image pairs on the device.

    ratio: Lowe's ratio (a match is kept iff d1 < ratio^2 d2 on squared distances); mutual: keep a match only if it is the best in
    both directions; tol: inlier threshold, an ABSOLUTE distance in pixels of the candidate (B) image, not scaled by the image or
    the keypoint size (default DEFAULT_TOL = 12); refine_rounds: rounds of affine least-squares refinement after the exhaustive
    hypothesis search; extractor: what `verify` extracts the query with (default KeypointRootSIFT(nfeatures=2000))."""

    def __init__(self, ratio: float = 0.8, mutual: bool = True, tol: float = DEFAULT_TOL, refine_rounds: int = 2, extractor=None,
                 ctx=None):
        self.ratio = _check_ratio(ratio)
        self.mutual = _check_bool("mutual", mutual)
        if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not (tol > 0 and np.isfinite(tol)):
            raise ValueError(f"tol must be a positive number of pixels, got {tol!r}")
        if isinstance(refine_rounds, bool) or not isinstance(refine_rounds, (int, np.integer)) or refine_rounds < 0:
            raise ValueError(f"refine_rounds must be a non-negative integer, got {refine_rounds!r}")
        if extractor is not None and not hasattr(extractor, "device_descriptors"):
            raise ValueError("the extractor must provide device_descriptors(..., frames=True) (KeypointSIFT / KeypointRootSIFT)")
        self.tol, self.refine_rounds = float(tol), int(refine_rounds)
        self._extractor, self._ctx = extractor, ctx

    @property
    def extractor(self):
        if self._extractor is None:
            from .features import KeypointRootSIFT
            self._extractor = KeypointRootSIFT(nfeatures=2000, ctx=self._ctx)
        return self._extractor

    def verify_pairs(self, index_a: LocalFeatureIndex, index_b: LocalFeatureIndex, pairs) -> list:
        """Verify (position in index_a, position in index_b) pairs: one matching call per direction, one filter call and one
        verification call for the whole list.  -> [Verification] in the order of `pairs`."""
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        if len(pairs) and (pairs.min() < 0 or pairs[:, 0].max() >= len(index_a) or pairs[:, 1].max() >= len(index_b)):
            raise ValueError("a pair names an image outside its index")
        if not len(pairs):
            return []
        ctx = self._ctx if self._ctx is not None else index_b.ctx
        bufs, pairs32, out_a = _match_stage(ctx, index_a.rows.ptr, index_a.offsets, index_b.rows.ptr, index_b.offsets, pairs,
                                            self.ratio, self.mutual)
        n, ta = len(pairs32), int(out_a[-1])
        res = {"inl": ctx.buffer(n * 4), "mod": ctx.buffer(n * 48), "best": ctx.buffer(n * 4), "mask": ctx.buffer(max(ta, 1))}
        try:
            ctx.verify_dev(index_a.frames.ptr, index_a.offsets, index_b.frames.ptr, index_b.offsets, pairs32, bufs["matches"].ptr,
                           bufs["counts"].ptr, self.tol, self.refine_rounds, res["inl"].ptr, res["mod"].ptr, res["best"].ptr,
                           res["mask"].ptr)
            counts = bufs["counts"].download((n,), np.int32)
            inl = res["inl"].download((n,), np.int32)
            models = res["mod"].download((n, 2, 3), np.float64)
            best = res["best"].download((n,), np.int32)
            matches = bufs["matches"].download((max(ta, 1), 2), np.int32)
            mask = res["mask"].download((max(ta, 1),), np.uint8)
        finally:
            for x in (*bufs.values(), *res.values()):
                x.free()
        fa, fb = index_a.host_frames(), index_b.host_frames()
        out = []
        for p, (ia, ib) in enumerate(pairs32):
            lo, m = int(out_a[p]), int(counts[p])
            mt = matches[lo:lo + m].copy()
            out.append(Verification(int(inl[p]), models[p].copy(), mt, fa[int(index_a.offsets[ia]) + mt[:, 0]],
                                    fb[int(index_b.offsets[ib]) + mt[:, 1]], mask[lo:lo + m].astype(bool), int(best[p])))
        return out

    def verify(self, query_image, index: LocalFeatureIndex, candidates) -> list:
        """Verify one query image against `candidates` (paths held by `index`).  The query is extracted once; the models map
        query coordinates to candidate coordinates.  -> [Verification] in the order of the candidates; KeyError for a path the
        index does not hold."""
        positions = [index.position(c) for c in candidates]
        if not positions:
            return []
        q = LocalFeatureIndex.from_images([query_image], self.extractor, paths=["query"], ctx=index.ctx)
        try:
            return self.verify_pairs(q, index, [(0, p) for p in positions])
        finally:
            q.close()

    def __repr__(self):
        return (f"SpatialVerifier(ratio={self.ratio}, mutual={self.mutual}, tol={self.tol}, refine_rounds={self.refine_rounds})")
