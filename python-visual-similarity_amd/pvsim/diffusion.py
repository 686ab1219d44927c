"""Diffusion re-ranking on the kNN graph of a resident index.

    g = Diffusion.build(index, k=50, gamma=3)               # offline: the graph of a pvsim.index.DeviceIndex, resident on the device
    idx, val = g.rank(queries, k=10, kq=10, alpha=0.99)     # (nq, k) int64 / float64 diffusion scores
    g.last_solve                                            # per query: steps, residual = sqrt(rr / yy), converged
    g.save("graph.npz"); g = Diffusion.load("graph.npz", index)

Query expansion and database-side augmentation look one hop around the query.  Diffusion (Zhou et al., NIPS 2003; Iscen et al., CVPR
2017; "DFS" in Radenovic et al., PAMI 2018) follows the neighbour graph of the whole database: the query's first kq results are the
right-hand side y of (I - alpha S) f = y, S the symmetrically normalised mutual kNN graph, and the database is ranked by f -- so an
image far from the query in cosine but connected to it through a chain of near neighbours is found.  The graph (12 kg bytes per
image) is built and kept on the device, the system is solved there by conjugate gradients for a tile of queries at a time, and every
number is defined to the bit in include/pvsim.h; tests/diffusion_numpy.py restates it in NumPy.

The graph is a snapshot of the index it was built from: after `index.add` / `remove` it refuses to rank (build a new one)."""
from __future__ import annotations

import numpy as np

from . import _ffi
from .engine import diffuse_workspace

__all__ = ["Diffusion"]

GAMMA_MAX = 8
_TRANSPOSE_MAX_ROWS = 65535 * 32          # pvs_transpose_f64_dev
_VECTORS_PER_COLUMN = 5                   # Y (later the transposed scores), X and the solver's r, p, Ap


def _check_int(name, v, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
        rng = f"in {lo}..{hi}" if hi is not None else f">= {lo}"
        raise ValueError(f"{name} must be an integer {rng}, got {v!r}")
    return int(v)


def _check_solver(alpha, tol, maxiter, check_every, width):
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.integer, np.floating)) or not 0.0 < alpha < 1.0:
        raise ValueError(f"alpha must lie in (0, 1), got {alpha!r}")
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not (0.0 <= tol < float("inf")):
        raise ValueError(f"tol must be a finite number >= 0, got {tol!r}")
    _check_int("maxiter", maxiter, 0)
    _check_int("check_every", check_every, 1)
    if width not in (0, 1, 4, 16, 64):
        raise ValueError(f"width must be 0 (chosen from the number of columns), 1, 4, 16 or 64, got {width!r}")


class Diffusion:
    """The normalised mutual kNN graph of a DeviceIndex, resident on the device: `nbr` int32 (N, kg) and `s` float64 (N, kg) in
    fixed-width rows (a slot that is not mutual holds +0)."""

    COLUMN_BYTES = 1 << 30                 # device bytes one tile of queries may take in `rank` / `solve`

    def __init__(self, ctx, d_nbr, d_s, n: int, kg: int, gamma: int, index=None):
        self.ctx, self._d_nbr, self._d_s, self.n, self.kg, self.gamma, self.index = ctx, d_nbr, d_s, int(n), int(kg), int(gamma), index
        self._mods = index.modifications if index is not None else 0
        self.last_solve = None

    # ---- construction
    @classmethod
    def build(cls, index, k: int = 50, gamma: int = 3, block: int = 4096) -> "Diffusion":
        """Every row of `index` is ranked against the whole index to depth k + 1, `block` rows at a time (the ranking of
        `index.rank`, lists left on the device), the row itself is dropped, and the graph kernels turn the lists into nbr and s.
        1 <= k <= N - 1; integer 0 <= gamma <= 8 (the affinity is the similarity to that power)."""
        from .index import DeviceIndex
        if not isinstance(index, DeviceIndex):
            raise TypeError("Diffusion.build needs a pvsim.index.DeviceIndex (a dict or a compact index keeps no resident rows to rank)")
        N, L = index.shape
        gamma = _check_int("gamma", gamma, 0, GAMMA_MAX)
        block = _check_int("block", block, 1)
        if N < 2 or L < 1:
            raise ValueError(f"a graph needs at least 2 rows of at least 1 column, the index has shape {(N, L)}")
        kg = _check_int("k", k, 1, N - 1)
        ctx, dt = index.ctx, index.dtype
        with ctx.scratch() as tmp:
            d_nbr, d_a, d_w, d_s, d_deg, d_r = tmp(N * kg * 4), tmp(N * kg * 8), tmp(N * kg * 8), tmp(N * kg * 8), tmp(N * 8), tmp(N * 8)
            for b0 in range(0, N, block):
                b = min(N, b0 + block) - b0
                with ctx.scratch() as lists:
                    _, d_idx, d_val = index._rank_dev_buffers(lists, index._db.ptr + b0 * L * dt.itemsize, b, kg + 1)
                    ctx.graph_affinity_dev(d_idx.ptr, d_val.ptr, dt == np.float64, b, kg, b0, N, gamma, d_nbr.ptr, d_a.ptr)
            ctx.graph_mutual_dev(d_nbr.ptr, d_a.ptr, N, kg, d_w.ptr)
            ctx.graph_degrees_dev(d_w.ptr, N, kg, d_deg.ptr, d_r.ptr)
            ctx.graph_normalise_dev(d_nbr.ptr, d_w.ptr, d_r.ptr, N, kg, d_s.ptr)
            ctx.sync()
            return cls(ctx, tmp.keep(d_nbr), tmp.keep(d_s), N, kg, gamma, index)      # the graph's from here on

    @classmethod
    def from_arrays(cls, nbr, s, gamma: int, index=None, ctx=None) -> "Diffusion":
        """A graph from host arrays nbr (N, kg) integers and s (N, kg) float64 (what `save` wrote, or a hand-made one).  Without
        `index` it can `solve` but not `rank`."""
        from .engine import default_context
        nbr = np.ascontiguousarray(nbr)
        s = np.ascontiguousarray(s)
        if nbr.ndim != 2 or nbr.shape != s.shape or nbr.dtype.kind != "i" or s.dtype != np.float64:
            raise ValueError("nbr must be an (N, kg) integer array and s a float64 array of the same shape")
        N, kg = nbr.shape
        if N < 2 or not 1 <= kg <= N - 1:
            raise ValueError(f"need N >= 2 and 1 <= kg <= N - 1, got N = {N}, kg = {kg}")
        gamma = _check_int("gamma", gamma, 0, GAMMA_MAX)
        if index is not None and len(index) != N:
            raise ValueError(f"the graph has {N} rows, the index {len(index)}")
        ctx = index.ctx if index is not None else (ctx or default_context())
        nbr32 = np.where((nbr >= 0) & (nbr < N), nbr, -1).astype(np.int32)
        with ctx.scratch() as tmp:
            d_nbr, d_s = tmp.upload(nbr32), tmp.upload(s)
            return cls(ctx, tmp.keep(d_nbr), tmp.keep(d_s), N, kg, gamma, index)

    # ---- the arrays
    @property
    def nbr(self) -> np.ndarray:
        """(N, kg) int32 host copy"""
        return self._d_nbr.download((self.n, self.kg), np.int32)

    @property
    def s(self) -> np.ndarray:
        """(N, kg) float64 host copy"""
        return self._d_s.download((self.n, self.kg), np.float64)

    def save(self, path: str) -> None:
        """One .npz of plain arrays (no pickles): nbr, s, gamma and the state of the index the graph belongs to."""
        np.savez(path, nbr=self.nbr, s=self.s, gamma=np.int64(self.gamma), index_modifications=np.int64(self._mods))

    @classmethod
    def load(cls, path: str, index) -> "Diffusion":
        """The graph `save` wrote, for the index it was built from: RuntimeError if that index has changed since."""
        from .index import DeviceIndex
        if not isinstance(index, DeviceIndex):
            raise TypeError("Diffusion.load needs the pvsim.index.DeviceIndex the graph was built from")
        with np.load(path if str(path).endswith(".npz") else str(path) + ".npz", allow_pickle=False) as z:
            nbr, s, gamma, mods = z["nbr"], z["s"], int(z["gamma"]), int(z["index_modifications"])
        if nbr.ndim != 2 or nbr.shape[0] != len(index) or mods != index.modifications:
            raise RuntimeError("the index has changed since the graph was built (rows were added or removed): build a new graph")
        return cls.from_arrays(nbr, s, gamma, index)

    def close(self):
        for b in (self._d_nbr, self._d_s):
            b.free()

    # ---- solving
    def _tile(self, nq: int, column_bytes) -> int:
        """columns solved together: what `column_bytes` device bytes hold, at least one"""
        budget = self.COLUMN_BYTES if column_bytes is None else _check_int("column_bytes", column_bytes, 1)
        return int(max(1, min(nq, budget // (_VECTORS_PER_COLUMN * 8 * self.n), _ffi.DIFFUSE_MAX_COLUMNS)))

    def _solve_dev(self, d_y, C, alpha, tol, maxiter, check_every, width, d_x, d_cols):
        """pvs_diffuse_cg_dev on C columns that are on the device; d_cols holds steps | rr | yy -> (steps, rr, yy) on the host"""
        nbytes = diffuse_workspace(self.n, C)
        with self.ctx.scratch() as tmp:
            self.ctx.diffuse_cg_dev(self._d_nbr.ptr, self._d_s.ptr, self.n, self.kg, d_y, C, alpha, tol, maxiter, check_every, width,
                                    tmp(nbytes).ptr, nbytes, d_x, d_cols.ptr, d_cols.ptr + 8 * C, d_cols.ptr + 16 * C)
            return (d_cols.download((C,), np.int32), d_cols.download((C,), np.float64, offset=8 * C),
                    d_cols.download((C,), np.float64, offset=16 * C))

    def _report(self, steps, rr, yy, tol):
        with np.errstate(divide="ignore", invalid="ignore"):
            res = np.where(yy > 0, np.sqrt(rr / yy), 0.0)
        self.last_solve = {"steps": steps, "residual": res, "converged": rr <= (tol * tol) * yy, "rr": rr, "yy": yy}

    def solve(self, Y, alpha: float = 0.99, tol: float = 1e-6, maxiter: int = 20, check_every: int = 4, column_bytes=None, width: int = 0):
        """(I - alpha S) F = Y for host columns Y (N, nq) float64 -> (F (N, nq), steps int32 (nq,), rr, yy).  Columns are solved in tiles
        of `column_bytes` device bytes; `check_every`: steps between two looks of the host at the convergence flags; `width`: the
        kernel's column width (0: chosen from the tile).  None of the three changes a bit of the result."""
        _check_solver(alpha, tol, maxiter, check_every, width)
        Y = np.asarray(Y)
        if Y.ndim != 2 or Y.shape[0] != self.n or Y.dtype != np.float64:
            raise ValueError(f"Y must be a float64 array of shape ({self.n}, nq)")
        nq = Y.shape[1]
        F = np.zeros((self.n, nq))
        steps, rr, yy = np.zeros(nq, np.int32), np.zeros(nq), np.zeros(nq)
        tile = self._tile(nq, column_bytes) if nq else 0
        for c0 in range(0, nq, max(tile, 1)):
            C = min(tile, nq - c0)
            with self.ctx.scratch() as tmp:
                d_y, d_x, d_cols = tmp.upload(Y[:, c0:c0 + C]), tmp(self.n * C * 8), tmp(24 * C)
                steps[c0:c0 + C], rr[c0:c0 + C], yy[c0:c0 + C] = self._solve_dev(d_y.ptr, C, alpha, tol, maxiter, check_every, width,
                                                                               d_x.ptr, d_cols)
                F[:, c0:c0 + C] = d_x.download((self.n, C), np.float64)
        self._report(steps, rr, yy, tol)
        return F, steps, rr, yy

    def _check_snapshot(self):
        if self.index is None:
            raise RuntimeError("this graph was made from arrays without an index: it can solve, not rank")
        if self.index.modifications != self._mods or len(self.index) != self.n:
            raise RuntimeError("the index has changed since the graph was built (rows were added or removed): build a new graph")

    def rank(self, query_vecs, k: int = 10, kq: int = 10, alpha: float = 0.99, tol: float = 1e-6, maxiter: int = 20, check_every: int = 4,
             column_bytes=None, width: int = 0):
        """The queries are ranked against the index to depth kq; the affinities of those results are the right-hand side; the
        system is solved on the device and the database ranked by the solution: -> (idx (nq, k) int64, val (nq, k) float64), score
        descending, index ascending.  The values are diffusion scores, not cosines; rows the query's results do not reach score
        exactly 0 and come in index order.  1 <= k <= N, 1 <= kq <= N.  `last_solve` reports the solver per query.
        A float64 query against a float32 index raises TypeError: the first ranking works in the index's dtype."""
        self._check_snapshot()
        _check_solver(alpha, tol, maxiter, check_every, width)
        index, N = self.index, self.n
        L, dt = index.shape[1], index.dtype
        q = np.asarray(query_vecs)
        if q.ndim != 2 or q.shape[1] != L:
            raise ValueError("query and database dimensions differ")
        if dt == np.float32 and q.dtype != np.float32:
            raise TypeError("diffusion ranks the queries in the index's dtype: a float32 index needs float32 queries")
        k = _check_int("k", k, 1, N)
        kq = _check_int("kq", kq, 1, N)
        if N > _TRANSPOSE_MAX_ROWS:
            raise NotImplementedError(f"ranking the solution needs its transpose, which serves at most {_TRANSPOSE_MAX_ROWS} rows")
        q = np.ascontiguousarray(q, dtype=dt)
        nq = q.shape[0]
        idx, val = np.zeros((nq, k), np.int64), np.zeros((nq, k), np.float64)
        steps, rr, yy = np.zeros(nq, np.int32), np.zeros(nq), np.zeros(nq)
        if nq == 0:
            self._report(steps, rr, yy, tol)
            return idx, val
        ctx = self.ctx
        tile = self._tile(nq, column_bytes)
        with ctx.scratch() as tmp:
            d_q, d_y, d_x = tmp.upload(q), tmp(N * tile * 8), tmp(N * tile * 8)
            d_cols, d_oi, d_ov = tmp(24 * tile), tmp(tile * k * 8), tmp(tile * k * 8)
            for c0 in range(0, nq, tile):
                C = min(tile, nq - c0)
                with ctx.scratch() as lists:
                    _, d_idx, d_val = index._rank_dev_buffers(lists, d_q.ptr + c0 * L * dt.itemsize, C, kq)
                    ctx.diffuse_rhs_dev(d_idx.ptr, d_val.ptr, dt == np.float64, C, kq, N, self.gamma, d_y.ptr)
                steps[c0:c0 + C], rr[c0:c0 + C], yy[c0:c0 + C] = self._solve_dev(d_y.ptr, C, alpha, tol, maxiter, check_every, width,
                                                                               d_x.ptr, d_cols)
                ctx.transpose_f64_dev(d_x.ptr, N, C, d_y.ptr)               # (N, C) -> (C, N): Y is not needed any more
                ctx.rank_f64_dev(d_y.ptr, C, N, N, k, d_oi.ptr, d_ov.ptr)
                idx[c0:c0 + C] = d_oi.download((C, k), np.int64)
                val[c0:c0 + C] = d_ov.download((C, k), np.float64)
        self._report(steps, rr, yy, tol)
        return idx, val
