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

The graph is a snapshot of the index it was built from: after `index.add` / `remove` it refuses to rank (build a new one).

    g = Diffusion.build(index, k=50, mutable=True)          # float32 indexes: the graph also keeps the forward similarities (16 kg bytes per image)
    g.add({"new.jpg": vec}); g.remove(["old.jpg"])          # change the index THROUGH the graph: no rebuild, the same bits as one
    g.last_update                                           # op, rows, reranked (lists ranked again from scratch), n

A mutable graph follows the index: an add ranks the new rows against the index and every old row against the
new rows alone, and merges; a remove re-ranks only the rows that listed a removed one.  Afterwards nbr, sim and s equal those of
`Diffusion.build` on the updated index, bit for bit."""
from __future__ import annotations

import numpy as np

from . import _ffi
from .engine import diffuse_workspace
from .index import _keep_positions

__all__ = ["Diffusion"]

GAMMA_MAX = 8
_TRANSPOSE_MAX_ROWS = 65535 * 32          # pvs_transpose_f64_dev
_VECTORS_PER_COLUMN = 5                   # Y (later the transposed scores), X and the solver's r, p, Ap


def _check_int(name, v, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
        rng = f"in {lo}..{hi}" if hi is not None else f">= {lo}"
        raise ValueError(f"{name} must be an integer {rng}, got {v!r}")
    return int(v)


def _check_mutable_dtype(dt):
    if dt != np.float32:
        raise TypeError("a mutable graph needs a float32 index: a float64 score depends on how its tile is split along k, and that "
                        "follows the shape of the call, so lists ranked in parts would not equal a rebuild's bit for bit")


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
    fixed-width rows (a slot that is not mutual holds +0).  A mutable graph also keeps `sim` float32 (N, kg), the similarities the
    ranking returned in list order, from which `add` and `remove` bring the lists to those of the updated index."""

    COLUMN_BYTES = 1 << 30                 # device bytes one tile of queries may take in `rank` / `solve`

    def __init__(self, ctx, d_nbr, d_s, n: int, kg: int, gamma: int, index=None, d_sim=None, block: int = 4096):
        self.ctx, self._d_nbr, self._d_s, self.n, self.kg, self.gamma, self.index = ctx, d_nbr, d_s, int(n), int(kg), int(gamma), index
        self._d_sim, self.block = d_sim, int(block)           # rows ranked together by `add` / `remove`, as by `build`
        self._mods = index.modifications if index is not None else 0
        self.last_solve = self.last_update = None

    @property
    def mutable(self) -> bool:
        """whether the graph keeps `sim` and so takes `add` / `remove`"""
        return self._d_sim is not None

    # ---- construction
    @classmethod
    def build(cls, index, k: int = 50, gamma: int = 3, block: int = 4096, mutable: bool = False) -> "Diffusion":
        """Every row of `index` is ranked against the whole index to depth k + 1, `block` rows at a time (the ranking of
        `index.rank`, lists left on the device), the row itself is dropped, and the graph kernels turn the lists into nbr and s.
        1 <= k <= N - 1; integer 0 <= gamma <= 8 (the affinity is the similarity to that power).
        mutable: the graph keeps the similarities of its lists and takes `add` / `remove`; the same nbr and s, bit for bit.  It needs
        a float32 index (TypeError otherwise)."""
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
        if mutable:
            _check_mutable_dtype(dt)
        with ctx.scratch() as tmp:
            d_nbr = tmp(N * kg * 4)
            d_sim = tmp(N * kg * 4) if mutable else None
            d_a = None if mutable else tmp(N * kg * 8)
            for b0 in range(0, N, block):
                b = min(N, b0 + block) - b0
                with ctx.scratch() as lists:
                    _, d_idx, d_val = index._rank_dev_buffers(lists, index._db.ptr + b0 * L * dt.itemsize, b, kg + 1)
                    if mutable:
                        ctx.graph_lists_dev(d_idx.ptr, d_val.ptr, b, kg, b0, N, d_nbr.ptr, d_sim.ptr)
                    else:
                        ctx.graph_affinity_dev(d_idx.ptr, d_val.ptr, dt == np.float64, b, kg, b0, N, gamma, d_nbr.ptr, d_a.ptr)
            d_s = cls._normalised(ctx, tmp, d_nbr, d_sim, d_a, N, kg, gamma)
            ctx.sync()
            return cls(ctx, tmp.keep(d_nbr), tmp.keep(d_s), N, kg, gamma, index, tmp.keep(d_sim) if mutable else None, block)  # the graph's from here on

    @staticmethod
    def _normalised(ctx, tmp, d_nbr, d_sim, d_a, N, kg, gamma):
        """a (from the stored similarities where it is not given) -> mutual -> degrees -> s, a buffer of the scratch scope `tmp`"""
        d_w, d_s, d_deg, d_r = tmp(N * kg * 8), tmp(N * kg * 8), tmp(N * 8), tmp(N * 8)
        if d_a is None:
            d_a = tmp(N * kg * 8)
            ctx.graph_affinity_sim_dev(d_sim.ptr, N, kg, gamma, d_a.ptr)
        ctx.graph_mutual_dev(d_nbr.ptr, d_a.ptr, N, kg, d_w.ptr)
        ctx.graph_degrees_dev(d_w.ptr, N, kg, d_deg.ptr, d_r.ptr)
        ctx.graph_normalise_dev(d_nbr.ptr, d_w.ptr, d_r.ptr, N, kg, d_s.ptr)
        return d_s

    @classmethod
    def from_arrays(cls, nbr, s, gamma: int, index=None, ctx=None, sim=None) -> "Diffusion":
        """A graph from host arrays nbr (N, kg) integers and s (N, kg) float64 (what `save` wrote, or a hand-made one).  Without
        `index` it can `solve` but not `rank`.  With `sim` (N, kg) float32, the similarities of the lists, the graph is mutable."""
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
        if sim is not None:
            sim = np.ascontiguousarray(sim)
            if sim.shape != nbr.shape or sim.dtype != np.float32:
                raise ValueError("sim must be a float32 array of the shape of nbr")
            if index is not None:
                _check_mutable_dtype(index.dtype)
        ctx = index.ctx if index is not None else (ctx or default_context())
        nbr32 = np.where((nbr >= 0) & (nbr < N), nbr, -1).astype(np.int32)
        with ctx.scratch() as tmp:
            d_nbr, d_s = tmp.upload(nbr32), tmp.upload(s)
            d_sim = tmp.upload(sim) if sim is not None else None
            return cls(ctx, tmp.keep(d_nbr), tmp.keep(d_s), N, kg, gamma, index, tmp.keep(d_sim) if sim is not None else None)

    # ---- the arrays
    @property
    def nbr(self) -> np.ndarray:
        """(N, kg) int32 host copy"""
        return self._d_nbr.download((self.n, self.kg), np.int32)

    @property
    def s(self) -> np.ndarray:
        """(N, kg) float64 host copy"""
        return self._d_s.download((self.n, self.kg), np.float64)

    @property
    def sim(self) -> np.ndarray:
        """(N, kg) float32 host copy of the similarities of the lists; a mutable graph's only"""
        if self._d_sim is None:
            raise AttributeError("only a mutable graph keeps sim (Diffusion.build(index, mutable=True))")
        return self._d_sim.download((self.n, self.kg), np.float32)

    def save(self, path: str) -> None:
        """One .npz of plain arrays (no pickles): nbr, s, gamma and the state of the index the graph belongs to; sim too where the
        graph is mutable."""
        extra = {"sim": self.sim} if self.mutable else {}
        np.savez(path, nbr=self.nbr, s=self.s, gamma=np.int64(self.gamma), index_modifications=np.int64(self._mods), **extra)

    @classmethod
    def load(cls, path: str, index) -> "Diffusion":
        """The graph `save` wrote, for the index it was built from: RuntimeError if that index has changed since.  A file that holds
        sim gives a mutable graph."""
        from .index import DeviceIndex
        if not isinstance(index, DeviceIndex):
            raise TypeError("Diffusion.load needs the pvsim.index.DeviceIndex the graph was built from")
        with np.load(path if str(path).endswith(".npz") else str(path) + ".npz", allow_pickle=False) as z:
            nbr, s, gamma, mods = z["nbr"], z["s"], int(z["gamma"]), int(z["index_modifications"])
            sim = z["sim"] if "sim" in z.files else None
        if nbr.ndim != 2 or nbr.shape[0] != len(index) or mods != index.modifications:
            raise RuntimeError("the index has changed since the graph was built (rows were added or removed): build a new graph")
        return cls.from_arrays(nbr, s, gamma, index, sim=sim)

    def close(self):
        for b in (self._d_nbr, self._d_s, self._d_sim):
            if b is not None:
                b.free()

    # ---- following the index
    def _check_mutable(self):
        if not self.mutable:
            raise RuntimeError("this graph is immutable: build it with mutable=True to add or remove through it")
        self._check_snapshot()
        return self.index

    def _replace(self, d_nbr, d_s, d_sim, n: int, op: str, rows: int, reranked: int) -> None:
        self.close()
        self._d_nbr, self._d_s, self._d_sim, self.n, self._mods = d_nbr, d_s, d_sim, int(n), self.index.modifications
        self.last_update = {"op": op, "rows": int(rows), "reranked": int(reranked), "n": int(n)}

    def add(self, encoding_map) -> None:
        """`index.add(encoding_map)`, and the graph follows: the b new rows are ranked against the whole updated index, every old row
        against the new rows alone (to depth min(kg, b)), and each stored list is merged with its candidates -- 2 N b L work instead
        of a rebuild's N^2 L.  Refused before anything changes: an immutable graph, a stale one (RuntimeError both), and whatever
        `index.add` refuses (a known path, another length or dtype)."""
        index = self._check_mutable()
        N, kg, ctx, block = self.n, self.kg, self.ctx, self.block
        index.add(encoding_map)                                  # checks first, changes then
        M, L = index.shape
        b = M - N
        if b == 0:
            return
        with ctx.scratch() as tmp:
            d_nbr, d_sim = tmp(M * kg * 4), tmp(M * kg * 4)
            for b0 in range(N, M, block):                        # the new rows: build's own step
                nb = min(M, b0 + block) - b0
                with ctx.scratch() as lists:
                    _, d_idx, d_val = index._rank_dev_buffers(lists, index._db.ptr + b0 * L * 4, nb, kg + 1)
                    ctx.graph_lists_dev(d_idx.ptr, d_val.ptr, nb, kg, b0, M, d_nbr.ptr, d_sim.ptr)
            c = min(kg, b)
            for b0 in range(0, N, block):                        # the old rows, as queries against the new ones
                nb = min(N, b0 + block) - b0
                with ctx.scratch() as lists:
                    d_ci, d_cv = index._rank_dev_range(lists, index._db.ptr + b0 * L * 4, nb, c, N, M)
                    ctx.graph_merge_dev(self._d_nbr.ptr + b0 * kg * 4, self._d_sim.ptr + b0 * kg * 4, d_ci.ptr, d_cv.ptr, nb, kg, c, N, M,
                                        d_nbr.ptr + b0 * kg * 4, d_sim.ptr + b0 * kg * 4)
            d_s = self._normalised(ctx, tmp, d_nbr, d_sim, None, M, kg, self.gamma)
            ctx.sync()
            self._replace(tmp.keep(d_nbr), tmp.keep(d_s), tmp.keep(d_sim), M, "add", b, b)

    def remove(self, paths) -> None:
        """`index.remove(paths)`, and the graph follows: a surviving row that listed a removed one is ranked again against the whole
        updated index; every other list only has its entries renumbered and moves up.  Refused before anything changes: an immutable
        graph, a stale one (RuntimeError both), what `index.remove` refuses (an unknown path: KeyError; one named twice:
        ValueError), and a remove that would leave fewer than kg + 1 rows (ValueError)."""
        index = self._check_mutable()
        N, kg, ctx, block = self.n, self.kg, self.ctx, self.block
        paths = [paths] if isinstance(paths, str) else list(paths)      # read twice: here and by index.remove
        idx = index._ledger.removed_indices(paths)
        if idx.size == 0:
            return
        M, L = N - int(idx.size), index.shape[1]
        if kg > M - 1:
            raise ValueError(f"a graph of kg = {kg} neighbours per row needs at least {kg + 1} rows, this remove would leave {M}")
        with ctx.scratch() as tmp:
            keep, pos = _keep_positions(tmp, idx, N)
            flag, d_old = tmp(N), tmp(N * kg * 4)
            ctx.graph_damage_dev(self._d_nbr.ptr, N, kg, keep.ptr, flag.ptr)
            # pvs_compact_rows_dev checks its output as if every row stayed, so the compacted arrays get the room of the old ones
            flag_new, pos_new = tmp(N), tmp((M + 1) * 8)         # the damage flag and its positions in the new numbering
            ctx.compact_rows_dev(flag.ptr, N, 1, keep.ptr, pos.ptr, flag_new.ptr)
            ctx.keep_positions_dev(flag_new.ptr, M, pos_new.ptr)
            damaged = int(pos_new.download((1,), np.int64, offset=M * 8)[0])
            d_nbr, d_sim = tmp(N * kg * 4), tmp(N * kg * 4)
            ctx.graph_remap_dev(self._d_nbr.ptr, N, kg, keep.ptr, pos.ptr, d_old.ptr)
            ctx.compact_rows_dev(d_old.ptr, N, kg * 4, keep.ptr, pos.ptr, d_nbr.ptr)
            ctx.compact_rows_dev(self._d_sim.ptr, N, kg * 4, keep.ptr, pos.ptr, d_sim.ptr)
            index.remove(paths)
            if damaged:
                d_ids = tmp(M * 8)                               # the new ids of the damaged rows: an iota compacted by their flag
                ctx.compact_rows_dev(tmp.upload(np.arange(M, dtype=np.int64)).ptr, M, 8, flag_new.ptr, pos_new.ptr, d_ids.ptr)
                d_rows = tmp(min(damaged, block) * L * 4)
                for b0 in range(0, damaged, block):              # side by side they are one block of queries; self is dropped by the row's own new id
                    nb = min(damaged, b0 + block) - b0
                    ctx.graph_gather_rows_dev(index._db.ptr, M, L * 4, d_ids.ptr + b0 * 8, nb, d_rows.ptr)
                    with ctx.scratch() as lists:
                        _, d_idx, d_val = index._rank_dev_buffers(lists, d_rows.ptr, nb, kg + 1)
                        ctx.graph_lists_dev(d_idx.ptr, d_val.ptr, nb, kg, 0, M, d_nbr.ptr, d_sim.ptr, d_ids=d_ids.ptr + b0 * 8)
            d_s = self._normalised(ctx, tmp, d_nbr, d_sim, None, M, kg, self.gamma)
            ctx.sync()
            self._replace(tmp.keep(d_nbr), tmp.keep(d_s), tmp.keep(d_sim), M, "remove", idx.size, damaged)

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
