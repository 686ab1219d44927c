"""k-reciprocal re-ranking on the kNN lists of a resident index.

    r = KReciprocal.build(index, k=40, k1=20, k2=6, gamma=3)     # offline: the lists of a float32 pvsim.index.DeviceIndex and their sets
    idx, val = r.rank(queries, k=10, kq=80, lam=0.3)             # (nq, k) int64 / float64 scores: (1 - lam) Jaccard + lam cosine
    r.last_build, r.last_rank                                    # members kept and dropped, per row and per query
    r = KReciprocal.from_graph(g)                                # from a mutable Diffusion graph: its lists are copied, nothing is ranked
    r.save("krr.npz"); r = KReciprocal.load("krr.npz", index)

Zhong, Zheng, Cao, Li (CVPR 2017): the first kq results of a query are re-ordered by the Jaccard similarity of k-reciprocal
neighbourhoods, so a database image that is near the query but whose own neighbourhood does not contain the query's is demoted.
Diffusion (pvsim.diffusion) follows chains of neighbours; this removes false ones -- it helps where classes overlap and hub images
enter every list.  Two departures from the paper make the result a function of the lists alone, defined to the bit in
include/pvsim.h and restated in tests/reciprocal_numpy.py: a member of an expanded set keeps its weight only where it sits in the
row's own list (the others are counted in `dropped`), and the weights are the affinity of the graph, not exp(-d).

A KReciprocal is a snapshot of the index it was built from: after `index.add` / `remove` it refuses to rank.  With a mutable
Diffusion graph `g` that follows the index, `KReciprocal.from_graph(g)` after `g.add` / `g.remove` costs only the set kernels."""
from __future__ import annotations

import numpy as np

from . import _ffi
from .diffusion import GAMMA_MAX, Diffusion, _check_int, _check_mutable_dtype

__all__ = ["KReciprocal"]

MAX_K1, MAX_KQ = _ffi.KRR_MAX_K1, _ffi.KRR_MAX_KQ


def _check_params(kg, k1, k2, gamma):
    k1 = _check_int("k1", k1, 1, min(kg, MAX_K1))
    k2 = _check_int("k2", k2, 1, kg + 1)
    return k1, k2, _check_int("gamma", gamma, 0, GAMMA_MAX)


class KReciprocal:
    """The lists `nbr` int32 (N, kg) and `sim` float32 (N, kg) of a DeviceIndex with what the query side reads, resident on the
    device: the reciprocal mask at (k1 + 1) // 2, the unexpanded vectors v, v0 and the expanded ones w, w0 with their sums ws, all on the
    fixed support {i} + nbr[i]."""

    def __init__(self, ctx, bufs: dict, n: int, kg: int, k1: int, k2: int, gamma: int, index=None, report=None):
        self.ctx, self._b, self.n, self.kg, self.k1, self.k2, self.gamma, self.index = ctx, bufs, int(n), int(kg), int(k1), int(k2), int(gamma), index
        self._mods = index.modifications if index is not None else 0
        self.last_build, self.last_rank = report, None

    # ---- construction
    @classmethod
    def _from_lists(cls, ctx, tmp, d_nbr, d_sim, N, kg, k1, k2, gamma, index):
        """the set kernels on lists that are on the device (buffers of the scratch scope `tmp`, kept from here on)"""
        d_m1, d_mh, d_memb, d_drop = tmp(N * 8), tmp(N * 8), tmp(N * kg), tmp(N * 4)
        d_v, d_v0, d_w, d_w0, d_ws = tmp(N * kg * 8), tmp(N * 8), tmp(N * kg * 8), tmp(N * 8), tmp(N * 8)
        ctx.krr_sets_dev(d_nbr.ptr, N, kg, k1, d_m1.ptr, d_mh.ptr)
        ctx.krr_members_dev(d_nbr.ptr, d_m1.ptr, d_mh.ptr, N, kg, d_memb.ptr, d_drop.ptr)
        ctx.krr_weights_dev(d_sim.ptr, d_memb.ptr, N, kg, gamma, d_v.ptr, d_v0.ptr)
        ctx.krr_expand_dev(d_nbr.ptr, d_v.ptr, d_v0.ptr, N, kg, k2, d_w.ptr, d_w0.ptr, d_ws.ptr)
        ctx.sync()
        dropped = d_drop.download((N,), np.int32)
        kept = d_memb.download((N, kg), np.uint8).sum(axis=1, dtype=np.int64)
        report = {"members": kept, "dropped": dropped, "dropped_fraction": float(dropped.sum() / max(1, int(kept.sum()) + int(dropped.sum())))}
        bufs = {"nbr": d_nbr, "sim": d_sim, "maskh": d_mh, "members": d_memb, "v": d_v, "v0": d_v0, "w": d_w, "w0": d_w0, "ws": d_ws}
        for b in bufs.values():
            tmp.keep(b)
        return cls(ctx, bufs, N, kg, k1, k2, gamma, index, report)

    @classmethod
    def build(cls, index, k: int = 40, k1: int = 20, k2: int = 6, gamma: int = 3, block: int = 4096) -> "KReciprocal":
        """Every row of `index` is ranked against the whole index to depth k + 1, `block` rows at a time, the row itself is dropped
        (the calls of `Diffusion.build(mutable=True)`), and the set kernels run on the lists.  1 <= k <= N - 1, 1 <= k1 <= min(k, 64),
        1 <= k2 <= k + 1, integer 0 <= gamma <= 8.  A float32 DeviceIndex only (TypeError otherwise)."""
        from .index import DeviceIndex
        if not isinstance(index, DeviceIndex):
            raise TypeError("KReciprocal.build needs a pvsim.index.DeviceIndex (a dict or a compact index keeps no resident rows to rank)")
        _check_mutable_dtype(index.dtype)
        N, L = index.shape
        block = _check_int("block", block, 1)
        if N < 2 or L < 1:
            raise ValueError(f"the lists need at least 2 rows of at least 1 column, the index has shape {(N, L)}")
        kg = _check_int("k", k, 1, N - 1)
        k1, k2, gamma = _check_params(kg, k1, k2, gamma)
        ctx = index.ctx
        with ctx.scratch() as tmp:
            d_nbr, d_sim = tmp(N * kg * 4), tmp(N * kg * 4)
            for b0 in range(0, N, block):
                b = min(N, b0 + block) - b0
                with ctx.scratch() as lists:
                    _, d_idx, d_val = index._rank_dev_buffers(lists, index._db.ptr + b0 * L * 4, b, kg + 1)
                    ctx.graph_lists_dev(d_idx.ptr, d_val.ptr, b, kg, b0, N, d_nbr.ptr, d_sim.ptr)
            return cls._from_lists(ctx, tmp, d_nbr, d_sim, N, kg, k1, k2, gamma, index)

    @classmethod
    def from_graph(cls, g, k1: int = 20, k2: int = 6, gamma: int = 3) -> "KReciprocal":
        """From a mutable `Diffusion` graph of a DeviceIndex: its resident nbr and sim are copied on the device and nothing is ranked.
        The arrays are those of `build` on the same index with k = g.kg."""
        if not isinstance(g, Diffusion):
            raise TypeError("from_graph needs a pvsim.Diffusion")
        if not g.mutable:
            raise ValueError("from_graph needs a mutable graph (Diffusion.build(index, mutable=True)): only that keeps the similarities")
        g._check_snapshot()
        N, kg, ctx = g.n, g.kg, g.ctx
        k1, k2, gamma = _check_params(kg, k1, k2, gamma)
        with ctx.scratch() as tmp:
            d_nbr, d_sim = tmp(N * kg * 4), tmp(N * kg * 4)
            ctx.copy_dev(d_nbr.ptr, g._d_nbr.ptr, N * kg * 4)
            ctx.copy_dev(d_sim.ptr, g._d_sim.ptr, N * kg * 4)
            return cls._from_lists(ctx, tmp, d_nbr, d_sim, N, kg, k1, k2, gamma, g.index)

    @classmethod
    def from_arrays(cls, nbr, sim, k1: int = 20, k2: int = 6, gamma: int = 3, index=None, ctx=None) -> "KReciprocal":
        """From host lists nbr (N, kg) integers and sim (N, kg) float32 (what `save` wrote, or hand-made ones).  Without `index` it
        serves `rank_lists` but not `rank`."""
        from .engine import default_context
        nbr = np.ascontiguousarray(nbr)
        sim = np.ascontiguousarray(sim)
        if nbr.ndim != 2 or nbr.shape != sim.shape or nbr.dtype.kind != "i" or sim.dtype != np.float32:
            raise ValueError("nbr must be an (N, kg) integer array and sim a float32 array of the same shape")
        N, kg = nbr.shape
        if N < 2 or not 1 <= kg <= N - 1:
            raise ValueError(f"need N >= 2 and 1 <= kg <= N - 1, got N = {N}, kg = {kg}")
        k1, k2, gamma = _check_params(kg, k1, k2, gamma)
        if index is not None:
            if len(index) != N:
                raise ValueError(f"the lists have {N} rows, the index {len(index)}")
            _check_mutable_dtype(index.dtype)
        ctx = index.ctx if index is not None else (ctx or default_context())
        nbr32 = np.where((nbr >= 0) & (nbr < N), nbr, -1).astype(np.int32)
        with ctx.scratch() as tmp:
            return cls._from_lists(ctx, tmp, tmp.upload(nbr32), tmp.upload(sim), N, kg, k1, k2, gamma, index)

    # ---- the arrays
    def _host(self, name, shape, dtype):
        return self._b[name].download(shape, dtype)

    @property
    def nbr(self) -> np.ndarray:
        """(N, kg) int32 host copy"""
        return self._host("nbr", (self.n, self.kg), np.int32)

    @property
    def sim(self) -> np.ndarray:
        """(N, kg) float32 host copy"""
        return self._host("sim", (self.n, self.kg), np.float32)

    @property
    def members(self) -> np.ndarray:
        """(N, kg) uint8 host copy: 1 where the slot holds a member of the row's expanded set"""
        return self._host("members", (self.n, self.kg), np.uint8)

    @property
    def v(self) -> np.ndarray:
        return self._host("v", (self.n, self.kg), np.float64)

    @property
    def v0(self) -> np.ndarray:
        return self._host("v0", (self.n,), np.float64)

    @property
    def w(self) -> np.ndarray:
        """(N, kg) float64 host copy of the expanded vectors; `w0` (N,) is the row's own entry and `ws` (N,) the sum of both"""
        return self._host("w", (self.n, self.kg), np.float64)

    @property
    def w0(self) -> np.ndarray:
        return self._host("w0", (self.n,), np.float64)

    @property
    def ws(self) -> np.ndarray:
        return self._host("ws", (self.n,), np.float64)

    def save(self, path: str) -> None:
        """One .npz of plain arrays (no pickles): the lists, the parameters and the state of the index they belong to.  Everything
        else is derived again by `load`."""
        np.savez(path, nbr=self.nbr, sim=self.sim, k1=np.int64(self.k1), k2=np.int64(self.k2), gamma=np.int64(self.gamma),
                 index_modifications=np.int64(self._mods))

    @classmethod
    def load(cls, path: str, index) -> "KReciprocal":
        """What `save` wrote, for the index it was built from: RuntimeError if that index has changed since."""
        from .index import DeviceIndex
        if not isinstance(index, DeviceIndex):
            raise TypeError("KReciprocal.load needs the pvsim.index.DeviceIndex the lists were built from")
        with np.load(path if str(path).endswith(".npz") else str(path) + ".npz", allow_pickle=False) as z:
            nbr, sim, k1, k2, gamma, mods = z["nbr"], z["sim"], int(z["k1"]), int(z["k2"]), int(z["gamma"]), int(z["index_modifications"])
        if nbr.ndim != 2 or nbr.shape[0] != len(index) or mods != index.modifications:
            raise RuntimeError("the index has changed since the lists were built (rows were added or removed): build a new KReciprocal")
        return cls.from_arrays(nbr, sim, k1, k2, gamma, index)

    def close(self):
        for b in self._b.values():
            b.free()

    # ---- ranking
    def _check_snapshot(self):
        if self.index is None:
            raise RuntimeError("this KReciprocal was made from arrays without an index: it can re-rank lists (rank_lists), not rank")
        if self.index.modifications != self._mods or len(self.index) != self.n:
            raise RuntimeError("the index has changed since the lists were built (rows were added or removed): build a new KReciprocal")

    def _check_rank(self, k, kq, kr, lam):
        kq = _check_int("kq", kq, 1, min(self.n, MAX_KQ))
        kr = kq if kr is None else _check_int("kr", kr, 1, kq)
        k = _check_int("k", k, 1, kr)
        if isinstance(lam, bool) or not isinstance(lam, (int, float, np.integer, np.floating)) or not 0.0 <= lam <= 1.0:
            raise ValueError(f"lam must lie in [0, 1], got {lam!r}")
        return k, kq, kr, float(lam)

    def _rerank_dev(self, tmp, d_qidx, d_qval, nq, k, kq, kr, lam):
        """query + score + ranking of lists that are on the device -> (positions (nq, k) int64, val (nq, k), the report of
        `last_rank`, the buffers of wq, sq and the scores)"""
        b, N, kg, ctx = self._b, self.n, self.kg, self.ctx
        d_wq, d_sq, d_kept, d_drop = tmp(nq * kq * 8), tmp(nq * 8), tmp(nq * 4), tmp(nq * 4)
        d_sc, d_oi, d_ov = tmp(nq * kr * 8), tmp(nq * k * 8), tmp(nq * k * 8)
        ctx.krr_query_dev(b["nbr"].ptr, b["sim"].ptr, b["maskh"].ptr, b["v"].ptr, b["v0"].ptr, N, kg, self.k1, self.k2, self.gamma,
                          d_qidx, d_qval, nq, kq, d_wq.ptr, d_sq.ptr, d_kept.ptr, d_drop.ptr)
        ctx.krr_score_dev(b["nbr"].ptr, b["w"].ptr, b["w0"].ptr, b["ws"].ptr, N, kg, d_qidx, d_qval, d_wq.ptr, d_sq.ptr, nq, kq, kr, lam,
                          d_sc.ptr)
        ctx.rank_f64_dev(d_sc.ptr, nq, kr, kr, k, d_oi.ptr, d_ov.ptr)
        report = {"members": d_kept.download((nq,), np.int32), "dropped": d_drop.download((nq,), np.int32)}
        return d_oi.download((nq, k), np.int64), d_ov.download((nq, k), np.float64), report, d_wq, d_sq, d_sc

    def rank_lists(self, qidx, qval, k: int = 10, kr=None, lam: float = 0.3, details: bool = False):
        """Re-rank first rankings that are given: qidx (nq, kq) integers, qval (nq, kq) float32 -> (idx (nq, k) int64, val (nq, k)
        float64).  `details`: also a dict of wq, sq and the scores (nq, kr), for tests."""
        qidx = np.ascontiguousarray(qidx, dtype=np.int64)
        qval = np.ascontiguousarray(qval)
        if qidx.ndim != 2 or qidx.shape != qval.shape or qval.dtype != np.float32:
            raise ValueError("qidx must be an (nq, kq) integer array and qval a float32 array of the same shape")
        nq = qidx.shape[0]
        k, kq, kr, lam = self._check_rank(k, qidx.shape[1], kr, lam)
        if nq == 0:
            self.last_rank = {"members": np.zeros(0, np.int32), "dropped": np.zeros(0, np.int32)}
            out = np.zeros((0, k), np.int64), np.zeros((0, k), np.float64)
            return out + ({},) if details else out
        with self.ctx.scratch() as tmp:
            pos, val, self.last_rank, d_wq, d_sq, d_sc = self._rerank_dev(tmp, tmp.upload(qidx).ptr, tmp.upload(qval).ptr, nq, k, kq, kr, lam)
            idx = np.take_along_axis(qidx, pos, axis=1)
            if not details:
                return idx, val
            return idx, val, {"wq": d_wq.download((nq, kq), np.float64), "sq": d_sq.download((nq,), np.float64),
                              "scores": d_sc.download((nq, kr), np.float64)}

    def rank(self, query_vecs, k: int = 10, kq: int = 80, kr=None, lam: float = 0.3):
        """The queries are ranked against the index to depth kq by the index's own path; the first kr of those (default kq) are
        scored (1 - lam) Jaccard + lam cosine and ranked again: -> (idx (nq, k) int64, val (nq, k) float64), score descending, then
        the position in the first ranking ascending.  1 <= k <= kr <= kq <= min(N, 1024), 0 <= lam <= 1; lam = 1 is the first
        ranking.  `last_rank` reports the members kept and dropped per query.  Float32 queries (TypeError otherwise)."""
        self._check_snapshot()
        index = self.index
        q = np.asarray(query_vecs)
        if q.ndim != 2 or q.shape[1] != index.shape[1]:
            raise ValueError("query and database dimensions differ")
        if q.dtype != np.float32:
            raise TypeError("k-reciprocal re-ranking ranks the queries in the index's dtype: a float32 index needs float32 queries")
        k, kq, kr, lam = self._check_rank(k, kq, kr, lam)
        nq = q.shape[0]
        if nq == 0:
            self.last_rank = {"members": np.zeros(0, np.int32), "dropped": np.zeros(0, np.int32)}
            return np.zeros((0, k), np.int64), np.zeros((0, k), np.float64)
        with self.ctx.scratch() as tmp:
            d_q = tmp.upload(np.ascontiguousarray(q))
            _, d_idx, d_val = index._rank_dev_buffers(tmp, d_q.ptr, nq, kq)
            pos, val, self.last_rank = self._rerank_dev(tmp, d_idx.ptr, d_val.ptr, nq, k, kq, kr, lam)[:3]
            return np.take_along_axis(d_idx.download((nq, kq), np.int64), pos, axis=1), val
