"""Retrieval metrics with the signatures of pyvisim/eval.py:13-145, batched on the MI355X.

The reference loops over queries in Python: encode one query, cosine against the whole database (which
sklearn re-normalises every time), full argsort, slice k.  Here all queries are encoded together, scored
with ONE Q x N similarity GEMM and ranked with the fused top-k kernel; the label bookkeeping is unchanged.
Ranking order is (score descending, index ascending) -- identical to the reference's lists wherever its
own (non-stable) argsort is unambiguous, i.e. on tie-free scores."""
from __future__ import annotations

from typing import Iterable

import numpy as np

from ._utils import cosine_similarity  # re-exported like the reference's `from ._utils import *`
from .engine import default_context

__all__ = ["retrieve_top_k_similar", "top_k_map", "top_k_accuracy", "rerank_spatial", "expand_verified", "retrieve_similar",
           "find_duplicates"]



def _first_rows(encoder, queries) -> np.ndarray:
    """encoder.encode(query) per query, keeping row 0 (the reference scores `cosine(...)[0]`), stacked."""
    queries = list(queries)
    if queries and all(isinstance(q, np.ndarray) and q.ndim == 3 for q in queries):
        enc = encoder.encode(queries)                       # one batched encode
        return enc.reshape(len(queries), -1) if enc.ndim == 1 else enc
    rows = []
    for q in queries:
        v = encoder.encode(q)
        rows.append(v.reshape(1, -1)[0] if v.ndim == 1 else v[0])
    return np.vstack(rows) if rows else np.zeros((0, 0), np.float32)


def _first_row(encoder, image) -> np.ndarray:
    v = encoder.encode(image)
    return (v.reshape(1, -1) if v.ndim == 1 else v)[:1]


def _clamped(rank, n: int, query_vecs: np.ndarray, k: int | None, dtype=np.float32, **kw):
    """rank(query_vecs, k') with k' = min(k, N) (k=None: all N), or the empty result of scores `dtype`: once, for every kind"""
    kk = n if k is None else max(0, min(int(k), n))
    if query_vecs.shape[0] == 0 or kk == 0:
        return np.zeros((query_vecs.shape[0], 0), np.int64), np.zeros((query_vecs.shape[0], 0), dtype)
    return rank(query_vecs, kk, **kw)


def _check_features(query_vecs: np.ndarray, L: int):
    if query_vecs.shape[-1] <= 1 or L <= 1:
        raise ValueError(f"Cosine similarity requires at least 2 features. Got {query_vecs.shape[-1]} features "
                         f"for x and {L} features for y.")


def _rank(query_vecs: np.ndarray, all_vectors: np.ndarray, k: int | None, ctx=None):
    """-> (indices (nq, k') int64, scores (nq, k')) with k' = min(k, N) (k=None: all N), against a host matrix."""
    def cosine(q, kk):
        _check_features(q, all_vectors.shape[-1])
        c = ctx or default_context()
        # the reference's dtype rule (pyvisim/_utils.py:312-330 -> sklearn): float32 scores iff BOTH operands are float32;
        # anything else (Fisher encodings are float64) is scored and ranked in float64
        if q.dtype == np.float32 and all_vectors.dtype == np.float32:
            return c.cosine_topk(np.ascontiguousarray(q), np.ascontiguousarray(all_vectors), kk)
        return c.cosine_topk_f64(q, all_vectors, kk)
    return _clamped(cosine, all_vectors.shape[0], query_vecs, k)


class _Plan:
    """A dataset resolved once for ranking: `n` rows, `paths` in index order (the index's own list, not a copy), `matrix` (the
    stacked host rows of a dict, None for an index), `index_of(path)` and `rank(query_vecs, k)` -> (idx (nq, k'), val (nq, k'))."""

    def __init__(self, n, paths, rank, matrix=None, index_of=None):
        self.n, self.paths, self.rank, self.matrix, self._index_of = n, paths, rank, matrix, index_of

    def index_of(self, path) -> int:
        if self._index_of is None:                                  # a dict: its positions are made when first asked for
            self._index_of = {p: i for i, p in enumerate(self.paths)}.__getitem__
        return self._index_of(path)


def _check_allowed(dataset, expand, rerank, nprobe, diffuse, reciprocal) -> None:
    """allowed= ranks within a set on a dict, a float32 DeviceIndex and an Int8Index, first stage only: everything else is refused by name"""
    from .asmk import ASMKIndex
    from .compact import CompactIndex
    for name, given in (("expand", expand is not None), ("rerank", bool(rerank)), ("nprobe", nprobe is not None),
                        ("diffuse", diffuse is not None), ("reciprocal", reciprocal is not None)):
        if given:
            raise ValueError(f"allowed= together with {name}= is not built: a subset ranking is the first stage alone")
    if isinstance(dataset, (CompactIndex, ASMKIndex)):
        raise ValueError(f"allowed= on {'an' if type(dataset).__name__[0] in 'AI' else 'a'} {type(dataset).__name__} is not built: subset "
                         "search covers a dict, a float32 DeviceIndex and an Int8Index")


def _no_full_subset_ranking():
    raise ValueError("allowed= together with k=None is not built: a subset ranking is a finite list, pass k")


def _plan_ivf_int8(dataset, expand, rerank, nprobe, diffuse, reciprocal, allowed) -> _Plan:
    """An IVFInt8Index ranks one way, the int8 score over the nprobe best lists of a query: nprobe= is required, k is finite, and
    every other option is refused by name."""
    for name, given, needs in (("allowed", allowed is not None, "subset search covers a dict, a float32 DeviceIndex and an Int8Index"),
                               ("expand", expand is not None, "query expansion needs the full-precision rows of a dict or a DeviceIndex"),
                               ("rerank", bool(rerank), "a second stage needs the kept projected rows of a CompactIndex"),
                               ("diffuse", diffuse is not None, "diffusion runs on the DeviceIndex the graph was built on"),
                               ("reciprocal", reciprocal is not None, "k-reciprocal re-ranking runs on the DeviceIndex the lists were built on")):
        if given:
            raise ValueError(f"{name}= on an IVFInt8Index is not built: {needs}")
    if nprobe is None:
        raise ValueError("an IVFInt8Index scans the nprobe best lists of a query: pass nprobe=")
    n = len(dataset)

    def rank(q, k):
        if k is None:
            raise ValueError("k=None on an IVFInt8Index is not built: it ranks a finite list over the probed lists, pass k (the complete "
                             "ranking needs the full-precision rows -- use a dict or a DeviceIndex for that)")
        return _clamped(lambda q, kk: dataset.rank(q, kk, nprobe), n, q, k)
    return _Plan(n, dataset._ledger.paths, rank, index_of=dataset._ledger.index_of)


def _plan(dataset, expand=None, rerank: int = 0, nprobe=None, diffuse=None, ctx=None, reciprocal=None, allowed=None) -> _Plan:
    """What `dataset` is (a dict, a DeviceIndex, an Int8Index, an IVFInt8Index, a CompactIndex, an IVFCompactIndex), whether it takes these options (every
    refusal is raised here, before anything is encoded), and how it ranks.  A DeviceIndex is never asked for its host rows.
    `allowed`: one set of images for all queries (a pvsim.Subset of the index, indices, a boolean mask or paths); k is then clamped to
    the size of the set.  A dict is cut to the allowed paths here, on the host, and ranked as any dict."""
    from .compact import CompactIndex, IVFCompactIndex
    from .index import DeviceIndex
    from .ivf_int8 import IVFInt8Index
    from .quantized import Int8Index
    if isinstance(dataset, IVFInt8Index):
        return _plan_ivf_int8(dataset, expand, rerank, nprobe, diffuse, reciprocal, allowed)
    if allowed is not None:
        _check_allowed(dataset, expand, rerank, nprobe, diffuse, reciprocal)
    dense, compact = isinstance(dataset, DeviceIndex), isinstance(dataset, CompactIndex)
    int8 = isinstance(dataset, Int8Index)
    if allowed is not None and (dense or int8):
        from .subset import Subset, _index_of, _kind, normalise
        _kind(dataset)                                            # a float64 DeviceIndex: TypeError naming float32
        if isinstance(allowed, Subset):
            allowed.check(dataset)
            size = len(allowed)
        else:                                                     # sorted ids; rank makes and destroys the device copy per call
            allowed = normalise(allowed, len(dataset), _index_of(dataset))
            size = int(allowed.size)

        def within(q, k):
            if k is None:
                _no_full_subset_ranking()
            if dense:
                _check_features(q, dataset.shape[1])
            return _clamped(lambda q, kk: dataset.rank(q, kk, allowed=allowed), size, q, k)
        return _Plan(len(dataset), dataset._ledger.paths, within, index_of=dataset._ledger.index_of)
    if int8:                                      # one ranking, the cosine of the codes: every option names what it needs instead
        if expand is not None:
            raise ValueError("expand= needs the full-precision rows: use a dict or a DeviceIndex, not an Int8Index")
        if rerank:
            raise ValueError("rerank= needs the kept projected rows of a CompactIndex: an Int8Index has no second stage")
        if nprobe is not None:
            raise ValueError("nprobe= needs the inverted lists of an IVFCompactIndex: an Int8Index scans every row")
        if diffuse is not None:
            raise ValueError("diffuse= needs the DeviceIndex the graph was built on, not an Int8Index")
        if reciprocal is not None:
            raise ValueError("reciprocal= needs the DeviceIndex the lists were built on, not an Int8Index")
    if diffuse is not None:                      # the graph's own index only, and none of the other re-ranking options
        from .diffusion import Diffusion
        if not isinstance(diffuse, Diffusion):
            raise TypeError("diffuse must be a pvsim.Diffusion")
        if not dense:
            raise TypeError("diffuse= needs the pvsim.index.DeviceIndex the graph was built on, not a dict or a compact index")
        if diffuse.index is not dataset:
            raise ValueError("diffuse= needs the DeviceIndex the graph was built on: this graph belongs to another index")
        if expand is not None or rerank or nprobe is not None:
            raise ValueError("diffuse= excludes expand=, rerank= and nprobe=")
    if reciprocal is not None:                    # as diffuse=: the lists' own index only, and no other re-ranking option
        from .reciprocal import KReciprocal
        if not isinstance(reciprocal, KReciprocal):
            raise TypeError("reciprocal must be a pvsim.KReciprocal")
        if not dense:
            raise TypeError("reciprocal= needs the pvsim.index.DeviceIndex the lists were built on, not a dict or a compact index")
        if reciprocal.index is not dataset:
            raise ValueError("reciprocal= needs the DeviceIndex the lists were built on: this KReciprocal belongs to another index")
        if expand is not None or rerank or nprobe is not None or diffuse is not None:
            raise ValueError("reciprocal= excludes expand=, rerank=, nprobe= and diffuse=")
    if expand is not None and compact:
        raise ValueError("query expansion needs the full-precision rows: use a dict or a DeviceIndex, not a CompactIndex")
    if rerank and not compact:
        raise ValueError("rerank= applies to a CompactIndex only")
    if isinstance(dataset, IVFCompactIndex):
        if nprobe is None:
            raise ValueError("an IVFCompactIndex scans the nprobe best lists of a query: pass nprobe=")
    elif nprobe is not None:
        raise ValueError("nprobe= applies to an IVFCompactIndex only")

    if compact:                                   # ADC ranking, optionally re-ranked exactly; rerank < k raises in index.rank
        def rank(q, k):
            if k is None:
                raise ValueError("a CompactIndex ranks a finite list: pass k (k=None asks for the complete ranking, which needs the "
                                 "full-precision rows -- use a dict or a DeviceIndex for that)")
            args = () if nprobe is None else (nprobe,)
            return _clamped(lambda q, kk: dataset.rank(q, kk, *args, rerank=rerank), n, q, k)
    elif int8:
        def rank(q, k):
            if k is None:
                raise ValueError("an Int8Index ranks a finite list: pass k (k=None asks for the complete ranking, which needs the "
                                 "full-precision rows -- use a dict or a DeviceIndex for that)")
            return _clamped(dataset.rank, n, q, k)
    elif dense:
        def plain(q, kk):
            _check_features(q, dataset.shape[1])
            return dataset.rank(q, kk)
        if diffuse is not None:
            rank = lambda q, k: _clamped(diffuse.rank, n, q, k, np.float64)
        elif reciprocal is not None:              # rank's own kq where it holds k results, as many candidates as results beyond that
            def reranked(q, kk):
                _check_features(q, dataset.shape[1])
                return reciprocal.rank(q, kk, kq=min(n, max(kk, 80)))       # k beyond the most rank serves is refused there
            rank = lambda q, k: _clamped(reranked, n, q, k, np.float64)
        elif expand is not None:
            rank = lambda q, k, members=None: _clamped(dataset.rank_expanded, n, q, k, qe=expand, members=members)
        else:
            rank = lambda q, k: _clamped(plain, n, q, k)
    else:
        paths, matrix = list(dataset.keys()), np.array(list(dataset.values()))        # stacked as the reference does (eval.py:28)
        if allowed is not None:                                     # the map cut to the allowed paths, in index order
            from .subset import Subset, normalise
            if isinstance(allowed, Subset):
                raise ValueError("a pvsim.Subset belongs to the index it was made for: on a dict pass indices, a boolean mask or paths")
            pos = {p: i for i, p in enumerate(paths)}
            ids = normalise(allowed, len(paths), pos.__getitem__)
            paths, matrix = [paths[i] for i in ids.tolist()], matrix[ids]
            cut = lambda q, k: _no_full_subset_ranking() if k is None else _rank(q, matrix, k, ctx)
            return _Plan(matrix.shape[0], paths, cut, matrix)

        def expanded(q, kk, members=None):                          # on a DeviceIndex that holds the dict for this call
            temp = DeviceIndex(dict(zip(paths, matrix)), ctx or default_context())
            try:
                return temp.rank_expanded(q, kk, expand, members=members)
            finally:
                temp.close()
        if expand is not None:
            rank = lambda q, k, members=None: _clamped(expanded, matrix.shape[0], q, k, members=members)
        else:
            rank = lambda q, k: _rank(q, matrix, k, ctx)            # the module's _rank at the time of the call: tests replace it
        return _Plan(matrix.shape[0], paths, rank, matrix)
    n = len(dataset)
    return _Plan(n, dataset._ledger.paths, rank, index_of=dataset._ledger.index_of)


def retrieve_top_k_similar(uploaded_image: np.ndarray, dataset: dict[str, np.ndarray], encoder,
                           k: int = 5, rerank: int = 0, expand=None, nprobe=None, diffuse=None, reciprocal=None,
                           allowed=None) -> list[tuple[str, float]]:
    """[(image_path, similarity)] of the k most similar database entries, best first.  `rerank=R` (CompactIndex only): the
    ADC top-R re-ranked by the exact cosine of the kept projected rows.  `expand`: a pvsim.expand.QueryExpansion; the list is
    then the ranking of the expanded query (dict or DeviceIndex; a dict is uploaded for the call).  `nprobe` (IVFCompactIndex
    only, and required there): the inverted lists scanned; the list is shorter than k when they hold fewer rows.  `diffuse`: a
    pvsim.Diffusion graph built on `dataset` (a DeviceIndex); the list is then the diffusion ranking and its float64 scores, and
    `rerank`, `expand` and `nprobe` are excluded.  `reciprocal`: a pvsim.KReciprocal built on `dataset` (a DeviceIndex); the list is
    then the k-reciprocal re-ranking of the first max(k, 80) results and its float64 scores, and every other option is excluded.
    `allowed`: rank within this set of images only (a pvsim.Subset of the index, indices, a boolean mask of the entries or paths; a
    dict, a float32 DeviceIndex or an Int8Index; every other option is excluded); k is clamped to the size of the set."""
    plan = _plan(dataset, expand, rerank, nprobe, diffuse, getattr(encoder, "context", None), reciprocal, allowed)
    idx, val = plan.rank(_first_row(encoder, uploaded_image), k)
    return [(plan.paths[i], s) for i, s in zip(idx[0], val[0]) if i >= 0]     # unfilled slots of an IVF list are dropped


class _ResidentF32:
    """`dataset` as the float32 DeviceIndex a threshold search runs on: the index itself, or a dict uploaded for the block (the
    dict-or-DeviceIndex rule of retrieve_top_k_similar).  Anything else is refused by name before the device is touched."""

    def __init__(self, dataset, ctx=None):
        from .duplicates import _check_index
        from .index import DeviceIndex
        self.temp = None
        if isinstance(dataset, dict):
            rows = np.array(list(dataset.values()))
            if rows.dtype != np.float32:
                raise NotImplementedError(f"threshold search runs on a float32 pvsim.index.DeviceIndex: these encodings are {rows.dtype}")
            self.index = self.temp = DeviceIndex(dataset, ctx or default_context())
        else:
            _check_index(dataset)
            self.index = dataset

    def __enter__(self):
        return self.index

    def __exit__(self, *exc):
        if self.temp is not None:
            self.temp.close()


def retrieve_similar(uploaded_image: np.ndarray, dataset, encoder, threshold: float, max_results=None) -> list[tuple[str, float]]:
    """[(image_path, similarity)] of EVERY database entry whose cosine with the image is at least `threshold`, best first: the
    threshold form of retrieve_top_k_similar.  `dataset`: a dict of float32 encodings (uploaded for the call) or a float32 DeviceIndex.
    More than `max_results` entries raise CapacityError carrying their number."""
    from .duplicates import _check_threshold
    _check_threshold(threshold)
    with _ResidentF32(dataset, getattr(encoder, "context", None)) as index:
        q = _first_row(encoder, uploaded_image)
        _check_features(q, index.shape[1])
        _, idx, val = index.range_search(q, threshold, max_results=max_results)
        paths = index._ledger.paths
        return [(paths[i], s) for i, s in zip(idx, val)]


def find_duplicates(dataset, threshold: float) -> list[list[str]]:
    """The groups of near duplicates of `dataset` (a dict of float32 encodings or a float32 DeviceIndex): lists of paths whose
    entries are connected by pairs with cosine at least `threshold`, members in index order, groups by their first member."""
    from .duplicates import _check_threshold, find_duplicates as _find
    _check_threshold(threshold)
    with _ResidentF32(dataset) as index:
        return _find(index, threshold).paths


def expand_verified(uploaded_image: np.ndarray, ranked, index, encoder, k: int = 5, qe=None,
                    min_inliers: int = 4) -> list[tuple[str, float]]:
    """Query expansion over spatially verified results (Chum et al., ICCV 2007): `ranked` is what `rerank_spatial` returned,
    [(image_path, similarity, inliers)]; its first `qe.n` entries with at least `min_inliers` inliers are folded into the query
    (pvsim.expand.QueryExpansion; the default is average expansion over 10), and the k best entries of `index` (a dict or a
    DeviceIndex) for the expanded query come back as [(image_path, similarity)].  With no verified entry there is nothing to
    expand with: the first k of `ranked`, without the inlier counts."""
    from .expand import QueryExpansion
    qe = QueryExpansion() if qe is None else qe
    if not isinstance(qe, QueryExpansion):
        raise TypeError("qe must be a pvsim.expand.QueryExpansion")
    if isinstance(min_inliers, bool) or int(min_inliers) != min_inliers or min_inliers < 0:
        raise ValueError(f"min_inliers must be a non-negative integer, got {min_inliers!r}")
    if isinstance(k, bool) or int(k) != k or k < 0:
        raise ValueError(f"k must be a non-negative integer, got {k!r}")
    plan = _plan(index, expand=qe, ctx=getattr(encoder, "context", None))
    ranked = list(ranked)
    verified = [path for path, _, inliers in ranked if inliers >= min_inliers][:qe.n]
    if not verified or min(int(k), plan.n) == 0:
        return [(path, sim) for path, sim, _ in ranked[:k]]
    members = np.full((1, min(qe.n, plan.n)), -1, np.int64)
    members[0, :len(verified)] = [plan.index_of(p) for p in verified]
    idx, val = plan.rank(_first_row(encoder, uploaded_image), k, members=members)
    return [(plan.paths[i], s) for i, s in zip(idx[0], val[0])]


def rerank_spatial(uploaded_image: np.ndarray, hits, local_index, verifier, k: int | None = None,
                   min_inliers: int = 4) -> list[tuple[str, float, int]]:
    """Re-order the shortlist `retrieve_top_k_similar` returned by geometric verification (pvsim.verify):
    the candidates with at least `min_inliers` inliers first, by inliers descending (ties in their incoming order), the others
    behind them in their incoming order.  -> [(image_path, similarity, inliers)], the first k (all if None).
    KeyError if `local_index` does not hold one of the paths."""
    if isinstance(min_inliers, bool) or int(min_inliers) != min_inliers or min_inliers < 0:
        raise ValueError(f"min_inliers must be a non-negative integer, got {min_inliers!r}")
    if k is not None and (isinstance(k, bool) or int(k) != k or k < 0):
        raise ValueError(f"k must be a non-negative integer or None, got {k!r}")
    hits = list(hits)
    for path, _ in hits:
        if path not in local_index:
            raise KeyError(path)
    results = verifier.verify(uploaded_image, local_index, [path for path, _ in hits]) if hits else []
    scored = [(path, sim, int(r.inliers)) for (path, sim), r in zip(hits, results)]
    front = sorted((h for h in scored if h[2] >= min_inliers), key=lambda h: -h[2])        # sorted() is stable
    back = [h for h in scored if h[2] < min_inliers]
    return (front + back)[:k]


def _ranked_labels(images, encoding_map, path_labels_dict, encoder, k, expand, rerank, nprobe, diffuse, reciprocal=None, allowed=None):
    """-> (ranked indices (nq, k'), -1 in the unfilled slots at the end of an IVF list; the label of every database entry)"""
    plan = _plan(encoding_map, expand, rerank, nprobe, diffuse, getattr(encoder, "context", None), reciprocal, allowed)
    idx, _ = plan.rank(_first_rows(encoder, images), k)
    return idx, [path_labels_dict[p] for p in plan.paths]


def top_k_map(images: Iterable[np.ndarray], image_labels: Iterable[int], encoding_map: dict[str, np.ndarray],
              path_labels_dict: dict[str, int], encoder, k: int = None, expand=None, rerank: int = 0, nprobe=None, diffuse=None,
              reciprocal=None, allowed=None) -> float:
    """Mean average precision; R is counted inside the (possibly truncated) ranked list (eval.py:95).  `expand`: rank the
    expanded queries (pvsim.expand.QueryExpansion).  `rerank` (a CompactIndex) and `nprobe` (an IVFCompactIndex, required
    there), `diffuse` (a pvsim.Diffusion graph of the DeviceIndex) and `reciprocal` (a pvsim.KReciprocal of it) as in
    retrieve_top_k_similar.  `allowed`: one set of database images for all queries, as there (k is required then)."""
    labels = list(image_labels)
    idx, db_labels = _ranked_labels(images, encoding_map, path_labels_dict, encoder, k, expand, rerank, nprobe, diffuse, reciprocal, allowed)
    aps = []
    for row, true_label in zip(idx, labels):
        relevant_count, precision_sum = 0, 0.0
        for rank, i in enumerate(row, start=1):
            if i >= 0 and db_labels[i] == true_label:                # i < 0: an unfilled slot at the end of an IVF list
                relevant_count += 1
                precision_sum += relevant_count / rank
        aps.append(precision_sum / relevant_count if relevant_count > 0 else 0.0)
    return float(np.mean(aps))


def top_k_accuracy(images: Iterable[np.ndarray], image_labels: Iterable[int], encoding_map: dict[str, np.ndarray],
                   path_labels_dict: dict[str, int], encoder, k: int, expand=None, rerank: int = 0, nprobe=None, diffuse=None,
                   reciprocal=None, allowed=None) -> float:
    """Fraction of queries with at least one same-label entry among their k nearest (eval.py:102-145).  `expand`: rank the
    expanded queries (pvsim.expand.QueryExpansion).  `rerank` (a CompactIndex) and `nprobe` (an IVFCompactIndex, required
    there), `diffuse` (a pvsim.Diffusion graph of the DeviceIndex) and `reciprocal` (a pvsim.KReciprocal of it) as in
    retrieve_top_k_similar.  `allowed`: one set of database images for all queries, as there."""
    images = list(images)
    labels = list(image_labels)
    idx, db_labels = _ranked_labels(images, encoding_map, path_labels_dict, encoder, k, expand, rerank, nprobe, diffuse, reciprocal, allowed)
    correct = sum(1 for row, true_label in zip(idx, labels) if any(i >= 0 and db_labels[i] == true_label for i in row))
    return float(correct / len(images))
