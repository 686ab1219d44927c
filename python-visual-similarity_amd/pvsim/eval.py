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

__all__ = ["retrieve_top_k_similar", "top_k_map", "top_k_accuracy", "rerank_spatial", "expand_verified"]



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


def _vectors_and_paths(encoding_map):
    """-> ((N, L) matrix, paths, resident index or None).  A pvsim.index.DeviceIndex already holds the matrix (and a normalised
    copy on the GPU); a plain dict is stacked the way the reference does it (eval.py:28)."""
    from .compact import CompactIndex
    from .index import DeviceIndex
    if isinstance(encoding_map, DeviceIndex):
        return encoding_map.matrix, list(encoding_map.keys()), encoding_map
    if isinstance(encoding_map, CompactIndex):             # codes only: there is no host matrix, N comes from len()
        return None, encoding_map.paths, encoding_map
    return np.array(list(encoding_map.values())), list(encoding_map.keys()), None


def _check_nprobe(index, nprobe):
    """nprobe= goes with an IVFCompactIndex, and only with one"""
    from .compact import IVFCompactIndex
    if isinstance(index, IVFCompactIndex):
        if nprobe is None:
            raise ValueError("an IVFCompactIndex scans the nprobe best lists of a query: pass nprobe=")
    elif nprobe is not None:
        raise ValueError("nprobe= applies to an IVFCompactIndex only")


def _rank_compact(query_vecs: np.ndarray, index, k: int | None, rerank: int = 0, nprobe=None):
    """_rank against a pvsim.compact.CompactIndex (ADC ranking, optionally re-ranked exactly on the ADC top-`rerank`); an
    IVFCompactIndex takes `nprobe` as well, and its lists may end in unfilled slots (index -1)."""
    _check_nprobe(index, nprobe)
    if k is None:
        raise ValueError("a CompactIndex ranks a finite list: pass k (k=None asks for the complete ranking, which needs the "
                         "full-precision rows -- use a dict or a DeviceIndex for that)")
    kk = max(0, min(int(k), len(index)))
    if query_vecs.shape[0] == 0 or kk == 0:
        return np.zeros((query_vecs.shape[0], 0), np.int64), np.zeros((query_vecs.shape[0], 0), np.float32)
    if nprobe is not None:
        return index.rank(query_vecs, kk, nprobe, rerank=rerank)
    return index.rank(query_vecs, kk, rerank=rerank)             # rerank < k raises there, as it does for a direct call


def _rank_expanded(query_vecs: np.ndarray, all_vectors: np.ndarray, paths, k: int, ctx, resident, expand, members=None):
    """_rank with query expansion (pvsim.expand): on the resident index, or on a DeviceIndex that holds the dict for this call."""
    from .index import DeviceIndex
    if resident is not None:
        return resident.rank_expanded(query_vecs, k, expand, members=members)
    temp = DeviceIndex(dict(zip(paths, all_vectors)), ctx or default_context())
    try:
        return temp.rank_expanded(query_vecs, k, expand, members=members)
    finally:
        temp.close()


def _no_compact_expansion(all_vectors, expand):
    if expand is not None and all_vectors is None:
        raise ValueError("query expansion needs the full-precision rows: use a dict or a DeviceIndex, not a CompactIndex")


def _rank_diffused(query_vecs: np.ndarray, index, k: int | None, diffuse, expand=None, rerank: int = 0, nprobe=None):
    """_rank through a pvsim.Diffusion graph: the graph's own index only, and none of the other re-ranking options"""
    from .diffusion import Diffusion
    from .index import DeviceIndex
    if not isinstance(diffuse, Diffusion):
        raise TypeError("diffuse must be a pvsim.Diffusion")
    if not isinstance(index, DeviceIndex):
        raise TypeError("diffuse= needs the pvsim.index.DeviceIndex the graph was built on, not a dict or a compact index")
    if diffuse.index is not index:
        raise ValueError("diffuse= needs the DeviceIndex the graph was built on: this graph belongs to another index")
    if expand is not None or rerank or nprobe is not None:
        raise ValueError("diffuse= excludes expand=, rerank= and nprobe=")
    n = len(index)
    kk = n if k is None else max(0, min(int(k), n))
    if query_vecs.shape[0] == 0 or kk == 0:
        return np.zeros((query_vecs.shape[0], 0), np.int64), np.zeros((query_vecs.shape[0], 0), np.float64)
    return diffuse.rank(query_vecs, kk)


def _rank(query_vecs: np.ndarray, all_vectors: np.ndarray, k: int | None, ctx=None, resident=None, rerank: int = 0, nprobe=None):
    """-> (indices (nq, k') int64, scores (nq, k')) with k' = min(k, N) (k=None: all N)."""
    if all_vectors is None:                                     # a CompactIndex: no host matrix
        return _rank_compact(query_vecs, resident, k, rerank, nprobe)
    if rerank:
        raise ValueError("rerank= applies to a CompactIndex only")
    _check_nprobe(resident, nprobe)
    n = all_vectors.shape[0]
    kk = n if k is None else max(0, min(int(k), n))
    if query_vecs.shape[0] == 0 or kk == 0:
        return np.zeros((query_vecs.shape[0], 0), np.int64), np.zeros((query_vecs.shape[0], 0), np.float32)
    if query_vecs.shape[-1] <= 1 or all_vectors.shape[-1] <= 1:
        raise ValueError(f"Cosine similarity requires at least 2 features. Got {query_vecs.shape[-1]} features "
                         f"for x and {all_vectors.shape[-1]} features for y.")
    if resident is not None:
        return resident.rank(query_vecs, kk)
    ctx = ctx or default_context()
    # the reference's dtype rule (pyvisim/_utils.py:312-330 -> sklearn): float32 scores iff BOTH operands are float32;
    # anything else (Fisher encodings are float64) is scored and ranked in float64
    if query_vecs.dtype == np.float32 and all_vectors.dtype == np.float32:
        return ctx.cosine_topk(np.ascontiguousarray(query_vecs), np.ascontiguousarray(all_vectors), kk)
    return ctx.cosine_topk_f64(query_vecs, all_vectors, kk)


def _rank_maybe_expanded(query_vecs: np.ndarray, all_vectors: np.ndarray, paths, k: int | None, ctx, resident, expand, rerank: int = 0,
                         nprobe=None):
    """_rank, or with `expand` (a pvsim.expand.QueryExpansion) the ranking of the expanded queries: same k' and same empty results"""
    if expand is None:
        if not rerank and nprobe is None:
            return _rank(query_vecs, all_vectors, k, ctx, resident)
        return _rank(query_vecs, all_vectors, k, ctx, resident, rerank, nprobe)
    if rerank:
        raise ValueError("rerank= applies to a CompactIndex only")
    _check_nprobe(resident, nprobe)
    _no_compact_expansion(all_vectors, expand)
    n = all_vectors.shape[0]
    kk = n if k is None else max(0, min(int(k), n))
    if query_vecs.shape[0] == 0 or kk == 0:
        return np.zeros((query_vecs.shape[0], 0), np.int64), np.zeros((query_vecs.shape[0], 0), np.float32)
    return _rank_expanded(query_vecs, all_vectors, paths, kk, ctx, resident, expand)


def retrieve_top_k_similar(uploaded_image: np.ndarray, dataset: dict[str, np.ndarray], encoder,
                           k: int = 5, rerank: int = 0, expand=None, nprobe=None, diffuse=None) -> list[tuple[str, float]]:
    """[(image_path, similarity)] of the k most similar database entries, best first.  `rerank=R` (CompactIndex only): the
    ADC top-R re-ranked by the exact cosine of the kept projected rows.  `expand`: a pvsim.expand.QueryExpansion; the list is
    then the ranking of the expanded query (dict or DeviceIndex; a dict is uploaded for the call).  `nprobe` (IVFCompactIndex
    only, and required there): the inverted lists scanned; the list is shorter than k when they hold fewer rows.  `diffuse`: a
    pvsim.Diffusion graph built on `dataset` (a DeviceIndex); the list is then the diffusion ranking and its float64 scores, and
    `rerank`, `expand` and `nprobe` are excluded."""
    if diffuse is not None:
        _rank_diffused(np.zeros((0, 0)), dataset, 0, diffuse, expand, rerank, nprobe)          # refuse before anything is encoded
    all_vectors, all_paths, resident = _vectors_and_paths(dataset)
    _no_compact_expansion(all_vectors, expand)
    query_vector = encoder.encode(uploaded_image)
    if query_vector.ndim == 1:
        query_vector = query_vector.reshape(1, -1)
    if diffuse is not None:
        idx, val = _rank_diffused(query_vector[:1], dataset, k, diffuse)
    elif all_vectors is None:                                     # a CompactIndex: the only index that can re-rank
        idx, val = _rank_compact(query_vector[:1], resident, k, rerank, nprobe)
    else:
        if rerank:
            raise ValueError("rerank= applies to a CompactIndex only")
        _check_nprobe(resident, nprobe)
        idx, val = _rank_maybe_expanded(query_vector[:1], all_vectors, all_paths, k, getattr(encoder, "context", None), resident, expand)
    return [(all_paths[i], s) for i, s in zip(idx[0], val[0]) if i >= 0]      # unfilled slots of an IVF list are dropped


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
    all_vectors, all_paths, resident = _vectors_and_paths(index)
    _no_compact_expansion(all_vectors, qe)
    ranked = list(ranked)
    verified = [path for path, _, inliers in ranked if inliers >= min_inliers][:qe.n]
    kk = min(int(k), len(all_paths))
    if not verified or kk == 0:
        return [(path, sim) for path, sim, _ in ranked[:k]]
    pos = resident._pos if resident is not None else {p: i for i, p in enumerate(all_paths)}
    members = np.full((1, min(qe.n, len(all_paths))), -1, np.int64)
    members[0, :len(verified)] = [pos[p] for p in verified]
    query_vector = encoder.encode(uploaded_image)
    if query_vector.ndim == 1:
        query_vector = query_vector.reshape(1, -1)
    idx, val = _rank_expanded(query_vector[:1], all_vectors, all_paths, kk, getattr(encoder, "context", None), resident, qe, members)
    return [(all_paths[i], s) for i, s in zip(idx[0], val[0])]


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


def top_k_map(images: Iterable[np.ndarray], image_labels: Iterable[int], encoding_map: dict[str, np.ndarray],
              path_labels_dict: dict[str, int], encoder, k: int = None, expand=None, rerank: int = 0, nprobe=None, diffuse=None) -> float:
    """Mean average precision; R is counted inside the (possibly truncated) ranked list (eval.py:95).  `expand`: rank the
    expanded queries (pvsim.expand.QueryExpansion).  `rerank` (a CompactIndex) and `nprobe` (an IVFCompactIndex, required
    there) and `diffuse` (a pvsim.Diffusion graph of the DeviceIndex) as in retrieve_top_k_similar."""
    if diffuse is not None:
        _rank_diffused(np.zeros((0, 0)), encoding_map, 0, diffuse, expand, rerank, nprobe)     # refuse before anything is encoded
    all_vectors, all_paths, resident = _vectors_and_paths(encoding_map)
    _no_compact_expansion(all_vectors, expand)
    labels = list(image_labels)
    q = _first_rows(encoder, images)
    if diffuse is not None:
        idx, _ = _rank_diffused(q, encoding_map, k, diffuse)
    else:
        idx, _ = _rank_maybe_expanded(q, all_vectors, all_paths, k, getattr(encoder, "context", None), resident, expand, rerank, nprobe)
    db_labels = [path_labels_dict[p] for p in all_paths]
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
                   path_labels_dict: dict[str, int], encoder, k: int, expand=None, rerank: int = 0, nprobe=None, diffuse=None) -> float:
    """Fraction of queries with at least one same-label entry among their k nearest (eval.py:102-145).  `expand`: rank the
    expanded queries (pvsim.expand.QueryExpansion).  `rerank` (a CompactIndex) and `nprobe` (an IVFCompactIndex, required
    there) and `diffuse` (a pvsim.Diffusion graph of the DeviceIndex) as in retrieve_top_k_similar."""
    if diffuse is not None:
        _rank_diffused(np.zeros((0, 0)), encoding_map, 0, diffuse, expand, rerank, nprobe)     # refuse before anything is encoded
    all_vectors, all_paths, resident = _vectors_and_paths(encoding_map)
    _no_compact_expansion(all_vectors, expand)
    images = list(images)
    labels = list(image_labels)
    q = _first_rows(encoder, images)
    if diffuse is not None:
        idx, _ = _rank_diffused(q, encoding_map, k, diffuse)
    else:
        idx, _ = _rank_maybe_expanded(q, all_vectors, all_paths, k, getattr(encoder, "context", None), resident, expand, rerank, nprobe)
    db_labels = [path_labels_dict[p] for p in all_paths]
    correct = sum(1 for row, true_label in zip(idx, labels) if any(i >= 0 and db_labels[i] == true_label for i in row))
    return float(correct / len(images))
