"""NumPy twin of subset search (include/pvsim.h): the definition restated literally.

The subset ranking of a query is the index's FULL ranking -- (score descending, index ascending), -0 and +0 tied -- with the rows
outside S deleted, cut to k.  Indices stay in the numbering of the full index; a score is the one the full ranking reports (the top-k
kernels report a zero as +0).  Also the mask words of the handle, the three forms of `allowed`, and what the device reports in h_stats."""
import numpy as np


def restricted_topk(scores, ids, k):
    """scores float32 (nq, N), ids the allowed rows -> (idx int64 (nq, k), val float32 (nq, k))"""
    scores = np.asarray(scores, np.float32)
    nq, N = scores.shape
    allowed = np.zeros(N, bool)
    allowed[np.asarray(ids, np.int64)] = True
    assert 1 <= k <= int(allowed.sum())
    cols = np.arange(N, dtype=np.int64)
    idx, val = np.empty((nq, k), np.int64), np.empty((nq, k), np.float32)
    for r in range(nq):
        order = np.lexsort((cols, -scores[r]))              # the full ranking: -0.0 == 0.0 for the sort, the index decides
        order = order[allowed[order]][:k]                   # delete the rows outside S, cut
        idx[r], val[r] = order, scores[r][order] + np.float32(0)
    return idx, val


def brute_force(scores, ids, k):
    """the same lists by repeated selection, without a sort: for the twin's own test"""
    scores = np.asarray(scores, np.float32)
    out_i, out_v = [], []
    for r in range(scores.shape[0]):
        left, row_i, row_v = sorted(set(int(i) for i in ids)), [], []
        for _ in range(k):
            best = left[0]
            for j in left[1:]:
                if scores[r, j] > scores[r, best]:          # a tie keeps the smaller index: `left` ascends
                    best = j
            left.remove(best)
            row_i.append(best), row_v.append(scores[r, best] + np.float32(0))
        out_i.append(row_i), out_v.append(row_v)
    return np.array(out_i, np.int64), np.array(out_v, np.float32)


def bitmask(ids, N):
    """uint32 words (ceil(N / 32),): row i is bit i & 31 of word i >> 5; the bits beyond N are zero"""
    words = np.zeros((N + 31) // 32, np.uint32)
    for i in np.asarray(ids, np.int64).tolist():
        assert 0 <= i < N
        words[i >> 5] |= np.uint32(1 << (i & 31))
    return words


def normalise(allowed, N, paths=None):
    """the three forms of `allowed` -> sorted int64 ids: a boolean mask of length N; integer indices in any order (IndexError out of
    range, ValueError for a duplicate); paths looked up in `paths` (KeyError unknown, ValueError named twice); ValueError when empty"""
    items = list(allowed) if not isinstance(allowed, np.ndarray) else allowed.tolist()
    if isinstance(allowed, np.ndarray) and allowed.ndim != 1:
        raise ValueError("1-d only")
    if items and all(isinstance(v, (bool, np.bool_)) for v in items):
        if len(items) != N:
            raise ValueError("mask length")
        ids = [i for i, v in enumerate(items) if v]
    elif items and all(isinstance(v, (int, np.integer)) for v in items):
        for v in items:
            if not 0 <= v < N:
                raise IndexError(v)
        if len(set(items)) != len(items):
            raise ValueError("duplicate index")
        ids = sorted(int(v) for v in items)
    elif items:
        pos = {p: i for i, p in enumerate(paths)}
        ids = []
        for p in items:
            if p not in pos:
                raise KeyError(p)
            if pos[p] in ids:
                raise ValueError("duplicate path")
            ids.append(pos[p])
        ids.sort()
    else:
        ids = []
    if not ids:
        raise ValueError("empty set")
    return np.array(ids, np.int64)


def blocks(n, step):
    return [(a, min(step, n - a)) for a in range(0, n, step)]


def mask_stats(ids, nq, N, QT, NC):
    """h_stats of the mask path over row blocks of QT and column panels of NC: [1, scored, skipped, 0]; a panel counts once per row block"""
    ids = np.asarray(ids)
    empty = sum(1 for c0, cn in blocks(N, NC) if not ((ids >= c0) & (ids < c0 + cn)).any())
    nqb, ncb = len(blocks(nq, QT)), len(blocks(N, NC))
    return [1, nqb * (ncb - empty), nqb * empty, 0]


def listed_stats(ns, chunk):
    """h_stats of the listed path with chunks of `chunk` ids: [2, chunks, 0, ns]"""
    return [2, len(blocks(ns, chunk)), 0, ns]
