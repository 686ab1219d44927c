"""NumPy twin of the inverted lists of the compact index (include/pvsim.h): assignment, residual, storage,
coarse terms, probes, the probed ADC score and its ranking.

As in pq_numpy (imported as it is): every value comes from np.float32 ELEMENT operations in the defined order, vectorised only
across independent rows / centroids / queries.  The device kernels must agree with this bit for bit."""
import numpy as np

import pq_numpy as pq
import topk_numpy as tk

F = np.float32


def assign(x, centroids, chunk=512):
    """x (n, d), centroids (nlist, d) -> (list int32 (n,), residual f32 (n, d)).  acc_l from +0, t ascending; ties to the lowest l;
    the residual is one subtraction per element."""
    x, c = pq._f32(x), pq._f32(centroids)
    n, d = x.shape
    nlist = c.shape[0]
    assert c.shape[1] == d
    lists = np.zeros(n, np.int32)
    for r0 in range(0, n, chunk):
        xs = x[r0:r0 + chunk]
        acc = np.zeros((len(xs), nlist), F)
        for t in range(d):
            df = xs[:, t][:, None] - c[:, t][None, :]
            acc = acc + df * df
        best = acc[:, 0].copy()
        bl = np.zeros(len(xs), np.int64)
        for l in range(1, nlist):
            better = acc[:, l] < best                                       # strict: the lowest l keeps a tie
            best = np.where(better, acc[:, l], best)
            bl = np.where(better, l, bl)
        lists[r0:r0 + chunk] = bl
    return lists, x - c[lists]


def coarse(q, centroids):
    """q (nq, d) -> (nq, nlist): from +0, adds q[t] * C[l][t] for t ascending."""
    q, c = pq._f32(q), pq._f32(centroids)
    acc = np.zeros((q.shape[0], c.shape[0]), F)
    for t in range(q.shape[1]):
        acc = acc + q[:, t][:, None] * c[:, t][None, :]
    return acc


def sort_into_lists(lists, nlist):
    """list of every row -> (ids int32 (N,): original index of each stored row, sorted by (list, original index); list_off int64)"""
    lists = np.asarray(lists)
    ids = np.lexsort((np.arange(len(lists)), lists)).astype(np.int32)
    list_off = np.zeros(nlist + 1, np.int64)
    for l in range(nlist):
        list_off[l + 1] = list_off[l] + int((lists == l).sum())
    return ids, list_off


def probes(coarse_terms, nprobe):
    """-> (list numbers int64 (nq, nprobe), their coarse terms): the rule of pvs_topk_dev"""
    return pq.topk(coarse_terms, nprobe)


def search(table, coarse_terms, nprobe, list_off, ids, codes, inv_q, inv_db, k):
    """table (nq, m, ksub); coarse_terms (nq, nlist); codes (N, m), inv_db (N,) and ids (N,) in STORED order -> idx int64 (nq, k),
    val f32 (nq, k): per probed row, sum from the coarse term of its list over s ascending, then (sum * inv_q) * inv_db; ranked
    by (score descending, ORIGINAL index ascending), NaN last; slots the probed lists cannot fill are -1 / -inf."""
    table = pq._f32(table)
    codes = np.asarray(codes)
    nq, m, _ = table.shape
    iq = np.ones(nq, F) if inv_q is None else pq._f32(inv_q)
    idb = np.ones(len(codes), F) if inv_db is None else pq._f32(inv_db)
    plist, pval = probes(coarse_terms, nprobe)
    idx = np.empty((nq, k), np.int64)
    val = np.empty((nq, k), F)
    for q in range(nq):
        rows = np.concatenate([np.arange(list_off[l], list_off[l + 1]) for l in plist[q]]).astype(np.int64)
        acc = np.concatenate([np.full(int(list_off[l + 1] - list_off[l]), v, F) for l, v in zip(plist[q], pval[q])]).astype(F)
        for s in range(m):
            acc = acc + table[q, s, :][codes[rows, s].astype(np.int64)]
        idx[q], val[q] = tk.rank_row(ids[rows].astype(np.int64), (acc * iq[q]) * idb[rows], k)
    return idx, val
