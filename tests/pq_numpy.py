"""NumPy twin of the compact index (include/pvsim.h): encode, table, score, ranking, rescore, decode.

Every value is produced by np.float32 ELEMENT operations in the defined order -- explicit loops over t and s, one rounding per
multiply and one per add, no np.sum, no @ -- vectorised only across independent rows / codewords / queries, which does not
change any rounding.  The device kernels must agree with this bit for bit."""
import numpy as np

import topk_numpy as tk

F = np.float32


def _f32(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a


def encode(x, codebooks):
    """x (n, d) f32, codebooks (m, ksub, dsub) f32 -> uint8 (n, m).  acc_j from +0, t ascending; ties to the lowest j."""
    x, cb = _f32(x), _f32(codebooks)
    m, ksub, dsub = cb.shape
    n = x.shape[0]
    assert x.shape[1] == m * dsub
    codes = np.zeros((n, m), np.uint8)
    for s in range(m):
        acc = np.zeros((n, ksub), F)
        for t in range(dsub):
            df = x[:, s * dsub + t][:, None] - cb[s, :, t][None, :]         # float32 - float32 -> float32
            acc = acc + df * df                                             # one rounding for the product, one for the sum
        best = acc[:, 0].copy()
        bj = np.zeros(n, np.int64)
        for j in range(1, ksub):
            better = acc[:, j] < best                                       # strict: the lowest j keeps a tie
            best = np.where(better, acc[:, j], best)
            bj = np.where(better, j, bj)
        codes[:, s] = bj
    return codes


def decode(codes, codebooks):
    cb = _f32(codebooks)
    codes = np.asarray(codes)
    return np.concatenate([cb[s][codes[:, s].astype(np.int64)] for s in range(cb.shape[0])], axis=1)


def lut(q, codebooks):
    """q (nq, d) -> (nq, m, ksub): from +0, adds q[s dsub + t] * c[s][j][t] for t ascending."""
    q, cb = _f32(q), _f32(codebooks)
    m, ksub, dsub = cb.shape
    out = np.zeros((q.shape[0], m, ksub), F)
    for s in range(m):
        acc = np.zeros((q.shape[0], ksub), F)
        for t in range(dsub):
            acc = acc + q[:, s * dsub + t][:, None] * cb[s, :, t][None, :]
        out[:, s, :] = acc
    return out


def scores(table, codes, inv_q=None, inv_db=None):
    """table (nq, m, ksub), codes (N, m) -> (nq, N): sum from +0 over s ascending, then (sum * inv_q) * inv_db."""
    table = _f32(table)
    codes = np.asarray(codes)
    nq, m, _ = table.shape
    N = codes.shape[0]
    acc = np.zeros((nq, N), F)
    for s in range(m):
        acc = acc + table[:, s, :][:, codes[:, s].astype(np.int64)]
    iq = np.ones(nq, F) if inv_q is None else _f32(inv_q)
    idb = np.ones(N, F) if inv_db is None else _f32(inv_db)
    return (acc * iq[:, None]) * idb[None, :]


def topk(score, k, col_offset=0):
    """(score descending, global index ascending), NaN last -> idx int64 (nq, k), val f32 (nq, k): the rule of topk_numpy."""
    return tk.topk(_f32(score), k, col_offset)


def rescore(Q, X, cand, inv_q=None, inv_db=None):
    """Exact cosine of query q with rows cand[q]: dot in ascending t, then (dot * inv_q) * inv_db; cand < 0 -> -inf."""
    Q, X = _f32(Q), _f32(X)
    cand = np.asarray(cand, np.int64)
    nq, R = cand.shape
    safe = np.where(cand < 0, 0, cand)
    acc = np.zeros((nq, R), F)
    for t in range(Q.shape[1]):
        acc = acc + Q[:, t][:, None] * X[safe, t]
    iq = np.ones(nq, F) if inv_q is None else _f32(inv_q)
    idb = np.ones(X.shape[0], F) if inv_db is None else _f32(inv_db)
    out = (acc * iq[:, None]) * idb[safe]
    return np.where(cand < 0, F(-np.inf), out).astype(F)


def rerank(cand, exact, k):
    """candidates + their exact scores -> the first k by (exact score descending, index ascending), NaN last."""
    idx = np.empty((cand.shape[0], k), np.int64)
    val = np.empty((cand.shape[0], k), F)
    for r in range(cand.shape[0]):
        nan = np.isnan(exact[r])
        key = np.where(nan, F(-np.inf), exact[r])
        o = np.lexsort((cand[r], -key, nan))[:k]
        idx[r], val[r] = cand[r][o], exact[r][o]
    return idx, val
