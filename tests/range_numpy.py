"""NumPy twin of the cosine threshold join and the pair components (include/pvsim.h).  Everything works from a
float32 score matrix S (nq, N): what the device thresholds panel by panel, the twin thresholds whole.  A hit is S[i, j] >= t compared
in float32 (a NaN is never one, -0 >= 0 holds), the returned score is the stored one, and the self-join keeps j > i.  Corpus builders
for the tests: a lattice whose scores are exact multiples of 1/16, and a band of planted pairs around a threshold."""
import numpy as np


def eps(L: int) -> float:
    """the proven bound |s16 - s32| <= eps(L) of the fp16 prefilter for normalised scores ("Filtered top-k")"""
    return (9.77e-4 * (1.0 + 1.0 / 4096.0) + (1088.0 + L / 1024.0 + 2.0 * ((L + 32767) // 32768)) * 1.1920929e-7
            + 2.98e-8 * np.sqrt(float(L)))


def hits(S, t, upper=False):
    """-> (row int64, col int64, val float32) of every hit, in (row, col) order; upper: only col > row"""
    S = np.asarray(S, np.float32)
    with np.errstate(invalid="ignore"):
        mask = S >= np.float32(t)
    if upper:
        mask &= np.arange(S.shape[1])[None, :] > np.arange(S.shape[0])[:, None]
    row, col = np.nonzero(mask)                                     # row-major: (row, col) ascending
    return row.astype(np.int64), col.astype(np.int64), S[row, col]


def csr(S, t):
    """-> (indptr int64 (nq + 1,), indices int64, scores float32): per query (score descending, index ascending), -0 and +0 tied"""
    row, col, val = hits(S, t)
    order = np.lexsort((col, -val, row))
    indptr = np.zeros(S.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(row, minlength=S.shape[0]), out=indptr[1:])
    return indptr, col[order], val[order]


def upper_pairs(S, t):
    """the self-join: (i, j, score) with i < j in (i, j) order"""
    return hits(S, t, upper=True)


def tile_order(S, t, QT, NC, upper=False):
    """the device's order for row blocks of QT and column panels of NC: row blocks ascending, within a row block column panels
    ascending, within a tile (row, col) ascending"""
    S = np.asarray(S, np.float32)
    rows, cols, vals = [], [], []
    for q0 in range(0, S.shape[0], QT):
        for c0 in range(0, S.shape[1], NC):
            r, c, v = hits(S[q0:q0 + QT, c0:c0 + NC], t)
            r, c = r + q0, c + c0
            keep = c > r if upper else np.ones(r.shape, bool)
            rows.append(r[keep]), cols.append(c[keep]), vals.append(v[keep])
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)


def skipped_tiles(nq, N, QT, NC):
    """tiles of the self-join that lie entirely on or below the diagonal: c0 + cn <= q0 + 1"""
    return sum(1 for q0 in range(0, nq, QT) for c0 in range(0, N, NC) if min(c0 + NC, N) <= q0 + 1)


def union_find_labels(n, a, b):
    """label[i] = the smallest node of i's component of the undirected pairs (a[e], b[e]) over n nodes -> int64 (n,)"""
    parent = list(range(n))

    def root(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for x, y in zip(np.asarray(a).tolist(), np.asarray(b).tolist()):
        rx, ry = root(x), root(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    return np.array([root(i) for i in range(n)], np.int64)


def groups(labels, min_size=2):
    """index arrays, members ascending, groups by first member, at least min_size members"""
    labels = np.asarray(labels)
    return [np.flatnonzero(labels == l) for l in np.unique(labels) if (labels == l).sum() >= min_size]


def lattice(n, L, seed):
    """(n, L) float32 rows in {0, +-1} with 16 non-zeros each: the norm is 4, the inverse norm exactly 0.25, and a score is dot / 16
    exactly in float32 whatever the order of summation.  Rows 1 and 2 copy row 0 (score 1), row 3 is its negative, row 4 is zero
    when n allows."""
    assert L >= 16
    rng = np.random.default_rng(seed)
    x = np.zeros((n, L), np.float32)
    for i in range(n):
        x[i, rng.choice(L, 16, replace=False)] = rng.choice(np.array([-1, 1], np.float32), 16)
    if n > 4:
        x[1], x[2], x[3], x[4] = x[0], x[0], -x[0], 0
    return x


def lattice_inv(x):
    """exact inverse norms of lattice rows: 0.25, and 1 for a zero row (the convention of the norm kernel)"""
    return np.where(np.abs(x).sum(axis=1) > 0, np.float32(0.25), np.float32(1.0)).astype(np.float32)


def lattice_scores(xq, xd):
    """the exact float32 scores of lattice rows with lattice_inv: (0 + dot) * (inv_q * inv_d), every step exact"""
    dot = (xq.astype(np.int64) @ xd.astype(np.int64).T).astype(np.float32)
    return (np.float32(0) + dot) * (lattice_inv(xq)[:, None] * lattice_inv(xd)[None, :])


def planted_band(n, L, t, seed, steps=24):
    """(n, L) float32 rows: `steps` planted pairs v = cos(theta) u + sin(theta) w with unit u, w, u orthogonal to w, cos(theta)
    stepping through [t - 0.9 eps, t + 0.9 eps] (half below t, half above), scattered over the rows; the other rows are random
    directions.  -> (rows, planted (steps, 2) int64 row indices (i < j), their cos(theta) float64)"""
    assert n >= 2 * steps
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, L))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    place = rng.permutation(n)[:2 * steps].reshape(steps, 2)
    place.sort(axis=1)
    e = eps(L)
    cos = np.linspace(t - 0.9 * e, t + 0.9 * e, steps)
    for (i, j), c in zip(place, cos):
        u = x[i]
        w = rng.standard_normal(L)
        w -= (w @ u) * u
        w /= np.linalg.norm(w)
        x[j] = c * u + np.sqrt(1.0 - c * c) * w
    return x.astype(np.float32), place.astype(np.int64), cos


def cosine64(x):
    """float64 cosine matrix of the rows"""
    x = np.asarray(x, np.float64)
    xn = x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-300)
    return xn @ xn.T
