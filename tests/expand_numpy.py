"""NumPy twin of query expansion and database-side augmentation (include/pvsim.h, pvsim/expand.py): every sum as element operations
in the row dtype, one list slot at a time, so that each multiply and each add is rounded on its own -- the bits the device must give."""
import numpy as np


def combine(X, idx, w, self_rows=None, w_self=None, reverse=False):
    """out[i] = w_self[i] * self_rows[i] + sum_j w[i][j] * X[idx[i][j]], j ascending (descending with `reverse`: the order the
    definition does NOT ask for), slots outside [0, N) skipped.  -> (n, L) in X's dtype."""
    X = np.asarray(X)
    dt = X.dtype
    N, L = X.shape
    idx = np.asarray(idx, dtype=np.int64)
    n, r = idx.shape
    acc = np.zeros((n, L), dt)
    if self_rows is not None:
        ws = np.ones(n, dt) if w_self is None else np.asarray(w_self, dtype=dt)
        acc = acc + ws[:, None] * np.asarray(self_rows, dtype=dt)
    for j in (range(r - 1, -1, -1) if reverse else range(r)):
        c = idx[:, j]
        ok = (c >= 0) & (c < N)
        if ok.any():
            acc[ok] = acc[ok] + np.asarray(w, dtype=dt)[ok, j][:, None] * X[c[ok]]
    assert acc.dtype == dt
    return acc


def weights(scores, scheme, alpha):
    """expansion weights, one scalar at a time in the dtype of `scores`"""
    s = np.asarray(scores)
    t = s.dtype.type
    nq, n = s.shape
    out = np.empty_like(s)
    for i in range(nq):
        for j in range(n):
            if scheme == "average":
                out[i, j] = t(1)
            elif scheme == "linear":
                out[i, j] = t(n - j) / t(n)
            else:
                sp = s[i, j] if s[i, j] > 0 else t(0)
                v = t(1) if alpha == 0 else sp
                for _ in range(alpha - 1):
                    v = t(v * sp)
                out[i, j] = v
    return out


def drop_self(idx, val, own):
    """each list without the slot that holds the row's own index; without such a slot, without its last one"""
    out_i, out_v = [], []
    for row_i, row_v, me in zip(idx, val, own):
        pos = [p for p, c in enumerate(row_i) if c == me]
        d = pos[0] if pos else len(row_i) - 1
        out_i.append(np.delete(row_i, d))
        out_v.append(np.delete(row_v, d))
    shape = (len(idx), np.asarray(idx).shape[1] - 1)
    return np.array(out_i, dtype=np.int64).reshape(shape), np.array(out_v, dtype=np.asarray(val).dtype).reshape(shape)


def list_weights(idx, val, inv_db, scheme, alpha):
    """weights(...) * inv_db[idx], 0 on the -1 slots"""
    dt = np.asarray(val).dtype
    w = weights(val, scheme, alpha) * inv_db[np.where(idx >= 0, idx, 0)]
    return np.where(idx >= 0, w, dt.type(0)).astype(dt)


def expand_queries(Q, inv_q, X, inv_db, idx, val, scheme, alpha, query_weight):
    """the expanded queries of one pass: query_weight * q / |q| + sum_j w_j x_j / |x_j|"""
    dt = X.dtype
    return combine(X, idx, list_weights(idx, val, inv_db, scheme, alpha), Q, dt.type(query_weight) * inv_q)


def augment(X, inv_db, idx, val, scheme, alpha):
    """database-side augmentation from complete lists (self included): idx / val (N, r + 1) of every row against the database"""
    i2, v2 = drop_self(idx, val, np.arange(len(X)))
    return combine(X, i2, list_weights(i2, v2, inv_db, scheme, alpha), X, inv_db)


# ------------------------------------------------------------------ the planted corpus of the quality tests
def planted(seed=0, classes=32, per=32, L=64, nq=256, sig_db=1.0, sig_q=1.6):
    """-> (X (classes * per, L) f32, labels, Q (nq, L) f32, query labels)"""
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((classes, L)).astype(np.float32)
    lab = np.repeat(np.arange(classes), per)
    X = (P[lab] + sig_db * rng.standard_normal((classes * per, L))).astype(np.float32)
    ql = rng.integers(0, classes, nq)
    Q = (P[ql] + sig_q * rng.standard_normal((nq, L))).astype(np.float32)
    return X, lab, Q, ql


def inv_norms(X):
    return (1.0 / np.sqrt((X.astype(np.float64) ** 2).sum(axis=1))).astype(X.dtype)


def rank(Q, X, k):
    """cosine ranking (score descending, index ascending) -> (idx, val) in X's dtype"""
    S = ((Q * inv_norms(Q)[:, None]) @ (X * inv_norms(X)[:, None]).T).astype(X.dtype)
    idx = np.argsort(-S, axis=1, kind="stable")[:, :k]
    return idx.astype(np.int64), np.take_along_axis(S, idx, 1)


def precision(idx, lab, ql):
    return float((lab[idx] == ql[:, None]).mean())
