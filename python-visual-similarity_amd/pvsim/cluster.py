"""Image clustering on the device: k-means, spectral clustering and DBSCAN of encodings, and the three label scores the
reference reports (pyvisim/_utils.py:128-162, 333-361 -> scikit-learn 1.7.2).

The N-sized arithmetic runs on the MI355X through the C-ABI (include/pvsim.h, "image clustering"):
* the exact Euclidean neighbour search (pvs_l2_knn_dev, pvs_l2_radius_*_dev): the same float64 distance value and the same
  (distance, index) order as scikit-learn's brute-force reduction, so neighbour lists, graphs and DBSCAN labels are sklearn's;
* the spectral embedding's block eigensolver: CSR SpMM (pvs_csr_spmm_f64_dev), block Gram matrices and block updates
  (pvs_cosine_f64_dev with unit inverse norms); only the p x p Rayleigh-Ritz problems go to numpy.linalg.eigh;
* k-means: pvsim.learn.fit_kmeans (device Lloyd + k-means++, float32).
What stays on the host is O(N k) bookkeeping: symmetrising the kNN graph, DBSCAN's expansion (sklearn's order), and the
contingency-table scores.  Neither scipy nor scikit-learn is imported.
"""
from __future__ import annotations

import math
import warnings

import numpy as np

from .engine import Context, default_context

__all__ = ["kneighbors", "kneighbors_graph", "radius_neighbors", "spectral_embedding", "spectral_clustering", "dbscan",
           "kmeans", "rand_score", "adjusted_rand_score", "adjusted_mutual_info_score"]


# ------------------------------------------------------------------------------------------------ rows on the device
def _check_rows(X) -> np.ndarray:
    """sklearn check_array(dtype=[float64, float32]): float32 stays, everything else becomes float64; finite, 2-D."""
    try:
        import torch
        if isinstance(X, torch.Tensor):
            X = X.detach().cpu().numpy()
    except ImportError:
        pass
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError(f"Expected 2D array, got {X.ndim}D array instead")
    if X.dtype != np.float32:
        X = X.astype(np.float64)
    if X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError(f"Found array with shape {X.shape}; a minimum of 1 sample and 1 feature is required.")
    if not np.isfinite(X).all():
        raise ValueError("Input X contains NaN or infinity.")
    return np.ascontiguousarray(X)


class _Rows:
    def __init__(self, ctx: Context, X: np.ndarray):
        self.ctx, self.n, self.L = ctx, X.shape[0], X.shape[1]
        self.is_f64 = X.dtype == np.float64
        self.buf = ctx.buffer(X.nbytes).upload(X)

    def free(self):
        self.buf.free()


def _ctx(ctx):
    return ctx if ctx is not None else default_context()


# ------------------------------------------------------------------------------------------------ neighbour search
def kneighbors(X, n_neighbors: int, ctx: Context | None = None, return_stats: bool = False):
    """NearestNeighbors(n_neighbors).fit(X).kneighbors(X) (brute force, Euclidean): (distances (N, k) float64, indices (N, k)
    int64), the point itself included.  Order (distance, index); float32 rows are ranked by the float64 distance."""
    X = _check_rows(X)
    N = X.shape[0]
    k = int(n_neighbors)
    if not 1 <= k <= N:
        raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {k}, n_samples_fit = {N}")
    ctx = _ctx(ctx)
    rows = _Rows(ctx, X)
    idx_b, d_b = ctx.buffer(N * k * 8), ctx.buffer(N * k * 8)
    try:
        st = ctx.l2_knn_dev(rows.buf.ptr, N, rows.buf.ptr, N, rows.L, rows.is_f64, k, idx_b.ptr, d_b.ptr, stats=return_stats)
        idx = idx_b.download((N, k), np.int64)
        sq = d_b.download((N, k), np.float64)
    finally:
        rows.free(); idx_b.free(); d_b.free()
    out = (np.sqrt(sq), idx)
    return (out + (st,)) if return_stats else out


def kneighbors_graph(X, n_neighbors: int, include_self: bool = True, ctx: Context | None = None):
    """sklearn.neighbors.kneighbors_graph(X, n_neighbors, mode='connectivity', include_self) as CSR arrays
    (indptr int64 (N+1,), indices int64, data float64 ones)."""
    X = _check_rows(X)
    N = X.shape[0]
    k = int(n_neighbors)
    if include_self:
        _, idx = kneighbors(X, k, ctx)
    else:
        # sklearn's X=None query: k + 1 neighbours, the sample itself removed (or the last one if it is not in the list)
        if k + 1 > N:
            raise ValueError(f"Expected n_neighbors < n_samples_fit, but n_neighbors = {k}, n_samples_fit = {N}")
        _, idx = kneighbors(X, k + 1, ctx)
        mask = idx != np.arange(N)[:, None]
        dup = np.all(mask, axis=1)
        mask[:, 0][dup] = False
        idx = idx[mask].reshape(N, k)
    indptr = np.arange(0, N * k + 1, k, dtype=np.int64)
    return indptr, idx.reshape(-1).astype(np.int64), np.ones(N * k, dtype=np.float64)


def radius_neighbors(X, eps: float, ctx: Context | None = None, return_distance: bool = False):
    """NearestNeighbors(radius=eps).fit(X).radius_neighbors(X) as CSR: (indptr, indices[, distances]); per row the indices
    ascending (brute force order), membership decided on the float64 squared distance <= eps**2."""
    X = _check_rows(X)
    eps = float(eps)
    if not eps >= 0:
        raise ValueError(f"eps == {eps}, must be >= 0.0.")
    ctx = _ctx(ctx)
    N = X.shape[0]
    r = eps * eps
    rows = _Rows(ctx, X)
    cnt = ctx.buffer(N * 8)
    try:
        ctx.l2_radius_count_dev(rows.buf.ptr, N, rows.buf.ptr, N, rows.L, rows.is_f64, r, cnt.ptr)
        counts = cnt.download((N,), np.int64)
        indptr = np.zeros(N + 1, dtype=np.int64)
        np.cumsum(counts, out=indptr[1:])
        nnz = int(indptr[-1])
        ip = ctx.buffer((N + 1) * 8).upload(indptr)
        ib, db = ctx.buffer(max(nnz, 1) * 8), ctx.buffer(max(nnz, 1) * 8)
        try:
            ctx.l2_radius_fill_dev(rows.buf.ptr, N, rows.buf.ptr, N, rows.L, rows.is_f64, r, ip.ptr, ib.ptr,
                                   db.ptr if return_distance else None)
            indices = ib.download((nnz,), np.int64)
            dist = np.sqrt(db.download((nnz,), np.float64)) if return_distance else None
        finally:
            ip.free(); ib.free(); db.free()
    finally:
        rows.free(); cnt.free()
    return (indptr, indices, dist) if return_distance else (indptr, indices)


# ------------------------------------------------------------------------------------------------ spectral embedding
def _csr_sym_half(indptr, indices, N):
    """A = 0.5 (C + C^T) of a 0/1 connectivity graph, CSR with sorted column indices"""
    rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(indptr))
    r = np.concatenate([rows, indices])
    c = np.concatenate([indices, rows])
    key = r * N + c
    uk, cnt = np.unique(key, return_counts=True)
    data = 0.5 * cnt.astype(np.float64)
    ur, uc = uk // N, uk % N
    ptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(ur, minlength=N), out=ptr[1:])
    return ptr, uc.astype(np.int64), data, ur


def _normalised_affinity(indptr, indices, N):
    """scipy csgraph.laplacian(A, normed=True) as sklearn uses it: degrees without the self loops, dd = sqrt(degree) (1 for
    isolated nodes), L = I - S with S = D^-1/2 A D^-1/2 off the diagonal.  Returns S (CSR, zero diagonal dropped), dd."""
    ptr, col, data, row = _csr_sym_half(indptr, indices, N)
    diag = np.zeros(N)
    on = row == col
    diag[row[on]] = data[on]
    deg = np.bincount(row, weights=data, minlength=N) - diag
    iso = deg == 0
    dd = np.where(iso, 1.0, np.sqrt(np.where(iso, 1.0, deg)))
    keep = ~on
    s_row, s_col = row[keep], col[keep]
    s_data = data[keep] / dd[s_row] / dd[s_col]
    s_ptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(s_row, minlength=N), out=s_ptr[1:])
    n_comp = _n_components(ptr, col, N)
    return s_ptr, s_col.astype(np.int64), s_data, dd, n_comp


def _n_components(ptr, col, N):
    parent = np.arange(N)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    rows = np.repeat(np.arange(N), np.diff(ptr))
    for a, b in zip(rows.tolist(), col.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    return len({find(i) for i in range(N)})


class _Block:
    """An (N, p) float64 block on the device and the NT-GEMM / Gram helpers the eigensolver needs."""

    def __init__(self, ctx, N, p):
        self.ctx, self.N, self.p = ctx, N, p
        self.buf = ctx.buffer(N * p * 8)

    def free(self):
        self.buf.free()


class _Solver:
    def __init__(self, ctx, s_ptr, s_col, s_data, N, p):
        self.ctx, self.N, self.p = ctx, N, p
        self.ip = ctx.buffer((N + 1) * 8).upload(s_ptr)
        self.ix = ctx.buffer(max(len(s_col), 1) * 8).upload(s_col if len(s_col) else np.zeros(1, np.int64))
        self.dx = ctx.buffer(max(len(s_data), 1) * 8).upload(s_data if len(s_data) else np.zeros(1))
        self.t1, self.t2 = ctx.buffer(N * p * 8), ctx.buffer(N * p * 8)
        self.small = ctx.buffer(p * p * 8)
        self.vec = ctx.buffer(p * 8)
        self.gram_out = ctx.buffer(p * p * 8)

    def free(self):
        for b in (self.ip, self.ix, self.dx, self.t1, self.t2, self.small, self.vec, self.gram_out):
            b.free()

    def spmm(self, x, y, alpha=1.0, beta=None, z=None, gamma=0.0):
        bp = None
        if beta is not None:
            self.vec.upload(np.ascontiguousarray(np.broadcast_to(np.asarray(beta, np.float64), (self.p,))))
            bp = self.vec.ptr
        self.ctx.csr_spmm_f64_dev(self.N, self.ip.ptr, self.ix.ptr, self.dx.ptr, x.ptr, self.p, y.ptr, alpha, bp,
                                  z.ptr if z is not None else None, gamma)

    def gram(self, a, b):
        """a^T b (p x p) of two (N, p) blocks: transposes, then the f64 NT GEMM with unit inverse norms"""
        self.ctx.transpose_f64_dev(a.ptr, self.N, self.p, self.t1.ptr)
        if b is a:
            tb = self.t1
        else:
            self.ctx.transpose_f64_dev(b.ptr, self.N, self.p, self.t2.ptr)
            tb = self.t2
        self.ctx.cosine_f64_dev(self.t1.ptr, self.p, tb.ptr, self.p, self.N, None, None, self.gram_out.ptr, self.p)
        return self.gram_out.download((self.p, self.p), np.float64)

    def times(self, a, W, out):
        """out = a W  ((N, p) x (p, p)): NT GEMM with B = W^T"""
        self.small.upload(np.ascontiguousarray(W.T, dtype=np.float64))
        self.ctx.cosine_f64_dev(a.ptr, self.N, self.small.ptr, self.p, self.p, None, None, out.ptr, self.p)


def _orthonormalise(sv: _Solver, V, tmp):
    """V <- V G^-1/2 (G = V^T V), twice; eigen-decomposition of G on the host (p x p)"""
    for _ in range(2):
        G = sv.gram(V, V)
        lam, U = np.linalg.eigh(0.5 * (G + G.T))
        lam = np.maximum(lam, lam.max() * 1e-15)
        sv.times(V, U / np.sqrt(lam)[None, :], tmp)
        V, tmp = tmp, V
    return V, tmp


def spectral_embedding(indptr, indices, N: int, n_components: int, random_state=None, eigen_tol="auto",
                       max_iter: int = 500, degree: int = 10, ctx: Context | None = None):
    """sklearn.manifold._spectral_embedding(0.5 (C + C^T), n_components, norm_laplacian=True, drop_first=False) for a
    connectivity graph C given as CSR (indptr, indices).  Returns (maps (N, n_components), eigenvalues of the normalised
    Laplacian (ascending), iterations).

    The eigenvectors of L = I - S closest to 0 are the top eigenvectors of S = D^-1/2 A D^-1/2 (spectrum in [-1, 1]):
    Chebyshev-filtered subspace iteration on S with a block of p = n_components + guard vectors -- a degree-`degree` filter
    that damps [-1, a] (a = the lowest Ritz value of the block), orthonormalisation, Rayleigh-Ritz -- until every wanted
    residual |S v - theta v| is <= tol (eigen_tol, 'auto' = 1e-10).  A UserWarning is raised if max_iter is reached.
    Then the reference's post-processing: divide by dd, deterministic sign flip, drop_first=False."""
    from .learn import _rng
    ctx = _ctx(ctx)
    m = int(n_components)
    if not 1 <= m < N:
        raise ValueError(f"n_components={m} must be between 1 and n_samples - 1 = {N - 1}")
    tol = 1e-10 if eigen_tol == "auto" else float(eigen_tol)
    tol = max(tol, 1e-13)
    s_ptr, s_col, s_data, dd, n_comp = _normalised_affinity(np.asarray(indptr), np.asarray(indices), N)
    if n_comp > 1:
        warnings.warn("Graph is not fully connected, spectral embedding may not work as expected.", UserWarning,
                      stacklevel=2)
    rng = _rng(random_state)
    p = min(N, m + max(8, m // 2))
    sv = _Solver(ctx, s_ptr, s_col, s_data, N, p)
    blocks = [sv.ctx.buffer(N * p * 8) for _ in range(4)]
    try:
        V, T, Y0, Y1 = blocks
        X0 = rng.standard_normal((N, p))
        X0[:, 0] = dd
        V.upload(np.ascontiguousarray(X0))
        V, T = _orthonormalise(sv, V, T)
        a = None
        theta = None
        it = 0
        res = np.full(m, np.inf)
        for it in range(1, max_iter + 1):
            if a is not None:
                # Chebyshev filter on [-1, a]: Y_1 = (S - c) V / e, Y_{j+1} = 2 (S - c) Y_j / e - Y_{j-1}
                e, c = (a + 1.0) / 2.0, (a - 1.0) / 2.0
                sv.spmm(V, Y0, alpha=1.0 / e, beta=-c / e)
                prev, cur = V, Y0
                for _ in range(degree - 1):
                    nxt = [b for b in blocks if b is not prev and b is not cur][0]
                    sv.spmm(cur, nxt, alpha=2.0 / e, beta=-2.0 * c / e, z=prev, gamma=-1.0)
                    prev, cur = cur, nxt
                others = [b for b in blocks if b is not cur]
                V, T, Y0, Y1 = cur, others[0], others[1], others[2]
                V, T = _orthonormalise(sv, V, T)
            # Rayleigh-Ritz
            sv.spmm(V, Y0)
            H = sv.gram(V, Y0)
            theta, W = np.linalg.eigh(0.5 * (H + H.T))
            order = np.argsort(-theta, kind="stable")
            theta, W = theta[order], W[:, order]
            sv.times(V, W, T)
            sv.times(Y0, W, Y1)
            V, T = T, V
            # residuals R = S V - V diag(theta), column norms from the diagonal of R^T R
            sv.spmm(V, Y0, alpha=0.0, beta=-theta, z=Y1, gamma=1.0)
            R = sv.gram(Y0, Y0)
            res = np.sqrt(np.maximum(np.diag(R), 0.0))[:m]
            if np.all(res <= tol):
                break
            a = float(min(theta[-1], theta[m - 1] - 1e-12))
            a = max(a, -1.0 + 1e-6)
        else:
            warnings.warn(f"spectral_embedding: {max_iter} iterations without reaching the residual tolerance {tol:g} "
                          f"(largest residual {res.max():.3g})", UserWarning, stacklevel=2)
        vecs = V.download((N, p), np.float64)[:, :m]
    finally:
        for b in blocks:
            b.free()
        sv.free()
    emb = (vecs / dd[:, None]).T                        # (m, N), smallest Laplacian eigenvalue first
    max_abs = np.argmax(np.abs(emb), axis=1)            # sklearn.utils.extmath._deterministic_vector_sign_flip
    signs = np.sign(emb[range(emb.shape[0]), max_abs])
    emb *= signs[:, np.newaxis]
    return np.ascontiguousarray(emb.T), 1.0 - theta[:m], it


def spectral_clustering(X, n_clusters: int, *, n_neighbors: int = 10, n_components=None, n_init: int = 10,
                        eigen_tol="auto", random_state=None, ctx: Context | None = None, **kmeans_kwargs):
    """SpectralClustering(n_clusters, affinity='nearest_neighbors', assign_labels='kmeans', ...).fit_predict(X)"""
    from . import learn
    ctx = _ctx(ctx)
    rng = learn._rng(random_state)
    X = _check_rows(X)
    indptr, indices, _ = kneighbors_graph(X, n_neighbors, include_self=True, ctx=ctx)
    nc = n_clusters if n_components is None else int(n_components)
    maps, _, _ = spectral_embedding(indptr, indices, X.shape[0], nc, random_state=rng, eigen_tol=eigen_tol, ctx=ctx)
    return kmeans(maps, n_clusters, random_state=rng, n_init=n_init, ctx=ctx, **kmeans_kwargs)


def kmeans(X, n_clusters: int, *, random_state=None, ctx: Context | None = None, **kwargs) -> np.ndarray:
    """KMeans(n_clusters, random_state, **kwargs).fit_predict(X) on the device (pvsim.learn.fit_kmeans).  The device Lloyd runs
    in float32: float64 rows are clustered as their float32 rounding."""
    from . import learn
    X = _check_rows(X)
    ctx = _ctx(ctx)
    rows = learn.DeviceRows.from_host(ctx, X.astype(np.float32))
    try:
        return learn.fit_kmeans(rows, int(n_clusters), random_state=random_state, **kwargs).labels_.astype(np.int64)
    finally:
        rows.free()


def dbscan(X, eps: float = 0.5, min_samples: int = 5, ctx: Context | None = None) -> np.ndarray:
    """DBSCAN(eps, min_samples).fit_predict(X), Euclidean: radius CSR from the device, then sklearn's dbscan_inner
    (sklearn/cluster/_dbscan_inner.pyx) on the host -- clusters grown in order of core index, depth first over the
    neighbour lists in index order.  Noise is -1."""
    if int(min_samples) < 1:
        raise ValueError(f"min_samples == {min_samples}, must be >= 1.")
    indptr, indices = radius_neighbors(X, eps, ctx)
    N = len(indptr) - 1
    n_neighbors = np.diff(indptr)
    is_core = n_neighbors >= int(min_samples)
    labels = np.full(N, -1, dtype=np.int64)
    ind = indices.tolist()
    ptr = indptr.tolist()
    core = is_core.tolist()
    lab = labels.tolist()
    label_num = 0
    for i0 in range(N):
        if lab[i0] != -1 or not core[i0]:
            continue
        stack = []
        i = i0
        while True:
            if lab[i] == -1:
                lab[i] = label_num
                if core[i]:
                    for v in ind[ptr[i]:ptr[i + 1]]:
                        if lab[v] == -1:
                            stack.append(v)
            if not stack:
                break
            i = stack.pop()
        label_num += 1
    return np.asarray(lab, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ label scores (sklearn.metrics)
def _contingency(labels_true, labels_pred):
    labels_true = np.asarray(labels_true).reshape(-1)
    labels_pred = np.asarray(labels_pred).reshape(-1)
    if labels_true.shape != labels_pred.shape:
        raise ValueError(f"labels_true and labels_pred must have same size, got {labels_true.shape[0]} and "
                         f"{labels_pred.shape[0]}")
    classes, ci = np.unique(labels_true, return_inverse=True)
    clusters, ki = np.unique(labels_pred, return_inverse=True)
    key = ci.astype(np.int64) * len(clusters) + ki
    uk, cnt = np.unique(key, return_counts=True)   # nonzero cells, row-major (scipy.sparse.find order of a CSR matrix)
    return classes, clusters, uk // len(clusters), uk % len(clusters), cnt.astype(np.int64)


def _pair_confusion(labels_true, labels_pred):
    classes, clusters, r, c, v = _contingency(labels_true, labels_pred)
    n = int(v.sum())
    n_c = np.bincount(r, weights=v, minlength=len(classes)).astype(np.int64)
    n_k = np.bincount(c, weights=v, minlength=len(clusters)).astype(np.int64)
    sum_sq = int((v * v).sum())
    c01 = int((v * n_k[c]).sum()) - sum_sq
    c10 = int((v * n_c[r]).sum()) - sum_sq
    c11 = sum_sq - n
    c00 = n * n - c01 - c10 - sum_sq
    return c00, c01, c10, c11


def rand_score(labels_true, labels_pred) -> float:
    """sklearn.metrics.rand_score"""
    c00, c01, c10, c11 = _pair_confusion(labels_true, labels_pred)
    num, den = c00 + c11, c00 + c01 + c10 + c11
    if num == den or den == 0:
        return 1.0
    return num / den


def adjusted_rand_score(labels_true, labels_pred) -> float:
    """sklearn.metrics.adjusted_rand_score"""
    tn, fp, fn, tp = _pair_confusion(labels_true, labels_pred)
    if fn == 0 and fp == 0:
        return 1.0
    return 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))


def _entropy(labels):
    labels = np.asarray(labels).reshape(-1)
    if len(labels) == 0:
        return 1.0
    pi = np.bincount(np.unique(labels, return_inverse=True)[1]).astype(np.float64)
    pi = pi[pi > 0]
    if pi.size == 1:
        return 0.0
    s = np.sum(pi)
    return float(-np.sum((pi / s) * (np.log(pi) - math.log(s))))


def _mutual_info(r, c, v, n_rows, n_cols):
    s = float(v.sum())
    pi = np.bincount(r, weights=v, minlength=n_rows)
    pj = np.bincount(c, weights=v, minlength=n_cols)
    if pi.size == 1 or pj.size == 1:
        return 0.0
    log_nm = np.log(v.astype(np.float64))
    nm = v / s
    outer = pi.astype(np.int64)[r] * pj.astype(np.int64)[c]
    log_outer = -np.log(outer.astype(np.float64)) + math.log(pi.sum()) + math.log(pj.sum())
    mi = nm * (log_nm - math.log(s)) + nm * log_outer
    mi = np.where(np.abs(mi) < np.finfo(mi.dtype).eps, 0.0, mi)
    return float(np.clip(mi.sum(), 0.0, None))


def _expected_mutual_info(a, b, n):
    """sklearn/metrics/cluster/_expected_mutual_info_fast.pyx with math.lgamma for gammaln"""
    if a.size == 1 or b.size == 1:
        return 0.0
    top = int(max(a.max(), b.max()))
    nijs = np.arange(0, top + 1, dtype=np.float64)
    nijs[0] = 1
    term1 = nijs / n
    log_a, log_b = np.log(a.astype(np.float64)), np.log(b.astype(np.float64))
    log_Nnij = math.log(n) + np.log(nijs)
    lg = np.array([math.lgamma(x) if x > 0 else math.inf for x in range(0, n + 2)])    # lg[x] = lgamma(x); gammaln(x + 1) = lg[x + 1]
    gln_a, gln_b = lg[a + 1], lg[b + 1]
    gln_Na, gln_Nb = lg[n - a + 1], lg[n - b + 1]
    gln_Nnij = lg[nijs.astype(np.int64) + 1] + lg[n + 1]
    emi = 0.0
    for i in range(a.size):
        for j in range(b.size):
            start = max(1, int(a[i]) - n + int(b[j]))
            end = min(int(a[i]), int(b[j])) + 1
            if start >= end:
                continue
            nij = np.arange(start, end)
            term2 = log_Nnij[nij] - log_a[i] - log_b[j]
            gln = (gln_a[i] + gln_b[j] + gln_Na[i] + gln_Nb[j] - gln_Nnij[nij] - lg[a[i] - nij + 1] - lg[b[j] - nij + 1]
                   - lg[n - a[i] - b[j] + nij + 1])
            for t in (term1[nij] * term2 * np.exp(gln)).tolist():
                emi += t
    return emi


def adjusted_mutual_info_score(labels_true, labels_pred, *, average_method: str = "arithmetic") -> float:
    """sklearn.metrics.adjusted_mutual_info_score (average_method 'arithmetic', 'geometric', 'min' or 'max')"""
    classes, clusters, r, c, v = _contingency(labels_true, labels_pred)
    n = int(v.sum())
    if (len(classes) == len(clusters) == 1) or (len(classes) == len(clusters) == 0):
        return 1.0
    mi = _mutual_info(r, c, v, len(classes), len(clusters))
    a = np.bincount(r, weights=v, minlength=len(classes)).astype(np.int64)
    b = np.bincount(c, weights=v, minlength=len(clusters)).astype(np.int64)
    emi = _expected_mutual_info(a, b, n)
    h_true, h_pred = _entropy(labels_true), _entropy(labels_pred)
    if average_method == "min":
        norm = min(h_true, h_pred)
    elif average_method == "geometric":
        norm = math.sqrt(h_true * h_pred)
    elif average_method == "arithmetic":
        norm = (h_true + h_pred) / 2
    elif average_method == "max":
        norm = max(h_true, h_pred)
    else:
        raise ValueError("'average_method' must be 'min', 'geometric', 'arithmetic', or 'max'")
    den = norm - emi
    eps = np.finfo("float64").eps
    den = min(den, -eps) if den < 0 else max(den, eps)
    return float((mi - emi) / den)
