"""float64 NumPy restatements of the image-clustering device code (csrc/neighbors.hip and the device blocks of the spectral
solver in pvsim/cluster.py): the squared distance sklearn ranks, the k nearest rows under the total order (distance ascending,
index ascending), radius neighbours as CSR, the candidate count of the float32 prefilter, the CSR block product and a dense
eigen-decomposition of the normalised affinity.  Plain NumPy, no device, no scikit-learn.

On LATTICE rows (small integers stored as float32 or float64, see lattice / lattice_ok) every product, dot product, norm,
half-norm key and distance is an exact integer or half-integer in float32 and in float64, whatever the order of the additions.  The
device's lists then EQUAL the ones formed here -- indices and squared distances, on every path (the float32 prefilter, the full
float64 pass, the GEMM's own ranking of an overflowing query, the paged ranking, the radius passes) -- with no tolerance and no
near-tie exception.  Exact ties are frequent on a lattice, which is the point."""
import numpy as np

NB_CAP_MAX, NB_K_MAX = 1024, 256      # csrc/neighbors.hip
PANEL_COLS, TILE_F32 = 32768, 8192    # columns of a float32 score panel, queries of a float32 tile
TILE_F64_ELEMS = 128 << 20            # float64 panels: QT = 2^27 / N queries
EXACT32 = 2.0 ** 23                   # half-integers up to this magnitude are exact in float32


def lattice(seed, n, L, a, dtype=np.float32):
    """seeded rows of integers in [-a, a]"""
    return np.random.default_rng(seed).integers(-a, a + 1, (n, L)).astype(dtype)


def lattice_ok(*arrs):
    """Asserts the exact regime: integer valued rows of one length L with 4 L M^2 < 2^23 (M the largest magnitude), so that every
    partial sum of a dot product (<= L M^2), |y|^2 / 2, the key x.y - |y|^2 / 2 (within 1.5 L M^2) and the distance (<= 4 L M^2) is
    an integer or half-integer that float32 (and float64) holds exactly, in any order, fused or not.  -> M"""
    L = arrs[0].shape[1]
    M = 0.0
    for a in arrs:
        a = np.asarray(a)
        assert a.ndim == 2 and a.shape[1] == L and a.dtype in (np.float32, np.float64), (a.dtype, a.shape)
        assert np.array_equal(a, np.rint(a)), "not integer valued"
        M = max(M, float(np.abs(a).max()))
    assert 4 * L * M * M < EXACT32, (L, M)
    return M


def _norms(A):
    A = np.asarray(A, np.float64)
    return (A * A).sum(1)


def sqdist(Q, X, chunk=4096):
    """d(i, j) = max(0, (|x_i|^2 + (-2 x_i . y_j)) + |y_j|^2) in float64 -> (nq, N); queries in chunks.  The dot product is summed
    one dimension after the other, so the value is a function of the two rows alone: identical rows tie exactly on any input
    (a BLAS product may round the columns of two identical rows differently)."""
    Q64, XT = np.asarray(Q, np.float64), np.ascontiguousarray(np.asarray(X, np.float64).T)
    yn = _norms(XT.T)
    out = np.empty((len(Q64), XT.shape[1]))
    for s in range(0, len(Q64), chunk):
        q = Q64[s:s + chunk]
        dot = np.zeros((len(q), XT.shape[1]))
        tmp = np.empty_like(dot)
        for l in range(XT.shape[0]):
            np.multiply(q[:, l, None], XT[l][None, :], out=tmp)
            dot += tmp
        out[s:s + chunk] = np.maximum(0.0, (_norms(q)[:, None] + (-2.0 * dot)) + yn[None, :])
    return out


def _lists_of(d, k):
    """the k first columns of every row of d under (value ascending, index ascending)"""
    nq, N = d.shape
    kth = np.partition(d, k - 1, axis=1)[:, k - 1]
    r, c = np.nonzero(d <= kth[:, None])                       # row-major: per row the columns ascending
    v = d[r, c]
    order = np.lexsort((c, v, r))
    r, c, v = r[order], c[order], v[order]
    start = np.searchsorted(r, np.arange(nq))
    keep = (np.arange(len(r)) - start[r]) < k
    return c[keep].reshape(nq, k).astype(np.int64), v[keep].reshape(nq, k)


def knn_lists(Q, X, k, chunk=4096):
    """-> (idx (nq, k) int64, squared distances (nq, k)): the k nearest rows of X per query, (distance, index) ascending"""
    Q, X = np.asarray(Q), np.asarray(X)
    assert 1 <= k <= len(X)
    idx, sq = np.empty((len(Q), k), np.int64), np.empty((len(Q), k))
    for s in range(0, len(Q), chunk):
        idx[s:s + chunk], sq[s:s + chunk] = _lists_of(sqdist(Q[s:s + chunk], X), k)
    return idx, sq


def tied_at_kth(Q, X, k, chunk=4096):
    """per query the number of rows with d <= the k-th smallest distance: the candidates of the float64 path on lattice rows
    (its margin is far below 1, the spacing of the distances)"""
    Q, X = np.asarray(Q), np.asarray(X)
    out = np.empty(len(Q), np.int64)
    for s in range(0, len(Q), chunk):
        d = sqdist(Q[s:s + chunk], X)
        out[s:s + chunk] = (d <= np.partition(d, k - 1, axis=1)[:, k - 1:k]).sum(1)
    return out


def radius_csr(Q, X, r_sq, chunk=4096):
    """-> (indptr (nq + 1,), indices, squared distances): per query the rows with d <= r_sq, indices ascending"""
    Q, X = np.asarray(Q), np.asarray(X)
    counts, cols, vals = [], [], []
    for s in range(0, len(Q), chunk):
        d = sqdist(Q[s:s + chunk], X)
        m = d <= r_sq
        counts.append(m.sum(1))
        cols.append(np.nonzero(m)[1])
        vals.append(d[m])
    indptr = np.zeros(len(Q) + 1, np.int64)
    np.cumsum(np.concatenate(counts), out=indptr[1:])
    return indptr, np.concatenate(cols).astype(np.int64), np.concatenate(vals)


# ------------------------------------------------------------------------------------------------ the float32 prefilter
def slots(k):
    """candidate slots per query"""
    return min(NB_CAP_MAX, max(256, 8 * k))


def chain_term(L, generic=False):
    """the longest chain of f32 roundings of a score: 1025 + L / 1024 on the MFMA kernel, L + 1 on the generic tile kernel
    (L % 4 != 0 or a base pointer that is not 16-byte aligned)"""
    return float(L) + 1.0 if (generic or L % 4 != 0) else 1025.0 + float(L) / 1024.0


def key_error_f32(xnq, ym2, L, chain):
    """nb_key_error<float>, term for term"""
    xq, ym, Ld = np.sqrt(xnq), np.sqrt(ym2), float(L)
    f64 = (Ld + 4.0) * 2.0 ** -53 * (xnq + ym2 + 2.0 * xq * ym)
    u2 = 2.0 ** -23
    return (chain * u2 * xq * ym + u2 * (ym2 + xq * ym) + Ld * 2.0 ** -124 + 0.5 * f64) * 1.001


def candidate_counts(Q, X, k, chain=None, same=False, chunk=2048):
    """The candidates nb_collect_kernel<float> keeps per query: the columns whose key  x.y - fl32(|y|^2 / 2)  is >=
    fl32(a_k - 2 E), a_k the k-th best key (larger = nearer) and E = key_error_f32.  The rows are scored in panels of 32768
    columns and a panel is filtered against the k-th best key of the columns seen SO FAR (the running form); with one panel that
    is the final k-th key.  The largest norm is taken over the rows and, unless `same` (Q is X), the queries.
    -> (counts (nq,) int64, cap)"""
    Q, X = np.asarray(Q), np.asarray(X)
    lattice_ok(Q, X)
    N, L = X.shape
    chain = chain_term(L) if chain is None else chain
    yn, xn = _norms(X), _norms(Q)
    ym2 = yn.max() if same else max(yn.max(), xn.max())
    hy = (0.5 * yn).astype(np.float32)
    X64 = np.asarray(X, np.float64)
    counts = np.zeros(len(Q), np.int64)
    for s in range(0, len(Q), chunk):
        q = np.asarray(Q[s:s + chunk], np.float64)
        key = (q @ X64.T).astype(np.float32) - hy[None, :]                       # exact: half-integers below 2^23
        E = key_error_f32(xn[s:s + chunk], ym2, L, chain)
        for c0 in range(0, N, PANEL_COLS):
            c1 = min(N, c0 + PANEL_COLS)
            a_k = -np.partition(-key[:, :c1], k - 1, axis=1)[:, k - 1]             # k <= 32768 <= c1: the list is full
            thr = (a_k.astype(np.float64) - 2.0 * E).astype(np.float32)
            counts[s:s + chunk] += (key[:, c0:c1] >= thr[:, None]).sum(1)
    return counts, slots(k)


# ------------------------------------------------------------------------------------------------ the solver's blocks
def spmm(indptr, indices, data, X, alpha=1.0, beta=None, Z=None, gamma=0.0):
    """Y = alpha S X + X diag(beta) + gamma Z for a CSR matrix S (columns in any order); beta / Z may be None"""
    X = np.asarray(X, np.float64)
    n, m = X.shape
    S = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(indptr))
    np.add.at(S, (rows, np.asarray(indices)), np.asarray(data, np.float64))
    Y = alpha * (S @ X)
    if beta is not None:
        Y = Y + X * np.broadcast_to(np.asarray(beta, np.float64), (m,))[None, :]
    if Z is not None:
        Y = Y + gamma * np.asarray(Z, np.float64)
    return Y


def normalised_affinity_eigh(indptr, indices, N):
    """The matrix pvsim.cluster._normalised_affinity builds, dense: A = (C + C^T) / 2 of the 0/1 graph C, degrees without the
    diagonal, dd = sqrt(degree) (1 for isolated nodes), S = D^-1/2 A D^-1/2 off the diagonal -- and numpy.linalg.eigh of it.
    -> (theta (N,) descending, eigenvectors (N, N) in that order, dd); the normalised Laplacian's eigenvalues are 1 - theta"""
    C = np.zeros((N, N))
    rows = np.repeat(np.arange(N), np.diff(indptr))
    np.add.at(C, (rows, np.asarray(indices)), 1.0)             # an entry listed twice counts twice, as in _csr_sym_half
    A = 0.5 * (C + C.T)
    deg = A.sum(1) - np.diag(A)
    iso = deg == 0
    dd = np.where(iso, 1.0, np.sqrt(np.where(iso, 1.0, deg)))
    S = A / dd[:, None] / dd[None, :]
    np.fill_diagonal(S, 0.0)
    theta, U = np.linalg.eigh(S)
    return theta[::-1].copy(), U[:, ::-1].copy(), dd


def subspace_sine(A, B):
    """sine of the largest principal angle between span(A) and span(B) (equal dimension), formed as |(I - Qb Qb^T) Qa|_2: accurate
    near 0, where sqrt(1 - cos^2) is not"""
    qa, _ = np.linalg.qr(np.asarray(A, np.float64))
    qb, _ = np.linalg.qr(np.asarray(B, np.float64))
    return float(np.linalg.norm(qa - qb @ (qb.T @ qa), 2))
