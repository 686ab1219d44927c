"""NumPy twin of diffusion re-ranking (include/pvsim.h): every definition restated with element operations in
float64, each multiply, add, subtract and divide rounded on its own, in the stated order -- so the device's results can be compared
bit for bit.  Plus a dense solve of (I - alpha S) f = y, the yardstick of the twin's own conjugate gradients, and the curves corpus
of the quality measurement."""
import numpy as np

DOT_BLOCK = 256


# ------------------------------------------------------------------------------------------------ graph
def drop_self(idx, val, own):
    """the rule of pvsim.expand.drop_self: the first slot holding own[i] leaves, or the last slot where there is none"""
    n, m = idx.shape
    hit = idx == np.asarray(own).reshape(n, 1)
    drop = np.where(hit.any(axis=1), hit.argmax(axis=1), m - 1)
    keep = np.arange(m)[None, :] != drop[:, None]
    return idx[keep].reshape(n, m - 1), val[keep].reshape(n, m - 1)


def affinity(sim, gamma):
    """max(sim, 0) multiplied by itself gamma - 1 times, left to right (gamma = 0: 1), in float64; a NaN counts as 0"""
    v = np.asarray(sim).astype(np.float64)
    sp = np.where(v > 0, v, 0.0)
    if gamma == 0:
        return np.ones_like(sp)
    a = sp.copy()
    for _ in range(gamma - 1):
        a = a * sp
    return a


def mutual(nbr, a):
    """w[i][t] = min(a[i][t], a[j][u]) with j = nbr[i][t] and u the first slot of row j that holds i; +0 without such a slot and for
    a j outside [0, N)"""
    N, kg = nbr.shape
    valid = (nbr >= 0) & (nbr < N)
    j = np.where(valid, nbr, 0).astype(np.int64)
    hit = (nbr[j] == np.arange(N).reshape(N, 1, 1)) & valid[:, :, None]          # (N, kg, kg): slot u of row j holds i
    u = hit.argmax(axis=2)
    back = np.take_along_axis(a[j], u[:, :, None], axis=2)[:, :, 0]
    return np.where(hit.any(axis=2), np.minimum(a, back), 0.0)


def degrees(w):
    """deg_i from +0, slots ascending; r = 1 / sqrt(deg), 0 where deg = 0"""
    deg = np.zeros(w.shape[0])
    for t in range(w.shape[1]):
        deg = deg + w[:, t]
    with np.errstate(divide="ignore"):
        r = np.where(deg > 0, 1.0 / np.sqrt(deg), 0.0)
    return deg, r


def normalise(nbr, w, r):
    """s[i][t] = w[i][t] * (r[i] * r[j]); r[j] counts as 0 for a j outside [0, N)"""
    N = nbr.shape[0]
    valid = (nbr >= 0) & (nbr < N)
    rj = np.where(valid, r[np.where(valid, nbr, 0)], 0.0)
    return w * (r[:, None] * rj)


def graph(nbr, sim, gamma):
    """lists without self (nbr (N, kg) integers, sim (N, kg)) -> dict of every stage: nbr int32, a, w, deg, r, s"""
    nbr = np.asarray(nbr)
    nbr = np.where((nbr >= 0) & (nbr < nbr.shape[0]), nbr, -1).astype(np.int32)          # an index outside [0, N) is stored as -1
    a = affinity(sim, gamma)
    w = mutual(nbr, a)
    deg, r = degrees(w)
    return {"nbr": nbr, "a": a, "w": w, "deg": deg, "r": r, "s": normalise(nbr, w, r)}


def graph_from_lists(idx, val, gamma):
    """the complete rankings of every row against the index, depth kg + 1 -> graph()"""
    i, v = drop_self(idx, val, np.arange(idx.shape[0]))
    return graph(i, v, gamma)


def rhs(idx, val, N, gamma):
    """Y (N, nq): zero, except Y[idx[c][j]][c] = affinity(val[c][j]); slots outside [0, N) are skipped"""
    nq, kq = idx.shape
    Y = np.zeros((N, nq))
    a = affinity(val, gamma)
    for c in range(nq):
        ok = (idx[c] >= 0) & (idx[c] < N)
        Y[idx[c][ok], c] = a[c][ok]
    return Y


def dense(nbr, s):
    """S as a dense (N, N) matrix (entries of repeated slots add up, in slot order)"""
    N, kg = nbr.shape
    S = np.zeros((N, N))
    for t in range(kg):
        ok = (nbr[:, t] >= 0) & (nbr[:, t] < N)
        np.add.at(S, (np.arange(N)[ok], nbr[ok, t]), s[ok, t])
    return S


# ------------------------------------------------------------------------------------------------ solver
def dot(u, v):
    """per column: the products padded with +0 to a multiple of 256 rows, a fixed tree inside each block of 256 rows
    (v[0:h] += v[h:2h], h = 128 .. 1), the block results added from +0 in block order"""
    N, C = u.shape
    nb = (N + DOT_BLOCK - 1) // DOT_BLOCK
    prod = np.zeros((nb * DOT_BLOCK, C))
    prod[:N] = u * v
    t = prod.reshape(nb, DOT_BLOCK, C)
    h = DOT_BLOCK // 2
    while h >= 1:
        t = t[:, :h] + t[:, h:2 * h]
        h //= 2
    out = np.zeros(C)
    for b in range(nb):
        out = out + t[b, 0]
    return out


def apply(nbr, s, P, alpha):
    """Ap[i] = p[i] - alpha * (sum_t s[i][t] * p[nbr[i][t]]), the sum from +0 with t ascending; a slot outside [0, N) reads p as +0"""
    N = nbr.shape[0]
    acc = np.zeros_like(P)
    for t in range(nbr.shape[1]):
        ok = (nbr[:, t] >= 0) & (nbr[:, t] < N)
        pj = np.where(ok[:, None], P[np.where(ok, nbr[:, t], 0)], 0.0)
        acc = acc + s[:, t, None] * pj
    return P - alpha * acc


def cg(nbr, s, Y, alpha, tol, maxiter):
    """conjugate gradients on (I - alpha S) x = y, every column on its own -> (x, steps, rr, yy)"""
    Y = np.asarray(Y, dtype=np.float64)
    N, C = Y.shape
    x = np.zeros_like(Y)
    r = Y.copy()
    p = Y.copy()
    rr = dot(r, r)
    yy = rr.copy()
    thr = (tol * tol) * yy
    retired = np.zeros(C, bool)
    steps = np.zeros(C, np.int32)
    with np.errstate(all="ignore"):
        for _ in range(maxiter):
            act = (rr > thr) & ~retired
            if not act.any():
                break
            Ap = apply(nbr, s, p, alpha)
            pAp = dot(p, Ap)
            bad = act & ~(pAp > 0)
            retired |= bad
            act &= ~bad
            a = rr / pAp
            xn = x + a * p
            rn_vec = r - a * Ap
            rn = dot(rn_vec, rn_vec)
            b = rn / rr
            pn = rn_vec + b * p
            x = np.where(act, xn, x)
            r = np.where(act, rn_vec, r)
            p = np.where(act, pn, p)
            rr = np.where(act, rn, rr)
            steps += act
    return x, steps, rr, yy


def dense_solve(nbr, s, Y, alpha):
    return np.linalg.solve(np.eye(nbr.shape[0]) - alpha * dense(nbr, s), Y)


def residual_norm(nbr, s, Y, F, alpha):
    """|y - (I - alpha S) f|_2 per column, recomputed from f"""
    return np.sqrt(((Y - apply(nbr, s, F, alpha)) ** 2).sum(axis=0))


# ------------------------------------------------------------------------------------------------ ranking
def rank_scores(F, k):
    """F (N, nq) -> (idx (nq, k) int64, val (nq, k)): score descending, index ascending, NaN last"""
    Ft = np.ascontiguousarray(F.T) + 0.0                          # -0 ranks as +0
    nan = np.isnan(Ft)
    key = np.where(nan, -np.inf, Ft)
    order = np.lexsort((np.broadcast_to(np.arange(Ft.shape[1]), Ft.shape), -key, nan), axis=1)[:, :k]
    return order.astype(np.int64), np.take_along_axis(Ft, order, axis=1)


def cosine_rank(Q, X, k):
    """plain cosine ranking in float64 (score descending, index ascending)"""
    Q = np.asarray(Q, np.float64)
    X = np.asarray(X, np.float64)
    S = (Q / np.linalg.norm(Q, axis=1, keepdims=True)) @ (X / np.linalg.norm(X, axis=1, keepdims=True)).T
    order = np.lexsort((np.broadcast_to(np.arange(S.shape[1]), S.shape), -S), axis=1)[:, :k]
    return order.astype(np.int64), np.take_along_axis(S, order, axis=1)


def diffuse_rank(g, qidx, qval, gamma, alpha, tol, maxiter, k):
    """query lists (nq, kq) against graph g -> (idx, val, steps, rr, yy)"""
    Y = rhs(qidx, qval, g["nbr"].shape[0], gamma)
    x, steps, rr, yy = cg(g["nbr"], g["s"], Y, alpha, tol, maxiter)
    return rank_scores(x, k) + (steps, rr, yy)


# ------------------------------------------------------------------------------------------------ the curves corpus
def curves(seed=0, classes=32, per_class=32, dim=64, nq=256, noise=0.5):
    """`classes` open curves in `dim` dimensions, `per_class` database rows spread along each, `nq` queries at random positions on
    random curves; every row gets Gaussian noise about `noise` times the spacing of neighbouring rows along a curve long.  A curve
    bends through several directions, so its two ends are far apart in cosine while each row is close to the next: the case
    diffusion is for.  -> (X (N, dim) float32, labels, Q (nq, dim) float32, query labels)"""
    rng = np.random.default_rng(seed)
    centre = rng.standard_normal((classes, dim))
    basis = rng.standard_normal((classes, 4, dim))

    def point(c, t):
        ang = np.pi * t
        return (centre[c] + 2.0 * (np.cos(ang)[:, None] * basis[c, 0] + np.sin(ang)[:, None] * basis[c, 1]
                                   + np.cos(2 * ang)[:, None] * basis[c, 2] + np.sin(2 * ang)[:, None] * basis[c, 3]))

    t_db = np.tile(np.linspace(0.0, 1.0, per_class), classes)
    lab = np.repeat(np.arange(classes), per_class)
    X = point(lab, t_db)
    spacing = np.linalg.norm(X[1] - X[0])
    sigma = noise * spacing / np.sqrt(dim)                          # per coordinate: the noise vector is about noise * spacing long
    X = X + sigma * rng.standard_normal(X.shape)
    ql = rng.integers(0, classes, nq)
    Q = point(ql, rng.random(nq)) + sigma * rng.standard_normal((nq, dim))
    return X.astype(np.float32), lab, Q.astype(np.float32), ql


def precision(idx, labels, qlabels):
    return float((labels[idx] == np.asarray(qlabels)[:, None]).mean())
