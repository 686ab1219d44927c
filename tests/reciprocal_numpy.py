"""NumPy twin of k-reciprocal re-ranking (include/pvsim.h): every definition restated with element operations in
float64, each multiply, add and divide rounded on its own, in the stated order -- so the device's results can be compared bit for
bit.  Sets are Python sets and sums are Python floats: slow and plain on purpose.  Plus the dense algorithm of the paper (Zhong,
Zheng, Cao, Li, CVPR 2017) on full matrices with the same weights, the yardstick of what the truncation to a row's own list costs,
and the overlapping-blobs corpus of the quality measurement."""
import numpy as np

from diffusion_numpy import affinity, cosine_rank, precision, rank_scores  # noqa: F401  (precision and cosine_rank are re-exported)

MAX_K1 = 64
MAX_KQ = 1024


def clean(nbr):
    """an index outside [0, N) is stored as -1"""
    nbr = np.asarray(nbr)
    return np.where((nbr >= 0) & (nbr < nbr.shape[0]), nbr, -1).astype(np.int32)


def bits(mask):
    mask = int(mask)
    return [t for t in range(64) if (mask >> t) & 1]


# ------------------------------------------------------------------------------------------------ database side
def back_slot(nbr):
    """u[i][t]: the first slot of row j = nbr[i][t] that holds i; kg where there is none (or j is -1)"""
    N, kg = nbr.shape
    u = np.full((N, kg), kg, np.int64)
    for i in range(N):
        for t in range(kg):
            j = nbr[i, t]
            if j >= 0:
                hit = np.flatnonzero(nbr[j] == i)
                if hit.size:
                    u[i, t] = hit[0]
    return u


def sets(nbr, k1):
    """-> (mask1, maskh) uint64 (N,): bit t of mask1 iff t < k1 and u(i, t) < k1; of maskh the same with k1h = (k1 + 1) // 2"""
    N, kg = nbr.shape
    assert 1 <= k1 <= min(kg, MAX_K1)
    u = back_slot(nbr)
    out = []
    for k in (k1, (k1 + 1) // 2):
        m = np.zeros(N, np.uint64)
        for t in range(k):
            m |= (u[:, t] < k).astype(np.uint64) << np.uint64(t)
        out.append(m)
    return out[0], out[1]


def h_set(j, nbr, maskh):
    return {int(j)} | {int(nbr[j, t]) for t in bits(maskh[j])}


def expanded_set(own, b_ids, nbr, maskh):
    """rule 3: B = {own} + b_ids (own None for a query); E = B + every H(j), j in B without own, with 3 |H(j) & B| > 2 |H(j)|"""
    B = set(int(x) for x in b_ids)
    if own is not None:
        B.add(int(own))
    E = set(B)
    for j in sorted(B):
        if own is not None and j == own:
            continue
        H = h_set(j, nbr, maskh)
        if 3 * len(H & B) > 2 * len(H):
            E |= H
    return B, E


def truncate(E, own, ids):
    """departure 1: flag[t] = 1 iff ids[t] is a member other than own and t is the first slot that holds it -> (flags uint8,
    members dropped)"""
    flags = np.zeros(len(ids), np.uint8)
    seen = set()
    for t, m in enumerate(ids):
        m = int(m)
        if m < 0 or m in seen:
            continue
        seen.add(m)
        if m != own and m in E:
            flags[t] = 1
    return flags, len(E - seen - {own})


def members(nbr, mask1, maskh):
    """-> (flags uint8 (N, kg), dropped int32 (N,))"""
    N, kg = nbr.shape
    flags = np.zeros((N, kg), np.uint8)
    dropped = np.zeros(N, np.int32)
    for i in range(N):
        _, E = expanded_set(i, [nbr[i, t] for t in bits(mask1[i])], nbr, maskh)
        flags[i], dropped[i] = truncate(E, i, nbr[i])
    return flags, dropped


def weights(sim, flags, gamma):
    """departure 2: the affinity of the members, the self weight 1, the sum from +0 with self first and t ascending -> (v, v0)"""
    N, kg = flags.shape
    a = affinity(sim, gamma)
    v = np.zeros((N, kg))
    v0 = np.zeros(N)
    for i in range(N):
        s = 0.0 + 1.0
        for t in range(kg):
            if flags[i, t]:
                s = s + a[i, t]
        v0[i] = 1.0 / s
        for t in range(kg):
            if flags[i, t]:
                v[i, t] = a[i, t] / s
    return v, v0


def vec(j, m, nbr, v, v0):
    """V_j[m]: v0[j] when m = j, v[j][first slot holding m] when m sits in row j, +0 otherwise"""
    if m == j:
        return float(v0[j])
    hit = np.flatnonzero(nbr[j] == m)
    return float(v[j, hit[0]]) if hit.size else 0.0


def expand(nbr, v, v0, k2):
    """local expansion of every row over itself and its first k2 - 1 neighbours -> (w (N, kg), w0, ws)"""
    N, kg = nbr.shape
    assert 1 <= k2 <= kg + 1
    w, w0, ws = np.zeros((N, kg)), np.zeros(N), np.zeros(N)
    for i in range(N):
        src = [i] + [int(j) for j in nbr[i, :k2 - 1] if j >= 0]

        def mean(m):
            acc = 0.0
            for j in src:
                acc = acc + vec(j, m, nbr, v, v0)
            return acc / float(k2)
        w0[i] = mean(i)
        for t in range(kg):
            if nbr[i, t] >= 0:
                w[i, t] = mean(int(nbr[i, t]))
        s = 0.0 + w0[i]
        for t in range(kg):
            s = s + w[i, t]
        ws[i] = s
    return w, w0, ws


def database(nbr, sim, k1=20, k2=6, gamma=3):
    """lists without self -> dict of every stage"""
    nbr = clean(nbr)
    sim = np.asarray(sim, np.float32)
    mask1, maskh = sets(nbr, k1)
    flags, dropped = members(nbr, mask1, maskh)
    v, v0 = weights(sim, flags, gamma)
    w, w0, ws = expand(nbr, v, v0, k2)
    return {"nbr": nbr, "sim": sim, "mask1": mask1, "maskh": maskh, "members": flags, "dropped": dropped, "v": v, "v0": v0, "w": w,
            "w0": w0, "ws": ws, "k1": k1, "k2": k2, "gamma": gamma}


# ------------------------------------------------------------------------------------------------ query side
def query(db, qidx, qval):
    """rule 7 -> (wq (nq, kq) float64, sq (nq,), dropped int32 (nq,), member flags uint8 (nq, kq))"""
    nbr, sim, k1, k2, gamma = db["nbr"], db["sim"], db["k1"], db["k2"], db["gamma"]
    N = nbr.shape[0]
    qidx = np.asarray(qidx)
    qval = np.asarray(qval, np.float32)
    nq, kq = qidx.shape
    ids = np.where((qidx >= 0) & (qidx < N), qidx, -1).astype(np.int64)
    a = affinity(qval, gamma)
    wq, sq = np.zeros((nq, kq)), np.zeros(nq)
    dropped, flags = np.zeros(nq, np.int32), np.zeros((nq, kq), np.uint8)
    for q in range(nq):
        B = []
        for t in range(min(k1, kq)):
            g = ids[q, t]
            if g >= 0 and nbr[g, k1 - 1] >= 0 and qval[q, t] >= sim[g, k1 - 1]:      # float32 against float32; false for a NaN
                B.append(g)
        _, E = expanded_set(None, B, nbr, db["maskh"])
        flags[q], dropped[q] = truncate(E, None, ids[q])
        s = 0.0
        for t in range(kq):
            if flags[q, t]:
                s = s + a[q, t]
        vq = np.zeros(kq)
        if s > 0:
            for t in range(kq):
                if flags[q, t]:
                    vq[t] = a[q, t] / s
        first = {}
        for t in range(kq):
            if ids[q, t] >= 0:
                first.setdefault(int(ids[q, t]), t)
        src = [int(g) for g in ids[q, :k2 - 1] if g >= 0]
        for t in range(kq):
            m = int(ids[q, t])
            if m < 0:
                continue
            acc = 0.0 + vq[first[m]]
            for g in src:
                acc = acc + vec(g, m, nbr, db["v"], db["v0"])
            wq[q, t] = acc / float(k2)
        s = 0.0
        for t in range(kq):
            s = s + wq[q, t]
        sq[q] = s
    return wq, sq, dropped, flags


def score(db, qidx, qval, wq, sq, kr, lam):
    """rule 8 -> scores float64 (nq, kr)"""
    nbr, w, w0, ws = db["nbr"], db["w"], db["w0"], db["ws"]
    N, kg = nbr.shape
    qidx = np.asarray(qidx)
    qval = np.asarray(qval, np.float32)
    nq, kq = qidx.shape
    assert 1 <= kr <= kq and 0.0 <= lam <= 1.0
    out = np.zeros((nq, kr))
    for q in range(nq):
        first = {}
        for t in range(kq):
            if 0 <= qidx[q, t] < N:
                first.setdefault(int(qidx[q, t]), t)
        for r in range(kr):
            c = int(qidx[q, r])
            J = 0.0
            if 0 <= c < N:
                m_sum = 0.0 + min(wq[q, first[c]], w0[c])
                seen = {c}
                for s in range(kg):
                    m = int(nbr[c, s])
                    if m < 0 or m in seen:
                        continue
                    seen.add(m)
                    if m in first:
                        m_sum = m_sum + min(wq[q, first[m]], w[c, s])
                den = (sq[q] + ws[c]) - m_sum
                J = m_sum / den if den > 0 else 0.0
            with np.errstate(invalid="ignore"):
                out[q, r] = np.float64(1.0 - lam) * np.float64(J) + np.float64(lam) * np.float64(qval[q, r])
    return out


def rerank(db, qidx, qval, k, kr=None, lam=0.3):
    """the whole query side -> (idx int64 (nq, k), val float64 (nq, k), report dict)"""
    qidx = np.asarray(qidx)
    kr = qidx.shape[1] if kr is None else kr
    wq, sq, dropped, flags = query(db, qidx, qval)
    sc = score(db, qidx, qval, wq, sq, kr, lam)
    pos, val = rank_scores(sc.T, k)
    return np.take_along_axis(qidx.astype(np.int64), pos, axis=1), val, {"wq": wq, "sq": sq, "dropped": dropped, "members": flags,
                                                                            "scores": sc}


def lists(X, kg):
    """the lists of the rows of X against X in float64 cosine, self dropped by position (for the CPU tests; the GPU tests feed the
    twin with the index's own lists)"""
    idx, val = cosine_rank(X, X, kg + 1)
    N = idx.shape[0]
    hit = idx == np.arange(N)[:, None]
    drop = np.where(hit.any(axis=1), hit.argmax(axis=1), kg)
    keep = np.arange(kg + 1)[None, :] != drop[:, None]
    return idx[keep].reshape(N, kg).astype(np.int32), val[keep].reshape(N, kg).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the dense algorithm of the paper
def dense_rerank(X, Q, k, k1=20, k2=6, gamma=3, lam=0.3):
    """The paper on full matrices: the same reciprocal sets and the same expansion rule, but every member of E keeps its weight (no
    truncation to a list), the vectors are N long, the local expansion averages whole vectors and the whole database is re-ranked.
    Weights are the affinity, as in the twin.  Plain NumPy sums: a yardstick, not a definition.  -> idx (nq, k)"""
    X64, Q64 = np.asarray(X, np.float64), np.asarray(Q, np.float64)
    Xn = X64 / np.linalg.norm(X64, axis=1, keepdims=True)
    Qn = Q64 / np.linalg.norm(Q64, axis=1, keepdims=True)
    S, Sq = Xn @ Xn.T, Qn @ Xn.T
    N, nq = S.shape[0], Sq.shape[0]
    Sx = S.copy()
    np.fill_diagonal(Sx, -np.inf)
    order = np.lexsort((np.broadcast_to(np.arange(N), S.shape), -Sx), axis=1)
    nbr = order[:, :k1].astype(np.int32)
    mask1, maskh = sets(nbr, k1)
    A = affinity(S, gamma)
    V = np.zeros((N, N))
    for i in range(N):
        _, E = expanded_set(i, [nbr[i, t] for t in bits(mask1[i])], nbr, maskh)
        E = sorted(E - {i})
        V[i, E] = A[i, E]
        V[i, i] = 1.0
        V[i] /= V[i].sum()
    W = V.copy()
    for j in range(k2 - 1):
        W += V[order[:, j]]
    W /= k2
    qorder = np.lexsort((np.broadcast_to(np.arange(N), Sq.shape), -Sq), axis=1)
    Aq = affinity(Sq, gamma)
    kth = np.take_along_axis(S, nbr[:, k1 - 1:k1].astype(np.int64), axis=1)[:, 0]
    out = np.zeros((nq, k), np.int64)
    for q in range(nq):
        B = [g for g in qorder[q, :k1] if Sq[q, g] >= kth[g]]
        _, E = expanded_set(None, B, nbr, maskh)
        vq = np.zeros(N)
        E = sorted(E)
        vq[E] = Aq[q, E]
        if vq.sum() > 0:
            vq /= vq.sum()
        wq = vq.copy()
        for j in range(k2 - 1):
            wq += V[qorder[q, j]]
        wq /= k2
        m_sum = np.minimum(wq[None, :], W).sum(axis=1)
        den = wq.sum() + W.sum(axis=1) - m_sum
        J = np.where(den > 0, m_sum / np.where(den > 0, den, 1.0), 0.0)
        sc = (1.0 - lam) * J + lam * Sq[q]
        out[q] = np.lexsort((np.arange(N), -sc))[:k]
    return out


# ------------------------------------------------------------------------------------------------ the blobs corpus
def blobs(seed=0, classes=32, per_class=32, dim=64, nq=256, spread=1.6):
    """`classes` centres drawn N(0, I) in `dim` dimensions, `per_class` database rows at centre + spread N(0, I) around each, `nq`
    queries drawn the same way around random centres: the classes overlap, so rows of other classes enter every list -- the case
    k-reciprocal re-ranking is for.  -> (X (N, dim) float32, labels, Q (nq, dim) float32, query labels)"""
    rng = np.random.default_rng(seed)
    centre = rng.standard_normal((classes, dim))
    lab = np.repeat(np.arange(classes), per_class)
    X = centre[lab] + spread * rng.standard_normal((classes * per_class, dim))
    ql = rng.integers(0, classes, nq)
    Q = centre[ql] + spread * rng.standard_normal((nq, dim))
    return X.astype(np.float32), lab, Q.astype(np.float32), ql
