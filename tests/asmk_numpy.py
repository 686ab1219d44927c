"""NumPy twin of the ASMK* index (include/pvsim.h): entries (word, binary signature of the summed residual),
integer weights, gamma, the selectivity table, the score by a plain double loop over image pairs, and the ranking.

Written from the definitions of the header, not from the kernels: float32 values come from np.float32 ELEMENT operations in the
defined order (vectorised only across the independent coordinates t), integers from Python / int64 arithmetic.  The device kernels
and pvsim.asmk must agree with this bit for bit."""
import math

import numpy as np

import topk_numpy as tk

F = np.float32
SCALE = 1023            # sel[0] and the factor of gamma
IDF_SCALE = 64          # wt = rint(64 ln(N / df))
MAX_ROWS = 8192


# ------------------------------------------------------------------------------------------------ rows and labels
def rootsift(raw):
    """raw (n, D) uint8 or float32 SIFT rows -> float32 sqrt(raw / (sum + 1e-7)), element operations in float32"""
    x = np.asarray(raw).astype(F)
    s = x.sum(axis=1, dtype=F) if x.shape[1] else np.zeros(len(x), F)       # integer-valued rows: any order gives the same sum
    return np.sqrt(x / (s[:, None] + F(1e-7)))


def labels_and_gap(x, centroids):
    """nearest centroid of every row in float64 (ties to the lowest index) and the smallest relative gap between the best and the
    second best squared distance: a test asserts the gap of its own inputs before it trusts the labels"""
    x64, c64 = np.asarray(x, np.float64), np.asarray(centroids, np.float64)
    d = (x64 * x64).sum(axis=1)[:, None] - 2.0 * (x64 @ c64.T) + (c64 * c64).sum(axis=1)[None, :]   # (n, K) only: K may be 65536
    lab = d.argmin(axis=1).astype(np.int32)
    if c64.shape[0] < 2 or len(x64) == 0:
        return lab, np.inf
    part = np.partition(d, 1, axis=1)
    gap = (part[:, 1] - part[:, 0]) / np.maximum(part[:, 1], 1e-300)
    return lab, float(gap.min())


def random_projection(bits, dim, random_state=0):
    """a seeded matrix with orthonormal rows (bits <= dim) or columns (bits > dim): Q of the QR of a normal draw, float32 (bits, dim)"""
    rng = np.random.RandomState(random_state)
    m = max(bits, dim)
    q, r = np.linalg.qr(rng.standard_normal((m, m)))
    q = q * np.sign(np.where(np.diag(r) == 0, 1.0, np.diag(r)))[None, :]
    return np.ascontiguousarray(q[:bits, :dim], dtype=F)


# ------------------------------------------------------------------------------------------------ entries
def signature(z):
    """z float32 (B,) -> uint32 (B / 32,): bit t is 1 iff z[t] >= 0, in word t / 32 at position t % 32"""
    B = len(z)
    assert B % 32 == 0
    out = np.zeros(B // 32, np.uint32)
    for t in range(B):
        if z[t] >= 0:
            out[t // 32] |= np.uint32(1) << np.uint32(t % 32)
    return out


def image_entries(x, labels, centroids, proj=None, bits=None):
    """x float32 (n, D) in row order, labels (n,) -> (words int32 (E,) ascending, sigs uint32 (E, B / 32))"""
    x, c = np.asarray(x), np.asarray(centroids)
    assert x.dtype == F and c.dtype == F
    n, D = x.shape
    if n > MAX_ROWS:
        raise NotImplementedError(f"an image of {n} rows exceeds {MAX_ROWS}")
    B = D if proj is None else np.asarray(proj).shape[0]
    assert bits is None or bits == B
    assert B in (32, 64, 96, 128)
    words = np.unique(np.asarray(labels)).astype(np.int32)
    sigs = np.zeros((len(words), B // 32), np.uint32)
    for e, w in enumerate(words):
        V = np.zeros(D, F)
        for j in np.flatnonzero(np.asarray(labels) == w):          # ascending j
            V = V + (x[j] - c[w])                                   # one float32 subtraction, one float32 addition
        if proj is None:
            z = V
        else:
            P = np.asarray(proj)
            assert P.dtype == F and P.shape == (B, D)
            z = np.zeros(B, F)
            for u in range(D):                                      # u ascending: a multiply, then an add
                z = z + P[:, u] * V[u]
        sigs[e] = signature(z)
    return words, sigs


def entries(images, centroids, proj=None, labels=None):
    """list of float32 (n_i, D) arrays -> list of (words, sigs); labels default to the float64 nearest centroid"""
    out = []
    for i, x in enumerate(images):
        lab = labels_and_gap(x, centroids)[0] if labels is None else labels[i]
        out.append(image_entries(x, lab, centroids, proj))
    return out


# ------------------------------------------------------------------------------------------------ integer weights
def selectivity(bits, alpha=3.0, tau=0.0):
    """sel int32 (B + 1,): with u = 1 - 2 h / B, rint(1023 u^alpha) where u > tau, 0 otherwise (float64)"""
    assert alpha > 0 and 0 <= tau < 1
    sel = np.zeros(bits + 1, np.int32)
    for h in range(bits + 1):
        u = 1.0 - 2.0 * h / bits
        if u > tau:
            sel[h] = int(np.rint(SCALE * u ** alpha))
    return sel


def word_weights(db_entries, K, idf=True):
    """wt int32 (K,): 0 for a word no database image holds, else clip(rint(64 ln(N / df)), 1, 1023); 64 when idf is off"""
    N = len(db_entries)
    df = np.zeros(K, np.int64)
    for words, _ in db_entries:
        df[np.asarray(words, np.int64)] += 1
    wt = np.zeros(K, np.int32)
    for w in np.flatnonzero(df):
        wt[w] = min(max(int(np.rint(IDF_SCALE * math.log(N / df[w]))), 1), 1023) if idf else IDF_SCALE
    return wt


def weight_sum(words, wt):
    """sum of 1023 wt[w] over an image's entries, a Python int"""
    return int(sum(SCALE * int(wt[w]) for w in words))


def gamma(words, wt):
    s = weight_sum(words, wt)
    return F(1.0 / math.sqrt(float(s))) if s > 0 else F(0)


def check_query(words, wt):
    if weight_sum(words, wt) >= 1 << 32:
        raise ValueError("the query's weights sum to 2^32 or more: the integer score could overflow")


# ------------------------------------------------------------------------------------------------ score
def popcount(a):
    return sum(bin(int(v)).count("1") for v in a)


def pair_acc(q, x, wt, sel):
    """integer score of two entry lists: sum over shared words of wt[w] sel[popcount(xor)]"""
    qw, qs = q
    xw, xs = x
    pos = {int(w): e for e, w in enumerate(xw)}
    acc = 0
    for e, w in enumerate(qw):
        f = pos.get(int(w))
        if f is not None:
            acc += int(wt[w]) * int(sel[popcount(np.bitwise_xor(qs[e], xs[f]))])
    return acc


def to_score(acc, gq, gx):
    assert 0 <= acc < 1 << 32
    return (F(np.uint32(acc)) * F(gq)) * F(gx)          # uint32 -> float32 rounds to nearest even


def scores(q_entries, db_entries, wt, sel):
    """the plain double loop over image pairs -> float32 (nq, N)"""
    out = np.zeros((len(q_entries), len(db_entries)), F)
    gdb = [gamma(x[0], wt) for x in db_entries]
    for a, q in enumerate(q_entries):
        check_query(q[0], wt)
        gq = gamma(q[0], wt)
        for b, x in enumerate(db_entries):
            out[a, b] = to_score(pair_acc(q, x, wt, sel), gq, gdb[b])
    return out


def rank(score, k):
    """(score descending, image ascending): the rule of pvs_topk_dev"""
    return tk.topk(np.ascontiguousarray(score, dtype=F), k)


# ------------------------------------------------------------------------------------------------ inverted file
def invert(db_entries, K):
    """entries sorted by (word, image) -> (word_off int64 (K + 1,), ent_img int32 (E,), ent_sig uint32 (E, W))"""
    W = db_entries[0][1].shape[1] if db_entries else 1
    rows = [(int(w), i, e) for i, (words, _) in enumerate(db_entries) for e, w in enumerate(words)]
    rows.sort(key=lambda r: (r[0], r[1]))
    word_off = np.zeros(K + 1, np.int64)
    for w, _, _ in rows:
        word_off[w + 1] += 1
    np.cumsum(word_off, out=word_off)
    ent_img = np.array([r[1] for r in rows], np.int32)
    ent_sig = np.array([db_entries[r[1]][1][r[2]] for r in rows], np.uint32).reshape(len(rows), W)
    return word_off, ent_img, ent_sig


def scores_inverted(q_entries, word_off, ent_img, ent_sig, N, wt, sel, gamma_db):
    """the same scores through the inverted file: per query word, walk its list"""
    out = np.zeros((len(q_entries), N), F)
    for a, (qw, qs) in enumerate(q_entries):
        check_query(qw, wt)
        acc = [0] * N
        for e, w in enumerate(qw):
            if not 0 <= w < len(wt):
                continue
            for p in range(int(word_off[w]), int(word_off[w + 1])):
                acc[int(ent_img[p])] += int(wt[w]) * int(sel[popcount(np.bitwise_xor(qs[e], ent_sig[p]))])
        gq = gamma(qw, wt)
        for b in range(N):
            out[a, b] = to_score(acc[b], gq, gamma_db[b])
    return out


# ------------------------------------------------------------------------------------------------ the planted corpus
def planted_corpus(seed=7, D=32, K=64, n_images=96, n_queries=48, clutter=20):
    """Lattice centroids (coordinates in {0, 4}), images of 20..59 rows near centroids, queries = half of an image's rows with a
    fifth of the coordinates moved by +-1, plus `clutter` rows near random centroids.  Integer-valued float32 rows.
    -> (centroids, images, queries, truth)"""
    rng = np.random.RandomState(seed)
    cent = set()
    while len(cent) < K:
        cent.add(tuple((rng.randint(0, 2, D) * 4).tolist()))
    cent = np.array(sorted(cent), F)

    def near(words):
        return (cent[words] + rng.randint(-1, 2, (len(words), D))).astype(F)

    images = [near(rng.randint(0, K, rng.randint(20, 60))) for _ in range(n_images)]
    truth = rng.permutation(n_images)[:n_queries]
    queries = []
    for i in truth:
        x = images[i]
        keep = rng.permutation(len(x))[:max(1, len(x) // 2)]
        part = x[np.sort(keep)].copy()
        move = rng.random_sample(part.shape) < 0.2
        part = part + move * rng.choice([-1.0, 1.0], part.shape)
        queries.append(np.concatenate([part.astype(F), near(rng.randint(0, K, clutter))]))
    return cent, images, queries, truth
