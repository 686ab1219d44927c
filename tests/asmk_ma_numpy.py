"""NumPy twin of the multiple assignment of query rows (include/pvsim.h): the top-m list of a row, the entries
of an image whose rows carry m labels, and the guard a test asserts on its own inputs before it trusts a float64 order.

Written from the definitions of the header, not from the kernels.  `topm` ranks in float64; `v_chain` restates the float32 value the
header defines (the fma chain in the stated order), for the inputs on which the float64 value is not exactly a float32."""
import numpy as np

import asmk_numpy as tw

F = np.float32
MAX_M = 8
MAX_KEYS = 16384


# ------------------------------------------------------------------------------------------------ top-m
def values64(x, c):
    """v_j = |c_j|^2 - 2 x . c_j in float64, (n, K); NaN and +inf count as +inf"""
    x64, c64 = np.asarray(x, np.float64), np.asarray(c, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (c64 * c64).sum(axis=1)[None, :] - 2.0 * (x64 @ c64.T)
    return np.where(v < np.inf, v, np.inf)


def _rank(v, m):
    """the first m columns of every row in the order (v ascending, column ascending)"""
    order = np.argsort(v, axis=1, kind="stable")[:, :m]            # stable: equal values keep ascending columns
    return order.astype(np.int32), np.take_along_axis(v, order, axis=1)


def topm(x, c, m):
    """x (n, D), c (K, D) -> (labels int32 (n, m), v float64 (n, m)): v in float64, ranked by (v, j), NaN as +inf"""
    K = np.asarray(c).shape[0]
    if isinstance(m, bool) or int(m) != m or not (1 <= m <= min(K, MAX_M)):
        raise ValueError(f"m must lie in 1..{min(K, MAX_M)}, got {m!r}")
    return _rank(values64(x, c), int(m))


def _fma32(a, b, acc):
    """float32 fma(a, b, acc), correctly rounded: the product of two float32 is exact in float64; its sum with acc is rounded to
    odd in float64 (TwoSum gives the error's sign), and 53 >= 24 + 2 bits make the final rounding to float32 the single one"""
    p = a.astype(np.float64) * b.astype(np.float64)
    z = acc.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + z
        bb = s - p
        err = (p - (s - bb)) + (z - bb)
    fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(F)


def cnorm32(c):
    """|c_j|^2 as the codebook stores it: a sequential float32 sum of float32 squares"""
    c = np.asarray(c, F)
    s = np.zeros(c.shape[0], F)
    for d in range(c.shape[1]):
        s = s + c[:, d] * c[:, d]
    return s


def v_chain(x, c):
    """the float32 v of the header, (n, K): dot starts at +0 and runs over the dims (8t + e, 8t + 4 + e), e = 0..3, t ascending, one
    fma each; v = fma(-2, dot, |c|^2); NaN and +inf count as +inf"""
    x, c = np.asarray(x, F), np.asarray(c, F)
    n, D = x.shape
    dot = np.zeros((n, c.shape[0]), F)
    with np.errstate(invalid="ignore", over="ignore"):
        for b8 in range(0, D, 8):
            for e in range(4):
                for d in (b8 + e, b8 + 4 + e):
                    if d < D:
                        dot = _fma32(np.broadcast_to(c[None, :, d], dot.shape), np.broadcast_to(x[:, None, d], dot.shape), dot)
        v = _fma32(np.full(dot.shape, -2, F), dot, np.broadcast_to(cnorm32(c)[None, :], dot.shape))
    return np.where(v < np.inf, v, F(np.inf)).astype(F)


def topm_chain(x, c, m):
    """the list of the header from its own float32 values -> (labels int32 (n, m), v float32 (n, m))"""
    return _rank(v_chain(x, c), int(m))


def rank_gap_ratios(x, c, m):
    """per row: the smallest gap between consecutive float64 v among the ranks 1 .. m + 1, over 2^-12 (|x| max|c| + max|c|^2)
    -> float64 (n,); +inf where there is nothing to compare"""
    x64, c64 = np.asarray(x, np.float64), np.asarray(c, np.float64)
    K = c64.shape[0]
    if len(x64) == 0 or K < 2:
        return np.full(len(x64), np.inf)
    v = np.sort(values64(x, c), axis=1)[:, :min(K, m + 1)]
    with np.errstate(invalid="ignore"):
        gap = np.diff(v, axis=1)
    cmax = np.sqrt((c64 * c64).sum(axis=1).max())
    thr = 2.0 ** -12 * (np.sqrt((x64 * x64).sum(axis=1)) * cmax + cmax * cmax)
    return (np.where(np.isnan(gap), 0.0, gap) / thr[:, None]).min(axis=1)


def rank_gaps(x, c, m):
    """True when the float64 order of the first m + 1 ranks of every row can be trusted for the float32 values of the header: the
    smallest gap between consecutive float64 v among the ranks 1 .. m + 1 exceeds 2^-12 (|x| max|c| + max|c|^2).
    A 128-term float32 chain errs by at most 128 2^-24 of sum |x_t c_t| <= |x| |c|, doubled by the -2, plus the same on |c|^2: less
    than 2^-16 of that scale.  The guard is 16 times that.  -> (ok, smallest gap / its threshold)"""
    r = rank_gap_ratios(x, c, m)
    return bool((r > 1.0).all()), float(r.min(initial=np.inf))


# ------------------------------------------------------------------------------------------------ entries
def image_entries_ma(x, labels_nm, c, proj=None):
    """x float32 (n, D) in row order, labels_nm (n, m) with the m labels of a row distinct -> (words int32 (E,) ascending, sigs
    uint32 (E, B / 32)): the entries are the distinct labels over all rows and slots; V of word w adds (x_j - c_w) for j ascending
    over the rows that hold w in any slot; float32 element operations as in asmk_numpy.image_entries"""
    x, c = np.asarray(x), np.asarray(c)
    lab = np.asarray(labels_nm)
    assert x.dtype == F and c.dtype == F and lab.ndim == 2 and lab.shape[0] == x.shape[0]
    n, D = x.shape
    m = lab.shape[1]
    if n > tw.MAX_ROWS or n * m > MAX_KEYS:
        raise NotImplementedError(f"an image of {n} rows x {m} labels exceeds {tw.MAX_ROWS} rows or {MAX_KEYS} keys")
    for r in range(n):
        assert len(set(lab[r].tolist())) == m, f"row {r}: its labels are not distinct"
    B = D if proj is None else np.asarray(proj).shape[0]
    assert B in (32, 64, 96, 128)
    words = np.unique(lab).astype(np.int32)
    sigs = np.zeros((len(words), B // 32), np.uint32)
    for e, w in enumerate(words):
        V = np.zeros(D, F)
        for j in np.flatnonzero((lab == w).any(axis=1)):           # ascending j
            V = V + (x[j] - c[w])                                   # one float32 subtraction, one float32 addition
        if proj is None:
            z = V
        else:
            P = np.asarray(proj)
            assert P.dtype == F and P.shape == (B, D)
            z = np.zeros(B, F)
            for u in range(D):                                      # u ascending: a multiply, then an add
                z = z + P[:, u] * V[u]
        sigs[e] = tw.signature(z)
    return words, sigs


def entries_ma(images, c, m, proj=None):
    """list of float32 (n_i, D) arrays -> list of (words, sigs) with the float64 top-m labels of every row"""
    return [image_entries_ma(x, topm(x, c, m)[0] if len(x) else np.zeros((0, m), np.int32), c, proj) for x in images]


# ------------------------------------------------------------------------------------------------ the planted corpus
def planted_corpus_ma(seed=11, side=4, D=32, n_images=400, n_queries=60, rows=(6, 12), sigma=2.0, clutter=40):
    """A corpus on which a query row often leaves its cell.  The vocabulary is a lattice of side^5 = 1024 words: the first five
    coordinates run over 4 * {0 .. side - 1}, the rest are 0.  A database image is 6..11 rows at random words plus uniform noise in
    [-1, 1] on every coordinate (inside its cell: the cell's half width is 2).  A query is half of an image's rows plus Gaussian
    noise of `sigma` on the five lattice coordinates (at sigma = 2, the cell's half width, about three quarters of the rows change
    their nearest word), plus `clutter` rows at random words.  float32 rows.
    -> (centroids, images, queries, truth, moved) with `moved` the share of the perturbed rows whose nearest word changed"""
    rng = np.random.RandomState(seed)
    K = side ** 5
    cent = np.zeros((K, D), F)
    w = np.arange(K)
    for a in range(5):
        cent[:, a] = ((w // side ** a) % side) * 4
    lo, hi = rows

    def near(words):
        return (cent[words] + rng.uniform(-1, 1, (len(words), D))).astype(F)

    images = [near(rng.randint(0, K, rng.randint(lo, hi))) for _ in range(n_images)]
    truth = rng.permutation(n_images)[:n_queries]
    queries, changed, total = [], 0, 0
    for i in truth:
        x = images[i]
        keep = np.sort(rng.permutation(len(x))[:max(1, len(x) // 2)])
        part = x[keep].astype(np.float64)
        part[:, :5] += rng.standard_normal((len(part), 5)) * sigma
        part = part.astype(F)
        changed += int((topm(part, cent, 1)[0][:, 0] != topm(x[keep], cent, 1)[0][:, 0]).sum())
        total += len(part)
        queries.append(np.concatenate([part, near(rng.randint(0, K, clutter))]))
    return cent, images, queries, truth, changed / max(total, 1)


def recall_at_1(cent, images, queries, truth, ma, bits=32):
    """share of the queries whose own image ranks first: database single assignment, queries at `ma` words per row"""
    db = tw.entries(images, cent, None)
    K = len(cent)
    wt, sel = tw.word_weights(db, K), tw.selectivity(bits, 3.0, 0.0)
    word_off, ent_img, ent_sig = tw.invert(db, K)
    gdb = np.array([tw.gamma(e[0], wt) for e in db], F)
    q = entries_ma(queries, cent, ma, None) if ma > 1 else tw.entries(queries, cent, None)
    score = tw.scores_inverted(q, word_off, ent_img, ent_sig, len(images), wt, sel, gdb)
    idx, _ = tw.rank(score, 1)
    return float((idx[:, 0] == np.asarray(truth)).mean())
