"""NumPy twin of the inverted lists over the int8 code rows (csrc/ivf_sq8.hip, pvsim/ivf_int8.py): the definitions of include/pvsim.h
and DESIGN.md section 26 restated on top of sq8_numpy (imported as it is): encode, factors, acc, scores, topk.

  centroids   code rows: encode(centroid rows) -> cent_codes, cent_inv.
  list        of a database row: the first entry of topk(scores(codes, inv, cent_codes, cent_inv), 1).
  probes      of a query: the first nprobe entries of the same ranking.
  storage     rows sorted by (list, original index): ids, list_off.
  candidates  the probed lists in probe order, padded to W = the nprobe longest lists rounded up to 64, at least 64; padding is
              (-inf, -1); a probe outside [0, nlist) is an empty list.
  result      the first k candidates by a literal argsort on (-score, id); unfilled slots are -1 / -inf.
  training    spherical k-means; the centroid sums use the arithmetic of pvs_combine_rows_dev as expand_numpy.combine restates it.
  updates     insert and remove equal a rebuild from the surviving rows."""
import numpy as np

import expand_numpy as xp
import sq8_numpy as sq

F = np.float32
COMBINE_MEMBERS = 4096


def blas_scores(qcodes, inv_q, codes, inv_d):
    """sq8_numpy.scores with the integer sums formed by a float64 matrix product: every partial sum is an integer below 2^53, so the
    product is exact in any order (the argument of tests/test_sq8_host.py).  For the corpora a test cannot afford in int64."""
    a = qcodes.astype(np.float64) @ codes.astype(np.float64).T
    assert (np.abs(a) < 2 ** 31).all()
    return (a.astype(np.int32).astype(F) * np.asarray(inv_q, F)[:, None]) * np.asarray(inv_d, F)[None, :]


def assign(codes, inv, cent_codes, cent_inv, scores=sq.scores):
    """-> int64 (n,): the best centroid of every code row, ties to the lowest list number"""
    if len(codes) == 0:
        return np.zeros(0, np.int64)
    return sq.topk(scores(codes, inv, cent_codes, cent_inv), 1)[0][:, 0]


def probes(qcodes, inv_q, cent_codes, cent_inv, nprobe, scores=sq.scores):
    """-> int64 (nq, nprobe): the nprobe best lists of every query, best first"""
    return sq.topk(scores(qcodes, inv_q, cent_codes, cent_inv), nprobe)[0]


def sort_into_lists(lists, nlist):
    """list of every row -> (ids int32 (N,): the original index of each stored row, sorted by (list, original index); list_off int64)"""
    lists = np.asarray(lists, np.int64)
    ids = np.lexsort((np.arange(len(lists)), lists)).astype(np.int32)
    list_off = np.zeros(nlist + 1, np.int64)
    for l in range(nlist):
        list_off[l + 1] = list_off[l] + int((lists == l).sum())
    return ids, list_off


def width(list_off, nprobe):
    """W: the nprobe longest lists together, rounded up to 64, at least 64"""
    longest = np.sort(np.diff(list_off))[::-1][:nprobe]
    return max(64, 64 * ((int(longest.sum()) + 63) // 64))


def candidate_rows(qcodes, inv_q, probe, list_off, codes, inv_db, ids, scores=sq.scores):
    """codes / inv_db / ids in STORED order -> (cval float32 (nq, W), cid int32 (nq, W))"""
    nq, nprobe = probe.shape
    nlist = len(list_off) - 1
    W = width(list_off, nprobe)
    cval = np.full((nq, W), -np.inf, F)
    cid = np.full((nq, W), -1, np.int32)
    for q in range(nq):
        rows = [np.arange(list_off[l], list_off[l + 1]) for l in probe[q] if 0 <= l < nlist]
        rows = np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)
        if rows.size:
            cval[q, :rows.size] = scores(qcodes[q:q + 1], inv_q[q:q + 1], codes[rows], inv_db[rows])[0]
            cid[q, :rows.size] = ids[rows]
    return cval, cid


def select(cval, cid, k):
    """the first k live candidates of every row by (score descending, id ascending), -0 and +0 tied -> idx int64, val float32"""
    nq = cval.shape[0]
    idx = np.full((nq, k), -1, np.int64)
    val = np.full((nq, k), -np.inf, F)
    for q in range(nq):
        live = np.flatnonzero(cid[q] >= 0)
        s, i = cval[q, live] + F(0), cid[q, live].astype(np.int64)       # -0 + 0 = +0
        o = np.lexsort((i, -s))[:k]
        idx[q, :o.size], val[q, :o.size] = i[o], s[o]
    return idx, val


def search(qcodes, inv_q, probe, list_off, codes, inv_db, ids, k, scores=sq.scores):
    return select(*candidate_rows(qcodes, inv_q, probe, list_off, codes, inv_db, ids, scores), k)


def build(x, centroids, scores=sq.scores):
    """float32 rows and centroid rows -> dict of every array an IVFInt8Index holds (codes, inv, ids in stored order)"""
    codes, inv = sq.encode(x) if len(x) else (np.zeros((0, sq.ld_of(np.shape(x)[1])), np.int8), np.zeros(0, F))
    cc, ci = sq.encode(centroids)
    ids, list_off = sort_into_lists(assign(codes, inv, cc, ci, scores), len(cc))
    return dict(codes=codes[ids], inv=inv[ids], ids=ids, list_off=list_off, cent_codes=cc, cent_inv=ci)


def rank(q, x, centroids, k, nprobe, scores=sq.scores):
    """float32 queries, rows and centroids -> the lists an IVFInt8Index built from them gives"""
    b = build(x, centroids, scores)
    qc, iq = sq.encode(q)
    pr = probes(qc, iq, b["cent_codes"], b["cent_inv"], nprobe, scores)
    return search(qc, iq, pr, b["list_off"], b["codes"], b["inv"], b["ids"], k, scores)


def train(x, inv_norms, init, max_iter=10, scores=sq.scores):
    """Spherical k-means on the sample rows x float32 (nt, L) with their inverse norms: the initial centroids are the rows x[init]; per
    iteration the centroids are encoded, every sample row is labelled by `assign`, and the centroid of list l becomes the sum of
    inv_norms[i] * x[i] over its members i ascending, added in passes of at most COMBINE_MEMBERS members through the self term of
    combine; an empty list keeps its centroid.  Stops when no label changes or after max_iter iterations.  -> float32 (nlist, L)"""
    x = np.ascontiguousarray(x, F)
    inv_norms = np.asarray(inv_norms, F)
    cent = x[np.asarray(init, np.int64)].copy()
    nlist = len(cent)
    xc, xi = sq.encode(x)
    prev = None
    for _ in range(max_iter):
        cc, ci = sq.encode(cent)
        labels = assign(xc, xi, cc, ci, scores)
        if prev is not None and np.array_equal(labels, prev):
            break
        members = [np.flatnonzero(labels == l) for l in range(nlist)]
        most = max(1, max(len(m) for m in members))
        idx = np.full((nlist, most), -1, np.int64)
        for l, m in enumerate(members):
            idx[l, :len(m)] = m
        w = np.where(idx >= 0, inv_norms[np.where(idx >= 0, idx, 0)], F(0)).astype(F)
        new = None
        for c0 in range(0, most, COMBINE_MEMBERS):
            new = xp.combine(x, idx[:, c0:c0 + COMBINE_MEMBERS], w[:, c0:c0 + COMBINE_MEMBERS], new)
        for l, m in enumerate(members):
            if len(m) == 0:
                new[l] = cent[l]
        cent, prev = new, labels
    return cent


# ------------------------------------------------------------------ the update rule: insert and remove equal a rebuild
def insert(b, new_x):
    """the arrays of `build` after new rows arrive (ids N, N + 1, ...): a list keeps its old rows and appends its new ones in arrival order"""
    codes, inv = sq.encode(new_x)
    lists = assign(codes, inv, b["cent_codes"], b["cent_inv"])
    n, nlist = len(b["ids"]), len(b["cent_codes"])
    out = {k: [] for k in ("codes", "inv", "ids")}
    off = np.zeros(nlist + 1, np.int64)
    for l in range(nlist):
        old = slice(b["list_off"][l], b["list_off"][l + 1])
        mine = np.flatnonzero(lists == l)
        out["codes"] += [b["codes"][old], codes[mine]]
        out["inv"] += [b["inv"][old], inv[mine]]
        out["ids"] += [b["ids"][old], (n + mine).astype(np.int32)]
        off[l + 1] = off[l] + (old.stop - old.start) + len(mine)
    return dict(b, codes=np.concatenate(out["codes"]), inv=np.concatenate(out["inv"]), ids=np.concatenate(out["ids"]).astype(np.int32),
                list_off=off)


def remove(b, removed):
    """the arrays of `build` after the rows with original indices `removed` leave: survivors keep their stored order and are renumbered"""
    n, nlist = len(b["ids"]), len(b["cent_codes"])
    keep = np.ones(n, bool)
    keep[np.asarray(removed, np.int64)] = False
    pos = np.concatenate([[0], np.cumsum(keep)])
    stay = keep[b["ids"]]
    before = np.concatenate([[0], np.cumsum(stay)])
    return dict(b, codes=b["codes"][stay], inv=b["inv"][stay], ids=pos[b["ids"][stay]].astype(np.int32),
                list_off=before[b["list_off"]].astype(np.int64))


def same(a, b):
    """two `build` dicts hold the same bytes"""
    return all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in ("codes", "ids", "list_off", "cent_codes")) and \
        np.array_equal(a["inv"].view(np.uint32), b["inv"].view(np.uint32))
