"""float64 NumPy restatements of the vocabulary-training passes (csrc/learn.hip, launch_gmm_em_step in csrc/fisher.hip, and the
host halves in pvsim/learn.py): greedy k-means++, the Lloyd step and its host update, per-label sums, the Gram matrix, the EM
step's sufficient statistics.  Plain NumPy, no device.

On LATTICE inputs (small integers stored as float32, see lattice_ok) every squared distance, every |c|^2 - 2 x.c score, every
fp32 sum over a 4096-row chunk and every fp64 sum is an exact integer, whatever the order of the additions.  The device's results
then EQUAL the values formed here: distances and potentials bit for bit, drawn indices index for index, labels with first-minimum
ties, sums, counts and inertia -- no tolerance, no near-tie exception.  The EM step (exp, log) is not exact; it keeps tolerances."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(REPO, "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(REPO, "oracle"))

import pvsim_oracle as orc  # noqa: E402

CHUNK = 4096          # rows per fp32 partial sum of the Lloyd step / label sums, and per block of the seeding's draw
EXACT = 2.0 ** 24     # integers below this are exact in float32


def lattice_ok(x, *others):
    """Asserts the exact regime for rows `x` (n, D) and further (m, D) tables (centres, candidates): float32, integer valued,
    non-negative, and with M the largest value:
      3 D M^2 < 2^24   every partial sum of (x - c)^2 (at most D M^2), of x.c (at most D M^2) and of |c|^2 - 2 x.c (within
                       [-2 D M^2, D M^2]) is an integer that float32 holds exactly, in any order, fused or not;
      4096 M^2 < 2^24  so is every fp32 sum of x - c, x or fl32(x^2) over a chunk of 4096 rows.
    -> M"""
    arrs = [np.asarray(x)] + [np.asarray(o) for o in others]
    D = arrs[0].shape[1]
    M = 0.0
    for a in arrs:
        assert a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == D, (a.dtype, a.shape)
        assert np.array_equal(a, np.rint(a)), "not integer valued"
        assert a.min() >= 0, "negative entries: (x - c)^2 is no longer bounded by M^2"
        M = max(M, float(a.max()))
    assert 3 * D * M * M < EXACT, (D, M)
    assert CHUNK * M * M < EXACT, M
    return M


def sqdist(x, c):
    """|x_i - c_j|^2 in float64 -> (m, n)"""
    x64 = np.asarray(x, np.float64)
    c64 = np.asarray(c, np.float64).reshape(-1, x64.shape[1])
    return np.stack([((x64 - cj) ** 2).sum(1) for cj in c64])


# ------------------------------------------------------------------------------------------------ k-means++
def block_sums(mind):
    """sums of mind over blocks of 4096 entries (pvs_min_update_dev)"""
    mind = np.asarray(mind, np.float64)
    return np.add.reduceat(mind, np.arange(0, len(mind), CHUNK))


def draw_flat(mind, r):
    """candidate_ids of sklearn's _kmeans_plusplus: searchsorted(cumsum(mind), r), clipped to n - 1"""
    cum = np.cumsum(np.asarray(mind, np.float64))
    return np.minimum(np.searchsorted(cum, r), len(cum) - 1).astype(np.int64)


def draw_two_level(mind, r):
    """The device's draw, restated: the 4096-entry block from the running sum of the block sums (pvsim/learn.py:_draw_candidates /
    the `u` branch of learn_pick_kernel), inside it the run of 64 entries, inside that the position; entries past the end of a short
    last block count as zeros and the position is clipped to the block's last row."""
    mind = np.asarray(mind, np.float64)
    n = len(mind)
    bs = block_sums(mind)
    cum = np.cumsum(bs)
    out = np.empty(len(r), np.int64)
    for c, tgt in enumerate(np.asarray(r, np.float64)):
        b = min(int(np.searchsorted(cum, tgt)), len(cum) - 1)
        run = cum[b - 1] if b > 0 else 0.0
        lo = b * CHUNK
        cnt = min(CHUNK, n - lo)
        vals = np.zeros(CHUNK)
        vals[:cnt] = mind[lo:lo + cnt]
        part = vals.reshape(64, 64).sum(1)
        sub = 63
        for q in range(64):
            if run + part[q] >= tgt:
                sub = q
                break
            run += part[q]
        pos = min(sub * 64 + 63, cnt - 1)
        for i in range(64):
            run += vals[sub * 64 + i]
            if run >= tgt:
                pos = sub * 64 + i
                break
        out[c] = lo + min(pos, cnt - 1)
    return out


def kmeanspp(x, K, first, u, trace=None):
    """Greedy k-means++ as pvsim/learn.py restates sklearn's _kmeans_plusplus: `first` is the first index, u[c - 1] are the
    uniforms of step c (targets u * potential), candidates = min(searchsorted(cumsum(mind), r), n - 1), the winner is the
    np.argmin of sum(min(mind, d_j)).  -> (indices (K,), potentials (K,): the potential after every step).
    `trace` (a list) receives per step (candidate indices, candidate potentials, winning slot)."""
    n = len(x)
    u = np.asarray(u, np.float64).reshape(max(K - 1, 0), -1)
    idx = np.empty(K, np.int64)
    pots = np.empty(K, np.float64)
    idx[0] = first
    mind = sqdist(x, x[first])[0]
    pots[0] = mind.sum()
    for c in range(1, K):
        cand = draw_flat(mind, u[c - 1] * pots[c - 1])
        d = sqdist(x, x[cand])
        p = np.minimum(mind[None, :], d).sum(1)
        j = int(np.argmin(p))
        if trace is not None:
            trace.append((cand, p, j))
        idx[c], pots[c] = cand[j], p[j]
        mind = np.minimum(mind, d[j])
    return idx, pots


# ------------------------------------------------------------------------------------------------ Lloyd
def lloyd_stats(x, centres, prev_labels=None):
    """One pass of pvs_kmeans_step_dev: labels = FIRST argmin of |c|^2 - 2 x.c, per-cluster sum of (x - c_label), counts,
    per-row squared distance to the own centre, inertia, number of labels that differ from prev_labels (0 without them).
    -> (labels int32, resid (K, D), counts (K,), sqdist (n,), inertia, changed)"""
    x64, c64 = np.asarray(x, np.float64), np.asarray(centres, np.float64)
    K = len(c64)
    labels = np.empty(len(x64), np.int32)
    for r0 in range(0, len(x64), 8192):                      # row blocks: (n, K) scores at K = 2048 stay small
        xb = x64[r0:r0 + 8192]
        labels[r0:r0 + 8192] = np.argmin((c64 * c64).sum(1)[None, :] - 2.0 * (xb @ c64.T), axis=1)
    diff = x64 - c64[labels]
    resid = np.zeros_like(c64)
    np.add.at(resid, labels, diff)
    counts = np.bincount(labels, minlength=K).astype(np.float64)
    sq = (diff * diff).sum(1)
    changed = 0 if prev_labels is None else int((labels != np.asarray(prev_labels)).sum())
    return labels, resid, counts, sq, float(sq.sum()), changed


def farthest_rows(sq, m):
    """the m rows with the largest squared distance, largest first (ties: lower index first), and the (m+1)-th value"""
    order = np.lexsort((np.arange(len(sq)), -np.asarray(sq, np.float64)))
    nxt = float(sq[order[m]]) if len(sq) > m else -np.inf
    return order[:m], nxt


def lloyd_update(x, centres, labels, resid, counts, sq):
    """The host update of pvsim/learn.py:_lloyd in float64: sum_x = resid + count * c; every empty cluster (ascending) takes the
    farthest remaining row (descending distance), which leaves its own cluster (_relocate_empty_clusters_dense); new centre =
    sum_x / count cast to float32, a cluster without members keeps its centre.  -> (centres float32, counts, relocated rows)"""
    c32 = np.asarray(centres, np.float32)
    counts = np.array(counts, np.float64)
    sum_x = np.asarray(resid, np.float64) + counts[:, None] * c32.astype(np.float64)
    empty = np.where(counts == 0)[0]
    far, _ = farthest_rows(sq, len(empty))
    for new_id, i in zip(empty, far):
        xi = np.asarray(x[i], np.float64)
        old = int(labels[i])
        sum_x[old] -= xi
        sum_x[new_id] = xi
        counts[new_id] = 1
        counts[old] -= 1
    new = c32.copy()
    nz = counts > 0
    new[nz] = (sum_x[nz] / counts[nz, None]).astype(np.float32)
    return new, counts, far


# ------------------------------------------------------------------------------------------------ label sums, Gram
def label_sums(x, labels, K, square):
    """pvs_label_sums_dev: per label the sum of x (square = False) or of x * x formed in float32 (square = True), in float64"""
    x = np.asarray(x, np.float32)
    v = (x * x) if square else x
    out = np.zeros((K, x.shape[1]), np.float64)
    np.add.at(out, np.asarray(labels), v.astype(np.float64))
    return out


def gram(x):
    """pvs_gram_dev: column sums and X^T X in float64"""
    x64 = np.asarray(x, np.float64)
    return x64.sum(0), x64.T @ x64


# ------------------------------------------------------------------------------------------------ EM
def em_stats(x, w, mu, cov, block=4096):
    """pvs_gmm_em_step_dev: s0 = sum gamma, s1 = sum gamma x, s2 = sum gamma fl(x * x) (in x's dtype, as scikit-learn forms X * X)
    and sum_i log p(x_i), from the oracle's posterior (orc.gmm_predict_proba) in row blocks."""
    x = np.asarray(x)
    K, D = np.asarray(mu).shape
    s0, s1, s2, ll = np.zeros(K), np.zeros((K, D)), np.zeros((K, D)), 0.0
    for r0 in range(0, len(x), block):
        xb = x[r0:r0 + block]
        resp, lse = orc.gmm_predict_proba(xb, w, mu, cov, return_log_prob_norm=True)
        s0 += resp.sum(0)
        s1 += resp.T @ xb
        s2 += resp.T @ (xb * xb)
        ll += float(lse.sum())
    return s0, s1, s2, ll


def m_step(s0, s1, s2, n, reg_covar=1e-6):
    """_estimate_gaussian_parameters ('diag') + the weights of GaussianMixture._m_step -> (weights, means, covariances)"""
    nk = s0 + 10 * np.finfo(np.float64).eps
    mu = s1 / nk[:, None]
    cov = s2 / nk[:, None] - mu ** 2 + reg_covar
    w = nk / n
    return w / w.sum(), mu, cov
