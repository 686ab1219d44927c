"""tests/neighbors_numpy.py against scikit-learn's recorded results (tests/golden/cluster_*.npz), and the conditions that
tests/test_gpu_neighbors.py relies on, asserted on the very rows it uploads (tests/neighbors_cases.py) -- no GPU needed.

A device test that asserts `filtered` with `overflowed == 0` needs every query's candidate count within its slots; a radius test
needs a pair exactly on the radius to tell `<=` from `<`; the subspace bound of the spectral tests needs the gap it divides by.
These are conditions on the inputs, not measurements of the device."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

import neighbors_cases as nc  # noqa: E402
import neighbors_numpy as nn  # noqa: E402
from cluster_inputs import cluster_set  # noqa: E402
from test_gpu_cluster import _check_lists  # noqa: E402


def _gold(name):
    return np.load(os.path.join(REPO, "tests", "golden", f"cluster_{name}.npz"))


# ------------------------------------------------------------------------------------------------ the restatements are sklearn's
@pytest.mark.parametrize("name", ["easy", "f64"])
def test_knn_lists_reproduce_sklearn(name):
    g = _gold(name)
    X, _ = cluster_set(name)
    idx, sq = nn.knn_lists(X, X, int(g["knn_idx"].shape[1]))
    _check_lists(idx, sq, g["knn_idx"], g["knn_sqdist"], g["norm_sq"])


@pytest.mark.parametrize("name", ["easy", "f64"])
def test_radius_csr_reproduces_sklearn(name):
    g = _gold(name)
    X, _ = cluster_set(name)
    indptr, indices, sq = nn.radius_csr(X, X, float(g["eps"]) ** 2)
    assert np.array_equal(indptr, g["radius_indptr"])
    assert np.array_equal(indices, g["radius_indices"])
    assert len(sq) == indptr[-1] and sq.max() <= float(g["eps"]) ** 2


def test_dense_eigenvalues_reproduce_sklearn():
    g = _gold("easy")
    N, k = g["knn_idx"].shape
    theta, U, dd = nn.normalised_affinity_eigh(np.arange(0, N * k + 1, k), g["knn_idx"].reshape(-1), N)
    m = len(g["laplacian_eigs"])
    assert np.allclose(1.0 - theta[:m], g["laplacian_eigs"], rtol=0, atol=1e-9)


def test_restatements_on_a_case_worked_by_hand():
    X = np.array([[0, 0], [3, 4], [0, 0], [6, 8]], np.float32)
    Q = np.array([[0, 0], [3, 4]], np.float32)
    assert np.array_equal(nn.sqdist(Q, X), [[0, 25, 0, 100], [25, 0, 25, 25]])
    idx, sq = nn.knn_lists(Q, X, 3)
    assert np.array_equal(idx, [[0, 2, 1], [1, 0, 2]]) and np.array_equal(sq, [[0, 0, 25], [0, 25, 25]])
    indptr, indices, rsq = nn.radius_csr(Q, X, 25.0)
    assert np.array_equal(indptr, [0, 3, 7]) and np.array_equal(indices, [0, 1, 2, 0, 1, 2, 3])
    assert np.array_equal(rsq, [0, 25, 0, 25, 0, 25, 25])
    assert np.array_equal(nn.tied_at_kth(Q, X, 2), [2, 4])
    # S = [[0, 2], [0.5, 0]] with the columns of row 1 listed first-to-last, row 0 holding one entry
    Y = nn.spmm([0, 1, 2], [1, 0], [2.0, 0.5], [[1.0, 2.0], [4.0, 8.0]], alpha=2.0, beta=[1.0, -1.0], Z=[[1.0, 1.0], [1.0, 1.0]],
                gamma=0.5)
    assert np.array_equal(Y, [[17.5, 30.5], [5.5, -5.5]])


# ------------------------------------------------------------------------------------------------ conditions of the device tests
@pytest.mark.parametrize("name", sorted(nc.KNN_FILTERED))
def test_filtered_cases_stay_within_their_slots(name):
    Q, X, k = nc.knn_rows(name)
    nn.lattice_ok(Q, X)
    counts, cap = nn.candidate_counts(Q, X, k, same=Q is X)
    assert counts.min() >= k and counts.max() <= cap, (counts.max(), cap)
    generic = nn.candidate_counts(Q, X, k, chain=nn.chain_term(X.shape[1], generic=True), same=Q is X)[0]
    assert generic.max() <= cap
    if name == "margin_L256":        # here the two chain terms keep different candidates: the count shows which one the device used
        assert generic.sum() < counts.sum()


def test_the_slot_counts_cover_every_branch():
    ks = {c[4] for c in nc.KNN_FILTERED.values()}
    assert {1, 7, 10, 64, 129, 256} <= ks
    assert {nn.slots(k) for k in ks} >= {256, 512, 1024}
    assert nn.slots(129) < 8 * 129 and nn.slots(256) < 8 * 256


def test_the_other_knn_cases_are_exact_and_cross_their_seams():
    for name, (nq, N, L, a, k, seed) in nc.KNN_F64.items():
        assert 4 * L * a * a < nn.EXACT32
    nq, N, L, a, k, _ = nc.KNN_F64["seam"]
    assert nc.SEAM_QT == 67108 < nq
    Q, X, k = nc.knn_rows("seam", np.float64, nc.KNN_F64)
    tied = nn.tied_at_kth(Q, X, k)
    assert tied.max() <= nn.slots(k)                   # every query is re-scored, none keeps the GEMM's ranking
    assert (tied[nc.SEAM_QT:] > k).any()               # exact ties at the k-th place beyond the seam
    counts, cap = nn.candidate_counts(Q.astype(np.float32), X.astype(np.float32), k)
    assert counts.max() <= cap                         # the same values as float32 rows: the prefilter without overflow
    nq, N, L, a, k, _ = nc.KNN_F64["paged"]
    assert k > 4096 and N > 8192
    nq, N = nc.KNN_FILTERED["query_tiles"][:2]
    assert nq > nn.TILE_F32
    for name in ("short_k10", "short_k64"):
        N, k = nc.KNN_FILTERED[name][1], nc.KNN_FILTERED[name][4]
        assert 0 < N - nn.PANEL_COLS < k
    # |row|^2 of the scaled rows: every row above 2^100, every sum still an exact integer multiple of 2^102
    Q, X, _ = nc.knn_rows("huge", np.float32, nc.KNN_F64)
    assert ((X.astype(np.float64) * nc.HUGE_SCALE) ** 2).sum(1).max() > 2.0 ** 100
    assert np.isfinite((X * np.float32(nc.HUGE_SCALE)).astype(np.float32)).all()


def test_overflow_case_overflows_only_where_it_should():
    X, k = nc.overflow_rows()
    counts, cap = nn.candidate_counts(X, X, k, same=True)
    assert (counts[:300] > cap).all()                  # the identical rows: 300 candidates at distance 0
    tied = nn.tied_at_kth(X, X, k)
    assert (tied[:300] > cap).all() and (tied[300:] <= cap).any()      # f64 pass: GEMM's ranking for some, re-score for others
    assert len(np.unique(X[300:], axis=0)) == 400


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_radius_cases_have_pairs_exactly_on_the_radius(dtype):
    X, eps = nc.radius_self_rows(dtype)
    nn.lattice_ok(X)
    d = nn.sqdist(X, X)
    assert (d == eps * eps).sum() > 0 and (d < eps * eps).sum() > len(X)
    assert ((d == 0).sum(1) == 2)[:6].all() and ((d == 0).sum(1) == 2)[-6:].all()      # the planted duplicates, for eps = 0
    Q, Y, r = nc.radius_query_rows(dtype)
    d = nn.sqdist(Q, Y)
    assert (d == r).sum() > 0 and (d < r).sum() > 0 and (d > r).sum() > 0


def test_radius_seam_case_has_pairs_on_the_radius_beyond_the_seam():
    Q, X, r = nc.radius_seam_rows()
    indptr, indices, sq = nn.radius_csr(Q, X, r)
    beyond = sq[indptr[nc.SEAM_QT]:]
    assert (beyond == r).sum() > 0 and (sq[:indptr[nc.SEAM_QT]] == r).sum() > 0
    assert 10 < indptr[-1] / len(Q) < 100               # a few dozen neighbours per query


@pytest.mark.parametrize("name", sorted(nc.GRAPHS))
def test_graphs_have_the_gap_the_subspace_bound_divides_by(name):
    indptr, indices, N, m = nc.graph(name)
    theta, U, dd = nn.normalised_affinity_eigh(indptr, indices, N)
    assert theta[m - 1] - theta[m] >= nc.MIN_GAP, theta[:m + 1]
    iso = nc.GRAPHS[name][2]
    if iso:                                             # no edge from or to the last `iso` nodes: dd = 1 there
        assert (np.diff(indptr)[N - iso:] == 0).all() and indices.max() < N - iso and (dd[N - iso:] == 1.0).all()
    assert abs(theta[0] - 1.0) < 1e-12                  # a connected part: eigenvalue 1 of S, 0 of the Laplacian
    assert np.allclose(U.T @ U, np.eye(N), atol=1e-10)
