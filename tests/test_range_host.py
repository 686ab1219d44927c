"""CPU tests of the threshold join: the NumPy twin (tests/range_numpy.py) against brute force, the planted facts
of the corpora the GPU tests run on, the argument validation of the Python layer (raised before the device is touched), and the two
symbols in the header and the ctypes table."""
import os

import numpy as np
import pytest

import range_numpy as tw
from conftest import REPO

# the corpora of tests/test_gpu_range.py
BAND = dict(n=200, L=64, t=0.8, seed=24)
BAND_CAPACITY = 64
LATTICE = dict(n=130, L=64, seed=7)
LATTICE_T = 2.0 / 16.0


def _brute(S, t, upper=False):
    out = []
    for i in range(S.shape[0]):
        for j in range(S.shape[1]):
            if S[i, j] >= np.float32(t) and (not upper or j > i):
                out.append((i, j, S[i, j]))
    return out


def _scores(rng, nq, N):
    S = rng.standard_normal((nq, N)).astype(np.float32)
    S[rng.random((nq, N)) < 0.2] = np.float32(0.5)                 # ties at the threshold
    S.flat[::7] = np.float32(-0.0)
    S.flat[3::11] = np.nan
    return S


@pytest.mark.parametrize("t", [0.5, 0.0, -10.0, np.nextafter(np.float32(0.5), np.float32(1))])
def test_twin_hits_match_brute_force(t):
    rng = np.random.default_rng(1)
    for nq, N in ((1, 1), (5, 9), (9, 9), (17, 40)):
        S = _scores(rng, nq, N)
        for upper in (False, True) if nq == N else (False,):
            want = _brute(S, t, upper)
            row, col, val = tw.hits(S, t, upper)
            assert list(zip(row, col)) == [(i, j) for i, j, _ in want]
            assert np.array_equal(val.view(np.uint32), np.array([v for _, _, v in want], np.float32).view(np.uint32))
            for QT, NC in ((1, 1), (4, 8), (8, 4), (64, 64)):      # the tile order is a permutation with the stated nesting
                r2, c2, v2 = tw.tile_order(S, t, QT, NC, upper)
                key = lambda r, c: sorted(zip(r.tolist(), c.tolist()))
                assert key(r2, c2) == key(row, col)
                block = (r2 // QT) * (N // NC + 1) + c2 // NC
                assert (np.diff(block) >= 0).all()
                same = np.diff(block) == 0
                assert ((np.diff(r2) > 0) | ((np.diff(r2) == 0) & (np.diff(c2) > 0)))[same].all()
    S = _scores(rng, 6, 6)
    assert not np.isnan(tw.hits(S, -10.0)[2]).any()                 # a NaN score is never a hit
    zero = np.array([[-0.0, 0.0]], np.float32)
    assert tw.hits(zero, 0.0)[1].tolist() == [0, 1] and np.signbit(tw.hits(zero, 0.0)[2][0])     # -0 >= 0, bits kept


def test_twin_csr_is_in_ranker_order():
    rng = np.random.default_rng(2)
    S = _scores(rng, 12, 50)
    indptr, idx, val = tw.csr(S, 0.0)
    assert indptr[0] == 0 and indptr[-1] == idx.size == len(_brute(S, 0.0))
    for i in range(12):
        cols, vals = idx[indptr[i]:indptr[i + 1]], val[indptr[i]:indptr[i + 1]]
        want = sorted(((-float(v), j) for ii, j, v in _brute(S, 0.0) if ii == i))
        assert [(-float(v) + 0.0, j) for v, j in zip(vals, cols)] == [(a + 0.0, j) for a, j in want]


def test_twin_components_and_groups():
    rng = np.random.default_rng(3)
    for n, e in ((1, 0), (2, 1), (30, 12), (100, 60), (100, 300)):
        a, b = rng.integers(0, n, e), rng.integers(0, n, e)
        labels = tw.union_find_labels(n, a, b)
        adj = np.eye(n, dtype=bool)
        adj[a, b] = adj[b, a] = True
        for _ in range(8):                                            # transitive closure by squaring: n <= 100 < 2^8
            adj = (adj.astype(np.int32) @ adj.astype(np.int32)) > 0
        assert np.array_equal(labels, adj.argmax(axis=1))             # the first reachable node is the smallest
        gs = tw.groups(labels)
        assert all(g.size >= 2 and (np.diff(g) > 0).all() and labels[g[0]] == g[0] for g in gs)
        assert [g[0] for g in gs] == sorted(g[0] for g in gs)
    assert tw.skipped_tiles(130, 130, 64, 64) == 3 and tw.skipped_tiles(257, 257, 128, 128) == 4      # with the 1 x 1 tile of row 256
    assert tw.skipped_tiles(64, 64, 64, 64) == 0 and tw.skipped_tiles(65, 65, 64, 64) == 2      # the 1 x 64 and the 1 x 1 tile of row 64


def test_planted_facts_of_the_band_corpus():
    x, place, cos = tw.planted_band(**BAND)
    t, e = BAND["t"], tw.eps(BAND["L"])
    c = tw.cosine64(x)
    got = c[place[:, 0], place[:, 1]]
    assert np.abs(got - cos).max() < 1e-6                              # float32 rows keep the planted cosine to 1e-6 << eps
    assert ((got >= t - e) & (got < t)).sum() >= 8 and ((got >= t) & (got <= t + e)).sum() >= 8
    planted = np.zeros(c.shape, bool)
    planted[place[:, 0], place[:, 1]] = planted[place[:, 1], place[:, 0]] = True
    off = ~planted & ~np.eye(c.shape[0], dtype=bool)
    assert np.abs(c[off] - t).min() > 2 * e                            # no unplanted pair within 2 eps of t
    assert (np.triu(c, 1) >= t - 2 * e).sum() <= 2 * BAND_CAPACITY + 4096        # the candidates fit the staging list
    assert (np.triu(c, 1) >= t).sum() <= BAND_CAPACITY
    assert 1e-3 < e < 1.2e-3


def test_planted_facts_of_the_lattice():
    x = tw.lattice(**LATTICE)
    assert set(np.unique(x)) == {-1.0, 0.0, 1.0} and (np.abs(x).sum(axis=1)[5:] == 16).all()
    S = tw.lattice_scores(x, x)
    assert np.array_equal(S * 16, np.round(S * 16)) and np.array_equal(S, S.T)
    up = np.triu(np.ones(S.shape, bool), 1)
    assert (S[up] == np.float32(LATTICE_T)).sum() >= 8                 # pairs exactly at t
    assert S[0, 1] == 1 and S[0, 3] == -1 and not S[4].any()
    above = np.nextafter(np.float32(LATTICE_T), np.float32(1))
    assert (S[up] >= above).sum() < (S[up] >= np.float32(LATTICE_T)).sum()


def test_python_layer_validates_before_the_device():
    import pvsim
    from pvsim import duplicates as dup
    from pvsim import eval as pv_eval
    assert dup._check_threshold(0.1) == np.float32(0.1) and dup._check_threshold(0.1).dtype == np.float32
    for bad in (np.nan, np.inf, -np.inf, 1e39):
        with pytest.raises(ValueError):
            dup._check_threshold(bad)
    for bad in ("0.5", None, True, [0.5]):
        with pytest.raises(TypeError):
            dup._check_threshold(bad)
    for bad in (-1, 1.5, True, (1 << 40) + 1):
        with pytest.raises(ValueError):
            dup._check_limit("max_results", bad)
    assert dup._check_limit("max_pairs", None) is None and dup._check_limit("max_pairs", 7) == 7
    with pytest.raises(ValueError):
        dup._path_code("fast")
    assert [dup._path_code(p) for p in ("auto", "exact", "filtered")] == [0, 1, 2]
    for not_an_index in ({}, object()):
        with pytest.raises(NotImplementedError, match="float32 pvsim.index.DeviceIndex"):
            pvsim.find_duplicates(not_an_index, 0.9)
    f64 = {"a": np.ones(4), "b": np.ones(4)}
    with pytest.raises(NotImplementedError, match="float32"):
        pv_eval.find_duplicates(f64, 0.9)
    with pytest.raises(NotImplementedError, match="float32"):
        pv_eval.retrieve_similar(np.zeros((4, 4, 3)), f64, None, 0.9)
    with pytest.raises(ValueError):
        pv_eval.find_duplicates({"a": np.ones(4, np.float32)}, np.nan)
    assert {"retrieve_similar", "find_duplicates"} <= set(pv_eval.__all__) and "find_duplicates" in pvsim.__all__


def test_header_and_ctypes_table_carry_the_symbols():
    import __graft_entry__ as g
    g.build()
    from pvsim import _ffi
    header = open(os.path.join(REPO, "include", "pvsim.h")).read()
    for name, nargs in (("pvs_cosine_range_dev", 18), ("pvs_pair_components_dev", 7)):
        assert f"int {name}(" in header and len(_ffi.SIGNATURES[name]) == nargs and hasattr(_ffi.lib(), name)
    assert "#define PVS_RANGE_UPPER 1" in header and _ffi.RANGE_UPPER == 1
    assert _ffi.lib().pvs_version() == 103
