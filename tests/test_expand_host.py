"""CPU tests of query expansion and database-side augmentation (pvsim/expand.py): the weights and the drop rule against the twin
(tests/expand_numpy.py), argument validation, and what expansion buys on a planted corpus, computed with the twin alone."""
import numpy as np
import pytest

import expand_numpy as tw


def test_module_and_binding_exist():
    """the feature's entry points: the module, the exported class and the C-ABI binding"""
    import pvsim
    from pvsim import _ffi, expand
    assert pvsim.QueryExpansion is expand.QueryExpansion
    assert "pvs_combine_rows_dev" in _ffi.SIGNATURES and len(_ffi.SIGNATURES["pvs_combine_rows_dev"]) == 12
    assert hasattr(_ffi.lib(), "pvs_combine_rows_dev")
    assert _ffi.COMBINE_CHUNK_BYTES % 16 == 0 and _ffi.COMBINE_BATCH >= 2


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("scheme", ["average", "alpha", "linear"])
def test_weights_equal_the_twin(dtype, scheme):
    from pvsim.expand import expansion_weights
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 10):
        s = rng.uniform(-0.4, 1.0, (6, n)).astype(dtype)
        s[0, 0] = 0
        s[-1, -1] = 1
        for alpha in range(9):
            got = expansion_weights(s, scheme, alpha)
            want = tw.weights(s, scheme, alpha)
            assert got.dtype == dtype and got.shape == s.shape
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (scheme, alpha, n)
    if scheme == "alpha":
        assert (expansion_weights(s, scheme, 3)[s < 0] == 0).all()          # negative similarities weigh nothing
    assert expansion_weights(np.zeros((3, 0), dtype), scheme, 3).shape == (3, 0)


def test_drop_rule():
    from pvsim.expand import drop_self
    idx = np.array([[0, 5, 6, 7],        # self first
                    [5, 6, 1, 7],        # self in the middle
                    [5, 6, 7, 8],        # self absent (a duplicate row took its place): the last slot goes
                    [9, 8, 7, 3]],       # self last
                   dtype=np.int64)
    val = np.arange(16, dtype=np.float32).reshape(4, 4)
    gi, gv = drop_self(idx, val, np.arange(4))
    assert np.array_equal(gi, [[5, 6, 7], [5, 6, 7], [5, 6, 7], [9, 8, 7]])
    assert np.array_equal(gv, [[1, 2, 3], [4, 5, 7], [8, 9, 10], [12, 13, 14]])
    ti, tv = tw.drop_self(idx, val, np.arange(4))
    assert np.array_equal(gi, ti) and np.array_equal(gv, tv) and gv.dtype == val.dtype
    own = np.array([10, 11])                                                 # a block that does not start at row 0
    gi, gv = drop_self(np.array([[3, 10], [11, 4]]), np.array([[.5, .4], [.9, .1]]), own)
    assert np.array_equal(gi, [[3], [4]]) and np.array_equal(gv, [[.5], [.1]])
    gi, gv = drop_self(np.array([[0]]), np.array([[1.0]]), np.array([0]))    # N = 1: nothing is left
    assert gi.shape == (1, 0) and gv.shape == (1, 0)


@pytest.mark.parametrize("kwargs", [
    {"n": 0}, {"n": -1}, {"n": 2.5}, {"n": True}, {"scheme": "mean"}, {"scheme": None}, {"alpha": -1}, {"alpha": 9}, {"alpha": 2.0},
    {"alpha": True}, {"query_weight": -0.5}, {"query_weight": float("nan")}, {"query_weight": float("inf")}, {"query_weight": "1"},
    {"passes": 0}, {"passes": 1.5},
])
def test_query_expansion_validates(kwargs):
    from pvsim import QueryExpansion
    with pytest.raises(ValueError):
        QueryExpansion(**kwargs)


def test_query_expansion_defaults():
    from pvsim import QueryExpansion
    qe = QueryExpansion()
    assert (qe.n, qe.scheme, qe.alpha, qe.query_weight, qe.passes) == (10, "average", 3, 1.0, 1)
    qe = QueryExpansion(n=3, scheme="alpha", alpha=0, query_weight=0, passes=2)
    assert (qe.n, qe.scheme, qe.alpha, qe.query_weight, qe.passes) == (3, "alpha", 0, 0.0, 2)
    assert "alpha" in repr(qe)


def test_weights_validate():
    from pvsim.expand import expansion_weights
    s = np.zeros((2, 3), np.float32)
    for bad in ({"scheme": "pow"}, {"scheme": "alpha", "alpha": 9}, {"scheme": "alpha", "alpha": -1}):
        with pytest.raises(ValueError):
            expansion_weights(s, **bad)
    with pytest.raises(ValueError):
        expansion_weights(np.zeros(3, np.float32), "average", 3)
    with pytest.raises(ValueError):
        expansion_weights(np.zeros((2, 3), np.int32), "average", 3)


def test_expansion_on_a_compact_index_is_refused():
    """the combination is out of scope: a CompactIndex keeps no full-precision rows to sum (refused before anything is encoded)"""
    from pvsim import CompactIndex, QueryExpansion
    from pvsim import eval as ev

    class NoEncoder:
        def encode(self, *_):
            raise AssertionError("refused before the query is encoded")

    ci = CompactIndex.__new__(CompactIndex)          # no device here; the refusal needs none
    ci._paths = ["a", "b"]
    qe = QueryExpansion(n=1)
    img = np.zeros((4, 4, 3), np.uint8)
    with pytest.raises(ValueError, match="CompactIndex"):
        ev.retrieve_top_k_similar(img, ci, NoEncoder(), k=1, expand=qe)
    with pytest.raises(ValueError, match="CompactIndex"):
        ev.top_k_map([img], [0], ci, {"a": 0, "b": 1}, NoEncoder(), k=1, expand=qe)
    with pytest.raises(ValueError, match="CompactIndex"):
        ev.top_k_accuracy([img], [0], ci, {"a": 0, "b": 1}, NoEncoder(), k=1, expand=qe)
    with pytest.raises(ValueError, match="CompactIndex"):
        ev.expand_verified(img, [("a", 0.9, 10)], ci, NoEncoder(), k=1, qe=qe)
    with pytest.raises(ValueError):
        ev.expand_verified(img, [("a", 0.9, 10)], {"a": np.ones(4, np.float32)}, NoEncoder(), k=1, min_inliers=-1)
    with pytest.raises(TypeError):
        ev.expand_verified(img, [("a", 0.9, 10)], {"a": np.ones(4, np.float32)}, NoEncoder(), k=1, qe={"n": 3})


def test_twin_combine_definition():
    """the twin against the definition written out by hand, scalar by scalar"""
    X = np.array([[1, 2], [3, 4], [5, 6]], np.float32)
    idx = np.array([[2, -1, 0, 3], [1, 1, -1, -1]])
    w = np.array([[.5, 9, 2, 9], [1, -1, 9, 9]], np.float32)
    selfr = np.array([[10, 20], [30, 40]], np.float32)
    got = tw.combine(X, idx, w, selfr, np.array([2, 0], np.float32))
    assert np.array_equal(got, [[20 + 2.5 + 2, 40 + 3 + 4], [0, 0]])
    assert np.array_equal(tw.combine(X, idx, w), [[2.5 + 2, 3 + 4], [0, 0]])
    assert np.array_equal(tw.combine(X, idx[:, :0], w[:, :0], selfr), selfr)


def test_expansion_helps_on_the_planted_corpus():
    """32 classes x 32 rows in 64-d, database noise 1.0 sigma, 256 queries at 1.6 sigma: precision@20 after average query expansion
    (n = 5) and after database-side augmentation (r = 8, linear weights) each beat the plain ranking by at least 0.05 (measured
    in NumPy over four seeds: +0.08 .. +0.11).  Twin only: tests/test_gpu_expand.py asserts the same of the device."""
    X, lab, Q, ql = tw.planted(seed=0)
    inv_db, inv_q = tw.inv_norms(X), tw.inv_norms(Q)
    k = 20
    i0, s0 = tw.rank(Q, X, k)
    base = tw.precision(i0, lab, ql)
    Qe = tw.expand_queries(Q, inv_q, X, inv_db, i0[:, :5], s0[:, :5], "average", 3, 1.0)
    aqe = tw.precision(tw.rank(Qe, X, k)[0], lab, ql)
    di, ds = tw.rank(X, X, 9)
    Xa = tw.augment(X, inv_db, di, ds, "linear", 3)
    dba = tw.precision(tw.rank(Q, Xa, k)[0], lab, ql)
    print(f"precision@20: plain {base:.4f}, AQE(n=5) {aqe:.4f}, DBA(r=8, linear) {dba:.4f}")
    assert aqe >= base + 0.05
    assert dba >= base + 0.05
