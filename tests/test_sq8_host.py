"""Host tests of the int8 resident index: properties of the NumPy twin (tests/sq8_numpy.py) the GPU tests
lean on, the quality of the quantiser on a planted VLAD-like corpus, the .npz layout, and the refusals of eval._plan.  No GPU."""
import numpy as np
import pytest

import sq8_numpy as tw


# ------------------------------------------------------------------------------------------------ the integer sum
def test_acc_is_unchanged_by_chunking_and_permutation():
    rng = np.random.default_rng(1)
    L = 1000
    q = rng.integers(-127, 128, (5, L)).astype(np.int8)
    d = rng.integers(-127, 128, (7, L)).astype(np.int8)
    want = tw.acc(q, d)
    for chunk in (1, 4, 16, 32, 64, 333, 1000):
        got = np.zeros_like(want)
        for t0 in range(0, L, chunk):
            got += tw.acc(q[:, t0:t0 + chunk], d[:, t0:t0 + chunk])
        assert np.array_equal(got, want), chunk
    for seed in range(3):
        p = np.random.default_rng(seed).permutation(L)
        assert np.array_equal(tw.acc(q[:, p], d[:, p]), want)
    # the order inside a k-step of 32 bytes, reversed: what a matrix instruction may do with the values of a step
    step = np.arange(L + (-L) % 32).reshape(-1, 32)[:, ::-1].ravel()
    step = step[step < L]
    assert np.array_equal(tw.acc(q[:, step], d[:, step]), want)


def test_largest_sum_is_exactly_the_bound():
    L = tw.MAX_L
    sign = np.where(np.arange(L) % 3 == 0, -127, 127).astype(np.int8)
    a = tw.acc(sign[None, :], np.stack([sign, -sign]))
    assert a[0, 0] == 2114060288 == 127 * 127 * L and a[0, 1] == -2114060288
    assert 2114060288 < 2 ** 31
    with pytest.raises(AssertionError):                                  # -128 does not occur in a code row: with it the bound breaks
        tw.acc(np.full((1, L), -128, np.int8), np.full((1, L), -128, np.int8))
    # above 2^24 the conversion merges neighbours: the index decides such ties
    assert np.float32(np.int32(2 ** 24 + 1)) == np.float32(np.int32(2 ** 24))


def test_encode_rule_on_chosen_values():
    # exact halves: the scaled value lands on k + 1/2 for even and odd k of both signs, and goes to the even neighbour
    hx, ht = tw.exact_halves(3.0)
    kk = np.floor(ht).astype(np.int64)
    assert ((kk % 2 == 0) & (ht > 0)).any() and ((kk % 2 == 1) & (ht > 0)).any()
    assert ((kk % 2 == 0) & (ht < 0)).any() and ((kk % 2 == 1) & (ht < 0)).any()
    hc, _ = tw.encode(np.concatenate([[np.float32(3.0)], hx])[None, :])
    want = np.where(kk % 2 == 0, kk, kk + 1)
    assert hc[0, 0] == 127 and np.array_equal(hc[0, 1:1 + hx.size], want)
    x = np.zeros((6, 8), np.float32)
    x[0] = [1, 0.5, 0.25, -0.5, -1, 0.75, 0, -0.25]   # dyadic ratios: 127, 63.5, 31.75, ...
    x[1] = 0                                       # a zero row
    x[2, 3] = -2.5                                 # one-hot
    x[3] = np.float32(1e-45) * np.array([3, -3, 1, 2, 0, -1, 3, -2], np.float32)      # subnormal amax
    x[4] = np.array([1, -1, 1, 1, -1, -1, 1, -1], np.float32) * np.float32(2 ** 20)   # +-amax
    x[5] = np.float32(2 ** -20) * np.arange(8, dtype=np.float32)
    codes, inv = tw.encode(x)
    assert codes.shape == (6, 64) and not codes[:, 8:].any()
    assert codes[0, :8].tolist() == [127, 64, 32, -64, -127, 95, 0, -32]  # 63.5 -> 64 (even), 31.75 -> 32, 95.25 -> 95
    assert not codes[1].any() and inv[1] == 0
    assert codes[2, :8].tolist() == [0, 0, 0, -127, 0, 0, 0, 0] and inv[2] == np.float32(1 / 127)
    assert codes[3, :8].tolist() == [127, -127, 42, 85, 0, -42, 127, -85]
    assert codes[4, :8].tolist() == [127, -127, 127, 127, -127, -127, 127, -127]
    assert codes.min() >= -127
    ss = (codes[0].astype(np.int64) ** 2).sum()
    assert inv[0] == np.float32(1.0 / np.sqrt(np.float64(ss)))


def test_ranking_breaks_ties_by_index():
    score = np.array([[1, 3, 3, 2, 3]], np.float32)
    idx, val = tw.topk(score, 4, col_offset=10)
    assert idx.tolist() == [[11, 12, 14, 13]] and val.tolist() == [[3, 3, 3, 2]]


# ------------------------------------------------------------------------------------------------ quality on a planted corpus
N_DB, N_CLUSTERS, D_SUB, N_QUERIES, N_SCENES = 4096, 64, 64, 256, 256
MEASURED_RECALL_AT_10 = 0.9996      # the twin on this fixture; the assertion allows 0.01 below it
MEASURED_TOP1 = 1.0


def _vlad_like(raw):
    """(n, N_CLUSTERS, D_SUB) residual sums -> rows: signed square root, L2-normalised"""
    x = (np.sign(raw) * np.sqrt(np.abs(raw))).reshape(raw.shape[0], -1)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@pytest.fixture(scope="module")
def corpus():
    """N_DB images of N_SCENES scenes: an image is its scene's residual sums plus its own, in N_CLUSTERS blocks of D_SUB dimensions
    whose energy is unequal (a few clusters carry most of a row).  A query is a database row plus noise."""
    rng = np.random.default_rng(20240607)
    scene = rng.standard_normal((N_SCENES, N_CLUSTERS, D_SUB)) * np.exp(rng.normal(0.0, 1.0, (N_SCENES, N_CLUSTERS, 1)))
    member = np.repeat(np.arange(N_SCENES), N_DB // N_SCENES)
    own = rng.standard_normal((N_DB, N_CLUSTERS, D_SUB)) * np.exp(rng.normal(0.0, 1.0, (N_DB, N_CLUSTERS, 1)))
    db = _vlad_like(scene[member] + 0.8 * own)
    planted = rng.choice(N_DB, N_QUERIES, replace=False)
    noise = _vlad_like(rng.standard_normal((N_QUERIES, N_CLUSTERS, D_SUB)))
    q = (db[planted] + np.float32(0.7) * noise).astype(np.float32)
    return db, q, planted


def test_quality_against_the_exact_float64_ranking(corpus):
    db, q, planted = corpus
    d64, q64 = db.astype(np.float64), q.astype(np.float64)
    exact = (q64 / np.linalg.norm(q64, axis=1, keepdims=True)) @ (d64 / np.linalg.norm(d64, axis=1, keepdims=True)).T
    exact_idx = np.argsort(-exact, axis=1, kind="stable")[:, :10]
    assert np.array_equal(exact_idx[:, 0], planted)                          # the fixture: the planted row is the exact top-1
    qc, iq = tw.encode(q)
    dc, idb = tw.encode(db)
    # float64 BLAS on integers: every partial sum is an integer below 2^53, so the product is exact in any order; held against
    # the int64 twin on a slice
    a = qc.astype(np.float64) @ dc.astype(np.float64).T
    assert np.array_equal(a[:8].astype(np.int64), tw.acc(qc[:8], dc))
    s = (a.astype(np.int32).astype(np.float32) * iq[:, None]) * idb[None, :]
    idx, _ = tw.topk(s, 10)
    top1 = float((idx[:, 0] == exact_idx[:, 0]).mean())
    recall = float(np.mean([len(set(idx[r]) & set(exact_idx[r])) / 10 for r in range(N_QUERIES)]))
    err = float(np.abs(np.take_along_axis(s, idx, 1) - np.take_along_axis(exact, idx, 1)).max())
    print(f"int8 twin: recall@10 = {recall:.4f}, top-1 agreement = {top1:.4f}, max |score - exact| on the lists = {err:.2e}")
    assert top1 == 1.0
    assert recall >= MEASURED_RECALL_AT_10 - 0.01


# ------------------------------------------------------------------------------------------------ persistence helpers
def test_npz_round_trip_and_wrong_kind(tmp_path):
    from pvsim.quantized import load_int8_arrays, padded_length, save_int8_arrays
    rng = np.random.default_rng(3)
    x = rng.standard_normal((5, 70)).astype(np.float32)
    codes, inv = tw.encode(x)
    assert padded_length(70) == 128 == codes.shape[1] and padded_length(64) == 64 and padded_length(1) == 64
    paths = [f"img/{i}.png" for i in range(5)]
    fn = str(tmp_path / "index.npz")
    save_int8_arrays(fn, paths, codes[:, :70], inv, 70)
    with np.load(fn, allow_pickle=False) as z:
        assert sorted(z.files) == ["L", "codes", "factors", "kind", "paths"] and str(z["kind"]) == "int8_index"
        assert z["codes"].dtype == np.int8 and z["codes"].shape == (5, 70)
    a = load_int8_arrays(fn)
    assert a["paths"] == paths and a["L"] == 70
    assert np.array_equal(a["codes"], codes[:, :70]) and np.array_equal(a["factors"].view(np.uint32), inv.view(np.uint32))
    assert load_int8_arrays(fn[:-4])["paths"] == paths                     # the suffix is optional, as for the other indexes
    with pytest.raises(ValueError):
        save_int8_arrays(fn, paths, codes, inv, 70)                          # padded codes are not the file's layout
    other = str(tmp_path / "other.npz")
    np.savez(other, kind="compact_index", paths=np.array(paths), codes=codes[:, :70], factors=inv, L=np.int64(70))
    with pytest.raises(ValueError, match="not an int8 index file"):
        load_int8_arrays(other)
    np.savez(other, paths=np.array(paths), vectors=x)
    with pytest.raises(ValueError, match="not an int8 index file"):
        load_int8_arrays(other)
    from pvsim.compact import load_arrays
    with pytest.raises(ValueError):
        load_arrays(fn)                                                      # and the compact index refuses this one


# ------------------------------------------------------------------------------------------------ eval._plan, without a context
def _bare_index(paths=("a", "b", "c")):
    from pvsim.index import _PathLedger
    from pvsim.quantized import Int8Index
    index = Int8Index.__new__(Int8Index)           # no device: _plan decides from the type and the ledger alone
    index._ledger, index._L, index._ld = _PathLedger(paths), 8, 64
    return index


def test_plan_refuses_what_an_int8_index_cannot_do():
    import pvsim
    from pvsim.eval import _plan
    index = _bare_index()
    for kw, needs in ((dict(expand=pvsim.QueryExpansion()), "DeviceIndex"), (dict(rerank=20), "CompactIndex"),
                      (dict(nprobe=4), "IVFCompactIndex"), (dict(diffuse=object()), "DeviceIndex"),
                      (dict(reciprocal=object()), "DeviceIndex")):
        with pytest.raises(ValueError, match=needs) as e:
            _plan(index, **kw)
        assert next(iter(kw)) + "=" in str(e.value)
    plan = _plan(index)
    assert plan.n == 3 and plan.paths == ["a", "b", "c"] and plan.index_of("c") == 2
    with pytest.raises(ValueError, match="ranks a finite list: pass k"):
        plan.rank(np.zeros((1, 8), np.float32), None)
    idx, val = plan.rank(np.zeros((1, 8), np.float32), 0)                    # k = 0: the empty result, no device touched
    assert idx.shape == (1, 0) and val.dtype == np.float32


def test_construction_checks_need_no_device():
    from pvsim.quantized import Int8Index, _all_finite
    big = np.full((2, 8), 3e38, np.float32)                  # finite, though its sum of squares overflows
    assert _all_finite(big) and _all_finite(np.zeros((0, 8), np.float32))
    for bad in (np.nan, np.inf, -np.inf):
        big[1, 3] = bad
        assert not _all_finite(big)
        assert not _all_finite(np.array([[1, bad, 2]], np.float32))
    with pytest.raises(TypeError, match="float64"):
        Int8Index({"a": np.zeros(8), "b": np.ones(8)})
    with pytest.raises(ValueError, match="NaN or an infinity"):
        Int8Index({"a": np.zeros(8, np.float32), "b": np.full(8, np.inf, np.float32)})
    with pytest.raises(ValueError):
        Int8Index({"a": np.zeros(8, np.float32), "b": np.zeros(9, np.float32)})
