"""CPU tests of the compact index: the NumPy twin against float64 brute force, retrieval quality on a planted
corpus, persistence, and argument validation.  Nothing here needs a GPU; the kernels are held to the twin bit for bit in
tests/test_gpu_pq.py."""
import numpy as np
import pytest

import pq_numpy as tw


@pytest.fixture(scope="session", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def _numpy_kmeans(x, k, rng, iters=8):
    """seeded Lloyd in float64 (the test's own trainer; the product trains with learn.fit_kmeans on the device)"""
    c = x[rng.choice(len(x), k, replace=False)].astype(np.float64)
    xd = x.astype(np.float64)
    for _ in range(iters):
        d2 = (xd * xd).sum(1)[:, None] - 2.0 * xd @ c.T + (c * c).sum(1)[None, :]
        lab = d2.argmin(1)
        for j in range(k):
            sel = lab == j
            if sel.any():
                c[j] = xd[sel].mean(0)
    return c.astype(np.float32)


def _train_codebooks(x, m, ksub, rng):
    dsub = x.shape[1] // m
    return np.stack([_numpy_kmeans(x[:, s * dsub:(s + 1) * dsub], ksub, rng) for s in range(m)])


# ------------------------------------------------------------------------------------------------ twin vs float64
@pytest.fixture(scope="module")
def seeded():
    rng = np.random.default_rng(20240607)
    m, ksub, dsub, n, nq = 8, 64, 4, 2000, 16
    cb = rng.standard_normal((m, ksub, dsub)).astype(np.float32)
    x = rng.standard_normal((n, m * dsub)).astype(np.float32)
    q = rng.standard_normal((nq, m * dsub)).astype(np.float32)
    return cb, x, q


def test_twin_codes_equal_float64_argmin_outside_the_rounding_margin(seeded):
    cb, x, _ = seeded
    m, ksub, dsub = cb.shape
    codes = tw.encode(x, cb)
    xs = x.astype(np.float64).reshape(len(x), m, 1, dsub)
    acc = ((xs - cb.astype(np.float64)[None]) ** 2).sum(-1)                    # (n, m, ksub) float64 distances
    order = np.sort(acc, axis=-1)
    bound = dsub * 2.0 ** -23 * acc.max(axis=-1)                               # float32 accumulation bound, per (row, sub-space)
    decided = (order[..., 1] - order[..., 0]) > bound
    excluded = 1.0 - decided.mean()
    print(f"excluded share {excluded:.5f}")
    assert excluded < 0.01
    assert np.array_equal(codes[decided], acc.argmin(-1)[decided])
    from pvsim import ProductQuantizer
    assert np.array_equal(ProductQuantizer.from_codebooks(cb).decode(codes), tw.decode(codes, cb))     # the product's decode = the twin's


def test_twin_adc_scores_equal_float64_decoded_product(seeded):
    cb, x, q = seeded
    m, ksub, dsub = cb.shape
    codes = tw.encode(x, cb)
    inv_db = (1.0 / np.linalg.norm(x.astype(np.float64), axis=1)).astype(np.float32)
    inv_q = (1.0 / np.linalg.norm(q.astype(np.float64), axis=1)).astype(np.float32)
    got = tw.scores(tw.lut(q, cb), codes, inv_q, inv_db).astype(np.float64)
    from pvsim import ProductQuantizer
    dec = ProductQuantizer.from_codebooks(cb).decode(codes)                                            # the product's decode
    assert dec.dtype == np.float32 and np.array_equal(dec, tw.decode(codes, cb))
    dec = dec.astype(np.float64)
    assert dec.shape == x.shape
    terms = np.abs(q.astype(np.float64))[:, None, :] * np.abs(dec)[None, :, :]
    scale = inv_q.astype(np.float64)[:, None] * inv_db.astype(np.float64)[None, :]
    ref = (q.astype(np.float64) @ dec.T) * scale
    # m * dsub roundings of the products and sums and the two factor products, each 2^-24 relative to partial sums <= sum |terms|:
    # half of m * dsub * 2^-23 covers them all, so the bound has headroom
    bound = m * dsub * 2.0 ** -23 * terms.sum(-1) * scale
    assert (np.abs(got - ref) <= bound).all(), float((np.abs(got - ref) / bound).max())


def test_twin_ranking_rule():
    s = np.array([[0.5, np.nan, 0.5, -0.0, 0.0, 2.0, 0.5]], np.float32)
    idx, val = tw.topk(s, 7, col_offset=10)
    assert idx.tolist() == [[15, 10, 12, 16, 13, 14, 11]]
    assert np.isnan(val[0, -1]) and val[0, 0] == 2.0
    cand = np.array([[4, -1, 2, 2]], np.int64)
    ex = tw.rescore(np.ones((1, 2), np.float32), np.arange(10, dtype=np.float32).reshape(5, 2), cand)
    assert ex[0].tolist() == [17.0, -np.inf, 9.0, 9.0]
    i2, v2 = tw.rerank(cand, ex, 3)
    assert i2.tolist() == [[4, 2, 2]] and v2.tolist() == [[17.0, 9.0, 9.0]]
    from pvsim.compact import order_exact                             # the host ordering CompactIndex.rank(rerank=) uses
    rng = np.random.default_rng(8)
    cand = rng.integers(0, 50, (6, 40)).astype(np.int64)
    ex = np.round(rng.standard_normal((6, 40)), 1).astype(np.float32)          # coarse: many equal scores
    ex[0, 3], ex[1, :] = np.nan, 0.5
    for k in (1, 7, 40):
        pi, pv = order_exact(cand, ex, k)
        ti, tv = tw.rerank(cand, ex, k)
        assert np.array_equal(pi, ti) and np.array_equal(pv.view(np.uint32), tv.view(np.uint32))


# ------------------------------------------------------------------------------------------------ quality
def test_planted_corpus_quality():
    """4096 rows of 32 clusters in 64-d (unit cluster sigma), 256 queries = planted row + 0.15 sigma noise, m = 8, ksub = 256,
    seeded NumPy k-means.  Measured with the committed seed by the twin: planted row in the ADC top-1 35.2 %, top-10 79.3 %,
    top-50 97.3 %, top-100 100 % (see the printed figures); exact top-1 = planted 100 %.  The recall@10 floor is that 0.793 minus
    0.05, a margin for another k-means seed path only -- the kernels are bit-exact with the twin."""
    rng = np.random.default_rng(7)
    centres = rng.standard_normal((32, 64)) * 2.0
    x = (centres[rng.integers(0, 32, 4096)] + rng.standard_normal((4096, 64))).astype(np.float32)
    planted = rng.choice(4096, 256, replace=False)
    q = (x[planted] + 0.15 * rng.standard_normal((256, 64))).astype(np.float32)
    cb = _train_codebooks(x, 8, 256, rng)
    codes = tw.encode(x, cb)
    inv_db = (1.0 / np.linalg.norm(x.astype(np.float64), axis=1)).astype(np.float32)
    inv_q = (1.0 / np.linalg.norm(q.astype(np.float64), axis=1)).astype(np.float32)
    sc = tw.scores(tw.lut(q, cb), codes, inv_q, inv_db)
    idx, _ = tw.topk(sc, 100)
    hit = idx == planted[:, None]
    recall = {r: float(hit[:, :r].any(1).mean()) for r in (1, 10, 50, 100)}
    print("planted recall", recall)
    exact = tw.rescore(q, x, idx, inv_q, inv_db)
    from pvsim.compact import order_exact
    first, _ = order_exact(idx, exact, 1)                   # the product's ordering of the re-scored short list
    assert np.array_equal(first, tw.rerank(idx, exact, 1)[0])
    assert np.array_equal(first[:, 0], planted)             # ADC top-100 + exact re-scoring: the planted row comes first, always
    assert recall[10] >= MEASURED_RECALL_AT_10 - 0.05


MEASURED_RECALL_AT_10 = 0.793


# ------------------------------------------------------------------------------------------------ persistence, validation
def test_pq_model_round_trip(tmp_path):
    from pvsim import ProductQuantizer
    from pvsim.models import load_model, save_model
    rng = np.random.default_rng(3)
    cb = rng.standard_normal((4, 16, 3)).astype(np.float32)
    pq = ProductQuantizer.from_codebooks(cb)
    save_model(str(tmp_path / "pq.npz"), pq)
    back = load_model(str(tmp_path / "pq.npz"))
    assert isinstance(back, ProductQuantizer) and (back.m, back.ksub, back.dsub, back.d) == (4, 16, 3, 12)
    assert np.array_equal(back.codebooks, cb) and back.projection is None
    pq.projection = rng.standard_normal((12, 40)).astype(np.float32)
    save_model(str(tmp_path / "pq2.npz"), pq)
    back = load_model(str(tmp_path / "pq2.npz"))
    assert np.array_equal(back.projection, pq.projection) and np.array_equal(back.codebooks, cb)
    codes = rng.integers(0, 16, (9, 4)).astype(np.uint8)
    assert np.array_equal(back.decode(codes), tw.decode(codes, cb))
    with pytest.raises(ValueError, match="not been fitted"):
        save_model(str(tmp_path / "x.npz"), ProductQuantizer(4))


def test_compact_index_npz_layout_round_trip(tmp_path):
    from pvsim.compact import load_arrays, save_arrays
    rng = np.random.default_rng(4)
    paths = [f"img/{i}.jpg" for i in range(7)]
    codes = rng.integers(0, 256, (7, 4)).astype(np.uint8)
    inv = rng.random(7).astype(np.float32)
    cb = rng.standard_normal((4, 256, 2)).astype(np.float32)
    w = rng.standard_normal((8, 20)).astype(np.float32)
    y = rng.standard_normal((7, 8)).astype(np.float32)
    fn = str(tmp_path / "ci.npz")
    save_arrays(fn, paths, codes, inv, cb, w, y)
    with np.load(fn, allow_pickle=False) as z:             # plain arrays, nothing pickled
        assert sorted(z.files) == ["codebooks", "codes", "inv_norms", "kind", "paths", "projected", "projection"]
    a = load_arrays(fn)
    assert a["paths"] == paths
    for key, want in (("codes", codes), ("inv_norms", inv), ("codebooks", cb), ("projection", w), ("projected", y)):
        assert np.array_equal(a[key], want) and a[key].dtype == want.dtype
    save_arrays(fn, paths, codes, inv, cb)
    a = load_arrays(fn)
    assert a["projection"] is None and a["projected"] is None
    np.savez(str(tmp_path / "other.npz"), kind="kmeans")
    with pytest.raises(ValueError, match="not a compact index"):
        load_arrays(str(tmp_path / "other.npz"))


def test_validation_messages():
    """all of these are raised before anything touches a device"""
    from pvsim import CompactIndex, ProductQuantizer
    rng = np.random.default_rng(5)
    x = rng.standard_normal((300, 12)).astype(np.float32)
    with pytest.raises(ValueError, match="ksub must be between 1 and 256"):
        ProductQuantizer(4, ksub=257)
    with pytest.raises(ValueError, match=r"d % m"):
        ProductQuantizer(5).fit(x)
    with pytest.raises(ValueError, match="need n >= ksub"):
        ProductQuantizer(4, ksub=256).fit(x[:255])
    with pytest.raises(TypeError, match="float32"):
        ProductQuantizer(4, ksub=16).fit(x.astype(np.float64))
    with pytest.raises(TypeError, match="float32"):
        ProductQuantizer.from_codebooks(np.zeros((4, 16, 3)))
    db = {f"p{i}": x[i] for i in range(300)}
    with pytest.raises(ValueError, match=r"d % m"):
        CompactIndex.fit(db, m=5)
    with pytest.raises(ValueError, match="ksub must be between 1 and 256"):
        CompactIndex.fit(db, m=4, ksub=300)
    with pytest.raises(ValueError, match="need n >= ksub"):
        CompactIndex.fit({k: db[k] for k in list(db)[:100]}, m=4, ksub=256)
    with pytest.raises(TypeError, match="float32"):
        CompactIndex.fit({k: v.astype(np.float64) for k, v in db.items()}, m=4, ksub=16)
    # an index from arrays stays on the host until its first search
    cb = rng.standard_normal((4, 16, 3)).astype(np.float32)
    codes = rng.integers(0, 16, (300, 4)).astype(np.uint8)
    ci = CompactIndex(list(db), codes, np.ones(300, np.float32), ProductQuantizer.from_codebooks(cb), projected=x)
    assert len(ci) == 300 and ci.paths[:2] == ["p0", "p1"]
    assert ci.nbytes == 300 * (4 + 4) + cb.nbytes + x.nbytes
    with pytest.raises(ValueError, match="rerank=5 must be >= k=10"):
        ci.rank(x[:2], 10, rerank=5)
    with pytest.raises(TypeError, match="float32"):
        ci.rank(x[:2].astype(np.float64), 10)
    with pytest.raises(ValueError, match="1 <= k <= 300"):
        ci.rank(x[:2], 301)
    bare = CompactIndex(list(db), codes, np.ones(300, np.float32), ProductQuantizer.from_codebooks(cb))
    with pytest.raises(ValueError, match="keep_projected=True"):
        bare.rank(x[:2], 10, rerank=20)
    with pytest.raises(TypeError, match="float32"):
        CompactIndex(list(db), codes, np.ones(300, np.float64), ProductQuantizer.from_codebooks(cb))


def test_eval_rejects_full_ranking_of_a_compact_index():
    from pvsim import CompactIndex, ProductQuantizer
    from pvsim import eval as ev
    rng = np.random.default_rng(6)
    cb = rng.standard_normal((2, 4, 2)).astype(np.float32)
    ci = CompactIndex(["a", "b", "c"], rng.integers(0, 4, (3, 2)).astype(np.uint8), np.ones(3, np.float32),
                      ProductQuantizer.from_codebooks(cb))
    plan = ev._plan(ci)
    assert plan.matrix is None and plan.paths == ["a", "b", "c"] and plan.paths is ci._paths and plan.n == 3
    with pytest.raises(ValueError, match="pass k"):
        plan.rank(np.zeros((1, 4), np.float32), None)

    class Identity:
        def encode(self, v):
            return v

    with pytest.raises(ValueError, match="CompactIndex only"):
        ev.retrieve_top_k_similar(np.zeros(4, np.float32), {"a": np.ones(4, np.float32)}, Identity(), k=1, rerank=3)
    with pytest.raises(ValueError, match="rerank=2 must be >= k=3"):           # not clamped up to k: the same error as rank()
        ev.retrieve_top_k_similar(np.zeros(4, np.float32), ci, Identity(), k=3, rerank=2)


def test_scan_plan_matches_the_arithmetic_both_scans_carried(tmp_path):
    """csrc/bench/scan_plan_check.cpp includes only pq_common.hpp, whose host part needs no HIP header: the segment size, the LDS
    bytes and the code-load width of a scan against the closed forms the flat and the probed scan each carried inline, for the 40960-
    and 36864-entry budgets, code bases at byte offsets 0, 4 and 1, and the (m, ksub) of the segment-limit cases of both GPU test
    files; also the (m, ksub) range both scans accept.  Built with the address and undefined-behaviour sanitizers, no GPU."""
    import os
    import shutil
    import subprocess

    from conftest import REPO
    src = os.path.join(REPO, "python-visual-similarity_amd", "csrc", "bench", "scan_plan_check.cpp")
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (g++, c++ or clang++) on PATH"
    exe = str(tmp_path / "scan_plan_check")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
