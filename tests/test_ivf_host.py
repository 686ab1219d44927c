"""CPU tests of the inverted lists of the compact index: the NumPy twin (tests/ivf_numpy.py) against float64,
its identities and ranking rule, retrieval quality on the planted corpus of test_pq_host.py, persistence and argument validation.
Nothing here needs a GPU; the kernels are held to the twin bit for bit in tests/test_gpu_ivf.py."""
import numpy as np
import pytest

import ivf_numpy as iv
import pq_numpy as tw


@pytest.fixture(scope="session", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _numpy_kmeans(x, k, rng, iters=8):
    """seeded Lloyd in float64 (the test's own trainer, as in test_pq_host.py; the product trains with learn.fit_kmeans)"""
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
    rng = np.random.default_rng(20261018)
    m, ksub, dsub, n, nq, nlist = 8, 64, 4, 2000, 16, 24
    d = m * dsub
    cent = (2.0 * rng.standard_normal((nlist, d))).astype(np.float32)
    x = (cent[rng.integers(0, nlist, n)] + rng.standard_normal((n, d))).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    cb = (0.7 * rng.standard_normal((m, ksub, dsub))).astype(np.float32)
    return cent, x, q, cb


def test_twin_assignment_equals_float64_argmin_outside_the_rounding_margin(seeded):
    cent, x, _, _ = seeded
    d = x.shape[1]
    lists, res = iv.assign(x, cent)
    acc = ((x.astype(np.float64)[:, None, :] - cent.astype(np.float64)[None]) ** 2).sum(-1)      # (n, nlist) float64 distances
    order = np.sort(acc, axis=-1)
    bound = d * 2.0 ** -23 * acc.max(axis=-1)                    # float32 accumulation bound of a chain of d terms, per row
    decided = (order[:, 1] - order[:, 0]) > bound
    excluded = 1.0 - decided.mean()
    print(f"excluded share {excluded:.5f}")
    assert excluded < 0.01
    assert lists.dtype == np.int32 and np.array_equal(lists[decided], acc.argmin(-1)[decided])
    assert res.dtype == np.float32 and np.array_equal(_bits(res), _bits(x - cent[lists]))         # one subtraction per element


def test_twin_adc_scores_equal_float64_centroid_plus_decoded_residual(seeded):
    cent, x, q, cb = seeded
    m, ksub, dsub = cb.shape
    d, n, nlist = x.shape[1], len(x), len(cent)
    lists, res = iv.assign(x, cent)
    ids, off = iv.sort_into_lists(lists, nlist)
    codes = tw.encode(res, cb)[ids]
    inv_db = (1.0 / np.linalg.norm(x.astype(np.float64), axis=1)).astype(np.float32)[ids]
    inv_q = (1.0 / np.linalg.norm(q.astype(np.float64), axis=1)).astype(np.float32)
    idx, val = iv.search(tw.lut(q, cb), iv.coarse(q, cent), nlist, off, ids, codes, inv_q, inv_db, n)
    assert (np.sort(idx, axis=1) == np.arange(n)[None, :]).all()                                   # every list probed: every row
    got = np.empty((len(q), n))
    np.put_along_axis(got, idx, val.astype(np.float64), axis=1)                                    # scores by original index
    recon = cent[lists].astype(np.float64) + tw.decode(tw.encode(res, cb), cb).astype(np.float64)  # c_l + decoded residual
    qd = q.astype(np.float64)
    inv_orig = np.empty(n)
    inv_orig[ids] = inv_db
    scale = inv_q.astype(np.float64)[:, None] * inv_orig[None, :]
    ref = (qd @ recon.T) * scale
    # roundings: 2 d in the coarse chain, 2 d in the table entries, m additions of entries, 2 factor products; each at most 2^-24
    # relative to a partial sum <= T = sum |q_t C_lt| + sum |q_t r^_t|.  (2 d + m) 2^-23 T is twice that count, so there is headroom.
    T = np.abs(qd) @ np.abs(cent[lists].astype(np.float64)).T + np.abs(qd) @ np.abs(recon - cent[lists].astype(np.float64)).T
    bound = (2 * d + m) * 2.0 ** -23 * T * scale
    assert (np.abs(got - ref) <= bound).all(), float((np.abs(got - ref) / bound).max())


# ------------------------------------------------------------------------------------------------ identities
def test_zero_centroid_one_list_gives_the_flat_lists_bit_for_bit(seeded):
    _, x, q, cb = seeded
    n = len(x)
    cent = np.zeros((1, x.shape[1]), np.float32)
    lists, res = iv.assign(x, cent)
    assert not lists.any() and np.array_equal(_bits(res), _bits(x))
    ids, off = iv.sort_into_lists(lists, 1)
    assert np.array_equal(ids, np.arange(n)) and off.tolist() == [0, n]
    codes = tw.encode(x, cb)
    inv_db = (1.0 / np.linalg.norm(x.astype(np.float64), axis=1)).astype(np.float32)
    table = tw.lut(q, cb)
    co = iv.coarse(q, cent)
    assert np.array_equal(_bits(co), np.zeros_like(_bits(co)))                                    # the coarse term is +0
    for k in (1, 10, 300):
        gi, gv = iv.search(table, co, 1, off, ids, codes, None, inv_db, k)
        wi, wv = tw.topk(tw.scores(table, codes, None, inv_db), k)
        assert np.array_equal(gi, wi) and np.array_equal(_bits(gv), _bits(wv))


def test_probing_every_list_returns_every_row(seeded):
    cent, x, q, cb = seeded
    n, nlist = len(x), len(cent)
    lists, res = iv.assign(x, cent)
    ids, off = iv.sort_into_lists(lists, nlist)
    idx, val = iv.search(tw.lut(q, cb), iv.coarse(q, cent), nlist, off, ids, tw.encode(res, cb)[ids], None, None, n)
    assert (np.sort(idx, axis=1) == np.arange(n)[None, :]).all() and np.isfinite(val).all()
    assert (np.diff(val.astype(np.float64), axis=1) <= 0).all()


# ------------------------------------------------------------------------------------------------ ranking
def _integer_case():
    """integer tables and coarse terms: every sum is exact, and equal scores occur inside and across lists.  List 2 is empty."""
    rng = np.random.default_rng(31)
    nq, m, ksub, nlist, n = 3, 4, 4, 5, 60
    table = rng.integers(-2, 3, (nq, m, ksub)).astype(np.float32)
    co = rng.integers(-1, 2, (nq, nlist)).astype(np.float32)
    co[:, 2] = 9.0                                               # the empty list is always the first probe
    lists = rng.integers(0, nlist - 1, n)
    lists[lists >= 2] += 1                                       # 0, 1, 3, 4
    lists[::7] = 4
    ids, off = iv.sort_into_lists(lists, nlist)
    codes = rng.integers(0, ksub, (n, m)).astype(np.uint8)       # stored order
    return table, co, lists, ids, off, codes


def test_ranking_is_by_score_then_original_index_across_lists():
    table, co, lists, ids, off, codes = _integer_case()
    nq, n, nlist = len(table), len(ids), len(co[0])
    assert off[3] == off[2]                                      # list 2 is empty
    for nprobe in (1, 3, nlist):
        plist, pval = iv.probes(co, nprobe)
        assert (plist[:, 0] == 2).all()
        for k in (1, 7, n):
            idx, val = iv.search(table, co, nprobe, off, ids, codes, None, None, k)
            for q in range(nq):
                # brute force in float64 over (score, original index): the sums are small integers, so float64 is exact too
                cand = [(-(float(co[q, l]) + sum(float(table[q, s, codes[r, s]]) for s in range(table.shape[1]))), int(ids[r]))
                        for l in plist[q] for r in range(off[l], off[l + 1])]
                cand.sort()
                want = cand[:k]
                filled = len(want)
                assert idx[q, :filled].tolist() == [i for _, i in want]
                assert val[q, :filled].tolist() == [-s for s, _ in want]
                assert (idx[q, filled:] == -1).all() and np.isneginf(val[q, filled:]).all()
                if nprobe == 1:
                    assert filled == 0                           # only the empty list was probed
                if nprobe == nlist:
                    scores = [s for s, _ in cand]
                    lists_of = {int(i): int(lists[i]) for i in ids}
                    ties = [(a, b) for a, b in zip(cand, cand[1:]) if a[0] == b[0]]
                    assert any(lists_of[a[1]] != lists_of[b[1]] for a, b in ties)      # equal scores in different lists occur
                    assert all(a[1] < b[1] for a, b in ties) and scores == sorted(scores)


# ------------------------------------------------------------------------------------------------ quality
def test_planted_corpus_quality_with_inverted_lists():
    """The planted corpus of test_pq_host.py (4096 x 64, 32 clusters, 256 queries at 0.15 sigma, m = 8, ksub = 256), nlist = 64,
    nprobe = 4, the test's own seeded Lloyd.  Conditions of the issue: (a) the planted row's list is probed for >= 95 % of the
    queries, (b) recall@10 >= 0.90, (c) recall@10 not below the flat recall@10 computed here.  Measured with the committed seed:
    see DESIGN.md section 14 (the figures are printed)."""
    rng = np.random.default_rng(7)
    centres = rng.standard_normal((32, 64)) * 2.0
    x = (centres[rng.integers(0, 32, 4096)] + rng.standard_normal((4096, 64))).astype(np.float32)
    planted = rng.choice(4096, 256, replace=False)
    q = (x[planted] + 0.15 * rng.standard_normal((256, 64))).astype(np.float32)
    inv_db = (1.0 / np.linalg.norm(x.astype(np.float64), axis=1)).astype(np.float32)
    inv_q = (1.0 / np.linalg.norm(q.astype(np.float64), axis=1)).astype(np.float32)
    # the flat index, as test_pq_host.py builds it
    cb = _train_codebooks(x, 8, 256, rng)
    flat_idx, _ = tw.topk(tw.scores(tw.lut(q, cb), tw.encode(x, cb), inv_q, inv_db), 10)
    flat = {r: float((flat_idx[:, :r] == planted[:, None]).any(1).mean()) for r in (1, 10)}
    # inverted lists: coarse centroids, then codebooks on the residuals
    nlist, nprobe = 64, 4
    cent = _numpy_kmeans(x, nlist, rng)
    lists, res = iv.assign(x, cent)
    rcb = _train_codebooks(res, 8, 256, rng)
    ids, off = iv.sort_into_lists(lists, nlist)
    codes = tw.encode(res, rcb)[ids]
    co = iv.coarse(q, cent)
    plist, _ = iv.probes(co, nprobe)
    probed = float((plist == lists[planted][:, None]).any(1).mean())
    idx, val = iv.search(tw.lut(q, rcb), co, nprobe, off, ids, codes, inv_q, inv_db[ids], 10)
    recall = {r: float((idx[:, :r] == planted[:, None]).any(1).mean()) for r in (1, 10)}
    scanned = float(np.mean([sum(off[l + 1] - off[l] for l in row) for row in plist])) / len(x)
    # RMS error of the ADC score against the exact cosine, over the scanned rows' top-10 (a figure, not a condition)
    exact = tw.rescore(q, x, idx, inv_q, inv_db)
    ok = idx >= 0
    rms = float(np.sqrt(np.mean((val[ok].astype(np.float64) - exact[ok].astype(np.float64)) ** 2)))
    print(f"ivf: planted list probed {probed:.4f}, recall@1 {recall[1]:.4f}, recall@10 {recall[10]:.4f}, scanned share {scanned:.4f}, "
          f"top-10 rms error {rms:.4f}; flat: recall@1 {flat[1]:.4f}, recall@10 {flat[10]:.4f}; list sizes {np.diff(off).min()}.."
          f"{np.diff(off).max()}")
    assert probed >= 0.95
    assert recall[10] >= 0.90
    assert recall[10] >= flat[10]


# ------------------------------------------------------------------------------------------------ persistence, validation
def _stub(rng, n=30, nlist=4, m=2, ksub=4, dsub=2, projected=False, projection=False):
    from pvsim import IVFCompactIndex, ProductQuantizer
    d = m * dsub
    cb = rng.standard_normal((m, ksub, dsub)).astype(np.float32)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    lists = rng.integers(0, nlist, n)
    ids, off = iv.sort_into_lists(lists, nlist)
    codes = rng.integers(0, ksub, (n, m)).astype(np.uint8)
    inv = rng.random(n).astype(np.float32)
    paths = [f"img/{i}.jpg" for i in range(n)]
    w = rng.standard_normal((d, 9)).astype(np.float32) if projection else None
    y = rng.standard_normal((n, d)).astype(np.float32) if projected else None
    index = IVFCompactIndex(paths, codes, inv, ProductQuantizer.from_codebooks(cb), cent, off, ids, projection=w, projected=y)
    return index, dict(paths=paths, codes=codes, inv=inv, cb=cb, cent=cent, off=off, ids=ids, w=w, y=y)


def test_ivf_index_surface_without_a_device():
    import pvsim
    from pvsim import CompactIndex, IVFCompactIndex
    assert "IVFCompactIndex" in pvsim.__all__ and issubclass(IVFCompactIndex, CompactIndex)
    index, a = _stub(np.random.default_rng(40), projected=True, projection=True)
    assert len(index) == 30 and index.paths == a["paths"] and index.keys() == a["paths"]
    assert index.nlist == 4 and index.d == 4 and index.input_dim == 9
    assert index.list_sizes.tolist() == np.diff(a["off"]).tolist() and index.list_sizes.sum() == 30
    parts = index.nbytes_breakdown
    assert parts["codes"] + parts["inv_norms"] == 30 * (2 + 4) and parts["ids"] == 30 * 4
    assert parts["centroids"] == 4 * 4 * 4 and parts["list_off"] == 5 * 8
    assert parts["inv_norms_original"] == 30 * 4                        # beside kept rows: the norms in original order, for rerank=
    assert index.nbytes == sum(parts.values()) == 30 * (2 + 4 + 4 + 4) + 64 + 40 + a["cb"].nbytes + a["w"].nbytes + a["y"].nbytes
    assert _stub(np.random.default_rng(40))[0].nbytes_breakdown["inv_norms_original"] == 0


def test_ivf_npz_round_trip_and_kind_messages(tmp_path):
    from pvsim import compact
    rng = np.random.default_rng(41)
    _, a = _stub(rng, projected=True, projection=True)
    fn = str(tmp_path / "ivf.npz")
    compact.save_arrays(fn, a["paths"], a["codes"], a["inv"], a["cb"], a["w"], a["y"], kind="ivf_compact_index", centroids=a["cent"],
                        list_off=a["off"], ids=a["ids"])
    with np.load(fn, allow_pickle=False) as z:                # plain arrays, nothing pickled
        assert sorted(z.files) == ["centroids", "codebooks", "codes", "ids", "inv_norms", "kind", "list_off", "paths", "projected",
                                   "projection"]
        assert str(z["kind"]) == "ivf_compact_index"
    back = compact.IVFCompactIndex.load(fn)
    assert back.paths == a["paths"] and back.nlist == 4
    for got, want in ((back.centroids, a["cent"]), (back._list_off, a["off"]), (back._ids, a["ids"]), (back._host["codes"], a["codes"]),
                      (back._host["inv"], a["inv"]), (back._host["projected"], a["y"]), (back.projection, a["w"]),
                      (back.quantizer.codebooks, a["cb"])):
        assert np.array_equal(got, want) and got.dtype == want.dtype
    # each loader refuses the other's file with the existing message
    with pytest.raises(ValueError, match="not a compact index file"):
        compact.CompactIndex.load(fn)
    flat = str(tmp_path / "flat.npz")
    compact.save_arrays(flat, a["paths"], a["codes"], a["inv"], a["cb"])
    with pytest.raises(ValueError, match="not an IVF compact index file"):
        compact.IVFCompactIndex.load(flat)
    assert compact.load_arrays(flat)["projection"] is None


def test_ivf_validation_messages():
    """all of these are raised before anything touches a device"""
    from pvsim import IVFCompactIndex, ProductQuantizer
    rng = np.random.default_rng(42)
    x = rng.standard_normal((300, 12)).astype(np.float32)
    db = {f"p{i}": x[i] for i in range(300)}
    for bad in (0, 65537, 2.5, True):
        with pytest.raises(ValueError, match="nlist must be an integer between 1 and 65536"):
            IVFCompactIndex.fit(db, bad, m=4, ksub=16)
    with pytest.raises(ValueError, match="need n >= nlist"):
        IVFCompactIndex.fit(db, 301, m=4, ksub=16)
    with pytest.raises(ValueError, match=r"d % m"):
        IVFCompactIndex.fit(db, 8, m=5)
    with pytest.raises(ValueError, match="need n >= ksub"):
        IVFCompactIndex.fit({k: db[k] for k in list(db)[:100]}, 8, m=4, ksub=256)
    with pytest.raises(TypeError, match="float32"):
        IVFCompactIndex.fit({k: v.astype(np.float64) for k, v in db.items()}, 8, m=4, ksub=16)
    index, a = _stub(rng, projected=True)
    q = np.zeros((2, 4), np.float32)
    for bad in (0, 5, None, 1.5, True):
        with pytest.raises(ValueError, match=r"1 <= nprobe <= 4"):
            index.rank(q, 3, bad)
    with pytest.raises(ValueError, match="1 <= k <= 30"):
        index.rank(q, 31, 2)
    with pytest.raises(ValueError, match="rerank=2 must be >= k=3"):
        index.rank(q, 3, 2, rerank=2)
    with pytest.raises(TypeError, match="float32"):
        index.rank(q.astype(np.float64), 3, 2)
    bare, _ = _stub(rng)
    with pytest.raises(ValueError, match="keep_projected=True"):
        bare.rank(q, 3, 2, rerank=5)
    pq = ProductQuantizer.from_codebooks(a["cb"])
    args = (a["paths"], a["codes"], a["inv"], pq)
    with pytest.raises(TypeError, match="float32"):
        IVFCompactIndex(*args, a["cent"].astype(np.float64), a["off"], a["ids"])
    with pytest.raises(ValueError, match="centroids must be float32"):
        IVFCompactIndex(*args, a["cent"][:, :3], a["off"], a["ids"])
    with pytest.raises(ValueError, match="list_off must be"):
        IVFCompactIndex(*args, a["cent"], a["off"][:-1], a["ids"])
    with pytest.raises(ValueError, match="list_off must rise from 0 to 30"):
        IVFCompactIndex(*args, a["cent"], a["off"] + 1, a["ids"])
    with pytest.raises(ValueError, match="permutation"):
        IVFCompactIndex(*args, a["cent"], a["off"], np.zeros(30, np.int32))
    big = np.zeros((1200, 4), np.float32)
    wide, _ = _stub(rng, n=1200, projected=True)
    with pytest.raises(ValueError, match="at most 1024 entries"):
        wide.rank(big[:1], 1025, 2)
    with pytest.raises(ValueError, match="at most 1024 entries"):
        wide.rank(big[:1], 10, 2, rerank=1100)


def test_eval_refusals_with_nprobe():
    from pvsim import CompactIndex, ProductQuantizer
    from pvsim import eval as ev
    rng = np.random.default_rng(43)
    index, a = _stub(rng)
    flat = CompactIndex(a["paths"], a["codes"], a["inv"], ProductQuantizer.from_codebooks(a["cb"]))
    labels = {p: 0 for p in a["paths"]}
    plan = ev._plan(index, nprobe=2)
    assert plan.matrix is None and plan.paths == a["paths"] and plan.paths is index._paths and plan.n == len(index)

    class Identity:
        def encode(self, v):
            return v

    q = np.zeros(4, np.float32)
    plain = {p: np.ones(4, np.float32) for p in a["paths"][:3]}
    for target in (flat, plain):
        with pytest.raises(ValueError, match="nprobe= applies to an IVFCompactIndex only"):
            ev.retrieve_top_k_similar(q, target, Identity(), k=2, nprobe=2)
        with pytest.raises(ValueError, match="nprobe= applies to an IVFCompactIndex only"):
            ev.top_k_map([q], [0], target, labels, Identity(), k=2, nprobe=2)
        with pytest.raises(ValueError, match="nprobe= applies to an IVFCompactIndex only"):
            ev.top_k_accuracy([q], [0], target, labels, Identity(), k=2, nprobe=2)
    with pytest.raises(ValueError, match="pass nprobe="):
        ev.retrieve_top_k_similar(q, index, Identity(), k=2)
    with pytest.raises(ValueError, match="pass k"):
        ev.top_k_map([q], [0], index, labels, Identity(), k=None, nprobe=2)
    from pvsim.expand import QueryExpansion
    for fn, args in ((ev.retrieve_top_k_similar, (q, index, Identity())), (ev.top_k_map, ([q], [0], index, labels, Identity())),
                     (ev.top_k_accuracy, ([q], [0], index, labels, Identity()))):
        with pytest.raises(ValueError, match="query expansion needs the full-precision rows"):
            fn(*args, k=2, nprobe=2, expand=QueryExpansion())
    with pytest.raises(ValueError, match="rerank=2 must be >= k=3"):
        ev.retrieve_top_k_similar(q, index, Identity(), k=3, rerank=2, nprobe=2)
    with pytest.raises(ValueError, match="CompactIndex only"):
        ev.top_k_map([q], [0], plain, labels, Identity(), k=2, rerank=3)
