"""GPU tests of k-reciprocal re-ranking (csrc/reciprocal.hip, pvsim/reciprocal.py, eval's reciprocal=): every array and every
returned list against the NumPy twin (tests/reciprocal_numpy.py), bit for bit -- include/pvsim.h fixes the order and the rounding of
every operation, so there is no tolerance to argue about.  The twin is fed with the index's own lists.  Outputs of direct kernel
calls are followed by guard bytes."""
import numpy as np
import pytest

import diffusion_numpy as dn
import reciprocal_numpy as tw

pytestmark = pytest.mark.gpu

GUARD = 64
DB_ARRAYS = ("nbr", "sim", "members", "v", "v0", "w", "w0", "ws")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _up(ctx, a):
    a = np.ascontiguousarray(a)
    return ctx.buffer(max(a.nbytes, 16)).upload(a)


def _out(ctx, nbytes):
    """an output buffer full of 0x5A with GUARD bytes behind it"""
    return ctx.buffer(nbytes + GUARD).fill_bytes(0x5A)


def _guard_intact(buf, nbytes):
    return bool((buf.download((GUARD,), np.uint8, offset=nbytes) == 0x5A).all())


def _index(ctx, X, tag="r"):
    from pvsim.index import DeviceIndex
    return DeviceIndex({f"{tag}{i:05d}": X[i] for i in range(len(X))}, ctx)


def _own_lists(index, X, kg):
    idx, val = index.rank(X, kg + 1)
    nbr, sim = dn.drop_self(idx, val, np.arange(len(X)))
    return nbr.astype(np.int32), sim


def _assert_db(r, want, what=""):
    for name in DB_ARRAYS:
        assert _same(getattr(r, name), want[name]), (name, what)
    assert np.array_equal(r.last_build["dropped"], want["dropped"]), what
    assert np.array_equal(r.last_build["members"], want["members"].sum(axis=1)), what


def _assert_rank(r, index, want_db, Q, k, kq, kr, lam, what=""):
    qi, qv = index.rank(Q, kq)
    idx, val = r.rank(Q, k=k, kq=kq, kr=kr, lam=lam)
    wi, wv, rep = tw.rerank(want_db, qi, qv, k, kr, lam)
    assert np.array_equal(idx, wi) and _same(val, wv), what
    assert np.array_equal(r.last_rank["dropped"], rep["dropped"]) and np.array_equal(r.last_rank["members"], rep["members"].sum(axis=1)), what
    return idx, wi, qi, qv


def _lattice(N, L, seed):
    """small-integer coordinates: many rows have exactly the same cosine to a third one, so lists tie and the order rule decides"""
    rng = np.random.default_rng(seed)
    X = rng.integers(-2, 3, (N, L)).astype(np.float32)
    X[:, 0] = 3
    return X


# ------------------------------------------------------------------------------------------------ the entry points on hand-made lists
def _hand_made(N, kg, seed):
    """lists of seeded rows, then by hand: empty slots (also at slot k1 - 1 = 5), a repeated id, a row that lists itself, a row with
    no reciprocal slot, an id outside [0, N), negative and NaN similarities"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((12, 6))[rng.integers(0, 12, N)] + 0.6 * rng.standard_normal((N, 6))
    nbr, sim = tw.lists(X, kg)
    nbr = nbr.astype(np.int64)
    nbr[rng.random(nbr.shape) < 0.06] = -1
    nbr[11, 5] = -1                                  # slot k1 - 1 of row 11 is empty: no query is reciprocal with it
    nbr[13, 1] = nbr[13, 0]                          # a repeated id
    nbr[17, 2] = 17                                  # a row that lists itself
    nbr[19] = [(19 + 7 * (t + 1)) % N for t in range(kg)]   # far rows that do not list 19 back (checked below)
    nbr[23, 0] = N + 5                               # outside [0, N): stored as -1
    sim[rng.random(sim.shape) < 0.05] *= -1
    sim[29, 1] = np.nan
    return nbr, sim


def _run_database(ctx, nbr32, sim, k1, k2, gamma):
    N, kg = nbr32.shape
    d_nbr, d_sim = _up(ctx, nbr32), _up(ctx, sim)
    outs = {"mask1": (N * 8, (N,), np.uint64), "maskh": (N * 8, (N,), np.uint64), "members": (N * kg, (N, kg), np.uint8),
            "dropped": (N * 4, (N,), np.int32), "v": (N * kg * 8, (N, kg), np.float64), "v0": (N * 8, (N,), np.float64),
            "w": (N * kg * 8, (N, kg), np.float64), "w0": (N * 8, (N,), np.float64), "ws": (N * 8, (N,), np.float64)}
    d = {name: _out(ctx, nb) for name, (nb, _, _) in outs.items()}
    ctx.krr_sets_dev(d_nbr.ptr, N, kg, k1, d["mask1"].ptr, d["maskh"].ptr)
    ctx.krr_members_dev(d_nbr.ptr, d["mask1"].ptr, d["maskh"].ptr, N, kg, d["members"].ptr, d["dropped"].ptr)
    ctx.krr_weights_dev(d_sim.ptr, d["members"].ptr, N, kg, gamma, d["v"].ptr, d["v0"].ptr)
    ctx.krr_expand_dev(d_nbr.ptr, d["v"].ptr, d["v0"].ptr, N, kg, k2, d["w"].ptr, d["w0"].ptr, d["ws"].ptr)
    got = {name: d[name].download(shape, dt) for name, (_, shape, dt) in outs.items()}
    for name, (nb, _, _) in outs.items():
        assert _guard_intact(d[name], nb), name
    d["nbr"], d["sim"] = d_nbr, d_sim
    return got, d


@pytest.mark.parametrize("gamma,k2", [(3, 3), (0, 1), (1, 8)])
def test_entry_points_match_twin_on_hand_made_lists(gpu_ctx, gamma, k2):
    ctx = gpu_ctx
    N, kg, k1 = 300, 7, 6                            # k1h = 3: an H of four ids can join with one new id
    nbr, sim = _hand_made(N, kg, 7)
    want = tw.database(nbr, sim, k1, k2, gamma)
    assert want["mask1"][19] == 0 and (want["nbr"][11, 5], want["nbr"][23, 0]) == (-1, -1)
    assert (want["dropped"] > 0).any() and want["members"].any()
    got, d = _run_database(ctx, want["nbr"], sim, k1, k2, gamma)
    for name in ("mask1", "maskh", "members", "dropped", "v", "v0", "w", "w0", "ws"):
        assert _same(got[name], want[name]), (name, gamma, k2)
    # queries: rankings of perturbed rows, then by hand: empty slots, a repeated id, an id outside [0, N), a NaN, a query below every
    # threshold (no member: sq = 0 with k2 = 1), and one whose first result is row 11
    rng = np.random.default_rng(3)
    nq, kq, kr = 9, 12, 5
    qidx = np.stack([rng.choice(N, kq, replace=False) for _ in range(nq)]).astype(np.int64)
    qidx[:6, :kg] = np.where(want["nbr"][[5, 40, 77, 120, 200, 299]] >= 0, want["nbr"][[5, 40, 77, 120, 200, 299]], 0)
    qval = np.sort(rng.uniform(0.2, 1.0, (nq, kq)).astype(np.float32), axis=1)[:, ::-1].copy()
    for q, own in ((4, 200), (5, 299)):                   # the row itself in front of its list: members of its H's fall outside
        qidx[q, 1:kg + 1], qidx[q, 0] = qidx[q, :kg].copy(), own
        qval[q, :kg + 1] = np.float32(1.0) - np.float32(0.01) * np.arange(kg + 1, dtype=np.float32)
    qidx[1, 2], qidx[1, 9] = -1, N
    qidx[2, 5] = qidx[2, 0]
    qval[3, 1] = np.nan
    qval[6] = np.float32(-0.5)
    qidx[7, 0] = 11
    wq, sq, dropped, flags = tw.query(want, qidx, qval)
    assert not flags[6].any() and (flags.sum(axis=1) > 0).sum() >= 4 and dropped.any()
    d_qi, d_qv = _up(ctx, qidx), _up(ctx, qval)
    d_wq, d_sq, d_dr, d_kp = _out(ctx, nq * kq * 8), _out(ctx, nq * 8), _out(ctx, nq * 4), _out(ctx, nq * 4)
    ctx.krr_query_dev(d["nbr"].ptr, d["sim"].ptr, d["maskh"].ptr, d["v"].ptr, d["v0"].ptr, N, kg, k1, k2, gamma, d_qi.ptr, d_qv.ptr, nq, kq,
                      d_wq.ptr, d_sq.ptr, d_kp.ptr, d_dr.ptr)
    assert _same(d_wq.download((nq, kq), np.float64), wq) and _same(d_sq.download((nq,), np.float64), sq)
    assert _same(d_dr.download((nq,), np.int32), dropped) and _same(d_kp.download((nq,), np.int32), flags.sum(axis=1).astype(np.int32))
    for lam in (0.3, 0.0, 1.0):
        d_sc = _out(ctx, nq * kr * 8)
        ctx.krr_score_dev(d["nbr"].ptr, d["w"].ptr, d["w0"].ptr, d["ws"].ptr, N, kg, d_qi.ptr, d_qv.ptr, d_wq.ptr, d_sq.ptr, nq, kq, kr, lam,
                          d_sc.ptr)
        sc = tw.score(want, qidx, qval, wq, sq, kr, lam)
        assert _same(d_sc.download((nq, kr), np.float64), sc), lam
        assert _guard_intact(d_sc, nq * kr * 8)
        d_sc.free()
    if k2 == 1:
        assert sq[6] == 0.0 and not tw.score(want, qidx, qval, wq, sq, kr, 0.0)[6].any()      # no member: J = +0
    for buf, nb in ((d_wq, nq * kq * 8), (d_sq, nq * 8), (d_dr, nq * 4), (d_kp, nq * 4)):
        assert _guard_intact(buf, nb)
        buf.free()
    ctx.krr_query_dev(d["nbr"].ptr, d["sim"].ptr, d["maskh"].ptr, d["v"].ptr, d["v0"].ptr, N, kg, k1, k2, gamma, None, None, 0, kq, None, None,
                      None, None)                    # zero queries are a no-op
    # the same lists through the Python surface: ids outside [0, N) as they came
    from pvsim import KReciprocal
    r = KReciprocal.from_arrays(nbr, sim, k1, k2, gamma, ctx=ctx)
    _assert_db(r, want, "from_arrays")
    for lam in (0.3, 0.0):
        idx, val, det = r.rank_lists(qidx, qval, k=kr, kr=kr, lam=lam, details=True)
        wi, wv, rep = tw.rerank(want, qidx, qval, kr, kr, lam)
        assert np.array_equal(idx, wi) and _same(val, wv) and _same(det["scores"], rep["scores"]), lam
    assert np.array_equal(r.last_rank["dropped"], dropped) and np.array_equal(r.last_rank["members"], flags.sum(axis=1))
    r.close()
    for b in list(d.values()) + [d_qi, d_qv]:
        b.free()


def test_entry_points_refuse_bad_arguments(gpu_ctx):
    ctx = gpu_ctx
    N, kg = 40, 5
    nbr, sim = tw.lists(np.random.default_rng(1).standard_normal((N, 4)), kg)
    d_nbr, d_sim = _up(ctx, nbr), _up(ctx, sim)
    d_a, d_b, d_c = _out(ctx, N * kg * 8), _out(ctx, N * kg * 8), _out(ctx, N * kg * 8)
    d_m, d_n = _out(ctx, N * 8), _out(ctx, N * 8)
    with pytest.raises(ValueError, match="k1"):
        ctx.krr_sets_dev(d_nbr.ptr, N, kg, 6, d_m.ptr, d_n.ptr)                     # k1 > kg
    d_big = _up(ctx, np.zeros((80, 70), np.int32))
    with pytest.raises(ValueError, match="k1"):
        ctx.krr_sets_dev(d_big.ptr, 80, 70, 65, d_m.ptr, d_n.ptr)                   # k1 > 64
    with pytest.raises(ValueError, match="overlap"):
        ctx.krr_sets_dev(d_nbr.ptr, N, kg, 3, d_m.ptr, d_m.ptr + 8)
    with pytest.raises(ValueError, match="null"):
        ctx.krr_sets_dev(None, N, kg, 3, d_m.ptr, d_n.ptr)
    with pytest.raises(ValueError, match="aligned"):
        ctx.krr_sets_dev(d_nbr.ptr, N, kg, 3, d_m.ptr + 4, d_n.ptr)
    with pytest.raises(ValueError, match="kg"):
        ctx.krr_sets_dev(d_nbr.ptr, N, N, 3, d_m.ptr, d_n.ptr)
    ctx.krr_sets_dev(d_nbr.ptr, N, kg, 3, d_m.ptr, d_n.ptr)
    with pytest.raises(ValueError, match="overlap"):
        ctx.krr_members_dev(d_nbr.ptr, d_m.ptr, d_n.ptr, N, kg, d_nbr.ptr, d_a.ptr)
    with pytest.raises(ValueError, match="gamma"):
        ctx.krr_weights_dev(d_sim.ptr, d_c.ptr, N, kg, 9, d_a.ptr, d_m.ptr)
    with pytest.raises(ValueError, match="overlap"):
        ctx.krr_weights_dev(d_sim.ptr, d_c.ptr, N, kg, 3, d_a.ptr, d_a.ptr + 64)
    with pytest.raises(ValueError, match="k2"):
        ctx.krr_expand_dev(d_nbr.ptr, d_a.ptr, d_m.ptr, N, kg, kg + 2, d_b.ptr, d_n.ptr, d_c.ptr)
    with pytest.raises(ValueError, match="overlap"):
        ctx.krr_expand_dev(d_nbr.ptr, d_a.ptr, d_m.ptr, N, kg, 2, d_a.ptr, d_n.ptr, d_c.ptr)
    d_qi, d_qv = _up(ctx, np.zeros((2, 8), np.int64)), _up(ctx, np.zeros((2, 8), np.float32))
    with pytest.raises(ValueError, match="kq"):
        ctx.krr_query_dev(d_nbr.ptr, d_sim.ptr, d_n.ptr, d_a.ptr, d_m.ptr, N, kg, 3, 2, 3, d_qi.ptr, d_qv.ptr, 2, N + 1, d_b.ptr, d_c.ptr, d_c.ptr + 64, d_c.ptr + 128)
    with pytest.raises(ValueError, match="overlap"):
        ctx.krr_query_dev(d_nbr.ptr, d_sim.ptr, d_n.ptr, d_a.ptr, d_m.ptr, N, kg, 3, 2, 3, d_qi.ptr, d_qv.ptr, 2, 8, d_a.ptr, d_c.ptr, d_c.ptr + 64, d_c.ptr + 128)
    with pytest.raises(ValueError, match="kr"):
        ctx.krr_score_dev(d_nbr.ptr, d_a.ptr, d_m.ptr, d_n.ptr, N, kg, d_qi.ptr, d_qv.ptr, d_b.ptr, d_c.ptr, 2, 8, 9, 0.3, d_c.ptr + 64)   # kr > kq
    with pytest.raises(ValueError, match="lambda"):
        ctx.krr_score_dev(d_nbr.ptr, d_a.ptr, d_m.ptr, d_n.ptr, N, kg, d_qi.ptr, d_qv.ptr, d_b.ptr, d_c.ptr, 2, 8, 4, 1.5, d_c.ptr + 64)
    with pytest.raises(ValueError, match="overlap"):
        ctx.krr_score_dev(d_nbr.ptr, d_a.ptr, d_m.ptr, d_n.ptr, N, kg, d_qi.ptr, d_qv.ptr, d_b.ptr, d_c.ptr, 2, 8, 4, 0.3, d_b.ptr)
    for buf, nb in ((d_a, N * kg * 8), (d_b, N * kg * 8), (d_c, N * kg * 8)):
        assert (buf.download((nb,), np.uint8) == 0x5A).all()                         # nothing was launched
    for b in (d_nbr, d_sim, d_a, d_b, d_c, d_m, d_n, d_big, d_qi, d_qv):
        b.free()


# ------------------------------------------------------------------------------------------------ the Python surface
@pytest.mark.parametrize("corpus", ["blobs", "curves"])
def test_both_corpora_through_the_device(gpu_ctx, corpus):
    """N = 1024 at the defaults.  The device's lists are the twin's lists (fed with the index's own rankings), hence its
    precision: no separate threshold"""
    from pvsim import KReciprocal
    X, lab, Q, ql = tw.blobs(seed=0) if corpus == "blobs" else dn.curves(seed=0)
    index = _index(gpu_ctx, X, "c")
    r = KReciprocal.build(index, k=40, k1=20, k2=6, gamma=3, block=512)
    want = tw.database(*_own_lists(index, X, 40), 20, 6, 3)
    _assert_db(r, want, corpus)
    idx, wi, qi, qv = _assert_rank(r, index, want, Q, 20, 80, None, 0.3, corpus)
    plain, got = tw.precision(qi[:, :20], lab, ql), tw.precision(idx, lab, ql)
    print(f"{corpus}: precision@20 on the device: plain {plain:.4f}, re-ranked {got:.4f}, dropped {r.last_build['dropped_fraction']:.3f}")
    assert got == tw.precision(wi, lab, ql)
    r.close()
    index.close()


# N, L, kg, k1, k2, nq, k, kq, kr
EDGES = [(2, 4, 1, 1, 1, 1, 1, 1, 1),          # the smallest index; kq = kr = 1
         (2, 4, 1, 1, 2, 3, 2, 2, 2),          # k2 = kg + 1 at kg = 1
         (257, 6, 8, 8, 1, 1, 5, 20, 20),      # k1 = kg, k2 = 1, one query; one row past a 256-row block
         (513, 6, 70, 64, 6, 65, 10, 80, 40),  # k1 = 64, kg past a wave, kr < kq, 65 queries; one row past two blocks
         (257, 5, 9, 5, 10, 65, 7, 20, 7),     # k1 odd (k1h = 3), k2 = kg + 1, k = kr
         (300, 6, 6, 3, 2, 3, 1, 1, 1)]        # kq = kr = 1 on a larger index


@pytest.mark.parametrize("shape", EDGES, ids=lambda s: "-".join(map(str, s)))
def test_edge_shapes_on_lattice_inputs(gpu_ctx, shape):
    from pvsim import KReciprocal
    N, L, kg, k1, k2, nq, k, kq, kr = shape
    X = _lattice(N, L, 100 + N + kg)
    Q = _lattice(nq, L, 200 + nq)
    index = _index(gpu_ctx, X)
    r = KReciprocal.build(index, k=kg, k1=k1, k2=k2, gamma=3, block=256)
    nbr, sim = _own_lists(index, X, kg)
    if N > 2:
        assert (np.diff(sim, axis=1) == 0).mean() > 0.2                              # the lists do tie
    want = tw.database(nbr, sim, k1, k2, 3)
    _assert_db(r, want, shape)
    _assert_rank(r, index, want, Q, k, kq, kr, 0.3, shape)
    r.close()
    index.close()


def test_threshold_tie_and_lambda(gpu_ctx):
    """qval exactly equal to sim[g][k1 - 1] is reciprocal, one ulp below is not; lambda = 1 returns index.rank; lambda = 0 with tied J
    keeps the order of the first ranking"""
    from pvsim import KReciprocal
    X = _lattice(300, 6, 11)
    index = _index(gpu_ctx, X)
    k1 = 5
    r = KReciprocal.build(index, k=10, k1=k1, k2=1, gamma=3)
    want = tw.database(r.nbr, r.sim, k1, 1, 3)
    sim = want["sim"]
    g = np.array([3, 50, 120, 250])
    qidx = np.stack([np.concatenate([[gi], (gi + 1 + np.arange(7)) % 300]) for gi in g]).astype(np.int64)
    qval = np.full((4, 8), np.float32(-1), np.float32)                               # below every threshold but the first slot's
    qval[:, 0] = sim[g, k1 - 1]
    qval[1, 0] = np.nextafter(qval[1, 0], np.float32(-1))
    wq, sq, dropped, flags = tw.query(want, qidx, qval)
    assert flags[:, 0].tolist() == [1, 0, 1, 1]
    idx, val, det = r.rank_lists(qidx, qval, k=8, lam=0.3, details=True)
    wi, wv, rep = tw.rerank(want, qidx, qval, 8, 8, 0.3)
    assert np.array_equal(idx, wi) and _same(val, wv) and _same(det["wq"], wq) and _same(det["sq"], sq) and _same(det["scores"], rep["scores"])
    # lambda = 0: query 1 has no member, every J is +0 and the candidates keep their first order
    idx0, val0 = r.rank_lists(qidx, qval, k=8, lam=0.0)
    assert np.array_equal(idx0[1], qidx[1]) and not val0[1].any()
    assert np.array_equal(idx0, tw.rerank(want, qidx, qval, 8, 8, 0.0)[0])
    Q = _lattice(5, 6, 12)
    fi, fv = index.rank(Q, 9)
    idx1, val1 = r.rank(Q, k=9, kq=30, kr=30, lam=1.0)
    assert np.array_equal(idx1, fi) and _same(val1, fv.astype(np.float64) + 0.0)
    r.close()
    index.close()


def test_from_graph_equals_build_and_follows_add_and_remove(gpu_ctx):
    from pvsim import Diffusion, KReciprocal
    rng = np.random.default_rng(31)
    X = (rng.standard_normal((10, 16))[rng.integers(0, 10, 340)] + 0.7 * rng.standard_normal((340, 16))).astype(np.float32)
    index = _index(gpu_ctx, X[:300], "g")
    g = Diffusion.build(index, k=12, gamma=3, mutable=True)

    def check(what):
        a, b = KReciprocal.from_graph(g, k1=7, k2=4, gamma=3), KReciprocal.build(index, k=12, k1=7, k2=4, gamma=3)
        for name in DB_ARRAYS:
            assert _same(getattr(a, name), getattr(b, name)), (name, what)
        assert np.array_equal(a.last_build["dropped"], b.last_build["dropped"])
        ra, rb = a.rank(X[:6], k=5, kq=20), b.rank(X[:6], k=5, kq=20)
        assert np.array_equal(ra[0], rb[0]) and _same(ra[1], rb[1]), what
        b.close()
        return a
    first = check("built")
    g.add({f"new{i:02d}": X[300 + i] for i in range(40)})
    with pytest.raises(RuntimeError, match="has changed"):
        first.rank(X[:2])                                                            # a snapshot: it does not follow
    first.close()
    check("after add").close()
    g.remove([f"g{i:05d}" for i in (3, 77, 299)] + ["new05"])
    assert len(index) == 336
    last = check("after remove")
    want = tw.database(last.nbr, last.sim, 7, 4, 3)
    _assert_db(last, want, "after remove")
    last.close()
    h = Diffusion.build(index, k=12, gamma=3)
    with pytest.raises(ValueError, match="mutable"):
        KReciprocal.from_graph(h)
    h.close()
    g.close()
    index.close()


def test_eval_keyword_save_load_and_refusals(gpu_ctx, tmp_path):
    from pvsim import Diffusion, KReciprocal
    from pvsim import eval as ev
    rng = np.random.default_rng(41)
    X = (rng.standard_normal((8, 12))[rng.integers(0, 8, 120)] + 0.8 * rng.standard_normal((120, 12))).astype(np.float32)
    Q = (X[rng.integers(0, 120, 4)] + 0.3 * rng.standard_normal((4, 12))).astype(np.float32)
    index = _index(gpu_ctx, X, "e")
    r = KReciprocal.build(index, k=15, k1=8, k2=3, gamma=3)
    want = tw.database(*_own_lists(index, X, 15), 8, 3, 3)
    _assert_db(r, want)

    class Enc:
        context = index.ctx

        def __init__(self, v):
            self.v = v

        def encode(self, _):
            return self.v

    paths = list(index.keys())
    qi, qv = index.rank(Q, 80)
    wi, wv, _ = tw.rerank(want, qi, qv, 10, 80, 0.3)                                 # eval: rank's defaults, kq = max(k, 80)
    hits = ev.retrieve_top_k_similar(None, index, Enc(Q[0]), k=10, reciprocal=r)
    assert [p for p, _ in hits] == [paths[i] for i in wi[0]] and np.array_equal(np.array([s for _, s in hits]), wv[0])
    labels = {p: i % 8 for i, p in enumerate(paths)}
    for q in range(3):
        assert ev.top_k_accuracy([None], [q], index, labels, Enc(Q[q]), k=10, reciprocal=r) == float(any(labels[paths[i]] == q for i in wi[q]))
    assert 0.0 <= ev.top_k_map([None], [0], index, labels, Enc(Q[0]), k=10, reciprocal=r) <= 1.0
    g = Diffusion.build(index, k=5)
    for kw in ({"diffuse": g}, {"rerank": 5}, {"nprobe": 2}):
        with pytest.raises(ValueError, match="excludes"):
            ev.retrieve_top_k_similar(None, index, Enc(Q[0]), k=5, reciprocal=r, **kw)
    g.close()
    with pytest.raises(TypeError):
        ev.retrieve_top_k_similar(None, dict(zip(paths, X)), Enc(Q[0]), k=5, reciprocal=r)
    other = _index(gpu_ctx, X[:50], "o")
    with pytest.raises(ValueError, match="another index"):
        ev.retrieve_top_k_similar(None, other, Enc(Q[0]), k=5, reciprocal=r)
    other.close()

    fn = str(tmp_path / "krr.npz")
    r.save(fn)
    with np.load(fn, allow_pickle=False) as z:
        assert sorted(z.files) == ["gamma", "index_modifications", "k1", "k2", "nbr", "sim"]
    h = KReciprocal.load(fn, index)
    _assert_db(h, want, "loaded")
    a, b = r.rank(Q, k=5, kq=40, kr=20), h.rank(Q, k=5, kq=40, kr=20)
    assert np.array_equal(a[0], b[0]) and _same(a[1], b[1])

    for bad in ({"k1": 65}, {"k1": 16}, {"k2": 17}, {"gamma": 9}, {"k": 120}):
        with pytest.raises(ValueError):
            KReciprocal.build(index, **{"k": 15, "k1": 8, **bad})
    for bad in ({"kr": 41, "kq": 40}, {"k": 21, "kr": 20, "kq": 40}, {"kq": 121}, {"lam": 1.5}, {"lam": -0.1}, {"kq": 0}):
        with pytest.raises(ValueError):
            r.rank(Q, **{"k": 5, **bad})
    with pytest.raises(TypeError, match="float32"):
        r.rank(Q.astype(np.float64))
    i64 = _index(gpu_ctx, X.astype(np.float64), "d")
    with pytest.raises(TypeError, match="float32"):
        KReciprocal.build(i64, k=15)
    i64.close()
    lone = KReciprocal.from_arrays(want["nbr"], want["sim"], 8, 3, 3, ctx=gpu_ctx)
    _assert_db(lone, want, "from arrays")
    with pytest.raises(RuntimeError, match="without an index"):
        lone.rank(Q)
    lone.close()
    index.add({"new": X[0] * 2})
    for x in (r, h):
        with pytest.raises(RuntimeError, match="has changed"):
            x.rank(Q)
    with pytest.raises(RuntimeError, match="has changed"):
        KReciprocal.load(fn, index)
    for x in (r, h):
        x.close()
    index.close()
