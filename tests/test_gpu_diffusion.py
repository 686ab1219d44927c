"""GPU tests of diffusion re-ranking (csrc/diffuse.hip, pvsim/diffusion.py, eval's diffuse=): everything against the NumPy twin
(tests/diffusion_numpy.py), bit for bit -- include/pvsim.h fixes the order and the rounding of every operation, so there is no
tolerance to argue about.  Outputs of direct kernel calls are followed by guard bytes."""
import numpy as np
import pytest

import diffusion_numpy as tw

pytestmark = pytest.mark.gpu

GUARD = 64
N_G, L_G = 300, 32               # graph cases: three blocks of 128 rows, the last one ragged
N_S, KG_S = 1000, 5              # solver cases: three full blocks of 256 rows + 232


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


# ------------------------------------------------------------------------------------------------ graph kernels
def _hand_made_lists(kg, dtype):
    """rankings of seeded rows to depth kg + 1 (mutual and one-sided pairs as they come), then by hand: a row absent from its own
    list, a row listed twice in one list, negative and zero similarities, and a row whose every similarity is <= 0"""
    rng = np.random.default_rng(100 + kg)
    X = rng.standard_normal((N_G, 8))
    idx, val = tw.cosine_rank(X, X, kg + 1)
    val = val.astype(dtype)
    idx[3, 0] = 250                                  # row 3 is absent from its own list: its last slot is dropped
    idx[9] = np.where(idx[9] == 9, 9, 12)            # row 12 fills every other slot of row 9 (kg >= 2: a duplicate)
    idx[12, -1] = 9                                  # ... and row 12 lists row 9 back
    val[rng.random(val.shape) < 0.1] *= -1           # negative similarities
    val[rng.random(val.shape) < 0.05] = 0            # zero similarities
    val[7] = -np.abs(val[7])                         # every affinity of row 7 is 0 (gamma >= 1): degree 0, r = 0
    val[20, :] = np.abs(val[20, :]) + dtype(0.01)    # a row that keeps positive similarities whatever the dice said
    return idx, val


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kg", [1, 5, 33])
def test_graph_kernels_match_twin(gpu_ctx, kg, dtype):
    ctx = gpu_ctx
    idx, val = _hand_made_lists(kg, dtype)
    d_idx, d_val = _up(ctx, idx), _up(ctx, val)
    isz = np.dtype(dtype).itemsize
    n = N_G * kg
    for gamma in (0, 1, 3):
        want = tw.graph_from_lists(idx, val, gamma)
        d_nbr, d_a, d_w, d_s = _out(ctx, n * 4), _out(ctx, n * 8), _out(ctx, n * 8), _out(ctx, n * 8)
        d_deg, d_r = _out(ctx, N_G * 8), _out(ctx, N_G * 8)
        for b0 in range(0, N_G, 128):
            b = min(N_G, b0 + 128) - b0
            ctx.graph_affinity_dev(d_idx.ptr + b0 * (kg + 1) * 8, d_val.ptr + b0 * (kg + 1) * isz, dtype == np.float64, b, kg, b0, N_G, gamma,
                                   d_nbr.ptr, d_a.ptr)
        ctx.graph_mutual_dev(d_nbr.ptr, d_a.ptr, N_G, kg, d_w.ptr)
        ctx.graph_degrees_dev(d_w.ptr, N_G, kg, d_deg.ptr, d_r.ptr)
        ctx.graph_normalise_dev(d_nbr.ptr, d_w.ptr, d_r.ptr, N_G, kg, d_s.ptr)
        got = {"nbr": d_nbr.download((N_G, kg), np.int32), "a": d_a.download((N_G, kg), np.float64), "w": d_w.download((N_G, kg), np.float64),
               "deg": d_deg.download((N_G,), np.float64), "r": d_r.download((N_G,), np.float64), "s": d_s.download((N_G, kg), np.float64)}
        for name in ("nbr", "a", "w", "deg", "r", "s"):            # r is the test of the device's 1 / sqrt against np.sqrt and /
            assert _same(got[name], want[name]), (name, kg, gamma, dtype.__name__)
        for buf, nbytes in ((d_nbr, n * 4), (d_a, n * 8), (d_w, n * 8), (d_s, n * 8), (d_deg, N_G * 8), (d_r, N_G * 8)):
            assert _guard_intact(buf, nbytes), (kg, gamma)
            buf.free()
        assert got["nbr"][3, -1] == idx[3, -2] and 3 not in got["nbr"][3]                   # the last slot went
        if gamma:
            assert got["deg"][7] == 0 and got["r"][7] == 0 and not got["s"][7].any()
        if kg >= 2:
            assert (got["nbr"][9] == 12).all()                                                # the duplicate stayed
        S = tw.dense(got["nbr"], got["s"])
        S[[9, 12]] = 0                                   # the repeated slots of row 9 add up on one side only
        S[:, [9, 12]] = 0
        assert np.array_equal(S.view(np.uint64), S.T.view(np.uint64))
        if kg == 5 and gamma == 3:
            assert ((got["w"] == 0) & (got["a"] > 0)).any() and (got["w"] > 0).any()        # one-sided and mutual pairs
    d_idx.free(), d_val.free()


def test_r_equals_numpy_on_awkward_degrees(gpu_ctx):
    """1 / sqrt(deg) on the device against np.sqrt and /: degrees over 600 binades, subnormal ones, and neighbours of squares"""
    rng = np.random.default_rng(5)
    n = 4096
    deg = np.concatenate([np.exp2(rng.uniform(-1000, 1000, n)), np.array([5e-324, 2.2250738585072014e-308, 1e-310, 1.0, 4.0, 0.0]),
                          np.nextafter(np.arange(1.0, 200.0) ** 2, 0), np.nextafter(np.arange(1.0, 200.0) ** 2, np.inf),
                          rng.random(n), 1 + rng.random(n) * 50])
    N = deg.size
    w = np.zeros((N, 2))
    w[:, 1] = deg                                       # deg = +0 + 0 + w
    d_w, d_deg, d_r = _up(gpu_ctx, w), _out(gpu_ctx, N * 8), _out(gpu_ctx, N * 8)
    gpu_ctx.graph_degrees_dev(d_w.ptr, N, 2, d_deg.ptr, d_r.ptr)
    wd, wr = tw.degrees(w)
    assert _same(d_deg.download((N,), np.float64), wd)
    got = d_r.download((N,), np.float64)
    bad = np.flatnonzero(got.view(np.uint64) != wr.view(np.uint64))
    assert bad.size == 0, (bad.size, deg[bad[:5]], got[bad[:5]], wr[bad[:5]])
    assert _guard_intact(d_deg, N * 8) and _guard_intact(d_r, N * 8)
    for b in (d_w, d_deg, d_r):
        b.free()


@pytest.fixture(scope="module")
def small_index(gpu_ctx):
    """300 seeded rows x 32 in both dtypes, as DeviceIndexes"""
    from pvsim.index import DeviceIndex
    rng = np.random.default_rng(21)
    X = (rng.standard_normal((12, L_G))[rng.integers(0, 12, N_G)] + 0.8 * rng.standard_normal((N_G, L_G))).astype(np.float32)
    out = {}
    for dt in (np.float32, np.float64):
        rows = X.astype(dt)
        out[dt] = (DeviceIndex({f"img{i:03d}": rows[i] for i in range(N_G)}, gpu_ctx), rows)
    yield out
    for index, _ in out.values():
        index.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_build_equals_twin_on_the_index_own_lists(small_index, dtype):
    from pvsim import Diffusion
    index, rows = small_index[dtype]
    for kg, gamma in ((5, 3), (33, 1)):
        g = Diffusion.build(index, k=kg, gamma=gamma, block=128)
        idx, val = index.rank(rows, kg + 1)
        want = tw.graph_from_lists(idx, val, gamma)
        assert _same(g.nbr, want["nbr"]) and _same(g.s, want["s"]), (kg, gamma)
        assert (g.n, g.kg, g.gamma) == (N_G, kg, gamma)
        g.close()
    with pytest.raises(ValueError):
        Diffusion.build(index, k=N_G)                 # kg > N - 1


# ------------------------------------------------------------------------------------------------ solver
ALPHA = 0.9


@pytest.fixture(scope="module")
def solver_case(gpu_ctx):
    """graph of 1000 seeded rows (row 5 isolated) by the twin, on the device; 65 right-hand sides: column 1 zero, column 2 on the
    isolated row, the others sparse with 1 .. 12 entries; the twin's solutions for both stopping rules, computed once"""
    from pvsim import Diffusion
    rng = np.random.default_rng(31)
    X = rng.standard_normal((40, 12))[rng.integers(0, 40, N_S)] + 0.7 * rng.standard_normal((N_S, 12))
    idx, val = tw.cosine_rank(X, X, KG_S + 1)
    val[5] = -np.abs(val[5])
    g = tw.graph_from_lists(idx, val, 3)
    assert g["deg"][5] == 0
    Y = np.zeros((N_S, 65))
    for c in range(65):
        m = 1 + c % 12
        Y[rng.choice(N_S, m, replace=False), c] = rng.random(m)
    Y[:, 1] = 0
    Y[:, 2] = 0
    Y[5, 2] = 0.75
    twin = {(tol, mi): tw.cg(g["nbr"], g["s"], Y, ALPHA, tol, mi) for tol, mi in ((1e-6, 60), (1e-12, 3))}
    steps = twin[(1e-6, 60)][1]
    assert steps[1] == 0 and steps[2] == 1 and len(set(steps.tolist())) >= 4 and steps.max() < 60       # columns stop at different steps
    assert (twin[(1e-12, 3)][1][[11, 23, 35, 47]] == 3).all()                                            # the cap is reached
    d = Diffusion.from_arrays(g["nbr"], g["s"], 3, ctx=gpu_ctx)
    yield d, g, Y, twin
    d.close()


@pytest.mark.parametrize("nq", [1, 3, 64, 65])
@pytest.mark.parametrize("stop", [(1e-6, 60), (1e-12, 3)])
def test_solver_matches_twin(solver_case, nq, stop):
    """a column depends on itself alone, so the twin's 65 columns serve every nq (tests/test_diffusion_host.py holds the twin to it)"""
    d, g, Y, twin = solver_case
    tol, maxiter = stop
    x, steps, rr, yy = twin[stop]
    cols = [17] if nq == 1 else list(range(nq))
    F, st, r2, y2 = d.solve(np.ascontiguousarray(Y[:, cols]), alpha=ALPHA, tol=tol, maxiter=maxiter)
    assert _same(F, np.ascontiguousarray(x[:, cols]))
    assert _same(st, steps[cols]) and _same(r2, rr[cols]) and _same(y2, yy[cols])
    assert np.array_equal(d.last_solve["steps"], st) and np.array_equal(d.last_solve["converged"], rr[cols] <= tol * tol * yy[cols])
    if nq >= 3:
        assert not F[:, 1].any() and st[1] == 0 and np.array_equal(F[:, 2], Y[:, 2]) and st[2] == 1     # zero column; exact after one step


def test_tiling_checks_and_widths_change_no_bit(solver_case):
    d, g, Y, twin = solver_case
    x, steps, rr, yy = twin[(1e-6, 60)]
    base = d.solve(Y, alpha=ALPHA, tol=1e-6, maxiter=60)
    assert _same(base[0], x) and _same(base[1], steps) and _same(base[2], rr)
    solo = d.solve(np.ascontiguousarray(Y[:, 17:18]), alpha=ALPHA, tol=1e-6, maxiter=60)
    assert _same(solo[0][:, 0], np.ascontiguousarray(base[0][:, 17])) and solo[1][0] == base[1][17] and solo[2][0] == base[2][17]
    small = 5 * 8 * N_S * 7                            # room for 7 columns: tiles of 7, the last one of 2
    assert d._tile(65, small) == 7
    variants = [{"check_every": 1}, {"check_every": 7}, {"column_bytes": small}, {"column_bytes": small, "check_every": 7, "width": 64},
                {"width": 1}, {"width": 4}, {"width": 16}, {"width": 64}]
    for kw in variants:
        got = d.solve(Y, alpha=ALPHA, tol=1e-6, maxiter=60, **kw)
        for a, b in zip(got, base):
            assert _same(a, b), kw


def test_cg_entry_point_keeps_inside_its_outputs(solver_case, gpu_ctx):
    from pvsim.engine import diffuse_workspace
    d, g, Y, twin = solver_case
    ctx = gpu_ctx
    for C, width in ((3, 0), (65, 0), (1, 1), (5, 16)):
        cols = list(range(C))
        nbytes = diffuse_workspace(N_S, C)
        d_y, d_work = _up(ctx, np.ascontiguousarray(Y[:, cols])), ctx.buffer(nbytes)
        d_x, d_st, d_rr, d_yy = _out(ctx, N_S * C * 8), _out(ctx, C * 4), _out(ctx, C * 8), _out(ctx, C * 8)
        ctx.diffuse_cg_dev(d._d_nbr.ptr, d._d_s.ptr, N_S, KG_S, d_y.ptr, C, ALPHA, 1e-6, 60, 3, width, d_work.ptr, nbytes, d_x.ptr, d_st.ptr,
                           d_rr.ptr, d_yy.ptr)
        x, steps, rr, yy = twin[(1e-6, 60)]
        assert _same(d_x.download((N_S, C), np.float64), np.ascontiguousarray(x[:, cols]))
        assert _same(d_st.download((C,), np.int32), steps[cols]) and _same(d_rr.download((C,), np.float64), rr[cols])
        assert _same(d_yy.download((C,), np.float64), yy[cols])
        with pytest.raises(ValueError, match="work buffer"):
            ctx.diffuse_cg_dev(d._d_nbr.ptr, d._d_s.ptr, N_S, KG_S, d_y.ptr, C, ALPHA, 1e-6, 60, 3, width, d_work.ptr, nbytes - 256, d_x.ptr,
                               d_st.ptr, d_rr.ptr, d_yy.ptr)
        with pytest.raises(ValueError, match="overlaps"):
            ctx.diffuse_cg_dev(d._d_nbr.ptr, d._d_s.ptr, N_S, KG_S, d_y.ptr, C, ALPHA, 1e-6, 60, 3, width, d_work.ptr, nbytes, d_y.ptr,
                               d_st.ptr, d_rr.ptr, d_yy.ptr)
        for buf, nb in ((d_x, N_S * C * 8), (d_st, C * 4), (d_rr, C * 8), (d_yy, C * 8)):
            assert _guard_intact(buf, nb), (C, width)
            buf.free()
        d_y.free(), d_work.free()


def test_rhs_and_rank_entry_points(gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(41)
    N, C, kq = 300, 7, 4
    idx = np.stack([rng.choice(N, kq, replace=False) for _ in range(C)]).astype(np.int64)
    idx[2, 1] = -1
    idx[3, 0] = N
    for dtype in (np.float32, np.float64):
        val = rng.uniform(-0.2, 1.0, (C, kq)).astype(dtype)
        d_idx, d_val, d_y = _up(ctx, idx), _up(ctx, val), _out(ctx, N * C * 8)
        for gamma in (0, 1, 3):
            ctx.diffuse_rhs_dev(d_idx.ptr, d_val.ptr, dtype == np.float64, C, kq, N, gamma, d_y.ptr)
            assert _same(d_y.download((N, C), np.float64), tw.rhs(idx, val, N, gamma)), (dtype.__name__, gamma)
            assert _guard_intact(d_y, N * C * 8)
        for b in (d_idx, d_val, d_y):
            b.free()
    F = rng.standard_normal((C, N)).round(1)                   # many ties
    F[0, :] = 0
    F[1, 5] = np.nan
    F[1, 6] = -0.0
    d_f = _up(ctx, F)
    for k in (1, 10, N):
        d_i, d_v = _out(ctx, C * k * 8), _out(ctx, C * k * 8)
        ctx.rank_f64_dev(d_f.ptr, C, N, N, k, d_i.ptr, d_v.ptr)
        wi, wv = tw.rank_scores(F.T, k)
        assert np.array_equal(d_i.download((C, k), np.int64), wi) and _same(d_v.download((C, k), np.float64), wv), k
        assert _guard_intact(d_i, C * k * 8) and _guard_intact(d_v, C * k * 8)
        d_i.free(), d_v.free()
    d_f.free()


# ------------------------------------------------------------------------------------------------ the Python surface
def _twin_rank(index, g, Q, k, kq, gamma, alpha, tol, maxiter):
    qi, qv = index.rank(Q, kq)
    return tw.diffuse_rank({"nbr": g.nbr, "s": g.s}, qi, qv, gamma, alpha, tol, maxiter, k)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rank_equals_twin_lists_ties_included(small_index, dtype):
    from pvsim import Diffusion
    from pvsim import eval as ev
    index, rows = small_index[dtype]
    g = Diffusion.build(index, k=5, gamma=3, block=128)
    rng = np.random.default_rng(51)
    Q = (rows[rng.integers(0, N_G, 9)] + 0.3 * rng.standard_normal((9, L_G))).astype(dtype)
    for k in (1, 10, N_G):
        idx, val = g.rank(Q, k=k, kq=5, alpha=0.99, tol=1e-6, maxiter=20)
        wi, wv, steps, rr, yy = _twin_rank(index, g, Q, k, 5, 3, 0.99, 1e-6, 20)
        assert np.array_equal(idx, wi) and _same(val, wv), k
        assert np.array_equal(g.last_solve["steps"], steps) and _same(g.last_solve["rr"], rr)
    zero = val[0] == 0
    assert zero.sum() >= 2 and (np.diff(idx[0][zero]) > 0).all()                          # unreachable rows: exactly 0, in index order
    one = g.rank(Q[4:5], k=10, kq=5)                                                      # one query = its column of the batch
    assert np.array_equal(one[0][0], g.rank(Q, k=10, kq=5)[0][4])

    class Enc:
        context = index.ctx

        def __init__(self, v):
            self.v = v

        def encode(self, _):
            return self.v

    wi, wv = _twin_rank(index, g, Q[:3], 10, 10, 3, 0.99, 1e-6, 20)[:2]                   # eval uses rank's defaults
    paths = list(index.keys())
    hits = ev.retrieve_top_k_similar(None, index, Enc(Q[0]), k=10, diffuse=g)
    assert [p for p, _ in hits] == [paths[i] for i in wi[0]] and np.array_equal(np.array([s for _, s in hits]), wv[0])
    labels = {p: i % 12 for i, p in enumerate(paths)}
    for q in range(3):
        want = float(any(labels[paths[i]] == q for i in wi[q]))
        assert ev.top_k_accuracy([None], [q], index, labels, Enc(Q[q]), k=10, diffuse=g) == want
    assert 0.0 <= ev.top_k_map([None], [0], index, labels, Enc(Q[0]), k=10, diffuse=g) <= 1.0
    if dtype == np.float32:
        with pytest.raises(TypeError, match="float32"):
            g.rank(Q.astype(np.float64))
    with pytest.raises(ValueError):
        g.rank(Q, k=N_G + 1)
    with pytest.raises(ValueError):
        g.rank(Q, kq=0)
    g.close()


def test_save_load_and_snapshot(gpu_ctx, tmp_path):
    from pvsim import Diffusion
    from pvsim.index import DeviceIndex
    rng = np.random.default_rng(61)
    rows = rng.standard_normal((60, 16)).astype(np.float32)
    index = DeviceIndex({f"p{i}": rows[i] for i in range(60)}, gpu_ctx)
    g = Diffusion.build(index, k=4, gamma=3)
    fn = str(tmp_path / "graph.npz")
    g.save(fn)
    h = Diffusion.load(fn, index)
    assert _same(h.nbr, g.nbr) and _same(h.s, g.s) and h.gamma == 3
    a, b = g.rank(rows[:4], k=5, kq=3), h.rank(rows[:4], k=5, kq=3)
    assert np.array_equal(a[0], b[0]) and _same(a[1], b[1])
    index.add({"new": rows[0] * 2})
    for graph in (g, h):
        with pytest.raises(RuntimeError, match="has changed"):
            graph.rank(rows[:4], k=5, kq=3)
    with pytest.raises(RuntimeError, match="has changed"):
        Diffusion.load(fn, index)
    del index["new"]                                          # the same rows again, but the graph cannot know: still refused
    with pytest.raises(RuntimeError, match="has changed"):
        g.rank(rows[:4], k=5, kq=3)
    g2 = Diffusion.build(index, k=4, gamma=3)                  # a new graph of the changed index ranks
    assert g2.rank(rows[:4], k=5, kq=3)[0].shape == (4, 5)
    for x in (g, h, g2):
        x.close()
    index.close()


def test_curves_corpus_through_the_device(gpu_ctx):
    """the device's lists are the twin's lists (fed with the index's own rankings), hence its precision: no separate threshold"""
    from pvsim import Diffusion
    from pvsim.index import DeviceIndex
    X, lab, Q, ql = tw.curves(seed=0)
    index = DeviceIndex({f"c{i:04d}": X[i] for i in range(len(X))}, gpu_ctx)
    g = Diffusion.build(index, k=10, gamma=3, block=512)
    di, dv = index.rank(X, 11)
    want_g = tw.graph_from_lists(di, dv, 3)
    assert _same(g.nbr, want_g["nbr"]) and _same(g.s, want_g["s"])
    idx, val = g.rank(Q, k=20, kq=5, alpha=0.99, tol=1e-6, maxiter=50)
    wi, wv, steps, rr, yy = _twin_rank(index, g, Q, 20, 5, 3, 0.99, 1e-6, 50)
    assert np.array_equal(idx, wi) and _same(val, wv)
    assert np.array_equal(g.last_solve["steps"], steps) and g.last_solve["converged"].all()
    plain = tw.precision(index.rank(Q, 20)[0], lab, ql)
    print(f"precision@20 on the device: plain {plain:.4f}, diffused {tw.precision(idx, lab, ql):.4f}, steps {steps.min()} .. {steps.max()}")
    assert tw.precision(idx, lab, ql) == tw.precision(wi, lab, ql)
    g.close()
    index.close()
