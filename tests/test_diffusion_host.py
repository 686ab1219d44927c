"""CPU tests of diffusion re-ranking (pvsim/diffusion.py): the entry points exist, arguments are validated
before any device is touched, and the NumPy twin (tests/diffusion_numpy.py) -- the statement every device result is held against in
tests/test_gpu_diffusion.py -- is itself held against a dense solve and measured on the curves corpus."""
import inspect

import numpy as np
import pytest

import diffusion_numpy as tw


class _FakeBuffer:
    def __init__(self, a):
        self.a = np.ascontiguousarray(a)

    def download(self, shape, dtype, offset=0):
        return self.a.view(np.uint8)[offset:].view(dtype)[:int(np.prod(shape))].reshape(shape).copy()

    def free(self):
        pass


def _graph_without_device(nbr, s, gamma, index=None):
    """a Diffusion over host arrays: enough for save / validation, which need no device"""
    from pvsim import Diffusion
    return Diffusion(None, _FakeBuffer(nbr.astype(np.int32)), _FakeBuffer(s), nbr.shape[0], nbr.shape[1], gamma, index)


def _seeded_graph(seed=3, N=200, kg=6, L=16, gamma=3, isolate=(5, 77)):
    """the graph of seeded rows by the twin; rows `isolate` get similarities <= 0 towards everyone, so their degree is 0"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, L))
    idx, val = tw.cosine_rank(X, X, kg + 1)
    for i in (i for i in isolate if i < N):
        val[i] = -np.abs(val[i])
        val[idx == i] = 0.0
    return tw.graph_from_lists(idx, val, gamma)


def test_module_class_bindings_and_keyword_exist():
    import pvsim
    from pvsim import _ffi, diffusion
    from pvsim import eval as ev
    from pvsim.index import DeviceIndex
    assert pvsim.Diffusion is diffusion.Diffusion and "Diffusion" in pvsim.__all__
    want = {"pvs_graph_affinity_dev": 11, "pvs_graph_mutual_dev": 6, "pvs_graph_degrees_dev": 6, "pvs_graph_normalise_dev": 7,
            "pvs_diffuse_rhs_dev": 9, "pvs_diffuse_workspace": 3, "pvs_diffuse_cg_dev": 18, "pvs_rank_f64_dev": 8}
    for name, nargs in want.items():
        assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name]) == nargs, name
        assert hasattr(_ffi.lib(), name), name
    assert _ffi.DIFFUSE_DOT_BLOCK == tw.DOT_BLOCK == 256
    assert _ffi.lib().pvs_version() == 103
    for fn in (ev.retrieve_top_k_similar, ev.top_k_map, ev.top_k_accuracy):
        assert inspect.signature(fn).parameters["diffuse"].default is None
    for name in ("graph_affinity_dev", "graph_mutual_dev", "graph_degrees_dev", "graph_normalise_dev", "diffuse_rhs_dev", "diffuse_cg_dev",
                 "rank_f64_dev"):
        assert callable(getattr(pvsim.Context, name))
    assert "_rank_dev_buffers" in vars(DeviceIndex)


def test_workspace_query_is_host_arithmetic():
    from pvsim.engine import diffuse_workspace
    a, b = diffuse_workspace(1000, 1), diffuse_workspace(1000, 64)
    assert a >= 3 * 1000 * 8 + 4 * 8 and b >= 64 * (3 * 1000 * 8 + 4 * 8) and a % 256 == 0 and b % 256 == 0
    for bad in ((0, 1), (1000, 0), (1 << 31, 1), (1000, (1 << 16) + 1)):
        with pytest.raises(ValueError):
            diffuse_workspace(*bad)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """the host checks come before the context is used: with a made-up context pointer, every call below must be refused without
    dereferencing it"""
    import ctypes as C
    from pvsim import _ffi
    lib = _ffi.lib()
    ctx = C.c_void_p(0x1000)                     # never dereferenced: every call below is refused first
    p = [C.c_void_p(0x100000 * (i + 1)) for i in range(8)]        # made-up device arrays, 1 MiB apart

    def msg():
        return lib.pvs_last_error().decode()

    assert lib.pvs_graph_mutual_dev(ctx, p[0], p[1], 10, 10, p[2]) == _ffi.PVS_ERR_INVALID and "kg <= N - 1" in msg()
    assert lib.pvs_graph_affinity_dev(ctx, p[0], p[1], 1, 4, 3, 8, 10, 3, p[2], p[3]) == _ffi.PVS_ERR_INVALID and "leave the index" in msg()
    assert lib.pvs_graph_affinity_dev(ctx, p[0], p[1], 1, 4, 3, 0, 10, 9, p[2], p[3]) == _ffi.PVS_ERR_INVALID and "gamma" in msg()
    assert lib.pvs_diffuse_rhs_dev(ctx, p[0], p[1], 1, 2, 11, 10, 3, p[2]) == _ffi.PVS_ERR_INVALID and "kq <= N" in msg()

    def cg(N=1000, kg=5, Cc=3, alpha=0.9, tol=1e-6, maxiter=5, every=1, width=0, work=p[3], wbytes=1 << 20, x=p[4], y=p[2]):
        return lib.pvs_diffuse_cg_dev(ctx, p[0], p[1], N, kg, y, Cc, alpha, tol, maxiter, every, width, work, wbytes, x, p[5], p[6], p[7])

    for kw, word in (({"alpha": 0.0}, "alpha"), ({"alpha": 1.0}, "alpha"), ({"alpha": float("nan")}, "alpha"), ({"kg": 1000}, "kg <= N - 1"),
                     ({"tol": -1.0}, "tol"), ({"maxiter": -1}, "maxiter"), ({"every": 0}, "check_every"), ({"width": 8}, "width"),
                     ({"Cc": 0}, "columns"), ({"wbytes": 1000}, "work buffer"), ({"x": p[2]}, "overlaps"),
                     ({"x": C.c_void_p(p[3].value + 512)}, "overlaps"), ({"work": C.c_void_p(p[3].value + 8)}, "aligned")):
        assert cg(**kw) == _ffi.PVS_ERR_INVALID, kw
        assert word in msg(), (kw, msg())
    assert lib.pvs_rank_f64_dev(ctx, p[0], 2, 10, 10, 11, p[1], p[2]) == _ffi.PVS_ERR_INVALID and "k <= ncols" in msg()


@pytest.mark.parametrize("kwargs", [{"alpha": 0.0}, {"alpha": 1.0}, {"alpha": "0.5"}, {"tol": -1e-3}, {"tol": float("inf")}, {"maxiter": -1},
                                    {"maxiter": 2.5}, {"check_every": 0}, {"width": 2}, {"width": 128}])
def test_solver_arguments_validate(kwargs):
    g = _seeded_graph(N=40, kg=3)
    d = _graph_without_device(g["nbr"], g["s"], 3)
    with pytest.raises(ValueError):
        d.solve(np.zeros((40, 1)), **kwargs)


def test_build_rank_and_eval_validate_without_a_device():
    from pvsim import Diffusion, QueryExpansion
    from pvsim import eval as ev
    from pvsim.index import DeviceIndex
    with pytest.raises(TypeError, match="DeviceIndex"):
        Diffusion.build({"a": np.ones(4, np.float32), "b": np.ones(4, np.float32)})
    with pytest.raises(TypeError, match="DeviceIndex"):
        Diffusion.load("nowhere.npz", {"a": np.ones(4, np.float32)})
    g = _seeded_graph(N=40, kg=3)
    d = _graph_without_device(g["nbr"], g["s"], 3)
    with pytest.raises(RuntimeError, match="without an index"):
        d.rank(np.zeros((1, 16), np.float32))
    with pytest.raises(ValueError, match="float64 array of shape"):
        d.solve(np.zeros((39, 1)))
    with pytest.raises(ValueError):
        Diffusion.from_arrays(g["nbr"], g["s"].astype(np.float32), 3)
    with pytest.raises(ValueError):
        Diffusion.from_arrays(g["nbr"], g["s"], 9)

    class NoEncoder:
        def encode(self, *_):
            raise AssertionError("refused before the query is encoded")

    index = DeviceIndex.__new__(DeviceIndex)                 # no device here; the refusals need none
    index._paths, index.modifications = [f"p{i}" for i in range(40)], 0
    other = DeviceIndex.__new__(DeviceIndex)
    other._paths, other.modifications = list(index._paths), 0
    d = _graph_without_device(g["nbr"], g["s"], 3, index)
    img = np.zeros((4, 4, 3), np.uint8)
    labels = {p: 0 for p in index._paths}
    calls = (lambda **kw: ev.retrieve_top_k_similar(img, kw.pop("ds"), NoEncoder(), k=1, **kw),
             lambda **kw: ev.top_k_map([img], [0], kw.pop("ds"), labels, NoEncoder(), k=1, **kw),
             lambda **kw: ev.top_k_accuracy([img], [0], kw.pop("ds"), labels, NoEncoder(), k=1, **kw))
    for call in calls:
        with pytest.raises(TypeError, match="dict or a compact index"):
            call(ds={p: np.ones(4, np.float32) for p in index._paths}, diffuse=d)
        with pytest.raises(TypeError, match="pvsim.Diffusion"):
            call(ds=index, diffuse="graph")
        with pytest.raises(ValueError, match="another index"):
            call(ds=other, diffuse=d)
        for extra in ({"expand": QueryExpansion(n=1)}, {"rerank": 5}, {"nprobe": 2}):
            with pytest.raises(ValueError, match="excludes"):
                call(ds=index, diffuse=d, **extra)
    index.modifications = 1                                  # what add / remove do
    with pytest.raises(RuntimeError, match="has changed"):
        d.rank(np.zeros((1, 16), np.float32))


def test_npz_round_trip_of_a_hand_made_graph(tmp_path):
    nbr = np.array([[1, 2], [0, 2], [0, 1], [0, -1]], np.int32)
    s = np.array([[.5, .25], [.5, .125], [.25, .125], [0, 0]])
    d = _graph_without_device(nbr, s, 2)
    fn = str(tmp_path / "graph.npz")
    d.save(fn)
    with np.load(fn, allow_pickle=False) as z:               # arrays only: loads without pickles
        assert sorted(z.files) == ["gamma", "index_modifications", "nbr", "s"]
        assert np.array_equal(z["nbr"], nbr) and z["nbr"].dtype == np.int32
        assert np.array_equal(z["s"].view(np.uint8), s.view(np.uint8))
        assert int(z["gamma"]) == 2 and int(z["index_modifications"]) == 0
    from pvsim import Diffusion
    from pvsim.index import DeviceIndex
    index = DeviceIndex.__new__(DeviceIndex)
    index._paths, index.modifications = list("abcd"), 2      # changed since the build
    with pytest.raises(RuntimeError, match="has changed"):
        Diffusion.load(fn, index)
    index._paths, index.modifications = list("abc"), 0       # another size
    with pytest.raises(RuntimeError, match="has changed"):
        Diffusion.load(fn, index)


def test_twin_definitions_by_hand():
    """the twin against the definitions written out scalar by scalar"""
    idx = np.array([[0, 1, 2], [1, 0, 3], [3, 0, 1], [0, 1, 2]])          # row 2 and row 3 are absent from their own lists
    val = np.array([[1, .5, .25], [1, .5, -.5], [.75, .25, .125], [.5, .25, 0]])
    i, v = tw.drop_self(idx, val, np.arange(4))
    assert np.array_equal(i, [[1, 2], [0, 3], [3, 0], [0, 1]]) and np.array_equal(v, [[.5, .25], [.5, -.5], [.75, .25], [.5, .25]])
    assert np.array_equal(tw.affinity(v, 0), np.ones((4, 2)))
    assert np.array_equal(tw.affinity(v, 1), np.maximum(v, 0))
    a = tw.affinity(v, 3)
    assert np.array_equal(a, [[.125, .015625], [.125, 0], [.421875, .015625], [.125, .015625]])
    w = tw.mutual(i.astype(np.int32), a)
    # 0-1 mutual (min .125, .125); 0-2 mutual (min .015625, .015625); 1-3 mutual (min 0, .015625) = 0; 2-3 one-sided; 3-0 one-sided
    assert np.array_equal(w, [[.125, .015625], [.125, 0], [0, .015625], [0, 0]])
    deg, r = tw.degrees(w)
    assert np.array_equal(deg, [.140625, .125, .015625, 0]) and r[3] == 0 and r[2] == 8.0
    s = tw.normalise(i.astype(np.int32), w, r)
    assert s[0, 0] == .125 * (r[0] * r[1]) and s[1, 0] == s[0, 0] and s[2, 1] == s[0, 1] and not s[3].any()
    u = np.arange(1, 301, dtype=np.float64).reshape(300, 1) * np.array([[1.0, 1e-3]])
    d = tw.dot(u, np.ones_like(u))
    blocks = [u[:256], np.vstack([u[256:], np.zeros((212, 2))])]
    want = np.zeros(2)
    for b in blocks:
        t = b.copy()
        for h in (128, 64, 32, 16, 8, 4, 2, 1):
            t[:h] = t[:h] + t[h:2 * h]
        want = want + t[0]
    assert np.array_equal(d, want)
    Y = tw.rhs(np.array([[2, 0], [1, 7]]), np.array([[.5, -1.0], [.25, .9]]), 4, 2)
    assert np.array_equal(Y, [[0, 0], [0, .0625], [.25, 0], [0, 0]])
    F = np.array([[1.0, np.nan], [-0.0, 2], [3, 2], [0.0, -1]])
    ri, rv = tw.rank_scores(F, 4)
    assert np.array_equal(ri, [[2, 0, 1, 3], [1, 2, 3, 0]]) and np.isnan(rv[1, 3]) and not np.signbit(rv[0, 2])


def test_s_is_symmetric_to_the_bit_with_isolated_rows():
    for gamma in (1, 3):
        g = _seeded_graph(gamma=gamma)
        assert g["deg"][5] == 0 and g["deg"][77] == 0 and g["r"][5] == 0 and not g["s"][5].any()
        assert (g["deg"] > 0).sum() >= 150
        one_sided = (g["w"] == 0) & (g["a"] > 0)
        assert one_sided.any() and (g["w"] > 0).any()                    # mutual and one-sided pairs are both there
        S = tw.dense(g["nbr"], g["s"])
        assert np.array_equal(S.view(np.uint64), S.T.view(np.uint64))
        assert np.abs(np.linalg.eigvalsh(S)).max() <= 1 + 1e-12


@pytest.mark.parametrize("alpha", [0.5, 0.99])
def test_twin_cg_against_the_dense_solve(alpha):
    """|f - f_dense|_2 <= rho / (1 - alpha) + N 2^-52 kappa |f_dense|_2 with rho the residual recomputed from f in float64 and
    kappa = (1 + alpha) / (1 - alpha): the eigenvalues of I - alpha S lie in [1 - alpha, 1 + alpha], so an error is at most the
    residual over 1 - alpha; the second term is the dense solver's own backward error.  Measured: the error sits at 0.58 .. 0.60
    of the bound at alpha = 0.5 and at 0.03 of it at alpha = 0.99."""
    g = _seeded_graph()
    N = g["nbr"].shape[0]
    rng = np.random.default_rng(8)
    Y = np.zeros((N, 6))
    for c in range(4):
        Y[rng.choice(N, 5, replace=False), c] = rng.random(5)
    Y[5, 4] = 0.75                                                           # supported on an isolated row; column 5 stays zero
    tol = 1e-6
    x, steps, rr, yy = tw.cg(g["nbr"], g["s"], Y, alpha, tol, 200)
    dense = tw.dense_solve(g["nbr"], g["s"], Y, alpha)
    rho = tw.residual_norm(g["nbr"], g["s"], Y, x, alpha)
    err = np.sqrt(((x - dense) ** 2).sum(axis=0))
    bound = rho / (1 - alpha) + N * 2.0 ** -52 * (1 + alpha) / (1 - alpha) * np.sqrt((dense ** 2).sum(axis=0))
    print("steps", steps, "error / bound", err[:5] / bound[:5])
    assert (err <= bound).all()
    assert (rr <= tol * tol * yy).all()                                      # every column converged, by construction of the stop
    assert steps[5] == 0 and not x[:, 5].any() and yy[5] == 0
    assert steps[4] == 1 and np.array_equal(x[:, 4], Y[:, 4])                # S y = 0: exact after one step
    assert (steps[:4] > 1).all()
    capped = tw.cg(g["nbr"], g["s"], Y, alpha, 1e-12, 3)
    assert (capped[1][:4] == 3).all() and (capped[2][:4] > 1e-24 * capped[3][:4]).all()


def test_each_column_depends_on_itself_alone():
    g = _seeded_graph()
    N = g["nbr"].shape[0]
    rng = np.random.default_rng(9)
    Y = rng.random((N, 5)) * (rng.random((N, 5)) < 0.05)
    x, steps, rr, yy = tw.cg(g["nbr"], g["s"], Y, 0.9, 1e-8, 50)
    for c in range(5):
        xc, sc, rc, yc = tw.cg(g["nbr"], g["s"], Y[:, c:c + 1], 0.9, 1e-8, 50)
        assert np.array_equal(xc[:, 0].view(np.uint64), x[:, c].view(np.uint64)) and sc[0] == steps[c] and rc[0] == rr[c] and yc[0] == yy[c]


def test_diffusion_helps_on_the_curves_corpus():
    """32 curves x 32 rows in 64-d, noise 0.5 of the spacing along a curve, 256 queries; kg = 10, kq = 5, gamma = 3, alpha = 0.99,
    tol = 1e-6, at most 50 steps.  Measured with the twin, seed 0: precision@20 0.7619 plain, 1.0000 diffused (gain 0.2381;
    conjugate gradients took 14 .. 42 steps).  The run is deterministic; the asserted margin of half the measured gain only guards
    against later edits of the generator.  The plain ranking is the baseline, never the code under test."""
    X, lab, Q, ql = tw.curves(seed=0)
    assert X.shape == (1024, 64) and Q.shape == (256, 64) and X.dtype == np.float32
    k = 20
    i0, s0 = tw.cosine_rank(Q, X, k)
    plain = tw.precision(i0, lab, ql)
    di, dv = tw.cosine_rank(X, X, 11)
    g = tw.graph_from_lists(di, dv, 3)
    idx, val, steps, rr, yy = tw.diffuse_rank(g, i0[:, :5], s0[:, :5], 3, 0.99, 1e-6, 50, k)
    diffused = tw.precision(idx, lab, ql)
    print(f"precision@20: plain {plain:.4f}, diffused {diffused:.4f}, steps {steps.min()} .. {steps.max()}")
    assert (rr <= 1e-12 * yy).all()
    assert diffused >= plain + 0.119
