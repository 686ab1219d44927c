"""Device memory that is handed out again without being cleared: the workspace slots of a context (csrc/workspace.hpp), its table block
cache (table_alloc / table_free in csrc/api.hip) and the buffer cache of pvsim.Context.

A CASE is a function of a `Run` (one context): it queues one entry point on seeded inputs and registers every output the entry point
writes, the statistics it reports included.  `Run.finish()` returns them as a dict of arrays.  For every case:

  fresh      a new context, every slot grows inside the call; the result is held against the family's NumPy twin or golden file at that
             family's tolerance, so that "equal to fresh" below never means "equally wrong".  Computed once and shared.
  poisoned   a second context on which the `big` form of the case has run first: every slot the case uses is at least as large as
             the fresh context left it (pvs_diag_ws_bytes) and does not grow again.  Slots, table block cache and the buffer cache are
             filled with 0xFF (NaN / -1 / the largest unsigned), 0x00 and 0x5A (large and finite) in turn; the bytes out must be those
             of the fresh run.
  neighbour  directly behind a case of another family that carves the same slot with another layout, nothing fetched in between.

Output buffers are pre-filled with 0xEE, so what an entry point leaves alone by contract compares equal as well.  The last test holds
the covered (slot, function) pairs against the table parsed out of workspace.hpp: a new ws_reserve user without a case fails there.
Every test opens and closes its own contexts, two at most at a time; the session context is never poisoned."""
import functools

import numpy as np
import pytest

import ws_ledger
from conftest import load_golden

pytestmark = pytest.mark.gpu

FILL_OUT = 0xEE
POISON_BYTES = (0xFF, 0x00, 0x5A)
DESC_F32, DESC_F32_ROOTSIFT, DESC_U8_ROOTSIFT = 0, 1, 2


# ====================================================================================================================== the harness
class Run:
    """One run of a case: its device buffers, the outputs it registers, and the checks against the twin it leaves for the fresh run."""

    def __init__(self, ctx, big=False, fetch=True):
        self.ctx, self.big, self.fetch = ctx, big, fetch
        self._bufs, self._outs, self._handles, self.res, self.checks = [], [], [], {}, []

    def up(self, a):
        a = np.ascontiguousarray(a)
        b = self.ctx.buffer(max(a.nbytes, 16))
        if a.nbytes:
            b.upload(a)
        self._bufs.append(b)
        return b

    def out(self, name, shape, dtype):
        shape = tuple(int(s) for s in np.atleast_1d(shape))
        n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        b = self.ctx.buffer(max(n, 16)).fill_bytes(FILL_OUT)
        self._bufs.append(b)
        self._outs.append((name, b, shape, dtype))
        return b

    def put(self, name, value):
        """a result the entry point hands to the host"""
        if isinstance(value, dict):
            value = np.array([int(v) if not isinstance(v, str) else sum(map(ord, v)) for v in value.values()], np.int64)
        self.res[name] = np.ascontiguousarray(value).copy()

    def own(self, handle):
        self._handles.append(handle)
        return handle

    def expect(self, check):
        """check(res): asserted on the fresh run only"""
        self.checks.append(check)

    def finish(self):
        try:
            if self.fetch:
                for name, b, shape, dtype in self._outs:
                    n = int(np.prod(shape, dtype=np.int64))
                    self.res[name] = b.download(shape, dtype) if n else np.zeros(shape, dtype)
        finally:
            for b in self._bufs:
                b.free()
            for h in self._handles:
                h.close()
        return self.res if self.fetch else None


CASES = {}


def case(covers, capped=(), grow=None):
    """covers: "WS_SLOT:function" pairs of the table in workspace.hpp that the case reaches; capped: slots whose block is bounded by a
    byte budget, so that the big form cannot make them larger than the case itself does; grow: the case whose big form enlarges the
    slots on the second context (the case's own big form when None: a block of a fixed size needs another user of the slot)"""
    def deco(fn):
        fn.covers = [tuple(c.split(":")) for c in covers]
        fn.capped = set(capped)
        fn.grow = grow
        CASES[fn.__name__] = fn
        return fn
    return deco


def execute(ctx, name, big=False, fetch=True):
    r = Run(ctx, big, fetch)
    try:
        CASES[name](r)
    except BaseException:
        r.fetch = False
        r.finish()
        raise
    return r, r.finish()


def same_bytes(got, want, where):
    assert sorted(got) == sorted(want), (where, sorted(got), sorted(want))
    for key in want:
        a, b = got[key], want[key]
        assert a.dtype == b.dtype and a.shape == b.shape, (where, key, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            ab, bb = a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8)
            first = int(np.flatnonzero(ab != bb)[0]) // a.dtype.itemsize
            raise AssertionError(f"{where}: output {key!r} differs from the fresh run in {int((ab != bb).sum())} bytes, first at element "
                                 f"{first}: {a.reshape(-1)[first]!r} instead of {b.reshape(-1)[first]!r}")


def poison(ctx, byte):
    """everything the context would hand out again: its workspace slots, its table block cache, the buffer cache of the Python layer"""
    import ctypes as C
    from pvsim import _ffi
    ctx.diag_poison(byte, _ffi.POISON_WORKSPACE | _ffi.POISON_TABLE_CACHE)
    for cap, p in ctx._cache:
        _ffi.check(_ffi.lib().pvs_memset(ctx.handle, C.c_void_p(p), int(byte), int(cap)))


@functools.lru_cache(maxsize=None)
def fresh(name):
    """-> (outputs, slot capacities afterwards, checks) of the case on a context of its own"""
    import pvsim
    ctx = pvsim.Context(0)
    try:
        assert not any(ctx.diag_ws_bytes().values()), "a new context holds a workspace block"
        r, res = execute(ctx, name)
        ctx.sync()
        return res, ctx.diag_ws_bytes(), r.checks
    finally:
        ctx.close()


# ====================================================================================================================== inputs
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _clustered(seed, n, L, spread=0.6, protos=40):
    """n float32 rows around `protos` directions: neighbours and scores are well separated"""
    rng = np.random.default_rng(seed)
    proto = rng.standard_normal((protos, L))
    return (proto[np.arange(n) % protos] + spread * rng.standard_normal((n, L))).astype(np.float32)


def _inv_norms(r, d_x, n, L):
    d_inv = r.ctx.buffer(max(n * 4, 16))
    r._bufs.append(d_inv)
    r.ctx.row_inv_norms_dev(d_x.ptr, n, L, d_inv.ptr)
    return d_inv


def _cosine64(q, x):
    q, x = q.astype(np.float64), x.astype(np.float64)
    nq, nx = np.linalg.norm(q, axis=1, keepdims=True), np.linalg.norm(x, axis=1, keepdims=True)
    return (q / np.where(nq > 0, nq, 1)) @ (x / np.where(nx > 0, nx, 1)).T


def _expect_ranking(r, idx_key, q, x, k, rows=slice(None)):
    """the lists are those of the float64 scores wherever those are unambiguous (gap above 1e-6 relative among the k + 1 best)"""
    def check(res):
        s = _cosine64(q, x)[rows]
        order = np.argsort(-s, axis=1, kind="stable")[:, :k + 1]
        best = np.take_along_axis(s, order, 1)
        clear = (np.abs(np.diff(best, axis=1)) > 1e-6 * np.maximum(np.abs(best[:, :-1]), np.abs(best[:, 1:]))).all(axis=1)
        assert clear.mean() > 0.9, clear.mean()
        assert np.array_equal(res[idx_key][rows][clear], order[clear, :k])
    r.expect(check)


# ====================================================================================================================== encoders
def _golden_images(big):
    g = load_golden("vlad_k256_d128")
    raw, off = g["raw_u8"], g["offsets"]
    if big:                                                     # the same images twice
        raw, off = np.concatenate([raw, raw]), np.concatenate([off, off[1:] + off[-1]])
    return g, np.ascontiguousarray(raw), np.ascontiguousarray(off)


@case(["WS_STAGE_IN:pvs_vlad_encode", "WS_PANEL_OUT:pvs_vlad_encode", "WS_LISTS:launch_assign"])
def vlad_host(r):
    """4654 uint8 rows: above the 4096 rows from which the assignment prefilter carves its list block"""
    g, raw, off = _golden_images(r.big)
    assert off[-1] >= 4096
    cb = r.own(r.ctx.codebook(load_golden("tables_k256_d128")["centroids"]))
    v, labels = r.ctx.vlad_encode(cb, raw, off, DESC_U8_ROOTSIFT, return_labels=True)
    r.put("vlad", v), r.put("labels", labels)
    r.expect(lambda res: np.testing.assert_allclose(res["vlad"], g["vlad"], rtol=0, atol=5e-7))
    r.expect(lambda res: np.array_equal(res["labels"], g["labels"]) or pytest.fail("labels differ from the golden file"))


@case(["WS_PROJECTED:project_if_needed", "WS_STAGE_IN:pvs_vlad_encode"])
def vlad_host_pca(r):
    g, raw, off = _golden_images(r.big)
    t, gp = load_golden("tables_k256_d128"), load_golden("vlad_pca64_k256")
    n = int(gp["n_images"]) if not r.big else len(off) - 1
    cb, pca = r.own(r.ctx.codebook(t["centroids_pca64"])), r.own(r.ctx.pca(t["pca_components"], t["pca_mean"]))
    r.put("vlad", r.ctx.vlad_encode(cb, raw[:off[n]], off[:n + 1], DESC_U8_ROOTSIFT, pca=pca))
    r.expect(lambda res: np.testing.assert_allclose(res["vlad"], gp["vlad"], rtol=0, atol=5e-6))


@case(["WS_SCRATCH:pvs_vlad_encode_dev"])
def vlad_dev_without_labels(r):
    """the device form without a label output: the labels live in WS_SCRATCH"""
    g, raw, off = _golden_images(r.big)
    cb = r.own(r.ctx.codebook(load_golden("tables_k256_d128")["centroids"]))
    n = len(off) - 1
    d_x, d_off = r.up(raw), r.up(off)
    d_out, d_inv = r.out("vlad", (n, 256 * 128), np.float32), r.out("inv_norm", (n,), np.float32)
    r.ctx.vlad_encode_dev(cb, d_x.ptr, DESC_U8_ROOTSIFT, d_off.ptr, n, int(off[-1]), d_out.ptr, d_inv_norm=d_inv.ptr)
    r.expect(lambda res: np.testing.assert_allclose(res["vlad"], g["vlad"], rtol=0, atol=5e-7))


def _fisher_images(big):
    import pvsim_oracle as orc
    from pvsim import pack_descriptors
    g, f = load_golden("vlad_k256_d128"), load_golden("fisher_k256_d128")
    raws = orc.split_ragged(g["raw_u8"], g["offsets"])
    sel = [raws[i] for i in f["image_index"]]
    return f, pack_descriptors(sel + sel if big else sel, 128, np.uint8)


@case(["WS_STAGE_IN:pvs_fisher_encode", "WS_PANEL_OUT:pvs_fisher_encode", "WS_SCRATCH:launch_fisher", "WS_AUX_ROWS:materialise_f32"])
def fisher_host(r):
    """uint8 rows: the RootSIFT rows are materialised in WS_AUX_ROWS first"""
    f, (packed, off) = _fisher_images(r.big)
    t = load_golden("tables_k256_d128")
    gm = r.own(r.ctx.gmm(t["gmm_weights"], t["gmm_means"], t["gmm_covariances"]))
    r.put("fisher", r.ctx.fisher_encode(gm, packed, off, DESC_U8_ROOTSIFT))
    r.expect(lambda res: np.testing.assert_allclose(res["fisher"], f["fisher"], rtol=0, atol=1e-9))


@case(["WS_PROJECTED:project_if_needed", "WS_STAGE_IN:pvs_fisher_encode"])
def fisher_host_pca(r):
    g, raw, off = _golden_images(r.big)
    t, fp = load_golden("tables_k256_d128"), load_golden("fisher_pca64_k64")
    n = int(fp["n_images"]) if not r.big else len(off) - 1
    gm = r.own(r.ctx.gmm(t["gmmp_weights"], t["gmmp_means"], t["gmmp_covariances"]))
    pca = r.own(r.ctx.pca(t["pca_components"], t["pca_mean"]))
    r.put("fisher", r.ctx.fisher_encode(gm, raw[:off[n]], off[:n + 1], DESC_U8_ROOTSIFT, pca=pca))
    r.expect(lambda res: np.testing.assert_allclose(res["fisher"], fp["fisher"], rtol=0, atol=2e-6))


@case(["WS_SCRATCH:launch_gmm_posterior"])
def gmm_posterior(r):
    import pvsim_oracle as orc
    g, f, t = load_golden("vlad_k256_d128"), load_golden("fisher_k256_d128"), load_golden("tables_k256_d128")
    x = orc.rootsift(orc.split_ragged(g["raw_u8"], g["offsets"])[3].astype(np.float32))
    if r.big:
        x = np.concatenate([x, x, x])
    gm = r.own(r.ctx.gmm(t["gmm_weights"], t["gmm_means"], t["gmm_covariances"]))
    d_x, d_resp = r.up(x), r.out("resp", (len(x), 256), np.float64)
    r.ctx.gmm_predict_proba_dev(gm, d_x.ptr, DESC_F32, len(x), d_resp.ptr)
    r.expect(lambda res: np.testing.assert_allclose(res["resp"], f["resp_img3"], rtol=0, atol=1e-12))


# ====================================================================================================================== similarity
def _pin_gemm_slots(r):
    """64 workgroup slots whatever the chip: three tiles are split over k, so the GEMM carves its partial images out of WS_AUX_ROWS"""
    from pvsim import _ffi
    r.ctx.set_option(_ffi.OPT_GEMM_SLOTS, 64)


def _unpin_gemm_slots(r):
    from pvsim import _ffi
    r.ctx.set_option(_ffi.OPT_GEMM_SLOTS, 0)


@case(["WS_STAGE_IN:pvs_cosine", "WS_PANEL_OUT:pvs_cosine", "WS_AUX_ROWS:launch_gemm_mfma"])
def cosine_host_f32(r):
    """1 x 3 tiles of rows 2600 long under 64 slots: every tile is split over k (the plan is read back)"""
    s = 2 if r.big else 1
    a, b = _clustered(31, 100 * s, 2600), _clustered(32, 384 * s, 2600)
    _pin_gemm_slots(r)
    try:
        r.put("scores", r.ctx.cosine(a, b))
        plan = r.ctx.gemm_last_plan()
    finally:
        _unpin_gemm_slots(r)
    r.put("plan", plan)
    r.expect(lambda res: plan["n_tail"] > 0 and plan["nparts"] > 1 or pytest.fail(f"no split-K tail ran: {plan}"))
    r.expect(lambda res: np.testing.assert_allclose(res["scores"], _cosine64(a, b), rtol=0, atol=2e-6))


@case(["WS_SCRATCH:launch_cosine_f64", "WS_AUX_ROWS:launch_gemm_f64", "WS_STAGE_IN:pvs_cosine"])
def cosine_host_f64(r):
    s = 2 if r.big else 1
    a, b = _clustered(33, 100 * s, 2600).astype(np.float64), _clustered(34, 384 * s, 2600).astype(np.float64)
    _pin_gemm_slots(r)
    try:
        r.put("scores", r.ctx.cosine(a, b))
        plan = r.ctx.gemm_last_plan()
    finally:
        _unpin_gemm_slots(r)
    r.put("plan", plan)
    r.expect(lambda res: plan["n_tail"] > 0 and plan["nparts"] > 1 or pytest.fail(f"no split-K tail ran: {plan}"))
    r.expect(lambda res: np.testing.assert_allclose(res["scores"], _cosine64(a, b), rtol=0, atol=1e-12))


@case(["WS_STAGE_IN:pvs_cosine_topk", "WS_SCRATCH:pvs_cosine_topk", "WS_PANEL_OUT:cosine_topk_impl", "WS_PANEL_OUT:panel_query_block"])
def topk_host(r):
    """fewer than 512 queries: the plain path, GEMM panel + select"""
    s = 2 if r.big else 1
    q, x, k = _clustered(41, 130 * s, 64), _clustered(42, 600 * s, 64), 5
    idx, val = r.ctx.cosine_topk(q, x, k)
    r.put("idx", idx), r.put("val", val)
    _expect_ranking(r, "idx", q, x, k)


@case(["WS_PANEL_OUT:cosine_topk_impl"])
def topk_host_two_queries(r):
    """one or two queries: the score rows of the one-pass kernel, reserved by cosine_topk_impl itself"""
    q, x, k = _clustered(43, 2, 64), _clustered(44, 700 * (3 if r.big else 1), 64), 7
    idx, val = r.ctx.cosine_topk(q, x, k)
    r.put("idx", idx), r.put("val", val)
    _expect_ranking(r, "idx", q, x, k)


@case(["WS_STAGE_IN:pvs_cosine_topk_f64", "WS_LISTS:pvs_cosine_topk_f64", "WS_PANEL_OUT:pvs_cosine_topk_f64_dev"])
def topk_f64_host(r):
    s = 2 if r.big else 1
    q, x, k = _clustered(45, 70 * s, 48).astype(np.float64), _clustered(46, 400 * s, 48).astype(np.float64), 6
    idx, val = r.ctx.cosine_topk_f64(q, x, k)
    r.put("idx", idx), r.put("val", val)
    _expect_ranking(r, "idx", q, x, k)
    r.expect(lambda res: np.testing.assert_allclose(res["val"], -np.sort(-_cosine64(q, x), axis=1)[:, :k], rtol=0, atol=1e-12))


def _filtered(r, x, k):
    n, L = x.shape
    d_x = r.up(x)
    d_inv = _inv_norms(r, d_x, n, L)
    d_idx, d_val = r.out("idx", (n, k), np.int64), r.out("val", (n, k), np.float32)
    st = r.ctx.cosine_topk_filtered_dev(d_x.ptr, n, d_x.ptr, n, L, d_inv.ptr, d_inv.ptr, k, d_idx.ptr, d_val.ptr)
    r.put("stats", st)
    return st


@case(["WS_FP16_ROWS:launch_cosine_topk_filtered", "WS_LISTS:launch_cosine_topk_filtered", "WS_PANEL_OUT:launch_cosine_topk_filtered"])
def filtered_topk(r):
    x, k = _clustered(15, 600 * (2 if r.big else 1), 64), 5
    st = _filtered(r, x, k)
    r.expect(lambda res: st["filtered"] and st["redone_exact"] == 0 or pytest.fail(f"the prefilter declined or overflowed: {st}"))
    _expect_ranking(r, "idx", x, x, k)


@case(["WS_PROJECTED:launch_cosine_topk_filtered", "WS_LISTS:launch_cosine_topk_filtered"])
def filtered_topk_overflow(r):
    """three all-zero rows score 0 against every row: more candidates than slots, redone by the exact path from WS_PROJECTED"""
    n = 400 * (2 if r.big else 1)
    x, k = np.concatenate([_clustered(16, n, 256), np.zeros((3, 256), np.float32)]), 5
    st = _filtered(r, x, k)
    r.expect(lambda res: st["filtered"] and st["redone_exact"] == 3 or pytest.fail(f"the three zero rows were not redone: {st}"))
    _expect_ranking(r, "idx", x, x, k, rows=slice(0, n))


# ====================================================================================================================== neighbours
def _lattice(seed, n, L, a, dtype=np.float32):
    import neighbors_numpy as nn
    return nn.lattice(seed, n, L, a, dtype)


def _knn(r, Q, X, k):
    import neighbors_numpy as nn
    d_x = r.up(X)
    d_q = d_x if Q is X else r.up(Q)
    d_idx, d_sq = r.out("idx", (len(Q), k), np.int64), r.out("sqdist", (len(Q), k), np.float64)
    st = r.ctx.l2_knn_dev(d_q.ptr, len(Q), d_x.ptr, len(X), X.shape[1], X.dtype == np.float64, k, d_idx.ptr, d_sq.ptr, stats=True)
    r.put("stats", st)

    def check(res):
        want = nn.knn_lists(Q, X, k)
        assert np.array_equal(res["idx"], want[0]) and np.array_equal(res["sqdist"], want[1])
    r.expect(check)
    return st


@case(["WS_NB_NORMS:pvs_l2_knn_dev", "WS_LISTS:pvs_l2_knn_dev", "WS_PANEL_OUT:pvs_l2_knn_dev"])
def knn_f32(r):
    """300 float32 rows: the prefilter with its carved list block"""
    s = 5 if r.big else 1
    st = _knn(r, _lattice(5101, 67 * s, 12, 4), _lattice(101, 300 * s, 12, 4), 10)
    r.expect(lambda res: st["filtered"] and st["overflowed"] == 0 or pytest.fail(f"the float32 path did not run: {st}"))


@case(["WS_LISTS:knn_f64_rows", "WS_PANEL_OUT:knn_f64_rows", "WS_NB_NORMS:pvs_l2_knn_dev"])
def knn_f64(r):
    s = 5 if r.big else 1
    st = _knn(r, _lattice(5101, 67 * s, 12, 4, np.float64), _lattice(101, 300 * s, 12, 4, np.float64), 10)
    r.expect(lambda res: not st["filtered"] or pytest.fail(str(st)))


@case(["WS_NB_F64_ROWS:to_f64_copies", "WS_LISTS:knn_f64_rows"])
def knn_f32_overflow(r):
    """300 identical rows overflow their 256 slots: everything is redone from float64 copies of the rows"""
    X = _lattice(301, 700 * (2 if r.big else 1), 12, 4)
    X[:300] = X[0]
    st = _knn(r, X, X, 10)
    r.expect(lambda res: st["filtered"] and st["overflowed"] >= 300 or pytest.fail(str(st)))


@case(["WS_NB_NORMS:radius_impl", "WS_PANEL_OUT:radius_impl", "WS_NB_F64_ROWS:to_f64_copies"])
def radius_f32(r):
    import neighbors_numpy as nn
    s = 3 if r.big else 1
    Q, X, r_sq = _lattice(402, 130 * s, 12, 2), _lattice(403, 700 * s, 12, 2), 30.0
    want = nn.radius_csr(Q, X, r_sq)                           # the sizes of the outputs are the twin's: the device must fill them exactly
    nq, nnz = len(Q), int(want[0][-1])
    d_x, d_q = r.up(X), r.up(Q)
    d_cnt = r.out("counts", (nq,), np.int64)
    r.ctx.l2_radius_count_dev(d_q.ptr, nq, d_x.ptr, len(X), 12, False, r_sq, d_cnt.ptr)
    d_ptr = r.up(want[0])
    d_ind, d_sq = r.out("indices", (nnz + 1,), np.int64), r.out("sqdist", (nnz + 1,), np.float64)
    r.ctx.l2_radius_fill_dev(d_q.ptr, nq, d_x.ptr, len(X), 12, False, r_sq, d_ptr.ptr, d_ind.ptr, d_sq.ptr)

    def check(res):
        assert np.array_equal(res["counts"], np.diff(want[0]))
        assert np.array_equal(res["indices"][:nnz], want[1]) and np.array_equal(res["sqdist"][:nnz], want[2])
        assert (res["indices"][nnz:].view(np.uint8) == FILL_OUT).all()
    r.expect(check)


# ====================================================================================================================== training
def _train_lattice(seed, n, D, hi=16):
    return np.random.default_rng(seed).integers(0, hi, (n, D)).astype(np.float32)


@case(["WS_PANEL_OUT:pvs_kmeans_step_dev", "WS_SCRATCH:launch_kmeans_step", "WS_LISTS:launch_assign"])
def kmeans_step(r):
    import learn_numpy as ln
    n, K, D = 4200 * (2 if r.big else 1), 40, 100
    x = _train_lattice(61, n, D)
    C = x[np.random.default_rng(62).permutation(n)[:K]].copy()
    cb = r.own(r.ctx.codebook(C))
    d_x, d_lab, d_sq = r.up(x), r.out("labels", (n,), np.int32), r.out("sqdist", (n,), np.float32)
    resid, counts, inertia, changed = r.ctx.kmeans_step_dev(cb, d_x.ptr, n, d_lab.ptr, None, d_sq.ptr)
    r.put("resid", resid), r.put("counts", counts), r.put("scalars", np.array([inertia, changed], np.float64))

    def check(res):
        labels, rs, cn, sq, ine, ch = ln.lloyd_stats(x, C)
        assert np.array_equal(res["labels"], labels) and np.array_equal(res["counts"], cn) and np.array_equal(res["resid"], rs)
        assert np.array_equal(res["sqdist"].astype(np.float64), sq) and res["scalars"][0] == ine
    r.expect(check)


@case(["WS_PANEL_OUT:pvs_label_sums_dev", "WS_PROJECTED:launch_label_sums", "WS_SCRATCH:launch_label_sums", "WS_AUX_ROWS:launch_label_sums"])
def label_sums_squared(r):
    import learn_numpy as ln
    n, K, D = 4100 * (2 if r.big else 1), 17, 30
    x = _train_lattice(63, n, D)
    labels = np.random.default_rng(64).integers(0, K, n).astype(np.int32)
    labels[labels == K // 2] = K - 1                           # a label that owns no row
    d_x, d_lab = r.up(x), r.up(labels)
    r.put("sums", r.ctx.label_sums_dev(d_x.ptr, D, n, d_lab.ptr, K, square=True))
    r.expect(lambda res: np.array_equal(res["sums"], ln.label_sums(x, labels, K, True)) or pytest.fail("label sums differ from the twin"))


@case(["WS_PANEL_OUT:pvs_gram_dev", "WS_AUX_ROWS:launch_gram", "WS_SCRATCH:launch_gram"])
def gram(r):
    import learn_numpy as ln
    n, D = 8193, 130 + (70 if r.big else 0)
    x = _train_lattice(65, n, D)
    s, g = r.ctx.gram_dev(r.up(x).ptr, D, n)
    r.put("sum", s), r.put("gram", g)
    r.expect(lambda res: (np.array_equal(res["sum"], ln.gram(x)[0]) and np.array_equal(res["gram"], ln.gram(x)[1]))
             or pytest.fail("the Gram matrix differs from the twin"))


@case(["WS_PANEL_OUT:pvs_gmm_em_step_dev", "WS_SCRATCH:launch_gmm_em_step"])
def gmm_em_step(r):
    import learn_numpy as ln
    from pvsim import learn
    g = load_golden("learn_k16_d32")
    n = 3000 * (2 if r.big else 1)
    x = np.ascontiguousarray(g["x_u8"][:n].astype(np.float32))
    w0, m0, c0 = g["g_w0"], g["g_m0"], 1.0 / g["g_p0"]
    gm = r.own(r.ctx.gmm(w0, m0, c0))
    s0, s1, s2, ll = r.ctx.gmm_em_step_dev(gm, r.up(x).ptr, n)
    r.put("s0", s0), r.put("s1", s1), r.put("s2", s2), r.put("ll", np.array([ll]))

    def check(res):
        nk, means, cov = learn._gmm_params_from_moments(res["s0"], res["s1"], res["s2"], 1e-6)
        r0, r1, r2, ll_ref = ln.em_stats(x, w0, m0, c0)
        w_ref, means_ref, cov_ref = ln.m_step(r0, r1, r2, n)
        w = nk / n
        np.testing.assert_allclose(w / w.sum(), w_ref, rtol=1e-9, atol=1e-13)
        np.testing.assert_allclose(means, means_ref, rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(cov, cov_ref, rtol=1e-9, atol=1e-11)
        assert abs(res["ll"][0] - ll_ref) / n < 1e-9
    r.expect(check)


def _seeding(r, stepwise):
    import learn_numpy as ln
    from pvsim import learn
    n, D, K = 4097 * (2 if r.big else 1), 30, 5
    x = _train_lattice(66, n, D)
    rows = learn.DeviceRows(r.ctx, n, D, r.up(x))
    centers, idx = learn.kmeans_plusplus(rows, K, random_state=7, stepwise=stepwise)
    r.put("indices", idx), r.put("centers", centers)

    def check(res):
        rs = np.random.RandomState(7)
        first = rs.randint(n)
        want, _ = ln.kmeanspp(x, K, first, rs.uniform(size=(K - 1, 2 + int(np.log(K)))))
        assert np.array_equal(res["indices"], want) and np.array_equal(res["centers"], x[want])
    r.expect(check)


@case(["WS_PROJECTED:pvs_kmeanspp_run_dev", "WS_SCRATCH:launch_kmeanspp_run"])
def kmeanspp_run(r):
    _seeding(r, stepwise=False)


@case(["WS_PANEL_OUT:pvs_seed_distances_dev", "WS_SCRATCH:launch_seed_distances", "WS_PANEL_OUT:pvs_seed_pick_dev",
       "WS_PANEL_OUT:pvs_min_update_dev"])
def kmeanspp_stepwise(r):
    _seeding(r, stepwise=True)


@case(["WS_LISTS:pvs_kmeans_topm_dev"])
def assign_topm_split(r):
    """K = 1000 is four blocks of 256 centroids: three splits leave partial lists in WS_LISTS"""
    import asmk_ma_numpy as ma
    rng = np.random.RandomState(2310)
    n, K, D, m = 700 * (2 if r.big else 1), 1000, 20, 5
    x, cent = rng.randint(-8, 9, (n, D)).astype(np.float32), (rng.randint(-16, 17, (K, D)) / 2.0).astype(np.float32)
    cb = r.own(r.ctx.codebook(cent))
    d_lab, d_val = r.out("labels", (n, m), np.int32), r.out("values", (n, m), np.float32)
    r.ctx.kmeans_topm_dev(cb, r.up(x).ptr, DESC_F32, n, m, d_lab.ptr, d_val.ptr, splits=3)

    def check(res):
        lab, v = ma.topm(x, cent, m)
        assert np.array_equal(res["labels"], lab) and np.array_equal(_bits(res["values"]), _bits(v.astype(np.float32)))
    r.expect(check)


# ====================================================================================================================== threshold join
@case(["WS_PROJECTED:pvs_cosine_range_dev", "WS_FP16_ROWS:pvs_cosine_range_dev", "WS_LISTS:pvs_cosine_range_dev",
       "WS_PANEL_OUT:pvs_cosine_range_dev"])
def range_join_filtered(r):
    """1024 query rows: the row count from which the join takes the prefilter on its own (path 0)"""
    import range_numpy as rn
    nq, N, L, t = 1024, 90 * (3 if r.big else 1), 16, np.float32(0.5)
    q, x = rn.lattice(nq, L, 71), rn.lattice(N, L, 72)
    S = rn.lattice_scores(q, x)
    want = rn.hits(S, t)
    cap = want[0].size + 8
    d_q, d_x = r.up(q), r.up(x)
    d_iq, d_ix = _inv_norms(r, d_q, nq, L), _inv_norms(r, d_x, N, L)
    outs = [r.out("row", (cap,), np.int64), r.out("col", (cap,), np.int64), r.out("val", (cap,), np.float32)]
    total, st = r.ctx.cosine_range_dev(d_q.ptr, nq, d_x.ptr, N, L, d_iq.ptr, d_ix.ptr, t, cap, *(o.ptr for o in outs), path=0)
    r.put("total", np.array([total])), r.put("stats", st)

    def check(res):
        assert st["filtered"] and total == want[0].size > 100, (st, total)
        m = want[0].size
        assert np.array_equal(res["row"][:m], want[0]) and np.array_equal(res["col"][:m], want[1])
        assert np.array_equal(_bits(res["val"][:m]), _bits(want[2]))
        assert (res["row"][m:].view(np.uint8) == FILL_OUT).all()
    r.expect(check)


@case(["WS_LISTS:pvs_pair_components_dev"], grow="knn_f32")
def pair_components(r):
    import range_numpy as rn
    n = 5000 * (2 if r.big else 1)
    rng = np.random.default_rng(8)
    a, b = rng.integers(0, n, 3000), rng.integers(0, n, 3000)
    d_lab = r.out("labels", (n,), np.int32)
    st = r.ctx.pair_components_dev(r.up(a.astype(np.int64)).ptr, r.up(b.astype(np.int64)).ptr, a.size, n, d_lab.ptr)
    # `rounds` is left out: the hooks of one round run concurrently, and how many rounds the fixed point takes depends on how they
    # interleave, not on the inputs alone (tests/test_gpu_range.py bounds it); the labels and the component count are functions of them
    r.put("components", np.array([st["components"]]))
    r.expect(lambda res: 1 <= st["rounds"] <= n + 1 or pytest.fail(str(st)))
    r.expect(lambda res: np.array_equal(res["labels"], rn.union_find_labels(n, a, b)) or pytest.fail("components differ from the twin"))


# ====================================================================================================================== score panels of the other rankers
def _int_codes(seed, n, L):
    """int8 code rows (n, 64 ceil(L / 64)), zero padded, and their factors"""
    import sq8_numpy as sq
    codes = np.zeros((n, sq.ld_of(L)), np.int8)
    codes[:, :L] = np.random.default_rng(seed).integers(-127, 128, (n, L))
    return codes, sq.factors(codes)


@case(["WS_PANEL_OUT:pvs_pq_scan_topk_dev"])
def pq_scan(r):
    import pq_numpy as pq
    rng = np.random.default_rng(81)
    nq, m, ksub, N, k = 6, 16, 256, 3000 * (2 if r.big else 1), 10
    table = rng.standard_normal((nq, m, ksub)).astype(np.float32)
    codes = rng.integers(0, ksub, (N, m)).astype(np.uint8)
    inv_q, inv_db = (0.5 + rng.random(nq)).astype(np.float32), (0.5 + rng.random(N)).astype(np.float32)
    d_idx, d_val = r.out("idx", (nq, k), np.int64), r.out("val", (nq, k), np.float32)
    r.ctx.pq_scan_topk_dev(r.up(table).ptr, nq, m, ksub, r.up(codes).ptr, N, r.up(inv_q).ptr, r.up(inv_db).ptr, k, 0, False, d_idx.ptr,
                           d_val.ptr)

    def check(res):
        wi, wv = pq.topk(pq.scores(table, codes, inv_q, inv_db), k)
        assert np.array_equal(res["idx"], wi) and np.array_equal(_bits(res["val"]), _bits(wv))
    r.expect(check)


@case(["WS_PANEL_OUT:pvs_sq8_topk_dev"])
def sq8_topk(r):
    import sq8_numpy as sq
    nq, N, L, k = 33, 1000 * (2 if r.big else 1), 65, 17
    (qc, iq), (dc, idb) = _int_codes(82, nq, L), _int_codes(83, N, L)
    dc[N - 1], dc[2] = dc[0], dc[1]                             # exact ties, decided by the index
    idb = sq.factors(dc)
    d_idx, d_val = r.out("idx", (nq, k), np.int64), r.out("val", (nq, k), np.float32)
    r.ctx.sq8_topk_dev(r.up(qc).ptr, r.up(iq).ptr, nq, r.up(dc).ptr, r.up(idb).ptr, N, L, k, 0, False, d_idx.ptr, d_val.ptr)

    def check(res):
        wi, wv = sq.topk(sq.scores(qc, iq, dc, idb), k)
        assert np.array_equal(res["idx"], wi) and np.array_equal(_bits(res["val"]), _bits(wv))
    r.expect(check)


def _subset_ids(N):
    return np.arange(0, N, 2, dtype=np.int64)


@case(["WS_PROJECTED:pvs_cosine_topk_subset_dev", "WS_PANEL_OUT:pvs_cosine_topk_subset_dev"])
def subset_f32_listed(r):
    """the listed path: the allowed rows are gathered chunk by chunk into WS_PROJECTED (tile 48: several chunks)"""
    import range_numpy as rn
    import subset_numpy as sn
    nq, N, L, k = 130, 200 * (3 if r.big else 1), 64, 16
    q, x = rn.lattice(nq, L, 2), rn.lattice(N, L, 1)
    ids = _subset_ids(N)
    d_q, d_x = r.up(q), r.up(x)
    d_iq, d_ix = _inv_norms(r, d_q, nq, L), _inv_norms(r, d_x, N, L)
    handle = r.own(r.ctx.subset_create(ids, N))
    d_idx, d_val = r.out("idx", (nq, k), np.int64), r.out("val", (nq, k), np.float32)
    st = r.ctx.cosine_topk_subset_dev(d_q.ptr, nq, d_x.ptr, N, L, d_iq.ptr, d_ix.ptr, handle, k, d_idx.ptr, d_val.ptr, path=2, tile=48)
    r.put("stats", st)

    def check(res):
        assert st["path"] == "listed" and st["rows_gathered"] >= ids.size, st
        wi, wv = sn.restricted_topk(rn.lattice_scores(q, x), ids, k)
        assert np.array_equal(res["idx"], wi) and np.array_equal(_bits(res["val"]), _bits(wv))
    r.expect(check)


@case(["WS_PROJECTED:pvs_sq8_topk_subset_dev", "WS_PANEL_OUT:pvs_sq8_topk_subset_dev"])
def subset_sq8_listed(r):
    import sq8_numpy as sq
    import subset_numpy as sn
    nq, N, L, k = 130, 200 * (3 if r.big else 1), 65, 16
    (qc, iq), (dc, idb) = _int_codes(84, nq, L), _int_codes(85, N, L)
    ids = _subset_ids(N)
    handle = r.own(r.ctx.subset_create(ids, N))
    d_idx, d_val = r.out("idx", (nq, k), np.int64), r.out("val", (nq, k), np.float32)
    st = r.ctx.sq8_topk_subset_dev(r.up(qc).ptr, r.up(iq).ptr, nq, r.up(dc).ptr, r.up(idb).ptr, N, L, handle, k, d_idx.ptr, d_val.ptr,
                                   path=2, tile=48)
    r.put("stats", st)

    def check(res):
        assert st["path"] == "listed" and st["rows_gathered"] >= ids.size, st
        wi, wv = sn.restricted_topk(sq.scores(qc, iq, dc, idb), ids, k)
        assert np.array_equal(res["idx"], wi) and np.array_equal(_bits(res["val"]), _bits(wv))
    r.expect(check)


# ====================================================================================================================== probed scans
def _two_long_lists(N):
    """N rows in two lists, every 41st row in list 1: with both probed a candidate row has 64 ceil(N / 64) slots"""
    import ivf_numpy as iv
    lists = np.zeros(N, np.int64)
    lists[::41] = 1
    return iv.sort_into_lists(lists, 2)


@case(["WS_IVF_CANDIDATES:pvs_ivf_scan_topk_dev"], capped=["WS_IVF_CANDIDATES"])
def ivf_scan_two_query_blocks(r):
    """16448 slots per query: the 64 MiB of candidate rows hold 510 queries, 600 queries are two blocks"""
    import ivf_numpy as iv
    N, nlist, m, ksub, nq, k, nprobe = 16400, 2, 4, 16, 600, 10, 2
    rng = np.random.default_rng(1300)
    table = rng.standard_normal((nq, m, ksub)).astype(np.float32)
    co = rng.standard_normal((nq, nlist)).astype(np.float32)
    ids, off = _two_long_lists(N)
    assert (64 << 20) // (8 * (-(-N // 64) * 64)) < nq
    codes = rng.integers(0, ksub, (N, m)).astype(np.uint8)
    inv_db = (0.5 + rng.random(N)).astype(np.float32)
    d_co, d_pi, d_pv = r.up(co), r.out("probe", (nq, nprobe), np.int64), r.out("probe_val", (nq, nprobe), np.float32)
    d_idx, d_val = r.out("idx", (nq, k), np.int64), r.out("val", (nq, k), np.float32)
    r.ctx.topk_dev(d_co.ptr, nq, nlist, nlist, nprobe, 0, False, d_pi.ptr, d_pv.ptr)
    r.ctx.ivf_scan_topk_dev(r.up(table).ptr, nq, m, ksub, d_pi.ptr, d_pv.ptr, nprobe, r.up(off).ptr, off, nlist, r.up(codes).ptr,
                            r.up(ids).ptr, None, r.up(inv_db).ptr, k, d_idx.ptr, d_val.ptr)

    def check(res):
        wi, wv = iv.search(table, co, nprobe, off, ids, codes, None, inv_db, k)
        assert np.array_equal(res["idx"], wi) and np.array_equal(_bits(res["val"]), _bits(wv))
    r.expect(check)


def _sq8_lists_case(r, nq, N, L, nlist, lists, nprobe, seed):
    import ivf_sq8_numpy as tw
    (qc, iq), (dc, idb) = _int_codes(seed, nq, L), _int_codes(seed + 1, N, L)
    ids, off = tw.sort_into_lists(lists, nlist)
    rng = np.random.default_rng(seed + 2)
    probe = np.stack([rng.permutation(nlist)[:nprobe] for _ in range(nq)]).astype(np.int64)
    stored = (np.ascontiguousarray(dc[ids]), np.ascontiguousarray(idb[ids]), ids, off)
    return qc, iq, probe, stored


def _expect_sq8_search(r, qc, iq, probe, stored, k):
    import ivf_sq8_numpy as tw

    def check(res):
        wi, wv = tw.search(qc, iq, probe, stored[3], stored[0], stored[1], stored[2], k)
        assert np.array_equal(res["idx"], wi) and np.array_equal(_bits(res["val"]), _bits(wv))
    r.expect(check)


@case(["WS_IVF_CANDIDATES:pvs_ivf_sq8_scan_topk_dev"], capped=["WS_IVF_CANDIDATES"])
def ivf_sq8_scan_two_query_blocks(r):
    N, nq, L, k = 16400, 600, 8, 10
    lists = np.zeros(N, np.int64)
    lists[::41] = 1
    qc, iq, probe, stored = _sq8_lists_case(r, nq, N, L, 2, lists, 2, 90)
    d_idx, d_val = r.out("idx", (nq, k), np.int64), r.out("val", (nq, k), np.float32)
    plan = r.ctx.ivf_sq8_scan_plan(nq, 2, stored[3], 2)
    r.ctx.ivf_sq8_scan_topk_dev(r.up(qc).ptr, r.up(iq).ptr, nq, L, r.up(probe).ptr, 2, r.up(stored[3]).ptr, stored[3], 2, r.up(stored[0]).ptr,
                                r.up(stored[1]).ptr, r.up(stored[2]).ptr, k, d_idx.ptr, d_val.ptr)
    r.expect(lambda res: plan["query_block"] < nq or pytest.fail(f"one query block: {plan}"))
    _expect_sq8_search(r, qc, iq, probe, stored, k)


@case(["WS_IVF_CANDIDATES:pvs_ivf_sq8_scan_lists_topk_dev", "WS_UPDATE:pvs_ivf_sq8_scan_lists_topk_dev"])
def ivf_sq8_scan_lists_three_query_blocks(r):
    """257 queries grouped 128 at a time: three query blocks share the candidate rows and the grouping block"""
    N, nq, L, nlist, nprobe, k = 1000 * (2 if r.big else 1), 257, 65, 7, 3, 17
    lists = np.random.default_rng(93).integers(0, nlist - 1, N)                    # the last list stays empty
    qc, iq, probe, stored = _sq8_lists_case(r, nq, N, L, nlist, lists, nprobe, 94)
    d_idx, d_val = r.out("idx", (nq, k), np.int64), r.out("val", (nq, k), np.float32)
    plan = r.ctx.ivf_sq8_scan_lists_plan(nq, nprobe, stored[3], nlist, 128)
    r.ctx.ivf_sq8_scan_lists_topk_dev(r.up(qc).ptr, r.up(iq).ptr, nq, L, r.up(probe).ptr, nprobe, r.up(stored[3]).ptr, stored[3], nlist,
                                      r.up(stored[0]).ptr, r.up(stored[1]).ptr, r.up(stored[2]).ptr, k, d_idx.ptr, d_val.ptr, query_block=128)
    r.expect(lambda res: plan["query_block"] == 128 or pytest.fail(f"not three query blocks: {plan}"))
    _expect_sq8_search(r, qc, iq, probe, stored, k)


@case(["WS_UPDATE:pvs_ivf_sq8_group_probes_dev"])
def ivf_sq8_group_probes(r):
    import ivf_sq8_lists_numpy as lt
    import ivf_sq8_numpy as tw
    nq, nlist, nprobe, N = 130 * (3 if r.big else 1), 64, 2, 700
    rng = np.random.default_rng(95)
    lists = rng.integers(0, nlist, N)
    lists[lists % 3 == 1] = 0
    list_off = tw.sort_into_lists(lists, nlist)[1]
    probe = np.stack([rng.permutation(nlist)[:nprobe] for _ in range(nq)]).astype(np.int64)
    probe[3, 1], probe[7, 0] = -1, nlist                        # probes outside [0, nlist): no pair
    sizes = (nq * nprobe, nq, nlist + 1, nq * nprobe, nq * nprobe)
    outs = [r.out(name, (n,), np.int32) for name, n in zip(("base", "total", "goff", "gq", "gbase"), sizes)]
    r.ctx.ivf_sq8_group_probes_dev(r.up(probe).ptr, nq, nprobe, r.up(list_off).ptr, nlist, *(o.ptr for o in outs))

    def check(res):
        base, total, goff, gq, gbase = lt.group_probes(probe, list_off)
        P = int(goff[nlist])
        assert np.array_equal(res["total"], total) and np.array_equal(res["goff"], goff)
        assert np.array_equal(res["gq"][:P], gq) and np.array_equal(res["gbase"][:P], gbase)
        live = ((probe >= 0) & (probe < nlist)).reshape(-1)
        assert np.array_equal(res["base"][live], np.asarray(base).reshape(-1)[live])
    r.expect(check)


# ====================================================================================================================== maintenance
def _random_keep(seed, n, share=0.6):
    return (np.random.default_rng(seed).random(n) < share).astype(np.uint8)


@case(["WS_UPDATE:pvs_keep_positions_dev"])
def keep_positions(r):
    import update_numpy as up
    n = (3 if not r.big else 9) * up.SCAN_TILE + 5
    keep = _random_keep(101, n)
    d_pos = r.out("pos", (n + 1,), np.int64)
    r.ctx.keep_positions_dev(r.up(keep).ptr, n, d_pos.ptr)
    r.expect(lambda res: np.array_equal(res["pos"], up.keep_positions(keep)) or pytest.fail("positions differ from the twin"))


@case(["WS_UPDATE:pvs_compact_rows_dev"])
def compact_rows_in_place(r):
    """in place, windows of 64 rows: the kept rows of every window are staged in WS_UPDATE"""
    import update_numpy as up
    from pvsim import _ffi
    n, rb = 301 * (3 if r.big else 1), 24
    rows = np.random.default_rng(102).integers(0, 256, (n, rb)).astype(np.uint8)
    keep = _random_keep(103, n)
    keep[:5] = 1
    pos = up.keep_positions(keep)
    first = int(np.flatnonzero(keep == 0)[0])
    d_rows = r.out("rows", (n + 2, rb), np.uint8)
    d_rows.upload(rows)
    with r.ctx.option(_ffi.OPT_UPDATE_WINDOW_ROWS, 64):
        r.ctx.compact_rows_dev(d_rows.ptr, n, rb, r.up(keep).ptr, r.up(pos).ptr, d_rows.ptr, first=first)

    def check(res):
        kept = int(pos[-1])
        assert np.array_equal(res["rows"][:kept], up.compact_rows(rows, keep, pos))
        assert (res["rows"][n:] == FILL_OUT).all()
    r.expect(check)


def _stored_lists(seed, n, nlist, m):
    from pvsim.compact import _sort_into_lists
    rng = np.random.default_rng(seed)
    lists = rng.integers(0, nlist, n)
    codes, inv = rng.integers(0, 256, (n, m)).astype(np.uint8), rng.random(n).astype(np.float32)
    ids, off = _sort_into_lists(lists.astype(np.int64), nlist)
    return np.ascontiguousarray(codes[ids]), np.ascontiguousarray(inv[ids]), ids, off


@case(["WS_UPDATE:pvs_ivf_insert_dev"])
def ivf_insert(r):
    import update_numpy as up
    nlist, m, n, b = 7, 8, 150 * (3 if r.big else 1), 40 * (3 if r.big else 1)
    codes, inv, ids, off = _stored_lists(104, n, nlist, m)
    rng = np.random.default_rng(105)
    new_codes, new_inv = rng.integers(0, 256, (b, m)).astype(np.uint8), rng.random(b).astype(np.float32)
    perm, new_off = up.sort_new_rows(rng.integers(0, nlist, b), nlist)
    ins = [r.up(a) for a in (codes, inv, ids, off, new_codes, new_inv, new_off, perm)]
    outs = [r.out("codes", (n + b, m), np.uint8), r.out("inv", (n + b,), np.float32), r.out("ids", (n + b,), np.int32),
            r.out("list_off", (nlist + 1,), np.int64)]
    r.ctx.ivf_insert_dev(m, nlist, ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, off, ins[4].ptr, ins[5].ptr, ins[6].ptr, new_off,
                         ins[7].ptr, *(o.ptr for o in outs))

    def check(res):
        want = up.ivf_insert(codes, inv, ids, off, new_codes, new_inv, new_off, perm)
        for key, w in zip(("codes", "inv", "ids", "list_off"), want):
            assert np.array_equal(_bits(res[key]), _bits(w)), key
    r.expect(check)


@case(["WS_UPDATE:pvs_ivf_remove_dev"])
def ivf_remove(r):
    import update_numpy as up
    nlist, m, n = 7, 8, 150 * (3 if r.big else 1)
    codes, inv, ids, off = _stored_lists(106, n, nlist, m)
    keep = _random_keep(107, n)
    left = int((keep != 0).sum())
    ins = [r.up(a) for a in (codes, inv, ids, off, keep, up.keep_positions(keep))]
    outs = [r.out("codes", (left, m), np.uint8), r.out("inv", (left,), np.float32), r.out("ids", (left,), np.int32),
            r.out("list_off", (nlist + 1,), np.int64)]
    r.ctx.ivf_remove_dev(m, nlist, n, *(x.ptr for x in ins), *(o.ptr for o in outs))

    def check(res):
        for key, w in zip(("codes", "inv", "ids", "list_off"), up.ivf_remove(codes, inv, ids, off, keep)):
            assert np.array_equal(_bits(res[key]), _bits(w)), key
    r.expect(check)


# ====================================================================================================================== ASMK
def _asmk_slots(seed, E, K, W):
    import asmk_update_numpy as au
    return au.make_slots(np.random.RandomState(seed), 40, E, K, W, "shared")


@case(["WS_UPDATE:pvs_asmk_invert_dev"])
def asmk_invert(r):
    import asmk_update_numpy as au
    E, K, W, img_base, tile = 1000 * (3 if r.big else 1), 257, 2, 1000, 256
    off, count, word, sig, _ = _asmk_slots(1901, E, K, W)
    n, total = len(off) - 1, int(off[-1])
    outs = [r.out("word_off", (K + 1,), np.int64), r.out("img", (total,), np.int32), r.out("sig", (total, W), np.uint32)]
    r.ctx.asmk_invert_dev(K, 32 * W, r.up(off).ptr, off, n, r.up(count).ptr, r.up(word).ptr, r.up(sig).ptr, img_base, outs[0].ptr,
                          outs[1].ptr, outs[2].ptr, tile)

    def check(res):
        want = au.invert(off, count, word, sig, K, img_base, tile)
        assert int(want[0][K]) == E and total > 3 * 256
        assert np.array_equal(res["word_off"], want[0]) and np.array_equal(res["img"][:E], want[1]) and np.array_equal(res["sig"][:E], want[2])
        assert (res["img"][E:].view(np.uint8) == FILL_OUT).all()
    r.expect(check)


def _asmk_file(seed, N, E, K, W):
    """-> (per-image entries, the inverted file of them by the twin: word_off, ent_img, ent_sig)"""
    import asmk_update_numpy as au
    ents = au.make_slots(np.random.RandomState(seed), N, E, K, W, "random")[4]
    off = np.zeros(len(ents) + 1, np.int64)
    np.cumsum([len(e[0]) for e in ents], out=off[1:])
    word = np.concatenate([e[0] for e in ents]).astype(np.int32)
    sig = np.concatenate([e[1].reshape(-1, W) for e in ents]).astype(np.uint32)
    return ents, au.invert(off, np.diff(off).astype(np.int32), word, sig, K)


@case(["WS_UPDATE:pvs_asmk_remove_dev"])
def asmk_remove(r):
    import asmk_update_numpy as au
    N, E, K, W = 200, 4000 * (3 if r.big else 1), 300, 2
    _, (word_off, img, sig) = _asmk_file(1902, N, E, K, W)
    keep = _random_keep(108, N, 0.7)
    pos = au.keep_positions(keep)
    outs = [r.out("word_off", (K + 1,), np.int64), r.out("img", (E,), np.int32), r.out("sig", (E, W), np.uint32)]
    r.ctx.asmk_remove_dev(K, 32 * W, N, r.up(word_off).ptr, word_off, r.up(img).ptr, r.up(sig).ptr, r.up(keep).ptr, r.up(pos).ptr,
                          outs[0].ptr, outs[1].ptr, outs[2].ptr)

    def check(res):
        want = au.remove(word_off, img, sig, keep, pos)
        left = len(want[1])
        assert 0 < left < E
        assert np.array_equal(res["word_off"], want[0]) and np.array_equal(res["img"][:left], want[1]) and np.array_equal(res["sig"][:left], want[2])
    r.expect(check)


@case(["WS_UPDATE:pvs_asmk_expand_dev"])
def asmk_expand_two_query_blocks(r):
    """130 queries: a block of 128 and one of 2 share the hit masks and chunk counts"""
    import asmk_expand_numpy as xt
    N, E, K, W, R, nq = 200, 4000, 257 * (3 if r.big else 1), 1, 10, 130
    ents, host = _asmk_file(1903, N, E, K, W)
    rng = np.random.RandomState(1904)
    wt = rng.randint(0, 1024, K).astype(np.int32)
    queries = []
    for q in range(nq):
        w = np.sort(rng.permutation(K)[:rng.randint(0, 9)]).astype(np.int32)
        queries.append((w, rng.randint(0, 1 << 32, (len(w), W), dtype=np.uint64).astype(np.uint32)))
    members = np.full((nq, R), -1, np.int32)
    for q in range(nq):
        ids = np.sort(rng.permutation(N)[:rng.randint(0, R + 1)])
        members[q, :len(ids)] = ids
    votes = (members >= 0).astype(np.int32)
    q_off = np.zeros(nq + 1, np.int64)
    np.cumsum([len(w) for w, _ in queries], out=q_off[1:])
    q_word = np.concatenate([w for w, _ in queries]).astype(np.int32)
    q_sig = np.concatenate([s.reshape(-1, W) for _, s in queries]).astype(np.uint32)
    query_vote, h_max, min_support = 2, 32 * W // 4, 1
    want, counts, sums = xt.expand(queries, *host, members, votes, query_vote, h_max, min_support, wt)
    cap = int(counts.max(initial=0)) + 3
    outs = [r.out("word", (nq, cap), np.int32), r.out("sig", (nq, cap, W), np.uint32), r.out("count", (nq,), np.int32),
            r.out("sum", (nq,), np.int64)]
    r.ctx.asmk_expand_dev(nq, q_off, r.up(q_word).ptr, r.up(q_sig).ptr, 32 * W, K, r.up(host[0]).ptr, r.up(host[1]).ptr, r.up(host[2]).ptr,
                          N, R, r.up(members).ptr, r.up(votes).ptr, query_vote, h_max, min_support, r.up(wt).ptr, cap, outs[0].ptr,
                          outs[1].ptr, outs[2].ptr, outs[3].ptr, 0)

    def check(res):
        assert np.array_equal(res["count"], counts) and np.array_equal(res["sum"], sums) and counts[128:].max() > 0
        for q in range(nq):
            c = int(counts[q])
            assert np.array_equal(res["word"][q, :c], want[q][0]) and np.array_equal(res["sig"][q, :c], want[q][1].reshape(-1, W)), q
            assert (res["word"][q, c:].view(np.uint8) == FILL_OUT).all(), q
    r.expect(check)


# ====================================================================================================================== SIFT front ends
def _keep_buffers(r, *bufs):
    r._bufs.extend(b for b in bufs if b is not None)


@case(["WS_DSIFT_TABLE:pvs_dsift_dev"])
def dense_sift(r):
    import dsift_numpy as tw
    from pvsim.features import DenseSIFT
    sizes, step = (4, 8), 16
    images = [tw.inputs()["rect"]] + ([tw.inputs()["small"], tw.inputs()["rect"]] if r.big else [])
    fx = DenseSIFT(step=step, sizes=sizes, ctx=r.ctx)
    rows, offs, n, total, _, h_off = fx.device_descriptors(images, r.ctx, 2)                    # DSIFT_F32_RAW
    _keep_buffers(r, rows, offs)
    r.put("raw", rows.download((total, 128), np.float32)), r.put("offsets", offs.download((n + 1,), np.int64))

    def check(res):
        t64, _ = tw.twin_pair("rect", sizes, step)
        _, e_raw = tw.yardsticks()
        top = float(np.abs(t64.raw).max())
        assert res["raw"].shape == t64.raw.shape and top > 0
        assert float(np.abs(res["raw"].astype(np.float64) - t64.raw).max()) / top <= 8 * e_raw
    r.expect(check)


@case(["WS_SIFT_PYRAMID:pvs_sift_dev", "WS_SIFT_TABLES:pvs_sift_dev", "WS_SIFT_KEYPOINTS:pvs_sift_dev"])
def keypoint_sift(r):
    import sift_numpy as tw
    from pvsim.features import KeypointSIFT
    images = [tw.inputs()["tex_gray"]] + ([np.tile(tw.inputs()["tex_gray"], (2, 1))] if r.big else [])
    fx = KeypointSIFT(ctx=r.ctx)
    rows, offs, n, total, _, h_off, frm = fx.device_descriptors(images, r.ctx, 1, frames=True)  # float32 rows
    _keep_buffers(r, rows, offs, frm)
    r.put("rows", rows.download((total, 128), np.float32)), r.put("frames", frm.download((total, 6), np.float32))
    r.put("offsets", offs.download((n + 1,), np.int64))

    def check(res):
        e, t = tw.yardsticks(), tw.twin64("tex_gray")
        idx, dev = tw.match_frames(t, res["frames"])
        m = idx >= 0
        only_dev = [j for j in np.nonzero(~m)[0] if not tw.frame_excused(t, res["frames"][j])]
        matched = set(idx[m].tolist())
        only_twin = [j for j in range(len(t.rows)) if j not in matched and not tw.row_excused(t, j)]
        assert not only_dev and not only_twin and m.sum() > 50
        assert float(np.abs(res["rows"][m].astype(np.float64) - t.v[idx[m]]).max()) <= 8 * e["desc"]
    r.expect(check)


# ====================================================================================================================== spatial verification
def _csr(parts):
    off = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=off[1:])
    return off


def _match_sets(big):
    import match_numpy as tw
    sizes = (33, 257, 700) + ((700, 513) if big else ())
    pa = [tw.planted_rows(n, 100 + k) for k, n in enumerate(sizes)]
    pb = [tw.planted_rows(n, 200 + k) for k, n in enumerate(sizes)]
    for k in range(len(sizes)):                                 # a row of A planted twice in B: an exact tie, the lowest index wins
        pb[k][2], pb[k][9] = pa[k][4], pa[k][4]
    pairs = np.array([(ia, ib) for ia in range(len(sizes)) for ib in range(len(sizes))], np.int32)
    return pa, pb, pairs


@case(["WS_MATCH_TABLE:pvs_match_u8_dev"])
def match_rows(r):
    import match_numpy as tw
    pa, pb, pairs = _match_sets(r.big)
    rows_a, rows_b, off_a, off_b = np.concatenate(pa), np.concatenate(pb), _csr(pa), _csr(pb)
    total = int(sum(len(pa[ia]) for ia, _ in pairs))
    outs = [r.out(name, (total,), np.int32) for name in ("idx", "d1", "d2")]
    r.ctx.match_u8_dev(r.up(rows_a).ptr, off_a, r.up(rows_b).ptr, off_b, pairs, *(o.ptr for o in outs))

    def check(res):
        want = tw.match_pairs(rows_a, off_a, rows_b, off_b, pairs)
        assert all(np.array_equal(res[key], w) for key, w in zip(("idx", "d1", "d2"), want))
    r.expect(check)


@case(["WS_MATCH_TABLE:upload_pairs"])
def match_filter(r):
    import match_numpy as tw
    pa, pb, pairs = _match_sets(r.big)
    rows_a, rows_b, off_a, off_b = np.concatenate(pa), np.concatenate(pb), _csr(pa), _csr(pb)
    fwd = tw.match_pairs(rows_a, off_a, rows_b, off_b, pairs)
    rev = tw.match_pairs(rows_b, off_b, rows_a, off_a, pairs[:, ::-1])
    total, rsq = len(fwd[0]), tw.ratio_sq(0.9)
    d_m, d_c = r.out("matches", (total, 2), np.int32), r.out("counts", (len(pairs),), np.int32)
    r.ctx.match_filter_dev(off_a, off_b, pairs, r.up(fwd[0]).ptr, r.up(fwd[1]).ptr, r.up(fwd[2]).ptr, r.up(rev[0]).ptr, rsq, True, d_m.ptr, d_c.ptr)

    def check(res):
        oa = ob = kept = 0
        for p, (ia, ib) in enumerate(pairs):
            n_a, n_b = len(pa[ia]), len(pb[ib])
            want = tw.filter_matches(fwd[0][oa:oa + n_a], fwd[1][oa:oa + n_a], fwd[2][oa:oa + n_a], rev[0][ob:ob + n_b], rsq, True)
            assert res["counts"][p] == len(want) and np.array_equal(res["matches"][oa:oa + len(want)], want), p
            kept += len(want)
            oa, ob = oa + n_a, ob + n_b
        assert kept >= 3
    r.expect(check)


@case(["WS_VERIFY_POINTS:pvs_verify_dev", "WS_VERIFY_SMALL:pvs_verify_dev", "WS_MATCH_TABLE:upload_pairs"])
def verify_pairs(r):
    import match_numpy as tw
    cases = [tw.planted_matches(5, 0.0, 1)[:3], tw.planted_matches(64, 0.0, 3)[:3], tw.planted_matches(300, 0.5, 6)[:3]]
    if r.big:
        cases += [tw.planted_matches(300, 0.4, 5)[:3], tw.planted_matches(300, 0.5, 6)[:3]]
    off_a, off_b = _csr([c[0] for c in cases]), _csr([c[1] for c in cases])
    n, total = len(cases), int(off_a[-1])
    pairs = np.array([(k, k) for k in range(n)], np.int32)
    matches = np.full((total, 2), -7, np.int32)
    for k, c in enumerate(cases):
        matches[off_a[k]:off_a[k] + len(c[2])] = c[2]
    counts = np.array([len(c[2]) for c in cases], np.int32)
    outs = [r.out("inliers", (n,), np.int32), r.out("models", (n, 2, 3), np.float64), r.out("best", (n,), np.int32),
            r.out("mask", (total,), np.uint8)]
    r.ctx.verify_dev(r.up(np.concatenate([c[0] for c in cases])).ptr, off_a, r.up(np.concatenate([c[1] for c in cases])).ptr, off_b, pairs,
                     r.up(matches).ptr, r.up(counts).ptr, tw.DEFAULT_TOL, 2, *(o.ptr for o in outs))

    def check(res):
        for k, c in enumerate(cases):
            m, lo = len(c[2]), int(off_a[k])
            t0, t2 = tw.verify(c[0], c[1], c[2], tw.DEFAULT_TOL, 0), tw.verify(c[0], c[1], c[2], tw.DEFAULT_TOL, 2)
            assert not t0.band.any() and not t2.final_band.any(), k      # a condition of the exact comparison: holds on these inputs
            mask = res["mask"][lo:lo + m].astype(bool)
            assert res["best"][k] == t0.best and res["inliers"][k] == t2.inliers == mask.sum() and np.array_equal(mask, t2.mask), k
            ref = tw.model_2x3(*tw.fit(t2.pa, t2.pb, mask)) if t2.converged else t2.model
            assert float(np.abs(res["models"][k] - ref).max()) / max(1.0, float(np.abs(ref).max())) <= 1e-9, k
    r.expect(check)


# ====================================================================================================================== the sweep
NAMES = sorted(CASES)
SLOTS = ws_ledger.slot_names()
# for a block of a fixed size (statistics of K x D numbers, a handful of counters): the case whose big form makes the slot larger
GROWERS = {"WS_PANEL_OUT": "topk_host", "WS_UPDATE": "asmk_invert", "WS_PROJECTED": "kmeanspp_run", "WS_SCRATCH": "gram",
           "WS_LISTS": "knn_f32", "WS_AUX_ROWS": "cosine_host_f32"}


@pytest.mark.parametrize("name", NAMES)
def test_fresh_context_equals_the_twin(name):
    """every slot grows inside the call; the slots the case is there for were reserved; the result is the twin's"""
    res, ws, checks = fresh(name)
    for slot, fn in CASES[name].covers:
        assert ws[slot] > 0, f"{name} is listed for ({slot}, {fn}) but {slot} was never reserved: the path did not run"
    assert checks, f"{name} holds its result against nothing"
    for check in checks:
        check(res)


@pytest.mark.parametrize("name", NAMES)
def test_poisoned_slots_and_caches_give_the_same_bytes(name):
    import pvsim
    want, ws_fresh, _ = fresh(name)
    fn = CASES[name]
    ctx = pvsim.Context(0)
    try:
        execute(ctx, fn.grow or name, big=True, fetch=False)
        if fn.grow:
            execute(ctx, name, big=True, fetch=False)
        listed = {s for s, _ in fn.covers} - fn.capped
        for slot in sorted(listed):                             # a block whose size the big form does not change: another user of the slot
            if ctx.diag_ws_bytes()[slot] <= ws_fresh[slot]:
                execute(ctx, GROWERS[slot], big=True, fetch=False)
        ctx.sync()
        before = ctx.diag_ws_bytes()
        for slot in SLOTS:
            if ws_fresh[slot]:
                assert before[slot] >= ws_fresh[slot], f"{slot}: {before[slot]} bytes after the big form, the case needs {ws_fresh[slot]}"
                if slot in listed:
                    assert before[slot] > ws_fresh[slot], f"{slot} is no larger than the case itself makes it ({before[slot]} bytes)"
        for byte in POISON_BYTES:
            poison(ctx, byte)
            _, got = execute(ctx, name)
            same_bytes(got, want, f"{name} on memory filled with {byte:#04x}")
            assert ctx.diag_ws_bytes() == before, f"{name}: a slot grew again although it was large enough"
    finally:
        ctx.close()


# every pair: a case directly behind a case of another family that carves a shared slot with another layout
NEIGHBOURS = [
    ("filtered_topk", "knn_f32"), ("knn_f32", "range_join_filtered"), ("range_join_filtered", "vlad_host"), ("vlad_host", "filtered_topk"),
    ("knn_f64", "topk_f64_host"), ("topk_f64_host", "assign_topm_split"), ("assign_topm_split", "pair_components"), ("pair_components", "knn_f32"),
    ("ivf_insert", "asmk_invert"), ("asmk_invert", "ivf_sq8_scan_lists_three_query_blocks"), ("ivf_sq8_scan_lists_three_query_blocks", "ivf_remove"),
    ("asmk_expand_two_query_blocks", "keep_positions"), ("keep_positions", "asmk_remove"), ("asmk_remove", "compact_rows_in_place"),
    ("compact_rows_in_place", "ivf_sq8_group_probes"), ("ivf_sq8_group_probes", "asmk_expand_two_query_blocks"), ("ivf_remove", "ivf_insert"),
    ("vlad_host_pca", "kmeanspp_run"), ("kmeanspp_run", "subset_f32_listed"), ("subset_f32_listed", "label_sums_squared"),
    ("label_sums_squared", "filtered_topk_overflow"), ("filtered_topk_overflow", "subset_sq8_listed"), ("subset_sq8_listed", "vlad_host_pca"),
    ("fisher_host_pca", "range_join_filtered"), ("kmeanspp_run", "fisher_host_pca"), ("filtered_topk", "knn_f64"),
    ("kmeans_step", "topk_host"), ("topk_host", "gmm_em_step"), ("gmm_em_step", "gram"), ("gram", "cosine_host_f64"),
    ("cosine_host_f64", "fisher_host"), ("fisher_host", "kmeanspp_stepwise"), ("kmeanspp_stepwise", "gmm_posterior"),
    ("gmm_posterior", "vlad_dev_without_labels"), ("vlad_dev_without_labels", "kmeans_step"),
    ("cosine_host_f32", "fisher_host"), ("gram", "cosine_host_f32"),
    ("pq_scan", "sq8_topk"), ("sq8_topk", "radius_f32"), ("radius_f32", "topk_host_two_queries"), ("topk_host_two_queries", "pq_scan"),
    ("knn_f32_overflow", "radius_f32"), ("radius_f32", "knn_f32_overflow"),
    ("ivf_scan_two_query_blocks", "ivf_sq8_scan_lists_three_query_blocks"), ("ivf_sq8_scan_two_query_blocks", "ivf_scan_two_query_blocks"),
    ("ivf_sq8_scan_lists_three_query_blocks", "ivf_sq8_scan_two_query_blocks"),
    ("match_rows", "match_filter"), ("match_filter", "verify_pairs"), ("verify_pairs", "match_rows"),
    ("dense_sift", "keypoint_sift"), ("keypoint_sift", "dense_sift"),
]


def test_every_case_runs_behind_a_neighbour_that_shares_a_slot():
    """the table above is complete (every case is the second of a pair) and honest (the two share a slot and are different families)"""
    second = {b for _, b in NEIGHBOURS}
    assert second == set(NAMES), sorted(set(NAMES) ^ second)
    for a, b in NEIGHBOURS:
        assert a != b and a in CASES
        if {a, b} <= {"dense_sift", "keypoint_sift"}:
            continue                                            # each of the two front ends has its slots to itself: they only follow each other
        shared = {s for s, _ in CASES[a].covers} & {s for s, _ in CASES[b].covers}
        shared |= {s for s in SLOTS if fresh(a)[1][s] and fresh(b)[1][s]}
        assert shared, f"{a} and {b} share no workspace slot"


@pytest.mark.parametrize("first,name", NEIGHBOURS, ids=[f"{a}-then-{b}" for a, b in NEIGHBOURS])
def test_behind_a_neighbour_with_another_layout(first, name):
    import pvsim
    want, _, _ = fresh(name)
    ctx = pvsim.Context(0)
    try:
        execute(ctx, first, fetch=False)                        # nothing fetched, no sync, no poison: what it left is what the case finds
        _, got = execute(ctx, name)
        same_bytes(got, want, f"{name} directly behind {first}")
    finally:
        ctx.close()


# ====================================================================================================================== the table block cache
TABLE_CASES = ("vlad_host", "vlad_host_pca", "fisher_host", "fisher_host_pca")


def test_tables_built_in_recycled_blocks_give_the_same_bytes():
    """Tables filled with NaN and ordinary tables, of the shapes the cases create and of slightly larger ones, are created and
    destroyed: their blocks wait in the cache, an oversized one among them for every request (the cache hands out a block of up to
    twice the size asked for).  The blocks are filled with 0xFF as well.  The real tables are then built in them."""
    import pvsim
    t = load_golden("tables_k256_d128")
    want = {name: fresh(name)[0] for name in TABLE_CASES}
    ctx = pvsim.Context(0)
    try:
        rng = np.random.default_rng(7)
        for fill in (np.nan, None):
            made = []
            for K in (256, 272):
                c = np.full((K, 128), fill, np.float32) if fill is not None else rng.standard_normal((K, 128)).astype(np.float32)
                made.append(ctx.codebook(c))
                made.append(ctx.codebook(c[:, :64].copy()))
            for K, D in ((256, 128), (264, 128), (64, 64), (72, 64)):
                m = np.full((K, D), fill, np.float64) if fill is not None else rng.standard_normal((K, D))
                made.append(ctx.gmm(np.full(K, 1.0 / K), m, np.ones((K, D)) if fill is None else m))
            for C in (64, 72):
                w = np.full((C, 128), fill, np.float32) if fill is not None else rng.standard_normal((C, 128)).astype(np.float32)
                made.append(ctx.pca(w, w[0].copy()))
            for h in made:
                h.close()
        from pvsim import _ffi
        ctx.diag_poison(0xFF, _ffi.POISON_TABLE_CACHE)
        for name in TABLE_CASES:
            _, got = execute(ctx, name)
            same_bytes(got, want[name], f"{name} with its tables in recycled blocks")
    finally:
        ctx.close()


# ====================================================================================================================== the Python classes
class _Requests:
    """what a step asks of Context.buffer, and how much of it the cache served"""

    def __init__(self, ctx):
        self.ctx, self.sizes, self.hits, self._orig = ctx, [], 0, ctx._take_cached
        ctx._take_cached = self._spy

    def _spy(self, nbytes):
        hit = self._orig(nbytes)
        self.sizes.append(int(nbytes))
        self.hits += hit is not None
        return hit

    def stop(self):
        del self.ctx._take_cached                              # the class's method again
        return self.sizes, self.hits


def _seed_cache(ctx, sizes):
    """buffers of the sizes the next step will ask for, filled with 0xFF and freed: the step is served from them"""
    ctx.trim()
    want = sorted(set(sizes), reverse=True)[:ctx._CACHE_BLOCKS]
    bufs = [ctx.buffer(n).fill_bytes(0xFF) for n in want]
    for b in bufs:
        b.free()
    ctx.sync()
    return len(want)


def _run_scenario(ctx, make, steps, seed_with=None):
    """-> (outputs of every step by name, the buffer sizes every step requested, cache hits per step)"""
    obj = make(ctx)
    out, sizes, hits = {}, [], []
    try:
        for i, (name, fn) in enumerate(steps):
            if seed_with is not None:
                _seed_cache(ctx, seed_with[i])
            spy = _Requests(ctx)
            try:
                res = fn(obj)
            finally:
                s, h = spy.stop()
            sizes.append(s), hits.append(h)
            for key, v in (res if isinstance(res, dict) else {}).items():      # add / remove return nothing, or the index itself
                out[f"{name}.{key}"] = np.ascontiguousarray(v).copy()
    finally:
        close = getattr(obj, "close", None)
        if close:
            close()
    return out, sizes, hits


def _lists(idx, val):
    return {"idx": idx, "val": val}


def _corpus(seed=7400, L=64, n=480):
    rng = np.random.default_rng(seed)
    proto = rng.standard_normal((9, L))
    x = (proto[rng.integers(0, 9, n)] + 0.7 * rng.standard_normal((n, L))).astype(np.float32)
    return x, [f"img/{i:04d}.jpg" for i in range(n)]


X, PATHS = _corpus()
GONE = sorted({0, 299} | set(np.random.default_rng(7401).choice(300, 60, replace=False).tolist()))
QUERIES = np.ascontiguousarray(np.concatenate([X[[5, 77, 430]], np.random.default_rng(7402).standard_normal((3, 64)).astype(np.float32)]))
MANY_QUERIES = np.ascontiguousarray((X[np.arange(600) % 480] + 0.3 * np.random.default_rng(7403).standard_normal((600, 64))).astype(np.float32))


def _first(n=300):
    return {PATHS[i]: X[i] for i in range(n)}


def _added():
    return {PATHS[i]: X[i] for i in range(300, 340)}


def _removed():
    return [PATHS[i] for i in GONE]


def _tables(L=64, d=64, m=8, ksub=16, nlist=7):
    rng = np.random.default_rng(7100 + L)
    cb = (0.4 * rng.standard_normal((m, ksub, d // m))).astype(np.float32)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    return cb, cent


def _make_device_index(ctx):
    from pvsim.index import DeviceIndex
    return DeviceIndex(_first(), ctx)


def _make_int8_index(ctx):
    from pvsim import Int8Index
    return Int8Index(_first(), ctx)


def _make_compact(kind):
    def make(ctx):
        from pvsim import CompactIndex, IVFCompactIndex, ProductQuantizer
        from pvsim.compact import _sort_into_lists
        cb, cent = _tables()
        pq = ProductQuantizer.from_codebooks(cb, ctx)
        y, n, d = X[:300], 300, 64
        d_y, d_inv = ctx.buffer(y.nbytes).upload(y), ctx.buffer(n * 4)
        ctx.row_inv_norms_dev(d_y.ptr, n, d, d_inv.ptr)
        inv = d_inv.download((n,), np.float32)
        if kind == "flat":
            d_y.free(), d_inv.free()
            return CompactIndex(PATHS[:n], pq.encode(y), inv, pq, None, y, ctx)
        nlist = cent.shape[0]
        d_cent, d_lists, d_res = ctx.buffer(cent.nbytes).upload(cent), ctx.buffer(n * 4), ctx.buffer(n * d * 4)
        ctx.ivf_assign_dev(d_y.ptr, n, d, d_cent.ptr, nlist, d_lists.ptr, d_res.ptr)
        lists, res = d_lists.download((n,), np.int32), d_res.download((n, d), np.float32)
        for b in (d_y, d_inv, d_cent, d_lists, d_res):
            b.free()
        ids, off = _sort_into_lists(lists, nlist)
        return IVFCompactIndex(PATHS[:n], pq.encode(res)[ids], inv[ids], pq, cent, off, ids, None, y, ctx)
    return make


def _make_ivf_int8(ctx):
    import pvsim
    return pvsim.IVFInt8Index.build(_first(), _tables()[1], ctx)


def _stored(names, arrays):
    return dict(zip(names, arrays))


def _update_steps(rank, stored):
    return [("rank", rank), ("add", lambda ix: ix.add(_added())), ("rank_after_add", rank), ("remove", lambda ix: ix.remove(_removed())),
            ("stored", stored), ("rank_after_remove", rank)]


class _GraphOver:
    """a structure built over a DeviceIndex: both are closed together"""

    def __init__(self, index, top):
        self.index, self.top = index, top

    def close(self):
        self.top.close()
        self.index.close()


def _make_diffusion(ctx):
    from pvsim import Diffusion
    index = _make_device_index(ctx)
    return _GraphOver(index, Diffusion.build(index, k=10, gamma=3, block=128, mutable=True))


def _make_reciprocal(ctx):
    from pvsim import KReciprocal
    index = _make_device_index(ctx)
    return _GraphOver(index, KReciprocal.build(index, k=20, k1=10, k2=4, gamma=3, block=128))


def _asmk_inputs():
    import asmk_numpy as tw
    rng = np.random.RandomState(1850)
    K = 30
    proto = rng.randint(0, 80, (K, 128)).astype(np.uint8)

    def rows(words):
        return np.clip(proto[words].astype(np.int64) + rng.randint(-2, 3, (len(words), 128)), 0, 255).astype(np.uint8)

    images = [rows(rng.randint(0, K, n)) for n in [0, 1, 7, 25, 40, 3, 12, 30, 18, 9, 22, 5, 14, 33, 8, 21]]
    queries = [images[4][::2].copy(), np.concatenate([images[7][:15], rows(rng.randint(0, K, 6))]), np.zeros((0, 128), np.uint8)]
    return tw.rootsift(proto), images, queries


def _make_asmk(ctx):
    from pvsim import ASMKIndex
    from pvsim.verify import LocalFeatureIndex
    cent, images, _ = _asmk_inputs()
    local = LocalFeatureIndex.from_arrays(images[:12], [np.zeros((len(r), 6), np.float32) for r in images[:12]], [f"im{i}" for i in range(12)],
                                          ctx=ctx)
    return _GraphOver(local, ASMKIndex.build(local, cent, bits=128, on_device=True).freeze())    # fixed weights: add and remove in place


def _asmk_steps():
    from pvsim import ASMKExpansion
    _, images, queries = _asmk_inputs()
    rank = lambda o: _lists(*o.top.rank_rows(queries, 5))                                            # noqa: E731
    expanded = lambda o: _lists(*o.top.rank_rows(queries, 5, expand=ASMKExpansion(n=3, min_support=1)))   # noqa: E731
    stored = lambda o: {"word_off": o.top.word_off, "ent_img": o.top.ent_img, "ent_sig": o.top.ent_sig, "gamma_db": o.top.gamma_db}   # noqa: E731
    return [("rank", rank), ("rank_expanded", expanded), ("add", lambda o: o.top.add([f"im{i}" for i in range(12, 16)], images[12:16])),
            ("rank_after_add", rank), ("remove", lambda o: o.top.remove(["im3", "im14", "im0"])), ("stored", stored), ("rank_after_remove", rank)]


def _verify_images():
    import dsift_numpy as dtw
    import match_numpy as tw
    h, w = 160, 200
    th, s = np.deg2rad(15.0), 1.15
    M = s * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    c = np.array([(w - 1) / 2.0, (h - 1) / 2.0])
    model = np.concatenate([M, (c + np.array([6.0, -4.0]) - M @ c)[:, None]], axis=1)
    u8 = lambda im: np.clip(np.floor(im + 0.5), 0, 255).astype(np.uint8)                              # noqa: E731
    base = dtw.texture(h, w, 21, channels=1)
    return u8(base), {"other1": u8(dtw.texture(h, w, 22, channels=1)), "copy": u8(tw.warp_bilinear(base, model, (h, w)))}


def _make_verifier(ctx):
    from pvsim.features import KeypointSIFT
    from pvsim.verify import LocalFeatureIndex, SpatialVerifier
    _, images = _verify_images()
    ext = KeypointSIFT(ctx=ctx)
    index = LocalFeatureIndex.from_images(list(images.values()), ext, batch=2, paths=list(images), ctx=ctx)
    return _GraphOver(index, type("V", (), {"ver": SpatialVerifier(extractor=ext, ctx=ctx), "close": lambda self: None})())


def _verify_step(o):
    query, images = _verify_images()
    out = {}
    for path, v in zip(images, o.top.ver.verify(query, o.index, list(images))):
        out.update({f"{path}.inliers": np.array([v.inliers, v.best]), f"{path}.model": v.model, f"{path}.matches": v.matches,
                    f"{path}.mask": v.mask})
    return out


def _scenarios():
    rank = lambda ix: _lists(*ix.rank(QUERIES, 10))                                                  # noqa: E731
    graph = lambda o: {"nbr": o.top.nbr, "s": o.top.s, "sim": o.top.sim}                             # noqa: E731
    return {
        "DeviceIndex": (_make_device_index, _update_steps(rank, lambda ix: {"matrix": ix.matrix, "inv_norms": ix.inv_norms})
                        + [("rank_filtered", lambda ix: _lists(*ix.rank(MANY_QUERIES, 5)))]),
        "Int8Index": (_make_int8_index, _update_steps(rank, lambda ix: _stored(("codes", "factors"), ix._download()))),
        "CompactIndex": (_make_compact("flat"), _update_steps(lambda ix: _lists(*ix.rank(QUERIES, 10, rerank=30)),
                                                             lambda ix: _stored(("codes", "inv"), ix._download()))),
        "IVFCompactIndex": (_make_compact("ivf"), _update_steps(lambda ix: _lists(*ix.rank(QUERIES, 10, 3, rerank=30)),
                                                               lambda ix: {**_stored(("codes", "inv"), ix._download()), "list_off": ix._list_off,
                                                                           "ids": ix._ids})),
        "IVFInt8Index": (_make_ivf_int8, _update_steps(lambda ix: _lists(*ix.rank(QUERIES, 10, 3, scan="queries")),
                                                      lambda ix: _stored(("codes", "factors", "ids", "list_off"), ix._download()))
                         + [("rank_by_lists", lambda ix: _lists(*ix.rank(MANY_QUERIES, 10, 3, scan="lists", query_block=256)))]),
        "ASMKIndex": (_make_asmk, _asmk_steps()),
        "Diffusion": (_make_diffusion, [("rank", lambda o: _lists(*o.top.rank(QUERIES, k=10, kq=10))), ("add", lambda o: o.top.add(_added())),
                                        ("remove", lambda o: o.top.remove(_removed())), ("stored", graph),
                                        ("rank_after_update", lambda o: _lists(*o.top.rank(QUERIES, k=10, kq=10)))]),
        "KReciprocal": (_make_reciprocal, [("rank", lambda o: _lists(*o.top.rank(QUERIES, k=10, kq=30)))]),
        "SpatialVerifier": (_make_verifier, [("verify", _verify_step)]),
    }


@pytest.mark.parametrize("name", sorted(_scenarios()))
def test_python_classes_on_a_seeded_buffer_cache(name):
    """One rank / search call and one add + remove of every index class (the re-rankers: one rank; the verifier: one verify), first
    on a fresh context, recording the buffer sizes every step requests; then on a second context whose buffer cache holds 0xFF-filled
    blocks of exactly those sizes before every step.  The same bytes out, the same stored arrays after the updates."""
    import pvsim
    make, steps = _scenarios()[name]
    ctx = pvsim.Context(0)
    try:
        want, sizes, _ = _run_scenario(ctx, make, steps)
    finally:
        ctx.close()
    assert want and any(sizes), f"{name}: nothing came out, or no step asked for a buffer"
    ctx = pvsim.Context(0)
    try:
        got, sizes2, hits = _run_scenario(ctx, make, steps, seed_with=sizes)
    finally:
        ctx.close()
    assert sizes2 == sizes, f"{name}: the second run asked for other buffers than the first"
    for (step, _), s, h in zip(steps, sizes, hits):
        assert h > 0 or not s, f"{name}.{step}: none of its {len(s)} buffers came out of the seeded cache"
    same_bytes(got, want, f"{name} with a buffer cache of 0xFF")


# ====================================================================================================================== coverage
def test_every_pair_of_the_workspace_table_is_reached_by_a_case():
    """(slot, function) pairs parsed out of the comment table of csrc/workspace.hpp against the pairs the cases declare (and the
    fresh run of each case proves: its slots were reserved).  A new user of ws_reserve enters the table (tests/test_ws_ledger_host.py
    insists) and then needs a case here."""
    declared = {}
    for name, fn in CASES.items():
        for pair in fn.covers:
            declared.setdefault(pair, []).append(name)
    table = ws_ledger.table_pairs()
    missing = [p for p in table if p not in declared]
    assert not missing, f"no case reaches {missing}"
    unknown = sorted(set(declared) - set(table))
    assert not unknown, f"cases name pairs the table does not hold: {unknown}"
    assert {s for s, _ in table} == set(SLOTS) and len(table) >= 83 and len(CASES) >= 46
