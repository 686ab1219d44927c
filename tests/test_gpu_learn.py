"""The device passes of vocabulary training (csrc/learn.hip, launch_gmm_em_step in csrc/fisher.hip) against the float64
restatements of tests/learn_numpy.py, at the shapes where their indexing changes path: ragged chunks, blocks and tiles, the scalar
and float4 loads, candidates in LDS and in global memory, the long-row forms, padded K, two cluster blocks, the K limit, and -- with
PVS_OPT_TRAIN_BATCH_CHUNKS -- the seam between two batches.

Inputs are LATTICE rows (small integers as float32, learn_numpy.lattice_ok): every distance, score and sum is an exact integer in
float32 and float64 alike, so the device must EQUAL the restatement -- distances and potentials bit for bit, drawn rows index for
index, labels with first-minimum ties (exact ties are frequent on the lattice), sums, counts and inertia.  No tolerance.  The EM
step (exp, log) is compared with the tolerances tests/test_gpu_parity.py already uses for the same quantities."""
import warnings

import numpy as np
import pytest

import learn_numpy as ln
import pvsim_oracle as orc
from conftest import load_golden
from pvsim import _ffi, learn

pytestmark = pytest.mark.gpu

_BIG = 0x7F                                      # learn._BIG_F32_BYTE: "no centre yet"


def _lattice(rng, n, D, hi=16):
    return rng.integers(0, hi, (n, D)).astype(np.float32)


def _rows(ctx, x):
    return learn.DeviceRows.from_host(ctx, x)


def _f32buf(ctx, a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return ctx.buffer(a.nbytes).upload(a)


# ================================================================================ seeding distances
SEED_CASES = ([(n, 32, nc, 16) for nc in (1, 3, 8) for n in (1, 31, 33, 257, 4097)]
              # scalar loads (D % 4 != 0), float4 with a ragged last 32-dim step (36), fewer dims than the 8 lanes of a row (2, 4)
              + [(4097, D, 5, 16) for D in (2, 4, 30, 36, 130)]
              # 8 candidates fit in LDS up to D = 1983; from 1984 they are read from global memory (float4 at 1984, scalar at 1985)
              + [(513, D, 8, 4) for D in (1983, 1984, 1985)])


@pytest.mark.parametrize("n,D,n_cand,hi", SEED_CASES)
def test_seed_distances_equal_the_restatement(gpu_ctx, n, D, n_cand, hi):
    rng = np.random.default_rng(n * 10007 + D * 13 + n_cand)
    x = _lattice(rng, n, D, hi)
    cand = x[rng.integers(0, n, n_cand)].copy()
    if n_cand > 1:
        cand[-1] = _lattice(rng, 1, D, hi)[0]                    # a candidate that is no row of x
    ln.lattice_ok(x, cand)
    d = ln.sqdist(x, cand)
    mind = ln.sqdist(x, x[rng.integers(0, n, 2)]).min(0)
    rows = _rows(gpu_ctx, x)
    dist = gpu_ctx.buffer(n_cand * n * 4).fill_bytes(0xFF)
    mbuf = _f32buf(gpu_ctx, mind)
    try:
        for mb, want in ((None, d.sum(1)), (mbuf, np.minimum(mind[None, :], d).sum(1))):
            pot = gpu_ctx.seed_distances_dev(rows.ptr, D, n, cand, mb.ptr if mb else None, dist.ptr)
            got = dist.download((n_cand, n), np.float32)
            assert np.array_equal(got.astype(np.float64), d)
            assert np.array_equal(pot, want), (pot, want)
            dist.fill_bytes(0xFF)
    finally:
        for b in (dist, mbuf):
            b.free()
        rows.free()


# ================================================================================ running minimum, block sums, candidate draw
@pytest.mark.parametrize("n", [4095, 4096, 4097, 8193])
def test_min_update_and_pick_equal_the_restatement(gpu_ctx, n):
    D = 30
    rng = np.random.default_rng(n)
    x = _lattice(rng, n, D)
    ln.lattice_ok(x)
    d0, d1 = ln.sqdist(x, x[rng.integers(0, n, 2)])
    rows = _rows(gpu_ctx, x)
    mind = gpu_ctx.buffer(n * 4).fill_bytes(_BIG)
    b0, b1 = _f32buf(gpu_ctx, d0), _f32buf(gpu_ctx, d1)
    cand = gpu_ctx.buffer(64 * D * 4)
    try:
        sums = gpu_ctx.min_update_dev(mind.ptr, b0.ptr, n)
        assert np.array_equal(sums, ln.block_sums(d0))
        sums = gpu_ctx.min_update_dev(mind.ptr, b1.ptr, n)
        m = np.minimum(d0, d1)
        assert np.array_equal(sums, ln.block_sums(m))
        assert np.array_equal(mind.download((n,), np.float32).astype(np.float64), m)
        assert np.array_equal(gpu_ctx.min_update_dev(mind.ptr, None, n), ln.block_sums(m))      # sums only
        # the draw: u = 0, u -> 1, targets ON a cumulative sum and next to one, and uniform ones -- 64 per call
        pot, cum = m.sum(), np.cumsum(m)
        hit = cum[rng.integers(0, n, 40)]
        r = np.concatenate([np.array([0.0, np.nextafter(1.0, 0.0), 1.0 - 2.0 ** -30, 2.0 ** -60]) * pot, hit,
                            np.nextafter(hit, -np.inf), np.minimum(np.nextafter(hit, np.inf), pot), rng.uniform(size=68) * pot])
        assert len(r) == 192
        for g0 in range(0, len(r), 64):
            rg = r[g0:g0 + 64]
            ids = learn._draw_candidates(rows, mind, sums, rg, cand)
            assert np.array_equal(ids, ln.draw_flat(m, rg)), g0
            assert np.array_equal(cand.download((64, D), np.float32), x[ids])
        assert ln.draw_flat(m, r).max() == n - 1                 # the last row (alone in its block at 4097 and 8193) was drawn
    finally:
        for b in (mind, b0, b1, cand):
            b.free()
        rows.free()


# ================================================================================ whole seeding runs
def _reference_run(x, K, seed, trials, trace=None):
    rs = np.random.RandomState(seed)
    first = rs.randint(len(x))
    return ln.kmeanspp(x, K, first, rs.uniform(size=(K - 1, trials)), trace)


@pytest.mark.parametrize("stepwise", [False, True])
@pytest.mark.parametrize("n,D,K", [(8193, 32, 16), (4097, 30, 5), (300, 6, 40), (64, 4, 64)])
def test_kmeans_plusplus_picks_the_rows_of_the_restatement(gpu_ctx, n, D, K, stepwise):
    x = _lattice(np.random.default_rng(n + D + K), n, D)
    ln.lattice_ok(x)
    trials = 2 + int(np.log(K))
    want, pots = _reference_run(x, K, 7, trials)
    if K == n:
        assert pots[-1] == 0 and pots[-2] > 0                    # every row chosen: the potential reaches 0 at the last step
    rows = _rows(gpu_ctx, x)
    try:
        centers, idx = learn.kmeans_plusplus(rows, K, random_state=7, stepwise=stepwise)
        assert np.array_equal(idx, want), (idx, want)
        assert np.array_equal(centers, x[want])
    finally:
        rows.free()


@pytest.mark.parametrize("trials", [11, 17])
def test_kmeans_plusplus_with_more_than_eight_local_trials(gpu_ctx, trials):
    """two and three scoring groups of 8: the winner of a step whose group was overwritten by a later one has its distances
    recomputed before the running minimum is updated"""
    n, D, K = 8193, 32, 12
    x = _lattice(np.random.default_rng(trials), n, D)
    ln.lattice_ok(x)
    trace = []
    want, _ = _reference_run(x, K, 21, trials, trace)
    last_group = ((trials - 1) // 8) * 8
    slots = np.array([j for _, _, j in trace])
    assert (slots < last_group).any(), slots                     # the recompute branch runs ...
    assert (slots >= 8).any(), slots                             # ... and a later group beats an earlier one at least once
    rows = _rows(gpu_ctx, x)
    try:
        centers, idx = learn.kmeans_plusplus(rows, K, random_state=21, n_local_trials=trials)
        assert np.array_equal(idx, want), (idx, want)
        assert np.array_equal(centers, x[want])
    finally:
        rows.free()


# ================================================================================ Lloyd step
def _centres_with_a_duplicate(rng, x, K):
    """K - 1 distinct rows of x and, at a higher index, a copy of one of them -> (centres, index of the original, of the copy)"""
    if K == 1:
        return x[:1].copy(), None, None
    uniq = np.unique(x, axis=0, return_index=True)[1]
    assert len(uniq) >= K - 1
    C = x[rng.permutation(uniq)[:K - 1]]
    a = int(rng.integers(0, K - 1))
    b = int(rng.integers(a + 1, K))
    return np.insert(C, b, C[a], axis=0), a, b


def _check_lloyd_step(ctx, rows, x, C, prev, ref):
    labels, resid, counts, sq, inertia, changed = ref
    n = len(x)
    cb = ctx.codebook(C)
    lab, sqd = ctx.buffer(n * 4).fill_bytes(0xFF), ctx.buffer(n * 4).fill_bytes(0xFF)
    pb = ctx.buffer(n * 4).upload(prev.astype(np.int32)) if prev is not None else None
    try:
        r, c, i, ch = ctx.kmeans_step_dev(cb, rows.ptr, n, lab.ptr, pb.ptr if pb else None, sqd.ptr)
        got = lab.download((n,), np.int32)
        assert np.array_equal(got, labels), (np.flatnonzero(got != labels)[:8], got[got != labels][:8], labels[got != labels][:8])
        assert np.array_equal(c, counts)
        assert np.array_equal(r, resid), np.abs(r - resid).max()
        assert np.array_equal(sqd.download((n,), np.float32).astype(np.float64), sq)
        assert i == inertia and ch == changed, (i, inertia, ch, changed)
        return r, c, i, got, sqd.download((n,), np.float32)
    finally:
        for b in (lab, sqd, pb):
            if b is not None:
                b.free()
        cb.close()


LLOYD_SHAPES = [(1, 1, 4),               # one row
                (4095, 17, 30),          # below the prefilter's 4096-row threshold, scalar loads, padded K
                (4097, 40, 100),         # above it, a chunk of one row
                (9000, 256, 128),        # the descriptor shape, three chunks
                (5000, 300, 36),         # two cluster blocks
                (6000, 64, 516),         # the wide-row lane layout of the aggregate
                (4200, 8, 1024),         # D = AGG_D_MAX: the aggregate's largest register count
                (700, 8, 1025),          # D > AGG_D_MAX: learn_label_residual_kernel
                (4200, 2048, 8)]         # the K limit


@pytest.mark.parametrize("n,K,D", LLOYD_SHAPES)
def test_lloyd_step_equals_the_restatement(gpu_ctx, n, K, D):
    rng = np.random.default_rng(n + 31 * K + D)
    x = _lattice(rng, n, D)
    C, a, b = _centres_with_a_duplicate(rng, x, K)
    ln.lattice_ok(x, C)
    ref = ln.lloyd_stats(x, C)
    if K > 1:
        assert ref[2][b] == 0 and ref[2][a] >= 1                 # the exact tie goes to the lower index
    rows = _rows(gpu_ctx, x)
    try:
        _check_lloyd_step(gpu_ctx, rows, x, C, None, ref)
        prev = ref[0].copy()
        altered = rng.choice(n, min(n, 37), replace=False) if K > 1 else np.zeros(0, np.int64)
        prev[altered] = (prev[altered] + 1) % K
        ref = ln.lloyd_stats(x, C, prev)
        assert ref[5] == len(altered)
        _check_lloyd_step(gpu_ctx, rows, x, C, prev, ref)
    finally:
        rows.free()


# ================================================================================ per-label sums
@pytest.mark.parametrize("square", [False, True])
@pytest.mark.parametrize("n,K,D", [(4095, 17, 30), (9000, 256, 128), (4200, 8, 1024), (700, 8, 1025), (700, 8, 2600),
                                   (4097, 1, 30), (4097, 1, 2600)])       # K = 1: learn._column_moments
def test_label_sums_equal_the_restatement(gpu_ctx, n, K, D, square):
    rng = np.random.default_rng(n + 31 * K + D)
    x = _lattice(rng, n, D)
    ln.lattice_ok(x)
    labels = rng.integers(0, K, n).astype(np.int32)
    if K > 1:
        labels[labels == K // 2] = K - 1                         # a label that owns no row
    want = ln.label_sums(x, labels, K, square)
    assert K == 1 or not want[K // 2].any()
    rows = _rows(gpu_ctx, x)
    lab = gpu_ctx.buffer(n * 4).upload(labels)
    try:
        got = gpu_ctx.label_sums_dev(rows.ptr, D, n, lab.ptr, K, square=square)
        assert np.array_equal(got, want), np.abs(got - want).max()
    finally:
        lab.free()
        rows.free()


# ================================================================================ Gram matrix, PCA
@pytest.mark.parametrize("n,D", [(1, 1), (31, 64), (33, 65), (8193, 130), (20000, 200), (300, 1000)])
def test_gram_equals_the_restatement(gpu_ctx, n, D):
    """one, two, three, four and sixteen 64-column tiles per side, a ragged last tile (65, 130, 200, 1000), a ragged last
    32-row step, a chunk of one row (8193) and a ragged third chunk (20000)"""
    x = _lattice(np.random.default_rng(n + D), n, D)
    ln.lattice_ok(x)
    s_ref, g_ref = ln.gram(x)
    rows = _rows(gpu_ctx, x)
    try:
        s, g = gpu_ctx.gram_dev(rows.ptr, D, n)
        assert np.array_equal(s, s_ref)
        assert np.array_equal(g, g.T)
        assert np.array_equal(g, g_ref), np.argwhere(g != g_ref)[:8]
    finally:
        rows.free()


def test_fit_pca_beyond_one_tile(gpu_ctx):
    rng = np.random.default_rng(8)
    n, D = 5000, 130
    q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    x = ((rng.standard_normal((n, D)) * np.linspace(6.0, 0.5, D)) @ q.T + rng.standard_normal(D)).astype(np.float32)
    rows = _rows(gpu_ctx, x)
    try:
        m = learn.fit_pca(rows, 16)
    finally:
        rows.free()
    c64, mean64, ev64 = orc.pca_fit(x.astype(np.float64), 16)
    np.testing.assert_allclose(m.mean_, mean64, rtol=2.0 ** -24, atol=0)      # the model keeps the mean in float32: half an ulp
    np.testing.assert_allclose(np.abs(np.sum(m.components_.astype(np.float64) * c64, axis=1)), 1.0, atol=1e-6)
    np.testing.assert_allclose(m.explained_variance_, ev64, rtol=1e-9)


# ================================================================================ empty-cluster relocation
def test_fit_kmeans_relocates_empty_clusters_as_the_restatement(gpu_ctx):
    rng = np.random.default_rng(17)
    n, D, K = 5000, 32, 16
    x = _lattice(rng, n, D)
    x[1234] = 0                                                  # two rows far from every centre ...
    x[1234, :3] = 1
    x[4321] = 15                                                 # ... at different distances
    c0 = x[rng.choice(n, K, replace=False)].copy()
    c0[11] = c0[4]                                               # a duplicate: cluster 11 gets no row
    c0[6] = 40                                                   # no row is nearest to this one
    ln.lattice_ok(x, c0)
    labels, resid, counts, sq, _, _ = ln.lloyd_stats(x, c0)
    assert np.array_equal(np.where(counts == 0)[0], [6, 11])
    far, third = ln.farthest_rows(sq, 2)
    assert sq[far[0]] > sq[far[1]] > third                       # the order argpartition leaves ties in cannot matter
    want, cnt, _ = ln.lloyd_update(x, c0, labels, resid, counts, sq)
    assert np.array_equal(want[6], x[far[0]]) and np.array_equal(want[11], x[far[1]]) and np.all(cnt > 0)
    rows = _rows(gpu_ctx, x)
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            m = learn.fit_kmeans(rows, K, init=c0, n_init=1, max_iter=1, tol=0.0)
    finally:
        rows.free()
    assert not [w for w in rec if "distinct clusters" in str(w.message)]
    assert m.n_iter_ == 1 and np.array_equal(m.cluster_centers_, want)
    # labels under the new (no longer integer) centres: the float64 argmin except at near ties, bounded as in
    # test_vlad_shapes_vs_oracle (what a D-term fp32 evaluation of |c|^2 - 2 x.c resolves)
    lab64, gap = orc.assignment_margin(x, want)
    bad = m.labels_ != lab64
    cmax = float(np.linalg.norm(want, axis=1).max())
    lim = 2.0 * (D + 4) * 2.0 ** -23 * (np.linalg.norm(x[bad].astype(np.float64), axis=1) * cmax + cmax * cmax)
    assert np.all(gap[bad] < lim), (gap[bad] / lim).max()
    assert np.bincount(m.labels_, minlength=K).min() >= 1


# ================================================================================ batch seams
SEAM_N = 20000              # five 4096-row chunks, three 8192-row chunks: a ragged last chunk in a ragged last batch


def _golden_rows():
    g = load_golden("learn_k16_d32")
    return g, g["x_u8"].astype(np.float32) / np.float32(16.0)


@pytest.mark.parametrize("K,D", [(16, 32), (40, 100)])
def test_lloyd_step_across_batch_seams(gpu_ctx, K, D):
    rng = np.random.default_rng(K + D)
    x = _lattice(rng, SEAM_N, D)
    C, a, b = _centres_with_a_duplicate(rng, x, K)
    ln.lattice_ok(x, C)
    ref = ln.lloyd_stats(x, C)
    rows = _rows(gpu_ctx, x)
    try:
        for v in (1, 3):
            with gpu_ctx.option(_ffi.OPT_TRAIN_BATCH_CHUNKS, v):
                _check_lloyd_step(gpu_ctx, rows, x, C, None, ref)
    finally:
        rows.free()
    assert gpu_ctx.get_option(_ffi.OPT_TRAIN_BATCH_CHUNKS) == 0
    if (K, D) != (16, 32):
        return
    # non-integer rows: the chunk sums are added in the same order whatever the batch size -> the same bits
    g, xg = _golden_rows()
    rows = _rows(gpu_ctx, xg)
    cb = gpu_ctx.codebook(g["c0"])
    lab, sqd = gpu_ctx.buffer(SEAM_N * 4), gpu_ctx.buffer(SEAM_N * 4)
    try:
        out = []
        for v in (0, 1, 3):
            with gpu_ctx.option(_ffi.OPT_TRAIN_BATCH_CHUNKS, v):
                r, c, i, ch = gpu_ctx.kmeans_step_dev(cb, rows.ptr, SEAM_N, lab.ptr, None, sqd.ptr)
            out.append((r.copy(), c.copy(), i, lab.download((SEAM_N,), np.int32), sqd.download((SEAM_N,), np.float32)))
        for o in out[1:]:
            assert all(np.array_equal(p, q) for p, q in zip(o, out[0]))
    finally:
        for b_ in (lab, sqd):
            b_.free()
        cb.close()
        rows.free()


@pytest.mark.parametrize("square", [False, True])
@pytest.mark.parametrize("K,D", [(16, 32), (40, 100)])
def test_label_sums_across_batch_seams(gpu_ctx, K, D, square):
    rng = np.random.default_rng(K + D)
    x = _lattice(rng, SEAM_N, D)
    ln.lattice_ok(x)
    labels = rng.integers(0, K, SEAM_N).astype(np.int32)
    want = ln.label_sums(x, labels, K, square)
    cases = [(x, want)]
    if (K, D) == (16, 32):
        cases.append((_golden_rows()[1], None))
    lab = gpu_ctx.buffer(SEAM_N * 4).upload(labels)
    try:
        for xs, exact in cases:
            rows = _rows(gpu_ctx, xs)
            try:
                base = gpu_ctx.label_sums_dev(rows.ptr, D, SEAM_N, lab.ptr, K, square=square)
                for v in (1, 3):
                    with gpu_ctx.option(_ffi.OPT_TRAIN_BATCH_CHUNKS, v):
                        got = gpu_ctx.label_sums_dev(rows.ptr, D, SEAM_N, lab.ptr, K, square=square)
                    assert np.array_equal(got, base), v
                    assert exact is None or np.array_equal(got, exact), v
            finally:
                rows.free()
    finally:
        lab.free()
    assert gpu_ctx.get_option(_ffi.OPT_TRAIN_BATCH_CHUNKS) == 0


@pytest.mark.parametrize("D", [32, 100])
def test_gram_across_batch_seams(gpu_ctx, D):
    x = _lattice(np.random.default_rng(D), SEAM_N, D)
    ln.lattice_ok(x)
    cases = [(x, ln.gram(x))]
    if D == 32:
        cases.append((_golden_rows()[1], None))
    for xs, exact in cases:
        rows = _rows(gpu_ctx, xs)
        try:
            s0, g0 = gpu_ctx.gram_dev(rows.ptr, D, SEAM_N)
            for v in (1, 2, 3):                                  # three, two and one batch(es) of the three chunks
                with gpu_ctx.option(_ffi.OPT_TRAIN_BATCH_CHUNKS, v):
                    s, g = gpu_ctx.gram_dev(rows.ptr, D, SEAM_N)
                assert np.array_equal(s, s0) and np.array_equal(g, g0), v
                assert exact is None or (np.array_equal(s, exact[0]) and np.array_equal(g, exact[1])), v
        finally:
            rows.free()
    assert gpu_ctx.get_option(_ffi.OPT_TRAIN_BATCH_CHUNKS) == 0


def test_em_step_across_batch_seams(gpu_ctx):
    g, xg = _golden_rows()
    n = 5000                                                     # three 2048-row chunks, the last ragged
    rows = _rows(gpu_ctx, xg[:n])
    gm = gpu_ctx.gmm(g["g_w0"], g["g_m0"], 1.0 / g["g_p0"])
    try:
        base = [np.copy(a) for a in gpu_ctx.gmm_em_step_dev(gm, rows.ptr, n)]
        for v in (1, 2, 3):
            with gpu_ctx.option(_ffi.OPT_TRAIN_BATCH_CHUNKS, v):
                s0, s1, s2, ll = gpu_ctx.gmm_em_step_dev(gm, rows.ptr, n)
            assert np.array_equal(s0, base[0]) and np.array_equal(s1, base[1]) and np.array_equal(s2, base[2]), v
            assert abs(ll - float(base[3])) / n < 1e-9, v        # its tree is per batch
    finally:
        gm.close()
        rows.free()
    assert gpu_ctx.get_option(_ffi.OPT_TRAIN_BATCH_CHUNKS) == 0


def test_train_batch_chunks_range(gpu_ctx):
    for bad in (-1, 1025):
        with pytest.raises(Exception):
            gpu_ctx.set_option(_ffi.OPT_TRAIN_BATCH_CHUNKS, bad)
    assert gpu_ctx.get_option(_ffi.OPT_TRAIN_BATCH_CHUNKS) == 0
    with gpu_ctx.option(_ffi.OPT_TRAIN_BATCH_CHUNKS, 1024):
        assert gpu_ctx.get_option(_ffi.OPT_TRAIN_BATCH_CHUNKS) == 1024
    assert gpu_ctx.get_option(_ffi.OPT_TRAIN_BATCH_CHUNKS) == 0


# ================================================================================ EM step
@pytest.mark.parametrize("n,K,D", [(1, 1, 1), (127, 1, 5), (2049, 3, 30), (4225, 256, 33), (2500, 257, 64), (3000, 1024, 8),
                                   (1500, 512, 8), (1500, 513, 8)])
def test_em_step_equals_the_restatement(gpu_ctx, n, K, D):
    """one row, one component, a chunk of one row (2049), the MFMA posterior's limit of 256 components with an odd D, the general
    posterior with two moment slabs (257), the component limit (1024), and 512 / 513 components: the general posterior keeps the
    log-probabilities of 32 rows in LDS up to 512 components (all 160 KiB at 512) and of 16 rows above.  Tolerances: those of test_learn_gmm_matches_reference_fit
    (K <= 256) and test_learn_gmm_more_than_256_components (above)."""
    rng = np.random.default_rng(n + K + D)
    mu = rng.normal(0, 4, (K, D))
    x = (mu[rng.integers(0, K, n)] + rng.standard_normal((n, D))).astype(np.float32)
    w0, m0, c0 = np.full(K, 1.0 / K), mu + 0.3 * rng.standard_normal((K, D)), np.ones((K, D))
    rows = _rows(gpu_ctx, x)
    gm = gpu_ctx.gmm(w0, m0, c0)
    try:
        s0, s1, s2, ll = gpu_ctx.gmm_em_step_dev(gm, rows.ptr, n)
    finally:
        gm.close()
        rows.free()
    nk, means, cov = learn._gmm_params_from_moments(s0, s1, s2, 1e-6)
    w = nk / n
    w = w / w.sum()
    r0, r1, r2, ll_ref = ln.em_stats(x, w0, m0, c0)
    w_ref, means_ref, cov_ref = ln.m_step(r0, r1, r2, n)
    rt, at = (1e-9, 1e-11) if K <= 256 else (1e-8, 1e-10)
    print(f"n={n} K={K} D={D}: weights {np.abs(w - w_ref).max():.3e} means {np.abs(means - means_ref).max():.3e} "
          f"cov {np.abs(cov - cov_ref).max():.3e} lower {abs(ll - ll_ref) / n:.3e}")
    np.testing.assert_allclose(w, w_ref, rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(means, means_ref, rtol=rt, atol=at)
    np.testing.assert_allclose(cov, cov_ref, rtol=rt, atol=at)
    assert abs(ll - ll_ref) / n < 1e-9
