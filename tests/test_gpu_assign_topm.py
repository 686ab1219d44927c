"""GPU tests of pvs_kmeans_topm_dev (csrc/assign_topm.hip): the top-m list of every row against the NumPy twin
(tests/asmk_ma_numpy.py), bit for bit.

Lattice inputs -- rows of integers in [-8, 8], centroids of multiples of 1/2 in [-8, 8] -- make every v exact in float32, so the
twin's float64 order is the only admissible one and exact ties are real (at D = 2 there are 1089 lattice points for 1000 centroids).
For the RootSIFT kinds the rows are SIFT-like; the test asserts `rank_gaps` on its own inputs before it trusts the float64 order, and
compares the values with the twin's float32 restatement of the header's chain."""
import numpy as np
import pytest

import asmk_ma_numpy as ma
import asmk_numpy as tw

pytestmark = pytest.mark.gpu

F = np.float32
DESC_F32, DESC_F32_ROOTSIFT, DESC_U8_ROOTSIFT = 0, 1, 2
FILL = 0x5A
MS = (1, 2, 5, 8)
TOTALS = (1, 255, 256, 257, 700)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _lattice(rng, n, K, D):
    return rng.randint(-8, 9, (n, D)).astype(F), (rng.randint(-16, 17, (K, D)) / 2.0).astype(F)


class _Rows:
    """rows on the device at an aligned and at a misaligned address (4 bytes off for float32, 1 byte for uint8: the scalar load path)"""

    def __init__(self, ctx, x):
        self.x = np.ascontiguousarray(x)
        self.n, esz = len(self.x), self.x.dtype.itemsize
        self.buf = ctx.buffer(self.x.nbytes + 64)
        self.off = {False: 0, True: esz}
        self.at = None

    def ptr(self, misaligned):
        if self.at != misaligned:
            self.buf.upload(self.x, self.off[misaligned])
            self.at = misaligned
        return self.buf.ptr + self.off[misaligned]

    def free(self):
        self.buf.free()


def _topm(ctx, cb, rows, kind, total, m, splits=0, misaligned=False, values=True):
    """-> (labels int32 (total, m), val float32 (total, m) or None); the arrays are pre-filled so an unwritten slot shows"""
    d_lab = ctx.buffer(max(total * m, 4) * 4).fill_bytes(FILL)
    d_val = ctx.buffer(max(total * m, 4) * 4).fill_bytes(FILL) if values else None
    try:
        ctx.kmeans_topm_dev(cb, rows.ptr(misaligned), kind, total, m, d_lab.ptr, d_val.ptr if values else None, splits)
        return d_lab.download((total, m), np.int32), d_val.download((total, m), F) if values else None
    finally:
        d_lab.free()
        if d_val is not None:
            d_val.free()


# ------------------------------------------------------------------------------------------------ lattice: labels and values
@pytest.mark.parametrize("D", [2, 20, 128, 136])
@pytest.mark.parametrize("K", [1, 5, 33, 256, 257, 1000])
def test_lattice_lists_equal_the_twin(gpu_ctx, K, D):
    """every m in {1, 2, 5, 8} that K allows and m = K (when K <= 8), every total in {1, 255, 256, 257, 700}, the vector and the
    scalar load path.  One reference per (K, D): the list at the deepest m; a shallower list is its prefix because the order is total."""
    rng = np.random.RandomState(2200 + 7 * K + D)
    x, cent = _lattice(rng, max(TOTALS), K, D)
    deepest = min(K, 8)
    want_lab, want_v = ma.topm(x, cent, deepest)
    assert np.array_equal(want_v, want_v.astype(F).astype(np.float64))     # the lattice keeps every v exact in float32
    ms = sorted({m for m in MS if m <= K} | ({K} if K <= 8 else set()))
    cb, rows = gpu_ctx.codebook(cent), _Rows(gpu_ctx, x)
    try:
        for misaligned in (False, True):
            for m in ms:
                for total in TOTALS:
                    lab, val = _topm(gpu_ctx, cb, rows, DESC_F32, total, m, misaligned=misaligned)
                    where = f"K={K} D={D} m={m} total={total} misaligned={misaligned}"
                    assert np.array_equal(lab, want_lab[:total, :m]), where
                    assert np.array_equal(_bits(val), _bits(want_v[:total, :m])), where
        lab, val = _topm(gpu_ctx, cb, rows, DESC_F32, 257, ms[-1], values=False)   # d_val may be NULL
        assert val is None and np.array_equal(lab, want_lab[:257, :ms[-1]])
    finally:
        cb.close()
        rows.free()


def test_65536_words_with_the_nearest_at_the_last_index(gpu_ctx):
    rng = np.random.RandomState(2300)
    x, cent = _lattice(rng, 64, 65536, 32)
    cent[65535] = x[0]                                                     # v = -|x|^2: below every other centroid of row 0
    want_lab, want_v = ma.topm(x, cent, 5)
    assert want_lab[0, 0] == 65535 and want_v[0, 0] < want_v[0, 1]
    cb, rows = gpu_ctx.codebook(cent), _Rows(gpu_ctx, x)
    try:
        for splits in (0, 1):
            lab, val = _topm(gpu_ctx, cb, rows, DESC_F32, 64, 5, splits=splits)
            assert np.array_equal(lab, want_lab) and np.array_equal(_bits(val), _bits(want_v)), f"splits = {splits}"
    finally:
        cb.close()
        rows.free()


# ------------------------------------------------------------------------------------------------ splits and seams
def test_every_split_count_gives_the_same_arrays(gpu_ctx):
    """K = 1000 is four 256-centroid blocks: splits 1, 2, 3, 4, the host's choice (0) and values the host clamps (7, -2)"""
    rng = np.random.RandomState(2310)
    x, cent = _lattice(rng, 700, 1000, 20)
    want_lab, want_v = ma.topm(x, cent, 8)
    cb, rows = gpu_ctx.codebook(cent), _Rows(gpu_ctx, x)
    try:
        for m in (1, 5, 8):
            for splits in (1, 2, 3, 4, 0, 7, -2):
                lab, val = _topm(gpu_ctx, cb, rows, DESC_F32, 700, m, splits=splits)
                assert np.array_equal(lab, want_lab[:, :m]) and np.array_equal(_bits(val), _bits(want_v[:, :m])), f"m={m} splits={splits}"
    finally:
        cb.close()
        rows.free()


def test_duplicate_centroids_across_every_seam(gpu_ctx):
    """A centroid and its copy at distance 4 (the other half-wave of the accumulator tile), 32 (the next tile), 256 (the next
    block) and 512 (another split at splits = 2 and 4), with a row exactly on them: equal v, the lower index first, both in the list
    when m >= 2."""
    rng = np.random.RandomState(2320)
    K, D = 1000, 20
    x, cent = _lattice(rng, 300, K, D)
    pairs = []
    for r, (i, d) in enumerate([(3, 4), (250, 4), (40, 32), (230, 32), (100, 256), (255, 256), (300, 512), (0, 512), (487, 512)]):
        p = rng.randint(-8, 9, D).astype(F)
        cent[i], cent[i + d], x[r] = p, p, p
        pairs.append((r, i, i + d))
    want_lab, want_v = ma.topm(x, cent, 8)
    for r, i, j in pairs:
        assert want_lab[r, 0] == i and want_lab[r, 1] == j and want_v[r, 0] == want_v[r, 1] < want_v[r, 2]
    cb, rows = gpu_ctx.codebook(cent), _Rows(gpu_ctx, x)
    try:
        for m in (1, 2, 5, 8):
            for splits in (1, 2, 4, 0):
                lab, val = _topm(gpu_ctx, cb, rows, DESC_F32, 300, m, splits=splits)
                for r, i, j in pairs:
                    assert lab[r, 0] == i and (m == 1 or lab[r, 1] == j), f"m={m} splits={splits} row {r}"
                assert np.array_equal(lab, want_lab[:, :m]) and np.array_equal(_bits(val), _bits(want_v[:, :m])), f"m={m} splits={splits}"
    finally:
        cb.close()
        rows.free()


# ------------------------------------------------------------------------------------------------ RootSIFT kinds
def _sift_like(rng, K, n_pool, m, n_keep):
    """prototypes, and rows around them whose first m + 1 ranks are clear of each other by the twin's guard"""
    proto = rng.randint(0, 80, (K, 128)).astype(np.uint8)
    cent = tw.rootsift(proto)
    raw = np.clip(proto[rng.randint(0, K, n_pool)].astype(np.int64) + rng.randint(-3, 4, (n_pool, 128)), 0, 255).astype(np.uint8)
    raw = raw[ma.rank_gap_ratios(tw.rootsift(raw), cent, m) > 1.5][:n_keep]
    return cent, raw


@pytest.mark.parametrize("kind", [DESC_U8_ROOTSIFT, DESC_F32_ROOTSIFT])
@pytest.mark.parametrize("K", [33, 257])
def test_rootsift_kinds_equal_the_twin(gpu_ctx, kind, K):
    rng = np.random.RandomState(2400 + K + kind)
    cent, raw = _sift_like(rng, K, 4000, 8, 300)
    assert len(raw) >= 257                                                  # more than one row block
    values = tw.rootsift(raw)
    ok, ratio = ma.rank_gaps(values, cent, 8)
    assert ok, f"the test's own rows are too close to a tie ({ratio})"
    want_lab, _ = ma.topm(values, cent, 8)
    chain_lab, chain_v = ma.topm_chain(values, cent, 8)
    assert np.array_equal(chain_lab, want_lab)                              # the guard holds what it promises
    cb, rows = gpu_ctx.codebook(cent), _Rows(gpu_ctx, raw if kind == DESC_U8_ROOTSIFT else raw.astype(F))
    try:
        for misaligned in (False, True):
            for m in MS:
                for total in (1, 256, len(raw)):
                    lab, val = _topm(gpu_ctx, cb, rows, kind, total, m, misaligned=misaligned)
                    where = f"m={m} total={total} misaligned={misaligned}"
                    assert np.array_equal(lab, want_lab[:total, :m]), where
                    assert np.array_equal(_bits(val), _bits(chain_v[:total, :m])), where
    finally:
        cb.close()
        rows.free()


# ------------------------------------------------------------------------------------------------ m = 1 against the exact kernel
@pytest.fixture(scope="module")
def predict_inputs():
    """K = 256 at D = 128 (the prefiltered assignment serves it from 4096 rows on): Gaussian rows and centroids for the plain
    kind, SIFT-like rows and RootSIFT centroids for the two fused kinds; the references are computed once"""
    import pvsim_oracle_c as orc_c
    rng = np.random.RandomState(2500)
    gauss_c, gauss_x = rng.standard_normal((256, 128)).astype(F), rng.standard_normal((5000, 128)).astype(F)
    proto = rng.randint(0, 80, (256, 128)).astype(np.uint8)
    raw = np.clip(proto[rng.randint(0, 256, 5000)].astype(np.int64) + rng.randint(-20, 21, (5000, 128)), 0, 255).astype(np.uint8)
    sift_c = tw.rootsift(proto)
    return {DESC_F32: (gauss_c, gauss_x, orc_c.assign_chain(gauss_x, gauss_c)),
            DESC_F32_ROOTSIFT: (sift_c, raw.astype(F), orc_c.assign_chain(tw.rootsift(raw), sift_c)),
            DESC_U8_ROOTSIFT: (sift_c, raw, orc_c.assign_chain(tw.rootsift(raw), sift_c))}


@pytest.mark.parametrize("total", [300, 5000])
@pytest.mark.parametrize("kind", [DESC_F32, DESC_F32_ROOTSIFT, DESC_U8_ROOTSIFT])
def test_column_0_is_the_label_of_the_exact_kernel(gpu_ctx, predict_inputs, kind, total):
    """non-lattice rows: column 0 at m = 1 and at m = 5 equals pvs_kmeans_predict_dev (total = 5000 goes through its prefiltered
    path) and the C restatement of the recurrence, exactly"""
    cent, x, chain = predict_inputs[kind]
    cb, rows = gpu_ctx.codebook(cent), _Rows(gpu_ctx, x)
    d_lab = gpu_ctx.buffer(total * 4).fill_bytes(FILL)
    try:
        gpu_ctx.kmeans_predict_dev(cb, rows.ptr(False), kind, total, d_lab.ptr)
        predict = d_lab.download((total,), np.int32)
        assert np.array_equal(predict, chain[:total])
        for m in (1, 5):
            lab, _ = _topm(gpu_ctx, cb, rows, kind, total, m)
            assert np.array_equal(lab[:, 0], predict), f"m = {m}"
    finally:
        d_lab.free()
        cb.close()
        rows.free()


# ------------------------------------------------------------------------------------------------ NaN, refusals, no-op
@pytest.mark.parametrize("K", [5, 33, 1000])
def test_a_row_with_nan_gets_the_first_m_indices(gpu_ctx, K):
    rng = np.random.RandomState(2600 + K)
    x, cent = _lattice(rng, 300, K, 20)
    x[0, 3] = np.nan
    x[257] = np.nan
    x[299, 19] = np.nan
    want_lab, want_v = ma.topm(x, cent, min(K, 8))
    cb, rows = gpu_ctx.codebook(cent), _Rows(gpu_ctx, x)
    d_lab = gpu_ctx.buffer(300 * 4)
    try:
        gpu_ctx.kmeans_predict_dev(cb, rows.ptr(False), DESC_F32, 300, d_lab.ptr)
        predict = d_lab.download((300,), np.int32)
        assert predict[0] == 0 and predict[257] == 0
        for m in sorted({1, 2, min(K, 5), min(K, 8)}):
            for splits in (0, 1):
                lab, val = _topm(gpu_ctx, cb, rows, DESC_F32, 300, m, splits=splits)
                for r in (0, 257, 299):
                    assert lab[r].tolist() == list(range(m)) and np.isposinf(val[r]).all(), f"m={m} row {r}"
                assert np.array_equal(lab, want_lab[:, :m]) and np.array_equal(_bits(val), _bits(want_v[:, :m]))
                assert np.array_equal(lab[:, 0], predict)
    finally:
        d_lab.free()
        cb.close()
        rows.free()


def test_refusals_and_the_empty_call(gpu_ctx):
    rng = np.random.RandomState(2700)
    x, cent = _lattice(rng, 10, 5, 20)
    cb, rows = gpu_ctx.codebook(cent), _Rows(gpu_ctx, x)
    try:
        for bad in (0, 9, 6, -1):                                          # m = 6 > K = 5
            with pytest.raises(ValueError, match="m must lie in"):
                _topm(gpu_ctx, cb, rows, DESC_F32, 10, bad)
        with pytest.raises(ValueError):
            _topm(gpu_ctx, cb, rows, 7, 10, 1)                             # unknown descriptor kind
        d_lab = gpu_ctx.buffer(64).fill_bytes(FILL)
        try:
            gpu_ctx.kmeans_topm_dev(cb, rows.ptr(False), DESC_F32, 0, 3, d_lab.ptr, None, 0)
            assert (d_lab.download((64,), np.uint8) == FILL).all()         # total_desc == 0: nothing is written
        finally:
            d_lab.free()
    finally:
        cb.close()
        rows.free()
