"""The float64 restatements of the training passes (tests/learn_numpy.py) checked on the CPU: the exactness claim the GPU tests
rest on (on lattice inputs a float32 evaluation in ANY order equals the float64 value), the device's two-level draw against the
flat searchsorted, and the restatements against the scikit-learn fits recorded in tests/golden/learn_k16_d32.npz.  No GPU."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import learn_numpy as ln  # noqa: E402
import pvsim_oracle as orc  # noqa: E402

KM_ATOL = 5e-4            # tests/test_gpu_parity.py: centres against scikit-learn's fp32 member sums


def _golden():
    return np.load(os.path.join(REPO, "tests", "golden", "learn_k16_d32.npz"), allow_pickle=False)


def _f32_sqdist(x, c, order):
    """sum_d (x_d - c_d)^2 as a float32 fma chain over the dimensions in `order` (every term and every partial sum is rounded
    to float32; on the lattice none of the roundings changes anything)"""
    acc = np.zeros(len(x), np.float32)
    for d in order:
        t = x[:, d] - c[d]
        acc = (acc.astype(np.float64) + t.astype(np.float64) * t.astype(np.float64)).astype(np.float32)   # fmaf: one rounding
    return acc


def _f32_scores(x, C, order):
    """|c|^2 - 2 x.c with the dot product as a float32 fma chain over `order`, then fmaf(-2, dot, |c|^2)"""
    dot = np.zeros((len(x), len(C)), np.float32)
    cn = np.zeros(len(C), np.float32)
    for d in order:
        dot = (dot.astype(np.float64) + np.outer(x[:, d], C[:, d]).astype(np.float64)).astype(np.float32)
        cn = (cn.astype(np.float64) + C[:, d].astype(np.float64) ** 2).astype(np.float32)
    return (cn[None, :].astype(np.float64) - 2.0 * dot.astype(np.float64)).astype(np.float32)


def test_float32_in_any_order_equals_float64_on_the_lattice():
    rng = np.random.default_rng(1)
    n, D, K = 8193, 130, 24
    x = rng.integers(0, 16, (n, D)).astype(np.float32)
    C = x[rng.choice(n, K, replace=False)].copy()
    C[7] = C[3]                                              # an exact tie for every row
    ln.lattice_ok(x, C)
    order = rng.permutation(D)
    # distances of the seeding and of the Lloyd step
    d64 = ln.sqdist(x, C[:3])
    assert d64.max() < ln.EXACT and d64.max() > 5000
    for j in range(3):
        assert np.array_equal(_f32_sqdist(x, C[j], order).astype(np.float64), d64[j])
    # scores, labels (first minimum), per-row distance of the Lloyd step
    s32 = _f32_scores(x, C, order)
    x64, c64 = x.astype(np.float64), C.astype(np.float64)
    assert np.array_equal(s32.astype(np.float64), (c64 * c64).sum(1)[None, :] - 2.0 * (x64 @ c64.T))
    labels, resid, counts, sq, inertia, changed = ln.lloyd_stats(x, C)
    assert np.array_equal(np.argmin(s32, axis=1), labels) and counts[7] == 0 and counts[3] > 0
    assert np.array_equal(sq, np.take_along_axis(ln.sqdist(x, C).T, labels[:, None].astype(np.int64), 1)[:, 0])
    # fp32 chunk sums of x - c in a shuffled row order, chunks added in fp64 = the float64 sums
    perm = rng.permutation(n)
    got = np.zeros((K, D))
    for r0 in range(0, n, ln.CHUNK):
        part = np.zeros((K, D), np.float32)
        rows = perm[r0:r0 + ln.CHUNK]
        np.add.at(part, labels[rows], x[rows] - C[labels[rows]])
        got += part
    assert np.array_equal(got, resid) and inertia == sq.sum() and changed == 0
    # the whole seeding run from float32 distances picks the same rows and reaches the same potentials
    u = np.random.RandomState(5).uniform(size=(K - 1, 5))
    idx, pots = ln.kmeanspp(x, K, 11, u)
    mind = _f32_sqdist(x, x[idx[0]], order)
    for c in range(1, K):
        assert float(mind.astype(np.float64).sum()) == pots[c - 1]
        mind = np.minimum(mind, _f32_sqdist(x, x[idx[c]], order))
    assert float(mind.astype(np.float64).sum()) == pots[-1]


def test_lattice_ok_rejects_inputs_outside_the_exact_regime():
    x = np.full((4, 2048), 15, np.float32)
    ln.lattice_ok(x)
    for bad in (x.astype(np.float64), x + np.float32(0.5), x - np.float32(16), np.full((4, 2048), 64, np.float32),
                np.full((4, 8), 80, np.float32)):
        with pytest.raises(AssertionError):
            ln.lattice_ok(bad)


@pytest.mark.parametrize("n", [1, 64, 4095, 4096, 4097, 8193, 12289])      # 4097, 8193, 12289: a last block of ONE row
def test_two_level_draw_equals_flat_searchsorted(n):
    rng = np.random.default_rng(n)
    x = rng.integers(0, 16, (n, 6)).astype(np.float32)
    first = rng.choice(n, min(n, 3), replace=False)
    mind = ln.sqdist(x, x[first]).min(0)                      # integer valued, zeros at the chosen rows (and their duplicates)
    pot = mind.sum()
    u = np.concatenate([[0.0, np.nextafter(1.0, 0.0), 1.0 - 2.0 ** -30, 2.0 ** -60], rng.uniform(size=2000)])
    # targets that fall exactly on a cumulative sum (every boundary rule shows here), one just below and one just above
    cum = np.cumsum(mind)
    hit = cum[rng.integers(0, n, 200)]
    r = np.concatenate([u * pot, hit, np.nextafter(hit, -np.inf), np.minimum(np.nextafter(hit, np.inf), pot)])
    flat = ln.draw_flat(mind, r)
    assert np.array_equal(ln.draw_two_level(mind, r), flat)
    assert flat.max() == n - 1 or pot == 0                    # u -> 1 reaches the last row
    if n > 1 and pot > 0:
        assert np.all(mind[flat[r > 0]] > 0)                  # a row at distance 0 is never drawn by a positive target
    # all-zero distances (every row chosen already): both give row 0
    z = np.zeros(n)
    assert np.array_equal(ln.draw_two_level(z, np.zeros(3)), ln.draw_flat(z, np.zeros(3)))


def test_three_lloyd_iterations_reproduce_the_recorded_fit():
    g = _golden()
    x = g["x_u8"].astype(np.float32) / np.float32(16.0)
    c, prev = g["c0"].copy(), None
    for _ in range(3):
        labels, resid, counts, sq, _, _ = ln.lloyd_stats(x, c, prev)
        c, _, far = ln.lloyd_update(x, c, labels, resid, counts, sq)
        assert len(far) == 0
        prev = labels
    labels, _, _, _, inertia, _ = ln.lloyd_stats(x, c)
    assert np.array_equal(labels, g["km3_labels"])
    np.testing.assert_allclose(c, g["km3_centers"], rtol=0, atol=KM_ATOL)
    assert abs(inertia - float(g["km3_inertia"])) <= 2e-5 * float(g["km3_inertia"])


def test_lloyd_update_relocates_empty_clusters_to_the_farthest_rows():
    rng = np.random.default_rng(3)
    x = rng.integers(0, 16, (500, 8)).astype(np.float32)
    x[40], x[41] = 0, 15                                       # |x - c|^2 of these two is far above the rest
    x[40, 0] = 1
    C = np.stack([x[5], x[9], x[5], np.full(8, 40, np.float32), np.full(8, 7, np.float32)])
    labels, resid, counts, sq, _, _ = ln.lloyd_stats(x, C)
    assert counts[2] == 0 and counts[3] == 0 and counts.sum() == 500
    far, nxt = ln.farthest_rows(sq, 2)
    assert sq[far[0]] > sq[far[1]] > nxt
    new, cnt, moved = ln.lloyd_update(x, C, labels, resid, counts, sq)
    assert np.array_equal(moved, far) and np.array_equal(new[2], x[far[0]]) and np.array_equal(new[3], x[far[1]])
    assert cnt.sum() == 500 and cnt[2] == 1 and cnt[3] == 1
    # the other centres are the means of their remaining members
    lab2 = labels.copy()
    lab2[far[0]], lab2[far[1]] = 2, 3
    for k in range(5):
        np.testing.assert_array_equal(new[k], x[lab2 == k].astype(np.float64).mean(0).astype(np.float32))


def test_label_sums_and_square_in_float32():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((300, 5)).astype(np.float32)
    lab = rng.integers(0, 4, 300)
    lab[lab == 2] = 3                                          # label 2 owns no row
    s1, s2 = ln.label_sums(x, lab, 4, False), ln.label_sums(x, lab, 4, True)
    assert not s1[2].any() and not s2[2].any()
    for k in (0, 1, 3):
        np.testing.assert_allclose(s1[k], x[lab == k].astype(np.float64).sum(0), rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(s2[k], (x[lab == k] * x[lab == k]).astype(np.float64).sum(0), rtol=1e-13)


def test_five_em_iterations_reproduce_the_recorded_fit():
    g = _golden()
    x = g["x_u8"].astype(np.float32) / np.float32(16.0)
    w, mu, cov = g["g_w0"], g["g_m0"], 1.0 / g["g_p0"]
    for _ in range(5):
        s0, s1, s2, ll = ln.em_stats(x, w, mu, cov)
        w, mu, cov = ln.m_step(s0, s1, s2, len(x))
    np.testing.assert_allclose(w, g["g5_weights"], rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(mu, g["g5_means"], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(cov, g["g5_cov"], rtol=1e-9, atol=1e-11)
    assert abs(ll / len(x) - float(g["g5_lower"])) < 1e-10
    # one block or many: the same statistics to rounding
    a, b = ln.em_stats(x[:5000], w, mu, cov, block=5000), ln.em_stats(x[:5000], w, mu, cov, block=777)
    for p, q in zip(a, b):
        np.testing.assert_allclose(p, q, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("D", [32, 130])
def test_gram_gives_the_covariance_of_pca_fit(D):
    if D == 32:
        x = _golden()["x_u8"].astype(np.float64) / 16
    else:
        rng = np.random.default_rng(8)
        q, _ = np.linalg.qr(rng.standard_normal((D, D)))
        x = (rng.standard_normal((5000, D)) * np.linspace(6.0, 0.5, D)) @ q.T + rng.standard_normal(D)
        x = x.astype(np.float32).astype(np.float64)
    n = len(x)
    s, g = ln.gram(x)
    assert np.array_equal(g, g.T)
    mean = s / n
    cov = (g - n * np.outer(mean, mean)) / (n - 1)
    np.testing.assert_allclose(cov, np.cov(x, rowvar=False), rtol=0, atol=1e-11 * np.abs(cov).max())
    vals, vecs = np.linalg.eigh(cov)
    c64, mean64, ev64 = orc.pca_fit(x, 16)
    np.testing.assert_allclose(mean, mean64, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(vals[::-1][:16], ev64, rtol=1e-9)
    np.testing.assert_allclose(np.abs(np.sum(vecs[:, ::-1][:, :16].T * c64, axis=1)), 1.0, atol=1e-6)
