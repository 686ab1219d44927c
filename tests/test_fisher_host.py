"""CPU-only checks of the Fisher twin (tests/fisher_numpy.py) and of the inputs and tolerances of the Fisher edge tests
(tests/fisher_cases.py): the twin agrees with the float64 oracle and the reference's goldens, every family's inputs meet
their conditions, and dev_ref (printed per family; DESIGN.md section 6 lists the figures) stays under the cap."""
import numpy as np
import pytest

import fisher_cases as fc
import fisher_numpy as fnp
import pvsim_oracle as orc
from conftest import load_golden

need_extended = pytest.mark.skipif(not fnp.EXTENDED, reason=fnp.NEED_EXTENDED)


def _small():
    g = load_golden("small_k16_d8")
    imgs = [r / np.float32(16.0) for r in orc.split_ragged(g["raw"], g["offsets"])]
    return g, imgs, (g["gmm_weights"], g["gmm_means"], g["gmm_covariances"])


def test_twin_posterior_agrees_with_the_oracle_on_the_goldens():
    g, imgs, tab = _small()
    x = np.concatenate(imgs)
    np.testing.assert_allclose(fnp.gmm_predict_proba(x, *tab).astype(np.float64), orc.gmm_predict_proba(x, *tab), rtol=0, atol=fc.RESP_ATOL)
    f = load_golden("fisher_deep_k32_d96")
    tab = (f["gmm_weights"], f["gmm_means"], f["gmm_covariances"])
    x = np.concatenate(list(f["desc"]))
    r = fnp.gmm_predict_proba(x, *tab)
    np.testing.assert_allclose(r.astype(np.float64), orc.gmm_predict_proba(x, *tab), rtol=0, atol=fc.RESP_ATOL)
    assert float(np.abs(r.sum(axis=1) - 1).max()) < 1e-15


def test_twin_posterior_agrees_with_the_recorded_reference_posterior(tables):
    """GaussianMixture.predict_proba of the reference itself on image 3 of the K = 256, D = 128 golden."""
    v, f = load_golden("vlad_k256_d128"), load_golden("fisher_k256_d128")
    x = orc.rootsift(orc.split_ragged(v["raw_u8"].astype(np.float32), v["offsets"])[3])
    r = fnp.gmm_predict_proba(x, tables["gmm_weights"], tables["gmm_means"], tables["gmm_covariances"])
    np.testing.assert_allclose(r.astype(np.float64), f["resp_img3"], rtol=0, atol=fc.RESP_ATOL)


@pytest.mark.parametrize("tag,kw", [("default", {}), ("p1", {"power": 1.0}), ("l1", {"norm_order": 1}), ("p03", {"power": 0.3})])
def test_twin_fisher_rows_agree_with_the_oracle_and_the_small_golden(tag, kw):
    g, imgs, tab = _small()
    F = fnp.fisher_encode(imgs, *tab, **kw).astype(np.float64)
    np.testing.assert_allclose(F, orc.fisher_encode(imgs, *tab, **kw), rtol=0, atol=fc.FISHER_ATOL)
    np.testing.assert_allclose(F, g["fisher_" + tag], rtol=0, atol=fc.FISHER_ATOL)


def test_twin_fisher_rows_agree_with_the_deep_golden():
    f = load_golden("fisher_deep_k32_d96")
    tab = (f["gmm_weights"], f["gmm_means"], f["gmm_covariances"])
    F = fnp.fisher_encode(list(f["desc"]), *tab).astype(np.float64)
    np.testing.assert_allclose(F, orc.fisher_encode(list(f["desc"]), *tab), rtol=0, atol=fc.FISHER_ATOL)
    np.testing.assert_allclose(F, f["fisher"], rtol=0, atol=fc.FISHER_ATOL)


def test_twin_options():
    """Norm orders 1, 2, general and +inf give unit norm of that order; eps enters the divisor; an empty image is a zero row;
    row blocks give the sums of the whole image; the float32 restatement is the twin rounded to float32 twice."""
    tab = fc.gmm_tables(17, 9)
    x = fc.draw(tab, 300)
    for p, o in fc.VARIANTS_ALL:
        v = fnp.fisher_encode_one(x, *tab, power=p, norm_order=o, eps=0.0)
        assert abs(float(np.linalg.norm(v.astype(np.float64), ord=o)) - 1.0) < 1e-12
    v, nrm = fnp.fisher_unnormalised(x, *tab)
    assert np.array_equal(fnp.fisher_encode_one(x, *tab, eps=0.25), v / (nrm + fnp.REAL(0.25)))
    for empty in (None, np.zeros((0, 9), np.float32)):
        row = fnp.fisher_encode_one(empty, *tab)
        assert row.shape == (17 + 2 * 17 * 9,) and not row.any()
    whole, blocks = fnp.fisher_encode_one(x, *tab), fnp.fisher_encode_one(x, *tab, block=64)
    assert float(np.abs(whole - blocks).max()) < 1e-15
    f32 = fnp.fisher_rows_f32([x, None], *tab)
    assert f32.dtype == np.float32 and not f32[1].any()
    # two float32 roundings (the stored gradient, then the quotient), half an ulp each, across at most one binade
    assert np.all(np.abs(f32[0].astype(np.float64) - whole.astype(np.float64)) <= 2 * np.spacing(np.abs(f32[0])))


def test_case_lists_cover_every_value_and_every_row_tail():
    want = {"post_mfma": ({1, 15, 17, 64, 65, 255, 256}, {1, 7, 8, 9, 33}, {1, 127, 128, 129, 300}, 128),
            "post_vec32": ({257, 300, 512}, {1, 63, 64, 65, 130}, {1, 31, 32, 33, 100}, 32),
            "post_vec16": ({513, 1024}, {1, 63, 64, 65, 130}, {1, 15, 16, 17, 100}, 16)}
    total = 0
    for fam, (ks, ds, ns, rows_per_block) in want.items():
        cases = fc.POSTERIOR_CASES[fam]
        total += len(cases)
        assert {c[0] for c in cases} == ks and {c[1] for c in cases} == ds and {c[2] for c in cases} == ns
        assert any(c[2] % rows_per_block and c[2] > rows_per_block for c in cases)      # a partial block after a full one
    assert 20 <= total <= 30
    assert sum(K <= 256 for K, _, _ in fc.EXTRA_SHAPES) == 1 and len(fc.EXTRA_SHAPES) == 2


def test_components_overlap_on_every_shape():
    """A condition on the inputs: with one-hot posteriors the tests would see nothing.  At least half of the rows have a largest
    responsibility below 0.9, for every (K, D) of the standard families (a mixture of one component is one-hot by definition)."""
    shapes = {(K, D) for fam in ("post_mfma", "post_vec32", "post_vec16") for K, D, _ in fc.POSTERIOR_CASES[fam]}
    shapes |= set(fc.VECTOR_SHAPES) | set(fc.MFMA_SHAPES) | set(fc.SCALE_SHAPES) | {(3, 2), (257, 2), fc.BYTES_SHAPE}
    for K, D in sorted(shapes):
        if K == 1:
            continue
        tab = fc.gmm_tables(K, D)
        top = orc.gmm_predict_proba(fc.draw(tab, 400, seed=5), *tab).max(axis=1)
        assert np.mean(top < 0.9) >= 0.5, (K, D, float(np.mean(top < 0.9)))


@need_extended
def test_far_rows_underflow_to_zero_outside_the_denormal_window():
    """Far rows: many responsibilities underflow.  The inputs keep every twin value out of the window in which a float64
    result is a denormal, so a correct float64 path gives exactly 0.0 wherever the twin is below 1e-320."""
    lo, hi = fc.DENORMAL_WINDOW
    for K, D, n in fc.EXTRA_SHAPES:
        tab, x, ref = fc.posterior_case("post_far", K, D, n)
        assert np.count_nonzero(ref < hi) > ref.size // 8
        assert not np.any((ref >= lo) & (ref < hi))
        assert np.all(orc.gmm_predict_proba(x, *tab)[ref < hi] == 0.0)


def test_duplicated_components_are_duplicates():
    for K, D, n in fc.EXTRA_SHAPES:
        w, mu, cov = fc.gmm_tables(K, D, dup=True)
        assert w[0] == w[K - 1] and np.array_equal(mu[0], mu[K - 1]) and np.array_equal(cov[0], cov[K - 1])
        w, mu, cov = fc.gmm_tables(K, D, floor=True)
        assert 0.2 < np.mean(cov == 1e-6) < 0.4


def test_seam_inputs_cross_their_seams():
    c = fc.seam_counts()
    assert len(c) == 65540 > 65535 and tuple(c[65533:65538]) == (3, 0, 5, 1, 4) and set(c[:65533]) == {0, 1, 2}
    K = fc.BYTES_SHAPE[0]
    per_image = 4096 + fc.BYTES_ROWS * K * 8                      # launch_fisher's accounting of one image
    assert 3 * per_image <= (3 << 30) < 4 * per_image and fc.BYTES_IMAGES == 5


@need_extended
@pytest.mark.parametrize("family", sorted(fc.POSTERIOR_CASES))
def test_posterior_dev_ref_is_under_the_cap(family):
    ref = fc.posterior_dev_ref(family)
    print(f"dev_ref {family}: {ref:.3g}  -> tolerance {fc.posterior_tol(family):.3g}")
    assert 16 * ref <= fc.DEV_REF_CAP


@need_extended
@pytest.mark.parametrize("family", sorted(fc.fisher_families()))
def test_fisher_dev_ref_is_under_the_cap(family):
    ref = fc.fisher_dev_ref(family)
    print(f"dev_ref {family}: {ref:.3g}  -> tolerance {fc.fisher_tol(family):.3g}")
    assert 16 * ref <= fc.DEV_REF_CAP


@pytest.mark.parametrize("Din,C", fc.PCA_SHAPES)
def test_pca_twin_bounds_the_float32_oracle(Din, C):
    comp, mean = fc.pca_tables(Din, C)
    x = fc.pca_rows(Din, 65)
    ref, mag = fnp.pca_transform(x, comp, mean)
    err = np.abs(orc.pca_transform(x, comp, mean).astype(fnp.REAL) - ref)
    assert np.all(err <= (Din + 2) * 2.0 ** -24 * mag)
