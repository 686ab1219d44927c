"""The Fisher encoder (csrc/fisher.hip) against the long-double twin of tests/fisher_numpy.py on every kernel path and seam:
the MFMA and both vector posterior kernels row by row; the vector-FMA moments kernel (K > 256) at bt = 128 and 256; the MFMA
moments kernel at the D seams with all seven epilogue instantiations and all three PVS_OPT_FISHER_SCALE forms, float64 and float32
rows; the image-batch loop of launch_fisher past 65535 images and past 3 GiB of responsibilities; the RootSIFT and PCA
prologues at odd shapes; empty calls and refusals.

Inputs, case lists and tolerances come from tests/fisher_cases.py (tolerance of a family = max(project constant, 16 x dev_ref),
dev_ref = the float64 oracle's own deviation from the twin, computed on the CPU; tests/test_fisher_host.py prints them)."""
import ctypes as C

import numpy as np
import pytest

import fisher_cases as fc
import fisher_numpy as fnp
import pvsim_oracle as orc
from pvsim import _ffi, pack_descriptors
from pvsim.engine import DESC_F32, DESC_F32_ROOTSIFT, DESC_U8_ROOTSIFT

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not fnp.EXTENDED, reason=fnp.NEED_EXTENDED)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _posterior_dev(ctx, gm, x, kind=DESC_F32):
    """pvs_gmm_predict_proba_dev on host rows -> (n, K) float64; the output starts as NaN, so an unwritten entry shows."""
    with ctx.scratch() as tmp:
        d_x = tmp.upload(x)
        d_r = tmp(len(x) * gm.K * 8).fill_bytes(0xFF)
        ctx.gmm_predict_proba_dev(gm, d_x.ptr, kind, len(x), d_r.ptr)
        ctx.sync()
        return d_r.download((len(x), gm.K), np.float64)


def _fisher_dev(ctx, gm, packed, off, out_f64, kind=DESC_F32, power=0.5, order=2, eps=1e-9, pca=None, total=None):
    """pvs_fisher_encode_dev on host rows -> (n, L) float64 or float32; packed = None passes a null descriptor pointer."""
    off = np.ascontiguousarray(off, dtype=np.int64)
    n, L = len(off) - 1, gm.K + 2 * gm.K * gm.D
    dt = np.float64 if out_f64 else np.float32
    with ctx.scratch() as tmp:
        d_x = tmp.upload(packed) if packed is not None and packed.size else None
        d_off = tmp.upload(off)
        d_out = tmp(n * L * np.dtype(dt).itemsize).fill_bytes(0xFF)
        try:
            ctx.fisher_encode_dev(gm, None if d_x is None else d_x.ptr, kind, d_off.ptr, n, int(off[-1]) if total is None else total,
                                  d_out.ptr, int(out_f64), power, order, eps, pca)
        finally:
            ctx.sync()
        return d_out.download((n, L), dt)


def _pack(case, lo=0, hi=None):
    return pack_descriptors(case.imgs[lo:hi], case.D, np.float32)


def _check_f64(got, ref, tol, what):
    assert got.dtype == np.float64 and np.isfinite(got).all(), what
    err = float(np.abs(got.astype(fnp.REAL) - ref).max())
    assert err <= tol, f"{what}: |device - twin| = {err:.3g} > {tol:.3g}"


def _check_f32(got, restated, family, what):
    assert got.dtype == np.float32 and np.isfinite(got).all(), what
    excess = np.abs(got.astype(np.float64) - restated.astype(np.float64)) - fc.f32_tol(restated, family)
    assert excess.max() <= 0, f"{what}: float32 row off the restatement by {float(excess.max()):.3g} beyond the bound"


# ================================================================================ a. posterior rows
def _post_params(families):
    return [pytest.param(fam, *c, id=f"{fam[5:]}-K{c[0]}-D{c[1]}-n{c[2]}") for fam in families for c in fc.POSTERIOR_CASES[fam]]


@pytest.mark.parametrize("family,K,D,n", _post_params(("post_mfma", "post_vec32", "post_vec16", "post_floor")))
def test_posterior_rows_equal_the_twin(gpu_ctx, family, K, D, n):
    tab, x, ref = fc.posterior_case(family, K, D, n)
    r = _posterior_dev(gpu_ctx, gpu_ctx.gmm(*tab), x)
    _check_f64(r, ref, fc.posterior_tol(family), f"posterior K={K} D={D} n={n}")
    np.testing.assert_allclose(r.sum(axis=1), 1.0, rtol=0, atol=1e-12)


@pytest.mark.parametrize("K,D,n", fc.EXTRA_SHAPES, ids=["mfma", "vector"])
def test_posterior_of_far_rows_underflows_to_exact_zero(gpu_ctx, K, D, n):
    tab, x, ref = fc.posterior_case("post_far", K, D, n)
    r = _posterior_dev(gpu_ctx, gpu_ctx.gmm(*tab), x)
    _check_f64(r, ref, fc.posterior_tol("post_far"), "far rows")
    gone = ref < fc.DENORMAL_WINDOW[1]
    assert gone.sum() > ref.size // 8 and np.all(r[gone] == 0.0)
    np.testing.assert_allclose(r.sum(axis=1), 1.0, rtol=0, atol=1e-12)


@pytest.mark.parametrize("K,D,n", fc.EXTRA_SHAPES, ids=["mfma", "vector"])
def test_duplicated_components_get_the_same_bits(gpu_ctx, K, D, n):
    tab, x, ref = fc.posterior_case("post_dup", K, D, n)
    r = _posterior_dev(gpu_ctx, gpu_ctx.gmm(*tab), x)
    _check_f64(r, ref, fc.posterior_tol("post_dup"), "duplicated components")
    assert _same_bits(r[:, 0], r[:, K - 1])


# ================================================================================ b. Fisher rows on the vector path
@pytest.mark.parametrize("K,D,floor", [(K, D, False) for K, D in fc.VECTOR_SHAPES] + [(257, 33, True)],
                         ids=lambda v: str(v))
def test_vector_path_rows_equal_the_twin(gpu_ctx, K, D, floor):
    """fisher_moments_kernel<128|256, false> behind both posterior widths: ragged images against the twin on every element,
    float64 rows from the host entry and float32 rows from the device entry, and the same bits from two calls split at image 4."""
    case = fc.ragged_case(K, D, floor)
    family = "fisher_vector_floor" if floor else "fisher_vector"
    gm = gpu_ctx.gmm(*case.tab)
    packed, off = _pack(case)
    (pa, oa), (pb, ob) = _pack(case, 0, 4), _pack(case, 4)
    for p, o in ([(0.5, 2)] if floor else fc.VARIANTS_4):
        what = f"K={K} D={D} {fc.variant_id((p, o))}"
        f64 = gpu_ctx.fisher_encode(gm, packed, off, power=p, norm_order=o)
        _check_f64(f64, case.twin(p, o), fc.fisher_tol(family), what)
        f32 = _fisher_dev(gpu_ctx, gm, packed, off, 0, power=p, order=o)
        _check_f32(f32, case.twin_f32(p, o), family, what)
        assert not f64[0].any() and not f64[-1].any() and not f32[0].any() and not f32[-1].any()
        two = np.concatenate([gpu_ctx.fisher_encode(gm, pa, oa, power=p, norm_order=o), gpu_ctx.fisher_encode(gm, pb, ob, power=p, norm_order=o)])
        assert _same_bits(f64, two), what
        two = np.concatenate([_fisher_dev(gpu_ctx, gm, pa, oa, 0, power=p, order=o), _fisher_dev(gpu_ctx, gm, pb, ob, 0, power=p, order=o)])
        assert _same_bits(f32, two), what


# ================================================================================ c. Fisher rows on the MFMA path
@pytest.mark.parametrize("K,D", fc.MFMA_SHAPES, ids=lambda v: str(v))
def test_mfma_path_rows_equal_the_twin_in_every_epilogue(gpu_ctx, K, D):
    """2D against the 16-wide posterior chunks, the x | x**2 split, a partial last 32-dim moment block; p in {1, 0.5, 0.3} x
    order in {2, 1, 3} and +inf reach all seven (PM, NM) instantiations of the fused epilogue."""
    case = fc.ragged_case(K, D)
    gm = gpu_ctx.gmm(*case.tab)
    packed, off = _pack(case)
    for p, o in fc.VARIANTS_ALL:
        f64 = gpu_ctx.fisher_encode(gm, packed, off, power=p, norm_order=o)
        _check_f64(f64, case.twin(p, o), fc.fisher_tol("fisher_mfma"), f"K={K} D={D} {fc.variant_id((p, o))}")
        assert not f64[0].any() and not f64[-1].any()


@pytest.mark.parametrize("K,D", fc.SCALE_SHAPES, ids=lambda v: str(v))
def test_scale_forms_give_the_same_bits_in_both_row_types(gpu_ctx, K, D):
    """PVS_OPT_FISHER_SCALE in {0, 1, 2}.  The in-kernel form ends with a 16-byte in-place division that has an alignment
    branch and a scalar tail: with K = 41 and K = 7 the row length is odd, so most float32 rows start off a 16-byte boundary and
    the aligned ones end in a tail; (16, 32) keeps every row aligned with no tail; (255, 65) is long enough for the unrolled loop."""
    case = fc.ragged_case(K, D)
    gm = gpu_ctx.gmm(*case.tab)
    packed, off = _pack(case)
    for p, o in fc.VARIANTS_4:
        what = f"K={K} D={D} {fc.variant_id((p, o))}"
        rows = {}
        for form in (0, 1, 2):
            with gpu_ctx.option(_ffi.OPT_FISHER_SCALE, form):
                rows[form] = (_fisher_dev(gpu_ctx, gm, packed, off, 1, power=p, order=o), _fisher_dev(gpu_ctx, gm, packed, off, 0, power=p, order=o))
        for form in (1, 2):
            assert _same_bits(rows[0][0], rows[form][0]), f"{what}: float64 rows, form {form}"
            assert _same_bits(rows[0][1], rows[form][1]), f"{what}: float32 rows, form {form}"
        _check_f64(rows[2][0], case.twin(p, o), fc.fisher_tol("fisher_mfma"), what)
        _check_f32(rows[2][1], case.twin_f32(p, o), "fisher_mfma", what)


# ================================================================================ d. the batch seam at 65535 images
def _host_entry(ctx, gm, packed, off):
    """pvs_fisher_encode itself, in ONE call (Context.fisher_encode cuts a long list into calls of 32768 images)."""
    off = np.ascontiguousarray(off, dtype=np.int64)
    out = np.full((len(off) - 1, gm.K + 2 * gm.K * gm.D), np.nan)
    prm = _ffi.norm_params(0.5, 2, 1e-9)
    _ffi.check(_ffi.lib().pvs_fisher_encode(ctx.handle, gm.handle, None, _ffi.ptr(packed), DESC_F32, _ffi.ptr(off), len(off) - 1,
                                            C.byref(prm), _ffi.ptr(out)))
    return out


def _seam_halves(case):
    packed, off = pack_descriptors(case.imgs, case.D, np.float32)
    s = fc.SEAM_SPLIT
    return packed, off, (packed[:off[s]], off[:s + 1]), (packed[off[s]:], off[s:] - off[s])


def test_image_batch_seam_on_the_mfma_path(gpu_ctx):
    """65540 images in one call: the second batch of launch_fisher starts at image 65535 (resp - t0 * K, d_offsets + img0,
    out + img0 * L).  float64 rows from the host entry; the rows around the seam against the twin, all rows against two calls."""
    case = fc.seam_case(3, 2)
    gm = gpu_ctx.gmm(*case.tab)
    packed, off, a, b = _seam_halves(case)
    one = _host_entry(gpu_ctx, gm, packed, off)
    _check_f64(one[case.sel], case.twin(), fc.fisher_tol("fisher_seam_images"), "images around the seam")
    assert _same_bits(one, np.concatenate([_host_entry(gpu_ctx, gm, *a), _host_entry(gpu_ctx, gm, *b)]))


def test_image_batch_seam_on_the_vector_path(gpu_ctx):
    """The same 65540 images with K = 257: gridDim.z of the vector moments kernel is the batch.  float32 rows (337 MB)."""
    case = fc.seam_case(257, 2)
    gm = gpu_ctx.gmm(*case.tab)
    packed, off, a, b = _seam_halves(case)
    one = _fisher_dev(gpu_ctx, gm, packed, off, 0)
    _check_f32(one[case.sel], case.twin_f32(), "fisher_seam_images", "images around the seam")
    assert _same_bits(one[:fc.SEAM_SPLIT], _fisher_dev(gpu_ctx, gm, *a, 0))
    assert _same_bits(one[fc.SEAM_SPLIT:], _fisher_dev(gpu_ctx, gm, *b, 0))
    gpu_ctx.trim()


# ================================================================================ e. the batch seam at 3 GiB
def test_byte_budget_seam(gpu_ctx):
    """K = 1024, D = 2, five images of 100 000 descriptors: 0.82 GB of responsibilities each, so launch_fisher takes three images
    and then two, and image 3 is the first of a batch whose rows start 300 000 rows into the call.  It must equal itself encoded
    alone bit for bit, and the twin (accumulated in row blocks)."""
    case = fc.bytes_case()
    gm = gpu_ctx.gmm(*case.tab)
    packed, off = pack_descriptors(case.imgs, case.D, np.float32)
    joint = _fisher_dev(gpu_ctx, gm, packed, off, 1)
    alone = _fisher_dev(gpu_ctx, gm, packed[off[3]:off[4]], off[3:5] - off[3], 1)
    assert _same_bits(joint[3:4], alone)
    _check_f64(joint[3:4], case.twin(), fc.fisher_tol("fisher_seam_bytes"), "image 3")
    assert np.isfinite(joint).all() and len({r.tobytes() for r in joint}) == 5
    np.testing.assert_allclose(np.linalg.norm(joint, axis=1), 1.0, rtol=0, atol=1e-6)


# ================================================================================ f. descriptor kinds
@pytest.mark.parametrize("K,D", fc.KIND_SHAPES, ids=lambda v: str(v))
def test_descriptor_kinds_into_the_fisher_path(gpu_ctx, K, D):
    """materialise_kernel at D = 2, 65 and 130 (below, just above and twice the 64 lanes of its row loop), one all-zero row."""
    case = fc.kind_case(K, D)
    gm = gpu_ctx.gmm(*case.tab)
    raw = fc.kind_rows(D)
    off = np.concatenate(([0], np.cumsum(fc.RAGGED))).astype(np.int64)
    u8 = gpu_ctx.fisher_encode(gm, raw, off, kind=DESC_U8_ROOTSIFT)
    f32r = gpu_ctx.fisher_encode(gm, raw.astype(np.float32), off, kind=DESC_F32_ROOTSIFT)
    plain = gpu_ctx.fisher_encode(gm, orc.rootsift(raw.astype(np.float32)), off, kind=DESC_F32)
    ref = case.twin()
    for got, what in ((u8, "u8 RootSIFT"), (f32r, "f32 RootSIFT"), (plain, "f32")):
        _check_f64(got, ref, fc.fisher_tol("fisher_kinds"), f"K={K} D={D} {what}")
    assert _same_bits(u8, f32r)


# ================================================================================ g. PCA prologue
@pytest.mark.parametrize("Din,C_", fc.PCA_SHAPES, ids=lambda v: str(v))
def test_pca_transform_dev_within_the_float32_bound(gpu_ctx, Din, C_):
    """pca_kernel (64 x 64 tiles, 16-wide k steps) at partial tiles in every direction.  Bound of a float32 dot product of
    Din terms in any order, plus the subtraction and the rounding of the offset: (Din + 2) 2^-24 (sum |x||comp| + |off|)."""
    comp, mean = fc.pca_tables(Din, C_)
    p = gpu_ctx.pca(comp, mean)
    for n in fc.PCA_ROWS:
        x = fc.pca_rows(Din, n)
        with gpu_ctx.scratch() as tmp:
            d_out = tmp(n * C_ * 4).fill_bytes(0xFF)
            gpu_ctx.pca_transform_dev(p, tmp.upload(x).ptr, DESC_F32, n, d_out.ptr)
            gpu_ctx.sync()
            got = d_out.download((n, C_), np.float32)
        ref, mag = fnp.pca_transform(x, comp, mean)
        assert np.isfinite(got).all()
        assert np.all(np.abs(got.astype(fnp.REAL) - ref) <= (Din + 2) * 2.0 ** -24 * mag), (Din, C_, n)


def test_fisher_after_pca_equals_the_twin_on_the_device_projection(gpu_ctx):
    """130 -> 65, K = 41.  The twin takes the device's own projected rows, so the float32 GEMM does not enter the tolerance."""
    comp, mean, tab, rows = fc.pca_fisher_inputs()
    Din, C_, K = fc.PCA_FISHER
    p, gm = gpu_ctx.pca(comp, mean), gpu_ctx.gmm(*tab)
    with gpu_ctx.scratch() as tmp:
        d_out = tmp(len(rows) * C_ * 4)
        gpu_ctx.pca_transform_dev(p, tmp.upload(rows).ptr, DESC_F32, len(rows), d_out.ptr)
        gpu_ctx.sync()
        projected = d_out.download((len(rows), C_), np.float32)
    case = fc.FisherCase(tab, fc.split_ragged(projected))
    off = np.concatenate(([0], np.cumsum(fc.RAGGED))).astype(np.int64)
    got = gpu_ctx.fisher_encode(gm, rows, off, pca=p)
    _check_f64(got, case.twin(), fc.fisher_tol("fisher_pca"), "Fisher after PCA")
    assert _same_bits(got, gpu_ctx.fisher_encode(gm, projected, off))


# ================================================================================ h. small cases
@pytest.mark.parametrize("K", [16, 300])
def test_a_call_of_empty_images_gives_zero_rows(gpu_ctx, K):
    gm = gpu_ctx.gmm(*fc.gmm_tables(K, 5))
    off = np.zeros(8, np.int64)
    for out_f64 in (1, 0):
        rows = _fisher_dev(gpu_ctx, gm, None, off, out_f64)
        assert rows.shape == (7, K + 2 * K * 5) and not _bits(rows).any()


def test_more_than_1024_components_are_refused(gpu_ctx):
    tab = fc.gmm_tables(1025, 2)
    gm = gpu_ctx.gmm(*tab)
    x = fc.draw(tab, 40)
    off = np.array([0, 17, 40], np.int64)
    with pytest.raises(NotImplementedError, match="1025"):
        gpu_ctx.fisher_encode(gm, x, off)
    with pytest.raises(NotImplementedError, match="1025"):
        _posterior_dev(gpu_ctx, gm, x)
    case = fc.ragged_case(1024, 3)
    ok = gpu_ctx.fisher_encode(gpu_ctx.gmm(*case.tab), *_pack(case))
    _check_f64(ok, case.twin(), fc.fisher_tol("fisher_vector"), "a valid call after the refusals")


@pytest.mark.parametrize("K", [16, 300])
def test_bad_offsets_are_refused_before_any_launch(gpu_ctx, K):
    tab = fc.gmm_tables(K, 5)
    gm = gpu_ctx.gmm(*tab)
    x = fc.draw(tab, 12)
    L = K + 2 * K * 5
    for off, total in (([0, 5, 3, 10], 10), ([0, 5, 10], 12), ([1, 5, 12], 12)):
        off = np.array(off, np.int64)
        with gpu_ctx.scratch() as tmp:
            d_out = tmp((len(off) - 1) * L * 8).fill_bytes(0xFF)
            with pytest.raises(ValueError, match="offsets"):
                gpu_ctx.fisher_encode_dev(gm, tmp.upload(x).ptr, DESC_F32, tmp.upload(off).ptr, len(off) - 1, total, d_out.ptr, 1)
            gpu_ctx.sync()
            assert np.all(d_out.download(((len(off) - 1) * L * 8,), np.uint8) == 0xFF)       # nothing was written
    good = np.array([0, 5, 12], np.int64)
    np.testing.assert_allclose(_fisher_dev(gpu_ctx, gm, x, good, 1), orc.fisher_encode([x[:5], x[5:]], *tab), rtol=0, atol=fc.FISHER_ATOL)
