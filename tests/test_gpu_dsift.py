"""GPU tests of the dense SIFT extractor (csrc/dsift.hip) against the NumPy twin (tests/dsift_numpy.py).

Tolerances come from the twin alone: E / E_raw = float32 twin against float64 twin over all inputs (tests/test_dsift_host.py
asserts them and the input conditions); the device is held to 8 E on the normalised rows of the strong rows, 8 E_raw of the
image's largest accumulator on the raw accumulators of all rows, |diff| <= 1 on the uint8 rows with equality outside the
rounding band, and exact zeros on zero rows."""
import numpy as np
import pytest

import dsift_numpy as tw

pytestmark = pytest.mark.gpu

DSIFT_U8, DSIFT_F32, DSIFT_F32_RAW = 0, 1, 2


def _extract(ctx, fx, images, out_kind):
    rows, offs, n, total, _, h_off = fx.device_descriptors(images, ctx, out_kind)
    try:
        out = rows.download((total, 128), np.uint8 if out_kind == DSIFT_U8 else np.float32)
        d_off = offs.download((n + 1,), np.int64)
    finally:
        rows.free()
        offs.free()
    assert np.array_equal(d_off, h_off)
    return out, d_off


@pytest.mark.parametrize("name,sizes,step", tw.cases())
def test_device_matches_the_twin(gpu_ctx, name, sizes, step):
    from pvsim.features import DenseSIFT
    e, e_raw = tw.yardsticks()
    assert 8 * e < 1e-4
    img = tw.inputs()[name]
    fx = DenseSIFT(step=step, sizes=sizes, ctx=gpu_ctx)
    t64, _ = tw.twin_pair(name, sizes, step)
    raw, _ = _extract(gpu_ctx, fx, [img], DSIFT_F32_RAW)
    v, _ = _extract(gpu_ctx, fx, [img], DSIFT_F32)
    u8, _ = _extract(gpu_ctx, fx, [img], DSIFT_U8)
    assert raw.shape == v.shape == u8.shape == t64.raw.shape
    if t64.raw.shape[0] == 0:
        return
    zero, weak, strong = tw.classify(t64.raw)
    top = float(np.abs(t64.raw).max())
    dev_raw = float(np.abs(raw.astype(np.float64) - t64.raw).max()) / top if top > 0 else float(np.abs(raw).max())
    dev_v = float(np.abs(v[strong].astype(np.float64) - t64.v[strong]).max()) if strong.any() else 0.0
    print(f"{name} sizes={sizes} step={step}: raw deviation {dev_raw:.3e} (8 E_raw = {8 * e_raw:.3e}), "
          f"normalised deviation {dev_v:.3e} (8 E = {8 * e:.3e})")
    assert dev_raw <= 8 * e_raw
    assert dev_v <= 8 * e
    assert not raw[zero].any() and not v[zero].any() and not u8[zero].any()
    if name == "const":
        assert zero.all()
    keep = zero | strong
    diff = np.abs(u8[keep].astype(np.int32) - t64.u8[keep].astype(np.int32))
    excused = tw.excused_entries(t64, 8 * e)[keep]
    print(f"    uint8: {int(diff.astype(bool).sum())} entries differ, {int((diff.astype(bool) & ~excused).sum())} outside the band, "
          f"band share {100 * excused.mean():.2f} %")
    assert diff.max() <= 1
    assert not (diff.astype(bool) & ~excused).any()
    assert excused.mean() <= 0.05
    # the uint8 rows are the quantised normalised rows, bit for bit
    assert np.array_equal(u8, np.minimum(255.0, np.floor(512.0 * v.astype(np.float64) + 0.5)).astype(np.uint8))


@pytest.mark.parametrize("out_kind", [DSIFT_U8, DSIFT_F32, DSIFT_F32_RAW])
def test_batch_composition_and_reruns_give_the_same_bits(gpu_ctx, out_kind):
    from pvsim.features import DenseSIFT
    imgs = [im for im in tw.inputs().values() if im.ndim == 3 and im.dtype == np.uint8]      # rect, small, const: mixed sizes
    imgs = imgs + [np.ascontiguousarray(imgs[0][:50, :33])]                                      # 33 wide: no rows for s >= 8
    fx = DenseSIFT(step=8, sizes=(4, 6, 8, 10), ctx=gpu_ctx)
    batch, off = _extract(gpu_ctx, fx, imgs, out_kind)
    again, _ = _extract(gpu_ctx, fx, imgs, out_kind)
    assert np.array_equal(batch.view(np.uint8), again.view(np.uint8))
    assert off[-1] == batch.shape[0] == sum(fx.count(*im.shape[:2]) for im in imgs)
    for i, im in enumerate(imgs):
        one, _ = _extract(gpu_ctx, fx, [im], out_kind)
        assert np.array_equal(one.view(np.uint8), batch[off[i]:off[i + 1]].view(np.uint8)), i
    rev, roff = _extract(gpu_ctx, fx, imgs[::-1], out_kind)
    assert np.array_equal(rev[roff[-2]:roff[-1]].view(np.uint8), batch[off[0]:off[1]].view(np.uint8))


def test_pixel_offsets_huge_step_and_quantised_float_rows(gpu_ctx):
    """The C entry point with images NOT packed back to back (h_pix_offsets), a step far beyond the image (one origin per
    axis, tile choice must not overflow), and PVS_DSIFT_F32_QUANT = the uint8 rows as float32, bit for bit."""
    from pvsim._ffi import DSIFT_F32_QUANT, PIX_U8_RGB
    from pvsim.features import DenseSIFT
    imgs = [tw.inputs()["small"], tw.inputs()["rect"]]
    sizes, step = (4, 8), 8
    fx = DenseSIFT(step=step, sizes=sizes, ctx=gpu_ctx)
    want, off = _extract(gpu_ctx, fx, imgs, DSIFT_U8)
    quant, _ = _extract(gpu_ctx, fx, imgs, DSIFT_F32_QUANT)
    assert quant.dtype == np.float32 and np.array_equal(quant, want.astype(np.float32))
    gaps = [1000, 37]                                                   # bytes of filler in front of each image
    flat, offsets = [], []
    for gap, im in zip(gaps, imgs):
        flat.append(np.full(gap, 255, np.uint8))
        offsets.append(sum(len(f) for f in flat))
        flat.append(im.reshape(-1))
    flat = np.concatenate(flat)
    pix = gpu_ctx.buffer(flat.nbytes).upload(flat)
    rows = gpu_ctx.buffer(want.shape[0] * 128)
    offs = gpu_ctx.buffer(3 * 8)
    try:
        hw = np.array([im.shape[:2] for im in imgs], np.int32)
        gpu_ctx.dsift_dev(pix.ptr, PIX_U8_RGB, hw, np.array(offsets, np.int64), step, sizes, 0.0, DSIFT_U8, rows.ptr,
                          want.shape[0], offs.ptr)
        assert np.array_equal(rows.download(want.shape, np.uint8), want)
        assert np.array_equal(offs.download((3,), np.int64), off)
        with pytest.raises(ValueError):                                 # more rows than the output holds
            gpu_ctx.dsift_dev(pix.ptr, PIX_U8_RGB, hw, np.array(offsets, np.int64), step, sizes, 0.0, DSIFT_U8, rows.ptr,
                              want.shape[0] - 1, offs.ptr)
    finally:
        for b in (pix, rows, offs):
            b.free()
    far = DenseSIFT(step=2 ** 31 - 1, sizes=sizes, ctx=gpu_ctx)
    one, _ = _extract(gpu_ctx, far, [imgs[1]], DSIFT_U8)
    first = [0, fx.count(*imgs[1].shape[:2]) - len(tw.grid(imgs[1].shape[0], 8, step)) * len(tw.grid(imgs[1].shape[1], 8, step))]
    single, _ = _extract(gpu_ctx, fx, [imgs[1]], DSIFT_U8)
    assert one.shape == (2, 128) and np.array_equal(one, single[first])


def test_mirror_property_on_the_device(gpu_ctx):
    from pvsim.features import DenseSIFT
    e, _ = tw.yardsticks()
    sizes, step, h, w = (4, 8), 4, 61, 83
    img = np.rint(tw.texture(h, w, 11, 3)).astype(np.uint8)
    fx = DenseSIFT(step=step, sizes=sizes, ctx=gpu_ctx)
    a, _ = _extract(gpu_ctx, fx, [img], DSIFT_F32)
    b, _ = _extract(gpu_ctx, fx, [np.ascontiguousarray(img[:, ::-1])], DSIFT_F32)
    dev = float(np.abs(tw.mirror_rows(a, h, w, step, sizes).astype(np.float64) - b).max())
    print(f"mirror deviation on the device = {dev:.3e} (16 E = {16 * e:.3e})")
    assert dev <= 16 * e


def test_extractor_calls(gpu_ctx):
    from pvsim import synth
    from pvsim.features import DenseRootSIFT, DenseSIFT
    img = tw.inputs()["rect"]
    d, r = DenseSIFT(ctx=gpu_ctx), DenseRootSIFT(ctx=gpu_ctx)
    raw = r.raw(img)
    assert raw.dtype == np.uint8 and raw.shape == (d.count(*img.shape[:2]), 128) and raw.any()
    out = d(img)
    assert out.dtype == np.float32 and np.array_equal(out, raw.astype(np.float32))
    rs = r(img)
    assert rs.dtype == np.float32
    np.testing.assert_allclose(rs, tw.rootsift_tail(raw), rtol=0, atol=1e-7)
    np.testing.assert_allclose(rs, synth.rootsift(raw.astype(np.float32)), rtol=0, atol=1e-7)
    assert d(np.zeros((10, 10, 3), np.uint8)).shape == (0, 128)            # too small for every size
    thr = DenseSIFT(contrast_threshold=1e30, ctx=gpu_ctx)(img)              # everything below the threshold
    assert thr.shape == out.shape and not thr.any()
    with pytest.raises(NotImplementedError):
        DenseSIFT(sizes=(24,), ctx=gpu_ctx)(np.zeros((200, 200, 3), np.uint8))


def _models(rng, k=16, d=128, c=None):
    from pvsim.models import GMMModel, KMeansModel, PCAModel
    dim = c or d
    km = KMeansModel(rng.random((k, dim), dtype=np.float32) * 0.2)
    gm = GMMModel(np.full(k, 1.0 / k), rng.random((k, dim)) * 0.2, 0.01 + rng.random((k, dim)) * 0.02)
    pca = None
    if c:
        q, _ = np.linalg.qr(rng.standard_normal((d, c)))
        pca = PCAModel(q.T.astype(np.float32), np.full(d, 0.08, np.float32))
    return km, gm, pca


@pytest.mark.parametrize("with_pca", [False, True])
@pytest.mark.parametrize("which", ["vlad", "fisher"])
def test_device_handoff_equals_descriptor_entry_bit_for_bit(gpu_ctx, which, with_pca):
    from pvsim.encoders import FisherVectorEncoder, VLADEncoder
    from pvsim.features import DenseRootSIFT
    rng = np.random.default_rng(3)
    km, gm, pca = _models(rng, c=32 if with_pca else None)
    fx = DenseRootSIFT(step=8, sizes=(4, 8))
    if which == "vlad":
        enc = VLADEncoder(fx, kmeans_model=km, pca=pca, context=gpu_ctx)
    else:
        enc = FisherVectorEncoder(fx, gmm_model=gm, pca=pca, context=gpu_ctx)
    images = [tw.inputs()[n] for n in ("rect", "small", "const")] + [np.zeros((12, 300, 3), np.uint8)]   # the last has no rows
    got = enc.encode(images)
    raws = [fx.raw(im) for im in images]
    assert raws[-1].shape == (0, 128) and all(r.dtype == np.uint8 for r in raws)
    want = enc.encode_descriptors(raws, rootsift=True)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    assert not got[-1].any() and got[0].any()                              # no rows -> a zero encoding row
    one = enc.encode(images[0])
    assert np.array_equal(one[0].view(np.uint8), got[0].view(np.uint8))
    # gray and colour images in one list, from a generator: cut into runs by kind, same rows as one image at a time
    mixed = [images[0], tw.inputs()["odd_gray"], images[1]]
    got_mixed = enc.encode(im for im in mixed)
    for i, im in enumerate(mixed):
        assert np.array_equal(got_mixed[i].view(np.uint8), enc.encode([im])[0].view(np.uint8)), i


def test_strict_compat_quirk_and_learn(gpu_ctx):
    from pvsim.encoders import FisherVectorEncoder, VLADEncoder
    from pvsim.features import DenseRootSIFT, DenseSIFT
    rng = np.random.default_rng(4)
    km, gm, _ = _models(rng)
    images = [tw.inputs()["odd_gray"], np.zeros((10, 10), np.uint8)]
    enc = VLADEncoder(DenseRootSIFT(), kmeans_model=km, context=gpu_ctx, strict_compat=True)
    q = enc.encode(images)
    assert q.shape == (16 * 128,) and not q.any()                           # vlad.py:92-93
    with pytest.raises(ZeroDivisionError):
        FisherVectorEncoder(DenseRootSIFT(), gmm_model=gm, context=gpu_ctx, strict_compat=True).encode(images)
    assert VLADEncoder(DenseRootSIFT(), kmeans_model=km, context=gpu_ctx).encode(images).shape == (2, 16 * 128)
    # learn() on images, then encode: the documented use
    train = [np.rint(tw.texture(96, 128, 20 + i, 3)).astype(np.uint8) for i in range(4)]
    for fx in (DenseRootSIFT(step=8), DenseSIFT(step=8)):
        enc = VLADEncoder(fx, kmeans_model=km, context=gpu_ctx)
        enc.learn(train, n_clusters=16, random_state=0)
        out = enc.encode(train)
        assert out.shape == (4, 16 * 128) and np.isfinite(out).all() and out.any(axis=1).all()
        ref = enc.encode_descriptors([fx(im) for im in train])
        np.testing.assert_allclose(out, ref, rtol=0, atol=2e-6)
    fenc = FisherVectorEncoder(DenseRootSIFT(step=8), gmm_model=gm, context=gpu_ctx)
    fenc.learn(train, n_clusters=16, random_state=0, max_iter=5)
    fout = fenc.encode(train)
    assert fout.shape == (4, 16 + 2 * 16 * 128) and np.isfinite(fout).all()


def test_files_to_index_to_retrieval(gpu_ctx, tmp_path):
    from PIL import Image
    import pvsim.index as pindex
    from pvsim.encoders import VLADEncoder
    from pvsim.features import DenseRootSIFT
    rng = np.random.default_rng(6)
    km, _, _ = _models(rng)
    enc = VLADEncoder(DenseRootSIFT(step=8), kmeans_model=km, context=gpu_ctx)
    imgs = [np.rint(tw.texture(90 + 6 * i, 120, 40 + i, 3)).astype(np.uint8) for i in range(6)]
    enc.learn(imgs, n_clusters=16, random_state=0)
    paths = []
    for i, im in enumerate(imgs):
        paths.append(str(tmp_path / f"img{i}.png"))
        Image.fromarray(im).save(paths[-1])
    emap = enc.generate_encoding_map(paths)
    assert list(emap) == paths
    direct = enc.encode(imgs)
    for p, row in zip(paths, direct):
        assert np.array_equal(emap[p], row)
    index = pindex.DeviceIndex(emap, gpu_ctx)
    from pvsim.eval import retrieve_top_k_similar
    for i, im in enumerate(imgs):
        top = retrieve_top_k_similar(im, index, enc, k=3)
        assert top[0][0] == paths[i], (i, top)
