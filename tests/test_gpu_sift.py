"""GPU tests of the keypoint SIFT extractor (csrc/sift.hip) against the NumPy twin (tests/sift_numpy.py).

Tolerances come from the twin alone (tests/test_sift_host.py asserts them): the device finds the float64 twin's keypoints except
inside the decision band (every decision within 8 yardsticks of its threshold; at most 5 % of the twin's keypoints), matched
keypoints agree within 8 E_pos / 8 E_scl / 8 E_angle on the frames and 8 E_desc on the normalised rows, uint8 rows differ by at
most one and only inside the rounding band, and bits and order do not depend on the batch, the chunking or the run."""
import numpy as np
import pytest

import dsift_numpy as ds
import sift_numpy as tw

pytestmark = pytest.mark.gpu

U8, F32, F32_RAW = 0, 1, 2


def _extract(ctx, fx, images, out_kind=U8):
    rows, offs, n, total, _, h_off, frm = fx.device_descriptors(images, ctx, out_kind, frames=True)
    try:
        out = rows.download((total, 128), np.uint8 if out_kind == U8 else np.float32)
        frames = frm.download((total, 6), np.float32)
        d_off = offs.download((n + 1,), np.int64)
    finally:
        for b in (rows, offs, frm):
            b.free()
    assert np.array_equal(d_off, h_off) and d_off[-1] == total
    return out, frames, d_off


@pytest.mark.parametrize("name", list(tw.inputs()))
def test_device_matches_the_twin(gpu_ctx, name):
    from pvsim.features import KeypointSIFT
    e = tw.yardsticks()
    t = tw.twin64(name)
    fx = KeypointSIFT(ctx=gpu_ctx)
    img = tw.inputs()[name]
    u8, frames, _ = _extract(gpu_ctx, fx, [img], U8)
    v, frames_v, _ = _extract(gpu_ctx, fx, [img], F32)
    assert np.array_equal(frames.view(np.uint32), frames_v.view(np.uint32))
    if not len(t.rows):
        assert len(frames) == 0
        return
    idx, dev = tw.match_frames(t, frames)
    m = idx >= 0
    only_dev = [j for j in np.nonzero(~m)[0] if not tw.frame_excused(t, frames[j])]
    matched = set(idx[m].tolist())
    only_twin = [j for j in range(len(t.rows)) if j not in matched and not tw.row_excused(t, j)]
    share = tw.band_share(t)
    dv = float(np.abs(v[m].astype(np.float64) - t.v[idx[m]]).max())
    resp = float(np.abs(frames[m, 4] - t.frames[idx[m], 4]).max() / t.dog_max)
    print(f"{name}: device {len(frames)} rows, twin {len(t.rows)}, matched {int(m.sum())}, band share {100 * share:.2f} %; "
          f"position {dev['pos']:.2e} (8 E_pos = {8 * e['pos']:.2e}), size {dev['size']:.2e} (8 E_scl = {8 * e['scl']:.2e}), "
          f"angle {dev['angle']:.2e} (8 E_angle = {8 * e['angle']:.2e}), rows {dv:.2e} (8 E_desc = {8 * e['desc']:.2e}), "
          f"response {resp:.2e} (8 E_contr = {8 * e['contr']:.2e})")
    assert not only_dev and not only_twin                       # outside the band the two sets are equal
    assert share <= 0.05
    assert len(set(idx[m].tolist())) == int(m.sum())            # one twin row per device row
    assert np.all(np.diff(idx[m]) > 0)                          # and in the twin's order: the defined order
    assert dv <= 8 * e["desc"] and resp <= 8 * e["contr"]       # frames are within their bounds by the matching itself
    # uint8 rows: at most one apart, equal outside the rounding band, and the quantised v bit for bit
    sub = type("T", (), dict(v=t.v[idx[m]], v1=t.v1[idx[m]]))
    diff = np.abs(u8[m].astype(np.int32) - t.u8[idx[m]].astype(np.int32))
    excused = ds.excused_entries(sub, 8 * e["desc"])
    print(f"    uint8: {int(diff.astype(bool).sum())} entries differ, {int((diff.astype(bool) & ~excused).sum())} outside the band, "
          f"band share {100 * excused.mean():.2f} %")
    assert diff.max() <= 1 and not (diff.astype(bool) & ~excused).any()
    assert np.array_equal(u8, np.minimum(255.0, np.floor(512.0 * v.astype(np.float64) + 0.5)).astype(np.uint8))
    # the integer key of the matched twin rows never decreases along the device's rows (the refinement may change the layer, so
    # the frames alone only show the octave)
    keys = t.keys[idx[m]]
    packed = (((keys[:, 0] * 64 + keys[:, 1]) * 65536 + keys[:, 2]) * 65536 + keys[:, 3]) * 64 + keys[:, 4]
    assert np.all(np.diff(packed) >= 0) and np.all(np.diff(frames[:, 5]) >= 0)


@pytest.mark.parametrize("out_kind", [U8, F32, F32_RAW])
def test_batch_composition_chunking_and_reruns_give_the_same_bits(gpu_ctx, out_kind):
    from pvsim.engine import sift_workspace
    from pvsim.features import KeypointSIFT
    imgs = [im for im in tw.inputs().values() if im.ndim == 3 and im.dtype == np.uint8]      # tex_rgb, tiny, const
    imgs = imgs + [np.ascontiguousarray(imgs[0][:70, :95]), np.rint(ds.texture(110, 90, 51, 3)).astype(np.uint8)]
    fx = KeypointSIFT(ctx=gpu_ctx)
    rows, frames, off = _extract(gpu_ctx, fx, imgs, out_kind)
    again, frames2, off2 = _extract(gpu_ctx, fx, imgs, out_kind)
    assert rows.shape[0] > 200
    assert np.array_equal(rows.view(np.uint8), again.view(np.uint8)) and np.array_equal(frames.view(np.uint32), frames2.view(np.uint32))
    assert np.array_equal(off, off2)
    for i, im in enumerate(imgs):
        one, f1, _ = _extract(gpu_ctx, fx, [im], out_kind)
        assert np.array_equal(one.view(np.uint8), rows[off[i]:off[i + 1]].view(np.uint8)), i
        assert np.array_equal(f1.view(np.uint32), frames[off[i]:off[i + 1]].view(np.uint32)), i
    rev, frev, roff = _extract(gpu_ctx, fx, imgs[::-1], out_kind)
    assert np.array_equal(rev[roff[-2]:roff[-1]].view(np.uint8), rows[off[0]:off[1]].view(np.uint8))
    assert np.array_equal(frev[roff[0]:roff[1]].view(np.uint32), frames[off[-2]:off[-1]].view(np.uint32))
    if out_kind != U8:
        return
    # a batch beyond the 256 MiB pyramid budget runs in several chunks: same bytes per image
    big = np.rint(ds.texture(400, 520, 52, 3)).astype(np.uint8)
    per_image = sift_workspace(400, 520)[0]
    n = int((256 << 20) // per_image) + 3
    batch = [big] * (n - 1) + [imgs[0]]
    brow, bfrm, boff = _extract(gpu_ctx, fx, batch, U8)
    one, f1, _ = _extract(gpu_ctx, fx, [big], U8)
    assert len(one) > 500
    for i in (0, n - 3, n - 2):
        assert np.array_equal(brow[boff[i]:boff[i + 1]], one) and np.array_equal(bfrm[boff[i]:boff[i + 1]].view(np.uint32), f1.view(np.uint32)), i
    assert np.array_equal(brow[boff[n - 1]:boff[n]], rows[off[0]:off[1]])


def test_capacity_protocol_and_nfeatures(gpu_ctx):
    from pvsim import CapacityError
    from pvsim._ffi import PIX_U8_RGB
    from pvsim.features import KeypointSIFT
    imgs = [tw.inputs()["tex_rgb"], tw.inputs()["const"], np.rint(ds.texture(110, 90, 51, 3)).astype(np.uint8)]
    fx = KeypointSIFT(ctx=gpu_ctx)
    want, wfrm, off = _extract(gpu_ctx, fx, imgs, U8)
    total = int(off[-1])
    cap = total // 2
    flat = np.concatenate([im.reshape(-1) for im in imgs])
    hw = np.array([im.shape[:2] for im in imgs], np.int32)
    pix = gpu_ctx.buffer(flat.nbytes).upload(flat)
    rows = gpu_ctx.buffer(cap * 128 + 4096).fill_bytes(0xA5)          # guard bytes behind the capacity
    frm = gpu_ctx.buffer(cap * 24 + 4096).fill_bytes(0xA5)
    offs = gpu_ctx.buffer(4 * 8)
    big = gpu_ctx.buffer(total * 128)
    try:
        with pytest.raises(CapacityError) as err:
            gpu_ctx.sift_dev(pix.ptr, PIX_U8_RGB, hw, None, 0, 3, 0.04, 10.0, 1.6, True, U8, rows.ptr, cap, frm.ptr, offs.ptr)
        assert err.value.args[1] == total
        assert np.array_equal(offs.download((4,), np.int64), off)      # the true CSR, although the rows did not fit
        got = rows.download((cap * 128 + 4096,), np.uint8)
        assert np.array_equal(got[:cap * 128].reshape(cap, 128), want[:cap]) and (got[cap * 128:] == 0xA5).all()
        gf = frm.download((cap * 24 + 4096,), np.uint8)
        assert np.array_equal(gf[:cap * 24], wfrm[:cap].view(np.uint8).reshape(-1)) and (gf[cap * 24:] == 0xA5).all()
        assert gpu_ctx.sift_dev(pix.ptr, PIX_U8_RGB, hw, None, 0, 3, 0.04, 10.0, 1.6, True, U8, big.ptr, total, None, offs.ptr) == total
        assert np.array_equal(big.download((total, 128), np.uint8), want)
        # capacity 0 with null rows: a pure count
        with pytest.raises(CapacityError):
            gpu_ctx.sift_dev(pix.ptr, PIX_U8_RGB, hw, None, 0, 3, 0.04, 10.0, 1.6, True, U8, None, 0, None, offs.ptr)
    finally:
        for b in (pix, rows, frm, offs, big):
            b.free()
    # the extractor's own retry: a first guess that is too small
    small = KeypointSIFT(ctx=gpu_ctx)
    small._rows_per_pixel = 1e-6
    again, _, _ = _extract(gpu_ctx, small, imgs, U8)
    assert np.array_equal(again, want)
    # nfeatures = n: the n strongest rows of each image by response, ties by row order, in the defined order
    n = 40
    part, pfrm, poff = _extract(gpu_ctx, KeypointSIFT(nfeatures=n, ctx=gpu_ctx), imgs, U8)
    for i in range(len(imgs)):
        f = wfrm[off[i]:off[i + 1]]
        keep = sorted(sorted(range(len(f)), key=lambda k: (-f[k, 4], k))[:n])
        assert np.array_equal(part[poff[i]:poff[i + 1]], want[off[i]:off[i + 1]][keep]), i
        assert np.array_equal(pfrm[poff[i]:poff[i + 1]].view(np.uint32), f[keep].view(np.uint32)), i


def test_extractor_calls(gpu_ctx):
    from pvsim import synth
    from pvsim.features import KeypointRootSIFT, KeypointSIFT
    img = tw.inputs()["tex_gray"]
    d, r = KeypointSIFT(ctx=gpu_ctx), KeypointRootSIFT(ctx=gpu_ctx)
    frames, raw = r.detect_and_compute(img)
    assert raw.dtype == np.uint8 and raw.shape == (len(frames), 128) and frames.shape[1] == 6 and len(frames) >= 100
    assert np.array_equal(r.raw(img), raw) and np.array_equal(r.keypoints(img).view(np.uint32), frames.view(np.uint32))
    assert np.array_equal(d(img), raw.astype(np.float32))
    np.testing.assert_allclose(r(img), synth.rootsift(raw.astype(np.float32)), rtol=0, atol=1e-7)
    acc = d.descriptors(img, normalised=False)
    assert acc.shape == raw.shape and (acc >= 0).all() and acc.any()
    assert d(np.zeros((6, 40, 3), np.uint8)).shape == (0, 128) and d(tw.inputs()["const"]).shape == (0, 128)
    assert (frames[:, 0] >= 0).all() and (frames[:, 0] <= img.shape[1]).all() and (frames[:, 1] <= img.shape[0]).all()
    assert len(KeypointSIFT(upsample=False, ctx=gpu_ctx)(img)) > 0
    with pytest.raises(NotImplementedError):
        KeypointSIFT(sigma=12.0, ctx=gpu_ctx)(img)                          # blur radius beyond the tile's halo


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
    from pvsim.features import KeypointRootSIFT
    rng = np.random.default_rng(3)
    km, gm, pca = _models(rng, c=32 if with_pca else None)
    fx = KeypointRootSIFT()
    if which == "vlad":
        enc = VLADEncoder(fx, kmeans_model=km, pca=pca, context=gpu_ctx)
    else:
        enc = FisherVectorEncoder(fx, gmm_model=gm, pca=pca, context=gpu_ctx)
    images = [tw.inputs()["tex_rgb"], np.rint(ds.texture(110, 90, 51, 3)).astype(np.uint8), tw.inputs()["tiny"], tw.inputs()["const"]]
    got = enc.encode(images)
    raws = [fx.raw(im) for im in images]
    assert raws[-1].shape == (0, 128) and raws[2].shape == (0, 128) and all(r.dtype == np.uint8 for r in raws)
    want = enc.encode_descriptors(raws, rootsift=True)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    assert not got[-1].any() and not got[2].any() and got[0].any()           # no keypoints -> a zero encoding row
    one = enc.encode(images[0])
    assert np.array_equal(one[0].view(np.uint8), got[0].view(np.uint8))
    mixed = [images[0], tw.inputs()["tex_gray"], images[1]]                  # gray and colour in one list, from a generator
    got_mixed = enc.encode(im for im in mixed)
    for i, im in enumerate(mixed):
        assert np.array_equal(got_mixed[i].view(np.uint8), enc.encode([im])[0].view(np.uint8)), i


def test_learn_then_encode_and_strict_compat(gpu_ctx):
    from pvsim.encoders import FisherVectorEncoder, VLADEncoder
    from pvsim.features import KeypointRootSIFT, KeypointSIFT
    rng = np.random.default_rng(4)
    km, gm, _ = _models(rng)
    train = [np.rint(ds.texture(120, 150, 60 + i, 3)).astype(np.uint8) for i in range(4)]
    for fx in (KeypointRootSIFT(), KeypointSIFT()):
        enc = VLADEncoder(fx, kmeans_model=km, context=gpu_ctx)
        enc.learn(train, n_clusters=16, random_state=0)
        out = enc.encode(train)
        assert out.shape == (4, 16 * 128) and np.isfinite(out).all() and out.any(axis=1).all()
        ref = enc.encode_descriptors([fx(im) for im in train])
        np.testing.assert_allclose(out, ref, rtol=0, atol=2e-6)
    fenc = FisherVectorEncoder(KeypointRootSIFT(), gmm_model=gm, context=gpu_ctx)
    fenc.learn(train, n_clusters=16, random_state=0, max_iter=5)
    fout = fenc.encode(train)
    assert fout.shape == (4, 16 + 2 * 16 * 128) and np.isfinite(fout).all()
    q = VLADEncoder(KeypointRootSIFT(), kmeans_model=km, context=gpu_ctx, strict_compat=True).encode([train[0], tw.inputs()["const"]])
    assert q.shape == (16 * 128,) and not q.any()                            # the reference's single zero vector (vlad.py:92-93)


def test_files_to_index_to_retrieval(gpu_ctx, tmp_path):
    from PIL import Image
    import pvsim.index as pindex
    from pvsim.encoders import VLADEncoder
    from pvsim.eval import retrieve_top_k_similar
    from pvsim.features import KeypointRootSIFT
    rng = np.random.default_rng(6)
    km, _, _ = _models(rng)
    enc = VLADEncoder(KeypointRootSIFT(), kmeans_model=km, context=gpu_ctx)
    imgs = [np.rint(ds.texture(110 + 6 * i, 140, 70 + i, 3)).astype(np.uint8) for i in range(6)]
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
    for i, im in enumerate(imgs):
        top = retrieve_top_k_similar(im, index, enc, k=3)
        assert top[0][0] == paths[i], (i, top)


def test_shipped_vocabulary_end_to_end(gpu_ctx):
    import warnings
    from pvsim.encoders import KMeansWeights, VLADEncoder
    from pvsim.features import KeypointRootSIFT
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                       # the stand-in table announces itself
        enc = VLADEncoder(KeypointRootSIFT(), weights=KMeansWeights.OXFORD102_K256_ROOTSIFT, context=gpu_ctx)
    imgs = [np.rint(ds.texture(120, 150, 80 + i, 3)).astype(np.uint8) for i in range(5)]
    out = enc.encode(imgs)
    assert out.shape[0] == 5 and np.isfinite(out).all() and out.any(axis=1).all()
    s = gpu_ctx.cosine(out, out)
    np.testing.assert_allclose(np.diag(s), 1.0, rtol=0, atol=1e-5)
    assert (s - np.eye(5)).max() < 0.999
