"""CPU tests of the dense SIFT extractor's host side: the public classes, the grid arithmetic of pvs_dsift_count /
pvs_dsift_frames, argument validation, the NumPy twin's own checks (the yardstick E, the input conditions, the mirror
property) and the Pillow decoding path of generate_encoding_map.  Nothing here needs a GPU."""
import numpy as np
import pytest

import dsift_numpy as tw


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def test_public_classes_exist_and_mirror_the_sift_pair(monkeypatch):
    import sys
    monkeypatch.setitem(sys.modules, "cv2", None)
    from pvsim.features import DenseRootSIFT, DenseSIFT, RootSIFT, SIFT
    from pvsim._base_classes import FeatureExtractorBase
    d, r = DenseSIFT(), DenseRootSIFT()
    assert isinstance(d, FeatureExtractorBase) and isinstance(r, DenseSIFT)
    assert d.output_dim == 128 and r.output_dim == 128
    assert (d.step, d.sizes, d.contrast_threshold) == (16, (4, 8), 0.0)
    assert r.fused_rootsift is True and RootSIFT.fused_rootsift is True and not getattr(d, "fused_rootsift", False)
    assert callable(r.raw) and callable(d.device_descriptors)
    n = d.count(500, 600)
    assert n == tw.count(500, 600, 16, (4, 8)) and 1500 < n < 2500          # near the ~1257 rows per image of the sizing
    with pytest.raises(ImportError):                                          # keypoint SIFT still needs OpenCV
        SIFT()(np.zeros((32, 32, 3), np.uint8))


@pytest.mark.parametrize("h,w,step,sizes", [(500, 600, 16, (4, 8)), (45, 140, 8, (4, 6, 8, 10)), (97, 131, 3, (6,)),
                                            (19, 19, 1, (4,)), (18, 40, 4, (4,)), (30, 30, 7, (8, 4, 16)), (39, 38, 5, (8,))])
def test_count_and_frames_follow_the_grid_rule(h, w, step, sizes):
    from pvsim.features import DenseSIFT
    d = DenseSIFT(step=step, sizes=sizes)
    ref = tw.frames(h, w, step, sizes)
    assert d.count(h, w) == len(ref) == tw.count(h, w, step, sizes)
    f = d.frames(h, w)
    assert f.dtype == np.float32 and f.shape == (len(ref), 3)
    np.testing.assert_array_equal(f, ref)
    for s in sizes:                                   # the closed form of the issue, and supports inside the image
        nx = (w - 5 * s + 1) // step + 1 if w >= 5 * s - 1 else 0
        ny = (h - 5 * s + 1) // step + 1 if h >= 5 * s - 1 else 0
        assert int((ref[:, 2] == s).sum()) == nx * ny
        sel = ref[ref[:, 2] == s]
        if len(sel):
            x0, y0 = sel[:, 0] - 1.5 * s, sel[:, 1] - 1.5 * s
            assert x0.min() - s + 1 >= 0 and x0.max() + 4 * s - 1 <= w - 1
            assert y0.min() - s + 1 >= 0 and y0.max() + 4 * s - 1 <= h - 1
            assert w - 1 - (x0.max() + 4 * s - 1) < step                  # no further origin would fit


def test_argument_validation():
    from pvsim._errors import InvalidImageError
    from pvsim.features import DenseRootSIFT, DenseSIFT
    for bad in (0, -3, 1.5):
        with pytest.raises(ValueError):
            DenseSIFT(step=bad)
    with pytest.raises(ValueError):
        DenseSIFT(sizes=())
    for bad in ((0,), (4, -1), (2.5,)):
        with pytest.raises(ValueError):
            DenseRootSIFT(sizes=bad)
    with pytest.raises(ValueError):
        DenseSIFT(contrast_threshold=-1.0)
    # the C entry points refuse the same arguments
    from pvsim import engine
    with pytest.raises(ValueError):
        engine.dsift_count(100, 100, 0, (4,))
    with pytest.raises(ValueError):
        engine.dsift_count(100, 100, 4, ())
    with pytest.raises(ValueError):
        engine.dsift_count(100, 100, 4, (4, 0))
    with pytest.raises(ValueError):
        engine.dsift_count(100, 100, 4, (2 ** 30,))
    assert engine.dsift_count(100, 100, 2 ** 31 - 1, (4, 8)) == 2       # any step beyond the image: one origin per axis
    # images are validated before anything touches the device
    for fx in (DenseSIFT(), DenseRootSIFT()):
        with pytest.raises(InvalidImageError):
            fx(np.zeros((40, 40, 4), np.uint8))
        with pytest.raises(InvalidImageError):
            fx(np.full((40, 40, 3), 300.0, np.float32))
        with pytest.raises(InvalidImageError):
            fx(np.full((40, 40), 0.5, np.float32))
        with pytest.raises(InvalidImageError):
            fx.raw(np.full((40, 40, 3), -1.0, np.float32))
    import torch
    with pytest.raises(TypeError):
        DenseSIFT()(torch.zeros(40, 40, 3))


def test_twin_yardstick_and_input_conditions():
    """E and E_raw (float32 twin against float64 twin), and the conditions the device comparisons rest on: 8 E < 1e-4, weak
    rows <= 5 % of an input's rows, excused uint8 entries <= 5 %, every float32-vs-float64 uint8 mismatch inside the band."""
    e, e_raw = tw.yardsticks()
    print(f"E = {e:.3e}  E_raw = {e_raw:.3e}")
    assert 0 < e and 8 * e < 1e-4
    assert 0 < e_raw < 1e-5
    seen_zero = seen_weak = seen_small = False
    for name, sizes, step in tw.cases():
        if True:
            img = tw.inputs()[name]
            t64, t32 = tw.twin_pair(name, sizes, step)
            assert t64.raw.shape[0] == tw.count(img.shape[0], img.shape[1], step, sizes)
            if any(min(img.shape[:2]) < 5 * s - 1 for s in sizes):
                seen_small = True
            if t64.raw.shape[0] == 0:
                continue
            zero, weak, strong = tw.classify(t64.raw)
            seen_zero |= bool(zero.any()) and name != "const"
            seen_weak |= bool(weak.any())
            assert weak.mean() <= 0.05, (name, sizes, weak.mean())
            if name == "const":
                assert zero.all() and not t64.u8.any() and not t32.u8.any()
            keep = zero | strong
            excused = tw.excused_entries(t64, 8 * e)[keep]
            share = excused.mean()
            print(f"{name} sizes={sizes} step={step}: rows {len(zero)} zero {zero.sum()} weak {weak.sum()} excused {100 * share:.2f} %")
            assert share <= 0.05, (name, sizes, share)
            diff = np.abs(t64.u8[keep].astype(np.int32) - t32.u8[keep].astype(np.int32))
            assert diff.max() <= 1
            assert not (diff.astype(bool) & ~excused).any()
            assert not t32.raw[zero].any() and not t32.u8[zero].any()      # zero rows are zero in any arithmetic
    assert seen_zero and seen_weak and seen_small


def test_edge_yardstick_and_conditions():
    """E and E_raw over the edge cases of tests/test_gpu_dsift_edges.py alone, and what those comparisons rest on: the shapes are
    the edges they are named for, no weak rows outside `rect`, excused uint8 entries <= 5 %, every float32-vs-float64 uint8
    mismatch inside the band."""
    e, e_raw = tw.edge_yardsticks()
    d, d_raw = tw.yardsticks()
    print(f"edge cases: E = {e:.3e}  E_raw = {e_raw:.3e}   (default cases: E = {d:.3e}  E_raw = {d_raw:.3e})")
    assert 0 < e and 8 * e < 1e-4                                            # sanity ceilings only
    assert 0 < e_raw < 1e-5
    assert set(tw.inputs()).isdisjoint(tw.edge_inputs())
    for name, sizes, step in tw.EDGE_CASES:
        img = tw.image(name)
        h, w = img.shape[:2]
        t64, t32 = tw.twin_pair(name, sizes, step)
        assert t64.raw.shape[0] == tw.count(h, w, step, sizes) > 0
        zero, weak, strong = tw.classify(t64.raw)
        assert name == "rect" or not (weak.any() or zero.any())
        keep = zero | strong
        excused = tw.excused_entries(t64, 8 * e)[keep]
        one_e, one_raw = tw._yardsticks(((name, sizes, step),))
        print(f"{name} sizes={sizes} step={step}: rows {len(zero)} weak {weak.sum()} E {one_e:.2e} E_raw {one_raw:.2e} "
              f"excused {100 * excused.mean():.2f} %")
        assert excused.mean() <= 0.05, (name, sizes)
        diff = np.abs(t64.u8[keep].astype(np.int32) - t32.u8[keep].astype(np.int32))
        assert diff.max() <= 1 and not (diff.astype(bool) & ~excused).any()
    rem = lambda name, s, step: tuple((x - 5 * s + 1) % step for x in tw.image(name).shape[:2])
    for name, s in (("e19x19", 4), ("e39x39", 8)):                           # exactly 5 s - 1: one descriptor, all four borders
        assert tw.image(name).shape[:2] == (5 * s - 1, 5 * s - 1) and tw.count(5 * s - 1, 5 * s - 1, 8, (s,)) == 1
    assert tw.image("e89x105").shape == (89, 105) and len(tw.grid(89, 18, 16)) == 1 and len(tw.grid(105, 18, 16)) == 2
    assert rem("e89x105", 18, 16) == (0, 0) and rem("e27x35", 4, 8) == (0, 0) and tw.count(27, 35, 8, (4,)) == 6
    assert rem("e75x83", 12, 8) == (0, 0) and rem("e87x95", 16, 8) == (0, 0)      # the single-descriptor regime, remainder 0
    assert tw.count(23, 31, 1, (1, 2, 3)) == 1085
    assert len(tw.grid(59, 4, 1)) > 8 * 4 and len(tw.grid(67, 12, 1)) == 9       # beyond the 8 x 8 tile cap; s = 12: one per tile
    assert len(tw.SIXTEEN) == 16 and min(tw.image("e83x90").shape) >= 5 * 16 - 1
    from pvsim import engine
    assert engine.dsift_count(83, 90, 8, tw.SIXTEEN) == tw.count(83, 90, 8, tw.SIXTEEN)
    with pytest.raises(NotImplementedError):
        engine.dsift_count(83, 90, 8, tuple(range(1, 18)))                        # DS_MAX_SIZES = 16


def test_contrast_threshold_sits_between_the_row_norms():
    thr, norms, band = tw.contrast_case()
    nz = np.sort(norms[norms > 0])
    near = float(np.abs(norms - thr).min())
    print(f"rect sizes (4, 8) step 8: {len(norms)} rows, norms 0 .. {norms.max():.1f}, quartiles of the non-zero ones "
          f"{np.quantile(nz, (0.25, 0.5, 0.75)).round(1).tolist()}; threshold {thr:.3f}, nearest norm {near:.3f} away, band {band:.4f}")
    assert near > band                                                        # no row of the twin may flip
    assert nz[len(nz) // 4 - 8] < thr < nz[len(nz) // 4 + 9]                  # about the lower quartile
    below = (norms <= thr) & (norms > 0)
    assert below.sum() >= len(nz) // 8 and (norms > thr).sum() >= len(nz) // 2
    for dtype in (np.float64, np.float32):
        t = tw.dense_sift(tw.image("rect"), 8, (4, 8), dtype, contrast_threshold=thr)
        assert np.array_equal(~t.v.any(axis=1), norms <= thr) and np.array_equal(~t.u8.any(axis=1), norms <= thr)
        assert t.raw.any(axis=1)[below].all()                                 # the accumulators are not touched


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_twin_mirror_property(dtype):
    """(W - 5 s + 1) % step == 0: the flipped image gives the same rows with x0 reversed, i -> 3 - i, o -> (4 - o) mod 8."""
    e, _ = tw.yardsticks()
    sizes, step, h, w = (4, 8), 4, 61, 83
    img = np.rint(tw.texture(h, w, 11, 3)).astype(np.uint8)
    a = tw.dense_sift(img, step, sizes, dtype)
    b = tw.dense_sift(img[:, ::-1], step, sizes, dtype)
    _, _, strong = tw.classify(tw.dense_sift(img, step, sizes, np.float64).raw)
    assert strong.all()
    pred = tw.mirror_rows(a.v, h, w, step, sizes)
    dev = float(np.abs(pred.astype(np.float64) - b.v).max())
    print(f"mirror deviation ({np.dtype(dtype).name}) = {dev:.3e}")
    assert dev <= (2 * e if dtype == np.float32 else 1e-12)


def test_encoder_cuts_its_input_lazily_and_by_kind():
    from pvsim.encoders._base_encoder import ImageEncoderBase
    pulled = []

    def gen():
        for i in range(600):
            pulled.append(i)
            yield np.zeros((8, 8) if i in (300, 301) else (8, 8, 3), np.uint8)

    it = ImageEncoderBase._image_chunks(gen())
    first = next(it)
    assert len(first) == 256 and len(pulled) == 257                     # nothing beyond the next image is decoded
    sizes = [len(first)] + [len(c) for c in it]
    assert sizes == [256, 44, 2, 256, 42] and len(pulled) == 600        # gray images form their own run
    big = [np.zeros((4096, 4096, 3), np.uint8)] * 3                     # 192 MiB each as float32: one per run
    assert [len(c) for c in ImageEncoderBase._image_chunks(big)] == [1, 1, 1]


def test_generate_encoding_map_decodes_with_pillow_when_cv2_is_absent(tmp_path, monkeypatch):
    import sys
    from PIL import Image
    from pvsim.encoders import VLADEncoder
    from pvsim.features import Lambda
    from pvsim.models import KMeansModel
    monkeypatch.setitem(sys.modules, "cv2", None)             # `import cv2` raises ImportError, whether OpenCV is installed or not
    rng = np.random.default_rng(5)
    imgs = [rng.integers(0, 256, size=(20 + 3 * i, 31, 3), dtype=np.uint8) for i in range(3)]
    paths = []
    for i, im in enumerate(imgs):
        p = str(tmp_path / f"im{i}.png")
        Image.fromarray(im).save(p)
        paths.append(p)
    gray_path = str(tmp_path / "gray.png")                  # a gray file is widened to RGB, as imread does
    Image.fromarray(imgs[0][:, :, 0]).save(gray_path)
    enc = VLADEncoder(Lambda(lambda im: np.zeros((1, 8), np.float32), 8), kmeans_model=KMeansModel(np.eye(8, dtype=np.float32)))
    seen = []

    def fake_encode(images):
        got = list(images)
        seen.extend(got)
        return np.arange(len(got), dtype=np.float32)[:, None] * np.ones((1, 4), np.float32)

    monkeypatch.setattr(enc, "encode", fake_encode)
    out = enc.generate_encoding_map(paths + [gray_path])
    assert list(out) == paths + [gray_path]
    for im, got in zip(imgs, seen):
        assert got.dtype == np.uint8 and np.array_equal(got, im)
    assert np.array_equal(seen[3], np.repeat(imgs[0][:, :, :1], 3, axis=2))
    assert [float(v[0]) for v in out.values()] == [0.0, 1.0, 2.0, 3.0]
