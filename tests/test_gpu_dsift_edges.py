"""GPU tests of the dense SIFT extractor (csrc/dsift.hip) at its edges, against the NumPy twin (tests/dsift_numpy.py): images one
descriptor fits exactly (the support touches all four borders), remainder 0 on both axes in the tiled and in the single-descriptor
LDS regime, bin sizes 1 to 3, step 1 across the tile cap, sixteen sizes, a contrast threshold between the row norms of an image, and
more images than one launch's grid.y holds.

The rule is the one of tests/test_gpu_dsift.py with the yardsticks of the edge cases (tw.edge_yardsticks(): float32 twin against
float64 twin over tw.EDGE_CASES; tests/test_dsift_host.py asserts and prints them): 8 E on the normalised rows of the strong rows,
8 E_raw of the image's largest accumulator on the raw accumulators, uint8 rows at most one apart and equal outside the rounding
band, exact zeros on zero rows."""
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


def _compare(ctx, label, img, sizes, step, t64, threshold=0.0, flips=None):
    """The assertions of test_gpu_dsift.test_device_matches_the_twin, with the edge yardsticks.  `flips`: rows whose zeroing by the
    contrast threshold may differ from the twin's (None: none may)."""
    from pvsim.features import DenseSIFT
    e, e_raw = tw.edge_yardsticks()
    fx = DenseSIFT(step=step, sizes=sizes, contrast_threshold=threshold, ctx=ctx)
    raw, _ = _extract(ctx, fx, [img], DSIFT_F32_RAW)
    v, _ = _extract(ctx, fx, [img], DSIFT_F32)
    u8, _ = _extract(ctx, fx, [img], DSIFT_U8)
    assert raw.shape == v.shape == u8.shape == t64.raw.shape and len(raw) == fx.count(*img.shape[:2]) > 0
    zero, weak, strong = tw.classify(t64.raw)
    gone = ~t64.v.any(axis=1)                                       # zero rows and rows at or below the threshold
    same = np.ones(len(raw), dtype=bool) if flips is None else ~flips
    sure = same & ~weak                                             # a weak row is held to its raw accumulators only
    assert np.array_equal(~v.any(axis=1)[sure], gone[sure]) and np.array_equal(~u8.any(axis=1)[sure], gone[sure])
    top = float(np.abs(t64.raw).max())
    dev_raw = float(np.abs(raw.astype(np.float64) - t64.raw).max()) / top
    cmp = strong & ~gone & same
    dev_v = float(np.abs(v[cmp].astype(np.float64) - t64.v[cmp]).max())
    print(f"{label}: {len(raw)} rows, raw deviation {dev_raw:.3e} (8 E_raw = {8 * e_raw:.3e}), "
          f"normalised deviation {dev_v:.3e} (8 E = {8 * e:.3e})")
    assert dev_raw <= 8 * e_raw
    assert dev_v <= 8 * e
    assert not raw[zero].any() and not v[gone & same].any() and not u8[gone & same].any()
    keep = (zero | strong) & same
    diff = np.abs(u8[keep].astype(np.int32) - t64.u8[keep].astype(np.int32))
    excused = tw.excused_entries(t64, 8 * e)[keep]
    print(f"    uint8: {int(diff.astype(bool).sum())} entries differ, {int((diff.astype(bool) & ~excused).sum())} outside the band, "
          f"band share {100 * excused.mean():.2f} %")
    assert diff.max() <= 1
    assert not (diff.astype(bool) & ~excused).any()
    assert excused.mean() <= 0.05
    assert np.array_equal(u8, np.minimum(255.0, np.floor(512.0 * v.astype(np.float64) + 0.5)).astype(np.uint8))
    return fx, v


@pytest.mark.parametrize("name,sizes,step", tw.EDGE_CASES, ids=[f"{n}-s{'_'.join(map(str, s)) if len(s) < 5 else '1to16'}-step{st}"
                                                                 for n, s, st in tw.EDGE_CASES])
def test_device_matches_the_twin_at_edge_shapes(gpu_ctx, name, sizes, step):
    img = tw.image(name)
    t64, _ = tw.twin_pair(name, sizes, step)
    fx, _ = _compare(gpu_ctx, f"{name} sizes={sizes} step={step}", img, sizes, step, t64)
    if sizes == tw.SIXTEEN:
        # rows ordered by (size, y0, x0): the frames say so, and the twin's rows were compared in that order above
        f = fx.frames(*img.shape[:2])
        assert np.array_equal(f, tw.frames(img.shape[0], img.shape[1], step, sizes))
        assert sorted(set(f[:, 2].tolist())) == [float(s) for s in sizes] and np.all(np.diff(f[:, 2]) >= 0)


def test_seventeen_sizes_are_refused(gpu_ctx):
    from pvsim.features import DenseSIFT
    with pytest.raises(NotImplementedError):
        DenseSIFT(step=8, sizes=tuple(range(1, 18)), ctx=gpu_ctx)(tw.image("e83x90"))


def test_contrast_threshold_between_the_row_norms(gpu_ctx):
    thr, norms, band = tw.contrast_case()
    img = tw.image("rect")
    t = tw.dense_sift(img, 8, (4, 8), np.float64, contrast_threshold=thr)
    flips = np.abs(norms - thr) <= band                       # only these may be zeroed differently: none (tests/test_dsift_host.py)
    assert not flips.any()
    gone = ~t.v.any(axis=1)
    print(f"threshold {thr:.3f}: {int(gone.sum())} of {len(norms)} rows zeroed ({int((norms == 0).sum())} of norm 0), nearest norm "
          f"{np.abs(norms - thr).min():.3f} away, band {band:.3f}")
    _, v = _compare(gpu_ctx, f"rect sizes=(4, 8) step=8 threshold={thr:.3f}", img, (4, 8), 8, t, threshold=thr, flips=flips)
    assert np.array_equal(~v.any(axis=1), norms <= thr)      # zeroed rows are exactly zero, kept rows are not


def test_more_images_than_one_launch_holds(gpu_ctx):
    """65,537 packed 19 x 19 uint8 gray images in one pvs_dsift_dev call: grid.y holds 65,535, so images 65,535 and 65,536 run in
    a second launch (img0 = 65,535).  One repeated image, distinct textures on either side of the seam and at index 0."""
    from pvsim._ffi import PIX_U8_GRAY
    from pvsim.features import DenseSIFT
    n, h, w = 65537, 19, 19
    rep = tw.image("e19x19")
    special = {i: np.rint(tw.texture(h, w, 71 + k, 1)).astype(np.uint8) for k, i in enumerate((0, 65534, 65535, 65536))}
    flat = np.tile(rep.reshape(-1), n).reshape(n, h * w)
    for i, im in special.items():
        flat[i] = im.reshape(-1)
    fx = DenseSIFT(step=8, sizes=(4,), ctx=gpu_ctx)
    want_rep, _ = _extract(gpu_ctx, fx, [rep], DSIFT_U8)
    assert want_rep.shape == (1, 128) and want_rep.any()
    pix = gpu_ctx.buffer(flat.nbytes).upload(flat.reshape(-1))
    rows = gpu_ctx.buffer(n * 128).fill_bytes(0xA5)
    offs = gpu_ctx.buffer((n + 1) * 8)
    try:
        gpu_ctx.dsift_dev(pix.ptr, PIX_U8_GRAY, np.tile(np.array([h, w], np.int32), (n, 1)), None, 8, (4,), 0.0, DSIFT_U8, rows.ptr, n,
                          offs.ptr)
        got = rows.download((n, 128), np.uint8)
        assert np.array_equal(offs.download((n + 1,), np.int64), np.arange(n + 1))
    finally:
        for b in (pix, rows, offs):
            b.free()
    distinct = {want_rep.tobytes()}
    for i, im in special.items():
        one, _ = _extract(gpu_ctx, fx, [im], DSIFT_U8)
        assert np.array_equal(got[i], one[0]), i
        distinct.add(one.tobytes())
    assert len(distinct) == 5                                  # a row in the wrong place would not go unnoticed
    for i in (1, 2, 32767, 32768, 65533):
        assert np.array_equal(got[i], want_rep[0]), i
    others = np.ones(n, dtype=bool)
    others[list(special)] = False
    assert (got[others] == want_rep[0]).all()
