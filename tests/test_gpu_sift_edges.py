"""GPU tests of the keypoint SIFT extractor (csrc/sift.hip) at its edges, against the NumPy twin (tests/sift_numpy.py): non-default
parameters, every octave of a planted input (blur tile corner, detect-block seam, the 5-pixel margin, a 16-pixel octave, an odd
octave that is halved), the largest supported blur, the chunk seam by image count, `nfeatures` cuts through ties, and batch
independence at non-default parameters.

The rule is the one of tests/test_gpu_sift.py.  A case is (input, parameters) and has its own yardsticks: its float32 twin against
its float64 twin (tests/test_sift_host.py asserts and prints them, with the band shares and the planted facts).  The device finds
the float64 twin's keypoints except inside the decision band (empty for the planted inputs, at most 5 % for textures), matched
keypoints agree within 8 E_pos / 8 E_scl / 8 E_angle / 8 E_contr on the frames and 8 E_desc on the normalised rows, uint8 rows differ
by at most one and only inside the rounding band."""
import numpy as np
import pytest

import dsift_numpy as ds
import sift_numpy as tw

pytestmark = pytest.mark.gpu

U8, F32, F32_RAW = 0, 1, 2


def _fx(ctx, prm, nfeatures=0):
    from pvsim.features import KeypointSIFT
    return KeypointSIFT(nfeatures=nfeatures, n_octave_layers=prm.L, contrast_threshold=prm.C, edge_threshold=prm.r, sigma=prm.sigma,
                        upsample=prm.upsample, ctx=ctx)


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


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8 if a.dtype == np.uint8 else np.uint32)


@pytest.mark.parametrize("case", tw.edge_cases(), ids=tw.case_id)
def test_device_matches_the_twin_at_every_case(gpu_ctx, case):
    name, prm = case
    img = tw.image(name)
    fx = _fx(gpu_ctx, prm)
    if tw.blur_radius(prm) > tw.MAX_RADIUS:                      # beyond the blur tile's halo: refused, not computed some other way
        with pytest.raises(NotImplementedError):
            fx(img)
        return
    e, t = tw.yardsticks(name, prm), tw.twin64(name, prm)
    u8, frames, _ = _extract(gpu_ctx, fx, [img], U8)
    v, frames_v, _ = _extract(gpu_ctx, fx, [img], F32)
    assert np.array_equal(_bits(frames), _bits(frames_v))
    if not len(t.rows):
        assert len(frames) == 0
        return
    idx, dev = tw.match_frames(t, frames, prm, e)
    m = idx >= 0
    only_dev = [j for j in np.nonzero(~m)[0] if not tw.frame_excused(t, frames[j], prm, e)]
    matched = set(idx[m].tolist())
    only_twin = [j for j in range(len(t.rows)) if j not in matched and not tw.row_excused(t, j, prm, e)]
    share = tw.band_share(t, prm, e)
    dv = float(np.abs(v[m].astype(np.float64) - t.v[idx[m]]).max())
    resp = float(np.abs(frames[m, 4] - t.frames[idx[m], 4]).max() / t.dog_max)
    print(f"{tw.case_id(case)}: device {len(frames)} rows, twin {len(t.rows)}, matched {int(m.sum())}, band share {100 * share:.2f} %; "
          f"position {dev['pos']:.2e} (8 E_pos = {8 * e['pos']:.2e}), size {dev['size']:.2e} (8 E_scl = {8 * e['scl']:.2e}), "
          f"angle {dev['angle']:.2e} (8 E_angle = {8 * e['angle']:.2e}), rows {dv:.2e} (8 E_desc = {8 * e['desc']:.2e}), "
          f"response {resp:.2e} (8 E_contr = {8 * e['contr']:.2e})")
    assert not only_dev and not only_twin                       # outside the band the two sets are equal
    assert share <= tw.band_cap(name)
    assert len(matched) == int(m.sum())                         # one twin row per device row
    assert np.all(np.diff(idx[m]) > 0)                          # and in the twin's order: the defined order
    assert dv <= 8 * e["desc"] and resp <= 8 * e["contr"]       # position, size and angle are within their bounds by the matching
    # uint8 rows: at most one apart, equal outside the rounding band, and the quantised v bit for bit
    sub = type("T", (), dict(v=t.v[idx[m]], v1=t.v1[idx[m]]))
    diff = np.abs(u8[m].astype(np.int32) - t.u8[idx[m]].astype(np.int32))
    excused = ds.excused_entries(sub, 8 * e["desc"])
    print(f"    uint8: {int(diff.astype(bool).sum())} entries differ, {int((diff.astype(bool) & ~excused).sum())} outside the band, "
          f"band share {100 * excused.mean():.2f} %")
    assert diff.max() <= 1 and not (diff.astype(bool) & ~excused).any()
    assert np.array_equal(u8, np.minimum(255.0, np.floor(512.0 * v.astype(np.float64) + 0.5)).astype(np.uint8))
    keys = t.keys[idx[m]]
    packed = (((keys[:, 0] * 64 + keys[:, 1]) * 65536 + keys[:, 2]) * 65536 + keys[:, 3]) * 64 + keys[:, 4]
    assert np.all(np.diff(packed) >= 0) and np.all(np.diff(frames[:, 5]) >= 0)
    # section 10 step 9 for this `upsample`, from the twin's octave coordinates: x = x_o 2^o / u - off, size = 2 scl 2^o / u
    u, off = (2.0, 0.25) if prm.upsample else (1.0, 0.0)
    o = keys[:, 0].astype(np.float64)
    sc = 2.0 ** o / u
    xo, yo, lay = t.oct_pos[idx[m]].T
    assert np.array_equal(frames[m, 5], o)
    ulp = np.spacing(np.abs(frames[m]))                         # frames are stored as float32
    assert np.all(np.abs(frames[m, 0] - (xo * sc - off)) <= 8 * e["pos"] * sc + ulp[:, 0])
    assert np.all(np.abs(frames[m, 1] - (yo * sc - off)) <= 8 * e["pos"] * sc + ulp[:, 1])
    size = 2.0 * prm.sigma * 2.0 ** (lay / prm.L) * sc
    assert np.all(np.abs(frames[m, 2] - size) <= 8 * e["scl"] * size + ulp[:, 2])
    if name not in tw.PLANTED:
        return
    # a planted input: every twin row is matched, so every octave the twin reports is there, and so are the planted keys
    assert matched == set(range(len(t.rows)))
    assert set(keys[:, 0].tolist()) == set(t.keys[:, 0].tolist())
    if name == "ladder":
        assert len(set(keys[:, 0].tolist())) == (4 if prm.upsample else 3)          # each octave of the ladder has a keypoint
        if prm.upsample:
            at = {(k[0], k[2], k[3]) for k in keys.tolist()}
            assert {tw.LADDER_TILE_CORNER, tw.LADDER_MARGIN, tw.LADDER_ROW_11, *tw.LADDER_BLOCK_PAIR} <= at


def test_a_sigma_just_above_the_supported_blur_is_refused(gpu_ctx):
    ok, over = tw.params(sigma=4.1), tw.params(sigma=4.15)
    assert tw.blur_radius(ok) == tw.MAX_RADIUS and tw.blur_radius(over) == tw.MAX_RADIUS + 1
    with pytest.raises(NotImplementedError):
        _fx(gpu_ctx, over)(tw.image("blobs43"))
    base_only = tw.params(sigma=8.3, n_octave_layers=8, upsample=False)               # only the base blur is too wide
    base, inc = tw.layer_sigmas(base_only)
    assert np.ceil(4.0 * base) > tw.MAX_RADIUS >= max(np.ceil(4.0 * s) for s in inc)
    with pytest.raises(NotImplementedError):
        _fx(gpu_ctx, base_only)(tw.image("blobs43"))


def test_chunk_seam_by_image_count(gpu_ctx):
    """1,030 images in one call: SF_CHUNK_IMAGES = 1024 cuts it into two chunks by count (the pyramids are far below the byte budget).
    8 x 8 images with four 150 x 110 textures at the first and last place of each chunk."""
    small = tw.image("tiny8")
    at = {0: tw.image("tex_gray").astype(np.float32)}
    for k, pos in enumerate((1023, 1024, 1029)):
        at[pos] = np.rint(ds.texture(150, 110, 90 + k, 1)).astype(np.float32)
    n = 1030
    batch = [at.get(i, small) for i in range(n)]
    fx = _fx(gpu_ctx, tw.DEFAULT)
    rows, frames, off = _extract(gpu_ctx, fx, batch, U8)
    one_small = _extract(gpu_ctx, fx, [small], U8)
    assert len(one_small[0]) == len(tw.twin64("tiny8").rows) == 2
    counts = np.diff(off)
    want = np.full(n, len(one_small[0]), dtype=np.int64)
    for i in sorted(set(at) | {1, 1022, 1025, 1028}):                                    # the four textures and their neighbours
        r1, f1, o1 = _extract(gpu_ctx, fx, [batch[i]], U8) if i in at else one_small
        want[i] = len(r1)
        assert np.array_equal(rows[off[i]:off[i + 1]], r1), i
        assert np.array_equal(_bits(frames[off[i]:off[i + 1]]), _bits(f1)), i
        assert off[i + 1] - off[i] == o1[1], i
        if i in at:
            assert len(r1) >= 100, i
    assert np.array_equal(counts, want)                                                  # every other image gave tiny8's two rows
    assert off[0] == 0 and np.array_equal(off[1:], np.cumsum(want))                      # the offsets are the running sum
    # and all copies of the small image gave the same rows
    k = len(one_small[0])
    others = np.array([i for i in range(n) if i not in at])
    got = np.stack([rows[off[i]:off[i] + k] for i in others])
    assert (got == one_small[0][None]).all()


@pytest.mark.parametrize("name", ["ladder", "pair"])
def test_nfeatures_cuts_through_ties_in_row_order(gpu_ctx, name):
    """Every n from 1 to the row count: the kept rows are the first n of the order (float32 response descending, row index
    ascending), returned in the defined order.  Two rows of one candidate always tie, and so do the two blobs of `pair`."""
    img = tw.image(name)
    full, ffrm, _ = _extract(gpu_ctx, _fx(gpu_ctx, tw.DEFAULT), [img], U8)
    m = len(full)
    assert m == len(tw.twin64(name).rows)
    resp = ffrm[:, 4]
    order = sorted(range(m), key=lambda k: (-resp[k], k))
    ties = sum(resp[order[k]] == resp[order[k + 1]] for k in range(m - 1))
    assert ties >= (3 if name == "pair" else 6)              # pair: all four rows tie; ladder: the second row of its two-row keypoints
    if name == "pair":
        assert len(set(resp.tolist())) == 1
    for n in range(1, m + 1):
        part, pfrm, _ = _extract(gpu_ctx, _fx(gpu_ctx, tw.DEFAULT, nfeatures=n), [img], U8)
        keep = sorted(order[:n])
        assert np.array_equal(part, full[keep]), n
        assert np.array_equal(_bits(pfrm), _bits(ffrm[keep])), n


@pytest.mark.parametrize("out_kind", [U8, F32, F32_RAW])
def test_batch_composition_and_reruns_give_the_same_bits_without_enlargement(gpu_ctx, out_kind):
    prm = tw.params(upsample=False, n_octave_layers=4)
    imgs = [im for im in tw.inputs().values() if im.ndim == 3 and im.dtype == np.uint8]      # tex_rgb, tiny, const
    imgs = imgs + [np.ascontiguousarray(imgs[0][:70, :95]), np.rint(ds.texture(110, 90, 51, 3)).astype(np.uint8)]
    fx = _fx(gpu_ctx, prm)
    rows, frames, off = _extract(gpu_ctx, fx, imgs, out_kind)
    again, frames2, off2 = _extract(gpu_ctx, fx, imgs, out_kind)
    assert rows.shape[0] > 100
    assert np.array_equal(_bits(rows), _bits(again)) and np.array_equal(_bits(frames), _bits(frames2))
    assert np.array_equal(off, off2)
    for i, im in enumerate(imgs):
        one, f1, _ = _extract(gpu_ctx, fx, [im], out_kind)
        assert np.array_equal(_bits(one), _bits(rows[off[i]:off[i + 1]])), i
        assert np.array_equal(_bits(f1), _bits(frames[off[i]:off[i + 1]])), i
    rev, frev, roff = _extract(gpu_ctx, fx, imgs[::-1], out_kind)
    assert np.array_equal(_bits(rev[roff[-2]:roff[-1]]), _bits(rows[off[0]:off[1]]))
    assert np.array_equal(_bits(frev[roff[0]:roff[1]]), _bits(frames[off[-2]:off[-1]]))
