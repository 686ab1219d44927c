"""CPU tests of the keypoint SIFT extractor: the NumPy twin (tests/sift_numpy.py) is Lowe's SIFT on inputs with known answers,
the yardsticks and the decision band that tests/test_gpu_sift.py holds the device to (float32 twin against float64 twin, no code
under test involved), and the host side of the new API.

Measured with the float64 twin (asserted below with margin): an isolated Gaussian blob of std b at a sub-pixel centre gives its
strongest keypoint within 0.031 pixels of the centre (b = 2, 3, 4.5; bound 0.06) with sigma = size / 2 between 0.879 b and
0.885 b (bound: within 3 % of the closed form).  The closed form for a DoG with layer ratio k = 2^(1/3) is sigma = b / sqrt(k) =
0.891 b: the response 1 / (b^2 + k^2 s^2) - 1 / (b^2 + s^2) of a Gaussian blob peaks at s^2 = b^2 / k.  The issue quotes
"scale ~ sqrt(2) b"; no quantity of this definition equals that (size = 2 sigma = 1.77 b is 25 % above it), so the test
asserts the closed form, which is tighter, and additionally that size lies within 30 % of sqrt(2) b."""
import numpy as np
import pytest

import sift_numpy as tw


def _strongest(t):
    return t.frames[int(np.argmax(t.frames[:, 4]))]


@pytest.mark.parametrize("b,cy,cx", [(2.0, 60.8, 66.4), (3.0, 47.3, 50.6), (4.5, 60.8, 66.4)])
def test_twin_finds_a_blob_at_its_centre_and_scale(b, cy, cx):
    t = tw.sift(tw.blob_image(128, 128, cy, cx, b), tw.DEFAULT, np.float64)
    assert len(t.rows) >= 1
    f = _strongest(t)
    err = float(np.hypot(f[0] - cx, f[1] - cy))
    ratio = f[2] / 2.0 / b
    print(f"blob b={b}: centre error {err:.4f} px (bound 0.06), sigma / b = {ratio:.4f} (closed form {2 ** (-1 / 6):.4f}, bound 3 %), "
          f"size / (sqrt(2) b) = {f[2] / (np.sqrt(2.0) * b):.3f}")
    assert err <= 0.06
    assert abs(ratio / 2 ** (-1.0 / 6.0) - 1.0) <= 0.03
    assert abs(f[2] / (np.sqrt(2.0) * b) - 1.0) <= 0.30
    if b < 3.0:          # sigma = 0.89 b is below layer 1 of the first octave (1.6 * 2^(1/3)) unless the image is enlarged
        return
    # without the enlargement the same blob is found at the same place
    t1 = tw.sift(tw.blob_image(128, 128, cy, cx, b), tw.params(upsample=False), np.float64)
    f1 = _strongest(t1)
    assert np.hypot(f1[0] - cx, f1[1] - cy) <= 0.06 and abs(f1[2] / f[2] - 1.0) <= 0.03


def test_twin_finds_nothing_on_an_edge_a_constant_and_a_tiny_image():
    edge = np.full((80, 100), 50.0)
    edge[:, 47:] = 200.0
    assert len(tw.sift(edge, tw.DEFAULT, np.float64).rows) == 0            # the Hessian test rejects a straight edge
    assert len(tw.sift(edge.T.copy(), tw.DEFAULT, np.float32).rows) == 0
    for name in ("const", "tiny"):
        assert len(tw.twin64(name).rows) == 0 and len(tw.twin32(name).rows) == 0
    assert len(tw.twin64("tiny").pyr) == 0 and tw.n_octaves(14, 120) == 0 and tw.n_octaves(16, 120) == 1


def test_twin_rot90_rotates_the_keypoints():
    """Octave 0 only: the later octaves keep the even pixels, and x -> W0 - 1 - x maps even to odd, so only the first octave
    is sampled on a grid that the rotation maps onto itself."""
    rng = np.random.default_rng(5)
    h, w = 72, 90
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), 128.0)
    for _ in range(40):
        cy, cx, b = rng.uniform(8, h - 8), rng.uniform(8, w - 8), rng.uniform(0.9, 1.6)
        sy = rng.uniform(1.3, 2.0)                                          # elongated: a defined orientation
        img += rng.choice((-1.0, 1.0)) * 60.0 * np.exp(-((yy - cy) ** 2 / (2 * (b * sy) ** 2) + (xx - cx - 0.3 * (yy - cy)) ** 2 / (2 * b * b)))
    e = tw.yardsticks()
    a = tw.sift(img, tw.DEFAULT, np.float64)
    r = tw.sift(np.rot90(img).copy(), tw.DEFAULT, np.float64)
    w0 = 2 * w
    ka = {(i, w0 - 1 - x, y, (b - 9) % 36): j for j, (o, i, y, x, b) in enumerate(a.keys.tolist()) if o == 0}
    kr = {(i, y, x, b): j for j, (o, i, y, x, b) in enumerate(r.keys.tolist()) if o == 0}
    assert len(ka) >= 20
    odd = [k for k in set(ka) ^ set(kr)]
    # a float64 rotation differs from the original by rounding only: anything that flips must sit in the band
    for k in odd:
        j = ka.get(k)
        assert (tw.cand_excused(a.rows[j]["rec"], a.dog_max) or tw.bin_excused(a.rows[j]["rec"], a.rows[j]["key"][4])) if j is not None \
            else tw.cand_excused(r.rows[kr[k]]["rec"], r.dog_max) or tw.bin_excused(r.rows[kr[k]]["rec"], r.rows[kr[k]]["key"][4])
    worst_v = worst_a = 0.0
    for k in set(ka) & set(kr):
        ja, jr = ka[k], kr[k]
        da = (a.frames[ja, 3] - 90.0 - r.frames[jr, 3]) % 360.0
        worst_a = max(worst_a, min(da, 360.0 - da))
        worst_v = max(worst_v, float(np.abs(a.v[ja] - r.v[jr]).max()))
        assert abs(a.frames[ja, 1] - r.frames[jr, 0]) <= 1e-9 and abs((w - 1 - a.frames[ja, 0]) - r.frames[jr, 1]) <= 1e-9
    print(f"rot90: {len(set(ka) & set(kr))} octave-0 keypoints, angle deviation {worst_a:.2e} deg, descriptor deviation {worst_v:.2e} "
          f"(E_desc = {e['desc']:.2e})")
    assert worst_a <= e["angle"] and worst_v <= e["desc"]


def test_yardsticks_are_small_and_printed():
    e = tw.yardsticks()
    print("yardsticks (float32 twin vs float64 twin):", {k: f"{v:.3e}" for k, v in e.items()})
    assert 0 < e["dog"] < 1e-4 and 0 < e["desc"] < 1e-3 and 0 < e["pos"] < 5e-3 and 0 < e["off"] < 5e-3
    assert 0 < e["angle"] < 0.05 and 0 < e["hist"] < 1e-3 and 0 < e["q"] < 1e-2 and e["scl"] < 1e-3


@pytest.mark.parametrize("name", list(tw.inputs()))
def test_float32_and_float64_twins_agree_outside_the_band(name):
    t64, t32 = tw.twin64(name), tw.twin32(name)
    only64, only32 = tw.compare_keys(t64, t32.keys)
    share = tw.band_share(t64)
    print(f"{name}: {len(t64.rows)} keypoints (float64), {len(t32.rows)} (float32), {len(t64.cands)} candidates incl. near ones, "
          f"band share {100 * share:.2f} %")
    assert not only64 and not only32
    assert share <= 0.05
    if name in tw.TEXTURED:
        assert len(t64.rows) >= 100
    if len(t64.rows):
        assert np.all(np.diff(t64.keys.view([("", np.int64)] * 5).ravel().argsort(kind="stable")) > 0)     # rows are in key order
        assert t64.u8.shape == (len(t64.rows), 128) and t64.u8.any()
    # uint8 rows of keypoints both twins found: at most one apart
    kb = {tuple(k): j for j, k in enumerate(t32.keys.tolist())}
    pairs = [(j, kb[tuple(k)]) for j, k in enumerate(t64.keys.tolist()) if tuple(k) in kb]
    if pairs:
        ja, jb = map(list, zip(*pairs))
        assert np.abs(t64.u8[ja].astype(int) - t32.u8[jb].astype(int)).max() <= 1


def test_nfeatures_keeps_the_strongest_in_order():
    img = tw.inputs()["tex_gray"]
    full = tw.twin64("tex_gray")
    part = tw.sift(img, tw.params(nfeatures=25), np.float64)
    assert len(part.rows) == 25
    resp = np.float32(full.frames[:, 4])
    order = sorted(range(len(resp)), key=lambda k: (-resp[k], k))[:25]
    assert np.array_equal(part.keys, full.keys[sorted(order)])


@pytest.mark.parametrize("case", tw.edge_cases(), ids=tw.case_id)
def test_edge_case_twins_agree_outside_the_band_and_yardsticks_are_printed(case):
    """Every case of tests/test_gpu_sift_edges.py: its own yardsticks (float32 twin against float64 twin of this input and these
    parameters), the two twins equal outside the band, and the band within its cap: empty on a planted input, 5 % on a texture."""
    name, prm = case
    e = tw.yardsticks(name, prm)
    t64, t32 = tw.twin64(name, prm), tw.twin32(name, prm)
    assert t64.e is e and tw.prm_key(t64.prm) == tw.prm_key(prm)
    only64, only32 = tw.compare_keys(t64, t32.keys)
    share = tw.band_share(t64)
    print(f"{tw.case_id(case)}: {len(t64.rows)} keypoints (float64), {len(t32.rows)} (float32), octaves {sorted(set(t64.keys[:, 0].tolist()))}, "
          f"blur radius {tw.blur_radius(prm)}, band share {100 * share:.2f} % (cap {100 * tw.band_cap(name):.0f} %)")
    print("    yardsticks:", {k: f"{v:.3e}" for k, v in e.items()})
    assert not only64 and not only32
    assert share <= tw.band_cap(name)
    if name == "thin":
        assert not t64.pyr and not t64.rows and not any(e.values())
        return
    assert len(t64.rows) >= (100 if name in tw.TEXTURED else 2)
    assert 0 < e["dog"] < 1e-4 and 0 < e["desc"] < 1e-3 and 0 < e["pos"] < 5e-3 and 0 < e["off"] < 5e-3          # sanity ceilings only
    assert 0 < e["angle"] < 0.05 and 0 < e["hist"] < 1e-3 and 0 < e["q"] < 1e-2 and 0 < e["scl"] < 1e-3 and 0 < e["contr"] < 1e-4
    kb = {tuple(k): j for j, k in enumerate(t32.keys.tolist())}
    ja, jb = map(list, zip(*[(j, kb[tuple(k)]) for j, k in enumerate(t64.keys.tolist()) if tuple(k) in kb]))
    assert np.abs(t64.u8[ja].astype(int) - t32.u8[jb].astype(int)).max() <= 1
    # the contrast line follows the case's parameters: a keypoint is at or above 255 C / L, a contrast reject below
    thr = float(np.float32(255.0 * prm.C / prm.L))
    assert all(abs(c["contr"]) >= thr for c in t64.cands if c["status"] == "keypoint")
    assert all(abs(c["contr"]) < thr for c in t64.cands if c["status"] == "contrast")


def test_default_cases_keep_their_yardsticks():
    """The default parameters on the six inputs share the yardsticks over those six, whatever else has been measured."""
    e = tw.yardsticks()
    for name in tw.inputs():
        assert tw.yardsticks(name) is e and tw.yardsticks(name, tw.params()) is e and tw.twin64(name).e is e
    assert tw.yardsticks("ladder") is not e and tw.yardsticks("tex_rgb", tw.params(sigma=1.2)) is not e
    assert set(tw.inputs()).isdisjoint(tw.edge_inputs())


def test_the_ladder_reaches_every_octave_and_seam():
    """What the ladder is planted for, from the float64 twin alone."""
    img = tw.image("ladder")
    assert img.shape == (64, 96) and img.dtype == np.float32 and np.array_equal(img, np.rint(img))
    t = tw.twin64("ladder")
    assert [g.shape[1:] for g in t.pyr] == [(128, 192), (64, 96), (32, 48), (16, 24)]
    for prm in (tw.DEFAULT, tw.params(n_octave_layers=2), tw.params(n_octave_layers=5)):
        tp = tw.twin64("ladder", prm)
        assert set(tp.keys[:, 0].tolist()) == {0, 1, 2, 3}, prm.L                  # every octave, the 16-row one included
        assert tw.band_share(tp) == 0.0
    assert set(tw.twin64("ladder", tw.params(upsample=False)).keys[:, 0].tolist()) == {0, 1, 2}
    at = {(o, y, x): i for o, i, y, x, _ in t.keys.tolist()}
    assert tw.LADDER_TILE_CORNER in at and tw.LADDER_TILE_CORNER[1] % tw.BLUR_TILE == 0 and tw.LADDER_TILE_CORNER[2] % tw.BLUR_TILE == 0
    assert tw.LADDER_MARGIN in at and tw.LADDER_MARGIN[1] == tw.BORDER             # on the margin itself
    assert tw.LADDER_ROW_11 in at and tw.LADDER_ROW_11[1] == 11
    (oa, ya, xa), (ob, yb, xb) = tw.LADDER_BLOCK_PAIR
    w0 = t.pyr[0].shape[2]
    assert oa == ob == 0 and at[(oa, ya, xa)] == at[(ob, yb, xb)]                  # one layer,
    assert (ya * w0 + xa) // tw.DETECT_BLOCK + 1 == (yb * w0 + xb) // tw.DETECT_BLOCK   # neighbouring detect blocks
    two_rows = sum(1 for c in t.cands if len(c.get("peaks", ())) >= 2)
    print(f"ladder: {len(t.rows)} rows of {sum(c['status'] == 'keypoint' for c in t.cands)} keypoints, {two_rows} with several orientations; "
          f"keys {t.keys.tolist()}")
    assert two_rows >= 6


def test_tiny_thin_odd_and_pair_are_what_they_are_planted_for():
    for name, shape in (("tiny8", (16, 16)), ("tiny8w", (16, 26))):
        t = tw.twin64(name)
        assert [g.shape[1:] for g in t.pyr] == [shape]                                # one octave of exactly 16 rows
        assert len(t.rows) == 2 and t.keys[0, :4].tolist() == t.keys[1, :4].tolist()  # one keypoint, two orientations
        assert tw.band_share(t) == 0.0
    assert tw.image("thin").shape == (7, 40) and not tw.twin64("thin").pyr and not tw.twin32("thin").rows
    odd = tw.twin64("odd")
    assert [g.shape[1] for g in odd.pyr] == [74, 37, 18] and [g.shape[2] for g in odd.pyr] == [106, 53, 26]
    assert 2 in odd.keys[:, 0]                                                        # keypoints beyond the odd octave that is halved
    odd1 = tw.twin64("odd", tw.params(upsample=False))
    assert [g.shape[1:] for g in odd1.pyr] == [(37, 53), (18, 26)] and 1 in odd1.keys[:, 0]
    pair = tw.twin32("pair")
    resp = np.float32(pair.frames[:, 4])
    print(f"pair: float32 responses {resp.tolist()}, keys {pair.keys.tolist()}")
    assert len(resp) == 4 and len(set(resp.tolist())) == 1                            # bit-equal: all four rows tie
    assert pair.keys[2, 3] - pair.keys[0, 3] == 2 * 48 and tw.band_share(tw.twin64("pair")) == 0.0


@pytest.mark.parametrize("name", ["ladder", "pair"])
def test_nfeatures_cuts_through_ties_in_row_order(name):
    """Every n up to the row count, with the cuts between the two rows of one keypoint and between the two equal blobs."""
    for dtype in (np.float64, np.float32):
        full = tw.sift(tw.image(name), tw.DEFAULT, dtype)
        m = len(full.rows)
        resp = np.float32(full.frames[:, 4])
        order = sorted(range(m), key=lambda k: (-resp[k], k))
        assert sum(resp[order[k]] == resp[order[k + 1]] for k in range(m - 1)) >= (3 if name == "pair" else 6)
        for n in range(1, m + 1):
            part = tw.sift(tw.image(name), tw.params(nfeatures=n), dtype)
            assert np.array_equal(part.keys, full.keys[sorted(order[:n])]), n
            assert np.array_equal(part.u8, full.u8[sorted(order[:n])]), n


def test_blur_radius_limits_of_the_cases():
    P = tw.params
    assert tw.blur_radius(tw.DEFAULT) == 13
    assert tw.blur_radius(P(sigma=4.1)) == tw.MAX_RADIUS == 32 and tw.blur_radius(P(sigma=4.15)) == 33
    wr = tw.BLUR_TILE + 2 * tw.MAX_RADIUS
    assert (wr * wr + wr * tw.BLUR_TILE) * 4 == 48 * 1024                              # tile + halo and the row pass: exactly 48 KiB
    assert tw.blur_radius(P(n_octave_layers=1)) == 45 and tw.blur_radius(P(n_octave_layers=1, sigma=1.15)) == 32
    assert len(tw.gaussian_taps(tw.layer_sigmas(P(sigma=4.1))[1][-1])) == 65


def test_host_api_validation_repr_and_symbols():
    from pvsim import CapacityError, _ffi
    from pvsim.engine import sift_workspace
    from pvsim.features import SIFT, KeypointRootSIFT, KeypointSIFT, RootSIFT
    for bad in (dict(nfeatures=-1), dict(nfeatures=1.5), dict(nfeatures=True), dict(n_octave_layers=0), dict(n_octave_layers=2.5),
                dict(contrast_threshold=-0.1), dict(contrast_threshold=float("nan")), dict(edge_threshold=0), dict(sigma=0),
                dict(sigma=float("inf")), dict(upsample=1)):
        with pytest.raises(ValueError):
            KeypointSIFT(**bad)
    fx = KeypointRootSIFT(nfeatures=500)
    assert fx.output_dim == 128 and fx.fused_rootsift and not getattr(KeypointSIFT(), "fused_rootsift", False)
    assert repr(fx) == ("KeypointRootSIFT(nfeatures=500, n_octave_layers=3, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6, "
                        "upsample=True, output_dim=128)")
    assert repr(KeypointSIFT(upsample=False)).startswith("KeypointSIFT(nfeatures=0,")
    try:
        import cv2  # noqa: F401
    except ImportError:
        for cls in (SIFT, RootSIFT):                                       # unchanged: OpenCV's classes still need OpenCV
            with pytest.raises(ImportError):
                cls()(np.zeros((32, 32, 3), np.uint8))
    lib = _ffi.lib()
    for sym in ("pvs_sift_dev", "pvs_sift_workspace"):
        assert sym in _ffi.SIGNATURES and hasattr(lib, sym)
    assert _ffi.PVS_ERR_CAPACITY == 6 and _ffi._EXC[6] is CapacityError and not issubclass(CapacityError, ValueError)
    nbytes, rows = sift_workspace(500, 600)
    assert 36e6 < nbytes < 42e6 and rows > 10000                           # ~ 40 MB of float32 over all octaves
    assert sift_workspace(7, 60) == (0, 0)
    with pytest.raises(ValueError):
        sift_workspace(0, 10)
    # without a device the entry point fails loudly before touching anything, and n_images == 0 is a no-op
    import ctypes as C
    total = C.c_int64(-7)
    assert lib.pvs_sift_dev(None, None, 0, None, None, 0, 0, 3, 0.04, 10.0, 1.6, 1, 0, None, 0, None, None, C.byref(total)) == _ffi.PVS_ERR_INVALID
