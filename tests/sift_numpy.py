"""NumPy statement of the keypoint SIFT definition, with the arithmetic dtype as a parameter.

Test infrastructure only: the package has no CPU path.  Lowe's algorithm (IJCV 2004) with OpenCV's parameter names and defaults,
NOT a bit-for-bit clone of cv2.SIFT (replicated borders, strict extrema, soft orientation binning, own octave count; see the
DESIGN section).  `sift(image, prm, dtype)` returns rows in the defined order (octave, layer, y, x of the integer extremum, peak
bin ascending), their frames (x, y, size, angle, response, octave) and integer keys, and the record of every candidate with the
margins of all its threshold decisions, from which `excused` builds the decision band of the float64 twin.

Also here: the seeded inputs shared by tests/test_sift_host.py and tests/test_gpu_sift.py, the yardsticks (float32 twin against
float64 twin) and the matching of a frame list without keys (the device's) against the float64 twin."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import dsift_numpy as ds

BORDER = 5            # extrema and refined positions stay this far from the octave's edge
MAX_STEPS = 5
MIN_OCTAVE = 16       # an octave exists while min(H_o, W_o) >= 16
BAND = 8.0            # decisions within BAND * yardstick of their threshold are excused
TWO_PI = 2.0 * np.pi


def params(nfeatures=0, n_octave_layers=3, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6, upsample=True):
    return SimpleNamespace(nfeatures=nfeatures, L=n_octave_layers, C=contrast_threshold, r=edge_threshold, sigma=sigma,
                           upsample=upsample)


DEFAULT = params()


# ------------------------------------------------------------------------------------------ pyramid
def upsample2(g: np.ndarray, dtype) -> np.ndarray:
    """2x bilinear enlargement: output pixel a samples the input at a / 2 - 0.25, clamped to the image."""
    def axis(n):
        s = np.clip((np.arange(2 * n, dtype=np.float64)) * 0.5 - 0.25, 0.0, n - 1.0)
        i0 = np.floor(s).astype(np.int64)
        return i0, np.minimum(i0 + 1, n - 1), (s - i0).astype(dtype)
    h, w = g.shape
    y0, y1, fy = axis(h)
    x0, x1, fx = axis(w)
    one = dtype(1.0)
    top = (one - fx)[None, :] * g[y0][:, x0] + fx[None, :] * g[y0][:, x1]
    bot = (one - fx)[None, :] * g[y1][:, x0] + fx[None, :] * g[y1][:, x1]
    return ((one - fy)[:, None] * top + fy[:, None] * bot).astype(dtype)


def gaussian_taps(sigma: float) -> np.ndarray:
    """float32 taps (normalised in float64), radius ceil(4 sigma)."""
    r = int(np.ceil(4.0 * sigma - 1e-12))
    d = np.arange(-r, r + 1, dtype=np.float64)
    t = np.exp(-d * d / (2.0 * sigma * sigma))
    return (t / t.sum()).astype(np.float32)


def blur(img: np.ndarray, sigma: float, dtype) -> np.ndarray:
    taps = gaussian_taps(sigma).astype(dtype)
    r = (len(taps) - 1) // 2
    h, w = img.shape
    p = np.pad(img, ((0, 0), (r, r)), mode="edge")
    acc = np.zeros((h, w), dtype=dtype)
    for k in range(2 * r + 1):
        acc += taps[k] * p[:, k:k + w]
    p = np.pad(acc, ((r, r), (0, 0)), mode="edge")
    out = np.zeros((h, w), dtype=dtype)
    for k in range(2 * r + 1):
        out += taps[k] * p[k:k + h, :]
    return out


def n_octaves(h0: int, w0: int) -> int:
    n = 0
    while (min(h0, w0) >> n) >= MIN_OCTAVE:
        n += 1
    return n


def layer_sigmas(prm):
    """(sigma of the base blur, incremental sigmas of layers 1 .. L + 2)."""
    assumed = 1.0 if prm.upsample else 0.5
    base = np.sqrt(max(prm.sigma ** 2 - assumed ** 2, 0.01))
    k = 2.0 ** (1.0 / prm.L)
    inc = [np.sqrt((prm.sigma * k ** i) ** 2 - (prm.sigma * k ** (i - 1)) ** 2) for i in range(1, prm.L + 3)]
    return base, inc


def pyramid(image: np.ndarray, prm, dtype):
    g = ds.gray(image, dtype).astype(dtype)
    if prm.upsample:
        g = upsample2(g, dtype)
    base, inc = layer_sigmas(prm)
    octs = []
    cur = blur(g, base, dtype)
    for _o in range(n_octaves(*g.shape)):
        layers = [cur]
        for s in inc:
            layers.append(blur(layers[-1], s, dtype))
        octs.append(np.stack(layers))
        h, w = cur.shape
        cur = np.ascontiguousarray(layers[prm.L][0:2 * (h // 2):2, 0:2 * (w // 2):2])
    return octs


# ------------------------------------------------------------------------------------------ detection
def _half_dist(x: float) -> float:
    """distance of x to the nearest half-integer"""
    return abs(x - (np.floor(x) + 0.5))


def _refine(D, i, y, x, prm, dtype, thr_c):
    """-> record fields of one candidate.  D: (L + 2, H, W) DoG of the octave in `dtype`; scalar arithmetic in `dtype`."""
    _, H, W = D.shape
    half, quarter, two = dtype(0.5), dtype(0.25), dtype(2.0)
    rec = dict(status="steps", visited=[(i, y, x)], m_off=np.inf)
    for _step in range(MAX_STEPS):
        v = D[i, y, x]
        dx = (D[i, y, x + 1] - D[i, y, x - 1]) * half
        dy = (D[i, y + 1, x] - D[i, y - 1, x]) * half
        dz = (D[i + 1, y, x] - D[i - 1, y, x]) * half
        dxx = D[i, y, x + 1] + D[i, y, x - 1] - two * v
        dyy = D[i, y + 1, x] + D[i, y - 1, x] - two * v
        dss = D[i + 1, y, x] + D[i - 1, y, x] - two * v
        dxy = (D[i, y + 1, x + 1] - D[i, y + 1, x - 1] - D[i, y - 1, x + 1] + D[i, y - 1, x - 1]) * quarter
        dxs = (D[i + 1, y, x + 1] - D[i + 1, y, x - 1] - D[i - 1, y, x + 1] + D[i - 1, y, x - 1]) * quarter
        dys = (D[i + 1, y + 1, x] - D[i + 1, y - 1, x] - D[i - 1, y + 1, x] + D[i - 1, y - 1, x]) * quarter
        c00 = dyy * dss - dys * dys
        c01 = dxs * dys - dxy * dss
        c02 = dxy * dys - dxs * dyy
        c11 = dxx * dss - dxs * dxs
        c12 = dxy * dxs - dxx * dys
        c22 = dxx * dyy - dxy * dxy
        det = dxx * c00 + dxy * c01 + dxs * c02
        if det == 0:
            rec["status"] = "singular"
            return rec
        inv = dtype(-1.0) / det
        X = ((c00 * dx + c01 * dy + c02 * dz) * inv, (c01 * dx + c11 * dy + c12 * dz) * inv,
             (c02 * dx + c12 * dy + c22 * dz) * inv)
        rec["m_off"] = min(rec["m_off"], min(_half_dist(float(t)) for t in X))
        if abs(X[0]) < half and abs(X[1]) < half and abs(X[2]) < half:
            rec["status"] = "converged"
            break
        if not all(abs(t) <= dtype(1048576.0) for t in X):      # also refuses NaN
            rec["status"] = "far"
            return rec
        x += int(np.floor(X[0] + half))
        y += int(np.floor(X[1] + half))
        i += int(np.floor(X[2] + half))
        if i < 1 or i > prm.L or x < BORDER or x > W - 1 - BORDER or y < BORDER or y > H - 1 - BORDER:
            rec["status"] = "left"
            return rec
        rec["visited"].append((i, y, x))
    else:
        return rec
    contr = v + half * (dx * X[0] + dy * X[1] + dz * X[2])
    tr = dxx + dyy
    det2 = dxx * dyy - dxy * dxy
    r = dtype(prm.r)
    q = tr * tr * r - dtype((prm.r + 1.0) ** 2) * det2
    rec.update(contr=float(contr), det2=float(det2), q=float(q), final=(i, y, x),
               X=tuple(float(t) for t in X), Xd=X)
    if not abs(contr) >= dtype(thr_c):
        rec["status"] = "contrast"
    elif det2 <= 0 or q >= 0:
        rec["status"] = "edge"
    else:
        rec["status"] = "keypoint"
    return rec


def _grad(G, y0, y1, x0, x1):
    """central differences (no 1/2) on the window rows y0..y1, cols x0..x1 (inclusive) of G; the window is interior"""
    gx = G[y0:y1 + 1, x0 + 1:x1 + 2] - G[y0:y1 + 1, x0 - 1:x1]
    gy = G[y0 + 1:y1 + 2, x0:x1 + 1] - G[y0 - 1:y1, x0:x1 + 1]
    return gx, gy


def _window(G, y, x, rad):
    H, W = G.shape
    y0, y1 = max(y - rad, 1), min(y + rad, H - 2)
    x0, x1 = max(x - rad, 1), min(x + rad, W - 2)
    return y0, y1, x0, x1


def _mag_theta(gx, gy, dtype):
    mag = np.sqrt(gx * gx + gy * gy)
    th = np.arctan2(gy, gx)
    th = np.where(th < 0, th + dtype(TWO_PI), th).astype(dtype)
    return mag, th


def _orientation(G, y, x, scl, dtype):
    """-> smoothed 36-bin histogram; soft binning between the two nearest bins, pixels in raster order"""
    rad = int(np.floor(dtype(4.5) * scl + dtype(0.5)))
    sw = dtype(1.5) * scl
    c = dtype(-1.0) / (dtype(2.0) * sw * sw)
    y0, y1, x0, x1 = _window(G, y, x, rad)
    raw = np.zeros(36, dtype=dtype)
    if y1 >= y0 and x1 >= x0:
        gx, gy = _grad(G, y0, y1, x0, x1)
        mag, th = _mag_theta(gx, gy, dtype)
        yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        d2 = ((xx - x) ** 2 + (yy - y) ** 2).astype(dtype)
        w = np.exp(d2 * c).astype(dtype)
        t = (th * dtype(36.0 / TWO_PI)).astype(dtype)
        b0 = np.floor(t)
        f = (t - b0).astype(dtype)
        b0 = b0.astype(np.int64) % 36
        wm = (w * mag).astype(dtype)
        np.add.at(raw, b0.ravel(), (wm * (dtype(1.0) - f)).ravel())
        np.add.at(raw, ((b0 + 1) % 36).ravel(), (wm * f).ravel())
    h = ((np.roll(raw, 2) + np.roll(raw, -2)) * dtype(1.0 / 16.0) + (np.roll(raw, 1) + np.roll(raw, -1)) * dtype(4.0 / 16.0)
         + raw * dtype(6.0 / 16.0)).astype(dtype)
    return h, rad


def _peaks(h, dtype):
    """-> [(bin index, interpolated bin)] ascending"""
    top = h.max()
    out = []
    for i in range(36):
        l, r = h[(i - 1) % 36], h[(i + 1) % 36]
        if h[i] > l and h[i] > r and h[i] >= dtype(0.8) * top:
            b = dtype(i) + dtype(0.5) * (l - r) / (l - dtype(2.0) * h[i] + r)
            if b < 0:
                b += dtype(36.0)
            if b >= 36:
                b -= dtype(36.0)
            out.append((i, b))
    return out


def _descriptor(G, y, x, scl, theta, dtype):
    """raw 128 accumulators, element (r * 4 + c) * 8 + o, pixels in raster order"""
    hw = dtype(3.0) * scl
    rad = int(np.floor(hw * dtype(np.sqrt(2.0) * 2.5) + dtype(0.5)))
    y0, y1, x0, x1 = _window(G, y, x, rad)
    acc = np.zeros(128, dtype=dtype)
    if y1 < y0 or x1 < x0:
        return acc
    ct, st = np.cos(theta).astype(dtype), np.sin(theta).astype(dtype)
    yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    dx, dy = (xx - x).astype(dtype), (yy - y).astype(dtype)
    c_rot = ((dx * ct + dy * st) / hw).astype(dtype)
    r_rot = ((dy * ct - dx * st) / hw).astype(dtype)
    rbin, cbin = r_rot + dtype(1.5), c_rot + dtype(1.5)
    inside = (rbin > -1) & (rbin < 4) & (cbin > -1) & (cbin < 4)
    gx, gy = _grad(G, y0, y1, x0, x1)
    mag, th = _mag_theta(gx, gy, dtype)
    w = np.exp((c_rot * c_rot + r_rot * r_rot) * dtype(-0.125)).astype(dtype)
    ob = ((th - theta) * dtype(8.0 / TWO_PI)).astype(dtype)
    ob = np.where(ob < 0, ob + dtype(8.0), ob).astype(dtype)
    ob = np.where(ob >= 8, ob - dtype(8.0), ob).astype(dtype)
    sel = inside.ravel()
    rbin, cbin, ob, v = rbin.ravel()[sel], cbin.ravel()[sel], ob.ravel()[sel], (w * mag).astype(dtype).ravel()[sel]
    r0, c0, o0 = np.floor(rbin), np.floor(cbin), np.floor(ob)
    fr, fc, fo = (rbin - r0).astype(dtype), (cbin - c0).astype(dtype), (ob - o0).astype(dtype)
    r0, c0, o0 = r0.astype(np.int64), c0.astype(np.int64), o0.astype(np.int64)
    one = dtype(1.0)
    # per pixel the eight contributions go to distinct elements, so a bin's sum runs over the pixels in raster order
    for dr in (0, 1):
        wr = fr if dr else one - fr
        for dc in (0, 1):
            wc = fc if dc else one - fc
            for do in (0, 1):
                wo = fo if do else one - fo
                rr, cc, oo = r0 + dr, c0 + dc, (o0 + do) % 8
                ok = (rr >= 0) & (rr < 4) & (cc >= 0) & (cc < 4)
                np.add.at(acc, ((rr * 4 + cc) * 8 + oo)[ok], (((v * wr).astype(dtype) * wc).astype(dtype) * wo).astype(dtype)[ok])
    return acc


def sift(image: np.ndarray, prm=DEFAULT, dtype=np.float64, tau: float = 0.0):
    """The extractor.  tau > 0 (absolute DoG tolerance) additionally records the pixels that miss the extremum test or the
    pre-threshold by less than tau: they become rejected candidates ("near") whose only purpose is the decision band."""
    dtype = np.dtype(dtype).type
    pyr = pyramid(image, prm, dtype)
    u = 2.0 if prm.upsample else 1.0
    pre = dtype(np.float32(0.5 * prm.C / prm.L * 255.0))
    thr_c = np.float32(255.0 * prm.C / prm.L)
    cands, dog_max = [], 0.0
    for o, G in enumerate(pyr):
        D = (G[1:] - G[:-1]).astype(dtype)
        dog_max = max(dog_max, float(np.abs(D).max()))
        _, H, W = D.shape
        if H < 2 * BORDER + 1 or W < 2 * BORDER + 1:
            continue
        ys, xs = slice(BORDER, H - BORDER), slice(BORDER, W - BORDER)
        for i in range(1, prm.L + 1):
            v = D[i, ys, xs]
            nmax = np.full(v.shape, -np.inf, dtype=dtype)
            nmin = np.full(v.shape, np.inf, dtype=dtype)
            for di in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        if di == 0 and dy == 0 and dx == 0:
                            continue
                        n = D[i + di, BORDER + dy:H - BORDER + dy, BORDER + dx:W - BORDER + dx]
                        np.maximum(nmax, n, out=nmax)
                        np.minimum(nmin, n, out=nmin)
            m_ext = np.where(v > 0, v - nmax, nmin - v)            # > 0: strict extremum of its sign
            m_pre = np.abs(v) - pre                                # > 0: passes the pre-threshold
            hit = (m_ext > -tau) & (m_pre > -tau)
            for yy, xx in zip(*np.nonzero(hit)):
                y, x = int(yy) + BORDER, int(xx) + BORDER
                rec = dict(key=(o, i, y, x), m_ext=float(m_ext[yy, xx]), m_pre=float(m_pre[yy, xx]))
                if m_ext[yy, xx] > 0 and m_pre[yy, xx] > 0:
                    rec.update(_refine(D, i, y, x, prm, dtype, thr_c))
                else:
                    rec.update(status="near", visited=[(i, y, x)])
                cands.append(rec)
    # orientation and descriptors
    rows = []
    for rec in cands:
        if rec["status"] != "keypoint":
            continue
        o, _, _, _ = rec["key"]
        i, y, x = rec["final"]
        X = rec["Xd"]
        scl = dtype(prm.sigma) * np.exp2((dtype(i) + X[2]) / dtype(prm.L)).astype(dtype)
        G = pyr[o][i]
        h, rad = _orientation(G, y, x, scl, dtype)
        rec.update(scl=float(scl), hist=h.astype(np.float64), m_rad=_half_dist(4.5 * float(scl)), peaks=[])
        xo, yo = dtype(x) + X[0], dtype(y) + X[1]
        scale = dtype(2.0 ** o)
        fx = xo * scale / dtype(u) - dtype(0.25 if prm.upsample else 0.0)
        fy = yo * scale / dtype(u) - dtype(0.25 if prm.upsample else 0.0)
        for b_i, b in _peaks(h, dtype):
            theta = b * dtype(TWO_PI / 36.0)
            raw = _descriptor(G, y, x, scl, theta, dtype)
            rec["peaks"].append(b_i)
            rows.append(dict(key=rec["key"] + (b_i,), rec=rec, raw=raw, oct_pos=(float(xo), float(yo), float(dtype(i) + X[2])),
                             frame=(float(fx), float(fy), float(dtype(2.0) * scl * scale / dtype(u)), float(b * dtype(10.0)),
                                    abs(rec["contr"]), float(o))))
    if prm.nfeatures and len(rows) > prm.nfeatures:
        order = sorted(range(len(rows)), key=lambda k: (-np.float32(rows[k]["frame"][4]), k))     # strongest first, ties by row order
        keep = sorted(order[:prm.nfeatures])
        rows = [rows[k] for k in keep]
    raw = np.array([r["raw"] for r in rows], dtype=dtype).reshape(-1, 128)
    v1, v = ds.normalise(raw, dtype)
    return SimpleNamespace(rows=rows, cands=cands, raw=raw, v1=v1, v=v, u8=ds.quantise(v), dog_max=dog_max, pyr=pyr, prm=prm,
                           keys=np.array([r["key"] for r in rows], dtype=np.int64).reshape(-1, 5),
                           frames=np.array([r["frame"] for r in rows], dtype=np.float64).reshape(-1, 6),
                           oct_pos=np.array([r["oct_pos"] for r in rows], dtype=np.float64).reshape(-1, 3))


# ------------------------------------------------------------------------------------------ inputs
def blob_image(h: int, w: int, cy: float, cx: float, b: float, amp: float = 120.0, base: float = 60.0) -> np.ndarray:
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return base + amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * b * b))


def blobs(h: int, w: int, seed: int, n: int = 40) -> np.ndarray:
    """float64 gray: Gaussian blobs of both signs, random sub-pixel centres and sizes"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 128.0)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    for _ in range(n):
        cy, cx, b = rng.uniform(8, h - 8), rng.uniform(8, w - 8), rng.uniform(1.5, 5.0)
        img += rng.choice((-1.0, 1.0)) * rng.uniform(30, 70) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * b * b))
    return np.clip(img, 0.0, 255.0)


@functools.lru_cache(maxsize=None)
def inputs():
    """name -> image: textured uint8 RGB (non-square) and uint8 gray, float32 RGB, float32 gray blobs (integer valued, as 2-D
    float images must be), one too small for any octave (7 rows: 14 < 16 after enlargement) and one constant."""
    return {
        "tex_rgb": np.rint(ds.texture(140, 190, 42, 3)).astype(np.uint8),
        "tex_gray": np.rint(ds.texture(150, 110, 32, 1)).astype(np.uint8),
        "f32_rgb": ds.texture(128, 170, 33, 3).astype(np.float32),
        "blobs_f32_gray": np.rint(blobs(128, 128, 34)).astype(np.float32),
        "tiny": np.rint(ds.texture(7, 60, 35, 3)).astype(np.uint8),
        "const": np.full((64, 90, 3), 117, dtype=np.uint8),
    }


TEXTURED = ("tex_rgb", "tex_gray", "f32_rgb")


def planted(h: int, w: int, blobs, base: float = 50.0) -> np.ndarray:
    """float32 gray, integer valued: slightly elongated (1.25 : 1), sheared (0.2) Gaussian blobs (cy, cx, std b, amplitude) on a
    flat ground.  The shear gives every blob a defined orientation, with two peaks in its histogram."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), base)
    for cy, cx, b, amp in blobs:
        img += amp * np.exp(-((yy - cy) ** 2 / (2.0 * (1.25 * b) ** 2) + (xx - cx - 0.2 * (yy - cy)) ** 2 / (2.0 * b * b)))
    assert img.max() <= 255.0
    return np.rint(img).astype(np.float32)


# The ladder (64 x 96, enlarged to 128 x 192: octaves of 128, 64, 32 and 16 rows).  Centres are in input pixels; octave-0 pixel a
# is input pixel a / 2 - 0.25.  Small blobs (b = 1.3) land in octave 0, b ~ 3 in octave 1, b ~ 6 in octave 2, b = 11 in octave 3.
#   (15.75, 15.75)  octave-0 pixel (32, 32): the first pixel of blur tile (1, 1)
#   (16.15, 47.9)   octave-0 pixel (33, 96): raster index 33 * 192 + 96 = 6432, detect block 25, while (32, 32) is index 6176,
#                   block 24: two candidates of one layer on either side of the block boundary at index 6400
#   (2.25, 40.3)    octave-0 row 5: on the 5-pixel margin itself
#   (5.2, 80.3)     octave-0 row 11
LADDER = ((15.75, 15.75, 1.3, 110.0), (16.15, 47.9, 1.3, 110.0), (47.8, 16.1, 1.3, 110.0), (5.2, 80.3, 1.3, 110.0),
          (58.9, 90.6, 1.3, 110.0), (2.25, 40.3, 1.3, 110.0), (31.7, 63.6, 2.8, 80.0), (40.2, 34.9, 3.0, 80.0),
          (24.3, 31.2, 5.8, 60.0), (36.5, 74.0, 5.6, 60.0), (30.0, 50.0, 11.0, 40.0))
LADDER_TILE_CORNER = (0, 32, 32)         # (octave, y, x) of integer extrema the ladder must have
LADDER_MARGIN = (0, 5, 81)
LADDER_ROW_11 = (0, 11, 161)
LADDER_BLOCK_PAIR = ((0, 32, 32), (0, 33, 96))
DETECT_BLOCK = 256                        # pixels of one (octave, layer) per block of the extremum kernel, in raster order
BLUR_TILE = 32


@functools.lru_cache(maxsize=None)
def edge_inputs():
    """name -> image of the edge cases (not part of the default yardsticks): the ladder above; tiny8 / tiny8w, 8 x 8 and 8 x 13 with
    one blob, a single octave of exactly 16 rows after the enlargement; thin, 7 x 40, no octave; odd, a 37 x 53 texture whose
    octaves are 74 -> 37 -> 18 rows (37 -> 18 without the enlargement): an odd octave is halved; pair, two identical blobs 48
    pixels apart, whose rows tie in response; blobs43 / blobs155, `blobs_f32_gray` with other seeds, for the parameter values at
    which that input (and the textures) excuse more than the cap with the case's own yardsticks."""
    return {
        "ladder": planted(64, 96, LADDER),
        "tiny8": planted(8, 8, ((3.75, 3.75, 1.3, 110.0),)),
        "tiny8w": planted(8, 13, ((3.75, 6.25, 1.3, 110.0),)),
        "thin": planted(7, 40, ((3.0, 20.0, 1.3, 110.0),)),
        "odd": np.rint(ds.texture(37, 53, 85, 1)).astype(np.uint8),
        "pair": planted(48, 96, ((23.6, 24.1, 1.3, 110.0), (23.6, 72.1, 1.3, 110.0))),
        "blobs43": np.rint(blobs(128, 128, 43)).astype(np.float32),
        "blobs155": np.rint(blobs(128, 128, 155)).astype(np.float32),
    }


PLANTED = ("ladder", "tiny8", "tiny8w", "pair")      # their decision band must be empty; textured inputs may excuse 5 %
BAND_CAP = 0.05


def edge_cases():
    """[(input name, parameters)]: every comparison beyond the default parameters on `inputs()`"""
    P = params
    return [("tex_rgb", P(sigma=1.2)), ("blobs43", P(sigma=2.4)), ("tex_rgb", P(upsample=False)),
            ("tex_rgb", P(upsample=False, n_octave_layers=4, sigma=2.1)), ("tex_gray", P(n_octave_layers=2)),
            ("blobs_f32_gray", P(n_octave_layers=1)),                  # blur radius 45: the twin runs it, the device refuses it
            ("blobs_f32_gray", P(n_octave_layers=1, sigma=1.15)),      # radius 32: L = 1 within the supported blur
            ("blobs155", P(n_octave_layers=8)),                        # 8 is the largest L
            ("blobs_f32_gray", P(edge_threshold=3.0)), ("blobs_f32_gray", P(contrast_threshold=0.09)),
            ("blobs43", P(sigma=4.1)),                                 # the largest sigma with radius 32 at L = 3
            ("ladder", DEFAULT), ("ladder", P(n_octave_layers=2)), ("ladder", P(n_octave_layers=5)), ("ladder", P(upsample=False)),
            ("tiny8", DEFAULT), ("tiny8w", DEFAULT), ("thin", DEFAULT), ("odd", DEFAULT), ("odd", P(upsample=False)),
            ("pair", DEFAULT)]


def case_id(case) -> str:
    name, prm = case
    d = [f"{k}={v}" for k, v, w in zip(("nfeatures", "L", "C", "r", "sigma", "upsample"), prm_key(prm), prm_key(DEFAULT)) if v != w]
    return name + ("[" + ",".join(d) + "]" if d else "")


MAX_RADIUS = 32                           # the blur radius the device supports (tile + halo within 48 KiB)


def band_cap(name: str) -> float:
    return 0.0 if name in PLANTED else BAND_CAP


def blur_radius(prm) -> int:
    """the largest blur radius of the pyramid"""
    base, inc = layer_sigmas(prm)
    return max(int(np.ceil(4.0 * s - 1e-12)) for s in [base] + inc)


def prm_key(prm):
    """The parameters as a hashable tuple, in the argument order of `params`."""
    return (prm.nfeatures, prm.L, prm.C, prm.r, prm.sigma, prm.upsample)


def is_default(prm) -> bool:
    return prm_key(prm) == prm_key(DEFAULT)


def image(name: str) -> np.ndarray:
    return inputs()[name] if name in inputs() else edge_inputs()[name]


@functools.lru_cache(maxsize=None)
def _twin32(name: str, key):
    return sift(image(name), params(*key), np.float32)


def twin32(name: str, prm=DEFAULT):
    return _twin32(name, prm_key(prm))


@functools.lru_cache(maxsize=None)
def _twin64_plain(name: str, key=prm_key(DEFAULT)):
    return sift(image(name), params(*key), np.float64)


def _measure(pairs):
    """The yardsticks of `yardsticks` over (float64 twin, float32 twin) pairs."""
    e = dict(dog=0.0, off=0.0, pos=0.0, scl=0.0, angle=0.0, q=0.0, det=0.0, hist=0.0, desc=0.0, contr=0.0)
    for a, b in pairs:
        if not a.pyr or a.dog_max < 1.0:          # a constant image has no DoG scale to relate to (and no candidates)
            continue
        for Ga, Gb in zip(a.pyr, b.pyr):
            e["dog"] = max(e["dog"], float(np.abs((Gb[1:] - Gb[:-1]).astype(np.float64) - (Ga[1:] - Ga[:-1])).max()) / a.dog_max)
        cb = {c["key"]: c for c in b.cands}
        for c in a.cands:
            d = cb.get(c["key"])
            if d is None or "q" not in c or "q" not in d or c["final"] != d["final"]:
                continue
            e["q"] = max(e["q"], abs(c["q"] - d["q"]) / a.dog_max ** 2)
            e["det"] = max(e["det"], abs(c["det2"] - d["det2"]) / a.dog_max ** 2)
            e["contr"] = max(e["contr"], abs(c["contr"] - d["contr"]) / a.dog_max)
            e["off"] = max(e["off"], max(abs(s - t) for s, t in zip(c["X"], d["X"])))
            if "hist" in c and "hist" in d:
                e["pos"] = max(e["pos"], max(abs(s - t) for s, t in zip(c["X"], d["X"])))
                e["scl"] = max(e["scl"], abs(c["scl"] - d["scl"]) / c["scl"])
                e["hist"] = max(e["hist"], float(np.abs(c["hist"] - d["hist"]).max() / c["hist"].max()))
        kb = {tuple(k): j for j, k in enumerate(b.keys)}
        for j, k in enumerate(a.keys):
            m = kb.get(tuple(k))
            if m is None:
                continue
            da = abs(a.frames[j, 3] - b.frames[m, 3])
            e["angle"] = max(e["angle"], min(da, 360.0 - da))
            e["desc"] = max(e["desc"], float(np.abs(a.v[j] - b.v[m].astype(np.float64)).max()))
    return e


@functools.lru_cache(maxsize=None)
def _yardsticks(name, key):
    names = list(inputs()) if name is None else [name]
    return _measure((_twin64_plain(n, key), _twin32(n, key)) for n in names)


def yardsticks(name=None, prm=DEFAULT):
    """float32 twin against float64 twin, on keypoints with equal keys: E_dog (DoG values, relative to the image's
    largest), E_off (refinement offsets of all refined candidates: octave pixels and layer units), E_pos (the same on keypoints
    only: what the frames carry), E_scl (relative scale of keypoints), E_angle (degrees), E_q / E_det (edge quantity q and the
    2 x 2 determinant, relative to the square of the largest DoG), E_contr (interpolated value, relative), E_hist (smoothed orientation histogram, relative to its largest bin), E_desc (normalised
    rows).  Involves no code under test.

    The default parameters on one of `inputs()` (or no name): the yardsticks over all of `inputs()`, as always.  Any other case
    (an input of `edge_inputs()`, or non-default parameters) has its own: its float32 twin against its float64 twin."""
    if is_default(prm) and (name is None or name in inputs()):
        return _yardsticks(None, prm_key(DEFAULT))
    return _yardsticks(name, prm_key(prm))


@functools.lru_cache(maxsize=None)
def _twin64(name: str, key):
    prm = params(*key)
    plain = _twin64_plain(name, key)
    e = yardsticks(name, prm)
    t = sift(image(name), prm, np.float64, tau=BAND * e["dog"] * plain.dog_max)
    assert np.array_equal(t.keys, plain.keys)
    t.e = e
    return t


def twin64(name: str, prm=DEFAULT):
    """float64 twin of the case (input, parameters) with the near-candidates of the decision band recorded; `.e` holds the
    case's yardsticks and `.prm` its parameters, which the band helpers below take from there unless told otherwise"""
    return _twin64(name, prm_key(prm))


# ------------------------------------------------------------------------------------------ decision band
def _of(t, prm, e):
    """(prm, e) of a twin result unless given: a plain `sift()` result has its parameters but only the default yardsticks"""
    return prm or t.prm, e or getattr(t, "e", None) or yardsticks()


def cand_excused(c, dog_max: float, e=None, prm=DEFAULT) -> bool:
    """One of the candidate's decisions up to the keypoint lies within BAND yardsticks of its threshold (float64 twin only)."""
    e = e or yardsticks()
    tau = BAND * e["dog"] * dog_max
    if abs(c["m_ext"]) <= tau or abs(c["m_pre"]) <= tau or c["status"] == "near":
        return True
    if c.get("m_off", np.inf) <= BAND * e["off"]:
        return True
    if "q" in c:
        if abs(abs(c["contr"]) - float(np.float32(255.0 * prm.C / prm.L))) <= BAND * e["contr"] * dog_max:
            return True
        if c["status"] in ("edge", "keypoint") and (abs(c["q"]) <= BAND * e["q"] * dog_max ** 2
                                                    or abs(c["det2"]) <= BAND * e["det"] * dog_max ** 2):
            return True
    if "scl" in c and c["m_rad"] <= 4.5 * c["scl"] * BAND * e["scl"]:
        return True
    return False


def bin_excused(c, b: int, e=None) -> bool:
    """Orientation bin b of keypoint c is within the band of being / not being a peak: against 0.8 max or a neighbour."""
    e = e or yardsticks()
    h = c["hist"]
    tol = BAND * e["hist"] * h.max()
    l, r = h[(b - 1) % 36], h[(b + 1) % 36]
    near_peak = h[b] > l - tol and h[b] > r - tol and h[b] >= 0.8 * h.max() - tol
    decided = abs(h[b] - l) > tol and abs(h[b] - r) > tol and abs(h[b] - 0.8 * h.max()) > tol
    # a second bin close to the maximum moves the 0.8 line of every bin: covered by tol on 0.8 max
    return near_peak and not decided


def row_excused(t, j: int, prm=None, e=None) -> bool:
    prm, e = _of(t, prm, e)
    r = t.rows[j]
    return cand_excused(r["rec"], t.dog_max, e, prm) or bin_excused(r["rec"], r["key"][4], e)


def band_share(t, prm=None, e=None) -> float:
    n = len(t.rows)
    return sum(row_excused(t, j, prm, e) for j in range(n)) / n if n else 0.0


def key_excused(t, key, prm=None, e=None) -> bool:
    """May a row with this key appear in / be missing from another arithmetic's output?  Looked up in the float64 twin t."""
    prm, e = _of(t, prm, e)
    for c in t.cands:
        if c["key"] == tuple(key[:4]):
            if cand_excused(c, t.dog_max, e, prm):
                return True
            return "hist" in c and bin_excused(c, int(key[4]), e)
    return False


def compare_keys(t64, keys_other, prm=None, e=None):
    """-> (keys only in t64 not excused, keys only in the other not excused)"""
    a = {tuple(k) for k in t64.keys.tolist()}
    b = {tuple(k) for k in np.asarray(keys_other).reshape(-1, 5).tolist()}
    return ([k for k in sorted(a - b) if not key_excused(t64, k, prm, e)], [k for k in sorted(b - a) if not key_excused(t64, k, prm, e)])


def match_frames(t64, frames, prm=DEFAULT, e=None):
    """Match keyless frames (n, 6) to the float64 twin's rows: same octave, position / size / angle within BAND yardsticks.
    -> (index of the twin row for every frame, -1 if none; the deviations of the matched ones)"""
    e = e or yardsticks()
    f = np.asarray(frames, dtype=np.float64).reshape(-1, 6)
    idx = np.full(len(f), -1, dtype=np.int64)
    dev = dict(pos=0.0, angle=0.0, size=0.0)
    if not len(f) or not len(t64.rows):
        return idx, dev
    u = 2.0 if prm.upsample else 1.0
    tf = t64.frames
    used = np.zeros(len(tf), dtype=bool)      # one twin row per frame: two extrema may converge to the same keypoint (equal frames)
    for j in range(len(f)):
        sc = 2.0 ** f[j, 5] / u                                        # input pixels per octave pixel
        dpos = np.maximum(np.abs(tf[:, 0] - f[j, 0]), np.abs(tf[:, 1] - f[j, 1])) / sc
        dsz = np.abs(tf[:, 2] - f[j, 2]) / tf[:, 2]
        dang = np.abs(tf[:, 3] - f[j, 3])
        dang = np.minimum(dang, 360.0 - dang)
        ok = (tf[:, 5] == f[j, 5]) & (dpos <= BAND * e["pos"]) & (dsz <= BAND * e["scl"]) \
            & (dang <= BAND * e["angle"])
        hit = np.nonzero(ok & ~used)[0]
        if len(hit):
            k = hit[np.argmin(dpos[hit] + dang[hit])]
            idx[j] = k
            used[k] = True
            dev["pos"] = max(dev["pos"], float(dpos[k]))
            dev["angle"] = max(dev["angle"], float(dang[k]))
            dev["size"] = max(dev["size"], float(dsz[k]))
    return idx, dev


def frame_excused(t64, frame, prm=DEFAULT, e=None) -> bool:
    """An unmatched frame is excused when an excused candidate of the float64 twin was visited within two octave pixels of it
    (a different move of the refinement ends at most there), or when its keypoint exists and the angle's bin is in the band."""
    e = e or yardsticks()
    u = 2.0 if prm.upsample else 1.0
    o = int(frame[5])
    sc = 2.0 ** o / u
    off = 0.25 if prm.upsample else 0.0
    xo, yo = (frame[0] + off) / sc, (frame[1] + off) / sc
    b = int(np.floor(frame[3] / 10.0 + 0.5)) % 36
    for c in t64.cands:
        if c["key"][0] != o:
            continue
        if not any(abs(x - xo) <= 2.0 and abs(y - yo) <= 2.0 for _, y, x in c["visited"]):
            continue
        if cand_excused(c, t64.dog_max, e, prm):
            return True
        if "hist" in c and any(bin_excused(c, (b + d) % 36, e) for d in (-1, 0, 1)):
            return True
    return False
