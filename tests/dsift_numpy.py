"""NumPy statement of the dense SIFT definition, with the arithmetic dtype as a parameter.

Test infrastructure only: the package has no CPU path.  Written on whole-image arrays with plain loops over the taps,
independently of the kernel's tiling.  `dense_sift(image, step, sizes, dtype)` returns the raw accumulators, the rows after the
first normalisation (before the 0.2 clamp), the final normalised rows and the uint8 rows.

Also here: the seeded test inputs shared by tests/test_dsift_host.py and tests/test_gpu_dsift.py, the row classes of the
issue (zero / weak / strong by the float64 twin's norm) and the yardsticks E and E_raw (float32 twin against float64 twin)."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

WEAK_REL = 1e-3          # rows below this fraction of the image's largest row norm are compared on raw accumulators only
PARAMS = (((4, 8), 16), ((6,), 8), ((4, 6, 8, 10), 8))      # (sizes, step) of the comparisons on every input
LARGE_PARAMS = (((12, 16), 8), ((18,), 16))                   # single-descriptor tiles (70-158 KiB of LDS), on `rect` only


def grid(extent: int, s: int, step: int) -> np.ndarray:
    """Descriptor origins along one axis: s - 1 + a step <= extent - 4 s."""
    if extent < 5 * s - 1:
        return np.zeros(0, dtype=np.int64)
    return s - 1 + step * np.arange((extent - 5 * s + 1) // step + 1, dtype=np.int64)


def count(h: int, w: int, step: int, sizes) -> int:
    return int(sum(len(grid(w, s, step)) * len(grid(h, s, step)) for s in sizes))


def frames(h: int, w: int, step: int, sizes) -> np.ndarray:
    out = []
    for s in sizes:
        for y0 in grid(h, s, step):
            for x0 in grid(w, s, step):
                out.append((x0 + 1.5 * s, y0 + 1.5 * s, s))
    return np.array(out, dtype=np.float32).reshape(-1, 3)


def gray(image: np.ndarray, dtype) -> np.ndarray:
    im = np.asarray(image).astype(dtype)
    if im.ndim == 2:
        return im
    return dtype(0.299) * im[:, :, 0] + dtype(0.587) * im[:, :, 1] + dtype(0.114) * im[:, :, 2]


def gaussian_taps(s: int) -> np.ndarray:
    """float32 taps (normalised in float64), radius ceil(4 sigma), sigma = s / 6."""
    sigma = s / 6.0
    r = int(np.ceil(4.0 * sigma - 1e-12))
    d = np.arange(-r, r + 1, dtype=np.float64)
    t = np.exp(-d * d / (2.0 * sigma * sigma))
    return (t / t.sum()).astype(np.float32)


def smooth(img: np.ndarray, s: int, dtype) -> np.ndarray:
    taps = gaussian_taps(s).astype(dtype)
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


def orientation_planes(sm: np.ndarray, dtype) -> np.ndarray:
    """(8, H, W): the gradient magnitude split between the two nearest orientation planes."""
    h, w = sm.shape
    gx = np.empty_like(sm)
    gy = np.empty_like(sm)
    gx[:, 1:-1] = dtype(0.5) * (sm[:, 2:] - sm[:, :-2])
    gx[:, 0] = sm[:, 1] - sm[:, 0]
    gx[:, -1] = sm[:, -1] - sm[:, -2]
    gy[1:-1, :] = dtype(0.5) * (sm[2:, :] - sm[:-2, :])
    gy[0, :] = sm[1, :] - sm[0, :]
    gy[-1, :] = sm[-1, :] - sm[-2, :]
    m = np.sqrt(gx * gx + gy * gy)
    theta = np.arctan2(gy, gx)
    theta = np.where(theta < 0, theta + dtype(2.0 * np.pi), theta).astype(dtype)
    t = (theta * dtype(8.0 / (2.0 * np.pi))).astype(dtype)
    fl = np.floor(t)
    frac = (t - fl).astype(dtype)
    b0 = fl.astype(np.int64) % 8
    b1 = (b0 + 1) % 8
    planes = np.zeros((8, h, w), dtype=dtype)
    for o in range(8):
        planes[o] += np.where(b0 == o, m * (dtype(1.0) - frac), dtype(0.0))
        planes[o] += np.where(b1 == o, m * frac, dtype(0.0))
    return planes


def bin_sums(planes: np.ndarray, s: int, dtype) -> np.ndarray:
    """(8, H, W): sum over |dx|, |dy| < s of w(dx) w(dy) plane[y + dy, x + dx] (zero outside the image: no support the grid
    allows reaches there)."""
    _, h, w = planes.shape
    p = np.pad(planes, ((0, 0), (0, 0), (s - 1, s - 1)))
    ax = np.zeros_like(planes)
    for d in range(-(s - 1), s):
        ax += (dtype(1.0) - dtype(abs(d)) / dtype(s)) * p[:, :, d + s - 1:d + s - 1 + w]
    p = np.pad(ax, ((0, 0), (s - 1, s - 1), (0, 0)))
    out = np.zeros_like(planes)
    for d in range(-(s - 1), s):
        out += (dtype(1.0) - dtype(abs(d)) / dtype(s)) * p[:, d + s - 1:d + s - 1 + h, :]
    return out


def normalise(raw: np.ndarray, dtype, contrast_threshold: float = 0.0):
    """-> (v1 = d / |d| before the clamp, v = final rows); rows with |d| <= threshold are zero in both."""
    n1 = np.sqrt((raw * raw).sum(axis=1, keepdims=True)).astype(dtype)
    live = n1 > dtype(contrast_threshold)
    v1 = np.where(live, raw / np.where(live, n1, dtype(1.0)), dtype(0.0)).astype(dtype)
    c = np.minimum(v1, dtype(0.2))
    n2 = np.sqrt((c * c).sum(axis=1, keepdims=True)).astype(dtype)
    v = np.where(live, c / np.where(live, n2, dtype(1.0)), dtype(0.0)).astype(dtype)
    return v1, v


def quantise(v: np.ndarray) -> np.ndarray:
    return np.minimum(255.0, np.floor(512.0 * v.astype(np.float64) + 0.5)).astype(np.uint8)


def dense_sift(image: np.ndarray, step: int, sizes, dtype=np.float64, contrast_threshold: float = 0.0):
    g = gray(image, dtype)
    h, w = g.shape
    rows = []
    for s in sizes:
        xs, ys = grid(w, s, step), grid(h, s, step)
        if len(xs) == 0 or len(ys) == 0:
            continue
        b = bin_sums(orientation_planes(smooth(g, s, dtype), dtype), s, dtype)
        off = s * np.arange(4)
        yy = (ys[:, None] + off[None, :])                      # (ny, 4)  bin-centre rows
        xx = (xs[:, None] + off[None, :])                      # (nx, 4)
        # d[b, a, j, i, o] = B[o, y0 + j s, x0 + i s]
        d = b[:, yy[:, None, :, None], xx[None, :, None, :]]   # (8, ny, nx, 4, 4)
        rows.append(np.moveaxis(d, 0, -1).reshape(len(ys) * len(xs), 128))
    raw = np.concatenate(rows).astype(dtype) if rows else np.zeros((0, 128), dtype=dtype)
    v1, v = normalise(raw, dtype, contrast_threshold)
    return SimpleNamespace(raw=raw, v1=v1, v=v, u8=quantise(v))


def rootsift_tail(raw_rows: np.ndarray) -> np.ndarray:
    d = raw_rows.astype(np.float32)
    if d.shape[0]:
        d /= (d.sum(axis=1, keepdims=True) + 1e-7)
        d = np.sqrt(d)
    return d


def mirror_rows(rows: np.ndarray, h: int, w: int, step: int, sizes) -> np.ndarray:
    """Rows of the horizontally flipped image predicted from the rows of the image (needs (w - 5 s + 1) % step == 0):
    x0 order reversed, bins i -> 3 - i, planes o -> (4 - o) mod 8."""
    out, r0 = [], 0
    perm_o = [(4 - o) % 8 for o in range(8)]
    for s in sizes:
        nx, ny = len(grid(w, s, step)), len(grid(h, s, step))
        if nx == 0 or ny == 0:
            continue
        assert (w - 5 * s + 1) % step == 0
        blk = rows[r0:r0 + nx * ny].reshape(ny, nx, 4, 4, 8)
        out.append(blk[:, ::-1, :, ::-1, :][..., perm_o].reshape(nx * ny, 128))
        r0 += nx * ny
    return np.concatenate(out) if out else rows[:0]


# ------------------------------------------------------------------------------------------ inputs
def texture(h: int, w: int, seed: int, channels: int = 3, rect=None) -> np.ndarray:
    """float64 (h, w[, 3]) in 0..255: band-limited random texture plus sharp edges, textured everywhere except inside `rect`
    = (y, x, hh, ww), which is exactly constant (gray level 40).  The rows that only catch the smoothing tail next to the
    rectangle carry the largest float32 error (differences of nearly equal smoothed values, amplified by the normalisation),
    so the level of the rectangle moves E; tests/test_dsift_host.py asserts the conditions the comparisons need."""
    rng = np.random.default_rng(seed)
    chans = []
    for _ in range(channels):
        spec = np.fft.rfft2(rng.standard_normal((h, w)))
        fy = np.fft.fftfreq(h)[:, None]
        fx = np.fft.rfftfreq(w)[None, :]
        r = np.sqrt(fy * fy + fx * fx)
        band = np.exp(-((r - 0.06) / 0.05) ** 2)
        t = np.fft.irfft2(spec * band, s=(h, w))
        t = t / np.abs(t).max()
        img = 128.0 + 70.0 * t
        # sharp edges: a few half-planes and boxes with random offsets
        for _k in range(4):
            y, x = rng.integers(0, h), rng.integers(0, w)
            hh, ww = rng.integers(8, max(9, h // 2)), rng.integers(8, max(9, w // 2))
            img[y:y + hh, x:x + ww] += rng.uniform(-45, 45)
        chans.append(np.clip(img, 0.0, 255.0))
    img = np.stack(chans, axis=-1) if channels == 3 else chans[0]
    if rect is not None:
        y, x, hh, ww = rect
        img[y:y + hh, x:x + ww] = 40.0
    return img


@functools.lru_cache(maxsize=None)
def inputs():
    """name -> image.  uint8 RGB, uint8 gray, float32 RGB (non-integer values) and float32 gray (integer valued: 2-D float
    images must be, pvsim._utils.is_numpy_image); odd and non-square sizes; `small` is too low for bin size 10 (45 < 49);
    `rect` holds a constant rectangle that contains whole descriptors of every size used; `const` is all constant."""
    imgs = {
        "rect": np.rint(texture(176, 215, 1, 3, rect=(30, 40, 110, 120))).astype(np.uint8),
        "odd_gray": np.rint(texture(97, 131, 2, 1)).astype(np.uint8),
        "f32_rgb": texture(83, 150, 3, 3).astype(np.float32),
        "f32_gray": np.rint(texture(120, 77, 4, 1)).astype(np.float32),
        "small": np.rint(texture(45, 140, 5, 3)).astype(np.uint8),
        "const": np.full((64, 90, 3), 117, dtype=np.uint8),
    }
    return imgs


def cases():
    """(input name, sizes, step) of every comparison."""
    out = [(name, sizes, step) for name in inputs() for sizes, step in PARAMS]
    return out + [("rect", sizes, step) for sizes, step in LARGE_PARAMS]


def classify(raw64: np.ndarray):
    """-> (zero, weak, strong) boolean masks over the rows, by the float64 twin's row norm relative to the largest."""
    n = np.sqrt((raw64 * raw64).sum(axis=1))
    top = n.max() if n.size else 0.0
    zero = n == 0.0
    weak = (~zero) & (n < WEAK_REL * top)
    return zero, weak, ~(zero | weak)


@functools.lru_cache(maxsize=None)
def edge_inputs():
    """name -> image of the edge shapes (not part of the default yardsticks), named by shape: exact fits of one descriptor
    (5 s - 1 pixels: the support touches all four borders), remainders 0 on both axes, and shapes for bin sizes 1 to 3, step 1
    and sixteen sizes.  uint8 gray and RGB and float32 RGB in turn."""
    u8 = lambda h, w, seed, ch: np.rint(texture(h, w, seed, ch)).astype(np.uint8)
    return {
        "e19x19": u8(19, 19, 61, 1), "e39x39": u8(39, 39, 62, 3), "e89x105": u8(89, 105, 63, 1),
        "e27x35": texture(27, 35, 64, 3).astype(np.float32), "e75x83": u8(75, 83, 65, 3), "e87x95": u8(87, 95, 66, 1),
        "e23x31": u8(23, 31, 67, 3), "e59x67": u8(59, 67, 68, 1), "e40x52": texture(40, 52, 69, 3).astype(np.float32),
        "e83x90": u8(83, 90, 70, 1),
    }


SIXTEEN = tuple(range(1, 17))
# (input, sizes, step) of the edge comparisons.  e19x19 / e39x39 / e89x105: one descriptor per axis that fits exactly (89 x 105 at
# s = 18, step 16: one down, two across, both border columns); e27x35: remainder 0 on both axes, six rows; e75x83 / e87x95: the
# single-descriptor LDS regime (s = 12 / 16) with remainder 0 on both axes, no image has that for both sizes at step 8 (59 and 79
# differ by 4 mod 8); e23x31: bin sizes 1 to 3 at step 1, 1,085 rows; e59x67: step 1 across the 8 x 8 tile cap and the single-
# descriptor regime; e40x52: odd sizes at step 3; e83x90: DS_MAX_SIZES = 16 sizes; rect at step 8: the contrast-threshold case
EDGE_CASES = (("e19x19", (4,), 8), ("e39x39", (8,), 8), ("e89x105", (18,), 16), ("e27x35", (4,), 8), ("e75x83", (12,), 8),
              ("e87x95", (16,), 8), ("e23x31", (1, 2, 3), 1), ("e59x67", (4, 12), 1), ("e40x52", (2, 5, 7), 3),
              ("e83x90", SIXTEEN, 8), ("rect", (4, 8), 8))


def image(name: str) -> np.ndarray:
    return inputs()[name] if name in inputs() else edge_inputs()[name]


@functools.lru_cache(maxsize=None)
def twin_pair(name: str, sizes, step: int):
    img = image(name)
    return dense_sift(img, step, sizes, np.float64), dense_sift(img, step, sizes, np.float32)


@functools.lru_cache(maxsize=None)
def edge_yardsticks():
    """(E, E_raw) of `yardsticks`, over EDGE_CASES alone"""
    return _yardsticks(EDGE_CASES)


@functools.lru_cache(maxsize=None)
def contrast_case():
    """-> (threshold, float64 row norms, band) for `rect` at sizes (4, 8), step 8: the threshold lies about the lower quartile of the
    non-zero row norms, in the middle of the widest gap between neighbouring norms there, so that no row is within `band` =
    8 E_raw top sqrt(128) of it (a row's norm moves by at most sqrt(128) times the error of an accumulator)."""
    t64, _ = twin_pair("rect", (4, 8), 8)
    n = np.sqrt((t64.raw * t64.raw).sum(axis=1))
    nz = np.sort(n[n > 0])
    q = len(nz) // 4
    lo = max(q - 8, 0)
    k = lo + int(np.argmax(np.diff(nz[lo:q + 9])))
    band = 8.0 * edge_yardsticks()[1] * float(np.abs(t64.raw).max()) * np.sqrt(128.0)
    return float(0.5 * (nz[k] + nz[k + 1])), n, band


@functools.lru_cache(maxsize=None)
def yardsticks():
    """(E, E_raw) over all inputs and parameter sets: the largest |twin(float32) - twin(float64)| on the normalised rows of
    the strong rows, and on the raw accumulators of all rows relative to the image's largest accumulator.  Involves no code
    under test."""
    return _yardsticks(tuple(cases()))


def _yardsticks(case_list):
    e = e_raw = 0.0
    for name, sizes, step in case_list:
        if True:
            t64, t32 = twin_pair(name, sizes, step)
            if t64.raw.shape[0] == 0:
                continue
            _, _, strong = classify(t64.raw)
            if strong.any():
                e = max(e, float(np.abs(t32.v[strong].astype(np.float64) - t64.v[strong]).max()))
            top = float(np.abs(t64.raw).max())
            if top > 0:
                e_raw = max(e_raw, float(np.abs(t32.raw.astype(np.float64) - t64.raw).max()) / top)
    return e, e_raw


def excused_entries(t64, tol: float) -> np.ndarray:
    """Entries of the uint8 rows that may differ by one: 512 v within 512 tol of a half-integer, or v1 within tol of the
    0.2 clamp."""
    x = 512.0 * t64.v
    near_half = np.abs(x - np.floor(x) - 0.5) <= 512.0 * tol
    near_clamp = np.abs(t64.v1 - 0.2) <= tol
    return near_half | near_clamp
