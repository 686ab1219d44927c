"""NumPy twin of the spatial re-ranking stages (csrc/match.hip): the same three definitions, stated a second
time without any code under test, plus the input generators and the yardstick that tests/test_match_host.py asserts and
tests/test_gpu_match.py holds the device to.

  stage 1  match_u8       exact squared distances in int64, best / second best per row, ties to the lowest index
  stage 2  filter_matches the ratio test as ONE float64 product and comparison, the mutual check, ascending order
  stage 3  verify         every match a similarity hypothesis, exhaustive count, least-squares affine refinement, all float64

Stages 1 and 2 are integer / single-comparison definitions: the device must give the same bits.  Stage 3 compares a residual with
a threshold in float64, and the device's cos / sin and summation order need not be NumPy's, so `verify` also returns, for every
(h, g), a band flag |r - tol| <= E.  E is a yardstick, not a measurement: the residual is formed from coordinates of magnitude at
most X = (1 + sigma_max) * max |coordinate| by a fixed handful of float64 operations (two differences, four products by cos / sin
good to an ulp, two sums, a difference, a square root), each contributing at most one ulp of X, i.e. X * 2^-52; E = SAFETY such
ulps with SAFETY = 64."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

INT32_MAX = np.iinfo(np.int32).max
SAFETY = 64.0
DEFAULT_TOL = 12.0
DEG = np.pi / 180.0


# ------------------------------------------------------------------------------------------------------------------ stage 1
def match_u8(rows_a: np.ndarray, rows_b: np.ndarray):
    """-> (idx int32 (nA,), d1 int32, d2 int32) of one image pair."""
    a = np.asarray(rows_a, dtype=np.uint8).reshape(-1, 128).astype(np.int64)
    b = np.asarray(rows_b, dtype=np.uint8).reshape(-1, 128).astype(np.int64)
    na, nb = len(a), len(b)
    idx = np.full(na, -1, np.int32)
    d1 = np.full(na, INT32_MAX, np.int32)
    d2 = np.full(na, INT32_MAX, np.int32)
    if na == 0 or nb == 0:
        return idx, d1, d2
    d = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T)
    j = np.argmin(d, axis=1)                                  # the first minimum: the lowest index
    idx[:] = j
    d1[:] = d[np.arange(na), j]
    if nb > 1:
        d[np.arange(na), j] = np.iinfo(np.int64).max
        d2[:] = d.min(axis=1)
    return idx, d1, d2


def match_pairs(rows_a, off_a, rows_b, off_b, pairs):
    """Stage 1 over a pair list: the concatenated per-row results in the layout of pvs_match_u8_dev."""
    out = [match_u8(rows_a[off_a[ia]:off_a[ia + 1]], rows_b[off_b[ib]:off_b[ib + 1]]) for ia, ib in np.asarray(pairs).reshape(-1, 2)]
    if not out:
        return tuple(np.zeros(0, np.int32) for _ in range(3))
    return tuple(np.concatenate([o[k] for o in out]) for k in range(3))


# ------------------------------------------------------------------------------------------------------------------ stage 2
def ratio_sq(ratio: float) -> float:
    return float(ratio) * float(ratio)


def filter_matches(idx, d1, d2, idx_rev, ratio_sq_: float, mutual: bool) -> np.ndarray:
    """-> (m, 2) int32 matches (i, j) of one pair in ascending i."""
    idx = np.asarray(idx)
    keep = (idx >= 0) & (np.asarray(d1).astype(np.float64) < np.float64(ratio_sq_) * np.asarray(d2).astype(np.float64))
    if mutual:
        back = np.asarray(idx_rev)
        keep &= np.array([k and back[j] == i for i, (j, k) in enumerate(zip(idx, keep))], dtype=bool).reshape(keep.shape)
    i = np.nonzero(keep)[0]
    return np.stack([i, idx[i]], axis=1).astype(np.int32).reshape(-1, 2)


# ------------------------------------------------------------------------------------------------------------------ stage 3
def points(frames_a, frames_b, matches):
    """float64 points and hypotheses of the matches: (pa (m, 2), pb (m, 2), c, s, valid)."""
    m = np.asarray(matches).reshape(-1, 2)
    fa = np.asarray(frames_a, dtype=np.float32).reshape(-1, 6)[m[:, 0]].astype(np.float64)
    fb = np.asarray(frames_b, dtype=np.float32).reshape(-1, 6)[m[:, 1]].astype(np.float64)
    valid = np.isfinite(fa[:, :4]).all(1) & np.isfinite(fb[:, :4]).all(1) & (fa[:, 2] > 0)
    with np.errstate(all="ignore"):
        sigma = fb[:, 2] / fa[:, 2]
        phi = (fb[:, 3] - fa[:, 3]) * DEG
        c, s = sigma * np.cos(phi), sigma * np.sin(phi)
    return fa[:, :2].copy(), fb[:, :2].copy(), c, s, valid


def yardstick(pa, pb, c, s, valid) -> float:
    """E: SAFETY ulps of float64 at the largest (scaled) coordinate."""
    if len(pa) == 0 or not valid.any():
        return 0.0
    sig = np.hypot(c[valid], s[valid]).max()
    fin = np.concatenate([pa[np.isfinite(pa)], pb[np.isfinite(pb)], [0.0]])
    return float(SAFETY * 2.0 ** -52 * (1.0 + sig) * np.abs(fin).max())


def _residual(M, ca, cb, pa, pb):
    da, db = pa - ca, pb - cb
    rx = (M[0, 0] * da[:, 0] + M[0, 1] * da[:, 1]) - db[:, 0]
    ry = (M[1, 0] * da[:, 0] + M[1, 1] * da[:, 1]) - db[:, 1]
    return rx * rx + ry * ry


def fit(pa, pb, mask):
    """Least-squares affine fit on `mask`: (M (2, 2), mean_a, mean_b) or None when fewer than 3 points or det C <= 1e-12 (tr C)^2."""
    mask = np.asarray(mask, dtype=bool)
    if mask.sum() < 3:
        return None
    a, b = pa[mask], pb[mask]
    ma, mb = a.sum(0) / len(a), b.sum(0) / len(a)
    at, bt = a - ma, b - mb
    cxx, cxy, cyy = (at[:, 0] * at[:, 0]).sum(), (at[:, 0] * at[:, 1]).sum(), (at[:, 1] * at[:, 1]).sum()
    bxx, bxy = (bt[:, 0] * at[:, 0]).sum(), (bt[:, 0] * at[:, 1]).sum()
    byx, byy = (bt[:, 1] * at[:, 0]).sum(), (bt[:, 1] * at[:, 1]).sum()
    det, tr = cxx * cyy - cxy * cxy, cxx + cyy
    if not det > 1e-12 * (tr * tr):
        return None
    M = np.array([[(bxx * cyy - bxy * cxy) / det, (bxy * cxx - bxx * cxy) / det],
                  [(byx * cyy - byy * cxy) / det, (byy * cxx - byx * cxy) / det]])
    return M, ma, mb


def model_2x3(M, ca, cb) -> np.ndarray:
    """(2, 3) [M | t] with p_b ~ M p_a + t, t = cb - M ca."""
    t = np.array([cb[0] - (M[0, 0] * ca[0] + M[0, 1] * ca[1]), cb[1] - (M[1, 0] * ca[0] + M[1, 1] * ca[1])])
    return np.concatenate([M, t[:, None]], axis=1)


def verify(frames_a, frames_b, matches, tol: float = DEFAULT_TOL, refine_rounds: int = 2):
    """Stage 3 on one pair.  -> namespace with
         r (m, m)        residual of match g under hypothesis h (NaN where undefined), band (m, m) = |r - tol| <= E, E
         certain (m,)    per hypothesis the inliers that are no band cases, doubtful (m,) its band cases
         best, inliers, model (2, 3), mask (m,) bool: the result of the definition evaluated in float64 here
         final_r (m,), final_band (m,): residuals of the final model and their band flags
         rounds: refinement rounds adopted; converged: the last adopted fit reproduced the set it was fitted on, so the
         model is the least-squares fit on the final mask."""
    pa, pb, c, s, valid = points(frames_a, frames_b, matches)
    m = len(pa)
    tol_sq = float(tol) * float(tol)
    E = yardstick(pa, pb, c, s, valid)
    out = SimpleNamespace(E=E, pa=pa, pb=pb, valid=valid)
    with np.errstate(all="ignore"):
        dax, day = pa[None, :, 0] - pa[:, None, 0], pa[None, :, 1] - pa[:, None, 1]
        dbx, dby = pb[None, :, 0] - pb[:, None, 0], pb[None, :, 1] - pb[:, None, 1]
        rx = (c[:, None] * dax - s[:, None] * day) - dbx
        ry = (s[:, None] * dax + c[:, None] * day) - dby
        r2 = rx * rx + ry * ry
        r2[~valid] = np.nan
        inl = r2 <= tol_sq                                   # NaN compares false
        out.r = np.sqrt(r2)
        out.band = np.abs(out.r - tol) <= E
    out.inl = inl
    out.certain = (inl & ~out.band).sum(1)
    out.doubtful = out.band.sum(1)
    counts = inl.sum(1)
    out.counts = counts
    out.rounds, out.converged = 0, False
    if m == 0 or counts.max() == 0:
        out.best, out.inliers, out.model, out.mask = -1, 0, np.zeros((2, 3)), np.zeros(m, bool)
        out.final_r, out.final_band = np.full(m, np.nan), np.zeros(m, bool)
        return out
    best = int(np.argmax(counts))                            # the first maximum: the lowest h
    M = np.array([[c[best], -s[best]], [s[best], c[best]]])
    ca, cb = pa[best].copy(), pb[best].copy()
    mask, count = inl[best].copy(), int(counts[best])
    for _ in range(int(refine_rounds)):
        f = fit(pa, pb, mask) if count >= 3 else None
        if f is None:
            break
        with np.errstate(all="ignore"):
            new = _residual(f[0], f[1], f[2], pa, pb) <= tol_sq
        if int(new.sum()) < count:
            break
        same = bool((new == mask).all())
        M, ca, cb, mask, count = f[0], f[1], f[2], new, int(new.sum())
        out.rounds += 1
        out.converged = same
        if same:
            break
    with np.errstate(all="ignore"):
        out.final_r = np.sqrt(_residual(M, ca, cb, pa, pb))
        out.final_band = np.abs(out.final_r - tol) <= E
    out.best, out.inliers, out.model, out.mask = best, count, model_2x3(M, ca, cb), mask
    return out


# ------------------------------------------------------------------------------------------------------------------ generators
def random_rows(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, size=(n, 128), dtype=np.uint8)


def sift_like_rows(n: int, seed: int) -> np.ndarray:
    """Rows with the statistics of quantised SIFT (many small values, a few at the clamp): distances spread as real ones do."""
    rng = np.random.default_rng(seed)
    v = rng.gamma(0.6, 1.0, size=(n, 128))
    v /= np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)
    v = np.minimum(v, 0.2)
    v /= np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)
    return np.minimum(255, np.floor(512.0 * v + 0.5)).astype(np.uint8)


def planted_rows(n: int, seed: int) -> np.ndarray:
    """Random rows with planted duplicates (rows 3 k repeat row k for small k, in both directions of the index order) and, when
    there is room, one all-0 and one all-255 row: ties, zero distances and the extremes of the sign shift."""
    x = random_rows(n, seed)
    for k in range(1, n // 3):
        if k % 4 == 1:
            x[3 * k] = x[k]
    if n >= 8:
        x[5] = 0
        x[6] = 255
    if n >= 40:
        x[37] = 0                                            # a second all-0 row: an exact tie at distance 0
    return x


def planted_matches(m: int, outlier_share: float, seed: int, scale: float = 1.37, rot_deg: float = 33.0, shift=(41.5, -17.25),
                    noise: float = 0.7, size_noise: float = 0.02, angle_noise: float = 1.5, extent=(640.0, 480.0)):
    """A planted similarity: frames of A, frames of B = the transform of A plus position / size / angle noise, the last
    round(outlier_share m) matches replaced by unrelated frames.  -> (frames_a (m, 6) f32, frames_b (m, 6) f32, matches (m, 2) int32,
    truth (2, 3) float64, is_inlier (m,) bool).  The matches visit the frames in a shuffled order."""
    rng = np.random.default_rng(seed)
    fa = np.zeros((m, 6), np.float32)
    fb = np.zeros((m, 6), np.float32)
    pa = rng.uniform((0.0, 0.0), extent, size=(m, 2))
    th = rot_deg * DEG
    M = scale * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    t = np.asarray(shift, dtype=np.float64)
    pb = pa @ M.T + t + rng.normal(0.0, noise, size=(m, 2))
    size_a = rng.uniform(2.0, 20.0, size=m)
    ang_a = rng.uniform(0.0, 360.0, size=m)
    size_b = size_a * scale * (1.0 + rng.normal(0.0, size_noise, size=m))
    ang_b = (ang_a + rot_deg + rng.normal(0.0, angle_noise, size=m)) % 360.0
    n_out = int(round(outlier_share * m))
    good = np.ones(m, bool)
    if n_out:
        good[m - n_out:] = False
        lo = pb[good].min(0) if good.any() else np.zeros(2)
        hi = pb[good].max(0) if good.any() else np.asarray(extent)
        pb[~good] = rng.uniform(lo, hi, size=(n_out, 2))
        size_b[~good] = rng.uniform(2.0, 30.0, size=n_out)
        ang_b[~good] = rng.uniform(0.0, 360.0, size=n_out)
    fa[:, 0:2], fa[:, 2], fa[:, 3], fa[:, 4] = pa, size_a, ang_a, 1.0
    fb[:, 0:2], fb[:, 2], fb[:, 3], fb[:, 4] = pb, size_b, ang_b, 1.0
    perm_a, perm_b = rng.permutation(m), rng.permutation(m)      # frame order differs from match order in both images
    frames_a, frames_b = np.empty_like(fa), np.empty_like(fb)
    frames_a[perm_a], frames_b[perm_b] = fa, fb
    matches = np.stack([perm_a, perm_b], axis=1).astype(np.int32)
    return frames_a, frames_b, matches, np.concatenate([M, t[:, None]], axis=1), good


def corner_error(model, truth, extent=(640.0, 480.0)) -> float:
    """Largest distance between the two (2, 3) transforms at the corners of the A image."""
    w, h = extent
    c = np.array([[0.0, 0.0, 1.0], [w, 0.0, 1.0], [0.0, h, 1.0], [w, h, 1.0]])
    return float(np.linalg.norm(c @ np.asarray(model).T - c @ np.asarray(truth).T, axis=1).max())


def warp_bilinear(img: np.ndarray, model, out_hw) -> np.ndarray:
    """Resample: out(p_b) = img(p_a) with p_b = M p_a + t, bilinear, replicated borders (NumPy only)."""
    model = np.asarray(model, dtype=np.float64)
    Minv = np.linalg.inv(model[:, :2])
    h, w = out_hw
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    bx, by = xx - model[0, 2], yy - model[1, 2]
    ax = np.clip(Minv[0, 0] * bx + Minv[0, 1] * by, 0.0, img.shape[1] - 1.0)
    ay = np.clip(Minv[1, 0] * bx + Minv[1, 1] * by, 0.0, img.shape[0] - 1.0)
    x0 = np.minimum(np.floor(ax).astype(np.int64), img.shape[1] - 2)
    y0 = np.minimum(np.floor(ay).astype(np.int64), img.shape[0] - 2)
    fx, fy = ax - x0, ay - y0
    if img.ndim == 3:
        fx, fy = fx[..., None], fy[..., None]
    return ((1 - fy) * ((1 - fx) * img[y0, x0] + fx * img[y0, x0 + 1]) + fy * ((1 - fx) * img[y0 + 1, x0] + fx * img[y0 + 1, x0 + 1]))
