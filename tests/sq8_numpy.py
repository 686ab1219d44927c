"""NumPy twin of the int8 resident index (csrc/sq8.hip, pvsim/quantized.py): the definitions of include/pvsim.h restated.

  code row    amax = max_t |x[t]|; amax == 0 -> zeros; else c[t] = (int8) rint((x[t] / amax) * 127.0f): a float32 division, then a
              float32 multiply, each rounded on its own (np.float32 element operations); rint rounds half to even.
  storage     int8 [N][ld], ld = 64 ceil(L / 64), bytes L .. ld zero.
  row factor  ss = sum c^2 (int64); inv = 0 if ss == 0 else float32(1.0 / sqrt(float64(ss))).
  score       acc = sum cq * cd (int64, asserted |acc| < 2^31); score = (float32(acc) * inv_q) * inv_d, separate roundings.
  ranking     (score descending, global index ascending): np.lexsort on (index, -score)."""
import numpy as np

F = np.float32
MAX_L = 131072


def ld_of(L):
    return 64 * ((int(L) + 63) // 64)


def encode(x):
    """float32 rows (n, L) -> (codes int8 (n, ld) zero padded, inv float32 (n,))"""
    x = np.ascontiguousarray(x, dtype=F)
    n, L = x.shape
    assert 1 <= L <= MAX_L and np.isfinite(x).all()
    codes = np.zeros((n, ld_of(L)), np.int8)
    amax = np.abs(x).max(axis=1) if n else np.zeros(0, F)
    nz = amax > 0
    with np.errstate(all="ignore"):
        ratio = x[nz] / amax[nz][:, None]                   # float32 / float32 -> float32, IEEE
        scaled = ratio * F(127.0)                           # float32 * float32 -> float32
    assert ratio.dtype == F and scaled.dtype == F
    c = np.rint(scaled)                                     # half to even
    assert (np.abs(c) <= 127).all()
    codes[nz, :L] = c.astype(np.int8)
    return codes, factors(codes)


def exact_halves(amax):
    """-> (x, t): float32 values |x| < amax whose scaled value t = (x / amax) * 127, in float32 arithmetic, is EXACTLY k + 1/2.
    (k + 1/2) / 127 is no float32, so such values exist only where the two roundings land there: found by trying the floats
    around (k + 1/2) amax / 127 for every k."""
    amax = F(amax)
    k = np.arange(-126, 126, dtype=np.float64) + 0.5
    x = (k * float(amax) / 127.0).astype(F)
    x = np.unique(np.concatenate([x, np.nextafter(x, F(np.inf)), np.nextafter(x, F(-np.inf))]))
    t = (x / amax) * F(127.0)
    keep = (t - np.floor(t)) == F(0.5)
    return x[keep], t[keep]


def factors(codes):
    ss = (codes.astype(np.int64) ** 2).sum(axis=1)
    inv = np.zeros(codes.shape[0], F)
    pos = ss > 0
    inv[pos] = (1.0 / np.sqrt(ss[pos].astype(np.float64))).astype(F)
    return inv


def acc(qcodes, codes):
    """int64 (nq, N) dot products of code rows, asserted to fit int32"""
    a = qcodes.astype(np.int64) @ codes.astype(np.int64).T
    assert (np.abs(a) < 2 ** 31).all()
    return a


def scores(qcodes, inv_q, codes, inv_d):
    """float32 (nq, N): ((float32)acc * inv_q) * inv_d"""
    a = acc(qcodes, codes).astype(np.int32).astype(F)       # int32 -> float32 rounds to nearest even
    return (a * np.asarray(inv_q, F)[:, None]) * np.asarray(inv_d, F)[None, :]


def topk(score, k, col_offset=0):
    """-> idx int64 (nq, k), val float32 (nq, k) by (score descending, global index ascending)"""
    score = np.asarray(score, F)
    nq, N = score.shape
    idx = np.empty((nq, k), np.int64)
    val = np.empty((nq, k), F)
    cols = np.arange(N, dtype=np.int64)
    for r in range(nq):
        o = np.lexsort((cols, -score[r]))[:k]
        idx[r], val[r] = o + col_offset, score[r][o]
    return idx, val


def rank(q, x, k):
    """float32 queries and rows -> the lists an Int8Index over x gives for q"""
    qc, iq = encode(q)
    dc, idb = encode(x)
    return topk(scores(qc, iq, dc, idb), k)
