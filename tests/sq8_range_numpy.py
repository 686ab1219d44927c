"""NumPy twin of the int8 threshold join (csrc/sq8_range.hip, include/pvsim.h): sq8_numpy.scores composed with
range_numpy.hits / tile_order.

  score      s(i, j) = (float32(acc) * inv_q[i]) * inv_d[j], acc the integer dot product of the two code rows: the bits of `rank`.
  hit        s >= t compared in float32; a NaN score is never a hit; a zero row has factor 0, scores +0 and hits iff t <= 0.
  self-join  the stored codes and factors on both sides; for i < j the pair is a hit iff s(i, j) >= t with row i in the QUERY role,
             and s(i, j) is the value.  The score is not symmetric ((a * x) * y against (a * y) * x): a pair with
             s(i, j) < t <= s(j, i) is not a hit.
  order      row blocks of QT ascending, column panels of NC ascending, (row, col) ascending within a tile.
  geometry   panel path: 8192 x 32768 (panel_dense); mask path: 8192 x 262144 (panel_mask), a mask row of 4 ceil(cols / 128) uint32
             words and the rows rounded up to 128; `tile` > 0 gives tile x tile on both paths."""
import numpy as np

import range_numpy as rn
import sq8_numpy as sq

F = np.float32
MASK_QT, MASK_NC = 8192, 262144
PANEL_QT, PANEL_NC = 8192, 32768


def scores(qcodes, inv_q, codes, inv_d):
    """sq8_numpy.scores; a loaded file may hold any factor, so NaN and infinite products are values here, not warnings"""
    with np.errstate(invalid="ignore", over="ignore"):
        return sq.scores(qcodes, inv_q, codes, inv_d)


def geometry(nq, N, path, tile=0):
    """-> (QT, NC) of path "panel" or "mask"; tile x tile when a tile is given"""
    if tile:
        return min(nq, tile), min(N, tile)
    return (min(nq, PANEL_QT), min(N, PANEL_NC)) if path == "panel" else (min(nq, MASK_QT), min(N, MASK_NC))


def mask_words(cols):
    return 4 * ((cols + 127) // 128)


def mask_bytes(QT, NC):
    return (QT + 127) // 128 * 128 * mask_words(NC) * 4


def join(qcodes, inv_q, codes, inv_d, t, QT, NC, upper=False):
    """-> (row, col, val) in the device's order for row blocks of QT and column panels of NC"""
    return rn.tile_order(scores(qcodes, inv_q, codes, inv_d), F(t), QT, NC, upper)


def self_join(codes, inv, t):
    """the self-join in (i, j) order: i < j and s(i, j) >= t, row i in the query role"""
    return rn.hits(scores(codes, inv, codes, inv), F(t), upper=True)


def skipped_tiles(nq, N, QT, NC):
    return rn.skipped_tiles(nq, N, QT, NC)


def asymmetric_pairs(S, t):
    """pairs i < j of a square score matrix on which the two roles disagree at t -> (lost, kept): `lost` has s(i, j) < t <= s(j, i)
    (not emitted), `kept` has s(j, i) < t <= s(i, j) (emitted), both as (n, 2) int64 arrays of (i, j)"""
    S = np.asarray(S, F)
    up = np.triu(np.ones(S.shape, bool), 1)
    lo, hi = S < F(t), S >= F(t)
    return np.argwhere(up & lo & hi.T), np.argwhere(up & hi & lo.T)


def brute(qcodes, inv_q, codes, inv_d, t, upper=False):
    """the definition as a double loop over Python integers and float32 scalars, (row, col) ascending"""
    t = F(t)
    out = []
    for i in range(qcodes.shape[0]):
        for j in range(codes.shape[0]):
            if upper and j <= i:
                continue
            a = sum(int(x) * int(y) for x, y in zip(qcodes[i].tolist(), codes[j].tolist()))
            s = F(F(F(np.int32(a)) * F(inv_q[i])) * F(inv_d[j]))
            if s >= t:
                out.append((i, j, s))
    return (np.array([o[0] for o in out], np.int64), np.array([o[1] for o in out], np.int64), np.array([o[2] for o in out], F))
