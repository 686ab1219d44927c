"""The seeded inputs of tests/test_gpu_neighbors.py, in one table that tests/test_neighbors_host.py reads too: the host test
asserts the conditions the device tests rely on (candidate counts within the slots, a pair exactly on the radius, spectral gaps)
on the very rows the device tests upload.  Every row set is a lattice (neighbors_numpy.lattice): small integers, so the device
must equal the float64 restatement exactly."""
import numpy as np

import neighbors_numpy as nn

# ------------------------------------------------------------------------------------------------ kNN, the filtered path
# name -> (nq, N, L, a, k, seed); nq = 0: the rows query themselves (Q is X).  With float32 rows every one of these takes the
# prefilter and must stay within its candidate slots (cap = min(1024, max(256, 8 k))).
KNN_FILTERED = {
    "k1":           (67, 1500, 12, 4, 1, 101),       # cap 256
    "k10":          (67, 1500, 12, 4, 10, 101),
    "short_k10":    (5, 32771, 8, 3, 10, 102),       # a second column panel of 3 columns, fewer than k
    "short_k64":    (5, 32771, 8, 3, 64, 102),       # cap 512
    "own_row_k10":  (-6, 32771, 8, 3, 10, 102),      # the same + six rows of X as queries, three of them from the short panel
    "own_row_k64":  (-6, 32771, 8, 3, 64, 102),
    "generic_L3":   (130, 700, 3, 6, 7, 103),        # L % 4 != 0: the generic tile GEMM, margin with one chain of L fma
    "generic_L1":   (130, 700, 1, 40, 7, 104),
    "chain_L1028":  (64, 2000, 1028, 3, 10, 105),    # MFMA GEMM with more than one 1024-long chain
    "k129":         (70, 3000, 24, 8, 129, 106),     # cap = 1024 < 8 k
    "k256":         (70, 3000, 24, 8, 256, 106),     # the largest filtered k
    "query_tiles":  (9000, 1200, 8, 5, 10, 107),     # two tiles of 8192 queries
    "self_L4097":   (0, 600, 4097, 2, 10, 108),      # Q is X on the generic GEMM
    "tiny_9":       (0, 9, 5, 3, 9, 109),            # k = N
    "one_row":      (3, 1, 4, 3, 1, 110),            # N = 1
    "tiny_65":      (65, 65, 5, 3, 65, 111),         # k = N, one column more than a wave
    "margin_L256":  (67, 1500, 256, 8, 10, 112),     # norms large enough that the margin reaches past exact ties (unaligned base)
}


def knn_rows(name, dtype=np.float32, table=None):
    """-> (Q, X, k); Q is X (the same object) for the self-query cases"""
    nq, N, L, a, k, seed = (table or KNN_FILTERED)[name]
    X = nn.lattice(seed, N, L, a, dtype)
    if name.startswith(("short_", "own_row_")):
        X[:3] *= 3                  # rows 0..2 far larger than rows N-3..N-1: a half norm read at the wrong panel offset shows
    if nq == 0:
        return X, X, k
    Q = nn.lattice(seed + 5000, abs(nq) if nq > 0 else 5, L, a, dtype)
    if nq < 0:
        Q = np.concatenate([Q, X[[0, 1, PANEL - 1, PANEL, PANEL + 1, PANEL + 2]]])
    return Q, X, k


PANEL = nn.PANEL_COLS

# ------------------------------------------------------------------------------------------------ kNN, the other paths
# k > 256 (no prefilter: the bare f64 ranking), the paged ranking, the query-tile seam of the float64 panels
KNN_F64 = {
    "k257":   (40, 300, 5, 4, 257, 201),
    "k300":   (40, 300, 5, 4, 300, 201),             # k = N
    "paged":  (8, 9000, 6, 6, 4200, 202),            # k above the ranking's page over more columns than its buffer
    "seam":   (70000, 2000, 6, 6, 10, 203),          # QT = 2^27 / 2000 = 67108 < nq
    "huge":   (40, 500, 12, 4, 10, 204),             # scaled by 2^51 in the test: |row|^2 > 2^100
}
SEAM_QT = nn.TILE_F64_ELEMS // 2000
HUGE_SCALE = 2.0 ** 51


def overflow_rows(dtype=np.float32):
    """300 identical rows followed by 400 seeded ones, querying themselves: the first 300 have 300 candidates at distance 0"""
    X = nn.lattice(301, 700, 12, 4, dtype)
    X[:300] = X[0]
    return X, 10


# ------------------------------------------------------------------------------------------------ radius neighbours
def radius_self_rows(dtype):
    """700 x 12 rows, the last 6 repeating the first 6; eps = 5 (eps^2 = 25 is a distance that occurs)"""
    X = nn.lattice(401, 700, 12, 2, dtype)
    X[-6:] = X[:6]
    return X, 5


def radius_query_rows(dtype):
    """130 queries against 700 rows; r^2 = 30"""
    return nn.lattice(402, 130, 12, 2, dtype), nn.lattice(403, 700, 12, 2, dtype), 30.0


def radius_seam_rows(dtype=np.float64):
    """the rows of KNN_F64["seam"]; r^2 = 30"""
    Q, X, _ = knn_rows("seam", dtype, KNN_F64)
    return Q, X, 30.0


# ------------------------------------------------------------------------------------------------ spectral embedding
# name -> (N, chords, isolated, m, seed): a ring i -> i + 1 over the first N - isolated nodes plus seeded chords
GRAPHS = {
    "ring":      (200, 100, 0, 4, 501),
    "isolated":  (203, 100, 3, 4, 501),              # the same ring and chords + three nodes without an edge
    "m1":        (200, 100, 0, 1, 501),
    "whole":     (12, 5, 0, 6, 502),                 # p = min(N, m + 8) = 12: the block is the whole space
}
MIN_GAP = 1e-3


def graph(name):
    """-> (indptr, indices, N, m) of the directed 0/1 graph (spectral_embedding symmetrises it)"""
    N, chords, iso, m, seed = GRAPHS[name]
    n = N - iso
    rng = np.random.default_rng(seed)
    edges = {(i, (i + 1) % n) for i in range(n)}
    while len(edges) < n + chords:
        i, j = (int(v) for v in rng.integers(0, n, 2))
        if i != j and (j, i) not in edges:
            edges.add((i, j))
    e = np.array(sorted(edges), np.int64)
    indptr = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(e[:, 0], minlength=N), out=indptr[1:])
    return indptr, e[:, 1].copy(), N, m
