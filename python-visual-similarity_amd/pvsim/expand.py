"""Query expansion and database-side augmentation.

    qe = QueryExpansion(n=10, scheme="alpha", alpha=3)
    idx, val = index.rank_expanded(queries, k, qe)          # pvsim.index.DeviceIndex
    augmented = index.augmented(r=10, scheme="linear")       # a second DeviceIndex, every row replaced

Average query expansion (Chum et al., "Total Recall", ICCV 2007) re-queries with the sum of the normalised query and its first n
results; alpha query expansion (Radenovic et al., PAMI 2018) weights result j by its similarity to the power alpha; database-side
augmentation (Arandjelovic & Zisserman, CVPR 2012) does the same to every database row, with weights that fall linearly with the
rank.  The weights are a few numbers per list and are computed here, in NumPy; the sums over whole encoding rows run on the device
(pvs_combine_rows_dev), against the resident rows of a DeviceIndex."""
from __future__ import annotations

import math

import numpy as np

__all__ = ["QueryExpansion", "expansion_weights", "drop_self", "SCHEMES"]

SCHEMES = ("average", "alpha", "linear")


def _check_scheme(scheme, alpha):
    if scheme not in SCHEMES:
        raise ValueError(f"scheme must be one of {SCHEMES}, got {scheme!r}")
    if isinstance(alpha, bool) or not isinstance(alpha, (int, np.integer)) or not 0 <= alpha <= 8:
        raise ValueError(f"alpha must be an integer in 0..8, got {alpha!r}")


def _check_count(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
        raise ValueError(f"{name} must be an integer >= 1, got {v!r}")


class QueryExpansion:
    """How `DeviceIndex.rank_expanded` (and `expand=` of pvsim.eval) re-queries: the expanded query is
    query_weight * q / |q| + sum_j w_j x_j / |x_j| over the first `n` results x_j of the previous ranking, with w_j from
    `expansion_weights(scores, scheme, alpha)`; `passes` > 1 repeats this from the lists of the expanded query (the sum always
    starts from the original query)."""

    def __init__(self, n: int = 10, scheme: str = "average", alpha: int = 3, query_weight: float = 1.0, passes: int = 1):
        _check_count("n", n)
        _check_scheme(scheme, alpha)
        _check_count("passes", passes)
        if isinstance(query_weight, bool) or not isinstance(query_weight, (int, float, np.integer, np.floating)) \
                or not math.isfinite(query_weight) or query_weight < 0:
            raise ValueError(f"query_weight must be a finite number >= 0, got {query_weight!r}")
        self.n, self.scheme, self.alpha, self.query_weight, self.passes = int(n), scheme, int(alpha), float(query_weight), int(passes)

    def __repr__(self):
        return (f"QueryExpansion(n={self.n}, scheme={self.scheme!r}, alpha={self.alpha}, query_weight={self.query_weight}, "
                f"passes={self.passes})")


def expansion_weights(scores: np.ndarray, scheme: str = "average", alpha: int = 3) -> np.ndarray:
    """(nq, n) similarities of the list entries, best first -> (nq, n) weights in the dtype of `scores`:
    "average" 1;  "alpha" max(s, 0) multiplied by itself alpha - 1 times, left to right (alpha = 0: 1) -- products, not pow, so
    that the bits are defined;  "linear" (n - j) / n for slot j."""
    _check_scheme(scheme, alpha)
    s = np.asarray(scores)
    if s.ndim != 2 or s.dtype not in (np.float32, np.float64):
        raise ValueError("scores must be a 2-d float32 or float64 array")
    t = s.dtype.type
    n = s.shape[1]
    if scheme == "linear":
        return np.broadcast_to((t(n) - np.arange(n, dtype=s.dtype)) / t(n), s.shape).copy()
    if scheme == "average" or alpha == 0:
        return np.ones_like(s)
    sp = np.maximum(s, t(0))
    w = sp.copy()
    for _ in range(alpha - 1):
        w = w * sp
    return w


def drop_self(idx: np.ndarray, val: np.ndarray, own: np.ndarray):
    """The lists of database rows ranked against their own index, without the row itself: from each row of idx / val (n, m) the
    first slot equal to own[i] is removed; where there is none (a duplicate or a tie took its place) the last slot is.
    -> (idx, val) of shape (n, m - 1)."""
    n, m = idx.shape
    hit = idx == np.asarray(own).reshape(n, 1)
    drop = np.where(hit.any(axis=1), hit.argmax(axis=1), m - 1)
    keep = np.arange(m)[None, :] != drop[:, None]
    return idx[keep].reshape(n, m - 1), val[keep].reshape(n, m - 1)
