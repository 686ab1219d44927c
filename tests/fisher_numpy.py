"""Extended-precision twin of the Fisher path -- TEST INFRASTRUCTURE ONLY.

Plain NumPy restatements, in np.longdouble, of the three operations the Fisher encoder is made of: the posterior
(oracle/pvsim_oracle.py:gmm_predict_proba), the Fisher vector of one image (fisher_encode_one) and PCA.transform.
The formulas are the oracle's, with its two float32 quirks kept: X**2 is squared in float32 before it is promoted,
and log(2 pi) is cast to the dtype of X.  The float64 oracle and the device are both float64 evaluations of the same
cancelling sums; the twin is what both are measured against (tests/fisher_cases.py: dev_ref).

Where np.longdouble carries no more digits than float64 the twin falls back to float64 (EXTENDED is False) and the
tests that need the extra digits skip with NEED_EXTENDED as the reason."""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np

EXTENDED = bool(np.finfo(np.longdouble).eps < 2.0 ** -53)
REAL = np.longdouble if EXTENDED else np.float64
NEED_EXTENDED = "np.longdouble is no wider than float64 on this machine: the twin has no digits to spare"


def _tables(weights, means, covariances):
    w = np.asarray(weights, np.float64).astype(REAL)
    mu = np.asarray(means, np.float64).astype(REAL)
    cov = np.asarray(covariances, np.float64).astype(REAL)
    return w, mu, cov


def _log_prob(x32, w, mu, cov):
    """Weighted log-densities (n, K) of float32 rows under REAL tables."""
    x = x32.astype(REAL)
    x2 = (x32 * x32).astype(REAL)                                   # squared in float32 first
    prec_chol = 1 / np.sqrt(cov)
    prec = prec_chol ** 2
    log_det = np.sum(np.log(prec_chol), axis=1)
    log_prob = np.sum(mu ** 2 * prec, axis=1) - 2 * (x @ (mu * prec).T) + x2 @ prec.T
    d_log2pi = REAL(mu.shape[1] * np.log(2 * np.pi).astype(x32.dtype))   # log(2 pi) in X's dtype
    return -(d_log2pi + log_prob) / 2 + log_det + np.log(w)


def _softmax(wlp):
    e = np.exp(wlp - np.max(wlp, axis=1, keepdims=True))           # one exp per entry: the same value to a few REAL ulps
    e /= np.sum(e, axis=1, keepdims=True)
    return e


def gmm_predict_proba(x, weights, means, covariances):
    """Responsibilities (n, K) in REAL of float32 rows x."""
    x32 = np.ascontiguousarray(x, dtype=np.float32)
    return _softmax(_log_prob(x32, *_tables(weights, means, covariances)))


def fisher_moments(desc, weights, means, covariances, block=4096):
    """(n, sum_i gamma (K), sum_i gamma x (K, D), sum_i gamma x**2 (K, D)) of one image in REAL.  The image goes through in
    row blocks, so the (n, K) responsibilities of a long image never exist at once."""
    w, mu, cov = _tables(weights, means, covariances)
    k, d = mu.shape
    n = 0 if desc is None else len(desc)
    s0 = np.zeros(k, REAL)
    s1 = np.zeros((k, d), REAL)
    s2 = np.zeros((k, d), REAL)
    x32 = np.ascontiguousarray(desc, dtype=np.float32) if n else None

    def one(i):
        xb = x32[i:i + block]
        g = _softmax(_log_prob(xb, w, mu, cov))
        return g.sum(axis=0), g.T @ xb.astype(REAL), g.T @ (xb * xb).astype(REAL)   # squared in float32 first

    starts = range(0, n, block)
    if len(starts) > 1:               # a long image: the blocks on a few threads (NumPy's loops release the lock), added in block order
        with ThreadPoolExecutor(max_workers=8) as pool:
            parts = list(pool.map(one, starts))
    else:
        parts = [one(i) for i in starts]
    for p0, p1, p2 in parts:
        s0 += p0
        s1 += p1
        s2 += p2
    return n, s0, s1, s2


def fisher_unnormalised(desc, weights, means, covariances, power=0.5, norm_order=2, block=4096, moments=None):
    """The power-normalised gradients [d_pi | d_mu | d_sigma] (REAL) of one image and their norm, before the division.
    An empty image gives a zero row with norm 0.  `moments` takes a fisher_moments result of the same image and tables."""
    w, mu, cov = _tables(weights, means, covariances)
    k, d = mu.shape
    n, s0, s1, s2 = moments if moments is not None else fisher_moments(desc, weights, means, covariances, block)
    if n == 0:
        return np.zeros(k + 2 * k * d, REAL), REAL(0)
    pp_sum = (s0 / n)[:, None]
    pp_x, pp_x2 = s1 / n, s2 / n
    sw = np.sqrt(w)
    d_pi = (pp_sum[:, 0] - w) / sw
    d_mu = (pp_x - pp_sum * mu) / (sw[:, None] * np.sqrt(cov))
    d_sg = (-pp_x2 - pp_sum * mu ** 2 + pp_sum * cov + 2 * pp_x * mu) / (np.sqrt(REAL(2)) * sw[:, None] * cov)
    v = np.concatenate((d_pi, d_mu.ravel(), d_sg.ravel()))
    v = np.sign(v) * np.abs(v) ** REAL(power)
    a = np.abs(v)
    if np.isinf(norm_order):
        nrm = a.max()
    elif norm_order == 1:
        nrm = a.sum()
    elif norm_order == 2:
        nrm = np.sqrt((v * v).sum())
    else:
        nrm = (a ** REAL(norm_order)).sum() ** (1 / REAL(norm_order))
    return v, nrm


def fisher_encode_one(desc, weights, means, covariances, power=0.5, norm_order=2, eps=1e-9, block=4096, moments=None):
    v, nrm = fisher_unnormalised(desc, weights, means, covariances, power, norm_order, block, moments)
    return v / (nrm + REAL(eps))


def fisher_encode(desc_list, weights, means, covariances, power=0.5, norm_order=2, eps=1e-9, moments=None):
    return np.vstack([fisher_encode_one(x, weights, means, covariances, power, norm_order, eps,
                                        moments=None if moments is None else moments[i]) for i, x in enumerate(desc_list)])


def fisher_rows_f32(desc_list, weights, means, covariances, power=0.5, norm_order=2, eps=1e-9, moments=None):
    """float32 rows as the device forms them: the gradients are stored as float32, the norm is taken from the float64
    values, and every stored element is divided in float64 and rounded once more: float32(float64(float32(v)) / den)."""
    rows = []
    for i, x in enumerate(desc_list):
        v, nrm = fisher_unnormalised(x, weights, means, covariances, power, norm_order,
                                     moments=None if moments is None else moments[i])
        den = np.float64(nrm + REAL(eps))
        rows.append((v.astype(np.float32).astype(np.float64) / den).astype(np.float32))
    return np.vstack(rows)


def pca_transform(x, components, mean):
    """PCA.transform in REAL: X @ comp^T - mean @ comp^T, and the magnitude sum_d |x_d| |comp_cd| + |off_c| that bounds
    the rounding of a float32 evaluation in any order.  -> (projected (n, C), magnitude (n, C))"""
    xr = np.ascontiguousarray(x, dtype=np.float32).astype(REAL)
    comp = np.asarray(components, np.float32).astype(REAL)
    off = comp @ np.asarray(mean, np.float32).astype(REAL).reshape(-1)
    return xr @ comp.T - off[None, :], np.abs(xr) @ np.abs(comp).T + np.abs(off)[None, :]
