"""Seeded planted-class encodings for the image-clustering fixtures (make_golden_cluster.py) and tests; the fixture stores the
seeds, not the rows (numpy's Generator streams are version-stable)."""
import numpy as np


def planted(n, n_classes, L, seed, dtype=np.float32, spread=0.35, blocks=64, n_dup=6):
    """Class centres plus noise, VLAD-like per-block normalisation (each of `blocks` blocks of a row scaled to unit norm, empty
    blocks left zero), so rows are not unit-norm; the last n_dup rows repeat earlier rows exactly (ties in the neighbour lists).
    -> (X (n, L), labels (n,) int64)"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_classes, L))
    y = np.sort(rng.integers(0, n_classes, size=n))
    X = centres[y] + spread * rng.standard_normal((n, L))
    bl = L // blocks
    Xb = X[:, :bl * blocks].reshape(n, blocks, bl)
    empty = rng.random((n, blocks)) < 0.1
    Xb[empty] = 0.0
    nrm = np.linalg.norm(Xb, axis=2, keepdims=True)
    Xb /= np.where(nrm > 0, nrm, 1.0)
    X[:, :bl * blocks] = Xb.reshape(n, bl * blocks)
    X = X.astype(dtype)
    if n_dup:
        src = rng.choice(n - n_dup, size=n_dup, replace=False)
        X[n - n_dup:] = X[src]
        y[n - n_dup:] = y[src]
    return np.ascontiguousarray(X), y.astype(np.int64)


SETS = {
    # well-separated, a clear spectral gap: spectral / k-means labels equal the reference's up to a permutation
    "easy": dict(n=480, n_classes=16, L=256, seed=9101, dtype=np.float32, spread=0.25),
    # float64 rows, smaller L
    "f64": dict(n=300, n_classes=8, L=130, seed=9102, dtype=np.float64, spread=0.6),
    # notebook-shaped: 2040 images, 102 classes, L = 32768 float32
    "notebook": dict(n=2040, n_classes=102, L=32768, seed=9103, dtype=np.float32, spread=1.2, blocks=256),
}


def cluster_set(name):
    return planted(**SETS[name])
