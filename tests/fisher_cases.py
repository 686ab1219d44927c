"""Seeded inputs, case lists and tolerances of the Fisher edge tests -- shared by tests/test_fisher_host.py (which checks the
conditions on the inputs and prints dev_ref per family) and tests/test_gpu_fisher_edges.py (which compares the device with
the twin).  References are computed once per process and handed out unchanged.

Tolerance of a family = max(project constant, 16 x dev_ref), where dev_ref = max |float64 oracle - long-double twin| over the
family's inputs: the oracle and the device are both float64 evaluations of the same cancelling sums, so both errors scale with
the same condition number, and the factor 16 covers the device's different summation order.  dev_ref never comes from device
output.  Every family must keep 16 x dev_ref <= DEV_REF_CAP; a family that does not gets other inputs, not a wider bound."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import fisher_numpy as fnp
import pvsim_oracle as orc

RESP_ATOL = 1e-12        # responsibilities (tests/test_gpu_round2.py)
FISHER_ATOL = 1e-9       # Fisher rows (tests/test_gpu_parity.py)
DEV_REF_CAP = 1e-8
MEAN_SCALE = 1.0         # means ~ N(0, MEAN_SCALE^2 / D): the components overlap whatever D is
RAGGED = (0, 1, 2, 31, 32, 33, 127, 129, 300, 0)

# (p, norm order): every (PM, NM) instantiation of the fused epilogue -- PM: p == 1 / 0.5 / other; NM: L2 / abs-based / general
VARIANTS_ALL = [(p, o) for p in (1.0, 0.5, 0.3) for o in (2, 1, 3)] + [(0.5, np.inf)]
VARIANTS_4 = [(0.5, 2), (1.0, 1), (0.3, 3), (0.5, np.inf)]


def variant_id(v):
    return f"p{v[0]:g}-l{v[1]:g}"


# ------------------------------------------------------------------------------------------------ inputs
def gmm_tables(K, D, seed=0, floor=False, dup=False):
    """weights random + 0.2 (normalised), covariances random + 0.3, overlapping means.  floor: about 30 % of the covariance
    entries at 1e-6 (scikit-learn's floor).  dup: the last component is a copy of the first one."""
    rng = np.random.default_rng([K, D, seed, 11])
    w = rng.random(K) + 0.2
    mu = rng.normal(size=(K, D)) * (MEAN_SCALE / np.sqrt(D))
    cov = rng.random((K, D)) + 0.3
    if floor:
        cov[rng.random((K, D)) < 0.3] = 1e-6
    if dup:
        w[K - 1], mu[K - 1], cov[K - 1] = w[0], mu[0], cov[0]
    w /= w.sum()
    return w, mu, cov


def draw(tab, n, seed=0, far=False):
    """n float32 rows drawn from the mixture.  far: every second row shifted by +50."""
    w, mu, cov = tab
    K, D = mu.shape
    rng = np.random.default_rng([K, D, n, seed, 23])
    comp = rng.choice(K, size=n, p=w)
    x = (mu[comp] + rng.normal(size=(n, D)) * np.sqrt(cov[comp])).astype(np.float32)
    if far:
        x[1::2] += np.float32(50.0)
    return x


def ragged_images(tab, counts=RAGGED, seed=0):
    rows = draw(tab, int(sum(counts)), seed)
    off = np.concatenate(([0], np.cumsum(counts)))
    return [rows[off[i]:off[i + 1]] for i in range(len(counts))]


# ------------------------------------------------------------------------------------------------ posterior cases
# (K, D, rows).  A covering set: every K, D and row count of each kernel appears, and every kernel meets a row tail.
POSTERIOR_CASES = {
    "post_mfma": [(1, 1, 1), (15, 7, 127), (17, 8, 128), (64, 9, 129), (65, 33, 300), (255, 1, 129), (256, 7, 300),
                  (256, 33, 128), (17, 9, 127), (64, 8, 1)],
    "post_vec32": [(257, 1, 1), (300, 63, 31), (512, 64, 32), (257, 65, 33), (300, 130, 100), (512, 65, 33), (257, 64, 31)],
    "post_vec16": [(513, 1, 1), (1024, 63, 15), (513, 64, 16), (1024, 65, 17), (513, 130, 100), (1024, 130, 17), (1024, 1, 100),
                   (513, 65, 15)],
}
EXTRA_SHAPES = [(64, 9, 129), (300, 63, 100)]      # one MFMA shape, one vector shape
for _name in ("far", "dup", "floor"):
    POSTERIOR_CASES["post_" + _name] = list(EXTRA_SHAPES)
# far rows: the window in which a float64 result is a denormal and not zero; no twin value of the far inputs may lie in it
# (a condition on the inputs, asserted on the host), so "exactly 0.0 below 1e-320" is a claim any correct float64 path meets
DENORMAL_WINDOW = (np.longdouble("1e-330"), np.longdouble("1e-320"))
FAR_SEED = 5             # seeds 0..11 leave 0 to 16 of the ~20 000 underflowing values in the window; this one leaves none at either shape


@lru_cache(maxsize=None)
def posterior_case(family, K, D, n):
    """-> (tables, rows float32, twin responsibilities)"""
    kind = family[5:]
    seed = FAR_SEED if kind == "far" else 0
    tab = gmm_tables(K, D, seed, floor=kind == "floor", dup=kind == "dup")
    x = draw(tab, n, seed, far=kind == "far")
    ref = fnp.gmm_predict_proba(x, *tab)
    for a in (*tab, x, ref):
        a.setflags(write=False)
    return tab, x, ref


@lru_cache(maxsize=None)
def posterior_dev_ref(family):
    worst = 0.0
    for K, D, n in POSTERIOR_CASES[family]:
        tab, x, ref = posterior_case(family, K, D, n)
        worst = max(worst, float(np.abs(orc.gmm_predict_proba(x, *tab) - ref).max()))
    return worst


def posterior_tol(family):
    return max(RESP_ATOL, 16 * posterior_dev_ref(family))


# ------------------------------------------------------------------------------------------------ Fisher cases
class FisherCase:
    """Tables, images and the twin's moments of the images that are compared (all of them unless `sel` is given)."""

    def __init__(self, tab, imgs, sel=None):
        self.tab, self.imgs = tab, imgs
        self.sel = list(range(len(imgs))) if sel is None else list(sel)
        self.K, self.D = tab[1].shape
        self.L = self.K + 2 * self.K * self.D
        self._mom = None

    @property
    def moments(self):
        if self._mom is None:
            self._mom = [fnp.fisher_moments(self.imgs[i], *self.tab) for i in self.sel]
        return self._mom

    def twin(self, power=0.5, order=2, eps=1e-9):
        return fnp.fisher_encode([self.imgs[i] for i in self.sel], *self.tab, power, order, eps, moments=self.moments)

    def twin_f32(self, power=0.5, order=2, eps=1e-9):
        return fnp.fisher_rows_f32([self.imgs[i] for i in self.sel], *self.tab, power, order, eps, moments=self.moments)

    def oracle(self, power=0.5, order=2, eps=1e-9):
        return orc.fisher_encode([self.imgs[i] for i in self.sel], *self.tab, power, order, eps)


VECTOR_SHAPES = [(257, 33), (300, 130), (513, 5), (1024, 3)]     # bt = 128 and 256, a partial last 16-cluster block, both posterior widths
MFMA_SHAPES = [(1, 1), (7, 31), (16, 32), (41, 33), (255, 65), (256, 2)]
SCALE_SHAPES = [(41, 33), (7, 31), (16, 32), (255, 65)]           # odd L twice; L * 4 divisible by 16; a row long enough for the unrolled loop
KIND_SHAPES = [(17, 2), (17, 65), (257, 130)]
SEAM_IMAGES = 65540
SEAM_SPLIT = 40000
SEAM_SEL = [0, 1, 2, 3] + list(range(65530, 65540))
BYTES_SHAPE, BYTES_ROWS, BYTES_IMAGES = (1024, 2), 100_000, 5       # 0.82 GB of responsibilities per image: batches of 3 and 2
PCA_SHAPES = [(1, 1), (17, 3), (130, 65), (128, 64)]              # (Din, C)
PCA_ROWS = [1, 63, 64, 65]
PCA_FISHER = (130, 65, 41)                                          # Din -> C, K


@lru_cache(maxsize=None)
def ragged_case(K, D, floor=False):
    tab = gmm_tables(K, D, floor=floor)
    return FisherCase(tab, ragged_images(tab))


def seam_counts():
    c = np.tile(np.array([0, 1, 2], np.int64), SEAM_IMAGES // 3 + 1)[:SEAM_IMAGES]
    c[65533:65538] = (3, 0, 5, 1, 4)
    return c


@lru_cache(maxsize=None)
def seam_case(K, D):
    tab = gmm_tables(K, D)
    return FisherCase(tab, ragged_images(tab, seam_counts()), SEAM_SEL)


@lru_cache(maxsize=None)
def bytes_case():
    tab = gmm_tables(*BYTES_SHAPE)
    return FisherCase(tab, ragged_images(tab, (BYTES_ROWS,) * BYTES_IMAGES), [3])


def kind_rows(D):
    """uint8 rows for the RootSIFT kinds in the ragged layout; row 5 is all zero."""
    rng = np.random.default_rng([D, 31])
    raw = rng.integers(0, 256, size=(int(sum(RAGGED)), D), dtype=np.uint8)
    raw[5] = 0
    return raw


@lru_cache(maxsize=None)
def kind_case(K, D):
    tab = gmm_tables(K, D)
    rows = orc.rootsift(kind_rows(D).astype(np.float32))
    off = np.concatenate(([0], np.cumsum(RAGGED)))
    return FisherCase(tab, [rows[off[i]:off[i + 1]] for i in range(len(RAGGED))])


def pca_tables(Din, C):
    rng = np.random.default_rng([Din, C, 41])
    comp = rng.normal(size=(C, Din)).astype(np.float32) / np.float32(np.sqrt(Din))
    mean = (rng.random(Din) + 0.5).astype(np.float32)
    return comp, mean


def pca_rows(Din, n):
    rng = np.random.default_rng([Din, n, 43])
    return (rng.random((n, Din)) * 2).astype(np.float32)


def pca_fisher_inputs():
    """-> (components, mean, tables over the projected space, unprojected rows in the ragged layout)"""
    Din, C, K = PCA_FISHER
    comp, mean = pca_tables(Din, C)
    return comp, mean, gmm_tables(K, C), pca_rows(Din, int(sum(RAGGED)))


def split_ragged(rows, counts=RAGGED):
    off = np.concatenate(([0], np.cumsum(counts)))
    return [rows[off[i]:off[i + 1]] for i in range(len(counts))]


@lru_cache(maxsize=None)
def pca_fisher_case():
    comp, mean, tab, rows = pca_fisher_inputs()
    return FisherCase(tab, split_ragged(orc.pca_transform(rows, comp, mean)))


def fisher_families():
    """family -> [(case, variants)]"""
    return {
        "fisher_vector": [(ragged_case(K, D), VARIANTS_4) for K, D in VECTOR_SHAPES],
        "fisher_vector_floor": [(ragged_case(257, 33, True), [(0.5, 2)])],
        "fisher_mfma": [(ragged_case(K, D), VARIANTS_ALL) for K, D in MFMA_SHAPES],
        "fisher_seam_images": [(seam_case(3, 2), [(0.5, 2)]), (seam_case(257, 2), [(0.5, 2)])],
        "fisher_seam_bytes": [(bytes_case(), [(0.5, 2)])],
        "fisher_kinds": [(kind_case(K, D), [(0.5, 2)]) for K, D in KIND_SHAPES],
        "fisher_pca": [(pca_fisher_case(), [(0.5, 2)])],
    }


@lru_cache(maxsize=None)
def fisher_dev_ref(family):
    worst = 0.0
    for case, variants in fisher_families()[family]:
        for p, o in variants:
            worst = max(worst, float(np.abs(case.oracle(p, o) - case.twin(p, o)).max()))
    return worst


def fisher_tol(family):
    return max(FISHER_ATOL, 16 * fisher_dev_ref(family))


def f32_tol(restated, family):
    """One float32 ulp of the restated value plus the float64 bound."""
    return np.spacing(np.abs(restated).astype(np.float32)).astype(np.float64) + fisher_tol(family)
