"""Golden results of the reference's image clustering (pyvisim/_utils.py:128-162 cluster_and_return_labels, :333-361
cluster_images_and_generate_statistics) on the seeded sets of cluster_inputs.py.

Imports the REFERENCE through the stand-ins of make_golden.py (nothing copied), pins one BLAS / OpenMP thread, calls its
_utils functions and records labels and scores per method, scikit-learn's kneighbors lists and squared distances, the radius
graph, DBSCAN core indices and labels, and (easy set) the spectral embedding and its leading eigenvalues; for the notebook-shaped
set the kNN lists and the spread of sklearn's k-means / spectral scores over ten random states.  Arrays only; the
inputs are stored as their seeds.  Writes tests/golden/cluster_<set>.npz.
Run:  python tests/golden/make_golden_cluster.py [--check]
"""
import os
import sys

os.environ["OMP_NUM_THREADS"] = "1"
os.environ["OPENBLAS_NUM_THREADS"] = "1"
os.environ["MKL_NUM_THREADS"] = "1"
sys.dont_write_bytecode = True
import warnings  # noqa: E402

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from cluster_inputs import SETS, cluster_set  # noqa: E402
from make_golden import _import_reference  # noqa: E402

K_NN = 10
PARAMS = {"easy": dict(eps=6.0, min_samples=5), "f64": dict(eps=6.6, min_samples=5)}


def record(name, ref_utils):
    from sklearn.cluster import DBSCAN
    from sklearn.manifold import spectral_embedding
    from sklearn.neighbors import NearestNeighbors, kneighbors_graph
    X, y = cluster_set(name)
    nc = SETS[name]["n_classes"]
    eps, ms = PARAMS[name]["eps"], PARAMS[name]["min_samples"]
    out = {"seed": np.int64(SETS[name]["seed"]), "labels_true": y, "eps": np.float64(eps), "min_samples": np.int64(ms)}
    nn = NearestNeighbors(n_neighbors=K_NN).fit(X)
    dist, idx = nn.kneighbors(X)
    # sklearn returns the distances in the rows' dtype; its ranking value is the float64 one, recomputed here for its lists
    Xd = X.astype(np.float64)
    n2 = (Xd * Xd).sum(1)
    out["norm_sq"] = n2
    D2 = np.maximum(0.0, n2[:, None] + n2[None, :] - 2 * Xd @ Xd.T)
    out["knn_idx"], out["knn_dist"] = idx.astype(np.int64), dist
    out["knn_sqdist"] = np.take_along_axis(D2, idx, axis=1)
    rad = NearestNeighbors(radius=eps).fit(X).radius_neighbors(X, return_distance=True, sort_results=False)
    out["radius_indptr"] = np.concatenate([[0], np.cumsum([len(r) for r in rad[1]])]).astype(np.int64)
    out["radius_indices"] = np.concatenate(rad[1]).astype(np.int64)
    # how close the closest pair is to the threshold (relative): the fixture is only meaningful if this is far above rounding
    out["radius_margin_rel"] = np.float64(np.min(np.abs(D2 - eps * eps)) / (eps * eps))
    db = DBSCAN(eps=eps, min_samples=ms).fit(X)
    out["dbscan_core"] = db.core_sample_indices_.astype(np.int64)
    out["dbscan_labels"] = ref_utils.cluster_and_return_labels(X, method="dbscan", eps=eps, min_samples=ms).astype(np.int64)
    for method in ("kmeans", "spectral"):
        out[f"{method}_labels"] = ref_utils.cluster_and_return_labels(X, method=method, n_clusters=nc).astype(np.int64)
    # k-means with ten k-means++ starts: a single start may stop in a local optimum that depends on the random stream
    out["kmeans10_labels"] = ref_utils.cluster_and_return_labels(X, method="kmeans", n_clusters=nc, n_init=10).astype(np.int64)
    for method in ("kmeans", "spectral", "dbscan"):
        kw = dict(eps=eps, min_samples=ms) if method == "dbscan" else {}
        st = ref_utils.cluster_images_and_generate_statistics(X, y, nc, method=method, **kw)
        out[f"{method}_stats"] = np.array([st["ri"], st["ari"], st["nmi"]], dtype=np.float64)
    if name == "easy":
        C = kneighbors_graph(X, n_neighbors=K_NN, include_self=True)
        A = 0.5 * (C + C.T)
        emb = spectral_embedding(A, n_components=nc, random_state=np.random.RandomState(42), drop_first=False)
        out["embedding"] = emb.astype(np.float64)
        from scipy.sparse.csgraph import laplacian
        Lap = laplacian(A, normed=True).toarray()
        np.fill_diagonal(Lap, 1.0)
        out["laplacian_eigs"] = np.linalg.eigvalsh(Lap)[:nc + 4]
    return out


def record_notebook(ref_utils):
    """The notebook-shaped set (2040 x 32768 f32, 102 classes): sklearn's kNN lists, the reference's labels and scores
    (random_state 42), and the spread of sklearn's own scores over random_state 0..9 (k-means' and spectral's random draws)."""
    from sklearn.cluster import KMeans, SpectralClustering
    from sklearn.metrics import adjusted_mutual_info_score, adjusted_rand_score
    from sklearn.neighbors import NearestNeighbors
    X, y = cluster_set("notebook")
    nc = SETS["notebook"]["n_classes"]
    out = {"seed": np.int64(SETS["notebook"]["seed"]), "labels_true": y}
    dist, idx = NearestNeighbors(n_neighbors=K_NN).fit(X).kneighbors(X)
    Xd = X.astype(np.float64)
    n2 = (Xd * Xd).sum(1)
    D2 = np.maximum(0.0, n2[:, None] + n2[None, :] - 2 * Xd @ Xd.T)
    out["norm_sq"], out["knn_idx"], out["knn_dist"] = n2, idx.astype(np.int64), dist
    out["knn_sqdist"] = np.take_along_axis(D2, idx, axis=1)
    for method in ("kmeans", "spectral"):
        st = ref_utils.cluster_images_and_generate_statistics(X, y, nc, method=method)
        out[f"{method}_stats"] = np.array([st["ri"], st["ari"], st["nmi"]], dtype=np.float64)
        spread = []
        for rs in range(10):
            if method == "kmeans":
                lab = KMeans(n_clusters=nc, random_state=rs).fit_predict(X)
            else:
                lab = SpectralClustering(n_clusters=nc, affinity="nearest_neighbors", random_state=rs).fit_predict(X)
            spread.append([adjusted_rand_score(y, lab), adjusted_mutual_info_score(y, lab)])
        out[f"{method}_spread"] = np.array(spread, dtype=np.float64)     # (10, 2): ARI, AMI per random_state
    return out


def main(check=False):
    warnings.simplefilter("ignore")
    _import_reference()
    import pyvisim._utils as ref_utils
    bad = []
    for name in ("easy", "f64", "notebook"):
        out = record_notebook(ref_utils) if name == "notebook" else record(name, ref_utils)
        path = os.path.join(HERE, f"cluster_{name}.npz")
        if check:
            old = np.load(path)
            for k, v in out.items():
                if k not in old or old[k].shape != np.shape(v) or not np.allclose(old[k], v, rtol=1e-9, atol=1e-12):
                    bad.append(f"{name}:{k}")
        else:
            np.savez_compressed(path, **out)
            print("wrote", path, os.path.getsize(path), "bytes")
    if check:
        print("cluster fixtures:", "OK" if not bad else f"DIFFER {bad}")
        return 1 if bad else 0
    return 0


if __name__ == "__main__":
    sys.exit(main("--check" in sys.argv))
