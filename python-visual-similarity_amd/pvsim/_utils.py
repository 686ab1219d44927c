"""The helpers of pyvisim/_utils.py that do arithmetic: the image validator that gates every extractor call (:34-53),
cosine_similarity (:312-330), and the image-clustering pair cluster_and_return_labels (:128-162) /
cluster_images_and_generate_statistics (:333-361), whose cost is an exact neighbour search over the encodings (pvsim.cluster,
on the device).  The plotting / HDF5 conveniences of the reference are out of scope."""
from __future__ import annotations

import numpy as np

from ._errors import InvalidImageError

__all__ = ["is_numpy_image", "cosine_similarity", "cluster_and_return_labels", "cluster_images_and_generate_statistics"]


def is_numpy_image(image: np.ndarray, pos: int) -> None:
    """2-D arrays must be integer valued (masks); 3-D arrays must be (H, W, 3) within [0, 255]."""
    if len(image.shape) == 2:
        if not np.all(image == image.astype(np.int64)):
            raise InvalidImageError(f"Mask values must be integers. Got min={image.min()} and max={image.max()}.")
    else:
        if image.shape[2] != 3:
            raise InvalidImageError(f"NumPy 3D images must have shape (H, W, 3). Got {image.shape}.")
        if image.min() < 0 or image.max() > 255:
            raise InvalidImageError(
                f"Image values must be in the range [0, 255]. Got min={image.min()} and max={image.max()} "
                f"for position {pos}.")


def _to_numpy(x):
    try:
        import torch
        if isinstance(x, torch.Tensor):
            return x.cpu().numpy()
    except ImportError:  # torch is optional for this function
        pass
    return np.asarray(x)


def cosine_similarity(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """(N, L), (M, L) -> (N, M) cosine similarities, computed on the MI355X.

    Same contract as pyvisim._utils.cosine_similarity: torch tensors are accepted, 1-D inputs become
    one row, fewer than 2 features raise ValueError, the result is float32 iff both operands are float32
    (else float64), zero rows give zero similarity."""
    from .engine import default_context
    x, y = _to_numpy(x), _to_numpy(y)
    x = x.reshape(1, -1) if len(x.shape) == 1 else x
    y = y.reshape(1, -1) if len(y.shape) == 1 else y
    if x.shape[-1] <= 1 or y.shape[-1] <= 1:
        raise ValueError(f"Cosine similarity requires at least 2 features. Got {x.shape[-1]} features for x "
                         f"and {y.shape[-1]} features for y.")
    if x.dtype not in (np.float32, np.float64):
        x = x.astype(np.float64)
    if y.dtype not in (np.float32, np.float64):
        y = y.astype(np.float64)
    return default_context().cosine(x, y)


# keyword arguments of the sklearn estimators the reference constructs (scikit-learn 1.7.2)
_KMEANS_KW = {"init", "n_init", "max_iter", "tol", "verbose", "copy_x", "algorithm"}
_DBSCAN_KW = {"eps", "min_samples", "metric", "metric_params", "algorithm", "leaf_size", "p", "n_jobs"}
_SPECTRAL_KW = {"eigen_solver", "n_components", "n_init", "gamma", "n_neighbors", "eigen_tol", "assign_labels", "degree",
                "coef0", "kernel_params", "n_jobs", "verbose"}


def _unknown(kwargs, known, name):
    bad = sorted(set(kwargs) - known)
    if bad:
        raise TypeError(f"{name}.__init__() got an unexpected keyword argument {bad[0]!r}")


def cluster_and_return_labels(data: np.ndarray, method: str = "kmeans", n_clusters=None, **kwargs) -> np.ndarray:
    """Clusters `data` (N, D) with 'kmeans', 'dbscan' or 'spectral' on the MI355X; same signature, defaults
    (random_state=42) and errors as pyvisim._utils.cluster_and_return_labels.

    kmeans:   KMeans(n_clusters, random_state=42, **kwargs).fit_predict -- pvsim.learn.fit_kmeans; the device Lloyd is float32,
              so float64 rows are clustered as their float32 rounding.
    dbscan:   DBSCAN(**kwargs).fit_predict -- eps (0.5), min_samples (5); Euclidean only.  Labels are sklearn's exactly.
    spectral: SpectralClustering(n_clusters, affinity='nearest_neighbors', random_state=42, **kwargs).fit_predict -- the kNN
              graph is sklearn's; the embedding comes from a block eigensolver instead of ARPACK, and the random draws are not
              sklearn's draw for draw.
    Options that cannot change the result (algorithm, leaf_size, n_jobs, verbose, copy_x) are accepted and ignored; sklearn
    options that are not built raise NotImplementedError; names sklearn does not know raise TypeError."""
    from . import cluster
    if method == "kmeans":
        if n_clusters is None:
            raise ValueError("n_clusters must be specified for KMeans.")
        _unknown(kwargs, _KMEANS_KW | {"random_state"}, "KMeans")
        kw = {k: v for k, v in kwargs.items() if k not in ("copy_x",)}
        kw.setdefault("random_state", 42)
        return cluster.kmeans(data, n_clusters, **kw)
    if method == "dbscan":
        _unknown(kwargs, _DBSCAN_KW, "DBSCAN")
        metric = kwargs.get("metric", "euclidean")
        if metric not in ("euclidean", "l2", "minkowski") or (metric == "minkowski" and kwargs.get("p", 2) not in (2, None)):
            raise NotImplementedError(f"DBSCAN metric={metric!r}: only the Euclidean metric is built")
        if kwargs.get("p") not in (None, 2):
            raise NotImplementedError(f"DBSCAN p={kwargs['p']!r}: only the Euclidean metric is built")
        if kwargs.get("metric_params"):
            raise NotImplementedError("DBSCAN metric_params: only the Euclidean metric is built")
        return cluster.dbscan(data, eps=kwargs.get("eps", 0.5), min_samples=kwargs.get("min_samples", 5))
    if method == "spectral":
        if n_clusters is None:
            raise ValueError("n_clusters must be specified for Spectral Clustering.")
        _unknown(kwargs, _SPECTRAL_KW | {"random_state"}, "SpectralClustering")
        if kwargs.get("assign_labels", "kmeans") != "kmeans":
            raise NotImplementedError(f"SpectralClustering assign_labels={kwargs['assign_labels']!r}: only 'kmeans' is built")
        if kwargs.get("eigen_solver") not in (None, "arpack", "lobpcg"):
            raise NotImplementedError(f"SpectralClustering eigen_solver={kwargs['eigen_solver']!r} is not built")
        return cluster.spectral_clustering(data, n_clusters, n_neighbors=kwargs.get("n_neighbors", 10),
                                           n_components=kwargs.get("n_components"), n_init=kwargs.get("n_init", 10),
                                           eigen_tol=kwargs.get("eigen_tol", "auto"),
                                           random_state=kwargs.get("random_state", 42))
    raise ValueError(f"Unknown method: {method}")


def cluster_images_and_generate_statistics(features: np.ndarray, true_labels: np.ndarray, n_clusters: int,
                                           method: str = "kmeans", **kwargs) -> dict:
    """Clusters the features (cluster_and_return_labels; dbscan gets n_clusters=None) and scores the labels against the
    truth: {"ri": rand_score, "ari": adjusted_rand_score, "nmi": adjusted_mutual_info_score}.  As in the reference, the
    "nmi" key holds the ADJUSTED mutual information (average_method='arithmetic')."""
    from .cluster import adjusted_mutual_info_score, adjusted_rand_score, rand_score
    labels = cluster_and_return_labels(data=features, method=method, n_clusters=n_clusters if method != "dbscan" else None,
                                       **kwargs)
    return {"ri": rand_score(true_labels, labels), "ari": adjusted_rand_score(true_labels, labels),
            "nmi": adjusted_mutual_info_score(true_labels, labels)}
