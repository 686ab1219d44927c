"""Device time of the image-clustering path, one JSON line per shape: the kNN graph (pvs_l2_knn_dev), the spectral embedding,
k-means on the embedding, the distance-GEMM FLOP and its share of the matrix-pipe peak, and -- same shape, same k, same run --
pvs_cosine_topk_dev as the control.  An sklearn CPU time only if sklearn is importable, with the cgroup CPU quota as `cores`.
Run:  python tests/tools/cluster_timing.py [--shapes notebook,fisher,large]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "python-visual-similarity_amd"))

PEAK = {"f32": 157.3e12, "f64": 78.6e12}
SHAPES = {"notebook": (2040, 32768, np.float32, 10), "fisher": (2040, 131584, np.float64, 10),
          "large": (65536, 32768, np.float32, 10)}


def cgroup_cores():
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else float(q) / float(p)
    except (OSError, ValueError):
        return None


def timed(ctx, fn, reps=1):
    ctx.sync()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return (time.perf_counter() - t) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="notebook,fisher,large")
    ap.add_argument("--classes", type=int, default=102)
    a = ap.parse_args()
    import pvsim
    from pvsim import cluster
    ctx = pvsim.Context(0)
    for name in a.shapes.split(","):
        N, L, dt, k = SHAPES[name]
        rng = np.random.default_rng(5)
        X = np.empty((N, L), dtype=dt)
        for s in range(0, N, 1024):                      # planted classes, generated in slabs
            e = min(N, s + 1024)
            X[s:e] = rng.standard_normal((e - s, L), dtype=np.float32) * 0.5
        X += np.repeat(rng.standard_normal((a.classes, L), dtype=np.float32), -(-N // a.classes), axis=0)[:N].astype(dt)
        f64 = dt == np.float64
        xb = ctx.buffer(X.nbytes).upload(X)
        ib, db = ctx.buffer(N * k * 8), ctx.buffer(N * k * 8)
        knn = lambda: ctx.l2_knn_dev(xb.ptr, N, xb.ptr, N, L, f64, k, ib.ptr, db.ptr)  # noqa: E731
        st = ctx.l2_knn_dev(xb.ptr, N, xb.ptr, N, L, f64, k, ib.ptr, db.ptr, stats=True)   # warm-up (workspace, plans) + stats
        t_knn = timed(ctx, knn)
        rec = {"shape": name, "N": N, "L": L, "dtype": np.dtype(dt).name, "k": k, "knn_ms": round(t_knn, 3), "knn_stats": st}
        flop = 2.0 * N * N * L
        rec["gemm_flop"] = flop
        rec["gemm_share_of_peak"] = round(flop / (t_knn * 1e-3) / PEAK["f64" if f64 else "f32"], 4)
        if not f64:
            vb, xi = ctx.buffer(N * k * 4), ctx.buffer(N * k * 8)
            ctl = lambda: ctx.cosine_topk_dev(xb.ptr, N, xb.ptr, N, L, None, None, k, 0, 0, xi.ptr, vb.ptr)  # noqa: E731
            ctl()
            rec["cosine_topk_ms"] = round(timed(ctx, ctl), 3)
            rec["knn_over_cosine_topk"] = round(t_knn / rec["cosine_topk_ms"], 3)
            vb.free(); xi.free()
        idx = ib.download((N, k), np.int64)
        indptr = np.arange(0, N * k + 1, k, dtype=np.int64)
        if N <= 4096:
            t = time.perf_counter()
            maps, _, iters = cluster.spectral_embedding(indptr, idx.reshape(-1), N, a.classes, random_state=42, ctx=ctx)
            rec["embedding_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            rec["embedding_iterations"] = iters
            for key in ("kmeans_first_ms", "kmeans_ms"):     # the first call in the process, then a warm one
                t = time.perf_counter()
                cluster.kmeans(maps, a.classes, random_state=42, n_init=10, ctx=ctx)
                rec[key] = round((time.perf_counter() - t) * 1e3, 1)
        else:
            rec["embedding_ms"] = rec["kmeans_ms"] = "not measured"
        if name != "large":                                     # k-means on the encodings themselves (method='kmeans')
            t = time.perf_counter()
            cluster.kmeans(X, a.classes, random_state=42, ctx=ctx)
            rec["kmeans_encodings_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        xb.free(); ib.free(); db.free()
        try:
            from sklearn.neighbors import kneighbors_graph
            if N <= 4096:
                t = time.perf_counter()
                kneighbors_graph(X, k, include_self=True)
                rec["sklearn_knn_cpu_ms"] = round((time.perf_counter() - t) * 1e3, 1)
                rec["cores"] = cgroup_cores()
        except ImportError:
            pass
        print(json.dumps(rec), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
