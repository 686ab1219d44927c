"""Timing of query expansion and database-side augmentation (csrc/expand.hip, pvsim/expand.py) at the headline corpus.

    python tests/tools/expand_timing.py [--steps 5] [--warmup 1] [--n 8189] [--dim 32768] [--r 10] [--out profiles/expand_timing.jsonl]

Corpus: n float32 rows of `dim` columns, planted in classes of 32 so that neighbour lists overlap the way real ones do.
  combine   pvs_combine_rows_dev alone over all n rows with their r nearest rows (and once with uniformly random lists), timed by
            the context's event timer (slot misc holds nothing else in that window).  `bytes` is what the algorithm moves,
            (n (r + 1) + n) dim 4: r + 1 rows read and one written per output row; `share_of_copy_rate` is bytes / time over the
            6.29 TB/s a float4 copy reaches on this device (MI355X_MICROARCH.md).  Lists that overlap are served partly from
            cache, so the figure is an algorithmic rate, not a DRAM rate.
  dba       DeviceIndex.augmented(r): wall time of the whole call (ranking in blocks, lists down, weights up, combine, the host
            copy of the new rows, its norms) and its split by the event timers.
  aqe       DeviceIndex.rank_expanded against DeviceIndex.rank for nq = 1 and nq = 1024, k = 10, QueryExpansion(n = 10), same run.
Appends one JSON line.  Nothing here is a pass / fail threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "python-visual-similarity_amd"))

COPY_RATE = 6.29e12        # bytes/s of a float4 copy, measured (MI355X_MICROARCH.md)


def _stats(samples):
    a = np.sort(np.asarray(samples))
    return {"median": round(float(np.median(a)), 4), "min": round(float(a[0]), 4), "max": round(float(a[-1]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=int, default=8189)
    ap.add_argument("--dim", type=int, default=32768)
    ap.add_argument("--r", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "expand_timing.jsonl"))
    args = ap.parse_args()

    import pvsim
    from pvsim import QueryExpansion
    from pvsim.expand import drop_self
    from pvsim.index import DeviceIndex

    ctx = pvsim.Context(0)
    rng = np.random.default_rng(13)
    n, L, r, k = args.n, args.dim, args.r, 10
    classes = max(1, n // 32)
    centres = rng.standard_normal((classes, L), dtype=np.float32)
    lab = rng.integers(0, classes, n)
    rows = centres[lab]
    rows += rng.standard_normal((n, L), dtype=np.float32)
    del centres
    rec = {"device": ctx.device_name(), "date": time.strftime("%Y-%m-%d"), "n": n, "dim": L, "r": r, "k": k, "dtype": "float32",
           "steps": args.steps, "warmup": args.warmup, "chunk_bytes": ctx.COMBINE_CHUNK_BYTES, "batch": ctx.COMBINE_BATCH,
           "grid_order": "row fastest, column chunk slowest"}
    index = DeviceIndex({str(i): rows[i] for i in range(n)}, ctx)
    del rows

    def timed(fn, steps=args.steps, warmup=args.warmup):
        for _ in range(warmup):
            fn()
        ctx.sync()
        wall = []
        ctx.timers_enable(True)
        ctx.timers_reset()
        for _ in range(steps):
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            wall.append((time.perf_counter() - t0) * 1e3)
        t = ctx.timers()
        ctx.timers_enable(False)
        return _stats(wall), {name + "_ms": round(ms / steps, 4) for name, (ms, cnt) in t.items() if cnt}

    # ---- the combine kernel alone
    idx, val = drop_self(*index.rank(index.matrix, r + 1), np.arange(n))
    w = index._list_weights(idx, val, "linear", 3)
    d_out = ctx.buffer(n * L * 4)
    d_ws = ctx.buffer(n * 4).upload(index.inv_norms)
    d_w = ctx.buffer(w.nbytes).upload(w)
    d_idx = ctx.buffer(idx.nbytes)
    nbytes = (n * (r + 1) + n) * L * 4
    for name, lists in (("neighbour_lists", idx), ("random_lists", rng.integers(0, n, (n, r)).astype(np.int64))):
        d_idx.upload(lists)
        wall, split = timed(lambda: ctx.combine_rows_dev(index._db.ptr, n, L, False, index._db.ptr, d_ws.ptr, d_idx.ptr, d_w.ptr, n, r,
                                                         d_out.ptr), steps=max(args.steps, 10), warmup=2)
        ms = split["misc_ms"]
        rec["combine_" + name] = {"kernel_ms": ms, "wall_ms": wall, "bytes": nbytes, "bytes_per_s": nbytes / (ms * 1e-3),
                                  "share_of_copy_rate": round(nbytes / (ms * 1e-3) / COPY_RATE, 4),
                                  "distinct_rows_read": int(np.unique(lists).size)}
    for b in (d_out, d_ws, d_w, d_idx):
        b.free()

    # ---- database-side augmentation, the whole call
    made = []

    def dba():
        for a in made:
            a.close()
        made[:] = [index.augmented(r=r, scheme="linear")]
    wall, split = timed(dba, steps=max(2, args.steps // 2))
    rec["dba"] = {"total_ms": wall, **split}
    for a in made:
        a.close()

    # ---- query expansion beside the plain ranking
    qe = QueryExpansion(n=10)
    for nq in (1, 1024):
        q = index.matrix[rng.integers(0, n, nq)] + rng.standard_normal((nq, L), dtype=np.float32)
        plain_wall, plain_split = timed(lambda: index.rank(q, k))
        exp_wall, exp_split = timed(lambda: index.rank_expanded(q, k, qe))
        rec[f"aqe_nq{nq}"] = {"rank_ms": plain_wall, "rank_expanded_ms": exp_wall, "rank_split": plain_split, "rank_expanded_split": exp_split}
    index.close()
    print(json.dumps(rec), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
