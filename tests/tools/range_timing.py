"""Timing of the cosine threshold join and the pair components (csrc/range.hip, pvsim/duplicates.py) at the headline
corpus.

    python tests/tools/range_timing.py [--steps 5] [--warmup 1] [--n 8189] [--dim 32768] [--pairs 4000] [--out profiles/range_timing.jsonl]

Corpus: n float32 rows of `dim` columns, random directions, with `pairs` planted near duplicates v = c u + sqrt(1 - c^2) w whose cosine c
is drawn from [0.80, 1.00]; the threshold is 0.9, so about half of them are hits and the prefilter sees a band of candidates around it.
All in one process:
  self_join    index.similar_pairs(0.9, path=...) for "exact" and "filtered": the whole Python call (join, download, sort), and the
               device call alone (pvs_cosine_range_dev into preallocated buffers), split by the context's event timers.
  search_1, search_1024   index.range_search(queries, 0.9, path=...) for 1 and 1024 queries on both paths, beside index.rank(queries, 10).
  components   pvs_pair_components_dev alone on the pair list of the join, left on the device.
Every time is wall time ended by a synchronise: median, min and max of `steps` rounds after `warmup`.  Appends one JSON line.  Nothing
here is a pass / fail threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "python-visual-similarity_amd"))


def _stats(samples):
    a = np.sort(np.asarray(samples, dtype=np.float64))
    return {"median": round(float(np.median(a)), 4), "min": round(float(a[0]), 4), "max": round(float(a[-1]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=int, default=8189)
    ap.add_argument("--dim", type=int, default=32768)
    ap.add_argument("--pairs", type=int, default=4000)
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "range_timing.jsonl"))
    args = ap.parse_args()

    import pvsim
    from pvsim import _ffi
    from pvsim.index import DeviceIndex

    ctx = pvsim.Context(0)
    rng = np.random.default_rng(24)
    n, L, t = args.n, args.dim, args.threshold
    npairs = min(args.pairs, n // 2)
    rows = rng.standard_normal((n, L), dtype=np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    place = rng.permutation(n)[:2 * npairs].reshape(npairs, 2)
    cos = rng.uniform(0.80, 1.00, npairs).astype(np.float32)
    rows[place[:, 1]] = cos[:, None] * rows[place[:, 0]] + np.sqrt(1 - cos * cos)[:, None] * rows[place[:, 1]]
    rec = {"device": ctx.device_name(), "date": time.strftime("%Y-%m-%d"), "n": n, "dim": L, "planted_pairs": int(npairs),
           "threshold": float(np.float32(t)), "dtype": "float32", "steps": args.steps, "warmup": args.warmup}
    index = DeviceIndex({str(i): rows[i] for i in range(n)}, ctx)
    queries = np.ascontiguousarray(rows[rng.integers(0, n, 1024)])
    del rows
    ctx.timers_enable(True)

    def timed(fn):
        wall, split = [], {}
        for it in range(args.warmup + args.steps):
            ctx.sync()
            ctx.timers_reset()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            ms = (time.perf_counter() - t0) * 1e3
            if it >= args.warmup:
                wall.append(ms)
                for name, (tt, cnt) in ctx.timers().items():
                    if cnt:
                        split[name] = split.get(name, 0.0) + tt
        return {"total_ms": _stats(wall), **{name + "_ms": round(tt / args.steps, 4) for name, tt in split.items()}}

    cap = 4 * n
    d_row, d_col, d_val = ctx.buffer(cap * 8), ctx.buffer(cap * 8), ctx.buffer(cap * 4)
    N = index.shape[0]
    last = {}

    def device_join(path):
        def run():
            last["total"], last["stats"] = ctx.cosine_range_dev(index._db.ptr, N, index._db.ptr, N, L, index._inv.ptr, index._inv.ptr, t, cap,
                                                               d_row.ptr, d_col.ptr, d_val.ptr, flags=_ffi.RANGE_UPPER, path=path)
        return run

    rec["self_join"] = {}
    for name, code in (("exact", _ffi.RANGE_PATH_EXACT), ("filtered", _ffi.RANGE_PATH_FILTERED)):
        entry = {"call": timed(lambda: index.similar_pairs(t, path=name)), "device": timed(device_join(code))}
        entry["pairs"], entry["stats"] = last["total"], last["stats"]
        rec["self_join"][name] = entry
    for nq in (1, 1024):
        q = queries[:nq]
        entry = {"rank_k10": timed(lambda: index.rank(q, 10))}
        for name in ("exact", "filtered"):
            entry[name] = timed(lambda: index.range_search(q, t, path=name))
            entry[name]["results"] = int(index.range_search(q, t, path=name)[1].size)
        rec[f"search_{nq}"] = entry
    total = last["total"]
    d_label = ctx.buffer(N * 4)
    comp = {}
    rec["components"] = timed(lambda: comp.update(ctx.pair_components_dev(d_row.ptr, d_col.ptr, total, N, d_label.ptr)))
    rec["components"].update(edges=int(total), **comp)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec, indent=1))
    index.close()
    ctx.close()


if __name__ == "__main__":
    main()
