"""Timing of k-reciprocal re-ranking (csrc/reciprocal.hip, pvsim/reciprocal.py) at the headline corpus.

    python tests/tools/reciprocal_timing.py [--steps 5] [--warmup 1] [--n 8189] [--dim 32768] [--k 40] [--out profiles/reciprocal_timing.jsonl]

Corpus: as tests/tools/diffusion_timing.py (n float32 rows of `dim` columns, planted in classes of 32).  All in one process:
  build        KReciprocal.build(index, k, k1=20, k2=6, gamma=3), split by the context's event timers into the ranking (cosine_gemm +
               topk + rescore) and everything else on the device (misc: the list kernel and the four set kernels).
  from_graph   KReciprocal.from_graph(g) of a mutable Diffusion graph of the same index and k: two copies and the set kernels.
  rank_1, rank_1024   r.rank(queries, k=10, kq=80, lam=0.3) for 1 and 1024 queries, beside index.rank(queries, 10) and
               Diffusion.rank(queries, k=10, kq=10) of the same queries.
Every time is the wall time of the whole Python call, ended by a synchronise, median of `steps` rounds after `warmup`.  Appends one
JSON line.  Nothing here is a pass / fail threshold."""
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
    ap.add_argument("--k", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "reciprocal_timing.jsonl"))
    args = ap.parse_args()

    import pvsim
    from pvsim import Diffusion, KReciprocal
    from pvsim.index import DeviceIndex

    ctx = pvsim.Context(0)
    rng = np.random.default_rng(13)
    n, L, kg = args.n, args.dim, args.k
    classes = max(1, n // 32)
    centres = rng.standard_normal((classes, L), dtype=np.float32)

    def draw(m):
        rows = centres[rng.integers(0, classes, m)]
        rows += rng.standard_normal((m, L), dtype=np.float32)
        return rows

    rows = draw(n)
    rec = {"device": ctx.device_name(), "date": time.strftime("%Y-%m-%d"), "n": n, "dim": L, "kg": kg, "k1": 20, "k2": 6, "gamma": 3,
           "kq": 80, "lam": 0.3, "dtype": "float32", "steps": args.steps, "warmup": args.warmup}
    index = DeviceIndex({str(i): rows[i] for i in range(n)}, ctx)
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
                for name, (t, cnt) in ctx.timers().items():
                    if cnt:
                        split[name] = split.get(name, 0.0) + t
        return {"total_ms": _stats(wall), **{name + "_ms": round(t / args.steps, 4) for name, t in split.items()}}

    made = []

    def keep(make):
        def run():
            for r in made:
                r.close()
            made[:] = [make()]
        return run

    rec["build"] = timed(keep(lambda: KReciprocal.build(index, k=kg, k1=20, k2=6, gamma=3)))
    r = made.pop()
    rec["dropped_fraction"] = round(r.last_build["dropped_fraction"], 4)
    rec["resident_bytes"] = n * (kg * (4 + 4 + 1 + 8 + 8) + 8 * 4)          # nbr, sim, members, v, w; maskh, v0, w0, ws
    g = Diffusion.build(index, k=kg, gamma=3, mutable=True)
    rec["from_graph"] = timed(keep(lambda: KReciprocal.from_graph(g, k1=20, k2=6, gamma=3)))
    r2 = made.pop()
    rec["from_graph_equals_build"] = bool(all(np.array_equal(getattr(r, a).view(np.uint8), getattr(r2, a).view(np.uint8))
                                              for a in ("nbr", "sim", "members", "w", "w0", "ws")))
    r2.close()
    for nq in (1, 1024):
        Q = draw(nq)
        rec[f"rank_{nq}"] = {"index_rank": timed(lambda: index.rank(Q, 10)),
                             "reciprocal_rank": timed(lambda: r.rank(Q, k=10, kq=80, lam=0.3)),
                             "diffusion_rank": timed(lambda: g.rank(Q, k=10, kq=10))}
        rec[f"rank_{nq}"]["dropped_per_query"] = round(float(r.last_rank["dropped"].mean()), 3)
    r.close()
    g.close()
    index.close()
    print(json.dumps(rec), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
