"""Timing of graph maintenance after add / remove (pvsim/diffusion.py) at the headline corpus, beside the rebuild.

    python tests/tools/diffusion_update_timing.py [--steps 5] [--warmup 1] [--n 8189] [--dim 32768] [--k 50] [--out profiles/diffusion_update_timing.jsonl]

Corpus: as tests/tools/diffusion_timing.py (n float32 rows of `dim` columns, planted in classes of 32).  All in one process:
  build     Diffusion.build(index, k, mutable=True): the yardstick.  Its ranking is the one of the immutable build.
  add_b     g.add of b = 1, 64, 1024 new rows (drawn from the same classes).  Between two timed rounds the rows are removed again
            through the graph, untimed, so every round starts from n rows.
  remove_r  g.remove of r = 1, 64, 1024 random rows, with last_update["reranked"] of every round beside the times.  Between two
            rounds the same rows are added again, untimed; they come back at the end of the index.
Every time is the wall time of the whole Python call, ended by a synchronise, median of `steps` rounds after `warmup`; the split by
the context's event timers of the same rounds stands beside it (cosine_gemm + topk + rescore = ranking, misc = everything else on the
device).  The wall time includes the host's share of index.add / index.remove (the upload of the new rows, the path ledger).
Once, outside the timed rounds, the maintained nbr, sim and s are compared with those of a rebuild: `equal_to_rebuild`.
Appends one JSON line.  Nothing here is a pass / fail threshold."""
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
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "diffusion_update_timing.jsonl"))
    args = ap.parse_args()

    import pvsim
    from pvsim import Diffusion
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
    rec = {"device": ctx.device_name(), "date": time.strftime("%Y-%m-%d"), "n": n, "dim": L, "kg": kg, "gamma": 3, "dtype": "float32",
           "steps": args.steps, "warmup": args.warmup}
    store = {str(i): rows[i] for i in range(n)}          # the tool's own host rows by path: what a removed row is added back from
    index = DeviceIndex(store, ctx)
    ctx.timers_enable(True)

    def timed(fn, prepare=None, undo=None, note=None):
        """fn timed `steps` times after `warmup`; prepare before and undo after every call of fn, both untimed; note() -> a number
        kept per timed round"""
        wall, split, notes = [], {}, []
        for it in range(args.warmup + args.steps):
            if prepare:
                prepare()
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
                if note:
                    notes.append(note())
            if undo:
                undo()
        out = {"total_ms": _stats(wall), **{name + "_ms": round(t / args.steps, 4) for name, t in split.items()}}
        if note:
            out["reranked"] = notes
        return out

    made = []

    def build():
        for g in made:
            g.close()
        made[:] = [Diffusion.build(index, k=kg, gamma=3, mutable=True)]
    rec["build"] = timed(build)
    g = made[0]
    rec["graph_bytes"] = n * kg * 16

    serial = [0]
    for b in (1, 64, 1024):
        new = draw(b)
        batch = {}

        def name_batch():
            batch.clear()
            batch.update({f"new{serial[0]}_{i}": new[i] for i in range(b)})
            serial[0] += 1
        rec[f"add_{b}"] = timed(lambda: g.add(batch), prepare=name_batch, undo=lambda: g.remove(list(batch)))
        assert g.n == n

    for r in (1, 64, 1024):
        gone = {}

        def pick():
            paths = list(index.keys())
            gone.clear()
            gone.update({paths[i]: store[paths[i]] for i in rng.choice(len(paths), r, replace=False)})
        rec[f"remove_{r}"] = timed(lambda: g.remove(list(gone)), prepare=pick, undo=lambda: g.add(gone),
                                   note=lambda: g.last_update["reranked"])
        assert g.n == n

    # ---- once, untimed: the maintained arrays are the rebuilt ones
    del store
    g.add({f"check{i}": v for i, v in enumerate(draw(3))})
    g.remove([list(index.keys())[i] for i in (0, n // 2, n + 1)])
    want = Diffusion.build(index, k=kg, gamma=3, mutable=True)
    rec["equal_to_rebuild"] = bool(np.array_equal(g.nbr, want.nbr) and np.array_equal(g.sim.view(np.uint32), want.sim.view(np.uint32))
                                   and np.array_equal(g.s.view(np.uint64), want.s.view(np.uint64)))
    want.close()
    g.close()
    index.close()
    print(json.dumps(rec), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
