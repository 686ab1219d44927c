"""Timing of diffusion re-ranking (csrc/diffuse.hip, pvsim/diffusion.py) at the headline corpus.

    python tests/tools/diffusion_timing.py [--steps 5] [--warmup 1] [--n 8189] [--dim 32768] [--k 50] [--out profiles/diffusion_timing.jsonl]

Corpus: n float32 rows of `dim` columns, planted in classes of 32 so that neighbour lists overlap the way real ones do.
  build     Diffusion.build(index, k): wall time of the whole call and its split by the event timers (cosine_gemm + topk = the
            ranking of every row against the index; misc = the four graph kernels and the norms of the blocks).
  rank      g.rank for nq = 1 and nq = 1024 (k = 10, kq = 10, alpha = 0.99, tol = 1e-6, maxiter = 20) beside index.rank and
            index.rank_expanded (QueryExpansion(n = 10)) in the same run, with the solver's steps per query.
  step      one conjugate-gradient step of pvs_diffuse_cg_dev for a tile of 1 and of 64 columns: tol = 0 keeps every column
            stepping and check_every > maxiter keeps the host out, so (time at 24 steps - time at 4 steps) / 20 is one step: the
            product kernel, the update kernel, the direction kernel and the two one-workgroup reductions.  `product_bytes` is what the
            product kernel moves by the algorithm, N kg (4 + 8 + 8 tile) + 3 N tile 8; `product_share_of_copy_rate` divides it by the
            WHOLE step's time and by the 6.29 TB/s a float4 copy reaches (MI355X_MICROARCH.md), so it is a lower bound of the
            product kernel's own share.  Gathers of overlapping lists are served partly from cache: an algorithmic rate.
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
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "diffusion_timing.jsonl"))
    args = ap.parse_args()

    import pvsim
    from pvsim import Diffusion, QueryExpansion
    from pvsim.engine import diffuse_workspace
    from pvsim.index import DeviceIndex

    ctx = pvsim.Context(0)
    rng = np.random.default_rng(13)
    n, L, kg = args.n, args.dim, args.k
    classes = max(1, n // 32)
    centres = rng.standard_normal((classes, L), dtype=np.float32)
    rows = centres[rng.integers(0, classes, n)]
    rows += rng.standard_normal((n, L), dtype=np.float32)
    del centres
    rec = {"device": ctx.device_name(), "date": time.strftime("%Y-%m-%d"), "n": n, "dim": L, "kg": kg, "gamma": 3, "dtype": "float32",
           "steps": args.steps, "warmup": args.warmup}
    index = DeviceIndex({str(i): rows[i] for i in range(n)}, ctx)

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

    # ---- the build, whole call
    made = []

    def build():
        for g in made:
            g.close()
        made[:] = [Diffusion.build(index, k=kg, gamma=3)]
    wall, split = timed(build, steps=max(2, args.steps // 2))
    rec["build"] = {"total_ms": wall, **split}
    g = made[0]
    s = g.s
    rec["graph"] = {"bytes": n * kg * 12, "nonzero_share": round(float((s != 0).mean()), 4), "isolated_rows": int((~(s != 0).any(axis=1)).sum())}

    # ---- ranking beside the plain and the expanded ranking
    qe = QueryExpansion(n=10)
    for nq in (1, 1024):
        q = rows[rng.integers(0, n, nq)] + rng.standard_normal((nq, L), dtype=np.float32)
        plain_wall, plain_split = timed(lambda: index.rank(q, 10))
        exp_wall, exp_split = timed(lambda: index.rank_expanded(q, 10, qe))
        dif_wall, dif_split = timed(lambda: g.rank(q, k=10, kq=10, alpha=0.99, tol=1e-6, maxiter=20))
        rec[f"rank_nq{nq}"] = {"rank_ms": plain_wall, "rank_expanded_ms": exp_wall, "diffusion_rank_ms": dif_wall, "rank_split": plain_split,
                               "rank_expanded_split": exp_split, "diffusion_rank_split": dif_split,
                               "cg_steps": _stats(g.last_solve["steps"]), "converged": int(g.last_solve["converged"].sum())}
    del rows

    # ---- one solver step
    for tile in (1, 64):
        Y = np.zeros((n, tile))
        for c in range(tile):
            Y[rng.choice(n, 10, replace=False), c] = rng.random(10)
        nbytes = diffuse_workspace(n, tile)
        d_y, d_x, d_work, d_cols = ctx.buffer(Y.nbytes).upload(Y), ctx.buffer(Y.nbytes), ctx.buffer(nbytes), ctx.buffer(24 * tile)

        def solve(maxiter):
            ctx.diffuse_cg_dev(g._d_nbr.ptr, g._d_s.ptr, n, kg, d_y.ptr, tile, 0.99, 0.0, maxiter, maxiter + 1, 0, d_work.ptr, nbytes,
                               d_x.ptr, d_cols.ptr, d_cols.ptr + 8 * tile, d_cols.ptr + 16 * tile)
        short, _ = timed(lambda: solve(4), steps=max(args.steps, 10), warmup=2)
        long_, _ = timed(lambda: solve(24), steps=max(args.steps, 10), warmup=2)
        step_ms = (long_["median"] - short["median"]) / 20
        product_bytes = n * kg * (4 + 8 + 8 * tile) + 3 * n * tile * 8
        rec[f"step_tile{tile}"] = {"width": 1 if tile == 1 else 64, "wall_4_steps_ms": short, "wall_24_steps_ms": long_,
                                   "step_ms": round(step_ms, 5), "product_bytes": product_bytes,
                                   "product_share_of_copy_rate": round(product_bytes / (step_ms * 1e-3) / COPY_RATE, 5) if step_ms > 0 else None}
        for b in (d_y, d_x, d_work, d_cols):
            b.free()
    g.close()
    index.close()
    print(json.dumps(rec), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
