"""Timing of the int8 resident index (csrc/sq8.hip): Int8Index.rank beside DeviceIndex.rank on the same rows, in the same run.

    python tests/tools/sq8_timing.py [--steps 10] [--warmup 2] [--sizes 8189,100000] [--out profiles/sq8_timing.jsonl]

Workload: N rows of L = 32768 float32 (N = 8189 and 10^5; the large corpus repeats a block of 8189 seeded Gaussian rows on the
device, so no 13 GB array is drawn on the host: times do not depend on the values), nq = 1 and 1024 Gaussian queries, k = 10.
Per case and index: wall time of one `rank` call (upload of the queries, their encoding, scores, top-k, download of the lists;
every call ends in the download, which waits for the stream), median / min / max of `steps` calls after `warmup` calls, and its
split by the context's event timers (`misc`: norms or the query encoding, `cosine_gemm`: the scores, `topk`, `rescore`).
Derived: `row_path_bytes_per_s` = N ld / score time at nq = 1 (the bytes of codes one pass reads) and `matrix_path_int_ops_per_s`
= 2 nq N ld / score time at nq = 1024 (a multiply and an add per byte pair), and the device bytes of both indexes.  Every case is
printed when it is done; one JSON line is appended at the end.  Nothing here is a pass / fail threshold, and no test reads it."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "python-visual-similarity_amd"))

BLOCK_ROWS, L, K = 8189, 32768, 10


def _stats(samples):
    a = np.sort(np.asarray(samples))
    return {"median": round(float(np.median(a)), 4), "min": round(float(a[0]), 4), "max": round(float(a[-1]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="8189,100000")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sq8_timing.jsonl"))
    args = ap.parse_args()

    import pvsim
    from pvsim import Int8Index
    from pvsim.index import DeviceIndex
    from pvsim.quantized import padded_length

    ctx = pvsim.Context(0)
    rng = np.random.default_rng(22)
    ld = padded_length(L)
    rec = {"device": ctx.device_name(), "date": time.strftime("%Y-%m-%d"), "L": L, "ld": ld, "k": K, "steps": args.steps,
           "warmup": args.warmup, "rows": "8189 seeded Gaussian rows, repeated on the device for the larger corpus", "cases": {}}
    block = rng.standard_normal((BLOCK_ROWS, L), dtype=np.float32)
    queries = {nq: rng.standard_normal((nq, L), dtype=np.float32) for nq in (1, 1024)}

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ctx.sync()
        wall = []
        ctx.timers_enable(True)
        ctx.timers_reset()
        for _ in range(args.steps):
            t0 = time.perf_counter()
            fn()                                        # ends in the download of the lists: the stream has drained
            wall.append((time.perf_counter() - t0) * 1e3)
        t = ctx.timers()
        ctx.timers_enable(False)
        return {"rank_ms": _stats(wall), **{name + "_ms": round(ms / args.steps, 4) for name, (ms, cnt) in t.items() if cnt}}

    for n in (int(s) for s in args.sizes.split(",")):
        d_rows = ctx.buffer(n * L * 4)
        d_block = ctx.buffer(block.nbytes).upload(block)
        for r0 in range(0, n, BLOCK_ROWS):
            ctx.copy_dev(d_rows.ptr + r0 * L * 4, d_block.ptr, min(BLOCK_ROWS, n - r0) * L * 4)
        ctx.sync()
        d_block.free()
        dense = DeviceIndex._from_device([str(i) for i in range(n)], d_rows, n, L, np.dtype(np.float32), ctx)
        int8 = Int8Index.from_index(dense)
        sizes = {"dense_bytes": n * L * 4 + n * 4, "int8_bytes": int8.nbytes}
        for nq, q in queries.items():
            case = dict(sizes)
            case["int8"] = timed(lambda: int8.rank(q, K))
            case["dense"] = timed(lambda: dense.rank(q, K))
            score_ms = case["int8"].get("cosine_gemm_ms", 0.0)
            if score_ms > 0 and nq == 1:
                case["row_path_bytes_per_s"] = n * ld / (score_ms * 1e-3)
            if score_ms > 0 and nq == 1024:
                case["matrix_path_int_ops_per_s"] = 2.0 * nq * n * ld / (score_ms * 1e-3)
            case["int8_over_dense_rank_time"] = round(case["int8"]["rank_ms"]["median"] / case["dense"]["rank_ms"]["median"], 4)
            rec["cases"][f"n{n}_nq{nq}"] = case
            print(f"n{n}_nq{nq}", json.dumps(case), flush=True)
        int8.close()
        dense.close()
    print(json.dumps(rec), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
