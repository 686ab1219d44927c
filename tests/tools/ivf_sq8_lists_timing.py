"""Timing of the probed int8 scan by list (csrc/ivf_sq8.hip): IVFInt8Index.rank with scan="queries" and with
scan="lists", and Int8Index.rank, on the same rows in the same process.

    python tests/tools/ivf_sq8_lists_timing.py [--steps 20] [--warmup 3] [--rows 100000] [--length 32768] [--nlist 256]
                                               [--out profiles/ivf_sq8_lists_timing.jsonl]

Workload: that of tests/tools/ivf_sq8_timing.py, made the same way: N = 10^5 code rows of L = 32768 (a block of 8189 seeded Gaussian
rows is encoded once and its codes are repeated on the device: times do not depend on the values, only on the list lengths, which are
recorded), the centroids are nlist = 256 rows of the block, k = 10; nq in {1, 8, 64, 256, 1024} Gaussian queries x nprobe in
{1, 8, 32, 256}.
Per case: wall time of one `rank` call (upload of the queries, their encoding, the probe selection, the scan, the top-k, the download
of the lists: every call ends in a download, which waits for the stream), median / min / max of `steps` calls after `warmup` calls of
the same shape, and the context's event timers per call, for the two scans and the flat index; the plan of the scan by list; and
whether the two scans' lists were byte-equal at that shape.  Counted, not timed: the code bytes each scan reads, candidates x ld for
the scan by query and (probed rows of a query block, each once) x ld for the scan by list.  Every case is printed when it is done; one
JSON line is appended at the end.  One run, one record: nothing here is a pass / fail threshold, and no test reads it."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "python-visual-similarity_amd"))

BLOCK_ROWS, K = 8189, 10
NPROBES, NQS = (1, 8, 32, 256), (1, 8, 64, 256, 1024)


def _stats(samples):
    a = np.sort(np.asarray(samples))
    return {"median": round(float(np.median(a)), 4), "min": round(float(a[0]), 4), "max": round(float(a[-1]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--length", type=int, default=32768)
    ap.add_argument("--nlist", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ivf_sq8_lists_timing.jsonl"))
    args = ap.parse_args()

    import pvsim
    from pvsim import Int8Index, IVFInt8Index
    from pvsim.quantized import padded_length

    ctx = pvsim.Context(0)
    rng = np.random.default_rng(26)
    n, L, nlist = args.rows, args.length, args.nlist
    ld = padded_length(L)
    block_rows = min(BLOCK_ROWS, n)
    block = rng.standard_normal((block_rows, L), dtype=np.float32)
    centroids = np.ascontiguousarray(block[rng.choice(block_rows, nlist, replace=False)])
    queries = {nq: rng.standard_normal((nq, L), dtype=np.float32) for nq in NQS}

    # the flat index: the block's codes and factors, repeated on the device
    small = Int8Index({str(i): block[i] for i in range(block_rows)}, ctx)
    flat = Int8Index.__new__(Int8Index)
    flat._init_empty([str(i) for i in range(n)], L, ctx, n)
    for r0 in range(0, n, block_rows):
        rn = min(block_rows, n - r0)
        ctx.copy_dev(flat._codes.ptr + r0 * ld, small._codes.ptr, rn * ld)
        ctx.copy_dev(flat._inv.ptr + r0 * 4, small._inv.ptr, rn * 4)
    ctx.sync()
    small.close()
    ivf = IVFInt8Index.build(flat, centroids, ctx)
    sizes = ivf.list_sizes
    rec = {"device": ctx.device_name(), "date": time.strftime("%Y-%m-%d"), "N": n, "L": L, "ld": ld, "nlist": nlist, "k": K,
           "steps": args.steps, "warmup": args.warmup,
           "rows": f"{block_rows} seeded Gaussian rows, their codes repeated on the device; the centroids are {nlist} of them",
           "list_sizes": {"min": int(sizes.min()), "median": float(np.median(sizes)), "max": int(sizes.max()), "empty": int((sizes == 0).sum())},
           "cases": {}}

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ctx.sync()
        wall = []
        ctx.timers_enable(True)
        ctx.timers_reset()
        for _ in range(args.steps):
            t0 = time.perf_counter()
            fn()                                        # ends in a download: the stream has drained
            wall.append((time.perf_counter() - t0) * 1e3)
        t = ctx.timers()
        ctx.timers_enable(False)
        return {"wall_ms": _stats(wall), **{name + "_ms": round(ms / args.steps, 4) for name, (ms, cnt) in t.items() if cnt}}

    for nq, q in queries.items():
        flat_case = timed(lambda: flat.rank(q, K))
        for nprobe in (p for p in NPROBES if p <= nlist):
            a = ivf.rank(q, K, nprobe)
            by_query = dict(ivf.last_scan)
            b = ivf.rank(q, K, nprobe, scan="lists")
            by_list = dict(ivf.last_scan)
            case = {"scans_byte_equal": bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))),
                    "queries": timed(lambda: ivf.rank(q, K, nprobe)), "lists": timed(lambda: ivf.rank(q, K, nprobe, scan="lists")),
                    "flat": flat_case if nprobe == NPROBES[0] else timed(lambda: flat.rank(q, K)), "plan_queries": by_query,
                    "plan_lists": by_list}
            # the rows a query block of the scan by list reads: the union of its queries' probed lists, every row once
            probes = _probes(ctx, ivf, q, nprobe, ld)
            qb = by_list["query_block"]
            once = sum(int(sizes[np.unique(probes[q0:q0 + qb])].sum()) for q0 in range(0, nq, qb))
            case["code_bytes_read_counted"] = {"queries": by_query["candidates"] * ld, "lists": once * ld}
            med = {name: case[name]["wall_ms"]["median"] for name in ("queries", "lists", "flat")}
            case["lists_over_queries_wall_time"] = round(med["lists"] / med["queries"], 4)
            case["lists_over_flat_wall_time"] = round(med["lists"] / med["flat"], 4)
            case["queries_over_flat_wall_time"] = round(med["queries"] / med["flat"], 4)
            if nprobe == nlist:                          # every list probed: the flat index's lists, at the sizes timed
                f = flat.rank(q, K)
                case["equals_flat_lists"] = bool(np.array_equal(b[0], f[0]) and np.array_equal(b[1].view(np.uint32), f[1].view(np.uint32)))
            rec["cases"][f"nq{nq}_nprobe{nprobe}"] = case
            print(f"nq{nq}_nprobe{nprobe}", json.dumps(case), flush=True)
    ivf.close()
    flat.close()
    print(json.dumps(rec), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


def _probes(ctx, ivf, q, nprobe, ld):
    """the probes `rank` selects for these queries -> host int64 (nq, nprobe)"""
    nq, L = q.shape
    with ctx.scratch() as tmp:
        d_q, d_qc, d_invq = tmp.upload(q), tmp(nq * ld), tmp(nq * 4)
        d_pidx, d_pval = tmp(nq * nprobe * 8), tmp(nq * nprobe * 4)
        ctx.sq8_encode_dev(d_q.ptr, nq, L, d_qc.ptr, d_invq.ptr)
        ctx.sq8_topk_dev(d_qc.ptr, d_invq.ptr, nq, ivf._cent_codes.ptr, ivf._cent_inv.ptr, ivf.nlist, L, nprobe, 0, False, d_pidx.ptr, d_pval.ptr)
        return d_pidx.download((nq, nprobe), np.int64)


if __name__ == "__main__":
    main()
