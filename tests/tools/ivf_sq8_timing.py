"""Timing of the inverted lists over the int8 code rows (csrc/ivf_sq8.hip): IVFInt8Index.rank beside Int8Index.rank on the same rows,
in the same process.

    python tests/tools/ivf_sq8_timing.py [--steps 20] [--warmup 3] [--rows 100000] [--length 32768] [--nlist 256]
                                         [--out profiles/ivf_sq8_timing.jsonl]

Workload: N = 10^5 code rows of L = 32768 (a block of 8189 seeded Gaussian rows is encoded once and its codes are repeated on the
device, so no 13 GB array is drawn anywhere: times do not depend on the values, only on the list lengths, which are recorded), the
centroids are nlist = 256 rows of the block, nprobe in {1, 8, 32, 256}, nq in {1, 64} Gaussian queries, k = 10.
Per case: wall time of one `rank` call (upload of the queries, their encoding, the probe selection, the scan, the top-k, the download
of the lists: every call ends in a download, which waits for the stream), median / min / max of `steps` calls after `warmup` calls of
the same shape, and the context's event timers per call.  The probe selection (pvs_sq8_encode_dev of the queries + pvs_sq8_topk_dev
against the centroid codes) is timed on its own in the same way; it shares the scoring and top-k slots with the scan, so the scan's
and the candidate top-k's event times are the call's minus the probe selection's, and are named `_by_difference`.  `Int8Index.rank`
runs on the same rows beside every case.  Counted, not timed: the rows a query scans (mean over the queries) and the bytes the scan
reads, candidates * ld + nlist * ld for the probes.  Derived: scan bytes per second over the scan's event time.  Every case is
printed when it is done; one JSON line is appended at the end.  One run, one record: nothing here is a pass / fail threshold, and
no test reads it."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "python-visual-similarity_amd"))

BLOCK_ROWS, K = 8189, 10
NPROBES, NQS = (1, 8, 32, 256), (1, 64)


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ivf_sq8_timing.jsonl"))
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
    t0 = time.perf_counter()
    ivf = IVFInt8Index.build(flat, centroids, ctx)
    build_s = time.perf_counter() - t0
    sizes = ivf.list_sizes
    rec = {"device": ctx.device_name(), "date": time.strftime("%Y-%m-%d"), "N": n, "L": L, "ld": ld, "nlist": nlist, "k": K,
           "steps": args.steps, "warmup": args.warmup,
           "rows": f"{block_rows} seeded Gaussian rows, their codes repeated on the device; the centroids are {nlist} of them",
           "list_sizes": {"min": int(sizes.min()), "median": float(np.median(sizes)), "max": int(sizes.max()), "empty": int((sizes == 0).sum())},
           "build_from_int8_index_s": round(build_s, 3), "flat_bytes": flat.nbytes, "ivf_bytes": ivf.nbytes, "cases": {}}

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

    def probe_selection(q, nprobe):
        """what rank does before the scan, and the download that ends it"""
        nq = q.shape[0]
        with ctx.scratch() as tmp:
            d_q, d_qc, d_invq = tmp.upload(q), tmp(nq * ld), tmp(nq * 4)
            d_pidx, d_pval = tmp(nq * nprobe * 8), tmp(nq * nprobe * 4)
            ctx.sq8_encode_dev(d_q.ptr, nq, L, d_qc.ptr, d_invq.ptr)
            ctx.sq8_topk_dev(d_qc.ptr, d_invq.ptr, nq, ivf._cent_codes.ptr, ivf._cent_inv.ptr, nlist, L, nprobe, 0, False, d_pidx.ptr,
                             d_pval.ptr)
            return d_pidx.download((nq, nprobe), np.int64)

    for nq, q in queries.items():
        flat_case = timed(lambda: flat.rank(q, K))
        for nprobe in (p for p in NPROBES if p <= nlist):
            case = {"ivf": timed(lambda: ivf.rank(q, K, nprobe)), "probe_selection": timed(lambda: probe_selection(q, nprobe)),
                    "flat": flat_case if nprobe == NPROBES[0] else timed(lambda: flat.rank(q, K))}
            scan = dict(ivf.last_scan)
            scanned = scan["candidates"] / nq
            case["scan_plan"] = scan
            case["rows_scanned_per_query"] = round(scanned, 1)
            case["fraction_of_rows_scanned"] = round(scanned / n, 5)
            case["scan_bytes_per_query_counted"] = int(scanned * ld + nlist * ld)
            for slot in ("cosine_gemm", "topk"):
                case[f"scan_{slot}_ms_by_difference"] = round(case["ivf"].get(slot + "_ms", 0.0) - case["probe_selection"].get(slot + "_ms", 0.0), 4)
            if case["scan_cosine_gemm_ms_by_difference"] > 0:
                case["scan_bytes_per_s"] = scan["candidates"] * ld / (case["scan_cosine_gemm_ms_by_difference"] * 1e-3)
            case["ivf_over_flat_wall_time"] = round(case["ivf"]["wall_ms"]["median"] / case["flat"]["wall_ms"]["median"], 4)
            if nprobe == nlist:                          # every list probed: the flat index's lists, at the sizes timed
                a, b = ivf.rank(q, K, nprobe), flat.rank(q, K)
                case["equals_flat_lists"] = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))
            rec["cases"][f"nq{nq}_nprobe{nprobe}"] = case
            print(f"nq{nq}_nprobe{nprobe}", json.dumps(case), flush=True)
    ivf.close()
    flat.close()
    print(json.dumps(rec), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
