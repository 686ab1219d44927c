"""Timing of the compact index (csrc/pq.hip): CompactIndex.rank on synthetic uniform codes, beside the dense DeviceIndex pass.

    python tests/tools/pq_timing.py [--steps 10] [--warmup 2] [--n 1000000] [--m 64] [--out profiles/pq_timing.jsonl]

Workload: N = 10^6 rows of m = 64 uniform random codes (ksub = 256, d = 128, no projection), k = 10, rerank = 0, for nq = 1 and
nq = 1024.  Per case: wall time of one `rank` call (upload of the queries, tables, scan, top-k, download of the lists), median of
`steps`, and its split by the context's event timers: `table` (slot misc: the query norms and pvs_pq_lut_dev), `scan` (slot
cosine_gemm: the scan kernel stands where the GEMM stands in the dense path) and `topk`.  `lookups_per_s` is nq N m over the
scan time; `lds_conflict_free_lookups_per_s` is 32 look-ups per clock per CU x CUs x the clock the device reports (the
published 2400 MHz peak when the runtime reports none; `clock_source` says which).
The same at N = 8189 beside DeviceIndex.rank over 8189 x 32768 float32 rows in the same process (the existing path, as a
yardstick), and the device bytes of both indexes.  Appends one JSON line.  Nothing here is a pass / fail threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "python-visual-similarity_amd"))


def _stats(samples):
    a = np.sort(np.asarray(samples))
    return {"median": round(float(np.median(a)), 4), "min": round(float(a[0]), 4), "max": round(float(a[-1]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pq_timing.jsonl"))
    args = ap.parse_args()

    import pvsim
    from pvsim import CompactIndex, ProductQuantizer
    from pvsim.index import DeviceIndex

    ctx = pvsim.Context(0)
    rng = np.random.default_rng(12)
    m, ksub, dsub, k = args.m, 256, 2, 10
    d = m * dsub
    cb = rng.standard_normal((m, ksub, dsub)).astype(np.float32)
    rec = {"device": ctx.device_name(), "date": time.strftime("%Y-%m-%d"), "m": m, "ksub": ksub, "d": d, "k": k, "rerank": 0,
           "steps": args.steps, "warmup": args.warmup}
    try:
        import torch
        prop = torch.cuda.get_device_properties(0)
        cus, mhz = int(prop.multi_processor_count), float(getattr(prop, "clock_rate", 0)) / 1e3
    except Exception:
        cus, mhz = 0, 0.0
    clock_source = "device properties"
    if mhz <= 0:                                        # this runtime reports no clock: the MI355X's published peak engine clock
        mhz, clock_source = 2400.0, "published peak engine clock (none reported by the runtime)"
    if cus <= 0:
        cus = 256
    rec["compute_units"], rec["clock_mhz"], rec["clock_source"] = cus, mhz, clock_source
    rec["lds_conflict_free_lookups_per_s"] = 32.0 * cus * mhz * 1e6

    def compact(n):
        codes = rng.integers(0, ksub, (n, m), dtype=np.uint8)
        return CompactIndex([str(i) for i in range(n)], codes, np.ones(n, np.float32), ProductQuantizer.from_codebooks(cb, ctx), ctx=ctx)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ctx.sync()
        wall = []
        ctx.timers_enable(True)
        ctx.timers_reset()
        for _ in range(args.steps):
            t0 = time.perf_counter()
            fn()
            wall.append((time.perf_counter() - t0) * 1e3)
        t = ctx.timers()
        ctx.timers_enable(False)
        return _stats(wall), {name: round(ms / args.steps, 4) for name, (ms, cnt) in t.items() if cnt}

    def compact_case(ci, nq):
        q = rng.standard_normal((nq, d)).astype(np.float32)
        wall, split = timed(lambda: ci.rank(q, k))
        scan = split.get("cosine_gemm", 0.0)
        out = {"rank_ms": wall, "table_ms": split.get("misc", 0.0), "scan_ms": scan, "topk_ms": split.get("topk", 0.0)}
        if scan > 0:
            out["lookups_per_s"] = float(nq) * len(ci) * m / (scan * 1e-3)
            if rec["lds_conflict_free_lookups_per_s"]:
                out["share_of_conflict_free_lds"] = round(out["lookups_per_s"] / rec["lds_conflict_free_lookups_per_s"], 4)
        return out

    big = compact(args.n)
    rec["n"] = args.n
    rec["compact_bytes"] = big.nbytes
    for nq in (1, 1024):
        rec[f"compact_nq{nq}"] = compact_case(big, nq)
    big.close()

    n2, L = 8189, 32768
    small = compact(n2)
    rec["n_small"], rec["compact_small_bytes"] = n2, small.nbytes
    for nq in (1, 1024):
        rec[f"compact_small_nq{nq}"] = compact_case(small, nq)
    small.close()
    rows = rng.standard_normal((n2, L), dtype=np.float32)
    dense = DeviceIndex({str(i): rows[i] for i in range(n2)}, ctx)
    rec["dense_small_bytes"] = int(rows.nbytes + n2 * 4)
    for nq in (1, 1024):
        q = rng.standard_normal((nq, L), dtype=np.float32)
        wall, split = timed(lambda: dense.rank(q, k))
        rec[f"dense_small_nq{nq}"] = {"rank_ms": wall, **{name + "_ms": v for name, v in split.items()}}
    dense.close()
    print(json.dumps(rec), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
