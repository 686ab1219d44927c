"""Timing of the int8 threshold join (csrc/sq8_range.hip, pvsim/quantized.py) at the headline corpus, beside the
float32 join of section 24 on the same rows.

    python tests/tools/sq8_range_timing.py [--steps 5] [--warmup 1] [--n 8189] [--dim 32768] [--pairs 4000] [--out profiles/sq8_range_timing.jsonl]

Corpus: that of tests/tools/range_timing.py: n float32 rows of `dim` columns, random directions, with `pairs` planted near duplicates
whose cosine is drawn from [0.80, 1.00]; the threshold is 0.9.  The Int8Index is made from the resident float32 rows.  All in one process:
  self_join               pvs_sq8_range_dev with PVS_RANGE_UPPER on the stored codes for "panel" and "mask" (the device call alone, into
                          preallocated buffers, split by the context's event timers) and Int8Index.similar_pairs (the whole Python call);
                          DeviceIndex.similar_pairs(path="filtered") and its device call beside them.
  search_1024, search_1   the same for 1024 queries and for 1 query: the device call on query codes made beforehand, Int8Index.range_search
                          (quantises the queries, joins, downloads, sorts) and DeviceIndex.range_search(path="filtered").
Every time is wall time ended by a synchronise: median, min and max of `steps` calls after `warmup`.  Appends one JSON line.  Nothing
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sq8_range_timing.jsonl"))
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
           "threshold": float(np.float32(t)), "steps": args.steps, "warmup": args.warmup,
           "method": "wall time ended by a synchronise; median [min, max] of `steps` calls after `warmup`, all in one process"}
    f32 = DeviceIndex({str(i): rows[i] for i in range(n)}, ctx)
    i8 = pvsim.Int8Index.from_index(f32)
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
    d_q = ctx.buffer(queries.nbytes).upload(queries)
    d_qc, d_iq, d_nq = ctx.buffer(1024 * i8._ld), ctx.buffer(1024 * 4), ctx.buffer(1024 * 4)
    ctx.sq8_encode_dev(d_q.ptr, 1024, L, d_qc.ptr, d_iq.ptr)
    f32._row_inv_norms(d_q.ptr, 1024, d_nq.ptr)
    ctx.sync()
    last = {}

    def sq8_device(nq, path, upper):
        qc, iq = (i8._codes.ptr, i8._inv.ptr) if upper else (d_qc.ptr, d_iq.ptr)

        def run():
            last["total"], last["stats"] = ctx.sq8_range_dev(qc, iq, nq, i8._codes.ptr, i8._inv.ptr, n, L, t, cap, d_row.ptr, d_col.ptr,
                                                             d_val.ptr, flags=_ffi.RANGE_UPPER if upper else 0, path=path)
        return run

    def f32_device(nq, upper):
        q, iq = (f32._db.ptr, f32._inv.ptr) if upper else (d_q.ptr, d_nq.ptr)

        def run():
            last["total"], last["stats"] = ctx.cosine_range_dev(q, nq, f32._db.ptr, n, L, iq, f32._inv.ptr, t, cap, d_row.ptr, d_col.ptr,
                                                                d_val.ptr, flags=_ffi.RANGE_UPPER if upper else 0,
                                                                path=_ffi.RANGE_PATH_FILTERED)
        return run

    for key, nq, upper in (("self_join", n, True), ("search_1024", 1024, False), ("search_1", 1, False)):
        q = queries[:nq]
        entry = {}
        for name, code in (("panel", _ffi.SQ8_RANGE_PATH_PANEL), ("mask", _ffi.SQ8_RANGE_PATH_MASK)):
            e = {"device": timed(sq8_device(nq, code, upper))}
            e["pairs"], e["stats"] = last["total"], last["stats"]
            e["call"] = timed((lambda: i8.similar_pairs(t, path=name)) if upper else (lambda: i8.range_search(q, t, path=name)))
            entry["int8_" + name] = e
        e = {"device": timed(f32_device(nq, upper))}
        e["pairs"], e["stats"] = last["total"], last["stats"]
        e["call"] = timed((lambda: f32.similar_pairs(t, path="filtered")) if upper else (lambda: f32.range_search(q, t, path="filtered")))
        entry["float32_filtered"] = e
        entry["int8_auto_takes"] = (i8.similar_pairs(t) if upper else i8.range_search(q, t)) and i8.last_range_stats["path"]
        rec[key] = entry
    rec["unmeasured"] = "no kernel profiled (no counters, no trace); nothing at 10^6 rows; one corpus, one threshold"
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec, indent=1))
    i8.close()
    f32.close()
    ctx.close()


if __name__ == "__main__":
    main()
