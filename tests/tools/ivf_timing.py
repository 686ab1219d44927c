"""Timing of the inverted lists of the compact index (csrc/ivf.hip): IVFCompactIndex.rank beside CompactIndex.rank in the same run.

    python tests/tools/ivf_timing.py [--steps 10] [--warmup 2] [--n 1000000] [--m 64] [--nlist 1024] [--out profiles/ivf_timing.jsonl]

Workload: N = 10^6 rows of m = 64 uniform random codes (ksub = 256, d = 128, no projection), k = 10, rerank = 0.  The list sizes
are real: coarse centroids from learn.fit_kmeans on 10^5 of N random rows, every row assigned by pvs_ivf_assign_dev.  One JSON line
per case (nprobe in {1, 8, 32, nlist}) x (nq in {1, 1024}): wall time of one `rank` call (median of `steps` after `warmup`), and
the stages timed one by one with the context's event timers: `coarse` (pvs_ivf_coarse_dev), `table` (query norms and
pvs_pq_lut_dev), `probe_select` (pvs_topk_dev on the coarse panel), `scan` and `select` (the two slots of
pvs_ivf_scan_topk_dev).  Also: rows scanned per query (mean over the queries), look-ups per second over the scan time, the
candidate-row width W, the longest and mean list length, and `flat_rank_ms`: CompactIndex.rank on the same N, m and queries,
timed in the same process.  Nothing here is a pass / fail threshold."""
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
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ivf_timing.jsonl"))
    args = ap.parse_args()

    import pvsim
    from pvsim import CompactIndex, IVFCompactIndex, ProductQuantizer
    from pvsim.compact import _fit_coarse, _sort_into_lists

    ctx = pvsim.Context(0)
    rng = np.random.default_rng(14)
    n, m, ksub, dsub, k, nlist = args.n, args.m, 256, 2, 10, args.nlist
    d = m * dsub
    cb = rng.standard_normal((m, ksub, dsub)).astype(np.float32)
    base = {"device": ctx.device_name(), "date": time.strftime("%Y-%m-%d"), "n": n, "m": m, "ksub": ksub, "d": d, "k": k, "rerank": 0,
            "nlist": nlist, "steps": args.steps, "warmup": args.warmup}

    # real list sizes: k-means on a sample, every row assigned on the device
    rows = rng.standard_normal((n, d), dtype=np.float32)
    cent = _fit_coarse(ctx, rows[:: max(1, n // 100000)], nlist, np.random.RandomState(15), 10)
    lists = np.empty(n, np.int32)
    d_c = ctx.buffer(cent.nbytes).upload(cent)
    for r0 in range(0, n, 1 << 17):
        rn = min(1 << 17, n - r0)
        d_x, d_l = ctx.buffer(rn * d * 4).upload(rows[r0:r0 + rn]), ctx.buffer(rn * 4)
        ctx.ivf_assign_dev(d_x.ptr, rn, d, d_c.ptr, nlist, d_l.ptr, None)
        lists[r0:r0 + rn] = d_l.download((rn,), np.int32)
        d_x.free(), d_l.free()
    d_c.free()
    del rows
    ids, list_off = _sort_into_lists(lists, nlist)
    sizes = np.diff(list_off)
    base.update(longest_list=int(sizes.max()), mean_list=round(float(sizes.mean()), 2), empty_lists=int((sizes == 0).sum()))
    codes = rng.integers(0, ksub, (n, m), dtype=np.uint8)
    paths = [str(i) for i in range(n)]
    ivf = IVFCompactIndex(paths, codes, np.ones(n, np.float32), ProductQuantizer.from_codebooks(cb, ctx), cent, list_off, ids, ctx=ctx)
    flat = CompactIndex(paths, codes, np.ones(n, np.float32), ProductQuantizer.from_codebooks(cb, ctx), ctx=ctx)
    base["ivf_bytes"], base["flat_bytes"] = ivf.nbytes, flat.nbytes

    def wall(fn):
        for _ in range(args.warmup):
            fn()
        ctx.sync()
        out = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t0) * 1e3)
        return _stats(out)

    def stage(fn, *slots):
        """event time of one stage per call, per timer slot: the stage alone between a reset and a read of the timers"""
        ctx.sync()
        ctx.timers_enable(True)
        ctx.timers_reset()
        for _ in range(args.steps):
            fn()
        ctx.sync()
        t = ctx.timers()
        ctx.timers_enable(False)
        out = [round(t[slot][0] / args.steps, 4) for slot in slots]
        return out[0] if len(out) == 1 else out

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    dev, table = ivf._device(), ivf.quantizer.table()
    for nq in (1, 1024):
        q = rng.standard_normal((nq, d)).astype(np.float32)
        flat_ms = wall(lambda: flat.rank(q, k))
        d_q, d_iq, d_lut = ctx.buffer(q.nbytes).upload(q), ctx.buffer(nq * 4), ctx.buffer(nq * m * ksub * 4)
        d_co = ctx.buffer(nq * nlist * 4)
        d_idx, d_val = ctx.buffer(nq * k * 8), ctx.buffer(nq * k * 4)

        def tables():
            ctx.row_inv_norms_dev(d_q.ptr, nq, d, d_iq.ptr)
            ctx.pq_lut_dev(table, d_q.ptr, nq, d_lut.ptr)

        table_ms = stage(tables, "misc")
        coarse_ms = stage(lambda: ctx.ivf_coarse_dev(d_q.ptr, nq, d, dev["cent"].ptr, nlist, d_co.ptr), "misc")
        for nprobe in sorted({1, 8, 32, min(nlist, 1024)}):
            if nprobe > nlist:
                continue
            d_pi, d_pv = ctx.buffer(nq * nprobe * 8), ctx.buffer(nq * nprobe * 4)
            probe_ms = stage(lambda: ctx.topk_dev(d_co.ptr, nq, nlist, nlist, nprobe, 0, False, d_pi.ptr, d_pv.ptr), "topk")

            def scan():
                ctx.ivf_scan_topk_dev(d_lut.ptr, nq, m, ksub, d_pi.ptr, d_pv.ptr, nprobe, dev["list_off"].ptr, list_off, nlist,
                                      dev["codes"].ptr, dev["ids"].ptr, d_iq.ptr, dev["inv"].ptr, k, d_idx.ptr, d_val.ptr)

            scan()                                                # the workspace grows here, not inside the timed calls
            scan_ms, select_ms = stage(scan, "cosine_gemm", "topk")
            probed = d_pi.download((nq, nprobe), np.int64)
            scanned = float(sizes[probed].sum(1).mean())
            width = -(-int(np.sort(sizes)[::-1][:nprobe].sum()) // 64) * 64
            rec = dict(base, nq=nq, nprobe=nprobe, rank_ms=wall(lambda: ivf.rank(q, k, nprobe)), flat_rank_ms=flat_ms,
                       coarse_ms=coarse_ms, table_ms=table_ms, probe_select_ms=probe_ms, scan_ms=scan_ms, select_ms=select_ms,
                       rows_scanned_per_query=round(scanned, 1), scanned_share=round(scanned / n, 5), candidate_row_width=max(64, width))
            if scan_ms > 0:
                rec["lookups_per_s"] = nq * scanned * m / (scan_ms * 1e-3)
            print(json.dumps(rec), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")
            d_pi.free(), d_pv.free()
        for b in (d_q, d_iq, d_lut, d_co, d_idx, d_val):
            b.free()
    ivf.close(), flat.close()
    ctx.close()


if __name__ == "__main__":
    main()
