"""Timing of index maintenance (csrc/update.hip): add and remove beside a plain device-to-device copy of the same
arrays (the control) and beside the from-scratch construction the update replaces (the alternative), all in one run.

    python tests/tools/update_timing.py [--steps 5] [--warmup 1] [--n 1000000] [--m 64] [--nlist 1024] [--dense-rows 8189]
                                        [--dense-cols 32768] [--out profiles/update_timing.jsonl]

Compact workload: N = 10^6 rows of m = 64 random codes (ksub = 256, d = 128, no projection, rows not kept), list numbers from
pvs_ivf_assign_dev against nlist = 1024 random centroids; a flat CompactIndex and an IVFCompactIndex over the same rows, built by
the array constructors.  Dense workload: a DeviceIndex of 8189 x 32768 float32 rows.  One JSON line per case:
  level "entry"  the movement alone: pvs_ivf_insert_dev, pvs_ivf_remove_dev (with its mask and positions), pvs_compact_rows_dev out
                 of place and in place, on prepared device arrays;
  level "class"  the public add / remove of the index classes, which also encode the new rows and keep the Python bookkeeping;
with `ms` the wall time of one call ending in a stream synchronise (median of `steps` after `warmup`), `copy_ms` pvs_copy_dev of all the
arrays' bytes timed the same way, `ratio` = ms / copy_ms, `moved_bytes` the row bytes the call reads (an in-place compaction moves the
rows behind the first removed one only), and for the class level `rebuild_ms`: the construction from the host that the update
replaces (IVF: download, argsort into lists, upload, as IVFCompactIndex.fit does it; flat and dense: the upload by the constructor).
An add is undone by an untimed remove of the same rows, a remove by an untimed add (which appends: every timed remove therefore names
the rows that stand at the same scattered POSITIONS at that moment).  The class level at N = 10^6 includes what Python costs on the
path list (one slice per run of kept paths).  Nothing here is a pass / fail threshold."""
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


def _timed(ctx, fn, steps, warmup, undo=None, prepare=None):
    """wall milliseconds of fn() + synchronise, `steps` samples after `warmup`; `prepare` runs untimed before every call and its
    result is passed to fn and undo; `undo` runs untimed after every call"""
    out = []
    for i in range(warmup + steps):
        args = () if prepare is None else (prepare(),)
        ctx.sync()
        t0 = time.perf_counter()
        fn(*args)
        ctx.sync()
        dt = (time.perf_counter() - t0) * 1e3
        if undo is not None:
            undo(*args)
        if i >= warmup:
            out.append(dt)
    return _stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--dense-rows", type=int, default=8189)
    ap.add_argument("--dense-cols", type=int, default=32768)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "update_timing.jsonl"))
    args = ap.parse_args()

    import pvsim
    from pvsim import CompactIndex, IVFCompactIndex, ProductQuantizer
    from pvsim.compact import _sort_into_lists
    from pvsim.index import DeviceIndex, _keep_positions

    ctx = pvsim.Context(0)
    rng = np.random.default_rng(15)
    n, m, ksub, dsub, nlist = args.n, args.m, 256, 2, args.nlist
    d = m * dsub
    base = {"device": ctx.device_name(), "date": time.strftime("%Y-%m-%d"), "steps": args.steps, "warmup": args.warmup}
    lines = []

    def emit(rec):
        rec = {**base, **rec}
        if "copy_ms" in rec:
            rec["ratio"] = round(rec["ms"]["median"] / rec["copy_ms"]["median"], 3)
        if "rebuild_ms" in rec:
            rec["rebuild_over_update"] = round(rec["rebuild_ms"]["median"] / rec["ms"]["median"], 2)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def copy_ms(nbytes):
        a, b = ctx.buffer(nbytes), ctx.buffer(nbytes)
        a.fill_bytes(1)
        out = _timed(ctx, lambda: ctx.copy_dev(b.ptr, a.ptr, nbytes), args.steps, args.warmup)
        a.free(), b.free()
        return out

    # ------------------------------------------------------------------ compact indexes
    cb = rng.standard_normal((m, ksub, dsub)).astype(np.float32)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    extra = 65536
    rows = rng.standard_normal((n + extra, d), dtype=np.float32)
    pq = ProductQuantizer.from_codebooks(cb, ctx)
    codes, inv, lists = np.empty((n + extra, m), np.uint8), np.empty(n + extra, np.float32), np.empty(n + extra, np.int32)
    d_c = ctx.buffer(cent.nbytes).upload(cent)
    for r0 in range(0, n + extra, 1 << 17):
        rn = min(1 << 17, n + extra - r0)
        d_x, d_l, d_i, d_r, d_k = (ctx.buffer(rn * d * 4).upload(rows[r0:r0 + rn]), ctx.buffer(rn * 4), ctx.buffer(rn * 4),
                                   ctx.buffer(rn * d * 4), ctx.buffer(rn * m))
        ctx.row_inv_norms_dev(d_x.ptr, rn, d, d_i.ptr)
        ctx.ivf_assign_dev(d_x.ptr, rn, d, d_c.ptr, nlist, d_l.ptr, d_r.ptr)
        ctx.pq_encode_dev(pq.table(), d_r.ptr, rn, d_k.ptr)
        lists[r0:r0 + rn], inv[r0:r0 + rn] = d_l.download((rn,), np.int32), d_i.download((rn,), np.float32)
        codes[r0:r0 + rn] = d_k.download((rn, m), np.uint8)
        for b in (d_x, d_l, d_i, d_r, d_k):
            b.free()
    d_c.free()
    paths = [f"img/{i:07d}.jpg" for i in range(n + extra)]
    ids, off = _sort_into_lists(lists[:n], nlist)
    shape = {"n": n, "m": m, "nlist": nlist, "d": d, "longest_list": int(np.diff(off).max())}
    stored_bytes = n * (m + 8)
    c_stored = copy_ms(stored_bytes)
    scattered = {r: np.sort(rng.choice(n, r, replace=False)).astype(np.int64) for r in (1, 256, n // 100)}

    # ---- entry level: the movement alone
    d_codes, d_inv, d_ids, d_off = (ctx.buffer(n * m).upload(codes[:n][ids]), ctx.buffer(n * 4).upload(inv[:n][ids]),
                                    ctx.buffer(n * 4).upload(ids), ctx.buffer(off.nbytes).upload(off))
    for b in (1, 256, extra):
        perm, new_off = _sort_into_lists(lists[n:n + b], nlist)
        ins = [ctx.buffer(a.nbytes).upload(a) for a in (codes[n:n + b], inv[n:n + b], new_off, perm)]
        outs = [ctx.buffer(s) for s in ((n + b) * m, (n + b) * 4, (n + b) * 4, (nlist + 1) * 8)]
        ms = _timed(ctx, lambda: ctx.ivf_insert_dev(m, nlist, d_codes.ptr, d_inv.ptr, d_ids.ptr, d_off.ptr, off, ins[0].ptr, ins[1].ptr,
                                                    ins[2].ptr, new_off, ins[3].ptr, *(o.ptr for o in outs)), args.steps, args.warmup)
        emit({"level": "entry", "index": "ivf", "op": "pvs_ivf_insert_dev", "rows": b, **shape, "ms": ms, "copy_ms": c_stored,
              "moved_bytes": (n + b) * (m + 8)})
        for x in ins + outs:
            x.free()
    for r, idx in scattered.items():
        outs = [ctx.buffer(s) for s in ((n - r) * m, (n - r) * 4, (n - r) * 4, (nlist + 1) * 8)]

        def remove():
            with ctx.scratch() as tmp:
                keep, pos = _keep_positions(tmp, idx, n)
                ctx.ivf_remove_dev(m, nlist, n, d_codes.ptr, d_inv.ptr, d_ids.ptr, d_off.ptr, keep.ptr, pos.ptr, *(o.ptr for o in outs))

        emit({"level": "entry", "index": "ivf", "op": "mask + positions + pvs_ivf_remove_dev", "rows": r, **shape,
              "ms": _timed(ctx, remove, args.steps, args.warmup), "copy_ms": c_stored, "moved_bytes": stored_bytes})
        for x in outs:
            x.free()
    c_codes = copy_ms(n * m)
    d_out = ctx.buffer(n * m)
    for r, idx in scattered.items():
        with ctx.scratch() as tmp:                                # kept past the block: freed below
            keep, pos = (tmp.keep(b) for b in _keep_positions(tmp, idx, n))
        ms = _timed(ctx, lambda: ctx.compact_rows_dev(d_codes.ptr, n, m, keep.ptr, pos.ptr, d_out.ptr), args.steps, args.warmup)
        emit({"level": "entry", "index": "codes", "op": "pvs_compact_rows_dev out of place", "rows": r, **shape, "ms": ms,
              "copy_ms": c_codes, "moved_bytes": n * m})
        # in place: the array is restored from d_out's source by an untimed copy (only the bytes behind the first removed row move)
        d_work = ctx.buffer(n * m)
        ctx.copy_dev(d_work.ptr, d_codes.ptr, n * m)
        ms = _timed(ctx, lambda: ctx.compact_rows_dev(d_work.ptr, n, m, keep.ptr, pos.ptr, d_work.ptr, first=int(idx[0])), args.steps,
                    args.warmup, undo=lambda: ctx.copy_dev(d_work.ptr, d_codes.ptr, n * m))
        emit({"level": "entry", "index": "codes", "op": "pvs_compact_rows_dev in place", "rows": r, "first": int(idx[0]), **shape, "ms": ms,
              "copy_ms": c_codes, "moved_bytes": (n - int(idx[0])) * m})
        for x in (keep, pos, d_work):
            x.free()
    for x in (d_codes, d_inv, d_ids, d_off, d_out):
        x.free()

    # ---- class level
    def rebuild_ivf():
        """what IVFCompactIndex.fit does after encoding: download, sort into lists on the host, upload"""
        a, b = flat._device()["codes"].download((n, m), np.uint8), flat._device()["inv"].download((n,), np.float32)
        i2, o2 = _sort_into_lists(lists[:n], nlist)
        bufs = [ctx.buffer(x.nbytes).upload(np.ascontiguousarray(x)) for x in (a[i2], b[i2], i2, o2)]
        for x in bufs:
            x.free()

    def rebuild_flat():
        tmp = CompactIndex(paths[:n], codes[:n], inv[:n], pq, ctx=ctx)
        tmp._device()
        for x in tmp._dev.values():
            if x is not None:
                x.free()
        tmp._dev = None

    flat = CompactIndex(paths[:n], codes[:n], inv[:n], pq, ctx=ctx)
    ivf = IVFCompactIndex(paths[:n], codes[:n][ids], inv[:n][ids], pq, cent, off, ids, ctx=ctx)
    flat._device(), ivf._device()
    rebuilds = {"flat": _timed(ctx, rebuild_flat, args.steps, args.warmup), "ivf": _timed(ctx, rebuild_ivf, args.steps, args.warmup)}
    copies = {"flat": copy_ms(n * (m + 4)), "ivf": c_stored}
    for name, index in (("flat", flat), ("ivf", ivf)):
        for b in (1, 256, extra):
            new = {paths[n + i]: rows[n + i] for i in range(b)}
            gone = paths[n:n + b]
            emit({"level": "class", "index": name, "op": "add", "rows": b, **shape, "copy_ms": copies[name], "rebuild_ms": rebuilds[name],
                  "ms": _timed(ctx, lambda: index.add(new), args.steps, args.warmup, undo=lambda: index.remove(gone))})
        for r, idx in scattered.items():
            emit({"level": "class", "index": name, "op": "remove", "rows": r, **shape, "copy_ms": copies[name], "rebuild_ms": rebuilds[name],
                  "ms": _timed(ctx, index.remove, args.steps, args.warmup, prepare=lambda: [index._paths[i] for i in idx],
                               undo=lambda gone: index.add({p: rows[int(p[4:11])] for p in gone}))})
    flat.close(), ivf.close()
    del rows, codes, inv

    # ------------------------------------------------------------------ dense index
    N, L = args.dense_rows, args.dense_cols
    mat = rng.standard_normal((N + 256, L), dtype=np.float32)
    dpaths = [f"vlad/{i:05d}" for i in range(N + 256)]
    dshape = {"n": N, "L": L, "row_bytes": L * 4}
    c_dense = copy_ms(N * L * 4)

    def rebuild_dense():
        DeviceIndex(dict(zip(dpaths[:N], mat[:N])), ctx).close()

    r_dense = _timed(ctx, rebuild_dense, max(2, args.steps // 2), 1)
    index = DeviceIndex(dict(zip(dpaths[:N], mat[:N])), ctx)
    index.reserve(N + 256)
    for b in (1, 256):
        new = {dpaths[N + i]: mat[N + i] for i in range(b)}
        emit({"level": "class", "index": "dense", "op": "add", "rows": b, **dshape, "copy_ms": c_dense, "rebuild_ms": r_dense,
              "ms": _timed(ctx, lambda: index.add(new), args.steps, args.warmup, undo=lambda: index.remove(list(new)))})
    for r in (1, 256, max(1, N // 100)):
        idx = np.sort(rng.choice(N, r, replace=False)) if r > 1 else np.array([N // 4])
        emit({"level": "class", "index": "dense", "op": "remove (in place)", "rows": r, "first": int(idx[0]), **dshape,
              "copy_ms": c_dense, "rebuild_ms": r_dense, "moved_bytes": (N - int(idx[0]) - r) * L * 4,
              "ms": _timed(ctx, index.remove, args.steps, args.warmup, prepare=lambda: [index._paths[i] for i in idx],
                           undo=lambda gone: index.add({p: mat[int(p[5:])] for p in gone}))})
        # the device's part alone: the in-place compaction of the resident rows, restored by an untimed copy
        with ctx.scratch() as tmp:
            keep, pos = (tmp.keep(b) for b in _keep_positions(tmp, idx.astype(np.int64), N))
        d_save = ctx.buffer(N * L * 4)
        ctx.copy_dev(d_save.ptr, index._db.ptr, N * L * 4)
        emit({"level": "entry", "index": "dense", "op": "pvs_compact_rows_dev in place", "rows": r, "first": int(idx[0]), **dshape,
              "copy_ms": c_dense, "moved_bytes": (N - int(idx[0]) - r) * L * 4,
              "ms": _timed(ctx, lambda: ctx.compact_rows_dev(index._db.ptr, N, L * 4, keep.ptr, pos.ptr, index._db.ptr, first=int(idx[0])),
                           args.steps, args.warmup, undo=lambda: ctx.copy_dev(index._db.ptr, d_save.ptr, N * L * 4))})
        for x in (keep, pos, d_save):
            x.free()
    index.close()
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
