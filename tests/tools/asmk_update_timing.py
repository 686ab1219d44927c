"""Timing of ASMK maintenance (csrc/asmk_update.hip): the device inversion, the device build, add and remove,
beside a plain device-to-device copy of the arrays (the control) and the host route the inversion replaces (the alternative), all in
one run.

    python tests/tools/asmk_update_timing.py [--steps 5] [--warmup 1] [--n 100000] [--entries 1000] [--words 65536] [--batch 1000]
                                             [--build-images 10000] [--out profiles/asmk_update_timing.jsonl]

Workload: that of asmk_timing.py, image-major: N = 10^5 images x 1000 synthetic entries (the pairs (image, word) drawn as one integer
and made unique, uniform over K = 65536 words, random 128-bit signatures), in slots as pvs_asmk_aggregate_dev leaves them, every
slot an entry.  One JSON line per case, `ms` the wall time of one call ending in a stream synchronise (median of `steps` after
`warmup`):
  invert        pvs_asmk_invert_dev on the resident slots
  copy          the control: pvs_copy_dev of the bytes the inverted file holds, E (4 + 16)
  host_route    the alternative, what ASMKIndex.build does by default: download the slots, np.argsort(kind="stable") on the host
                (pvsim.asmk.invert), upload the three arrays
  build_device / build_host   ASMKIndex.build(on_device=True / False) on `build-images` images x `entries` random uint8 rows: assign,
                aggregate, invert, weights, gamma (the whole corpus would spend its time in the assignment, which both routes share)
  add / remove  a frozen index over the whole inverted file takes `batch` images of `entries` random rows (assign, aggregate,
                invert, insert, gamma) and gives them up again; each timed add is undone by the timed remove
Nothing here is a pass / fail threshold."""
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


def _timed(ctx, fn, steps, warmup, name, after=None):
    """wall milliseconds of fn() + synchronise, `steps` samples after `warmup`; `after` runs untimed behind every call"""
    out = []
    for i in range(warmup + steps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        dt = (time.perf_counter() - t0) * 1e3
        if after is not None:
            after()
        print(f"  {name} run {i}: {dt:.2f} ms", flush=True)
        if i >= warmup:
            out.append(dt)
    return _stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--entries", type=int, default=1000)
    ap.add_argument("--words", type=int, default=65536)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--build-images", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "asmk_update_timing.jsonl"))
    args = ap.parse_args()

    import pvsim
    from pvsim import asmk
    from pvsim.asmk import ASMKIndex
    from pvsim.verify import LocalFeatureIndex

    ctx = pvsim.Context(0)
    rng = np.random.default_rng(18)
    N, K, bits, W = args.n, args.words, 128, 4
    base = {"device": ctx.device_name(), "date": time.strftime("%Y-%m-%d"), "n": N, "words": K, "bits": bits, "steps": args.steps,
            "warmup": args.warmup}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(case, **fields):
        rec = dict(base, case=case, **fields)
        print(json.dumps(rec), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")

    # ---- image-major entries in slots: every slot an entry
    keys = np.unique(rng.integers(0, K * N, N * args.entries, dtype=np.int64))          # image * K + word: sorted by (image, word)
    E = len(keys)
    words = (keys % K).astype(np.int32)
    counts = np.bincount(keys // K, minlength=N).astype(np.int32)
    del keys
    off = np.zeros(N + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    file_bytes = E * (4 + 4 * W)
    base.update(entries=int(E), file_bytes=int(file_bytes))
    d_off, d_cnt, d_word, d_sig = ctx.buffer(off.nbytes).upload(off), ctx.buffer(counts.nbytes).upload(counts), ctx.buffer(E * 4).upload(words), \
        ctx.buffer(E * 4 * W)
    step = 1 << 24
    for e0 in range(0, E, step):
        en = min(step, E - e0)
        d_sig.upload(rng.integers(0, 1 << 32, (en, W), dtype=np.uint64).astype(np.uint32), e0 * 4 * W)
    d_woff, d_img, d_osig = ctx.buffer((K + 1) * 8), ctx.buffer(E * 4), ctx.buffer(E * 4 * W)
    print(f"{E} entries in slots, {file_bytes / 1e9:.2f} GB inverted", flush=True)

    def invert():
        ctx.asmk_invert_dev(K, bits, d_off.ptr, off, N, d_cnt.ptr, d_word.ptr, d_sig.ptr, 0, d_woff.ptr, d_img.ptr, d_osig.ptr)

    ms = _timed(ctx, invert, args.steps, args.warmup, "invert")
    emit("invert", ms=ms, gbytes_per_s=file_bytes / (ms["median"] * 1e-3) / 1e9)

    d_copy = ctx.buffer(file_bytes)

    def copy():
        ctx.copy_dev(d_copy.ptr, d_img.ptr, E * 4)
        ctx.copy_dev(d_copy.ptr + E * 4, d_osig.ptr, E * 4 * W)

    copy_ms = _timed(ctx, copy, args.steps, args.warmup, "copy")
    emit("copy", ms=copy_ms, gbytes_per_s=file_bytes / (copy_ms["median"] * 1e-3) / 1e9)
    d_copy.free()

    host = {}

    def host_route():
        w, s = d_word.download((E,), np.int32), d_sig.download((E, W), np.uint32)
        c = d_cnt.download((N,), np.int32).astype(np.int64)
        ent_off = np.zeros(N + 1, np.int64)
        np.cumsum(c, out=ent_off[1:])
        host["file"] = asmk.invert(ent_off, w, s, K)                                     # every slot is an entry: nothing to compact
        for buf, a in zip((d_woff, d_img, d_osig), host["file"]):
            buf.upload(a)

    ms = _timed(ctx, host_route, args.steps, args.warmup, "host_route")
    emit("host_route", ms=ms)
    word_off, ent_img, ent_sig = host.pop("file")
    invert()                                                                             # the device's file against the host's
    same = (np.array_equal(d_woff.download((K + 1,), np.int64), word_off) and np.array_equal(d_img.download((E,), np.int32), ent_img)
            and np.array_equal(d_osig.download((E, W), np.uint32), ent_sig))
    emit("check", device_equals_host=bool(same))
    for b in (d_off, d_cnt, d_word, d_sig, d_woff, d_img, d_osig):
        b.free()

    # ---- the two build routes on a corpus of rows
    cent = rng.random((K, 128), dtype=np.float32) * np.float32(0.2)
    nb = args.build_images
    b_off = np.arange(nb + 1, dtype=np.int64) * args.entries
    rows = ctx.buffer(int(b_off[-1]) * 128)
    for r0 in range(0, int(b_off[-1]), 1 << 20):
        rn = min(1 << 20, int(b_off[-1]) - r0)
        rows.upload(rng.integers(0, 120, (rn, 128), dtype=np.uint8), r0 * 128)
    local = LocalFeatureIndex(ctx, rows, ctx.buffer(int(b_off[-1]) * 24), b_off, list(range(nb)))
    for name, on_device in (("build_device", True), ("build_host", False)):
        def build():
            host["index"] = ASMKIndex.build(local, cent, on_device=on_device)

        emit(name, ms=_timed(ctx, build, args.steps, args.warmup, name, after=lambda: host.pop("index").close()), images=nb,
             rows=int(b_off[-1]))
    local.close()

    # ---- add and remove on a frozen index over the whole file
    wt = asmk.word_weights(np.diff(word_off), N, True)
    sums = np.bincount(ent_img, weights=1023.0 * wt[np.repeat(np.arange(K, dtype=np.int32), np.diff(word_off))], minlength=N)
    gamma = np.where(sums > 0, 1.0 / np.sqrt(np.maximum(sums, 1.0)), 0.0).astype(np.float32)
    index = ASMKIndex(list(range(N)), cent, word_off, ent_img, ent_sig, gamma, wt, asmk.selectivity(bits), bits, ctx=ctx, frozen=True)
    del word_off, ent_img, ent_sig
    batch_rows = [rng.integers(0, 120, (args.entries, 128), dtype=np.uint8) for _ in range(args.batch)]
    state = {"round": 0}

    def names():
        return [N + state["round"] * args.batch + i for i in range(args.batch)]

    def add():
        index.add(names(), batch_rows)

    def remove():
        index.remove(names())
        state["round"] += 1

    add_ms, remove_ms = [], []
    for i in range(args.warmup + args.steps):
        a = _timed(ctx, add, 1, 0, "add")["median"]
        r = _timed(ctx, remove, 1, 0, "remove")["median"]
        if i >= args.warmup:
            add_ms.append(a)
            remove_ms.append(r)
    moved = int(index.word_off[-1]) * (4 + 4 * W)
    emit("add", ms=_stats(add_ms), images=args.batch, moved_bytes=moved, copy_ms=copy_ms, ratio=float(np.median(add_ms)) / copy_ms["median"])
    emit("remove", ms=_stats(remove_ms), images=args.batch, moved_bytes=moved, copy_ms=copy_ms,
         ratio=float(np.median(remove_ms)) / copy_ms["median"])
    index.close()
    ctx.close()


if __name__ == "__main__":
    main()
