"""Timing of the dense SIFT extractor (csrc/dsift.hip) next to the VLAD encode of the rows it produces.

    python tests/tools/dsift_timing.py [--steps 30] [--warmup 5] [--out profiles/dsift_timing.jsonl]

Shapes: one 500 x 600 uint8 RGB image and a batch of 256 of them, with the default parameters (step 16, sizes (4, 8)) and
with sizes (4, 6, 8, 10) at step 8.  Each timed step queues `inner` extractions (or encodes) back to back and waits for
the stream once; the figure is wall time per call.  Reported per shape: median and spread (min, p10, p90, max) of the
extraction, ms per image, descriptors/s, the least bytes the extraction must move (pixels in + 128 B per row out) and the
time those bytes take at the HBM peak rate, the median of pvs_vlad_encode_dev (K = 256, uint8 rows with the RootSIFT
tail fused) on the same rows in the same run, and the ratio of the two.  One JSON line per shape.

Then the design question of DESIGN.md section 9, in the same run: csrc/bench/dsift_hbm (built on demand with `make
bench/dsift_hbm`) times the product kernel, which keeps every intermediate in LDS, against a straightforward variant that
keeps the eight orientation planes in HBM, on the batch of 256 for both parameter sets, compares their rows byte for byte and
prints one JSON line each, appended to the file."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "python-visual-similarity_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

HBM_PEAK = 8.0e12          # bytes/s, MI355X data sheet


def _stats(samples):
    a = np.sort(np.asarray(samples))
    return {"median": float(np.median(a)), "min": float(a[0]), "p10": float(a[int(0.1 * (len(a) - 1))]),
            "p90": float(a[int(np.ceil(0.9 * (len(a) - 1)))]), "max": float(a[-1])}


def _time(ctx, fn, inner, steps, warmup):
    for _ in range(warmup):
        fn()
    ctx.sync()
    out = []
    for _ in range(steps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        ctx.sync()
        out.append((time.perf_counter() - t0) * 1e3 / inner)
    return _stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dsift_timing.jsonl"))
    args = ap.parse_args()

    import dsift_numpy as tw
    import pvsim
    from pvsim._ffi import DSIFT_U8, PIX_U8_RGB
    from pvsim.engine import DESC_U8_ROOTSIFT, dsift_count

    ctx = pvsim.Context(0)
    cents = np.load(os.path.join(REPO, "tests", "golden", "tables_k256_d128.npz"))["centroids"]
    cb = ctx.codebook(cents)
    base = [np.rint(tw.texture(500, 600, 100 + i, 3)).astype(np.uint8) for i in range(4)]
    lines = []
    for batch in (1, 256):
        imgs = [base[i % len(base)] for i in range(batch)]
        flat = np.concatenate([im.reshape(-1) for im in imgs])
        pix = ctx.buffer(flat.nbytes).upload(flat)
        hw = np.array([[500, 600]] * batch, np.int32)
        for sizes, step in (((4, 8), 16), ((4, 6, 8, 10), 8)):
            per = dsift_count(500, 600, step, sizes)
            total = per * batch
            rows = ctx.buffer(total * 128)
            offs = ctx.buffer((batch + 1) * 8)
            enc = ctx.buffer(batch * cb.K * cb.D * 4)
            inner = 20 if batch == 1 else 2

            def extract():
                ctx.dsift_dev(pix.ptr, PIX_U8_RGB, hw, None, step, sizes, 0.0, DSIFT_U8, rows.ptr, total, offs.ptr)

            def encode():
                ctx.vlad_encode_dev(cb, rows.ptr, DESC_U8_ROOTSIFT, offs.ptr, batch, total, enc.ptr)

            ex = _time(ctx, extract, inner, args.steps, args.warmup)
            en = _time(ctx, encode, inner, args.steps, args.warmup)
            min_bytes = flat.nbytes + total * 128
            line = {"device": ctx.device_name(), "images": batch, "image": "500x600 uint8 RGB", "sizes": list(sizes), "step": step,
                    "rows_per_image": per, "inner_calls_per_step": inner, "steps": args.steps, "warmup": args.warmup,
                    "extract_ms": ex, "extract_ms_per_image": ex["median"] / batch,
                    "descriptors_per_s": total / (ex["median"] * 1e-3),
                    "min_bytes": int(min_bytes), "min_bytes_ms_at_hbm_peak": min_bytes / HBM_PEAK * 1e3,
                    "min_bytes_GBps_achieved": min_bytes / (ex["median"] * 1e-3) / 1e9,
                    "vlad_encode_ms": en, "extract_over_encode": ex["median"] / en["median"]}
            print(json.dumps(line))
            lines.append(line)
            for b in (rows, offs, enc):
                b.free()
        pix.free()
    ctx.close()
    csrc = os.path.join(REPO, "python-visual-similarity_amd", "csrc")
    exe = os.path.join(csrc, "bench", "dsift_hbm")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", csrc, "bench/dsift_hbm"], check=True)
    for sizes, step in (((4, 8), 16), ((4, 6, 8, 10), 8)):
        res = subprocess.run([exe, "256", "500", "600", str(step), ",".join(map(str, sizes)), str(args.steps)], check=True,
                             capture_output=True, text=True, timeout=600)
        line = json.loads(res.stdout.strip().splitlines()[-1])
        line["sizes"] = list(sizes)
        print(json.dumps(line))
        lines.append(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
