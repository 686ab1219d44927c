"""Timing of the keypoint SIFT extractor (csrc/sift.hip).

    python tests/tools/sift_timing.py [--steps 10] [--warmup 2] [--out profiles/sift_timing.jsonl]

Shapes: one 500 x 600 uint8 RGB image and a batch of 256 of them, default parameters.  pvs_sift_dev waits for the stream itself
(it returns the row total), so every call is timed on its own, wall time, with a capacity that holds all rows.  Reported per
shape: median and spread of the call, ms per image, keypoints (rows) and keypoints/s.  One JSON line per shape.  The per-kernel
share comes from running this tool under `rocprofv3 --kernel-trace --stats -- python tests/tools/sift_timing.py --steps 3`."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "python-visual-similarity_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))


def _stats(samples):
    a = np.sort(np.asarray(samples))
    return {"median": float(np.median(a)), "min": float(a[0]), "p10": float(a[int(0.1 * (len(a) - 1))]),
            "p90": float(a[int(np.ceil(0.9 * (len(a) - 1)))]), "max": float(a[-1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sift_timing.jsonl"))
    args = ap.parse_args()

    import dsift_numpy as tw
    import pvsim
    from pvsim import CapacityError
    from pvsim._ffi import DSIFT_U8, PIX_U8_RGB

    ctx = pvsim.Context(0)
    base = [np.rint(tw.texture(500, 600, 100 + i, 3)).astype(np.uint8) for i in range(4)]
    lines = []
    for batch in (1, 256):
        imgs = [base[i % len(base)] for i in range(batch)]
        flat = np.concatenate([im.reshape(-1) for im in imgs])
        pix = ctx.buffer(flat.nbytes).upload(flat)
        hw = np.array([[500, 600]] * batch, np.int32)
        offs = ctx.buffer((batch + 1) * 8)
        try:
            total = ctx.sift_dev(pix.ptr, PIX_U8_RGB, hw, None, 0, 3, 0.04, 10.0, 1.6, True, DSIFT_U8, None, 0, None, offs.ptr)
        except CapacityError as e:
            total = e.args[1]
        rows = ctx.buffer(max(total, 1) * 128)

        def extract():
            return ctx.sift_dev(pix.ptr, PIX_U8_RGB, hw, None, 0, 3, 0.04, 10.0, 1.6, True, DSIFT_U8, rows.ptr, total, None, offs.ptr)

        for _ in range(args.warmup):
            extract()
        samples = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            extract()
            samples.append((time.perf_counter() - t0) * 1e3)
        ex = _stats(samples)
        line = {"device": ctx.device_name(), "images": batch, "image": "500x600 uint8 RGB", "keypoints": int(total),
                "keypoints_per_image": total / batch, "steps": args.steps, "warmup": args.warmup, "extract_ms": ex,
                "extract_ms_per_image": ex["median"] / batch, "keypoints_per_s": total / (ex["median"] * 1e-3)}
        print(json.dumps(line))
        lines.append(line)
        for b in (pix, rows, offs):
            b.free()
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
