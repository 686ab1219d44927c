"""Timing of the top-m assignment (csrc/assign_topm.hip) next to the exact single-assignment kernel (assign_kernel, csrc/vlad.hip).

    python tests/tools/assign_topm_timing.py [--steps 10] [--warmup 2] [--words 65536] [--out profiles/assign_topm_timing.jsonl]

Workload: K = 65536 words at D = 128 (RootSIFT rows of random SIFT-like prototypes), uint8 SIFT-like rows.  Two steps: one query of
2000 rows, and a batch of 10^6 rows.  Every step is its own child process under its own `timeout` (this driver never opens the
device); a step that fails or runs out of time ends the run.  Inside a step the variants ALTERNATE in the same process, round by
round: pvs_kmeans_predict_dev, then pvs_kmeans_topm_dev at m = 1, 5 and 8 with splits = 0 (the host's choice), and at 2000 rows also
with splits = 1.  Each call is timed on its own by the context's event timers (slot 0); the figure of a variant is the median of
`steps` rounds after `warmup` rounds.  One JSON line per step, appended to --out, with per variant the time and the achieved float32
FLOP/s, 2 n K D over the time, against the 157.3 TFLOP/s float32 MATRIX peak of the MI355X (v_mfma_f32_32x32x2_f32 runs at the
vector-FMA rate).  No profiler and no hardware counters are involved.  Nothing here is a pass / fail threshold."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "python-visual-similarity_amd"))

PEAK_F32_MATRIX_TFLOPS = 157.3
STEPS = {"query_2000": (2000, 120), "batch_1000000": (1000000, 420)}          # rows, seconds allowed


def _stats(samples):
    a = np.sort(np.asarray(samples))
    return {"median": round(float(np.median(a)), 4), "min": round(float(a[0]), 4), "max": round(float(a[-1]), 4)}


def run_step(args):
    import pvsim
    from pvsim.engine import DESC_U8_ROOTSIFT
    n, K, D = STEPS[args.step][0], args.words, 128
    rng = np.random.default_rng(23)
    proto = rng.integers(0, 80, (K, D), dtype=np.uint8)
    pf = proto.astype(np.float32)
    cent = np.sqrt(pf / (pf.sum(axis=1, keepdims=True) + np.float32(1e-7)))
    rows = np.clip(proto[rng.integers(0, K, n)].astype(np.int16) + rng.integers(-6, 7, (n, D), dtype=np.int16), 0, 255).astype(np.uint8)

    ctx = pvsim.Context(0)
    cb = ctx.codebook(cent)
    d_rows = ctx.buffer(rows.nbytes).upload(rows)
    d_lab, d_val = ctx.buffer(n * 8 * 4), ctx.buffer(n * 8 * 4)
    variants = [("predict", lambda: ctx.kmeans_predict_dev(cb, d_rows.ptr, DESC_U8_ROOTSIFT, n, d_lab.ptr))]
    for m in (1, 5, 8):
        variants.append((f"topm_m{m}", lambda m=m: ctx.kmeans_topm_dev(cb, d_rows.ptr, DESC_U8_ROOTSIFT, n, m, d_lab.ptr, d_val.ptr, 0)))
    if n <= 2000:
        for m in (1, 5, 8):
            variants.append((f"topm_m{m}_splits1", lambda m=m: ctx.kmeans_topm_dev(cb, d_rows.ptr, DESC_U8_ROOTSIFT, n, m, d_lab.ptr, d_val.ptr, 1)))

    samples = {name: [] for name, _ in variants}
    ctx.timers_enable(True)
    for rnd in range(args.warmup + args.steps):
        for name, fn in variants:                                              # the variants alternate inside a round
            ctx.sync()
            ctx.timers_reset()
            fn()
            ctx.sync()
            ms, launches = ctx.timers()["assign"]
            if rnd >= args.warmup:
                samples[name].append(ms)
    ctx.timers_enable(False)
    # the two entry points agree on the nearest word (checked once, outside the timed rounds)
    ctx.kmeans_predict_dev(cb, d_rows.ptr, DESC_U8_ROOTSIFT, n, d_lab.ptr)
    want = d_lab.download((n,), np.int32)
    ctx.kmeans_topm_dev(cb, d_rows.ptr, DESC_U8_ROOTSIFT, n, 5, d_lab.ptr, None, 0)
    same = bool(np.array_equal(d_lab.download((n, 5), np.int32)[:, 0], want))

    flop = 2.0 * n * K * D
    rec = {"tool": "tests/tools/assign_topm_timing.py", "step": args.step, "device": ctx.device_name(), "date": time.strftime("%Y-%m-%d"),
           "rows": n, "words": K, "dim": D, "kind": "uint8 RootSIFT", "steps": args.steps, "warmup": args.warmup,
           "method": "context event timers, slot 0; variants alternate in one process; median of steps after warmup; no profiler, no counters",
           "peak_f32_matrix_tflops": PEAK_F32_MATRIX_TFLOPS, "column0_equals_predict": same, "variants": {}}
    for name, _ in variants:
        st = _stats(samples[name])
        tf = flop / (st["median"] * 1e-3) / 1e12
        rec["variants"][name] = {"ms": st, "f32_tflops": round(tf, 2), "share_of_f32_matrix_peak": round(tf / PEAK_F32_MATRIX_TFLOPS, 4)}
    for b in (d_rows, d_lab, d_val):
        b.free()
    cb.close()
    ctx.close()
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--words", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "assign_topm_timing.jsonl"))
    ap.add_argument("--step", choices=sorted(STEPS), help="run this one step in this process (what the driver starts)")
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    for step, (_, limit) in STEPS.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--steps", str(args.steps),
               "--warmup", str(args.warmup), "--words", str(args.words), "--out", args.out]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"step {step} ended with status {rc}: nothing more is started", file=sys.stderr)
            sys.exit(rc)


if __name__ == "__main__":
    main()
