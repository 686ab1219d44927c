"""Timing of spatial re-ranking (csrc/match.hip): one query of 2000 rows against a shortlist of 100 images x 2000 rows.

    python tests/tools/match_timing.py [--steps 10] [--warmup 2] [--reps 50] [--images 100] [--rows 2000] [--out profiles/match_timing.jsonl]

Per stage and end to end, wall time of `reps` back-to-back calls closed by one stream synchronisation, divided by `reps` (a single
call is a fraction of a millisecond: too short a window on its own), median of `steps` such samples:
  match_forward   pvs_match_u8_dev, query -> every candidate (one launch for the shortlist)
  match_reverse   the transposed call of the mutual check (every candidate -> query)
  filter          pvs_match_filter_dev (ratio 0.8, mutual)
  verify          pvs_verify_dev (tol 12 px, two refinement rounds)
  end_to_end      the four calls back to back, one synchronisation
and the same matching done the only way the library could do it before: one pvs_l2_knn_dev(k = 2) call per image pair on float32
casts of the same rows (`knn_per_pair`, forward direction only, so it is compared with match_forward).  The float path's indices
and distances are checked against the int8 kernel's on the run.  `knn_over_match` is the measured ratio.  Appends one JSON line.
A third of each candidate's rows are noisy copies of query rows placed by a planted similarity, so the filter keeps several
hundred matches per pair and the verification has real work."""
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
    return {"median": round(float(np.median(a)), 4), "min": round(float(a[0]), 4), "max": round(float(a[-1]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "match_timing.jsonl"))
    args = ap.parse_args()

    import match_numpy as tw
    import pvsim

    n_img, n = args.images, args.rows
    rng = np.random.default_rng(3)
    q_rows = tw.sift_like_rows(n, 1)
    q_frames = np.zeros((n, 6), np.float32)
    q_frames[:, 0:2] = rng.uniform((0, 0), (640, 480), size=(n, 2))
    q_frames[:, 2], q_frames[:, 3] = rng.uniform(2, 20, n), rng.uniform(0, 360, n)
    db_rows = np.empty((n_img * n, 128), np.uint8)
    db_frames = np.zeros((n_img * n, 6), np.float32)
    th, sc = np.deg2rad(33.0), 1.37
    M = sc * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    for k in range(n_img):
        rows = tw.sift_like_rows(n, 100 + k)
        fr = np.zeros((n, 6), np.float32)
        fr[:, 0:2] = rng.uniform((0, 0), (900, 900), size=(n, 2))
        fr[:, 2], fr[:, 3] = rng.uniform(2, 30, n), rng.uniform(0, 360, n)
        src, dst = rng.choice(n, n // 3, replace=False), rng.choice(n, n // 3, replace=False)
        rows[dst] = np.clip(q_rows[src].astype(np.int64) + rng.integers(-5, 6, size=(len(src), 128)), 0, 255).astype(np.uint8)
        fr[dst, 0:2] = q_frames[src, 0:2] @ M.T + (41.5, -17.25) + rng.normal(0, 0.7, size=(len(src), 2))
        fr[dst, 2] = q_frames[src, 2] * sc * (1 + rng.normal(0, 0.02, len(src)))
        fr[dst, 3] = (q_frames[src, 3] + 33.0 + rng.normal(0, 1.5, len(src))) % 360.0
        db_rows[k * n:(k + 1) * n], db_frames[k * n:(k + 1) * n] = rows, fr

    ctx = pvsim.Context(0)
    up = lambda a: ctx.buffer(a.nbytes).upload(a)                            # noqa: E731
    d_q, d_qf, d_db, d_dbf = up(q_rows), up(q_frames), up(db_rows), up(db_frames)
    off_q, off_db = np.array([0, n], np.int64), np.arange(n_img + 1, dtype=np.int64) * n
    pairs = np.stack([np.zeros(n_img, np.int32), np.arange(n_img, dtype=np.int32)], axis=1)
    rev_pairs = np.ascontiguousarray(pairs[:, ::-1])
    ta = n_img * n
    fwd = [ctx.buffer(ta * 4) for _ in range(3)]
    rev = [ctx.buffer(ta * 4) for _ in range(3)]
    d_m, d_c = ctx.buffer(ta * 8), ctx.buffer(n_img * 4)
    d_inl, d_mod, d_best, d_mask = ctx.buffer(n_img * 4), ctx.buffer(n_img * 48), ctx.buffer(n_img * 4), ctx.buffer(ta)

    def s_fwd():
        ctx.match_u8_dev(d_q.ptr, off_q, d_db.ptr, off_db, pairs, fwd[0].ptr, fwd[1].ptr, fwd[2].ptr)

    def s_rev():
        ctx.match_u8_dev(d_db.ptr, off_db, d_q.ptr, off_q, rev_pairs, rev[0].ptr, rev[1].ptr, rev[2].ptr)

    def s_filter():
        ctx.match_filter_dev(off_q, off_db, pairs, fwd[0].ptr, fwd[1].ptr, fwd[2].ptr, rev[0].ptr, 0.8 * 0.8, True, d_m.ptr, d_c.ptr)

    def s_verify():
        ctx.verify_dev(d_qf.ptr, off_q, d_dbf.ptr, off_db, pairs, d_m.ptr, d_c.ptr, 12.0, 2, d_inl.ptr, d_mod.ptr, d_best.ptr, d_mask.ptr)

    def s_all():
        s_fwd(), s_rev(), s_filter(), s_verify()

    # the parent's way: float32 casts, one neighbour search per pair
    d_q32, d_db32 = up(q_rows.astype(np.float32)), up(db_rows.astype(np.float32))
    k_idx, k_d = ctx.buffer(ta * 2 * 8), ctx.buffer(ta * 2 * 8)

    def s_knn():
        for k in range(n_img):
            ctx.l2_knn_dev(d_q32.ptr, n, d_db32.ptr + k * n * 512, n, 128, False, 2, k_idx.ptr + k * n * 16, k_d.ptr + k * n * 16)

    def timed(fn, reps):
        for _ in range(args.warmup):
            fn()
        ctx.sync()
        out = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            ctx.sync()
            out.append((time.perf_counter() - t0) * 1e3 / reps)
        return _stats(out)

    rec = {"device": ctx.device_name(), "date": time.strftime("%Y-%m-%d"), "query_rows": n, "images": n_img, "rows_per_image": n,
           "steps": args.steps, "warmup": args.warmup, "reps": args.reps}
    for name, fn in (("match_forward", s_fwd), ("match_reverse", s_rev), ("filter", s_filter), ("verify", s_verify),
                     ("end_to_end", s_all), ("knn_per_pair", s_knn)):
        rec[name + "_ms"] = timed(fn, 1 if name == "knn_per_pair" else args.reps)      # the float path waits inside every call
    counts = d_c.download((n_img,), np.int32)
    inl = d_inl.download((n_img,), np.int32)
    rec["matches_per_pair"] = float(counts.mean())
    rec["inliers_per_pair"] = float(inl.mean())
    idx = fwd[0].download((ta,), np.int32)
    d1, d2 = fwd[1].download((ta,), np.int32), fwd[2].download((ta,), np.int32)
    kidx, kd = k_idx.download((ta, 2), np.int64), k_d.download((ta, 2), np.float64)
    rec["float_path_agrees"] = bool(np.array_equal(kidx[:, 0], idx) and np.array_equal(kd[:, 0], d1.astype(np.float64))
                                    and np.array_equal(kd[:, 1], d2.astype(np.float64)))
    rec["knn_per_pair_ms_per_call"] = round(rec["knn_per_pair_ms"]["median"] / n_img, 4)
    rec["knn_over_match"] = round(rec["knn_per_pair_ms"]["median"] / rec["match_forward_ms"]["median"], 2)
    pair_ops = 2.0 * n * n * 128 * n_img
    rec["match_forward_int8_tops"] = round(pair_ops / (rec["match_forward_ms"]["median"] * 1e-3) / 1e12, 2)
    print(json.dumps(rec), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
