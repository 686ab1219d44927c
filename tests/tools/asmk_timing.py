"""Timing of the ASMK* index (csrc/asmk.hip): aggregate, score and select, with a dense ranking of the same database size for scale.

    python tests/tools/asmk_timing.py [--steps 10] [--warmup 2] [--n 100000] [--entries 1000] [--words 65536] [--out profiles/asmk_timing.jsonl]

Workload: an inverted file of N = 10^5 images x 1000 synthetic entries (uniform random words of K = 65536, random 128-bit
signatures; the pairs (word, image) are drawn as one integer and made unique, so every image is at most once in a list), idf
weights from the real list lengths, alpha = 3, tau = 0.  Queries: nq in {1, 64} images of 1000 random words.  One JSON line per nq:
    aggregate_ms   pvs_asmk_aggregate_dev on 256 images x 1000 uint8 rows with random labels (timer slot 1), D = 128, no projection
    score_ms       pvs_asmk_score_dev (timer slot 2), with entries scanned per second and the bytes of the lists the queries touch
                   (20 bytes per entry: id + signature) over that time
    select_ms      pvs_topk_dev on the panel, k = 100 (timer slot 3)
    dense_rank_ms  pvs_cosine_topk_dev, the call DeviceIndex.rank makes, for the same queries' count against N x 32768 float32 rows
                   resident on the device (a block of random rows repeated), k = 100, wall time
Each figure is the median of `steps` calls after `warmup`, timed one call at a time.  Nothing here is a pass / fail threshold."""
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
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--entries", type=int, default=1000)
    ap.add_argument("--words", type=int, default=65536)
    ap.add_argument("--dense-dim", type=int, default=32768, help="0 skips the dense ranking")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "asmk_timing.jsonl"))
    args = ap.parse_args()

    import pvsim
    from pvsim import asmk

    ctx = pvsim.Context(0)
    rng = np.random.default_rng(17)
    N, K, bits, W, k = args.n, args.words, 128, 4, 100
    base = {"device": ctx.device_name(), "date": time.strftime("%Y-%m-%d"), "n": N, "words": K, "bits": bits, "k": k, "alpha": 3.0,
            "tau": 0.0, "steps": args.steps, "warmup": args.warmup}

    def event_ms(fn, slot):
        """event time of `slot` for single calls: median of steps after warmup"""
        for _ in range(args.warmup):
            fn()
        out = []
        ctx.timers_enable(True)
        for _ in range(args.steps):
            ctx.sync()
            ctx.timers_reset()
            fn()
            ctx.sync()
            out.append(ctx.timers()[slot][0])
        ctx.timers_enable(False)
        return _stats(out)

    # ---- the inverted file
    keys = np.unique(rng.integers(0, K * N, N * args.entries, dtype=np.int64))          # sorted by (word, image), each pair once
    E = len(keys)
    word_of = (keys // N).astype(np.int32)
    ent_img = (keys % N).astype(np.int32)
    del keys
    word_off = np.zeros(K + 1, np.int64)
    np.cumsum(np.bincount(word_of, minlength=K), out=word_off[1:])
    sizes = np.diff(word_off)
    wt = asmk.word_weights(sizes, N, True)
    sums = np.bincount(ent_img, weights=1023.0 * wt[word_of], minlength=N)
    gamma_db = np.where(sums > 0, 1.0 / np.sqrt(np.maximum(sums, 1.0)), 0.0).astype(np.float32)
    del word_of
    sel = asmk.selectivity(bits, 3.0, 0.0)
    base.update(entries=int(E), longest_list=int(sizes.max()), mean_list=round(float(sizes.mean()), 2), index_bytes=int(E) * (4 + 4 * W))
    dev = [ctx.buffer(a.nbytes).upload(a) for a in (word_off, ent_img, gamma_db, wt, sel)]
    d_sig = ctx.buffer(E * 4 * W)
    step = 1 << 24
    for e0 in range(0, E, step):                                                         # signatures in pieces: 1.6 GB in all
        en = min(step, E - e0)
        d_sig.upload(rng.integers(0, 1 << 32, (en, W), dtype=np.uint64).astype(np.uint32), e0 * 4 * W)
    del ent_img

    # ---- aggregate: 256 images x `entries` rows, random labels
    ni, D = 256, 128
    off = np.arange(ni + 1, dtype=np.int64) * args.entries
    total = int(off[-1])
    cb = ctx.codebook(rng.random((K, D), dtype=np.float32) * np.float32(0.2))
    ag = [ctx.buffer(total * D).upload(rng.integers(0, 120, (total, D), dtype=np.uint8)), ctx.buffer(off.nbytes).upload(off),
          ctx.buffer(total * 4).upload(rng.integers(0, K, total, dtype=np.int32)), ctx.buffer(total * 4), ctx.buffer(total * 4 * W),
          ctx.buffer(ni * 4)]
    aggregate_ms = event_ms(lambda: ctx.asmk_aggregate_dev(cb, ag[0].ptr, pvsim.engine.DESC_U8_ROOTSIFT, ag[1].ptr, off, ni, total, ag[2].ptr,
                                                           None, bits, ag[3].ptr, ag[4].ptr, ag[5].ptr), "aggregate")
    base.update(aggregate_images=ni, aggregate_rows=total)
    for b in ag:
        b.free()
    cb.close()

    # ---- dense rows for scale
    L = args.dense_dim
    d_dense = d_inv = None
    if L:
        blk = 2048
        d_dense, d_inv = ctx.buffer(N * L * 4), ctx.buffer(N * 4)
        d_dense.upload(rng.standard_normal((blk, L), dtype=np.float32))
        for r0 in range(blk, N, blk):
            ctx.copy_dev(d_dense.ptr + r0 * L * 4, d_dense.ptr, min(blk, N - r0) * L * 4)
        ctx.row_inv_norms_dev(d_dense.ptr, N, L, d_inv.ptr)
        ctx.sync()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for nq in (1, 64):
        q_words = np.concatenate([np.sort(rng.choice(K, args.entries, replace=False)) for _ in range(nq)]).astype(np.int32)
        q_off = np.arange(nq + 1, dtype=np.int64) * args.entries
        q_sigs = rng.integers(0, 1 << 32, (len(q_words), W), dtype=np.uint64).astype(np.uint32)
        gq = asmk.gammas(q_off, q_words, wt)
        bufs = [ctx.buffer(q_words.nbytes).upload(q_words), ctx.buffer(q_sigs.nbytes).upload(q_sigs), ctx.buffer(gq.nbytes).upload(gq),
                ctx.buffer(nq * N * 4), ctx.buffer(nq * k * 8), ctx.buffer(nq * k * 4)]
        d_w, d_s, d_g, d_panel, d_idx, d_val = bufs

        def score():
            ctx.asmk_score_dev(nq, q_off, d_w.ptr, d_s.ptr, bits, K, dev[0].ptr, dev[1].ptr, d_sig.ptr, N, dev[3].ptr, dev[4].ptr, d_g.ptr,
                               dev[2].ptr, d_panel.ptr, N)

        score_ms = event_ms(score, "cosine_gemm")
        select_ms = event_ms(lambda: ctx.topk_dev(d_panel.ptr, nq, N, N, k, 0, False, d_idx.ptr, d_val.ptr), "topk")
        scanned = int(sizes[q_words].sum())
        rec = dict(base, nq=nq, query_entries=args.entries, aggregate_ms=aggregate_ms, score_ms=score_ms, select_ms=select_ms,
                   entries_scanned=scanned, entries_per_s=scanned / (score_ms["median"] * 1e-3),
                   list_gbytes_per_s=scanned * (4 + 4 * W) / (score_ms["median"] * 1e-3) / 1e9)
        if L:
            d_q, d_iq = ctx.buffer(nq * L * 4).upload(rng.standard_normal((nq, L), dtype=np.float32)), ctx.buffer(nq * 4)
            ctx.row_inv_norms_dev(d_q.ptr, nq, L, d_iq.ptr)

            def dense():
                ctx.cosine_topk_dev(d_q.ptr, nq, d_dense.ptr, N, L, d_iq.ptr, d_inv.ptr, k, 0, False, d_idx.ptr, d_val.ptr)
                ctx.sync()

            for _ in range(args.warmup):
                dense()
            out = []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                dense()
                out.append((time.perf_counter() - t0) * 1e3)
            rec.update(dense_rank_ms=_stats(out), dense_dim=L)
            d_q.free(), d_iq.free()
        print(json.dumps(rec), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        for b in bufs:
            b.free()
    for b in dev + [d_sig] + ([d_dense, d_inv] if L else []):
        b.free()
    ctx.close()


if __name__ == "__main__":
    main()
