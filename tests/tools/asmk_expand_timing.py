"""Timing of the ASMK query expansion (csrc/asmk_expand.hip): the expand call beside the two score + top-k calls
it sits between, in one run.

    python tests/tools/asmk_expand_timing.py [--steps 5] [--warmup 1] [--n 100000] [--entries 1000] [--words 65536] [--members 10]
                                             [--min-support 2] [--out profiles/asmk_expand_timing.jsonl]

Workload: that of asmk_timing.py: N = 10^5 images x 1000 synthetic entries (the pairs (image, word) drawn as one integer and made
unique, uniform over K = 65536 words, random 128-bit signatures), inverted on the device.  A query is the entry list of a database
image with 8 of its 128 bits flipped per signature.  For nq = 1 and nq = 64, one JSON line per case, `ms` the wall time of the calls
ending in a stream synchronise (median of `steps` after `warmup`, with min and max):
  first     pvs_asmk_score_dev + pvs_topk_dev to depth R on the plain entries (the lists the members come from)
  expand    the fill of the output words, pvs_asmk_expand_dev, and the download of counts and sums (what one pass of
            ASMKIndex.rank_entries(expand=) does between the two rankings); idf weights, flat votes, query_vote 2, h_max 32
  second    pvs_asmk_score_dev + pvs_topk_dev to depth 100 on the expanded entries, in rows of `cap` slots
with the entry counts of the queries before and after.  Nothing here is a pass / fail threshold."""
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


def _timed(ctx, fn, steps, warmup, name):
    """wall milliseconds of fn() + synchronise, `steps` samples after `warmup`"""
    out = []
    for i in range(warmup + steps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        dt = (time.perf_counter() - t0) * 1e3
        print(f"  {name} run {i}: {dt:.3f} ms", flush=True)
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
    ap.add_argument("--members", type=int, default=10)
    ap.add_argument("--min-support", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "asmk_expand_timing.jsonl"))
    args = ap.parse_args()

    import pvsim
    from pvsim import ASMKExpansion, asmk

    ctx = pvsim.Context(0)
    rng = np.random.default_rng(19)
    N, K, bits, W, R, depth = args.n, args.words, 128, 4, args.members, 100
    expansion = ASMKExpansion(n=R, min_support=args.min_support)
    base = {"device": ctx.device_name(), "date": time.strftime("%Y-%m-%d"), "n": N, "words": K, "bits": bits, "members": R,
            "min_support": args.min_support, "steps": args.steps, "warmup": args.warmup}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(case, **fields):
        rec = dict(base, case=case, **fields)
        print(json.dumps(rec), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")

    # ---- the file: image-major entries in slots, inverted on the device; weights and gammas as ASMKIndex.build makes them
    keys = np.unique(rng.integers(0, K * N, N * args.entries, dtype=np.int64))          # image * K + word: sorted by (image, word)
    E = len(keys)
    words = (keys % K).astype(np.int32)
    counts = np.bincount(keys // K, minlength=N).astype(np.int32)
    del keys
    off = np.zeros(N + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    d_off, d_cnt, d_word, d_sig = ctx.buffer(off.nbytes).upload(off), ctx.buffer(counts.nbytes).upload(counts), ctx.buffer(E * 4).upload(words), \
        ctx.buffer(E * 4 * W)
    step = 1 << 24
    for e0 in range(0, E, step):
        en = min(step, E - e0)
        d_sig.upload(rng.integers(0, 1 << 32, (en, W), dtype=np.uint64).astype(np.uint32), e0 * 4 * W)
    d_woff, d_img, d_osig = ctx.buffer((K + 1) * 8), ctx.buffer(E * 4), ctx.buffer(E * 4 * W)
    ctx.asmk_invert_dev(K, bits, d_off.ptr, off, N, d_cnt.ptr, d_word.ptr, d_sig.ptr, 0, d_woff.ptr, d_img.ptr, d_osig.ptr)
    word_off = d_woff.download((K + 1,), np.int64)
    wt = asmk.word_weights(np.diff(word_off), N, True)
    d_wt, d_sums = ctx.buffer(wt.nbytes).upload(wt), ctx.buffer(N * 8)
    ctx.asmk_weight_sums_dev(K, d_off.ptr, off, N, d_cnt.ptr, d_word.ptr, d_wt.ptr, d_sums.ptr)
    gamma = asmk._gammas_of_sums(d_sums.download((N,), np.int64))
    d_gdb = ctx.buffer(gamma.nbytes).upload(gamma)
    sel = asmk.selectivity(bits)
    d_sel = ctx.buffer(sel.nbytes).upload(sel)
    base.update(entries=int(E), file_bytes=int(E * (4 + 4 * W)))
    print(f"{E} entries, {E * (4 + 4 * W) / 1e9:.2f} GB inverted", flush=True)

    for nq in (1, 64):
        # ---- queries: database images, 8 bits of every signature flipped
        picks = np.sort(rng.choice(N, nq, replace=False))
        q_off = np.zeros(nq + 1, np.int64)
        np.cumsum(counts[picks], out=q_off[1:])
        q_words = np.concatenate([words[off[i]:off[i + 1]] for i in picks])
        q_sigs = np.concatenate([d_sig.download((int(counts[i]), W), np.uint32, int(off[i]) * 4 * W) for i in picks])
        for _ in range(8):
            q_sigs[np.arange(len(q_sigs)), rng.integers(0, W, len(q_sigs))] ^= np.uint32(1) << rng.integers(0, 32, len(q_sigs)).astype(np.uint32)
        gq = asmk.gammas(q_off, q_words, wt)
        d_qw, d_qs, d_gq = ctx.buffer(q_words.nbytes).upload(q_words), ctx.buffer(q_sigs.nbytes).upload(q_sigs), ctx.buffer(gq.nbytes).upload(gq)
        d_panel = ctx.buffer(nq * N * 4)
        d_idx, d_val = ctx.buffer(nq * depth * 8), ctx.buffer(nq * depth * 4)

        def rank(d_w, d_s, h_off, d_g, k):
            ctx.asmk_score_dev(nq, h_off, d_w.ptr, d_s.ptr, bits, K, d_woff.ptr, d_img.ptr, d_osig.ptr, N, d_wt.ptr, d_sel.ptr, d_g.ptr,
                               d_gdb.ptr, d_panel.ptr, N)
            ctx.topk_dev(d_panel.ptr, nq, N, N, k, 0, 0, d_idx.ptr, d_val.ptr)

        first = _timed(ctx, lambda: rank(d_qw, d_qs, q_off, d_gq, R), args.steps, args.warmup, f"first nq={nq}")
        members, votes = expansion.members_of(d_idx.download((nq, R), np.int64))
        d_mem, d_vote = ctx.buffer(members.nbytes).upload(members), ctx.buffer(votes.nbytes).upload(votes)
        cap = max(1, min(K, int(np.diff(q_off).max()) + R * asmk.MAX_ROWS))
        d_xw, d_xs, d_cs = ctx.buffer(nq * cap * 4), ctx.buffer(nq * cap * 4 * W), ctx.buffer(nq * 12)
        got = {}

        def expand():
            d_xw.fill_bytes(asmk.PAD_BYTE)
            ctx.asmk_expand_dev(nq, q_off, d_qw.ptr, d_qs.ptr, bits, K, d_woff.ptr, d_img.ptr, d_osig.ptr, N, R, d_mem.ptr, d_vote.ptr,
                                expansion.query_vote, expansion.resolve_h_max(bits), expansion.min_support, d_wt.ptr, cap, d_xw.ptr,
                                d_xs.ptr, d_cs.ptr + nq * 8, d_cs.ptr)
            raw = d_cs.download((nq * 12,), np.uint8)
            got["sums"], got["counts"] = raw[:nq * 8].view(np.int64).copy(), raw[nq * 8:].view(np.int32).copy()

        exp = _timed(ctx, expand, args.steps, args.warmup, f"expand nq={nq}")
        x_off = np.arange(nq + 1, dtype=np.int64) * cap
        d_xg = ctx.buffer(nq * 4).upload(asmk._gammas_of_sums(got["sums"]))
        second = _timed(ctx, lambda: rank(d_xw, d_xs, x_off, d_xg, depth), args.steps, args.warmup, f"second nq={nq}")
        before, after = np.diff(q_off), got["counts"].astype(np.int64)
        emit("expand", nq=nq, first_ms=first, expand_ms=exp, second_ms=second, cap=int(cap),
             entries_before={"mean": float(before.mean()), "max": int(before.max())},
             entries_after={"mean": float(after.mean()), "max": int(after.max())}, searches=int(K) * int((members >= 0).sum(axis=1).max()))
        for b in (d_qw, d_qs, d_gq, d_panel, d_idx, d_val, d_mem, d_vote, d_xw, d_xs, d_cs, d_xg):
            b.free()
    ctx.close()


if __name__ == "__main__":
    main()
