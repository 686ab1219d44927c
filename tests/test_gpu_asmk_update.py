"""GPU tests of ASMK maintenance (csrc/asmk_update.hip, pvsim.ASMKIndex, pvsim.verify.LocalFeatureIndex): the
four entry points against their NumPy twin (tests/asmk_update_numpy.py), and an index through a sequence of adds and removes against
a from-scratch build of the survivors and against the twin of the index (tests/asmk_numpy.py).  Everything is integers or bit
patterns: np.array_equal throughout."""
import numpy as np
import pytest

import asmk_ma_numpy as mtw
import asmk_numpy as tw
import asmk_update_numpy as up

pytestmark = pytest.mark.gpu

F = np.float32
FILL = 0x5A
FILL32 = np.uint32(0x5A5A5A5A)


def _up(ctx, a):
    a = np.ascontiguousarray(a)
    return ctx.buffer(max(a.nbytes, 16)).upload(a) if a.nbytes else ctx.buffer(16)


def _down(buf, shape, dtype):
    return buf.download(shape, dtype) if int(np.prod(shape)) else np.zeros(shape, dtype)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------ invert and weight sums
def _invert(ctx, off, count, word, sig, K, W, img_base, tile):
    """-> (word_off, out_img, out_sig) as the device leaves them: arrays of `total` slots over a fill pattern"""
    n, total = len(off) - 1, int(off[-1])
    bufs = [_up(ctx, off), _up(ctx, count), _up(ctx, word), _up(ctx, sig), ctx.buffer((K + 1) * 8).fill_bytes(FILL),
            ctx.buffer(max(total, 4) * 4).fill_bytes(FILL), ctx.buffer(max(total, 4) * 4 * W).fill_bytes(FILL)]
    d_off, d_cnt, d_word, d_sig, d_woff, d_img, d_osig = bufs
    try:
        ctx.asmk_invert_dev(K, 32 * W, d_off.ptr, off, n, d_cnt.ptr, d_word.ptr, d_sig.ptr, img_base, d_woff.ptr, d_img.ptr, d_osig.ptr, tile)
        return d_woff.download((K + 1,), np.int64), _down(d_img, (total,), np.int32), _down(d_osig, (total, W), np.uint32)
    finally:
        for b in bufs:
            b.free()


def _weight_sums(ctx, off, count, word, wt):
    n = len(off) - 1
    bufs = [_up(ctx, off), _up(ctx, count), _up(ctx, word), _up(ctx, wt), ctx.buffer(max(n, 2) * 8).fill_bytes(FILL)]
    try:
        ctx.asmk_weight_sums_dev(len(wt), bufs[0].ptr, off, n, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr)
        return _down(bufs[4], (n,), np.int64)
    finally:
        for b in bufs:
            b.free()


INVERT_CASES = [  # n, E, K, W, flavor, img_base
    (0, 0, 5, 1, "random", 0), (1, 0, 5, 2, "random", 0), (1, 1, 1, 1, "random", 1000), (3, 1, 2, 3, "random", 0),
    (3, 255, 255, 4, "random", 0), (3, 256, 256, 2, "bad", 1000), (3, 257, 257, 1, "random", 0), (40, 0, 7, 4, "random", 0),
    (40, 36, 1, 3, "random", 1000), (40, 72, 2, 2, "random", 0), (40, 1000, 256, 3, "bad", 0), (40, 1000, 257, 1, "shared", 1000),
    (40, 1000, 1000, 4, "shared", 0), (40, 1000, 65536, 4, "distinct", 1000), (40, 1000, 65536, 2, "bad", 0),
    # the digit counts of a pass over tiles of 256 are more than one scan block of 2048, and more than 256 of them
    (40, 2000, 65536, 2, "random", 0), (40, 523000, 65536, 1, "random", 1000)]
SCAN_BLOCK = 2048                                                                 # counts one workgroup of the int32 scan takes


@pytest.mark.parametrize("n,E,K,W,flavor,img_base", INVERT_CASES)
def test_invert_and_weight_sums_match_the_twin(gpu_ctx, n, E, K, W, flavor, img_base):
    rng = np.random.RandomState(1900 + n + E + K + W)
    off, count, word, sig, ents = up.make_slots(rng, n, E, K, W, flavor)
    total = int(off[-1])
    want = up.invert(off, count, word, sig, K, img_base, 256)
    assert int(want[0][K]) == E == sum(len(e[0]) for e in ents)                  # the test's own input
    if n == 40 and E == 1000:
        assert total > 3 * 256                                                    # lists cross at least three tiles of 256
    if K == 65536:
        assert want[0][1] >= 1 and want[0][K] - want[0][K - 1] >= 1              # words 0 and 65535 are held
    ncounts = 257 * -(-total // 256)                                              # digit counts of a pass at tile 256
    if E == 2000:
        assert SCAN_BLOCK < ncounts <= 2 * SCAN_BLOCK                             # two scan blocks: a non-zero partial is applied
    if E == 523000:
        assert ncounts > 256 * SCAN_BLOCK                                         # 257 scan blocks: the partials carry between two rounds
    for tile in (256, 512, 0):
        word_off, img, osig = _invert(gpu_ctx, off, count, word, sig, K, W, img_base, tile)
        assert np.array_equal(word_off, want[0]), tile
        assert np.array_equal(img[:E], want[1]) and np.array_equal(osig[:E], want[2]), tile
        assert (img[E:].view(np.uint32) == FILL32).all() and (osig[E:] == FILL32).all(), tile   # nothing is written beyond E
    if flavor == "shared":
        assert np.array_equal(want[1][want[0][K - 1]:], img_base + np.array([i for i, e in enumerate(ents) if len(e[0])]))
    wt = rng.randint(0, 1024, K).astype(np.int32)
    assert np.array_equal(_weight_sums(gpu_ctx, off, count, word, wt), up.weight_sums(off, count, word, wt))


def test_weight_sum_beyond_2_to_32(gpu_ctx):
    """4200 entries of weight 1023 in one image: 4200 * 1023 * 1023 > 2^32; more than a wave's round of entries, and an empty image"""
    K = 65536
    off = np.array([0, 3, 3, 4300, 4302], np.int64)
    count = np.array([2, 0, 4200, 2], np.int32)
    word = np.full(4302, -1, np.int32)
    word[0:2], word[3:4203], word[4300:4302] = [5, 9], np.arange(100, 4300), [-1, K]
    wt = np.full(K, 1023, np.int32)
    got = _weight_sums(gpu_ctx, off, count, word, wt)
    assert got.tolist() == [2 * 1023 * 1023, 0, 4200 * 1023 * 1023, 0] and got[2] > 1 << 32
    assert np.array_equal(got, up.weight_sums(off, count, word, wt))


def test_invert_refuses_bad_arguments(gpu_ctx):
    off, count, word, sig, _ = up.make_slots(np.random.RandomState(1), 3, 12, 9, 4, "random")
    for K, W, base, tile in ((0, 4, 0, 0), (65537, 4, 0, 0), (9, 5, 0, 0), (9, 4, -1, 0), (9, 4, (1 << 31) - 2, 0), (9, 4, 0, -256)):
        with pytest.raises(ValueError):
            _invert(gpu_ctx, off, count, word, sig, K, W, base, tile)
    with pytest.raises(ValueError):
        _invert(gpu_ctx, off[::-1].copy(), count, word, sig, 9, 4, 0, 0)


# ------------------------------------------------------------------------------------------------ insert and remove
class _File:
    """an inverted file on the device"""

    def __init__(self, ctx, arrays, cap=None):
        self.ctx, (self.off, img, sig) = ctx, arrays
        self.W, self.E = sig.shape[1], len(img)
        cap = self.E if cap is None else cap
        self.d_off = _up(ctx, self.off)
        self.d_img, self.d_sig = ctx.buffer(max(cap, 4) * 4).fill_bytes(FILL), ctx.buffer(max(cap, 4) * 4 * self.W).fill_bytes(FILL)
        if self.E:
            self.d_img.upload(img)
            self.d_sig.upload(sig)

    def read(self, E):
        return (self.d_off.download((len(self.off),), np.int64), _down(self.d_img, (E,), np.int32),
                _down(self.d_sig, (E, self.W), np.uint32))

    def free(self):
        for b in (self.d_off, self.d_img, self.d_sig):
            b.free()


def _entry_file(ents, K, W, img_base=0):
    """the inverted file of per-image entries by the twin's own route: the slots hold exactly the entries"""
    off = np.zeros(len(ents) + 1, np.int64)
    np.cumsum([len(e[0]) for e in ents], out=off[1:])
    word = np.concatenate([e[0] for e in ents]).astype(np.int32) if ents else np.zeros(0, np.int32)
    sig = np.concatenate([e[1] for e in ents]).astype(np.uint32) if ents else np.zeros((0, W), np.uint32)
    return up.invert(off, np.diff(off).astype(np.int32), word, sig, K, img_base)


def _list_states(ents, split):
    """thin the words so that every state occurs: word % 4 == 1 only in new images, == 2 only in old ones, == 3 nowhere, == 0 in both"""
    out = []
    for i, (w, s) in enumerate(ents):
        ok = (w % 4 != (1 if i < split else 2)) & (w % 4 != 3)
        out.append((w[ok], s[ok]))
    return out


@pytest.mark.parametrize("K", [1, 7, 300])
@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_insert_and_remove_match_the_twin_and_a_rebuild(gpu_ctx, K, W):
    rng = np.random.RandomState(1950 + K + W)
    N, split = 23, 15
    ents = up.make_slots(rng, N, min(N * K, 400), K, W, "random")[4]
    ents[4] = (np.zeros(0, np.int32), np.zeros((0, W), np.uint32))
    if K == 300:
        ents = _list_states(ents, split)
    old, new, whole = _entry_file(ents[:split], K, W), _entry_file(ents[split:], K, W, split), _entry_file(ents, K, W)
    if K == 300:
        lo, ln = np.diff(old[0]), np.diff(new[0])
        assert ((lo == 0) & (ln > 0)).any() and ((lo > 0) & (ln == 0)).any() and ((lo > 0) & (ln > 0)).any() and ((lo == 0) & (ln == 0)).any()
    empty = _entry_file([], K, W)
    ctx = gpu_ctx
    for a, b in ((old, new), (empty, whole), (whole, empty), (empty, empty)):
        want = up.insert(*a, *b)
        if a is old:
            assert _same(want, whole)                                             # the twin's merge is the from-scratch file
        fa, fb = _File(ctx, a), _File(ctx, b)
        out = _File(ctx, (np.zeros(K + 1, np.int64), np.zeros(0, np.int32), np.zeros((0, W), np.uint32)), cap=len(want[1]) + 3)
        try:
            ctx.asmk_insert_dev(K, 32 * W, fa.d_off.ptr, a[0], fa.d_img.ptr, fa.d_sig.ptr, fb.d_off.ptr, b[0], fb.d_img.ptr, fb.d_sig.ptr,
                                out.d_off.ptr, out.d_img.ptr, out.d_sig.ptr)
            assert _same(out.read(len(want[1])), want)
            tail = out.d_img.download((len(want[1]) + 3,), np.int32)[len(want[1]):]
            assert (tail.view(np.uint32) == FILL32).all()
        finally:
            for f in (fa, fb, out):
                f.free()
    stored = _File(ctx, whole)
    try:
        for gone in ([], list(range(N)), [0], [N - 1], list(range(0, N, 2)), [3, 4, 11]):
            keep = np.ones(N, np.uint8)
            keep[gone] = 0
            pos = up.keep_positions(keep)
            want = up.remove(*whole, keep, pos)
            assert _same(want, _entry_file([e for i, e in enumerate(ents) if keep[i]], K, W)), gone
            out = _File(ctx, (np.zeros(K + 1, np.int64), np.zeros(0, np.int32), np.zeros((0, W), np.uint32)), cap=stored.E)
            d_keep, d_pos = _up(ctx, keep), ctx.buffer((N + 1) * 8)
            try:
                ctx.keep_positions_dev(d_keep.ptr, N, d_pos.ptr)
                ctx.asmk_remove_dev(K, 32 * W, N, stored.d_off.ptr, whole[0], stored.d_img.ptr, stored.d_sig.ptr, d_keep.ptr, d_pos.ptr,
                                    out.d_off.ptr, out.d_img.ptr, out.d_sig.ptr)
                assert _same(out.read(len(want[1])), want), gone
            finally:
                for b in (d_keep, d_pos):
                    b.free()
                out.free()
    finally:
        stored.free()


@pytest.mark.parametrize("E", [2048, 524288])
def test_remove_across_scan_blocks(gpu_ctx, E):
    """E + 1 survivor flags are 2 and 257 blocks of the int32 scan: a non-zero partial is applied, and the scan of the partials
    carries from its first round of 256 into a second.  Every word stores a sorted random subset of the images; 1000 are removed."""
    K, W, N = 300, 1, 4096
    assert -(-(E + 1) // SCAN_BLOCK) == (2 if E == 2048 else 257)                 # the test's own input
    rng = np.random.RandomState(1960 + E % 1000)
    sizes = np.full(K, E // K) + (np.arange(K) < E % K)
    assert sizes.sum() == E and sizes.max() <= N
    word_off = np.zeros(K + 1, np.int64)
    np.cumsum(sizes, out=word_off[1:])
    img = np.concatenate([np.sort(rng.permutation(N)[:c]) for c in sizes]).astype(np.int32)
    sig = rng.randint(0, 1 << 32, (E, W), dtype=np.uint64).astype(np.uint32)
    keep = np.ones(N, np.uint8)
    keep[rng.permutation(N)[:1000]] = 0
    pos = up.keep_positions(keep)
    want = up.remove(word_off, img, sig, keep, pos)
    left = keep[img] != 0
    S = int(left.sum())
    assert 0 < S < E and np.array_equal(want[1], pos[img[left]]) and np.array_equal(want[2], sig[left])
    assert np.array_equal(want[0], np.concatenate([[0], np.cumsum(left)])[word_off])
    stored = _File(gpu_ctx, (word_off, img, sig))
    out = _File(gpu_ctx, (np.zeros(K + 1, np.int64), np.zeros(0, np.int32), np.zeros((0, W), np.uint32)), cap=E)
    d_keep, d_pos = _up(gpu_ctx, keep), _up(gpu_ctx, pos)
    try:
        gpu_ctx.asmk_remove_dev(K, 32 * W, N, stored.d_off.ptr, word_off, stored.d_img.ptr, stored.d_sig.ptr, d_keep.ptr, d_pos.ptr,
                                out.d_off.ptr, out.d_img.ptr, out.d_sig.ptr)
        got_off, got_img, got_sig = out.read(E)
        assert _same((got_off, got_img[:S], got_sig[:S]), want)
        assert (got_img[S:].view(np.uint32) == FILL32).all() and (got_sig[S:] == FILL32).all()   # nothing is written beyond the survivors
    finally:
        for f in (stored, out, d_keep, d_pos):
            f.free()


def test_overlapping_buffers_are_refused(gpu_ctx):
    K, W, N = 7, 2, 6
    ents = up.make_slots(np.random.RandomState(2), N, 20, K, W, "random")[4]
    a, b = _entry_file(ents[:4], K, W), _entry_file(ents[4:], K, W, 4)
    fa, fb = _File(gpu_ctx, a, cap=40), _File(gpu_ctx, b, cap=40)
    out = _File(gpu_ctx, (np.zeros(K + 1, np.int64), np.zeros(0, np.int32), np.zeros((0, W), np.uint32)), cap=40)
    d_keep, d_pos = _up(gpu_ctx, np.ones(N, np.uint8)), _up(gpu_ctx, np.arange(N + 1, dtype=np.int64))
    try:
        def ins(o_off, o_img, o_sig):
            gpu_ctx.asmk_insert_dev(K, 32 * W, fa.d_off.ptr, a[0], fa.d_img.ptr, fa.d_sig.ptr, fb.d_off.ptr, b[0], fb.d_img.ptr, fb.d_sig.ptr,
                                    o_off, o_img, o_sig)

        def rem(o_off, o_img, o_sig):
            gpu_ctx.asmk_remove_dev(K, 32 * W, N, fa.d_off.ptr, a[0], fa.d_img.ptr, fa.d_sig.ptr, d_keep.ptr, d_pos.ptr, o_off, o_img, o_sig)

        ins(out.d_off.ptr, out.d_img.ptr, out.d_sig.ptr)
        rem(out.d_off.ptr, out.d_img.ptr, out.d_sig.ptr)
        for call in (ins, rem):
            for args in ((fa.d_off.ptr, out.d_img.ptr, out.d_sig.ptr), (out.d_off.ptr, fa.d_img.ptr, out.d_sig.ptr),
                         (out.d_off.ptr, out.d_img.ptr, fa.d_sig.ptr), (out.d_off.ptr, fa.d_img.ptr + 8, out.d_sig.ptr),
                         (out.d_off.ptr, out.d_img.ptr, out.d_img.ptr)):
                with pytest.raises(ValueError, match="overlap"):
                    call(*args)
        with pytest.raises(ValueError, match="overlap"):
            ins(out.d_off.ptr, fb.d_img.ptr, out.d_sig.ptr)
    finally:
        for f in (fa, fb, out, d_keep, d_pos):
            f.free()


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def tiny():
    """fifteen tiny images of uint8 rows around 30 prototypes, as the fixture of test_gpu_asmk.py builds them, with frames and queries"""
    rng = np.random.RandomState(1850)
    K = 30
    proto = rng.randint(0, 80, (K, 128)).astype(np.uint8)
    cent = tw.rootsift(proto)

    def rows(words):
        return np.clip(proto[words].astype(np.int64) + rng.randint(-2, 3, (len(words), 128)), 0, 255).astype(np.uint8)

    sizes = [4, 1, 7, 25, 40, 3, 12, 30, 18, 0, 22, 5, 9, 14, 6]
    images = [rows(rng.randint(0, K, n)) for n in sizes]
    queries = [images[4][::2].copy(), np.concatenate([images[7][:15], rows(rng.randint(0, K, 6))]), np.zeros((0, 128), np.uint8)]
    frames = [rng.uniform(0, 100, (len(r), 6)).astype(F) for r in images]
    for x in [tw.rootsift(r) for r in images + queries]:
        assert tw.labels_and_gap(x, cent)[1] > 1e-3
    return cent, images, frames, queries


def _arrays(index):
    return index.word_off, index.ent_img, index.ent_sig, _bits(index.gamma_db)


def _twin_gamma(db, wt):
    return _bits(np.array([tw.gamma(x[0], wt) for x in db], F))


@pytest.mark.parametrize("bits,projection", [(128, None), (64, "random")])
def test_index_through_adds_and_removes_equals_a_rebuild(gpu_ctx, tiny, bits, projection, tmp_path):
    from pvsim import ASMKIndex
    from pvsim.verify import LocalFeatureIndex
    cent, images, frames, queries = tiny
    K, names = len(cent), [f"im{i}" for i in range(len(images))]
    proj = tw.random_projection(bits, 128, 9) if projection else None
    ents = tw.entries([tw.rootsift(r) for r in images], cent, proj)
    q_values = [tw.rootsift(q) for q in queries]
    q1 = tw.entries(q_values, cent, proj)
    # three words per query row from the header's own float32 values (the list does not lean on a float64 order)
    q3 = [mtw.image_entries_ma(x, mtw.topm_chain(x, cent, 3)[0] if len(x) else np.zeros((0, 3), np.int32), cent, proj) for x in q_values]
    kw = dict(bits=bits, projection=projection, random_state=9)

    def local_of(ids):
        return LocalFeatureIndex.from_arrays([images[i] for i in ids], [frames[i] for i in ids], [names[i] for i in ids], ctx=gpu_ctx)

    def hold(index, local, ids):
        """every array and ranking of `index` against a from-scratch build of the images `ids` and against the twin"""
        db = [ents[i] for i in ids]
        assert index.paths == [names[i] for i in ids] == local.paths and len(index) == len(ids)
        want = (*tw.invert(db, K), _twin_gamma(db, index.wt)) if ids else (np.zeros(K + 1, np.int64), np.zeros(0, np.int32),
                                                                            np.zeros((0, bits // 32), np.uint32), np.zeros(0, np.uint32))
        assert _same(_arrays(index), want)
        assert np.array_equal(index.list_sizes(), np.diff(want[0]))
        with local_of(ids) as fresh_local, ASMKIndex.build(fresh_local, cent, weights=index.wt, **kw) as fresh:
            assert fresh.frozen and _same(_arrays(fresh), want) and np.array_equal(fresh.wt, index.wt)
            # LocalFeatureIndex.add / remove against from_arrays of the survivors
            total = fresh_local.total_rows
            assert np.array_equal(local.offsets, fresh_local.offsets) and local.total_rows == total
            if total:
                assert np.array_equal(local.rows.download((total, 128), np.uint8), fresh_local.rows.download((total, 128), np.uint8))
                assert np.array_equal(_bits(local.host_frames()), _bits(fresh_local.host_frames()))
            for ma, qe in ((1, q1), (3, q3)):
                got = index.rank_rows(queries, 5, ma=ma)
                ref = fresh.rank_rows(queries, 5, ma=ma)
                assert np.array_equal(got[0], ref[0]) and np.array_equal(_bits(got[1]), _bits(ref[1]))
                if ids:
                    kk = min(5, len(ids))
                    ridx, rval = tw.rank(tw.scores(qe, db, index.wt, index.sel), kk)
                    assert np.array_equal(got[0][:, :kk], ridx) and np.array_equal(_bits(got[1][:, :kk]), _bits(rval))

    first = list(range(8))
    local = local_of(first)
    try:
        host = ASMKIndex.build(local, cent, **kw)
        index = ASMKIndex.build(local, cent, on_device=True, **kw)
        try:
            # the device route equals the host route, array for array
            assert _same(_arrays(index), _arrays(host)) and np.array_equal(index.wt, host.wt) and np.array_equal(index.sel, host.sel)
            assert index.paths == host.paths and not index.frozen
            a, b = index.rank_rows(queries, 5), host.rank_rows(queries, 5)
            assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
            with pytest.raises(NotImplementedError, match="rebuild"):
                index.add(local)
            wt = index.wt.copy()
            assert index.freeze() is index and np.array_equal(index.wt, wt)
            hold(index, local, first)
            assert np.array_equal(tw.word_weights([ents[i] for i in first], K), wt)

            with local_of([8, 9, 10, 11]) as more:                          # image 9 has no rows
                with pytest.raises(ValueError):
                    index.add(["new", "im3"], [images[3], images[3]])      # a present path: nothing changes
                local.add(more)
                index.add(more)
            ids = first + [8, 9, 10, 11]
            hold(index, local, ids)

            gone = [0, 5, 11]                                                # scattered, the first and the last among them
            local.remove([names[i] for i in gone])
            index.remove([names[i] for i in gone])
            ids = [i for i in ids if i not in gone]
            hold(index, local, ids)

            E = int(index.word_off[-1])
            index.reserve(E + 2)                                             # the next batch does not fit: the buffers grow
            assert len(ents[12][0]) + len(ents[13][0]) > 2
            local.add(names[12:14], images[12:14], frames[12:14])
            index.add(names[12:14], images[12:14])
            ids = ids + [12, 13]
            hold(index, local, ids)

            del index["im4"]
            local.remove(["im4"])
            ids.remove(4)
            hold(index, local, ids)
            assert np.array_equal(index.wt, wt)

            p = str(tmp_path / "updated.npz")
            index.save(p)
            with np.load(p, allow_pickle=False) as z:                        # arrays sized E and N, not capacity
                assert z["ent_img"].shape == (int(index.word_off[-1]),) and z["gamma_db"].shape == (len(ids),)
            back = ASMKIndex.load(p, ctx=gpu_ctx)
            try:
                assert back.frozen and _same(_arrays(back), _arrays(index))
                back.add([names[14]], [images[14]])
                local.add([names[14]], [images[14]], [frames[14]])
                hold(back, local, ids + [14])
                back.remove(back.paths)                                      # removing everything leaves a valid empty index
                local.remove(local.paths)
                hold(back, local, [])
                back.add([names[2], names[9]], [images[2], images[9]])       # and adding to an empty index works
                local.add([names[2], names[9]], [images[2], images[9]], [frames[2], frames[9]])
                hold(back, local, [2, 9])
            finally:
                back.close()
        finally:
            index.close()
            host.close()
    finally:
        local.close()


def test_rerank_spatial_follows_the_updated_pair(gpu_ctx, tiny):
    """the documented pattern local.add(new); asmk.add(new): the shortlist of the updated ASMK index names images the updated
    LocalFeatureIndex holds, so rerank_spatial verifies all of them; a removed image is in neither"""
    import dsift_numpy as dtw
    from pvsim import ASMKIndex
    from pvsim.eval import rerank_spatial
    from pvsim.features import KeypointSIFT
    from pvsim.verify import LocalFeatureIndex, SpatialVerifier
    cent, images, frames, queries = tiny
    names = [f"im{i}" for i in range(len(images))]
    query_image = np.clip(np.floor(dtw.texture(160, 200, 31, channels=1) + 0.5), 0, 255).astype(np.uint8)
    local = LocalFeatureIndex.from_arrays(images[:6], frames[:6], names[:6], ctx=gpu_ctx)
    index = ASMKIndex.build(local, cent, on_device=True).freeze()
    try:
        with LocalFeatureIndex.from_arrays(images[6:9], frames[6:9], names[6:9], ctx=gpu_ctx) as new:
            local.add(new)
            index.add(new)
        local.remove(["im4"])
        index.remove(["im4"])
        idx, val = index.rank_rows([images[7][:15]], 8)
        hits = [(index.paths[int(i)], float(v)) for i, v in zip(idx[0], val[0]) if i >= 0]
        assert hits[0][0] == "im7" and len(hits) == 8 and "im4" not in [h[0] for h in hits]
        ranked = rerank_spatial(query_image, hits, local, SpatialVerifier(extractor=KeypointSIFT(ctx=gpu_ctx), ctx=gpu_ctx))
        assert sorted(r[0] for r in ranked) == sorted(h[0] for h in hits) and all(len(r) == 3 for r in ranked)
        with pytest.raises(KeyError):
            rerank_spatial(query_image, [("im4", 1.0)], local, SpatialVerifier(extractor=KeypointSIFT(ctx=gpu_ctx), ctx=gpu_ctx))
    finally:
        index.close()
        local.close()
