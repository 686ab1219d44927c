"""GPU tests of graph maintenance after add / remove (csrc/diffuse.hip, pvsim/diffusion.py).  Kernel level: each
new entry point against its NumPy twin (tests/diffusion_update_numpy.py), bit for bit, outputs followed by guard bytes.  End to end: after
every step of a sequence of adds and removes through a mutable graph, nbr, sim and s equal those of `Diffusion.build` on the same updated
index AND on a DeviceIndex made from the surviving rows, and `rank` returns the rebuilt graph's bits.  There is no tolerance anywhere."""
import numpy as np
import pytest

import diffusion_update_numpy as up
import topk_numpy as tk

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0x5A
N_G, L_G = 300, 32               # the small_index recipe of tests/test_gpu_diffusion.py
BLOCK = 128                      # block seams at 128 and 256


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _up(ctx, a):
    a = np.ascontiguousarray(a)
    return ctx.buffer(max(a.nbytes, 16)).upload(a)


def _out(ctx, nbytes):
    """an output buffer full of 0x5A with GUARD bytes behind it"""
    return ctx.buffer(nbytes + GUARD).fill_bytes(FILL)


def _guard_intact(buf, nbytes):
    return bool((buf.download((GUARD,), np.uint8, offset=nbytes) == FILL).all())


def _filled(shape, dtype):
    """what an untouched output of _out downloads as"""
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, FILL, np.uint8).view(dtype).reshape(shape)


def _awkward_values(rng, shape):
    """float32 similarities of few distinct values (ties), with NaN, -0, +0 and negatives among them"""
    v = (rng.integers(-2, 5, shape) / 4).astype(np.float32)
    dice = rng.random(shape)
    v[dice < 0.06] = np.nan
    v[(dice >= 0.06) & (dice < 0.12)] = -0.0
    return v


KGS = (1, 5, 33)
ROWS = (1, 255, 257)


# ------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("kg", KGS)
def test_lists_kernel_matches_twin(gpu_ctx, kg, rows):
    ctx = gpu_ctx
    rng = np.random.default_rng(1000 * kg + rows)
    N = max(rows + 3, kg + 2)
    idx = rng.integers(-1, N + 1, (rows, kg + 1)).astype(np.int64)          # -1 and N: outside [0, N)
    val = _awkward_values(rng, (rows, kg + 1))
    d_idx, d_val = _up(ctx, idx), _up(ctx, val)
    row0 = N - rows - 1
    ids = rng.permutation(N)[:rows].astype(np.int64)
    if rows > 2:
        ids[1], ids[-1] = N + 5, -1                                         # rows that belong nowhere write nothing
    for own, d_ids in ((row0 + np.arange(rows), None), (ids, _up(ctx, ids))):
        li = idx.copy()
        own = np.asarray(own, np.int64)
        hit = rng.random(rows) < 0.7                                        # most rows hold themselves somewhere, some twice
        li[hit, rng.integers(0, kg + 1, rows)[hit]] = own[hit]
        twice = hit & (rng.random(rows) < 0.2)
        li[twice, kg] = own[twice]
        d_idx.upload(li)
        want_nbr, want_sim = _filled((N, kg), np.int32), _filled((N, kg), np.float32)
        up.lists(li, val, own, N, want_nbr, want_sim)
        d_nbr, d_sim = _out(ctx, N * kg * 4), _out(ctx, N * kg * 4)
        ctx.graph_lists_dev(d_idx.ptr, d_val.ptr, rows, kg, row0 if d_ids is None else 0, N, d_nbr.ptr, d_sim.ptr,
                            d_ids=None if d_ids is None else d_ids.ptr)
        assert _same(d_nbr.download((N, kg), np.int32), want_nbr), (kg, rows, d_ids is None)
        assert _same(d_sim.download((N, kg), np.float32), want_sim), (kg, rows, d_ids is None)
        assert _guard_intact(d_nbr, N * kg * 4) and _guard_intact(d_sim, N * kg * 4)
        for b in (d_nbr, d_sim) + (() if d_ids is None else (d_ids,)):
            b.free()
    d_idx.free(), d_val.free()


def _sorted_lists(rng, rows, width, ids_pool, short=False):
    """per row `width` entries in list order: distinct ids drawn from ids_pool, awkward values, ranked by the stated order; with `short`
    every seventh row has one entry fewer (its last slot is idx -1, val -inf); afterwards some +0 become -0, which ties"""
    idx, val = np.empty((rows, width), np.int64), np.empty((rows, width), np.float32)
    for i in range(rows):
        m = width - 1 if short and width > 1 and i % 7 == 3 else width
        idx[i], val[i] = tk.rank_row(rng.choice(ids_pool, m, replace=False), _awkward_values(rng, m), width)
    flip = (val == 0) & (rng.random(val.shape) < 0.5)
    val[flip] = -0.0
    return idx, val


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("kg", KGS)
def test_merge_kernel_matches_twin(gpu_ctx, kg, rows):
    """c in {1, kg - 1, kg}; few distinct scores, so old and new entries tie all the time; NaN, -0 and empty candidate slots"""
    ctx = gpu_ctx
    rng = np.random.default_rng(2000 * kg + rows)
    n_old = max(rows, kg + 1) + 5
    for c in sorted({1, max(1, kg - 1), kg}):
        b = c + 3
        N = n_old + b
        nbr, sim = _sorted_lists(rng, rows, kg, np.arange(n_old))
        cidx, cval = _sorted_lists(rng, rows, c, np.arange(b), short=True)
        nbr = nbr.astype(np.int32)
        want_nbr, want_sim = up.merge(nbr, sim, cidx, cval, n_old, N)
        bufs = [_up(ctx, a) for a in (nbr, sim, cidx, cval)]
        d_on, d_os = _out(ctx, rows * kg * 4), _out(ctx, rows * kg * 4)
        ctx.graph_merge_dev(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, rows, kg, c, n_old, N, d_on.ptr, d_os.ptr)
        got_nbr, got_sim = d_on.download((rows, kg), np.int32), d_os.download((rows, kg), np.float32)
        assert _same(got_nbr, want_nbr) and _same(got_sim, want_sim), (kg, rows, c)
        assert _guard_intact(d_on, rows * kg * 4) and _guard_intact(d_os, rows * kg * 4)
        assert (got_nbr >= n_old).any() or rows == 1                        # candidates do get in
        with pytest.raises(ValueError, match="overlaps"):
            ctx.graph_merge_dev(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, rows, kg, c, n_old, N, bufs[0].ptr, d_os.ptr)
        for buf in bufs + [d_on, d_os]:
            buf.free()


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("kg", KGS)
def test_damage_remap_and_affinity_kernels_match_twin(gpu_ctx, kg, rows):
    ctx = gpu_ctx
    rng = np.random.default_rng(3000 * kg + rows)
    N = max(rows, kg + 1, 2)
    nbr = rng.integers(-1, N + 1, (N, kg)).astype(np.int32)
    keep = (rng.random(N) < 0.9).astype(np.uint8)
    keep[rng.integers(0, N)] = 0
    pos = np.concatenate([[0], np.cumsum(keep != 0)]).astype(np.int64)
    d_nbr, d_keep, d_pos = _up(ctx, nbr), _up(ctx, keep), _up(ctx, pos)
    d_flag, d_out = _out(ctx, N), _out(ctx, N * kg * 4)
    ctx.graph_damage_dev(d_nbr.ptr, N, kg, d_keep.ptr, d_flag.ptr)
    assert _same(d_flag.download((N,), np.uint8), up.damage(nbr, keep)) and _guard_intact(d_flag, N)
    ctx.graph_remap_dev(d_nbr.ptr, N, kg, d_keep.ptr, d_pos.ptr, d_out.ptr)
    assert _same(d_out.download((N, kg), np.int32), up.remap(nbr, keep, pos, out=_filled((N, kg), np.int32)))      # removed rows untouched
    assert _guard_intact(d_out, N * kg * 4)
    ctx.graph_remap_dev(d_nbr.ptr, N, kg, d_keep.ptr, d_pos.ptr, d_nbr.ptr)                                         # in place
    assert _same(d_nbr.download((N, kg), np.int32), up.remap(nbr, keep, pos))
    with pytest.raises(ValueError, match="overlaps"):
        ctx.graph_remap_dev(d_nbr.ptr, N, kg, d_keep.ptr, d_pos.ptr, d_nbr.ptr + 4)
    with pytest.raises(ValueError, match="overlaps"):
        ctx.graph_damage_dev(d_nbr.ptr, N, kg, d_keep.ptr, d_keep.ptr)
    sim = _awkward_values(rng, (N, kg))
    d_sim = _up(ctx, sim)
    for gamma in (0, 1, 3):
        d_a = _out(ctx, N * kg * 8)
        ctx.graph_affinity_sim_dev(d_sim.ptr, N, kg, gamma, d_a.ptr)
        assert _same(d_a.download((N, kg), np.float64), up.affinity_sim(sim, gamma)) and _guard_intact(d_a, N * kg * 8)
        d_a.free()
    with pytest.raises(ValueError, match="gamma"):
        ctx.graph_affinity_sim_dev(d_sim.ptr, N, kg, 9, d_out.ptr)
    for b in (d_nbr, d_keep, d_pos, d_flag, d_out, d_sim):
        b.free()


@pytest.mark.parametrize("L", [1, 32, 34])
@pytest.mark.parametrize("rows", ROWS)
def test_gather_rows_kernel_matches_twin(gpu_ctx, rows, L):
    ctx = gpu_ctx
    rng = np.random.default_rng(4000 + 10 * rows + L)
    n = 300
    X = _awkward_values(rng, (n, L))
    ids = rng.integers(0, n, rows).astype(np.int64)                         # repeats are served
    if rows > 2:
        ids[0], ids[-1] = n, -1
    d_x, d_ids, d_out = _up(ctx, X), _up(ctx, ids), _out(ctx, rows * L * 4)
    ctx.graph_gather_rows_dev(d_x.ptr, n, L * 4, d_ids.ptr, rows, d_out.ptr)
    assert _same(d_out.download((rows, L), np.float32), up.gather_rows(X, ids)) and _guard_intact(d_out, rows * L * 4)
    with pytest.raises(ValueError, match="overlaps"):
        ctx.graph_gather_rows_dev(d_x.ptr, n, L * 4, d_ids.ptr, rows, d_x.ptr)
    with pytest.raises(ValueError, match="multiple of 4"):
        ctx.graph_gather_rows_dev(d_x.ptr, n, L * 4 + 2, d_ids.ptr, rows, d_out.ptr)
    for b in (d_x, d_ids, d_out):
        b.free()


def test_affinity_from_sim_is_the_affinity_of_the_lists(gpu_ctx):
    """the same product, the same bits as pvs_graph_affinity_dev gives for the same float32 values"""
    ctx = gpu_ctx
    rng = np.random.default_rng(77)
    N, kg = 257, 5
    idx = np.stack([rng.permutation(N)[:kg + 1] for _ in range(N)]).astype(np.int64)
    val = rng.uniform(-0.3, 1.0, (N, kg + 1)).astype(np.float32)
    d_idx, d_val = _up(ctx, idx), _up(ctx, val)
    d_nbr, d_sim, d_nbr2 = _out(ctx, N * kg * 4), _out(ctx, N * kg * 4), _out(ctx, N * kg * 4)
    ctx.graph_lists_dev(d_idx.ptr, d_val.ptr, N, kg, 0, N, d_nbr.ptr, d_sim.ptr)
    for gamma in (0, 2, 3, 8):
        d_a, d_a2 = _out(ctx, N * kg * 8), _out(ctx, N * kg * 8)
        ctx.graph_affinity_dev(d_idx.ptr, d_val.ptr, False, N, kg, 0, N, gamma, d_nbr2.ptr, d_a.ptr)
        ctx.graph_affinity_sim_dev(d_sim.ptr, N, kg, gamma, d_a2.ptr)
        assert _same(d_a.download((N, kg), np.float64), d_a2.download((N, kg), np.float64)), gamma
        assert _same(d_nbr.download((N, kg), np.int32), d_nbr2.download((N, kg), np.int32))
        d_a.free(), d_a2.free()
    for b in (d_idx, d_val, d_nbr, d_sim, d_nbr2):
        b.free()


# ------------------------------------------------------------------------------------------------ end to end
def _recipe(n, L, seed=21):
    """the rows of small_index (tests/test_gpu_diffusion.py) for n = 300, L = 32, seed 21: twelve noisy clusters"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((12, L))[rng.integers(0, 12, n)] + 0.8 * rng.standard_normal((n, L))).astype(np.float32)


class Corpus:
    """an index, the mutable graph that follows it, and the dict of the surviving rows beside them; `check` rebuilds and compares"""

    def __init__(self, ctx, rows, kg, gamma, block):
        from pvsim import Diffusion
        from pvsim.index import DeviceIndex
        self.ctx, self.kg, self.gamma, self.block, self.serial = ctx, kg, gamma, block, 0
        self.live = {}
        self.live.update(self._named(rows))
        self.index = DeviceIndex(dict(self.live), ctx)
        self.g = Diffusion.build(self.index, k=kg, gamma=gamma, block=block, mutable=True)
        rng = np.random.default_rng(51)
        self.Q = (rows[rng.integers(0, len(rows), 7)] + 0.3 * rng.standard_normal((7, rows.shape[1]))).astype(np.float32)

    def _named(self, rows):
        out = {f"img{self.serial + i:05d}": r for i, r in enumerate(rows)}
        self.serial += len(rows)
        return out

    def add(self, rows):
        new = self._named(np.asarray(rows, np.float32))
        self.g.add(new)
        self.live.update(new)
        assert self.g.last_update == {"op": "add", "rows": len(new), "reranked": len(new), "n": len(self.live)}

    def remove(self, positions):
        paths = list(self.live)
        gone = [paths[int(p)] for p in positions]
        self.g.remove(gone)
        for p in gone:
            del self.live[p]
        u = self.g.last_update
        assert (u["op"], u["rows"], u["n"]) == ("remove", len(gone), len(self.live)) and 0 <= u["reranked"] <= len(self.live)
        return u["reranked"]

    def in_degree(self):
        nbr = self.g.nbr
        return np.bincount(nbr[nbr >= 0].ravel(), minlength=len(self.live))

    def check(self, what):
        from pvsim import Diffusion
        from pvsim.index import DeviceIndex
        g, n = self.g, len(self.live)
        assert g.n == n == len(self.index) and g._mods == self.index.modifications and g.mutable, what
        fresh = DeviceIndex(dict(self.live), self.ctx)
        same_index = Diffusion.build(self.index, k=self.kg, gamma=self.gamma, block=self.block, mutable=True)
        from_rows = Diffusion.build(fresh, k=self.kg, gamma=self.gamma, block=self.block, mutable=True)
        nbr, sim, s = g.nbr, g.sim, g.s
        for other, name in ((same_index, "the updated index"), (from_rows, "an index of the surviving rows")):
            assert _same(nbr, other.nbr), (what, name, "nbr", np.flatnonzero((nbr != other.nbr).any(axis=1))[:8])
            assert _same(sim, other.sim), (what, name, "sim")
            assert _same(s, other.s), (what, name, "s")
        k, kq = min(10, n), min(5, n)
        got, want = g.rank(self.Q, k=k, kq=kq), same_index.rank(self.Q, k=k, kq=kq)
        assert np.array_equal(got[0], want[0]) and _same(got[1], want[1]), (what, "rank")
        for x in (same_index, from_rows):
            x.close()
        fresh.close()

    def close(self):
        self.g.close()
        self.index.close()


@pytest.mark.parametrize("gamma", [1, 3])
@pytest.mark.parametrize("kg", [5, 33])
def test_graph_follows_adds_and_removes(gpu_ctx, kg, gamma):
    from pvsim import Diffusion
    rows = _recipe(N_G, L_G)
    pool = _recipe(400, L_G, seed=22)                                       # rows to add, from the same clusters' recipe
    c = Corpus(gpu_ctx, rows, kg, gamma, BLOCK)
    c.check("build")
    imm = Diffusion.build(c.index, k=kg, gamma=gamma, block=BLOCK)
    assert _same(imm.nbr, c.g.nbr) and _same(imm.s, c.g.s)                  # mutable or not: the same graph
    imm.close()
    c.add(pool[:1]), c.check("add 1")                                       # 301 rows
    c.add(pool[1:41]), c.check("add 40: b > kg, N odd afterwards")         # 341
    assert len(c.live) % 2 == 1
    c.add(pool[41:44]), c.check("add 3: b < kg")                            # 344
    c.add(pool[44:244]), c.check("add 200")                                 # 544: the new rows span two blocks
    twin = pool[300]
    c.add(np.stack([rows[10], twin, twin])), c.check("duplicates of an old row and of another new row")
    c.add(np.repeat(rows[20:21], kg + 2, axis=0))                           # kg + 3 equal rows: the last copies are not in their own top kg + 1
    c.check("a row pushed out of its own list")
    idx, _ = c.index.rank(rows[20:21], kg + 1)
    assert len(c.live) - 1 not in idx[0]
    c.add(np.zeros((1, L_G), np.float32)), c.check("a zero row")
    deg = c.in_degree()
    assert c.remove([int(deg.argmin())]) == deg.min()                       # exactly the rows that listed it are ranked again
    c.check("remove a leaf")
    deg = c.in_degree()
    hub = int(deg.argmax())
    assert c.remove([hub]) == deg[hub] > kg
    c.check("remove the row of the highest in-degree")
    c.remove([0]), c.check("remove row 0")
    c.remove([len(c.live) - 1]), c.check("remove the last row")
    c.remove(range(120, 136)), c.check("remove a run across the seam at 128")
    c.remove(range(0, len(c.live), 2)), c.check("remove every other row")
    c.remove(range(kg + 1, len(c.live))), c.check("remove down to kg + 1 rows")
    assert len(c.live) == kg + 1
    before = (c.g.nbr, c.g.sim, c.g.s, c.index.modifications)
    with pytest.raises(ValueError, match=f"{kg + 1} rows.*leave {kg}"):     # N' = kg: both numbers named, nothing changed
        c.remove([0])
    assert _same(before[0], c.g.nbr) and _same(before[1], c.g.sim) and _same(before[2], c.g.s) and before[3] == c.index.modifications
    c.add(pool[310:340]), c.check("mixed: add 30")
    c.remove([1, 7, 8, 20, 30]), c.check("mixed: remove 5")
    c.add(pool[340:342]), c.check("mixed: add 2")
    c.close()


def test_rows_of_34_columns_and_an_odd_first_new_row(gpu_ctx):
    """L = 34: a row is 136 bytes, so the sub-range of the new rows starts 8-byte aligned only (first new row 101), the filtered entry
    declines (L % 8 != 0) and every ranking of such rows takes the generic GEMM, whole index or sub-range"""
    rows, pool = _recipe(101, 34, seed=5), _recipe(20, 34, seed=6)
    c = Corpus(gpu_ctx, rows, 5, 3, 64)
    c.add(pool[:3]), c.check("add 3 at row 101")
    assert (c.index._db.ptr + 101 * 34 * 4) % 16 == 8
    c.add(pool[3:4]), c.check("add 1 at row 104")
    c.remove([3, 64, 101]), c.check("remove 3")
    c.add(pool[4:20]), c.check("add 16")
    c.close()


def test_the_filtered_path_ranks_the_old_rows(gpu_ctx):
    """N = 600 with block = 600: the old rows are 600 >= 512 queries in one call against the sub-range of the new rows, so the
    filtered entry ranks them (its statistics say that the filter ran); the build itself ranks 600 x 600 through it too"""
    from pvsim import Diffusion
    rows, pool = _recipe(600, L_G, seed=8), _recipe(64, L_G, seed=9)
    c = Corpus(gpu_ctx, rows, 5, 3, 600)
    c.add(pool[:40])
    st = c.index._last_range_stats
    assert st is not None and st["filtered"], st
    c.check("add 40 by the filtered path")
    plain = Diffusion.build(c.index, k=5, gamma=3, block=128, mutable=True)       # and the plain path's lists are the same
    assert _same(plain.nbr, c.g.nbr) and _same(plain.sim, c.g.sim) and _same(plain.s, c.g.s)
    plain.close()
    c.remove(range(0, 640, 5)), c.check("remove 128")
    c.close()


def test_refusals_change_nothing(gpu_ctx):
    from pvsim import Diffusion
    from pvsim.index import DeviceIndex
    rows = _recipe(40, 16, seed=3)
    named = {f"p{i}": rows[i] for i in range(40)}
    index = DeviceIndex(dict(named), gpu_ctx)
    imm = Diffusion.build(index, k=4)
    g = Diffusion.build(index, k=4, mutable=True)
    assert not imm.mutable and g.mutable
    with pytest.raises(AttributeError, match="mutable"):
        imm.sim

    def state():
        return g.nbr, g.sim, g.s, imm.nbr, imm.s, index.modifications, len(index), g.n, g.last_update

    def unchanged(was):
        now = state()
        return all(_same(a, b) for a, b in zip(was[:5], now[:5])) and was[5:] == now[5:]

    was = state()
    for call in (lambda: imm.add({"new": rows[0]}), lambda: imm.remove(["p3"])):
        with pytest.raises(RuntimeError, match="immutable"):
            call()
    with pytest.raises(ValueError, match="already indexed"):
        g.add({"new": rows[0], "p7": rows[1]})
    with pytest.raises(TypeError, match="float32"):
        g.add({"new": rows[0].astype(np.float64)})
    with pytest.raises(ValueError, match="length"):
        g.add({"new": rows[0][:8]})
    with pytest.raises(KeyError):
        g.remove(["p3", "nobody"])
    with pytest.raises(ValueError, match="twice"):
        g.remove(["p3", "p3"])
    with pytest.raises(ValueError, match="5 rows.*leave 4"):
        g.remove([f"p{i}" for i in range(36)])                 # N' = kg
    assert unchanged(was)
    g.add({}), g.remove([])                                    # nothing to do: nothing moves
    assert unchanged(was)
    index64 = DeviceIndex({p: v.astype(np.float64) for p, v in named.items()}, gpu_ctx)
    with pytest.raises(TypeError, match="float32 index.*split along k"):
        Diffusion.build(index64, k=4, mutable=True)
    assert index64.modifications == 0
    Diffusion.build(index64, k=4).close()                      # the immutable graph of a float64 index is built as ever
    index64.close()
    index.add({"direct": rows[5] * 2})                         # not through the graph: both graphs are stale
    was = state()
    for call in (lambda: g.add({"new": rows[0]}), lambda: g.remove(["p3"]), lambda: g.rank(rows[:2], k=3, kq=2),
                 lambda: imm.rank(rows[:2], k=3, kq=2)):
        with pytest.raises(RuntimeError, match="has changed"):
            call()
    assert unchanged(was)
    for x in (imm, g):
        x.close()
    index.close()


def test_save_load_round_trip_and_add_on_the_loaded_graph(gpu_ctx, tmp_path):
    from pvsim import Diffusion
    from pvsim.index import DeviceIndex
    rows, pool = _recipe(60, 16, seed=61), _recipe(9, 16, seed=62)
    index = DeviceIndex({f"p{i}": rows[i] for i in range(60)}, gpu_ctx)
    g = Diffusion.build(index, k=4, gamma=3, mutable=True)
    imm = Diffusion.build(index, k=4, gamma=3)
    fn, fn_imm = str(tmp_path / "mutable.npz"), str(tmp_path / "immutable.npz")
    g.save(fn), imm.save(fn_imm)
    with np.load(fn_imm, allow_pickle=False) as z:             # an immutable graph's file is what it always was
        assert sorted(z.files) == ["gamma", "index_modifications", "nbr", "s"]
    with np.load(fn, allow_pickle=False) as z:
        assert sorted(z.files) == ["gamma", "index_modifications", "nbr", "s", "sim"] and z["sim"].dtype == np.float32
    h, h_imm = Diffusion.load(fn, index), Diffusion.load(fn_imm, index)
    assert h.mutable and not h_imm.mutable
    assert _same(h.nbr, g.nbr) and _same(h.sim, g.sim) and _same(h.s, g.s) and _same(h_imm.s, g.s)
    h.add({f"q{i}": pool[i] for i in range(9)})
    h.remove(["p0", "q3"])
    want = Diffusion.build(index, k=4, gamma=3, mutable=True)
    assert _same(h.nbr, want.nbr) and _same(h.sim, want.sim) and _same(h.s, want.s) and h.n == 67
    a, b = h.rank(rows[:4], k=5, kq=3), want.rank(rows[:4], k=5, kq=3)
    assert np.array_equal(a[0], b[0]) and _same(a[1], b[1])
    for stale in (g, imm, h_imm):                              # the graph that was not the one updated is a snapshot like any other
        with pytest.raises(RuntimeError, match="has changed"):
            stale.rank(rows[:4], k=5, kq=3)
    with pytest.raises(RuntimeError, match="has changed"):
        Diffusion.load(fn, index)
    h.save(fn)
    again = Diffusion.load(fn, index)
    assert again.mutable and _same(again.sim, h.sim)
    for x in (g, imm, h, h_imm, want, again):
        x.close()
    index.close()


def test_readme_example_runs_as_written(gpu_ctx):
    from pvsim import Diffusion
    from pvsim.index import DeviceIndex
    rows = _recipe(120, 16, seed=90)
    index = DeviceIndex({f"{i}.jpg": rows[i] for i in range(100)}, gpu_ctx)
    g = Diffusion.build(index, k=50, mutable=True)
    g.add({"new1.jpg": rows[100], "new2.jpg": rows[101]})
    g.remove(["3.jpg", "new1.jpg"])
    assert (g.n, len(index)) == (100, 100) and g.last_update["op"] == "remove"
    idx, val = g.rank(rows[110:113], k=10, kq=10)
    assert idx.shape == (3, 10)
    g.close()
    index.close()
