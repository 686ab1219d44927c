"""pvsim.distributed.DevicePool under ShardedVLADIndex, pool logic only: a fake context hands out address ranges and runs nothing, a
stub communicator's collectives do nothing.  Repeated encode -> exchange -> topk and encode -> search cycles must never leave two
live arrays on the same bytes: a block that release_all() took back may be handed out again, and a handle of the earlier hand-out
must not be able to free it a second time."""
import numpy as np
import pytest

from pvsim import distributed as pd


class _FakeBuffer:
    def __init__(self, ptr, nbytes):
        self.ptr, self.nbytes, self.freed = ptr, nbytes, False

    def free(self):
        self.freed = True


class _FakeContext:
    """buffer() hands out disjoint address ranges; every device operation the index queues is a no-op."""
    handle = None

    def __init__(self):
        self._next, self.buffers = 1 << 20, []

    def buffer(self, nbytes):
        b = _FakeBuffer(self._next, int(nbytes))
        self._next += (int(nbytes) + 255) // 256 * 256
        self.buffers.append(b)
        return b

    def fill_dev(self, *a, **k):
        pass

    def vlad_encode_dev(self, *a, **k):
        pass

    def cosine_topk_dev(self, *a, **k):
        pass

    def topk_merge_dev(self, *a, **k):
        pass

    def sync(self):
        pass


class _FakeCodebook:
    K, D = 16, 8


class _StubComm:
    def __init__(self, ctx, world, rank=0):
        self.ctx, self.world, self.rank = ctx, world, rank

    def all_gather(self, send, recv, nbytes=None):
        pass

    def all_to_all(self, out, inp, nbytes_per_rank=None):
        pass


@pytest.fixture(autouse=True)
def _no_downloads(monkeypatch):
    monkeypatch.setattr(pd.DevArray, "numpy", lambda self: np.zeros(self.shape, dtype=self.dtype))


def _live(index, extra=()):
    named = [("enc_loc", getattr(index, "enc_loc", None)), ("inv_loc", getattr(index, "inv_loc", None)),
             ("enc_all", getattr(index, "enc_all", None)), ("inv_all", getattr(index, "inv_all", None))]
    named += [(f"lists[{i}]", a) for i, a in enumerate(getattr(index, "_lists", ()))]
    named += [(f"search_bufs[{i}]", a) for i, a in enumerate(getattr(index, "_search_bufs", ()))]
    named += list(extra)
    seen, out = set(), []
    for name, a in named:                       # at world 1 enc_all IS enc_loc: one array under two names
        if a is not None and id(a) not in seen:
            seen.add(id(a))
            out.append((name, a))
    return out


def _assert_disjoint(index, where, extra=()):
    live = sorted(_live(index, extra), key=lambda na: na[1].ptr)
    for (na, a), (nb, b) in zip(live, live[1:]):
        assert a.ptr + max(a.nbytes, 1) <= b.ptr, f"{where}: {na} [{a.ptr:#x}, +{a.nbytes}) and {nb} [{b.ptr:#x}, +{b.nbytes}) share memory"


def _index(world, n_total):
    ctx = _FakeContext()
    comm = _StubComm(ctx, world) if world > 1 else None
    return ctx, pd.ShardedVLADIndex(ctx, _FakeCodebook(), n_total, comm=comm)


WORLDS = {1: (5, 37, 1000), 8: (1000000,)}          # world -> corpus sizes; 10^6 images on 8 ranks: blocks of 125000


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("world", [1, 8])
def test_repeated_topk_cycles_keep_live_arrays_apart(world, k):
    for n in WORLDS[world]:
        ctx, index = _index(world, n)
        assert world == 1 or index.block == 125000
        for cycle in range(1, 4):
            where = f"world {world}, n {n}, k {k}, cycle {cycle}"
            index.encode_local(0, 0, 0, 0)
            _assert_disjoint(index, where + " after encode")
            index.exchange()
            _assert_disjoint(index, where + " after exchange")
            index.topk(k)
            _assert_disjoint(index, where + " after topk")
        index.pool.close()
        assert all(b.freed for b in ctx.buffers)


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("world", [1, 8])
def test_repeated_search_cycles_keep_live_arrays_apart(world, k):
    for n in WORLDS[world]:
        ctx, index = _index(world, n)
        n_loc = index.hi - index.lo
        queries = pd.DevicePool(ctx)                                     # the caller's arrays: not the index's to recycle
        q = queries.empty((n_loc, _FakeCodebook.K * _FakeCodebook.D), "float32")
        inv_q = queries.empty((n_loc,), "float32")
        extra = (("q", q), ("inv_q", inv_q))
        for cycle in range(1, 4):
            where = f"world {world}, n {n}, k {k}, cycle {cycle}"
            index.encode_local(0, 0, 0, 0)
            _assert_disjoint(index, where + " after encode", extra)
            index.search(q, inv_q, k)
            _assert_disjoint(index, where + " after search", extra)
            index.search(q, inv_q, k)                                    # a second query of the same cycle releases the first one's buffers
            _assert_disjoint(index, where + " after the second search", extra)
        index.pool.close()


@pytest.mark.parametrize("world", [1, 8])
def test_mixed_cycles_keep_live_arrays_apart(world):
    """topk and search on one index, k changing between cycles: the lists of one kind must not survive into a cycle of the other."""
    n = WORLDS[world][-1]
    ctx, index = _index(world, n)
    n_loc = index.hi - index.lo
    queries = pd.DevicePool(ctx)
    q, inv_q = queries.empty((n_loc, 128), "float32"), queries.empty((n_loc,), "float32")
    extra = (("q", q), ("inv_q", inv_q))
    for cycle, k in enumerate((1, 4, 1, 4, 1), 1):
        where = f"world {world}, k {k}, cycle {cycle}"
        index.encode_local(0, 0, 0, 0)
        index.exchange()
        index.topk(k)
        _assert_disjoint(index, where + " after topk", extra)
        index.encode_local(0, 0, 0, 0)
        _assert_disjoint(index, where + " after the second encode", extra)
        index.search(q, inv_q, k)
        _assert_disjoint(index, where + " after search", extra)


def test_encode_drops_every_handle_of_the_previous_cycle():
    for world in (1, 8):
        ctx, index = _index(world, WORLDS[world][-1])
        index.encode_local(0, 0, 0, 0)
        index.exchange()
        index.topk(4)
        q, inv_q = pd.DevicePool(ctx).empty((3, 128), "float32"), pd.DevicePool(ctx).empty((3,), "float32")
        index.search(q, inv_q, 4)
        assert index._lists and index._search_bufs
        index.encode_local(0, 0, 0, 0)
        assert index._lists == () and index._search_bufs == () and index.enc_all is None and index.inv_all is None
        assert len(index.pool._used) == 2                                # enc_loc and inv_loc


def test_release_ignores_a_handle_of_an_earlier_hand_out():
    pool = pd.DevicePool(_FakeContext())
    a = pool.empty((100,), "float32")
    pool.release_all()
    b = pool.empty((100,), "float32")
    assert b.ptr == a.ptr                                # the same block, handed out again
    pool.release(a)                                      # the earlier hand-out's handle: must not free b's block
    c = pool.empty((100,), "float32")
    assert c.ptr != b.ptr and len(pool._used) == 2
    pool.release(b)
    pool.release(b)                                      # released twice: the second is a no-op
    d = pool.empty((100,), "float32")
    e = pool.empty((100,), "float32")
    assert d.ptr == b.ptr and e.ptr not in (c.ptr, d.ptr)
    pool.release(c[10:])                                 # a view is not the array
    assert len(pool._used) == 3
