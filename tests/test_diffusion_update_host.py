"""CPU tests of the twin of graph maintenance (tests/diffusion_update_numpy.py): on seeded score matrices of small
integers -- ties everywhere, a few NaN rows and columns, a diagonal that is not the largest of its row -- the lists maintained through
add (merge) and remove (damage / remap / re-rank) equal the lists from scratch exactly, after every step of every sequence."""
import numpy as np
import pytest

import diffusion_update_numpy as up

N0, UNIVERSE = 40, 140
KGS = (1, 5, 39)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.fixture(scope="module")
def universe():
    """scores of 140 images against each other: integers in -2 .. 3 (so most comparisons tie), not symmetric, a diagonal like any other
    entry except where it is set to the row's maximum, NaN in three rows and three columns, a few -0"""
    rng = np.random.default_rng(2024)
    U = rng.integers(-2, 4, (UNIVERSE, UNIVERSE)).astype(np.float32)
    top = rng.random(UNIVERSE) < 0.7
    U[top, top] = 3.0                                    # most images rank themselves first (among ties, by index)
    U[U == 0] = np.where(rng.random((U == 0).sum()) < 0.3, np.float32(-0.0), np.float32(0.0))
    for i in (7, 44, 101):
        U[i, :] = np.nan
    for j in (3, 58, 120):
        U[:, j] = np.nan
    U.setflags(write=False)
    return U


class Maintained:
    """lists kept through adds and removes of universe images, beside the live ids"""

    def __init__(self, U, kg, live):
        self.U, self.kg, self.live = U, kg, list(live)
        self.nbr, self.sim = up.lists_from_scratch(self.scores(), kg)
        self.reranked = None

    def scores(self, live=None):
        live = self.live if live is None else live
        return self.U[np.ix_(live, live)]

    def add(self, new):
        self.live += list(new)
        self.nbr, self.sim = up.add_by_merge(self.nbr, self.sim, self.scores(), self.kg)

    def remove(self, positions):
        gone = set(int(p) for p in positions)
        live = [u for p, u in enumerate(self.live) if p not in gone]
        self.nbr, self.sim, self.reranked = up.remove_by_damage(self.nbr, self.sim, self.scores(live), sorted(gone), self.kg)
        self.live = live

    def check(self, what):
        nbr, sim = up.lists_from_scratch(self.scores(), self.kg)
        assert _same(self.nbr, nbr) and _same(self.sim, sim), (what, self.kg, len(self.live))


def test_lists_from_scratch_are_the_first_others(universe):
    """ranking to depth kg + 1 and dropping self = the first kg columns j != i of the complete ranking, self on top or not"""
    S = universe[:N0, :N0]
    for kg in KGS:
        nbr, sim = up.lists_from_scratch(S, kg)
        for i in range(N0):
            wi, wv = up.first_others(S, i, kg)
            assert np.array_equal(nbr[i], wi) and _same(sim[i], wv), (kg, i)
        assert not (nbr == np.arange(N0)[:, None]).any()
    assert (np.signbit(sim) & (sim == 0)).sum() == 0           # a ranking returns +0


@pytest.mark.parametrize("kg", KGS)
@pytest.mark.parametrize("b", [1, 3, 45])
def test_add_equals_scratch(universe, kg, b):
    """b = 1, b < kg, b > kg (for kg = 5; the other depths see the same three sizes on their side of kg)"""
    g = Maintained(universe, kg, range(N0))
    g.add(range(N0, N0 + b))
    g.check(f"add {b}")
    g.add(range(N0 + b, N0 + b + 2))                           # and again, on lists that were merged
    g.check(f"add {b} + 2")


def _start(universe, kg):
    """40 rows; the depth that fills them (kg = 39 = N - 1) first grows by 45 through the merge, so that rows can leave"""
    g = Maintained(universe, kg, range(N0))
    if kg == N0 - 1:
        g.add(range(N0, N0 + 45))
    return g


def _hub(nbr):
    return int(np.bincount(nbr[nbr >= 0].ravel(), minlength=nbr.shape[0]).argmax())


@pytest.mark.parametrize("kg", KGS)
def test_remove_equals_scratch(universe, kg):
    cases = {"one row": lambda g: [17], "a hub": lambda g: [_hub(g.nbr)], "first": lambda g: [0], "last": lambda g: [len(g.live) - 1],
             "a run": lambda g: list(range(10, 19)), "every other row": lambda g: list(range(0, len(g.live), 2))}
    for what, pick in cases.items():
        g = _start(universe, kg)
        g.remove(pick(g))
        g.check(what)
        assert 0 <= g.reranked <= len(g.live)
        if what == "a hub":
            assert g.reranked >= 1
    g = _start(universe, kg)
    g.remove(range(kg + 1, len(g.live)))                       # down to N' = kg + 1: every list is all the others
    g.check("down to kg + 1")
    assert len(g.live) == kg + 1
    with pytest.raises(ValueError, match="would survive"):     # N' = kg
        g.remove([0])
    assert len(g.live) == kg + 1
    g.check("after the refusal")


@pytest.mark.parametrize("kg", KGS)
def test_mixed_sequences_equal_scratch(universe, kg):
    rng = np.random.default_rng(kg)
    g = Maintained(universe, kg, range(N0))
    nxt = N0
    for step in range(12):
        if step % 3 != 2 or len(g.live) - kg - 1 < 1:
            b = int(rng.choice([1, 2, 7, 12]))
            b = min(b, UNIVERSE - nxt)
            if b == 0:
                continue
            g.add(range(nxt, nxt + b))
            nxt += b
            g.check(f"step {step}: add {b}")
        else:
            r = int(rng.integers(1, min(9, len(g.live) - kg - 1) + 1))
            g.remove(rng.choice(len(g.live), r, replace=False))
            g.check(f"step {step}: remove {r}")
    g.remove([_hub(g.nbr)])
    g.check("the hub at the end")


def test_refusal_leaves_nothing_changed(universe):
    g = Maintained(universe, 39, range(N0))                    # N = kg + 1 already
    nbr, sim = g.nbr.copy(), g.sim.copy()
    with pytest.raises(ValueError, match="would survive"):
        g.remove([5])
    assert _same(g.nbr, nbr) and _same(g.sim, sim) and len(g.live) == N0


def test_kernel_definitions_by_hand():
    nan = np.float32(np.nan)
    nbr = np.array([[1, 2, 3], [0, 2, 3], [0, 4, 1]], np.int32)
    sim = np.array([[3, 2, 2], [2, 0, nan], [1, 1, nan]], np.float32)
    cidx = np.array([[1, 0], [0, 1], [-1, 1]], np.int64)         # relative to 5; row 2's first candidate is an empty slot
    cval = np.array([[2, 1], [-0.0, nan], [9, 1]], np.float32)
    on, os = up.merge(nbr, sim, cidx, cval, 5, 7)
    assert np.array_equal(on, [[1, 2, 3], [0, 2, 5], [0, 4, 6]])   # 2 (id 6) ties 2 (ids 2, 3): the smaller ids stay; -0 (id 5) ties 0 (id 2)
    assert _same(os, np.array([[3, 2, 2], [2, 0, -0.0], [1, 1, 1]], np.float32))
    on, os = up.merge(nbr, sim, np.array([[0], [0], [0]], np.int64), np.array([[3], [nan], [1]], np.float32), 5, 7)
    assert np.array_equal(on, [[1, 5, 2], [0, 2, 3], [0, 4, 5]])   # equal score: the old id first; NaN against NaN: by id
    assert up.before(1.0, 9, nan, 0) and not up.before(nan, 0, 1.0, 9) and up.before(nan, 1, nan, 2) and not up.before(0.0, 3, -0.0, 3)
    keep = np.array([1, 1, 0, 1, 1], np.uint8)
    pos = np.array([0, 1, 2, 2, 3, 4], np.int64)
    big = np.array([[1, 3], [2, 0], [0, 1], [4, -1], [3, 9]], np.int32)
    assert np.array_equal(up.damage(big, keep), [0, 1, 0, 0, 0])   # row 2 lists kept rows only but leaves itself; -1 and 9 never count
    assert np.array_equal(up.remap(big, keep, pos), [[1, 2], [-1, 0], [0, 1], [3, -1], [2, -1]])
    n2, s2 = np.full((4, 2), 7, np.int32), np.full((4, 2), 7, np.float32)
    up.lists(np.array([[2, 0, 1], [0, 1, 3], [1, 2, 5]], np.int64), np.array([[3, 2, 1], [3, 2, 1], [3, 2, 1]], np.float32), [2, 3, 9], 4, n2, s2)
    assert np.array_equal(n2, [[7, 7], [7, 7], [0, 1], [0, 1]]) and np.array_equal(s2, [[7, 7], [7, 7], [2, 1], [3, 2]])
    assert np.array_equal(up.gather_rows(big, [4, -1, 0, 5]), [[3, 9], [0, 0], [1, 3], [0, 0]])
    assert _same(up.affinity_sim(np.array([[0.5, -1, nan]], np.float32), 3), np.array([[0.125, 0, 0]]))
