"""CPU tests of the multiple assignment of query rows: the NumPy twin (tests/asmk_ma_numpy.py) against the single-assignment twin it
extends, the validation of `ma` in pvsim.asmk before any device work, the header, and the quality record of DESIGN.md section 17 on a
planted corpus."""
import os
import re

import numpy as np
import pytest

import asmk_ma_numpy as ma
import asmk_numpy as tw

F = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lattice_inputs(rng, n, K, D):
    """rows: integers in [-8, 8]; centroids: multiples of 1/2 in [-8, 8] -- every v is exact in float32"""
    return rng.randint(-8, 9, (n, D)).astype(F), (rng.randint(-16, 17, (K, D)) / 2.0).astype(F)


# ------------------------------------------------------------------------------------------------ the twin
def test_twin_at_m_1_equals_the_single_assignment_twin():
    rng = np.random.RandomState(2100)
    cent = rng.standard_normal((40, 32)).astype(F)
    x = (cent[rng.randint(0, 40, 90)] + 0.1 * rng.standard_normal((90, 32))).astype(F)
    want_lab, gap = tw.labels_and_gap(x, cent)
    assert gap > 1e-3
    lab, v = ma.topm(x, cent, 1)
    assert lab.shape == (90, 1) and lab.dtype == np.int32 and np.array_equal(lab[:, 0], want_lab)
    for proj in (None, rng.standard_normal((64, 32)).astype(F)):
        w1, s1 = tw.image_entries(x, want_lab, cent, proj)
        w2, s2 = ma.image_entries_ma(x, lab, cent, proj)
        assert np.array_equal(w1, w2) and np.array_equal(s1, s2)


def test_twin_ties_go_to_the_lowest_index():
    cent = np.zeros((6, 4), F)
    cent[[1, 4]] = 1.0                                                     # 0, 2, 3, 5 are one point; 1, 4 another
    x = np.array([[0, 0, 0, 0], [1, 1, 1, 1], [np.nan, 0, 0, 0]], F)
    lab, v = ma.topm(x, cent, 6)
    assert lab[0].tolist() == [0, 2, 3, 5, 1, 4] and lab[1].tolist() == [1, 4, 0, 2, 3, 5]
    assert lab[2].tolist() == [0, 1, 2, 3, 4, 5] and np.isposinf(v[2]).all()       # NaN counts as +inf: index order
    assert np.array_equal(ma.topm_chain(x, cent, 6)[0], lab)
    with pytest.raises(ValueError):
        ma.topm(x, cent, 7)
    with pytest.raises(ValueError):
        ma.topm(x, cent, 0)


def test_twin_chain_is_exact_on_the_lattice_and_follows_the_stated_order():
    rng = np.random.RandomState(2110)
    x, cent = _lattice_inputs(rng, 37, 50, 20)
    assert np.array_equal(ma.v_chain(x, cent).astype(np.float64), ma.values64(x, cent))
    # off the lattice the chain is the header's order, dims (8t + e, 8t + 4 + e): against a scalar restatement with exact fmas
    from fractions import Fraction
    x, cent = rng.standard_normal((3, 13)).astype(F), rng.standard_normal((4, 13)).astype(F)

    def rn(fr):                                                            # a rational to the nearest float32, ties to even
        lo = F(float(fr))
        cands = {lo, np.nextafter(lo, F(-np.inf)), np.nextafter(lo, F(np.inf))}
        return min(cands, key=lambda c: (abs(Fraction(float(c)) - fr), int(np.array(c, F).view(np.uint32)) & 1))

    got = ma.v_chain(x, cent)
    for i in range(3):
        for j in range(4):
            acc = F(0)
            for b8 in range(0, 13, 8):
                for e in range(4):
                    for d in (b8 + e, b8 + 4 + e):
                        if d < 13:
                            acc = rn(Fraction(float(cent[j, d])) * Fraction(float(x[i, d])) + Fraction(float(acc)))
            cn = F(0)
            for d in range(13):
                cn = cn + cent[j, d] * cent[j, d]
            v = rn(Fraction(-2) * Fraction(float(acc)) + Fraction(float(cn)))
            assert got[i, j].view(np.uint32) == v.view(np.uint32), (i, j)


def test_twin_entries_with_shared_words():
    """two rows that hold the same word in different slots add to the same entry in row order"""
    cent = np.zeros((3, 32), F)
    cent[1, 0], cent[2, 0] = 4, 8
    x = np.zeros((2, 32), F)
    x[0, 0], x[1, 0] = 1.5, 5.5                                            # row 0: words 0, 1; row 1: words 1, 2 (nearest first)
    lab, _ = ma.topm(x, cent, 2)
    assert lab.tolist() == [[0, 1], [1, 2]]
    words, sigs = ma.image_entries_ma(x, lab, cent)
    assert words.tolist() == [0, 1, 2]
    # word 1: V[0] = (1.5 - 4) + (5.5 - 4) < 0, every other coordinate +0 -> bit 0 clear
    assert sigs[1, 0] == 0xFFFFFFFE and sigs[0, 0] == 0xFFFFFFFF and sigs[2, 0] == 0xFFFFFFFE
    with pytest.raises(AssertionError):
        ma.image_entries_ma(x, np.array([[1, 1], [1, 2]]), cent)           # a row's labels must be distinct


def test_rank_gaps_refuses_near_ties():
    rng = np.random.RandomState(2120)
    cent = rng.standard_normal((30, 16)).astype(F)
    x = rng.standard_normal((60, 16)).astype(F)
    x = x[ma.rank_gap_ratios(x, cent, 3) > 2.0]                            # keep the rows with clear ranks
    assert len(x) >= 10
    ok, ratio = ma.rank_gaps(x, cent, 3)
    assert ok and ratio > 1
    cent[7] = cent[ma.topm(x[:1], cent, 1)[0][0, 0]]                        # a duplicate of row 0's nearest word: gap 0
    assert not ma.rank_gaps(x, cent, 3)[0]


# ------------------------------------------------------------------------------------------------ pvsim.asmk
def _host_index(K=6, D=32):
    from pvsim import ASMKIndex
    from pvsim.asmk import selectivity
    from pvsim._ffi import DESC_F32
    cent = np.arange(K * D, dtype=F).reshape(K, D)
    return ASMKIndex(["a"], cent, np.zeros(K + 1, np.int64), np.zeros(0, np.int32), np.zeros((0, 1), np.uint32), np.zeros(1, F),
                     np.zeros(K, np.int32), selectivity(32), 32, desc_kind=DESC_F32, ctx=_NoDevice())


class _NoDevice:
    """stands where the context would: any use is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError(f"device work ({name}) before the arguments were checked")


@pytest.mark.parametrize("bad", [0, -1, 7, 9, 2.0, "3", None, True])
def test_ma_is_validated_before_any_device_work(bad):
    index = _host_index(K=6)
    rows = [np.zeros((4, 32), F)]
    with pytest.raises(ValueError, match="ma must be an integer in 1..6"):
        index.rank_rows(rows, 3, ma=bad)
    with pytest.raises(ValueError, match="ma must be"):
        index.rank_images([np.zeros((8, 8), np.uint8)], 3, ma=bad)
    with pytest.raises(ValueError, match="ma must be"):
        index.retrieve(np.zeros((8, 8), np.uint8), 3, ma=bad)
    with pytest.raises(ValueError, match="ma must be"):
        index.query_entries(0, np.array([0, 4]), ma=bad)


def test_rows_times_ma_beyond_16384_is_refused_before_any_device_work():
    index = _host_index(K=40)
    rows = [np.zeros((3, 32), F), np.zeros((2049, 32), F)]
    with pytest.raises(NotImplementedError, match=r"2049.*16392"):
        index.rank_rows(rows, 3, ma=8)
    with pytest.raises(NotImplementedError, match=r"3277.*16385"):
        index.query_entries(0, np.array([0, 3277]), ma=5)
    from pvsim.asmk import check_ma
    assert check_ma(8, 40, np.array([0, 2048])) == 8 and check_ma(5, 40, np.array([0, 2000])) == 5
    assert check_ma(1, 40, np.array([0, 8192])) == 1 and check_ma(np.int64(3), 40) == 3


def test_header_declares_the_new_symbols():
    text = open(os.path.join(REPO, "include", "pvsim.h")).read()
    assert re.search(r"\bint\s+pvs_kmeans_topm_dev\s*\(pvs_ctx\*", text)
    assert re.search(r"\bint\s+pvs_asmk_aggregate_ma_dev\s*\(pvs_ctx\*", text)
    from pvsim import _ffi
    assert len(_ffi.SIGNATURES["pvs_kmeans_topm_dev"]) == 9 and len(_ffi.SIGNATURES["pvs_asmk_aggregate_ma_dev"]) == 15


# ------------------------------------------------------------------------------------------------ quality record
def test_planted_corpus_recall_by_words_per_row():
    """A lattice vocabulary of 1024 words; the queries' rows are perturbed until about three quarters of them change their nearest
    word (asserted: between 0.70 and 0.80).  recall@1 of the twin, database single assignment, recorded in DESIGN.md section 17:
    0.617 at ma = 1, 0.917 at ma = 3, 0.950 at ma = 5.  The twin satisfies recall(ma = 3) >= recall(ma = 1) on this corpus, so that is
    asserted; the figures themselves are a record, not a threshold."""
    cent, images, queries, truth, moved = ma.planted_corpus_ma()
    assert len(cent) == 1024 and 0.70 <= moved <= 0.80
    recall = {m: ma.recall_at_1(cent, images, queries, truth, m) for m in (1, 3, 5)}
    print("planted corpus: moved", round(moved, 3), "recall@1", recall)
    assert recall[3] >= recall[1]
