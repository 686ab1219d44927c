"""CPU tests of the int8 threshold join: the NumPy twin (tests/sq8_range_numpy.py) against a brute-force double
loop, the asymmetry of the score and the self-join's definition on a seeded corpus that exercises it, the monotonicity in the integer
sum, zero rows, the mask geometry, and what the Python layer checks before the device is touched."""
import os
import subprocess

import numpy as np
import pytest

import sq8_numpy as sq
import sq8_range_numpy as tw
from conftest import REPO

F = np.float32


def random_codes(rng, n, L, zero_rows=()):
    """int8 (n, ld) code rows with L live bytes in -127 .. 127, the padding zero, and their factors"""
    c = np.zeros((n, sq.ld_of(L)), np.int8)
    c[:, :L] = rng.integers(-127, 128, (n, L), dtype=np.int64).astype(np.int8)
    for r in zero_rows:
        c[r] = 0
    return c, sq.factors(c)


def asymmetric_corpus(n=257, L=100, seed=30):
    """-> (codes, inv, t): the rows of a seeded corpus with two rows x, y whose score depends on the role, s(x as query, y) <
    s(y as query, x) = t, planted as x at 3, y at 10 and copies y at 20, x at 30.  At t the pair (3, 10) has s(i, j) < t <= s(j, i)
    and is NOT emitted; the pair (20, 30) has s(j, i) < t <= s(i, j) and is."""
    rng = np.random.default_rng(seed)
    c, inv = random_codes(rng, n, L)
    S = tw.scores(c, inv, c, inv)
    x, y = np.argwhere(S < S.T)[0]                                    # the first pair, in row-major order, whose two roles differ
    cx, cy = c[x].copy(), c[y].copy()
    c[3], c[10], c[20], c[30] = cx, cy, cy, cx
    inv = sq.factors(c)
    S = tw.scores(c, inv, c, inv)
    return c, inv, F(S[10, 3])


def test_twin_matches_the_double_loop():
    rng = np.random.default_rng(3)
    for nq, N, L in ((1, 1, 1), (5, 9, 3), (9, 9, 70), (17, 33, 130)):
        qc, iq = random_codes(rng, nq, L)
        dc, idb = random_codes(rng, N, L, zero_rows=(0,))
        S = tw.scores(qc, iq, dc, idb)
        for t in (F(-2.0), F(0.0), F(np.median(S)), np.nextafter(F(np.median(S)), F(1))):
            want = tw.brute(qc, iq, dc, idb, t)
            for QT, NC in ((nq, N), (4, 8), (1, 1)):
                got = tw.join(qc, iq, dc, idb, t, QT, NC)
                order = np.lexsort((got[1], got[0]))
                assert np.array_equal(got[0][order], want[0]) and np.array_equal(got[1][order], want[1])
                assert np.array_equal(got[2][order].view(np.uint32), want[2].view(np.uint32))
    c, inv = random_codes(rng, 21, 40)
    t = F(np.quantile(tw.scores(c, inv, c, inv), 0.6))
    want = tw.brute(c, inv, c, inv, t, upper=True)
    got = tw.self_join(c, inv, t)
    assert want[0].size > 10 and all(np.array_equal(g.view(np.uint8), w.view(np.uint8)) for g, w in zip(got, want))
    tiled = tw.join(c, inv, c, inv, t, 8, 8, upper=True)
    order = np.lexsort((tiled[1], tiled[0]))
    assert all(np.array_equal(g[order].view(np.uint8), w.view(np.uint8)) for g, w in zip(tiled, want))


def test_score_is_not_symmetric_and_the_corpus_exercises_both_cases():
    rng = np.random.default_rng(5)
    c, inv = random_codes(rng, 200, 64)
    S = tw.scores(c, inv, c, inv)
    differ = (S != S.T)[np.triu_indices(200, 1)].mean()
    assert 0.15 < differ < 0.6, differ                               # about a third of the pairs: (a x) y against (a y) x
    assert np.array_equal(sq.acc(c, c), sq.acc(c, c).T)              # the integer is symmetric; the two roundings are not
    c, inv, t = asymmetric_corpus()
    S = tw.scores(c, inv, c, inv)
    lost, kept = tw.asymmetric_pairs(S, t)
    assert [3, 10] in lost.tolist() and [20, 30] in kept.tolist()
    assert S[3, 10] < t <= S[10, 3] and S[30, 20] < t <= S[20, 30]
    i, j, s = tw.self_join(c, inv, t)
    pairs = set(zip(i.tolist(), j.tolist()))
    assert (3, 10) not in pairs and (20, 30) in pairs                # row i < j in the query role decides, whatever s(j, i) says
    assert all((a, b) not in pairs for a, b in lost.tolist()) and all((a, b) in pairs for a, b in kept.tolist())
    assert (s >= t).all() and np.array_equal(s.view(np.uint32), S[i, j].view(np.uint32))


def test_score_is_monotone_in_the_integer_sum():
    rng = np.random.default_rng(6)
    acc = np.unique(np.concatenate([rng.integers(-2 ** 31 + 1, 2 ** 31 - 1, 4000), np.arange(-300, 300),
                                    2 ** 24 + np.arange(-40, 40), -(2 ** 24) + np.arange(-40, 40), [2114060288, -2114060288]]))
    a = acc.astype(np.int32).astype(F)
    assert (np.diff(a) >= 0).all()
    for iq, idb in [(F(1.0 / np.sqrt(float(ss1))), F(1.0 / np.sqrt(float(ss2)))) for ss1, ss2 in rng.integers(1, 127 * 127 * 131072, (40, 2))] + \
            [(F(0), F(0.3)), (F(0.25), F(0)), (F(1e-30), F(1e-30))]:
        s = (a * iq) * idb
        assert (np.diff(s) >= 0).all(), (iq, idb)                    # each rounding is monotone and the factors are not negative


def test_zero_rows_hit_at_zero_and_not_above():
    rng = np.random.default_rng(7)
    c, inv = random_codes(rng, 40, 33, zero_rows=(4, 17))
    assert inv[4] == 0 and inv[17] == 0
    S = tw.scores(c, inv, c, inv)
    assert not S[4].any() and not S[:, 17].any() and not np.signbit(S[4]).any()      # +0 against everything
    row, col, _ = tw.join(c, inv, c, inv, F(0.0), 40, 40)
    assert (row == 4).sum() == 40 and (col == 17).sum() == 40
    row, col, _ = tw.join(c, inv, c, inv, np.nextafter(F(0), F(1)), 40, 40)
    assert not (row == 4).any() and not (col == 17).any() and row.size > 0
    inv_nan = inv.copy()
    inv_nan[9] = np.nan                                               # a loaded file may hold any factor: NaN scores never hit
    row, col, _ = tw.join(c, inv_nan, c, inv_nan, F(-10.0), 40, 40)
    assert not (row == 9).any() and not (col == 9).any() and row.size == 39 * 39


def test_mask_geometry_restated():
    assert tw.geometry(8189, 32768, "mask") == (8189, 32768) and tw.geometry(8189, 32768, "panel") == (8189, 32768)
    assert tw.geometry(10 ** 6, 10 ** 6, "mask") == (8192, 262144) and tw.geometry(10 ** 6, 10 ** 6, "panel") == (8192, 32768)
    assert tw.geometry(257, 129, "mask", 100) == (100, 100) == tw.geometry(257, 129, "panel", 100)
    assert [tw.mask_words(c) for c in (1, 100, 128, 129, 160, 262144)] == [4, 4, 4, 8, 8, 8192]
    assert tw.mask_bytes(8189, 32768) == 32 << 20 and tw.mask_bytes(8192, 262144) == 256 << 20 and tw.mask_bytes(1, 1) == 2048
    assert tw.mask_bytes(8192, 262144) * 32 == 8192 * 262144 * 4       # 1/32 of the float panel's bytes
    assert tw.skipped_tiles(257, 257, 128, 128) == 4 and tw.skipped_tiles(257, 257, 100, 100) == 3


def test_panel_plan_check_pins_the_mask_rule(tmp_path):
    """bench/panel_plan_check.cpp holds panel_mask value by value: built and run here as tests/test_topk_host.py does"""
    src = os.path.join(REPO, "python-visual-similarity_amd", "csrc", "bench", "panel_plan_check.cpp")
    assert "panel_mask(8189, 32768)" in open(src).read()
    exe = str(tmp_path / "panel_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "panel_plan_check: ok" in out.stdout, out.stderr


def _empty_index(L=8):
    """an Int8Index of no rows without a device: enough for everything the methods check before they touch one"""
    from pvsim.index import _PathLedger
    from pvsim.quantized import Int8Index, padded_length
    index = Int8Index.__new__(Int8Index)
    index.ctx, index._L, index._ld, index._ledger, index.last_range_stats = None, L, padded_length(L), _PathLedger([]), None
    return index


def test_python_layer_validates_before_the_device():
    import pvsim
    from pvsim import eval as pv_eval
    from pvsim import quantized
    assert [quantized._range_path_code(p) for p in ("auto", "panel", "mask")] == [0, 1, 2]
    for bad in ("exact", "filtered", "fast", None, 1):
        with pytest.raises(ValueError, match="auto"):
            quantized._range_path_code(bad)
    index = _empty_index()
    q = np.zeros((2, 8), np.float32)
    for call in (lambda: index.range_search(q, np.nan), lambda: index.similar_pairs(np.inf), lambda: index.duplicates(1e39),
                 lambda: index.range_search(q, 0.5, max_results=-1), lambda: index.similar_pairs(0.5, max_pairs=1.5),
                 lambda: index.range_search(q, 0.5, path="exact"), lambda: index.similar_pairs(0.5, path="filtered"),
                 lambda: index.duplicates(0.5, path="fast"), lambda: index.duplicates(0.5, min_size=0),
                 lambda: index.range_search(np.zeros((2, 9), np.float32), 0.5), lambda: index.range_search(np.zeros(8, np.float32), 0.5),
                 lambda: index.range_search(np.full((1, 8), np.nan, np.float32), 0.5)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: index.range_search(q, "0.5"), lambda: index.similar_pairs(None), lambda: index.duplicates(True),
                 lambda: index.range_search(q.astype(np.float64), 0.5)):
        with pytest.raises(TypeError):
            call()
    indptr, idx, val = index.range_search(q, 0.5)                      # no rows: nothing to search, the device is not touched
    assert indptr.tolist() == [0, 0, 0] and idx.size == 0 and val.dtype == np.float32
    assert index.last_range_stats == {"threshold": 0.5}
    assert all(a.size == 0 for a in index.similar_pairs(0.1)) and index.last_range_stats == {"threshold": float(np.float32(0.1))}
    d = index.duplicates(0.9)
    assert isinstance(d, pvsim.DuplicateGroups) and d.groups == [] and d.stats["pairs"] == 0
    # the free functions keep refusing an Int8Index, and now say where its threshold search lives
    for call in (lambda: pvsim.find_duplicates(index, 0.9), lambda: pv_eval.find_duplicates(index, 0.9),
                 lambda: pv_eval.retrieve_similar(np.zeros((1, 8), np.float32), index, None, 0.9)):
        with pytest.raises(NotImplementedError, match="float32 pvsim.index.DeviceIndex") as e:
            call()
        assert all(word in str(e.value) for word in ("Int8Index", "range_search", "similar_pairs", "duplicates"))
    with pytest.raises(NotImplementedError, match="float32 pvsim.index.DeviceIndex") as e:
        pvsim.find_duplicates(object(), 0.9)
    assert "range_search" not in str(e.value)
    from pvsim.ivf_int8 import IVFInt8Index
    assert not any(hasattr(IVFInt8Index, m) for m in ("range_search", "similar_pairs", "duplicates"))


def test_header_and_ctypes_table_carry_the_symbol():
    import __graft_entry__ as g
    g.build()
    from pvsim import _ffi
    header = open(os.path.join(REPO, "include", "pvsim.h")).read()
    assert "int pvs_sq8_range_dev(" in header and len(_ffi.SIGNATURES["pvs_sq8_range_dev"]) == 18 and hasattr(_ffi.lib(), "pvs_sq8_range_dev")
    assert (_ffi.SQ8_RANGE_PATH_AUTO, _ffi.SQ8_RANGE_PATH_PANEL, _ffi.SQ8_RANGE_PATH_MASK) == (0, 1, 2)
