"""CPU tests of the ranking twin (tests/topk_numpy.py) and of the planted panels (tests/topk_cases.py).

The twin is checked against a brute-force ranking that shares no code with it; every adversarial panel is checked, from the twin
alone, for the condition that makes the device kernels take the branch the panel is meant for.  Nothing here needs a GPU."""
import math
import struct

import numpy as np
import pytest

import ivf_numpy as iv
import pq_numpy as pq
import topk_cases as tc
import topk_numpy as tk


# ------------------------------------------------------------------------------------------------ brute force
def _brute(ids, vals, k, dtype):
    """Python's sorted over (is_nan, -value with zero normalised, index) tuples; values and bit patterns built with struct"""
    ent = []
    for i, v in zip(ids, vals):
        i, v = int(i), float(v)
        if i < 0:
            continue
        if math.isnan(v):
            ent.append((1, 0.0, i, float("nan")))
        else:
            z = 0.0 if v == 0.0 else v
            ent.append((0, -z, i, z))
    ent.sort(key=lambda e: e[:3])
    fmt, ufmt, qn = ("<f", "<I", 0x7fc00000) if dtype == np.float32 else ("<d", "<Q", 0x7ff8000000000000)
    idx, bits = [], []
    for e in ent[:k]:
        idx.append(e[2])
        bits.append(qn if e[0] else struct.unpack(ufmt, struct.pack(fmt, e[3]))[0])
    minus_inf = struct.unpack(ufmt, struct.pack(fmt, float("-inf")))[0]
    idx += [-1] * (k - len(idx))
    bits += [minus_inf] * (k - len(bits))
    return idx, bits


def _nasty_row(rng, n, dt):
    """small alphabet, so ties abound: numbers, +-0, +-inf, denormals, NaN with payloads and sign bits"""
    tiny = np.finfo(dt).smallest_subnormal
    alphabet = np.array([0.0, -0.0, 1.0, -1.0, 1.5, np.inf, -np.inf, tiny, -tiny, 3 * tiny, np.finfo(dt).max, np.nan, np.nan, np.nan],
                        dt)
    row = alphabet[rng.integers(0, len(alphabet), n)].copy()
    nan = np.flatnonzero(np.isnan(row))
    pat = np.array(tc._NAN_BITS[np.dtype(dt)], tk.bits(row).dtype)
    tk.bits(row)[nan] = pat[rng.integers(0, len(pat), len(nan))]
    return row


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_twin_equals_brute_force_ranking(dt):
    rng = np.random.default_rng(7)
    seen_payload = False
    for n in (0, 1, 2, 7, 40, 130):
        s = np.array([_nasty_row(rng, n, dt) for _ in range(6)], dt).reshape(6, n)
        seen_payload = seen_payload or bool((np.isnan(s) & (tk.bits(s) != tk.QNAN_BITS[np.dtype(dt)])).any())
        for k in (1, 3, n, n + 2):
            if k < 1:
                continue
            for off in (0, 1000, 0xfffffffe - n):
                idx, val = tk.topk(s, k, off)
                assert idx.dtype == np.int64 and val.dtype == dt and idx.shape == val.shape == (6, k)
                for r in range(6):
                    bi, bb = _brute(range(off, off + n), s[r], k, dt)
                    assert idx[r].tolist() == bi and tk.bits(val[r]).tolist() == bb
    assert seen_payload


def test_twin_panels_lists_and_candidates_are_one_rule():
    """merge_panels = topk of the concatenation in any arrival order; merge_lists / candidates = brute force with id < 0 skipped"""
    rng = np.random.default_rng(8)
    f = np.float32
    s = np.array([_nasty_row(rng, 90, f) for _ in range(4)], f)
    for k in (1, 5, 90, 95):
        want = tk.topk(s, k, 10)
        for cuts in ([0, 90], [0, 3, 90], [0, 40, 40, 77, 90]):
            panels = [s[:, a:b] for a, b in zip(cuts[:-1], cuts[1:])]
            offs = [10 + a for a in cuts[:-1]]
            for order in (range(len(panels)), reversed(range(len(panels)))):
                order = list(order)
                got = tk.merge_panels([panels[i] for i in order], [offs[i] for i in order], k)
                assert np.array_equal(got[0], want[0]) and np.array_equal(tk.bits(got[1]), tk.bits(want[1]))
    ids = np.array([rng.permutation(1 << 20)[:60] * 4093 for _ in range(4)], np.int64)      # distinct, up to 2^32
    assert ids.max() > 1 << 31
    ids[rng.random(ids.shape) < 0.3] = -1
    v = np.array([_nasty_row(rng, 60, f) for _ in range(4)], f)
    for k in (1, 7, 60, 64):
        ci, cv = tk.candidates(ids, v, k)
        li, lv = tk.merge_lists(ids.reshape(4, 3, 20).transpose(1, 0, 2), v.reshape(4, 3, 20).transpose(1, 0, 2), k)
        for r in range(4):
            bi, bb = _brute(ids[r], v[r], k, f)
            assert ci[r].tolist() == bi and tk.bits(cv[r]).tolist() == bb
            assert li[r].tolist() == bi and tk.bits(lv[r]).tolist() == bb


def test_value_rules_reach_the_other_twins():
    """pq_numpy.topk and ivf_numpy.search state the rule through topk_numpy: a -0 winner comes back as +0, a NaN as the quiet NaN"""
    s = np.array([[-0.0, 0.0, -1.0, np.nan]], np.float32)
    tk.bits(s)[0, 3] = 0xffc00001
    idx, val = pq.topk(s, 4, 5)
    assert idx.tolist() == [[5, 6, 7, 8]] and tk.bits(val).tolist() == [[0, 0, 0xbf800000, 0x7fc00000]]
    table = np.array([[[-0.0, -1.0, np.nan]]], np.float32)                     # one query, one sub-space, three codewords
    tk.bits(table)[0, 0, 2] = 0xffc00001
    codes = np.array([[0], [1], [2], [0]], np.uint8)
    co = np.array([[-0.0, -5.0]], np.float32)
    idx, val = iv.search(table, co, 1, np.array([0, 4, 4], np.int64), np.array([3, 2, 1, 0], np.int32), codes, None, None, 6)
    assert idx.tolist() == [[0, 3, 2, 1, -1, -1]]
    assert tk.bits(val).tolist() == [[0, 0, 0xbf800000, 0x7fc00000, 0xff800000, 0xff800000]]


# ------------------------------------------------------------------------------------------------ the panels meet their conditions
def _cases():
    for ncols in tc.NCOLS:
        for k in tc.KS + tc.KS_PAGED:
            n = tc.resolve_ncols(ncols, k)
            if n >= 0:
                yield n, k


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_every_panel_has_its_shape_dtype_and_is_reproducible(dt):
    for group, fns in tc.GROUPS.items():
        assert len(fns) <= 9 and len(fns) % 4 != 0                              # the wave kernels retire whole waves of four rows
        for n, k in ((0, 1), (1, 1), (65, 17), (2049, 16), (8197, 1024)):
            p = tc.panel(group, n, k, dt)
            assert p.shape == (len(fns), n) and p.dtype == dt
            assert np.array_equal(tk.bits(p), tk.bits(tc.panel(group, n, k, dt)))


def test_plateau_rows_overflow_the_wave_list():
    """k <= 16, complete chunks: the plateau straddles the cut at k, and more than 256 columns of one 2048-column chunk score at or
    above the k-th best known by the end of that chunk -- in the first chunk for one row, in a later chunk, after better scores have
    been listed, for the other.  The all-equal row overflows in every complete chunk."""
    f = np.float32
    for n in (2048, 2049, 4096, 4099, 6151, 8192, 8197, 16389):
        for k in (1, 2, 15, 16):
            rng = np.random.default_rng(k)
            first, late = tc.row_plateau_first_chunk(rng, n, k, f), tc.row_plateau_late_chunk(rng, n, k, f)
            for row in (first, late):
                _, val = tk.topk(row[None, :], k + 1)
                assert val[0, k - 1] == val[0, k] == f(0.5) and (row == f(0.5)).sum() >= tc.PLATEAU     # straddles the cut
                assert (row > f(0.5)).sum() == k // 2
            assert tc.wave_overflow_chunks(first, k)[:1] == [0]
            if n >= tc.SWITCH:                                                 # room for the plateau after the first chunk
                over = tc.wave_overflow_chunks(late, k)
                assert over and over[0] >= tc.WAVE_CHUNK
                if k >= 2:                                                     # entries already listed: the better scores came earlier
                    assert (late[:over[0]] > f(0.5)).sum() == k // 2
            assert tc.wave_overflow_chunks(tc.row_all_equal(rng, n, k, f), k) == list(range(0, n - tc.WAVE_CHUNK + 1, tc.WAVE_CHUNK))


def test_nan_lane_row_has_nan_among_the_first_chunks_lane_maxima():
    for n in (2048, 4099, 16389):
        row = tc.row_nan_lanes(np.random.default_rng(2), n, 16, np.float32)
        vec, sca = tc.nan_lane_counts(row)
        assert vec == 62 and sca == 56
        # 2 and 8 lanes keep a number: at k = 15, 16 the k-th largest lane maximum is a NaN in either layout, a threshold every
        # column of the chunk reaches, and the chunk has more columns than the list has room; at k = 1, 2 it is a number
        for k in (15, 16):
            assert 64 - vec < k and 64 - sca < k and min(n, tc.WAVE_CHUNK) > tc.WAVE_LIST
        assert 64 - vec >= 2 and 64 - sca >= 2
        assert not np.isnan(row[:tc.WAVE_CHUNK]).all()
    row = tc.row_fewer_numbers_than_k(np.random.default_rng(2), 4099, 16, np.float32)
    assert (~np.isnan(row)).sum() == 8


def test_radix_depth_row_needs_all_eight_passes():
    """the keys on either side of the cut agree in their top 56 bits: no histogram pass before the eighth can separate them, and no
    pivot bin before it is taken whole"""
    checked = 0
    for n, k in _cases():
        if k <= 3 or n < k + 2 + tc.RADIX_HOLES:
            continue
        row = tc.row_radix_depth(None, n, k, np.float32)
        a, b = tc.cut_keys(row, k)
        assert a > b and (a >> 8) == (b >> 8), (n, k)
        checked += 1
    assert checked > 50
    a, b = tc.cut_keys(tc.row_all_equal(None, 4099, 17, np.float32), 17)        # the all-equal row: same, except at k % 256 == 0
    assert (a >> 8) == (b >> 8)


def test_value_rows_put_their_values_among_the_winners():
    f = np.float32
    for n, k in ((65, 16), (4099, 17), (8197, 1024)):
        rng = np.random.default_rng(3)
        z = tc.row_signed_zeros(rng, n, k, f)
        idx, val = tk.topk(z[None, :], k)
        won = z[idx[0][idx[0] >= 0]]
        assert (won == 0).all() and np.signbit(won).any() and not np.signbit(won).all()           # -0 and +0 mixed among the winners
        assert not np.signbit(val[0]).any()
        d = tc.row_denormals(rng, n, k, f)
        assert (np.abs(d[d != 0]) < np.finfo(f).tiny).all() and (d > 0).any() and (d < 0).any()
        p = tc.row_nan_payloads(rng, n, k, f)
        nb = tk.bits(p)[np.isnan(p)]
        assert (nb >> 31).any() and (nb != 0x7fc00000).any() and ((nb & 0x00400000) == 0).any()  # signed, payload, signalling
        e = tc.row_exactly_k_numbers(rng, n, k, f)
        assert (~np.isnan(e)).sum() == min(n, k)
        t = tc.row_ties_across_chunks(rng, n, k, f)
        best = [c for c in (5, 5 + 2048, 5 + 8192) if c < n]
        assert (t[best] == t.max()).all() and tk.topk(t[None, :], len(best))[0][0].tolist() == best
        i = tc.row_infinities(rng, n, k, f)
        assert np.isposinf(i).any() and np.isneginf(i).any()


def test_merge_cases_meet_their_conditions():
    for k in (1, 2, 16, 17, 300, 1024):
        panels, offs = tc.merge_case("short_then_long", k)
        assert panels[0].shape[1] < k and panels[1].shape[1] >= tc.SWITCH        # a partly filled list, then the other kernel
        assert offs == [0, panels[0].shape[1]]
        assert (~np.isnan(np.concatenate(panels, axis=1)[5])).sum() == k // 3 < k   # NaN columns are among the best k of row 5
        for name in ("empty_middle", "empty_last"):
            panels, _ = tc.merge_case(name, k)
            assert 0 in [p.shape[1] for p in panels[1:]]
        panels, offs = tc.merge_case("ties_lower_and_higher", k)
        assert offs[1] + panels[1].shape[1] <= offs[0] and offs[2] >= offs[0] + panels[0].shape[1]
        _, val = tk.topk(panels[0], k, offs[0])
        for r in (1, 2) if k <= 300 else (1,):                                 # all-equal row, plateau row: the list's k-th entry ...
            kth = val[r, min(k, panels[0].shape[1]) - 1]
            assert (panels[1][r] == kth).any() and (panels[2][r] == kth).any()  # ... is tied from below and from above
        sizes = {tuple(p.shape[1] for p in tc.merge_case(n, k)[0]) for n in tc.MERGE_CASES}
        assert {len(s) for s in sizes} == {2, 3} and all(len(set(s)) == len(s) for s in sizes)   # two and three panels, unequal


def test_merge_lists_cases_meet_their_conditions():
    for n_lists in (1, 2, 8, 9):
        for k in (1, 16, 17, 1024):
            idx, val = tc.merge_lists_case(n_lists, k)
            assert idx.shape == val.shape == (n_lists, 5, k)
            assert (idx[:, 4] == -1).all()                                      # a query whose lists are all unfilled
            assert (idx < tc.INDEX_LIMIT).all() and np.isneginf(val[idx < 0]).all()
            for q in range(4):
                flat = idx[:, q][idx[:, q] >= 0]
                assert len(set(flat.tolist())) == len(flat)                     # distinct within a query
            if n_lists >= 2:
                assert (idx[:, 1] >= 0).sum() == k                              # exactly k valid entries
            if n_lists * k >= 64:
                assert (idx > 1 << 31).any() and (n_lists == 1 or (idx[1::2, 0, -1] == -1).any())  # ids above 2^31; unfilled tails
                v0 = val[:, 0][idx[:, 0] >= 0]
                assert len(np.unique(v0)) < len(v0)                             # equal scores, decided by id
    assert 9 * 1024 > tc.RADIX_CHUNK                                           # nine lists at k = 1024 are two chunks


def test_paging_rows_and_padding_meet_their_conditions():
    """the first NaN of rows 1 - 3 sits at rank 1023, 1024, 1025: on either side of the page boundary; ties cross it in rows 4 and 6; 1500
    and 2047 columns leave the second page short; padding columns are +inf and would outrank every planted score"""
    for ncols in tc.PAGING_NCOLS:
        rows = tc.paging_rows(ncols)
        assert rows.shape == (7, ncols) and rows.shape[0] % 4 != 0
        idx, val = tk.topk(rows, 2 * tc.KMAX + 1)
        for r, numbers in tc.PAGE_EDGE_ROWS:
            assert np.isnan(val[r, numbers]) and not np.isnan(val[r, numbers - 1])
        assert val[6, tc.KMAX - 1] == val[6, tc.KMAX] and val[4, tc.KMAX - 1] == val[4, tc.KMAX]   # equal scores cross the page boundary
        assert (idx[:, -1] == -1).all() == (ncols < 2 * tc.KMAX + 1)
    assert any(tc.KMAX < n < 2 * tc.KMAX for n in tc.PAGING_NCOLS)
    p = tc.panel("A", 63, 16)
    q = tc.padded(p, 3)
    assert q.shape == (9, 66) and np.isposinf(q[:, 63:]).all() and np.array_equal(tk.bits(q[:, :63]), tk.bits(p))
    assert not np.isposinf(p[[0, 2, 3]]).any()


# ------------------------------------------------------------------------------------------------ the score panels around the ranking
def test_panel_plan_rules_hold_their_literal_values(tmp_path):
    """csrc/bench/panel_plan_check.cpp includes only panel_plan.hpp, whose host part needs no HIP header, and runs as a stand-alone
    program under the address and undefined-behaviour sanitizers (nothing is loaded into Python): the block sizes of the dense, scan,
    filter and complete-row rules, the refusal of a deep ranking that needs more than one panel (status and message), the byte rule
    of a panel and the query block of the host float64 entry, each against literal values worked out by hand; then, over a sweep of
    (nq, N, k), that the blocks tile [0, nq) x [0, N) exactly once and stay within the 1 GiB budget unless a panel is one row."""
    import os
    import shutil
    import subprocess

    from conftest import REPO
    src = os.path.join(REPO, "python-visual-similarity_amd", "csrc", "bench", "panel_plan_check.cpp")
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (g++, c++ or clang++) on PATH"
    exe = str(tmp_path / "panel_plan_check")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
