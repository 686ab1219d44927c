"""Host tests of the probed int8 scan by list: the NumPy twin of the grouping against a stable sort and a literal
example, the tiles of the twin against the candidate rows of section 26, the host rule under the sanitizers, the exported names and
the refusals of `IVFInt8Index.rank(scan=...)`.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ivf_sq8_lists_numpy as lt
import ivf_sq8_numpy as tw
import sq8_numpy as sq
from conftest import REPO


def _ragged(rng, nlist, nprobe, nq, planted=(0, 1, 127, 128, 129, 257)):
    """list offsets with the planted lengths among random ones, and distinct probes per query with some outside [0, nlist)"""
    sizes = rng.integers(0, 40, nlist)
    sizes[rng.permutation(nlist)[:min(nlist, len(planted))]] = planted[:min(nlist, len(planted))]
    list_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    probe = np.stack([rng.permutation(nlist)[:nprobe] for _ in range(nq)]).astype(np.int64)
    for bad in (-1, nlist):
        probe[rng.integers(0, nq), rng.integers(0, nprobe)] = bad
    return list_off, probe


def test_grouping_by_hand():
    list_off = np.array([0, 3, 3, 5, 9], np.int64)                     # lengths 3, 0, 2, 4
    probe = np.array([[2, 0], [3, 1], [0, 4], [-1, 2]], np.int64)      # query 2 probes list 4 = nlist, query 3 probes -1: no pairs
    base, total, goff, gq, gbase = lt.group_probes(probe, list_off)
    assert base.tolist() == [[0, 2], [0, 4], [0, 3], [0, 0]] and total.tolist() == [5, 4, 3, 2]
    assert goff.tolist() == [0, 2, 3, 5, 6]                            # list 0: queries 0, 2; list 1: 1; list 2: 0, 3; list 3: 1
    assert gq.tolist() == [0, 2, 1, 0, 3, 1] and gbase.tolist() == [2, 0, 4, 0, 0, 0]
    assert all(a.dtype == np.int32 for a in (base, total, goff, gq, gbase))


@pytest.mark.parametrize("nlist,nprobe,nq", [(1, 1, 3), (7, 2, 130), (7, 7, 17), (64, 9, 40), (300, 300, 5)])
def test_grouping_is_the_stable_sort(nlist, nprobe, nq):
    rng = np.random.default_rng(nlist + nq)
    list_off, probe = _ragged(rng, nlist, nprobe, nq)
    base, total, goff, gq, gbase = lt.group_probes(probe, list_off)
    # every pair by hand, then a literal (list, query) sort: a query's probes are distinct, so the pair order is total
    pairs = []
    for q in range(nq):
        at = 0
        for j in range(nprobe):
            l = int(probe[q, j])
            assert base[q, j] == at
            if 0 <= l < nlist:
                pairs.append((l, q, at))
                at += int(list_off[l + 1] - list_off[l])
        assert total[q] == at
    pairs.sort(key=lambda t: (t[0], t[1]))
    assert gq.tolist() == [p[1] for p in pairs] and gbase.tolist() == [p[2] for p in pairs]
    assert goff.tolist() == [sum(1 for p in pairs if p[0] < l) for l in range(nlist + 1)]
    assert (np.diff(gq[goff[0]:goff[1]]) > 0).all()                    # queries ascend inside a group


@pytest.mark.parametrize("nlist,nprobe,nq", [(1, 1, 3), (7, 2, 130), (7, 7, 257), (64, 9, 40)])
def test_tiles_cover_each_live_slot_once(nlist, nprobe, nq):
    rng = np.random.default_rng(7 * nlist + nq)
    list_off, probe = _ragged(rng, nlist, nprobe, nq)
    tiles = lt.row_tiles(list_off)
    sizes = np.diff(list_off)
    assert len(tiles) == int(((sizes + lt.ROWS - 1) // lt.ROWS).sum()) and set(tiles[:, 0].tolist()) == set(np.flatnonzero(sizes).tolist())
    for l, r0, rows in tiles:                                          # a tile stays inside its list
        assert list_off[l] <= r0 and r0 + rows <= list_off[l + 1] and 1 <= rows <= lt.ROWS and (r0 - list_off[l]) % lt.ROWS == 0
    W = tw.width(list_off, nprobe)
    hit, total = lt.fill_counts(probe, list_off, W)
    live = np.arange(W)[None, :] < total[:, None]
    assert np.array_equal(hit, live.astype(np.int64))


def test_tiled_candidate_rows_equal_section_26():
    rng = np.random.default_rng(3)
    nlist, nprobe, nq, L = 7, 3, 9, 40
    list_off, probe = _ragged(rng, nlist, nprobe, nq)
    N = int(list_off[-1])
    codes, inv = sq.encode(rng.integers(-6, 7, (N, L)).astype(np.float32))
    qc, iq = sq.encode(rng.integers(-6, 7, (nq, L)).astype(np.float32))
    ids = rng.permutation(N).astype(np.int32)
    want = tw.candidate_rows(qc, iq, probe, list_off, codes, inv, ids)
    got = lt.candidate_rows(qc, iq, probe, list_off, codes, inv, ids)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


def test_query_block_rule():
    assert lt.query_block(64, 100096, 256) == 64 and lt.query_block(1024, 1000192, 256) == 8          # the slots
    assert lt.query_block(100000, 1024, 1024) == 1024                                               # the pairs: 2^20 / 1024
    assert lt.query_block(257, 704, 7, 127) == 127 and lt.query_block(257, 704, 7, 1000) == 257 and lt.query_block(1, 64, 1) == 1


def test_lists_plan_host_rule_under_sanitizers(tmp_path):
    """csrc/bench/ivf_sq8_lists_plan_check.cpp includes only ivf_sq8_plan.hpp and runs as a stand-alone program under the address and
    undefined-behaviour sanitizers (nothing is loaded into Python): the query block, the row tiles and the pair capacity against
    literal values, then over a sweep that row tiles x query tiles write every live (query, slot) exactly once."""
    src = os.path.join(REPO, "python-visual-similarity_amd", "csrc", "bench", "ivf_sq8_lists_plan_check.cpp")
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (g++, c++ or clang++) on PATH"
    exe = str(tmp_path / "ivf_sq8_lists_plan_check")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ivf_sq8_lists_plan_check: ok" in run.stdout


def test_names_are_exported():
    import pvsim
    from pvsim import _ffi
    with open(os.path.join(REPO, "include", "pvsim.h")) as f:
        header = f.read()
    for name, nargs in (("pvs_ivf_sq8_group_probes_dev", 11), ("pvs_ivf_sq8_scan_lists_topk_dev", 17), ("pvs_ivf_sq8_scan_lists_plan", 7)):
        assert f"int {name}(" in header and len(_ffi.SIGNATURES[name]) == nargs
    assert len(_ffi.SIGNATURES["pvs_ivf_sq8_scan_topk_dev"]) == 17     # the scan by query keeps its arguments
    for method in ("ivf_sq8_group_probes_dev", "ivf_sq8_scan_lists_topk_dev", "ivf_sq8_scan_lists_plan"):
        assert callable(getattr(pvsim.Context, method))


def test_rank_refuses_scan_arguments_before_touching_a_device():
    from pvsim.index import _PathLedger
    from pvsim.ivf_int8 import IVFInt8Index
    index = IVFInt8Index.__new__(IVFInt8Index)                         # no device: the refusals come first
    index._ledger, index._L, index._ld = _PathLedger(("a", "b", "c")), 8, 64
    index._centroids = np.zeros((2, 8), np.float32)
    q = np.zeros((1, 8), np.float32)
    for bad in ("auto", "list", "", None, 1):
        with pytest.raises(ValueError, match='scan must be "queries" or "lists"'):
            index.rank(q, 1, 1, scan=bad)
    with pytest.raises(ValueError, match="slice_rows"):
        index.rank(q, 1, 1, slice_rows=16, scan="lists")
    with pytest.raises(ValueError, match="query_block"):
        index.rank(q, 1, 1, query_block=4)
    with pytest.raises(ValueError, match="query_block"):
        index.rank(q, 1, 1, scan="queries", query_block=4)
    import inspect
    p = inspect.signature(IVFInt8Index.rank).parameters
    assert list(p) == ["self", "query_vecs", "k", "nprobe", "slice_rows", "scan", "query_block"]
    assert p["scan"].default == "queries" and p["slice_rows"].default == 0 and p["query_block"].default == 0
