"""CPU tests of index maintenance: the NumPy twin (tests/update_numpy.py) against the obvious definitions --
np.cumsum, np.delete and dict / list deletion, pvsim.compact._sort_into_lists on the concatenated list numbers -- and the argument
validation of add / remove that needs no device.  The kernels are held to the twin in tests/test_gpu_update.py."""
import numpy as np
import pytest

import update_numpy as up


@pytest.fixture(scope="session", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def _masks(rng, n):
    """keep masks of n entries: random at three densities, all, none, first / last removed, alternating"""
    out = [(rng.random(n) < p).astype(np.uint8) for p in (0.1, 0.5, 0.9)] + [np.ones(n, np.uint8), np.zeros(n, np.uint8)]
    if n:
        for i in (0, n - 1):
            k = np.ones(n, np.uint8)
            k[i] = 0
            out.append(k)
        out.append((np.arange(n) % 2).astype(np.uint8))
    return out


# ------------------------------------------------------------------------------------------------ keep positions, compaction
@pytest.mark.parametrize("tile", [4, 8, 2048])
def test_keep_positions_equal_the_exclusive_cumsum(tile):
    rng = np.random.default_rng(1500 + tile)
    for n in (0, 1, tile - 1, tile, tile + 1, 3 * tile + 5, min(tile * tile + 1, 70000), min(tile ** 3, 5000)):
        for keep in _masks(rng, n):
            want = np.concatenate([[0], np.cumsum(keep != 0)]).astype(np.int64)
            got = up.keep_positions(keep * 7, tile)                 # any non-zero byte keeps
            assert got.dtype == np.int64 and np.array_equal(got, want), (tile, n)


def test_keep_mask_is_fill_and_scatter():
    assert up.keep_mask([], 0).size == 0 and up.keep_mask([], 5).tolist() == [1] * 5
    assert up.keep_mask([4, 0, 4, -1, 5], 5).tolist() == [0, 1, 1, 1, 0]


@pytest.mark.parametrize("row_shape", [(), (1,), (3,), (16,)])
def test_compaction_equals_np_delete(row_shape):
    rng = np.random.default_rng(1510)
    for n in (0, 1, 2, 65, 300):
        rows = rng.integers(0, 256, (n,) + row_shape).astype(np.uint8)
        for keep in _masks(rng, n):
            pos = up.keep_positions(keep)
            want = np.delete(rows, np.flatnonzero(keep == 0), axis=0)
            assert np.array_equal(up.compact_rows(rows, keep, pos), want)
            removed = np.flatnonzero(keep == 0)
            first = int(removed[0]) if removed.size else n
            for window in (1, 7, 64, 1000):
                for f in (0, first):
                    buf = rows.copy()
                    up.compact_rows_in_place(buf, keep, pos, f, window)
                    assert np.array_equal(buf[:len(want)], want) and np.array_equal(buf[:first], rows[:first])


def test_removal_follows_dict_deletion():
    rng = np.random.default_rng(1511)
    d = {f"img/{i}.jpg": rng.integers(0, 99, 4) for i in range(40)}
    gone = [f"img/{i}.jpg" for i in (39, 0, 17, 18)]
    keep = up.keep_mask([list(d).index(p) for p in gone], len(d))
    rows = up.compact_rows(np.array(list(d.values())), keep, up.keep_positions(keep))
    for p in gone:
        del d[p]
    assert np.array_equal(rows, np.array(list(d.values())))
    from pvsim.index import _compact_host_rows, _compact_list, _removed_indices
    paths = [f"img/{i}.jpg" for i in range(40)]
    idx = _removed_indices(gone, {p: i for i, p in enumerate(paths)})
    assert idx.tolist() == [0, 17, 18, 39] and _compact_list(paths, idx) == list(d)
    buf = np.arange(80).reshape(40, 2)
    want = np.delete(buf, idx, axis=0)
    _compact_host_rows(buf, 40, idx)
    assert np.array_equal(buf[:36], want)


def test_path_ledger_follows_a_dict():
    """pvsim.index._PathLedger (paths <-> positions of every mutable index) against a plain dict given the same adds and removes"""
    from pvsim.index import _PathLedger
    rng = np.random.default_rng(1512)
    names = [f"img/{i}.jpg" for i in range(200)]
    d = dict.fromkeys(names[:60])
    ledger = _PathLedger(names[:60])

    def same():
        live = list(d)
        assert ledger.paths == live and len(ledger) == len(live)
        assert [ledger.index_of(p) for p in live] == list(range(len(live)))
        for p in names:
            assert (p in ledger) == (p in d)
            if p not in d:
                with pytest.raises(KeyError):
                    ledger.index_of(p)

    def add(paths):
        ledger.check_new(paths)
        ledger.append(paths)
        d.update(dict.fromkeys(paths))
        same()

    def remove(paths):
        idx = ledger.removed_indices(paths)
        assert idx.dtype == np.int64 and idx.tolist() == sorted(list(d).index(p) for p in paths)
        ledger.remove(idx)
        for p in paths:
            del d[p]
        same()

    same()
    remove([names[0]])                                              # the first path, then the last
    remove([names[59]])
    add([])
    remove([])
    add(names[60:93])                                               # 33 paths
    remove(names[90:93])                                            # right behind the add that brought them
    add([names[0]])                                                 # a removed path comes back, in the last place
    assert ledger.paths[-1] == names[0] and ledger.index_of(names[0]) == len(d) - 1
    for step in range(45):                                          # mixed: 0, 1, 33 new paths; 0, 1 or scattered removed ones
        absent = [p for p in names if p not in d]
        b = min((0, 1, 33)[step % 3], len(absent))
        add([absent[i] for i in rng.permutation(len(absent))[:b]])
        live = list(d)
        r = min((1, 0, int(rng.integers(2, 20)))[step % 3], len(live))
        remove([live[i] for i in rng.permutation(len(live))[:r]])
    # the four refusals leave everything as it was
    live, absent = list(d), [p for p in names if p not in d]
    for bad, exc, match in ((lambda: ledger.check_new([absent[0], live[3]]), ValueError, "is already indexed"),
                            (lambda: ledger.check_new([absent[0], absent[1], absent[0]]), ValueError, "named twice in one add"),
                            (lambda: ledger.removed_indices([live[0], absent[0]]), KeyError, None),
                            (lambda: ledger.removed_indices([live[0], live[1], live[0]]), ValueError, "named twice in one remove")):
        with pytest.raises(exc, match=match):
            bad()
        same()
    assert ledger.removed_indices(live[5]).tolist() == [5]          # one path as a string


# ------------------------------------------------------------------------------------------------ inverted lists
def _stored(rng, lists, nlist, m):
    """an index's storage from the list number of every row, by the product's own host sort"""
    from pvsim.compact import _sort_into_lists
    n = lists.size
    codes, inv = rng.integers(0, 256, (n, m)).astype(np.uint8), rng.random(n).astype(np.float32)
    ids, off = _sort_into_lists(lists, nlist)
    return codes, inv, codes[ids], inv[ids], ids, off


def _list_cases(rng, nlist, n):
    yield rng.integers(0, nlist, n)
    yield np.zeros(n, np.int64)
    yield np.full(n, nlist - 1)
    yield np.full(n, nlist // 2)
    yield rng.choice(np.arange(nlist)[::3], n) if nlist >= 3 else np.zeros(n, np.int64)      # two of three lists stay empty


@pytest.mark.parametrize("nlist,m", [(1, 1), (7, 3), (7, 8), (300, 8)])
def test_insert_equals_a_sort_of_the_concatenated_list_numbers(nlist, m):
    from pvsim.compact import _sort_into_lists
    rng = np.random.default_rng(1520 + nlist + m)
    for n in (0, 1, 50):
        for b in (0, 1, 33):
            for old_lists in _list_cases(rng, nlist, n):
                for new_lists in _list_cases(rng, nlist, b):
                    codes, inv, s_codes, s_inv, ids, off = _stored(rng, old_lists, nlist, m)
                    new_codes, new_inv = rng.integers(0, 256, (b, m)).astype(np.uint8), rng.random(b).astype(np.float32)
                    perm, new_off = up.sort_new_rows(new_lists, nlist)
                    p2, o2 = _sort_into_lists(new_lists.astype(np.int64), nlist)
                    assert np.array_equal(perm, p2) and np.array_equal(new_off, o2)
                    got = up.ivf_insert(s_codes, s_inv, ids, off, new_codes, new_inv, new_off, perm)
                    all_codes, all_inv = np.concatenate([codes, new_codes]), np.concatenate([inv, new_inv])
                    w_ids, w_off = _sort_into_lists(np.concatenate([old_lists, new_lists]).astype(np.int64), nlist)
                    for g, w in zip(got, (all_codes[w_ids], all_inv[w_ids], w_ids, w_off)):
                        assert g.dtype == w.dtype and np.array_equal(g, w)


@pytest.mark.parametrize("nlist,m", [(1, 1), (7, 3), (7, 8), (300, 8)])
def test_remove_equals_a_sort_of_the_surviving_list_numbers(nlist, m):
    from pvsim.compact import _sort_into_lists
    rng = np.random.default_rng(1530 + nlist + m)
    for n in (0, 1, 2, 60):
        for lists in _list_cases(rng, nlist, n):
            codes, inv, s_codes, s_inv, ids, off = _stored(rng, lists, nlist, m)
            masks = _masks(rng, n)
            if n > 3:
                k = np.ones(n, np.uint8)
                k[[0, 1, n - 2, n - 1]] = 0                        # adjacent removed ids at both ends
                masks.append(k)
                k = np.ones(n, np.uint8)
                k[lists == lists[0]] = 0                           # one list emptied
                masks.append(k)
            for keep in masks:
                got = up.ivf_remove(s_codes, s_inv, ids, off, keep)
                left = np.flatnonzero(keep)
                w_ids, w_off = _sort_into_lists(lists[left].astype(np.int64), nlist)
                for g, w in zip(got, (codes[left][w_ids], inv[left][w_ids], w_ids, w_off)):
                    assert g.dtype == w.dtype and np.array_equal(g, w)
                # the id remap is the exclusive cumsum of the mask
                remap = np.concatenate([[0], np.cumsum(keep)])[:-1]
                assert np.array_equal(np.sort(got[2]), np.sort(remap[left]))


# ------------------------------------------------------------------------------------------------ validation that needs no device
def _stub_ivf(rng, n=30, nlist=4, m=2, dsub=2, ksub=8, L=9):
    from pvsim import IVFCompactIndex, ProductQuantizer
    from pvsim.compact import _sort_into_lists
    d = m * dsub
    cb = rng.standard_normal((m, ksub, dsub)).astype(np.float32)
    ids, off = _sort_into_lists(rng.integers(0, nlist, n), nlist)
    w = rng.standard_normal((d, L)).astype(np.float32)
    return IVFCompactIndex([f"p{i}" for i in range(n)], rng.integers(0, ksub, (n, m)).astype(np.uint8), np.ones(n, np.float32),
                           ProductQuantizer.from_codebooks(cb), rng.standard_normal((nlist, d)).astype(np.float32), off, ids, w,
                           rng.standard_normal((n, d)).astype(np.float32))


def _stub_flat(rng, n=30, m=2, dsub=2, ksub=8):
    from pvsim import CompactIndex, ProductQuantizer
    cb = rng.standard_normal((m, ksub, dsub)).astype(np.float32)
    return CompactIndex([f"p{i}" for i in range(n)], rng.integers(0, ksub, (n, m)).astype(np.uint8), np.ones(n, np.float32),
                        ProductQuantizer.from_codebooks(cb))


def test_compact_index_update_validation_touches_no_device():
    rng = np.random.default_rng(1540)
    for index, L in ((_stub_flat(rng), 4), (_stub_ivf(rng), 9)):
        row = np.zeros(L, np.float32)
        with pytest.raises(ValueError, match="'p3' is already indexed"):
            index.add({"new": row, "p3": row})
        with pytest.raises(ValueError, match=f"the index takes {L}"):
            index.add({"new": np.zeros(L + 1, np.float32)})
        with pytest.raises(TypeError, match="float32"):
            index.add({"new": row.astype(np.float64)})
        with pytest.raises(KeyError):
            index.remove(["p1", "nope"])
        with pytest.raises(ValueError, match="'p1' is named twice"):
            index.remove(["p1", "p2", "p1"])
        with pytest.raises(KeyError):
            del index["nope"]
        index.add({})                                               # empty operations are no-ops: no device is needed for them
        index.remove([])
        assert len(index) == 30 and index.paths == [f"p{i}" for i in range(30)] and index._dev is None
    ivf = _stub_ivf(rng)
    with pytest.raises(ValueError, match="fewer than 2\\^31 rows"):
        ivf._check_size(2 ** 31)
    ivf._check_size(2 ** 31 - 1)
    assert np.array_equal(ivf._ids, np.sort(ivf._ids)[np.argsort(np.argsort(ivf._ids))])        # the host copy is there before an upload


def test_device_index_update_validation_touches_no_device():
    from pvsim.index import DeviceIndex, _PathLedger
    index = DeviceIndex.__new__(DeviceIndex)                        # the surface without a context: paths and the host mirror only
    index._ledger = _PathLedger(["a", "b", "c"])
    index._hbuf = np.arange(12, dtype=np.float32).reshape(3, 4)
    index._pending, index._mirror_rows, index._cap = [], 3, 3
    row = np.zeros(4, np.float32)
    with pytest.raises(ValueError, match="'b' is already indexed"):
        index.add({"d": row, "b": row})
    with pytest.raises(ValueError, match="the index's length 4"):
        index.add({"d": np.zeros(5, np.float32)})
    with pytest.raises(TypeError, match="float32 index takes float32"):
        index.add({"d": row.astype(np.float64)})
    with pytest.raises(KeyError):
        index.remove(["a", "z"])
    with pytest.raises(ValueError, match="named twice"):
        index.remove(["a", "a"])
    with pytest.raises(KeyError):
        del index["z"]
    index.add({})
    index.remove([])
    assert list(index) == ["a", "b", "c"] and index.capacity == 3 and np.array_equal(index.matrix, index._hbuf)
    # the host mirror follows lazily: notes of removes and of the adds behind them, applied in order when host rows are asked for
    rows = {p: np.full(4, i, np.float32) for i, p in enumerate("defgh")}
    index._pending = [("remove", np.array([0, 2])), ("add", np.stack([rows["d"], rows["e"]])), ("remove", np.array([1])),
                      ("add", np.stack([rows["f"]]))]
    index._ledger, index._cap = _PathLedger(["b", "e", "f"]), 8
    assert np.array_equal(index.matrix, np.stack([np.arange(4, 8, dtype=np.float32), rows["e"], rows["f"]]))
    assert index._pending == [] and index._mirror_rows == 3 and index._hbuf.shape[0] == 3


def test_list_core_host_rules(tmp_path):
    """csrc/bench/list_common_check.cpp includes only list_common.hpp and runs as a stand-alone program under the address and
    undefined-behaviour sanitizers (nothing is loaded into Python): byte ranges that touch, share a byte or are null or empty; the
    offset predicates on good and bad arrays; the score slice, the expand tile and the invert tile against the expressions the entry
    points carried inline, over a grid of inputs, with the invariants the kernels rely on."""
    import os
    import shutil
    import subprocess
    from conftest import REPO
    src = os.path.join(REPO, "python-visual-similarity_amd", "csrc", "bench", "list_common_check.cpp")
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (g++, c++ or clang++) on PATH"
    exe = str(tmp_path / "list_common_check")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr


def test_header_binding_and_constants_agree():
    import os
    import re
    from conftest import REPO
    from pvsim import _ffi
    header = open(os.path.join(REPO, "include", "pvsim.h")).read()
    assert int(re.search(r"#define PVS_SCAN_TILE (\d+)", header).group(1)) == _ffi.SCAN_TILE == up.SCAN_TILE
    assert re.search(r"PVS_OPT_UPDATE_WINDOW_ROWS = (\d+)", header).group(1) == str(_ffi.OPT_UPDATE_WINDOW_ROWS)
    for name, nargs in (("pvs_keep_mask_dev", 5), ("pvs_keep_positions_dev", 4), ("pvs_compact_rows_dev", 8), ("pvs_ivf_insert_dev", 17),
                        ("pvs_ivf_remove_dev", 14), ("pvs_copy_dev", 4)):
        assert f"int {name}(" in header and len(_ffi.SIGNATURES[name]) == nargs and hasattr(_ffi.lib(), name)
