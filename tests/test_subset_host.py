"""CPU tests of subset search: the NumPy twin against a brute-force loop, the three forms of `allowed` in the
package and in the twin, the mask words, the refusals of the retrieval functions on objects that never touch a device, and the host
arithmetic of csrc/subset_common.hpp as a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import subset_numpy as tw
from conftest import REPO
from pvsim.subset import Subset, normalise        # the feature itself: without it nothing in this file can run


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_twin_equals_brute_force(seed):
    rng = np.random.default_rng(seed)
    nq, N = 4, 37
    scores = rng.integers(-3, 4, (nq, N)).astype(np.float32) / np.float32(4)        # many ties
    scores[0, 5], scores[0, 9] = np.float32(-0.0), np.float32(0.0)                  # -0 and +0 tie: the index decides
    for ids in ([0], [N - 1], list(range(0, N, 2)), [9, 5], list(range(N)), list(rng.permutation(N)[:11])):
        for k in sorted({1, min(2, len(ids)), len(ids)}):
            got_i, got_v = tw.restricted_topk(scores, ids, k)
            want_i, want_v = tw.brute_force(scores, ids, k)
            assert np.array_equal(got_i, want_i), (seed, ids, k)
            assert np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32)), (seed, ids, k)
            assert set(got_i.ravel().tolist()) <= set(ids)
    i, v = tw.restricted_topk(scores[:1], [9, 5], 2)
    assert i[0].tolist() == [5, 9] and not np.signbit(v).any()


def test_twin_full_set_is_the_plain_ranking():
    rng = np.random.default_rng(7)
    scores = rng.standard_normal((3, 50)).astype(np.float32)
    scores[:, 10] = scores[:, 20]
    i, v = tw.restricted_topk(scores, range(50), 50)
    for r in range(3):
        assert i[r].tolist() == np.lexsort((np.arange(50), -scores[r])).tolist()
        assert np.array_equal(v[r], scores[r][i[r]])


# ------------------------------------------------------------------------------------------------ allowed= in its three forms
PATHS = [f"img/{i:03d}.jpg" for i in range(12)]


def _both(allowed, n=12):
    """the package's normalise and the twin's on the same input: equal ids, or the same exception class"""
    pos = {p: i for i, p in enumerate(PATHS)}
    out = []
    for f in (lambda: normalise(allowed, n, pos.__getitem__), lambda: tw.normalise(allowed, n, PATHS)):
        try:
            out.append(f())
        except (ValueError, IndexError, KeyError, TypeError) as e:
            out.append(type(e))
    if isinstance(out[0], type) or isinstance(out[1], type):
        assert out[0] is out[1], out
        return out[0]
    assert out[0].dtype == np.int64 and out[1].dtype == np.int64 and np.array_equal(out[0], out[1])
    return out[0]


def test_normalise_three_forms_agree():
    want = [1, 4, 7, 11]
    mask = np.zeros(12, bool)
    mask[want] = True
    for form in (np.array([7, 1, 11, 4]), [11, 7, 4, 1], np.array([4, 1, 7, 11], np.int32), np.array(want, np.uint8), mask, mask.tolist(),
                 [PATHS[i] for i in (7, 11, 1, 4)], tuple(PATHS[i] for i in want), np.array([PATHS[i] for i in want])):
        assert _both(form).tolist() == want
    assert _both(np.ones(12, bool)).tolist() == list(range(12))
    assert _both([0]).tolist() == [0] and _both([PATHS[11]]).tolist() == [11]


def test_normalise_errors():
    assert _both([3, 5, 3]) is ValueError                       # a duplicate index
    assert _both(np.array([0, 12])) is IndexError               # an index equal to N
    assert _both([-1, 2]) is IndexError                         # negative indices do not wrap
    assert _both([PATHS[1], "img/nope.jpg"]) is KeyError        # an unknown path
    assert _both([PATHS[1], PATHS[1]]) is ValueError            # a path named twice
    assert _both([]) is ValueError                              # an empty set
    assert _both(np.zeros(12, bool)) is ValueError              # an empty mask
    assert _both(np.ones(11, bool)) is ValueError               # a mask of another length
    assert _both(np.zeros((2, 3), np.int64)) is ValueError      # not 1-d
    with pytest.raises(TypeError):
        normalise(np.array([0.5, 1.0]), 12)
    with pytest.raises(ValueError, match="empty"):
        normalise(np.zeros(0, np.int64), 12)
    with pytest.raises(IndexError, match="12"):
        normalise([12], 12)
    with pytest.raises(ValueError, match="subset_path"):
        from pvsim.subset import _path_code
        _path_code("fast")


@pytest.mark.parametrize("N", [1, 31, 32, 33, 64, 65])
def test_bitmask_words(N):
    rng = np.random.default_rng(N)
    for ids in ([0], [N - 1], list(range(N)), list(range(0, N, 2)), sorted(rng.permutation(N)[:max(1, N // 3)].tolist())):
        words = tw.bitmask(ids, N)
        assert words.dtype == np.uint32 and words.shape == ((N + 31) // 32,)
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")              # bit i & 31 of word i >> 5, little-endian words
        assert np.flatnonzero(bits).tolist() == sorted(ids)
        assert not bits[N:].any()                                                  # the bits beyond N are zero


def test_stats_twin_counts_panels_and_chunks():
    ids = [i for i in range(200) if not 48 <= i < 128]
    assert tw.mask_stats(ids, 130, 200, 48, 48) == [1, 3 * 4, 3 * 1, 0]           # [48, 96) holds no id; [96, 144) holds 128..143
    assert tw.mask_stats(ids, 130, 200, 64, 64) == [1, 3 * 3, 3 * 1, 0]           # [64, 128) holds no id
    assert tw.mask_stats(ids, 5, 200, 5, 200) == [1, 1, 0, 0]
    assert tw.listed_stats(120, 48) == [2, 3, 0, 120] and tw.listed_stats(48, 48) == [2, 1, 0, 48]


# ------------------------------------------------------------------------------------------------ refusals that need no device
class _Encoder:
    def encode(self, image):
        raise AssertionError("a refusal must come before anything is encoded")


def _bare(cls):
    return cls.__new__(cls)                # no context, no device: the refusal reads the type alone


def test_eval_refuses_allowed_with_every_second_stage_and_unbuilt_index():
    from pvsim import eval as ev
    from pvsim.asmk import ASMKIndex
    from pvsim.compact import CompactIndex, IVFCompactIndex
    from pvsim.expand import QueryExpansion
    d = {p: np.ones(4, np.float32) for p in PATHS}
    labels = {p: 0 for p in PATHS}
    img = np.zeros((2, 2, 3), np.uint8)
    for kw, name in ((dict(expand=QueryExpansion()), "expand"), (dict(rerank=5), "rerank"), (dict(nprobe=2), "nprobe"),
                     (dict(diffuse=object()), "diffuse"), (dict(reciprocal=object()), "reciprocal")):
        with pytest.raises(ValueError, match=f"allowed= together with {name}= is not built"):
            ev.retrieve_top_k_similar(img, d, _Encoder(), k=3, allowed=[0, 1], **kw)
        with pytest.raises(ValueError, match=f"{name}= is not built"):
            ev.top_k_map([img], [0], d, labels, _Encoder(), k=3, allowed=[0, 1], **kw)
        with pytest.raises(ValueError, match=f"{name}= is not built"):
            ev.top_k_accuracy([img], [0], d, labels, _Encoder(), k=3, allowed=[0, 1], **kw)
    for cls in (CompactIndex, IVFCompactIndex, ASMKIndex):
        with pytest.raises(ValueError, match=f"allowed= on an? {cls.__name__} is not built"):
            ev.retrieve_top_k_similar(img, _bare(cls), _Encoder(), k=3, allowed=[0, 1])
    with pytest.raises(ValueError, match="Subset"):                       # a Subset belongs to an index, a dict has none
        ev._plan(d, allowed=_bare(Subset))


def test_eval_on_a_dict_cuts_the_map_before_ranking(monkeypatch):
    """the plan of a dict holds the allowed rows alone, in index order, so the existing path ranks exactly them; k=None is refused by name"""
    from pvsim import eval as ev
    rng = np.random.default_rng(3)
    d = {p: rng.standard_normal(6).astype(np.float32) for p in PATHS}
    seen = {}

    def fake_rank(q, matrix, k, ctx=None):
        seen["matrix"], seen["k"] = matrix, k
        kk = min(k, matrix.shape[0])
        return np.tile(np.arange(kk), (q.shape[0], 1)), np.zeros((q.shape[0], kk), np.float32)
    monkeypatch.setattr(ev, "_rank", fake_rank)
    for allowed in ([7, 2, 9], [PATHS[9], PATHS[2], PATHS[7]], np.isin(np.arange(12), [2, 7, 9])):
        plan = ev._plan(d, allowed=allowed)
        assert plan.n == 3 and plan.paths == [PATHS[2], PATHS[7], PATHS[9]]
        idx, _ = plan.rank(np.ones((1, 6), np.float32), 5)
        assert np.array_equal(seen["matrix"], np.stack([d[PATHS[i]] for i in (2, 7, 9)])) and idx.shape == (1, 3)
        with pytest.raises(ValueError, match="k=None is not built"):
            plan.rank(np.ones((1, 6), np.float32), None)
    with pytest.raises(KeyError):
        ev._plan(d, allowed=["img/nope.jpg"])
    with pytest.raises(IndexError):
        ev._plan(d, allowed=[12])
    with pytest.raises(ValueError):
        ev._plan(d, allowed=[])


def test_subset_is_exported_and_bound():
    import pvsim
    from pvsim import _ffi
    assert pvsim.Subset is __import__("pvsim.subset", fromlist=["Subset"]).Subset and "Subset" in pvsim.__all__
    for name in ("pvs_subset_create", "pvs_subset_destroy", "pvs_cosine_topk_subset_dev", "pvs_sq8_topk_subset_dev"):
        assert name in _ffi.SIGNATURES
    import inspect
    from pvsim.index import DeviceIndex
    from pvsim.quantized import Int8Index
    for cls in (DeviceIndex, Int8Index):
        p = inspect.signature(cls.rank).parameters
        assert list(p)[1:] == ["query_vecs", "k", "allowed", "subset_path"] and p["allowed"].default is None and p["subset_path"].default == "auto"
        assert callable(cls.subset)


# ------------------------------------------------------------------------------------------------ the host arithmetic, sanitized
def test_subset_common_host_arithmetic_under_sanitizers(tmp_path):
    """csrc/bench/subset_plan_check.cpp includes only subset_common.hpp and runs as a stand-alone program under the address and
    undefined-behaviour sanitizers (nothing is loaded into Python): the mask words bit by bit, the 64-column window for every
    col0 % 32 and every lane, the chunks tiling [0, ns) exactly once, the empty-panel test against a linear scan, the id check."""
    src = os.path.join(REPO, "python-visual-similarity_amd", "csrc", "bench", "subset_plan_check.cpp")
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (g++, c++ or clang++) on PATH"
    exe = str(tmp_path / "subset_plan_check")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "subset_plan_check: ok" in run.stdout
