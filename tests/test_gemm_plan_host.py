"""Host tests of the similarity GEMMs' launch plan and of the twins tests/test_gpu_gemm_plans.py compares the kernels with
(DESIGN.md section 27).  The plan rule (csrc/gemm_plan.hpp) runs as a stand-alone program under the address and undefined-behaviour
sanitizers; the twins of oracle/pvsim_oracle.c are checked against each other and against a long double sum.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pvsim_oracle_c as orc_c
from conftest import REPO


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ------------------------------------------------------------------------------------------------ the plan rule, sanitized
def test_plan_rule_under_sanitizers(tmp_path):
    """csrc/bench/gemm_plan_check.cpp includes only gemm_plan.hpp and runs as a stand-alone program under the sanitizers (nothing is
    loaded into Python).  tiles_m, tiles_n in 1..40, both forms, slots in {1, 2, 4, 7, 64, 256, 512}: every tile listed exactly once
    (the symmetric form lists exactly tn >= tm), n_main + n_tail == total, n_main a multiple of the slots in front of a tail, the
    split a power of two in 1..32; at 512 slots the plans and the tile order of the shipped workloads (64 x 64 symmetric, 16 x 64
    general) are the literals recorded from the rule as it stood inside build_plan."""
    src = os.path.join(REPO, "python-visual-similarity_amd", "csrc", "bench", "gemm_plan_check.cpp")
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (g++, c++ or clang++) on PATH"
    exe = str(tmp_path / "gemm_plan_check")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "gemm_plan_check: ok" in run.stdout


def test_plan_header_is_host_only_and_the_launcher_keeps_no_copy_of_the_rule():
    csrc = os.path.join(REPO, "python-visual-similarity_amd", "csrc")
    with open(os.path.join(csrc, "gemm_plan.hpp")) as f:
        hdr = f.read()
    assert "hip" not in re.sub(r"//.*", "", hdr).lower()                  # no HIP header, type or qualifier outside the comments
    with open(os.path.join(csrc, "cosine.hip")) as f:
        src = f.read()
    assert "gemm_plan_tiles(" in src and "gemm_plan_cut(" in src and "sk *= 2" not in src


def test_option_and_read_back_are_declared_alike_in_header_and_binding():
    from pvsim import _ffi
    with open(os.path.join(REPO, "include", "pvsim.h")) as f:
        header = f.read()
    with open(os.path.join(REPO, "include", "pvsim_diag.h")) as f:
        diag = f.read()
    assert re.search(r"PVS_OPT_GEMM_SLOTS = (\d+)", header).group(1) == str(_ffi.OPT_GEMM_SLOTS)
    assert int(re.search(r"PVS_OPT_COUNT_ = (\d+)", header).group(1)) == _ffi.OPT_GEMM_SLOTS + 1      # the last one before the count
    for name, value in (("EXACT_F32", _ffi.GEMM_EXACT_F32), ("F16_256", _ffi.GEMM_F16_256), ("F16_BOUNDED", _ffi.GEMM_F16_BOUNDED),
                        ("F64", _ffi.GEMM_F64), ("F16_2LVL", _ffi.GEMM_F16_2LVL), ("GENERIC", _ffi.GEMM_GENERIC)):
        assert re.search(rf"PVS_GEMM_MODEL_{name} = (\d+)", diag).group(1) == str(value)
    assert re.search(r"PVS_GEMM_TAIL_UNSPLIT_BYTES = (\d+)", diag).group(1) == str(_ffi.GEMM_TAIL_UNSPLIT_BYTES)
    assert re.search(r"PVS_GEMM_TAIL_UNSPLIT_ONE_SLICE = (\d+)", diag).group(1) == str(_ffi.GEMM_TAIL_UNSPLIT_ONE_SLICE)
    assert "pvs_gemm_last_plan" in diag and "pvs_gemm_last_plan" not in header                         # diagnostic, not product ABI
    assert len(_ffi.GEMM_PLAN_FIELDS) == 12 and "pvs_gemm_last_plan" in _ffi.SIGNATURES
    for name in ("pvs_diag_poison", "pvs_diag_ws_bytes"):                                              # recycled-memory diagnostics
        assert name in diag and name not in header and name in _ffi.SIGNATURES
    functions = set(re.findall(r"\b(pvs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", diag, flags=re.S)))
    assert functions == {"pvs_fused_profile", "pvs_gemm_last_plan", "pvs_diag_poison", "pvs_diag_ws_bytes"}
    with open(os.path.join(REPO, "python-visual-similarity_amd", "csrc", "workspace.hpp")) as f:
        enum = re.search(r"enum WsSlot : int \{(.*?)\};", f.read(), flags=re.S).group(1)
    slots = sorted(re.findall(r"(WS_[A-Z0-9_]+) = (\d+)", enum), key=lambda kv: int(kv[1]))
    assert tuple(n for n, _ in slots) == _ffi.WS_SLOTS and [int(v) for _, v in slots] == list(range(18))


# ------------------------------------------------------------------------------------------------ the twins
@pytest.mark.parametrize("L", [40, 1024, 2600, 4096])
def test_whole_matrix_chain_twin_equals_the_pair_form(L):
    """orc_cosine_chain (the definition, pair by pair) and its whole-matrix form give the same bits: on 500 sampled pairs, and on
    every pair of a corner block; with factors and without."""
    rng = np.random.default_rng(L)
    a = rng.standard_normal((37, L)).astype(np.float32)
    b = rng.standard_normal((29, L)).astype(np.float32)
    a[5] = 0
    ia = rng.uniform(0.5, 2, 37).astype(np.float32)
    ib = rng.uniform(0.5, 2, 29).astype(np.float32)
    pairs = np.stack([rng.integers(0, 37, 500), rng.integers(0, 29, 500)], axis=1)
    block = np.stack(np.meshgrid(np.arange(30, 37), np.arange(22, 29), indexing="ij"), axis=-1).reshape(-1, 2)
    pairs = np.concatenate([pairs, block])
    for fa, fb in ((ia, ib), (None, None), (ia, None)):
        full = orc_c.cosine_chain_full(a, b, fa, fb)
        assert full.shape == (37, 29) and full.dtype == np.float32
        assert np.array_equal(_bits(full[pairs[:, 0], pairs[:, 1]]), _bits(orc_c.cosine_chain(a, b, fa, fb, pairs)))
        assert (full[5] == 0).all()
    same = orc_c.cosine_chain_full(a, a, ia, ia)
    assert np.array_equal(_bits(same), _bits(same.T.copy()))              # fmaf(a, b, c) == fmaf(b, a, c): the definition is symmetric


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("L", [1, 2, 15, 37, 1001])
def test_sequential_twins_against_the_long_double_dot(dtype, L):
    """|twin - sum_k a_k b_k| <= (L - 1) u sum_k |a_k b_k| with u = 2^-24 / 2^-53 and the sums in long double.  The twin rounds once
    per fused multiply-add, L times in all; the bound counts the L - 1 additions, so it is a bound only where the first step -- the
    product added to zero -- is exact.  Column 0 therefore holds multiples of 2^-8 below 8 (11 significant bits: the product of two
    fits a float32); the other columns are normal deviates.  At L = 1 the bound is zero and the twin must be exact."""
    rng = np.random.default_rng(1000 + L)
    a = rng.standard_normal((19, L)).astype(dtype)
    b = rng.standard_normal((23, L)).astype(dtype)
    a[:, 0] = rng.integers(-2047, 2048, 19) / 256.0
    b[:, 0] = rng.integers(-2047, 2048, 23) / 256.0
    u = np.longdouble(2.0) ** (-24 if dtype == np.float32 else -53)
    got = orc_c.cosine_seq(a, b, None, None)
    assert got.dtype == dtype and got.shape == (19, 23)
    dot, mag = orc_c.dot_abs_ld(a, b)
    err = np.abs(got.astype(np.longdouble) - dot)
    assert (err <= (L - 1) * u * mag).all(), float((err / np.maximum((L - 1) * u * mag, np.finfo(np.longdouble).tiny)).max())
    # the long double sums themselves: exact on integers, and mag >= |dot|
    ai, bi = rng.integers(-50, 51, (4, L)), rng.integers(-50, 51, (5, L))
    d2, m2 = orc_c.dot_abs_ld(ai.astype(dtype), bi.astype(dtype))
    assert np.array_equal(d2, (ai @ bi.T).astype(np.longdouble)) and np.array_equal(m2, (np.abs(ai) @ np.abs(bi).T).astype(np.longdouble))
    assert (mag >= np.abs(dot)).all()
    # the factors: one product of the two, one product with the sum, each rounded once; a null factor is 1
    ia = rng.uniform(0.5, 2, 19).astype(dtype)
    ib = rng.uniform(0.5, 2, 23).astype(dtype)
    assert np.array_equal(_bits(orc_c.cosine_seq(a, b, ia, ib)), _bits(got * (ia[:, None] * ib[None, :])))
    assert np.array_equal(_bits(orc_c.cosine_seq(a, b, ia, None)), _bits(got * (ia[:, None] * np.ones(23, dtype)[None, :])))
