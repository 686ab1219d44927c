"""The similarity GEMMs under every launch plan, at small shapes (through the C-ABI).

Which kernels a GEMM call launches is decided by the host rule of csrc/gemm_plan.hpp from the tile count and the workgroup slots
of the chip.  PVS_OPT_GEMM_SLOTS pins the slots, so three or four tiles reach every plan -- whole tiles only, full rounds + a
split-K tail, every tile split -- and pvs_gemm_last_plan reads back what was launched: every case below asserts the plan it is
named for before it looks at a number, and fails if the read-back shows another one.

  * exact fp32 (pvs_cosine_dev, pvs_cosine_dual_dev): the WHOLE matrix, bit for bit, against the chain twin (orc_cosine_chain_full);
  * generic tile kernel (f32 and f64): bit for bit against the sequential twins (orc_cosine_seq_*);
  * f64 on the matrix pipe: within (L + 3) 2^-52 sum|a_k b_k| ia ib of the long double dot (the k order is defined, how one
    v_mfma_f64_16x16x4_f64 adds its four products is not; scores depend on the split, so the bound is asserted under each plan);
  * fp16 256 x 256 (8-phase main, two-stage split tail): within (L + 2) 2^-23 sum|a_k b_k| ia ib of the long double dot of the
    fp16-rounded operands (products of two halfs are exact in fp32);
  * bounded fp16 prefilter (128 x 128 and the 256 x 128 two-level kernel, one segment and two accumulated ones): the filtered
    top-k gives the exact path's indices and score bits;
  * row norms: within (L + 8) u of the long double value.

Outputs are pre-filled with 0xff bytes (a NaN no kernel produces); a leading dimension larger than the row keeps them in the
padding.  Out of scope: the unsplit fallback of a tail whose partial images exceed 1 GiB (it needs gigabytes of operands) and the
multi-GPU communicator entry points."""
import functools

import numpy as np
import pytest

import pvsim_oracle_c as orc_c
from pvsim import _ffi

pytestmark = pytest.mark.gpu

EXACT, F16_256, F16_BOUNDED, F64, F16_2LVL, GENERIC = range(6)
LD = np.longdouble


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _up(ctx, a):
    a = np.ascontiguousarray(a)
    return ctx.buffer(max(a.nbytes, 16)).upload(a)


def _expect(ctx, what, **want):
    """the read-back of the last GEMM must show the named plan"""
    plan = ctx.gemm_last_plan()
    got = {k: plan[k] for k in want}
    assert got == want, f"{what}: launched {plan}, the case needs {want}"
    return plan


def _padded(ctx, rows, ld, itemsize=4):
    return ctx.buffer(rows * ld * itemsize).fill_bytes(0xff)


def _take(buf, rows, cols, ld, dtype):
    """(inside, padding) of a rows x ld output"""
    full = buf.download((rows, ld), dtype)
    return np.ascontiguousarray(full[:, :cols]), full[:, cols:]


def _assert_padding_kept(pad):
    b = _bits(pad)
    assert (b == np.iinfo(b.dtype).max).all(), "a store went past the end of a row"


# ====================================================================================================== inputs and twins, built once
@functools.lru_cache(maxsize=None)
def _rows(M, L, seed):
    """float32 rows with a zero row and rows scaled by 1e+3 / 1e-3"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, L)).astype(np.float32)
    if M > 6:
        x[2] = 0
        x[4] *= np.float32(1e3)
        x[5] *= np.float32(1e-3)
    x.setflags(write=False)
    return x


_CHAIN = {}


def _chain_twin(key, a, b, ia, ib):
    if key not in _CHAIN:
        t = orc_c.cosine_chain_full(a, b, ia, ib)
        t.setflags(write=False)
        _CHAIN[key] = t
    return _CHAIN[key]


def _device_norms(ctx, d_x, rows, L):
    inv = ctx.buffer(rows * 4)
    ctx.row_inv_norms_dev(d_x.ptr, rows, L, inv.ptr)
    ctx.sync()
    return inv, inv.download((rows,), np.float32)


# ====================================================================================================== exact fp32
# (name, M, N, ((slots, n_main, n_tail, plan split), ...)): the cuts are the literals of csrc/bench/gemm_plan_check.cpp
GENERAL = [
    ("3x3 tiles, M = 1 and N = 127 mod 128", 257, 383, ((1, 9, 0, 1), (4, 8, 1, 4), (64, 0, 9, 16))),
    ("4x3 tiles, M = 1 mod 128", 385, 300, ((5, 10, 2, 2), (7, 7, 5, 4), (64, 0, 12, 16))),
    ("1x3 tiles, every tile in two slices", 100, 384, ((2, 2, 1, 2), (6, 0, 3, 2), (64, 0, 3, 16))),
]
SYMMETRIC = [
    ("3x3 tiles, N = 0 mod 128", 384, ((1, 6, 0, 1), (4, 4, 2, 2), (64, 0, 6, 8))),
    ("3x3 tiles, N = 1 mod 128", 257, ((1, 6, 0, 1), (4, 4, 2, 2), (64, 0, 6, 8))),
    ("2x2 tiles, N = 127 mod 128", 255, ((1, 3, 0, 1), (64, 0, 3, 16))),
]
EXACT_L = [40, 1024, 2600, 4096]        # one short chain / one chain / two chains + 552 with a partial last k-tile / four chains


def _chains(L):
    return -(-L // 1024)


def _exact_plan(ctx, what, tiles_m, tiles_n, symm, dual, n_main, n_tail, split, L):
    """read-back of an exact fp32 call: the cut, and the split the tail really used = min(plan split, chains of 1024 k)"""
    want = dict(model=EXACT, tiles_m=tiles_m, tiles_n=tiles_n, symm=int(symm), dual=int(dual), n_main=n_main, n_tail=n_tail,
                split=min(split, _chains(L)) if n_tail else 1, nparts=_chains(L) if n_tail else 0, tail_unsplit=0, main_8ph=0,
                accumulate=0)
    return _expect(ctx, what, **want)


@pytest.mark.parametrize("L", EXACT_L)
@pytest.mark.parametrize("case", GENERAL, ids=[c[0] for c in GENERAL])
def test_exact_fp32_general_every_plan_is_the_chain_twin(gpu_ctx, case, L):
    """pvs_cosine_dev, A != B: unsplit, full rounds + split tail, every tile split (a slice of several chains at L = 4096 with two
    slices, one chain per slice with 16, one slice at L <= 1024) -- every element equals the chain twin as bits, with null factors
    and with pvs_row_inv_norms_dev's; ldo = N + 5 keeps the sentinel in the padding."""
    what, M, N, plans = case
    ctx = gpu_ctx
    a, b = _rows(M, L, 11 * M + L), _rows(N, L, 13 * N + L + 1)
    da, db = _up(ctx, a), _up(ctx, b)
    dia, ia = _device_norms(ctx, da, M, L)
    dib, ib = _device_norms(ctx, db, N, L)
    assert ia[2] == 1 and ib[2] == 1                                    # the zero rows
    tm, tn = -(-M // 128), -(-N // 128)
    ldo = N + 5
    for norms in ("null", "device"):
        fa, fb = (None, None) if norms == "null" else (ia, ib)
        twin = _chain_twin(("g", M, N, L, norms), a, b, fa, fb)
        for slots, n_main, n_tail, split in plans:
            out = _padded(ctx, M, ldo)
            with ctx.option(_ffi.OPT_GEMM_SLOTS, slots):
                ctx.cosine_dev(da.ptr, M, db.ptr, N, L, None if fa is None else dia.ptr, None if fb is None else dib.ptr, out.ptr, ldo)
                _exact_plan(ctx, f"{what}, {slots} slots", tm, tn, False, False, n_main, n_tail, split, L)
            ctx.sync()
            got, pad = _take(out, M, N, ldo, np.float32)
            _assert_padding_kept(pad)
            bad = np.argwhere(_bits(got) != _bits(twin))
            assert bad.size == 0, f"{what}, L {L}, {norms} factors, {slots} slots: {len(bad)} elements differ, first at {bad[0]}"
            if norms == "device":
                assert (got[2] == 0).all() and (got[:, 2] == 0).all()
    assert ctx.get_option(_ffi.OPT_GEMM_SLOTS) == 0


@pytest.mark.parametrize("L", EXACT_L)
@pytest.mark.parametrize("case", SYMMETRIC, ids=[c[0] for c in SYMMETRIC])
def test_exact_fp32_symmetric_every_plan_is_the_chain_twin_and_its_own_transpose(gpu_ctx, case, L):
    """pvs_cosine_dev with A == B and one factor array: upper triangle + mirrored store under every plan.  Every element equals the
    chain twin; out == out.T as bits; the same rows at a second address run the general form and give the same bits."""
    what, N, plans = case
    ctx = gpu_ctx
    a = _rows(N, L, 17 * N + L)
    da, da2 = _up(ctx, a), _up(ctx, a)
    assert da.ptr != da2.ptr
    dia, ia = _device_norms(ctx, da, N, L)
    t = -(-N // 128)
    ldo = N + 3
    for norms in ("null", "device"):
        f = None if norms == "null" else ia
        dptr = None if f is None else dia.ptr
        twin = _chain_twin(("s", N, L, norms), a, a, f, f)
        assert np.array_equal(_bits(twin), _bits(twin.T.copy()))
        for slots, n_main, n_tail, split in plans:
            out = _padded(ctx, N, ldo)
            with ctx.option(_ffi.OPT_GEMM_SLOTS, slots):
                ctx.cosine_dev(da.ptr, N, da.ptr, N, L, dptr, dptr, out.ptr, ldo)
                _exact_plan(ctx, f"{what}, {slots} slots", t, t, True, False, n_main, n_tail, split, L)
            ctx.sync()
            got, pad = _take(out, N, N, ldo, np.float32)
            _assert_padding_kept(pad)
            assert np.array_equal(_bits(got), _bits(got.T.copy())), f"{what}, L {L}, {slots} slots: out != out.T"
            bad = np.argwhere(_bits(got) != _bits(twin))
            assert bad.size == 0, f"{what}, L {L}, {norms} factors, {slots} slots: {len(bad)} elements differ, first at {bad[0]}"
        # the second upload: another address -> the general form, all t x t tiles, same bits
        out = _padded(ctx, N, ldo)
        with ctx.option(_ffi.OPT_GEMM_SLOTS, 1):
            ctx.cosine_dev(da.ptr, N, da2.ptr, N, L, dptr, dptr, out.ptr, ldo)
            _exact_plan(ctx, f"{what}, second address", t, t, False, False, t * t, 0, 1, L)
        ctx.sync()
        got2, _ = _take(out, N, N, ldo, np.float32)
        assert np.array_equal(_bits(got2), _bits(twin))


DUAL = [
    ("3x3 tiles", 257, 383, ((1, 9, 0, 1), (4, 8, 1, 4), (64, 0, 9, 16))),
    ("3x3 tiles, M = 0 mod 128", 384, 300, ((2, 8, 1, 2), (64, 0, 9, 16))),
]


@pytest.mark.parametrize("L", EXACT_L)
@pytest.mark.parametrize("case", DUAL, ids=[c[0] for c in DUAL])
def test_exact_fp32_dual_store_is_the_panel_and_its_transpose(gpu_ctx, case, L):
    """pvs_cosine_dual_dev under every plan with ldo > N and ldt > M: out equals the chain twin and the single-store call, out_t ==
    out.T as bits, both paddings keep the sentinel (the transposed store is guarded by rows < N and columns < M, not by ldt)."""
    what, M, N, plans = case
    ctx = gpu_ctx
    a, b = _rows(M, L, 11 * M + L), _rows(N, L, 13 * N + L + 1)
    da, db = _up(ctx, a), _up(ctx, b)
    dia, ia = _device_norms(ctx, da, M, L)
    dib, ib = _device_norms(ctx, db, N, L)
    tm, tn = -(-M // 128), -(-N // 128)
    ldo, ldt = N + 5, M + 7
    twin = _chain_twin(("g", M, N, L, "device"), a, b, ia, ib)
    single = _padded(ctx, M, N)
    with ctx.option(_ffi.OPT_GEMM_SLOTS, 1):
        ctx.cosine_dev(da.ptr, M, db.ptr, N, L, dia.ptr, dib.ptr, single.ptr, N)
        _exact_plan(ctx, f"{what}, single store", tm, tn, False, False, tm * tn, 0, 1, L)
    ctx.sync()
    single = single.download((M, N), np.float32)
    for slots, n_main, n_tail, split in plans:
        out, out_t = _padded(ctx, M, ldo), _padded(ctx, N, ldt)
        with ctx.option(_ffi.OPT_GEMM_SLOTS, slots):
            ctx.cosine_dual_dev(da.ptr, M, db.ptr, N, L, dia.ptr, dib.ptr, out.ptr, ldo, out_t.ptr, ldt)
            _exact_plan(ctx, f"{what}, dual, {slots} slots", tm, tn, False, True, n_main, n_tail, split, L)
        ctx.sync()
        got, pad = _take(out, M, N, ldo, np.float32)
        got_t, pad_t = _take(out_t, N, M, ldt, np.float32)
        _assert_padding_kept(pad)
        _assert_padding_kept(pad_t)
        assert np.array_equal(_bits(got), _bits(twin)) and np.array_equal(_bits(got), _bits(single))
        assert np.array_equal(_bits(got_t), _bits(got.T.copy())), f"{what}, L {L}, {slots} slots: out_t != out.T"


def test_exact_fp32_k_tile_seam_every_k_tile_is_told_apart(gpu_ctx):
    """L = 16 x 32: row m of A is non-zero in k-tile m % 16 only, row n of B in k-tile (n // 3) % 16 only, each k-tile with its own
    magnitude (2^t), so a k-tile that is skipped, read twice or read from the wrong stage shows as a wrong or a non-zero element.
    Whole tiles and split tiles (one chain: the split collapses to one slice), against the chain twin, and by the pattern itself."""
    ctx = gpu_ctx
    M, N, L = 130, 150, 512
    rng = np.random.default_rng(5)
    a, b = np.zeros((M, L), np.float32), np.zeros((N, L), np.float32)
    ta, tb = np.arange(M) % 16, (np.arange(N) // 3) % 16
    for m in range(M):
        a[m, 32 * ta[m]:32 * ta[m] + 32] = rng.standard_normal(32).astype(np.float32) * np.float32(2.0 ** ta[m])
    for n in range(N):
        b[n, 32 * tb[n]:32 * tb[n] + 32] = rng.standard_normal(32).astype(np.float32) * np.float32(2.0 ** tb[n])
    twin = orc_c.cosine_chain_full(a, b, None, None)
    meet = ta[:, None] == tb[None, :]
    assert (twin[~meet] == 0).all() and (twin[meet] != 0).all()
    da, db = _up(ctx, a), _up(ctx, b)
    for slots, n_main, n_tail, split in ((1, 4, 0, 1), (64, 0, 4, 16)):
        out = _padded(ctx, M, N)
        with ctx.option(_ffi.OPT_GEMM_SLOTS, slots):
            ctx.cosine_dev(da.ptr, M, db.ptr, N, L, None, None, out.ptr, N)
            _exact_plan(ctx, f"seam, {slots} slots", 2, 2, False, False, n_main, n_tail, split, L)
        ctx.sync()
        got = out.download((M, N), np.float32)
        assert (got[~meet] == 0).all()
        assert np.array_equal(_bits(got), _bits(twin))


# ====================================================================================================== the plan's cache
def test_plan_cache_key_regrowth_and_slot_change():
    """One fresh context (its read-back is all -1 and its tile list unallocated, so the regrowth below is certain): shape P, a shape
    of more tiles than the first allocation holds (9 + 9/4 + 64 = 75 < 81), the symmetric form of P's tile counts, another slot
    count, P again.  Each call's read-back is its own plan, each output its twin, first and last equal as bits."""
    import pvsim
    with pvsim.Context(0) as ctx:
        assert set(ctx.gemm_last_plan().values()) == {-1}
        L = 1040                                                        # two chains: a split is real
        a, b = _rows(257, L, 1), _rows(383, L, 2)
        big_a, big_b = _rows(1100, 40, 3), _rows(1150, 40, 4)
        da, db, dba, dbb = _up(ctx, a), _up(ctx, b), _up(ctx, big_a), _up(ctx, big_b)
        twin = orc_c.cosine_chain_full(a, b, None, None)

        def run(d_x, M, d_y, N, Lx):
            out = _padded(ctx, M, N)
            ctx.cosine_dev(d_x.ptr, M, d_y.ptr, N, Lx, None, None, out.ptr, N)
            plan = ctx.gemm_last_plan()
            ctx.sync()
            return out.download((M, N), np.float32), plan

        with ctx.option(_ffi.OPT_GEMM_SLOTS, 4):
            first, p1 = run(da, 257, db, 383, L)                        # 1. P
            assert (p1["tiles_m"], p1["tiles_n"], p1["symm"], p1["n_main"], p1["n_tail"], p1["split"]) == (3, 3, 0, 8, 1, 2), p1
            big, p2 = run(dba, 1100, dbb, 1150, 40)                     # 2. 9 x 9 = 81 tiles: the device list regrows
            assert (p2["tiles_m"], p2["tiles_n"], p2["symm"], p2["n_main"], p2["n_tail"], p2["split"]) == (9, 9, 0, 80, 1, 1), p2
            assert np.array_equal(_bits(big), _bits(orc_c.cosine_chain_full(big_a, big_b, None, None)))
            sym, p3 = run(da, 257, da, 257, L)                          # 3. the same tile counts, symmetric: another key
            assert (p3["tiles_m"], p3["tiles_n"], p3["symm"], p3["n_main"], p3["n_tail"], p3["split"]) == (3, 3, 1, 4, 2, 2), p3
            assert np.array_equal(_bits(sym), _bits(orc_c.cosine_chain_full(a, a, None, None)))
            again, p4 = run(da, 257, db, 383, L)                        # and back: the general list is rebuilt, not the symmetric one reused
            assert p4 == p1 and np.array_equal(_bits(again), _bits(first))
        with ctx.option(_ffi.OPT_GEMM_SLOTS, 64):                       # 4. another slot count
            last, p5 = run(da, 257, db, 383, L)                         # 5. P again
            assert (p5["tiles_m"], p5["tiles_n"], p5["symm"], p5["n_main"], p5["n_tail"], p5["split"]) == (3, 3, 0, 0, 9, 2), p5
        assert np.array_equal(_bits(first), _bits(twin)) and np.array_equal(_bits(last), _bits(first))   # 6.
        default, p6 = run(da, 257, db, 383, L)                          # the option is back at 0: the chip's own slots
        assert p6["n_main"] + p6["n_tail"] == 9 and np.array_equal(_bits(default), _bits(first))


def test_slot_option_limits(gpu_ctx):
    assert gpu_ctx.get_option(_ffi.OPT_GEMM_SLOTS) == 0
    with gpu_ctx.option(_ffi.OPT_GEMM_SLOTS, 4096):
        assert gpu_ctx.get_option(_ffi.OPT_GEMM_SLOTS) == 4096
    for bad in (-1, 4097):
        with pytest.raises(ValueError):
            gpu_ctx.set_option(_ffi.OPT_GEMM_SLOTS, bad)
    assert gpu_ctx.get_option(_ffi.OPT_GEMM_SLOTS) == 0


# ====================================================================================================== generic tile kernel
GENERIC_SHAPES = [(1, 1, 1), (65, 64, 15), (64, 130, 37), (3, 200, 1001)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("M,N,L", GENERIC_SHAPES + [(70, 70, 40)])
def test_generic_kernel_is_the_sequential_twin(gpu_ctx, dtype, M, N, L):
    """L % 4 != 0 (f32) / odd L (f64) take the 64 x 64 tile kernel; so does (70, 70, 40) when the rows start 4 bytes (f32) or 8 bytes
    (f64: the nearest aligned double) past a 16-byte boundary.  Every element equals acc = fma(a_k, b_k, acc) in ascending k times
    (ia ib), with factors and without; ldo = N + 3; the read-back says generic."""
    ctx = gpu_ctx
    rng = np.random.default_rng(M + 3 * N + 7 * L)
    a = rng.standard_normal((M, L)).astype(dtype)
    b = rng.standard_normal((N, L)).astype(dtype)
    if N > 2:
        b[1] = 0
    ia = rng.uniform(0.5, 2, M).astype(dtype)
    ib = rng.uniform(0.5, 2, N).astype(dtype)
    size = np.dtype(dtype).itemsize
    shift = (4 if dtype == np.float32 else 8) if (M, N, L) == (70, 70, 40) else 0
    da, db = ctx.buffer(a.nbytes + 16), ctx.buffer(b.nbytes + 16)
    da.upload(a, offset=shift)
    db.upload(b, offset=shift)
    assert da.ptr % 16 == 0 and db.ptr % 16 == 0
    dia, dib = _up(ctx, ia), _up(ctx, ib)
    call = ctx.cosine_dev if dtype == np.float32 else ctx.cosine_f64_dev
    ldo = N + 3
    for fa, fb, pa, pb in ((None, None, None, None), (ia, ib, dia.ptr, dib.ptr)):
        out = _padded(ctx, M, ldo, size)
        call(da.ptr + shift, M, db.ptr + shift, N, L, pa, pb, out.ptr, ldo)
        _expect(ctx, "generic", model=GENERIC, tiles_m=-(-M // 64), tiles_n=-(-N // 64), symm=0, dual=0, n_tail=0, split=1)
        ctx.sync()
        got, pad = _take(out, M, N, ldo, dtype)
        _assert_padding_kept(pad)
        twin = orc_c.cosine_seq(a, b, fa, fb)
        bad = np.argwhere(_bits(got) != _bits(twin))
        assert bad.size == 0, f"{len(bad)} elements differ, first at {bad[0]}"
        if N > 2:
            assert (got[:, 1] == 0).all()


# ====================================================================================================== f64 on the matrix pipe
F64_L = [2, 18, 258, 4100]              # one k-tile of 16 (nothing to split) / two / 17 with a partial one / 257
_F64 = {}
RATIOS = {}                              # family -> largest error / bound seen in this session (printed per case)


def _f64_inputs(M, N, L, symm):
    key = (M, N, L, symm)
    if key not in _F64:
        rng = np.random.default_rng(1000 * M + N + L)
        a = rng.standard_normal((M, L)) * np.exp(rng.uniform(-3, 3, (M, 1)))
        a[2] = 0
        b = a if symm else rng.standard_normal((N, L))
        if not symm:
            b[3] = 0
        dot, mag = orc_c.dot_abs_ld(a, b)
        _F64[key] = (a, b, dot, mag)
    return _F64[key]


def _f64_bound_check(what, got, dot, mag, ia, ib, L):
    scale = ia.astype(LD)[:, None] * ib.astype(LD)[None, :]
    err = np.abs(got.astype(LD) - dot * scale)
    bound = (L + 3) * LD(2.0) ** -52 * mag * scale
    ratio = float((err / np.maximum(bound, np.finfo(LD).tiny)).max())
    RATIOS["f64"] = max(RATIOS.get("f64", 0.0), ratio)
    print(f"f64 {what}: largest error / bound = {ratio:.4f}")
    assert (err <= bound).all(), f"{what}: error / bound = {ratio}"


@pytest.mark.parametrize("L", F64_L)
@pytest.mark.parametrize("symm", [False, True], ids=["general", "symmetric"])
def test_f64_matrix_pipe_every_plan_within_the_summation_bound(gpu_ctx, symm, L):
    """pvs_cosine_f64_dev, 3 x 3 tiles (257 x 383 general, 384 symmetric), unsplit / full rounds + split tail / every tile split:
    |got - dot ia ib| <= (L + 3) 2^-52 sum|a_k b_k| ia ib against the long double dot under EACH plan (the split changes an f64
    score, so plans are not compared with each other).  L = 2 is a single k-tile: the tail runs unsplit and the read-back says
    why.  Zero rows score exactly 0; the symmetric form is its own transpose as bits; ldo = N + 1."""
    ctx = gpu_ctx
    M, N = (384, 384) if symm else (257, 383)
    a, b, dot, mag = _f64_inputs(M, N, L, symm)
    da = _up(ctx, a)
    db = da if symm else _up(ctx, b)
    dia = ctx.buffer(M * 8)
    ctx.row_inv_norms_f64_dev(da.ptr, M, L, dia.ptr)
    dib = dia if symm else ctx.buffer(N * 8)
    if not symm:
        ctx.row_inv_norms_f64_dev(db.ptr, N, L, dib.ptr)
    ctx.sync()
    ia, ib = dia.download((M,), np.float64), dib.download((N,), np.float64)
    assert ia[2] == 1.0
    nk = -(-L // 16)
    plans = ((1, 6, 0, 1), (4, 4, 2, 2), (64, 0, 6, 8)) if symm else ((1, 9, 0, 1), (4, 8, 1, 4), (64, 0, 9, 16))
    ldo = N + 1
    for slots, n_main, n_tail, split in plans:
        out = _padded(ctx, M, ldo, 8)
        with ctx.option(_ffi.OPT_GEMM_SLOTS, slots):
            ctx.cosine_f64_dev(da.ptr, M, db.ptr, N, L, dia.ptr, dib.ptr, out.ptr, ldo)
            sk = min(split, nk)
            _expect(ctx, f"f64, {slots} slots", model=F64, tiles_m=3, tiles_n=3, symm=int(symm), dual=0, n_main=n_main, n_tail=n_tail,
                    split=sk if n_tail else 1, nparts=sk if n_tail else 0,
                    tail_unsplit=_ffi.GEMM_TAIL_UNSPLIT_ONE_SLICE if (n_tail and sk == 1) else 0, main_8ph=0, accumulate=0)
        ctx.sync()
        got, pad = _take(out, M, N, ldo, np.float64)
        _assert_padding_kept(pad)
        _f64_bound_check(f"{'symmetric' if symm else 'general'} L {L} slots {slots}", got, dot, mag, ia, ib, L)
        assert (got[2] == 0).all()
        if symm:
            assert (got[:, 2] == 0).all() and np.array_equal(_bits(got), _bits(got.T.copy()))
        else:
            assert (got[:, 3] == 0).all()


# ====================================================================================================== fp16 256 x 256
F16_L = [8, 72, 136, 200, 1032]         # k-tiles of 64: 1 / 2 / 3 / 4 with a partial one / 17
_F16 = {}


def _f16_case(ctx, M, N, L, symm):
    """operands rounded on the device by pvs_f32_to_f16_dev, read back; float32 factors of the rounded rows; long double reference"""
    rng = np.random.default_rng(7 * M + N + L)
    a = (rng.standard_normal((M, L)) * 0.3).astype(np.float32)
    a[2] = 0
    b = a if symm else (rng.standard_normal((N, L)) * 0.3).astype(np.float32)
    if not symm:
        b[3] = 0

    def to16(x):
        src, dst = _up(ctx, x), ctx.buffer(x.size * 2)
        ctx.f32_to_f16_dev(src.ptr, x.size, dst.ptr)
        ctx.sync()
        h = dst.download(x.shape, np.float16)
        assert np.array_equal(h.view(np.uint16), x.astype(np.float16).view(np.uint16))     # round to nearest even
        return dst, h.astype(np.float32)

    da, a16 = to16(a)
    db, b16 = (da, a16) if symm else to16(b)
    key = (M, N, L, symm)
    if key not in _F16:
        def inv(x):
            s = (x.astype(np.float64) ** 2).sum(1)
            return np.where(s > 0, 1 / np.sqrt(np.maximum(s, 1e-300)), 1).astype(np.float32)
        _F16[key] = (inv(a16), inv(b16)) + orc_c.dot_abs_ld(a16, b16)
    ia, ib, dot, mag = _F16[key]
    return da, db, ia, ib, dot, mag


@pytest.mark.parametrize("L", F16_L)
@pytest.mark.parametrize("symm", [False, True], ids=["general 520x700", "symmetric 600"])
def test_fp16_256_every_plan_within_the_summation_bound(gpu_ctx, symm, L):
    """pvs_cosine_f16_dev, 3 x 3 tiles of 256: all tiles on the 8-phase kernel (1 slot), 8-phase main + two-stage split tail in one
    call (4 slots), every tile split (64 slots) -- at L = 8 and 72 the split (4, 8 or 16) exceeds the k-tiles (1, 2), so most
    slices are empty and must add exact zeros.  |got - dot ia ib| <= (L + 2) 2^-23 sum|a_k b_k| ia ib against the long double dot of
    the fp16-rounded operands; zero rows score exactly 0; symmetric out == out.T as bits under each plan; ldo = N + 4."""
    ctx = gpu_ctx
    M, N = (600, 600) if symm else (520, 700)
    da, db, ia, ib, dot, mag = _f16_case(ctx, M, N, L, symm)
    dia = _up(ctx, ia)
    dib = dia if symm else _up(ctx, ib)
    plans = ((1, 6, 0, 1), (4, 4, 2, 2), (64, 0, 6, 8)) if symm else ((1, 9, 0, 1), (4, 8, 1, 4), (64, 0, 9, 16))
    scale = ia.astype(LD)[:, None] * ib.astype(LD)[None, :]
    bound = (L + 2) * LD(2.0) ** -23 * mag * scale
    ldo = N + 4
    for slots, n_main, n_tail, split in plans:
        out = _padded(ctx, M, ldo)
        with ctx.option(_ffi.OPT_GEMM_SLOTS, slots):
            ctx.cosine_f16_dev(da.ptr, M, db.ptr, N, L, dia.ptr, dib.ptr, out.ptr, ldo)
            _expect(ctx, f"fp16 256, {slots} slots", model=F16_256, tiles_m=3, tiles_n=3, symm=int(symm), dual=0, n_main=n_main,
                    n_tail=n_tail, split=split if n_tail else 1, nparts=split if n_tail else 0, tail_unsplit=0,
                    main_8ph=int(n_main > 0), accumulate=0)
        ctx.sync()
        got, pad = _take(out, M, N, ldo, np.float32)
        _assert_padding_kept(pad)
        err = np.abs(got.astype(LD) - dot * scale)
        ratio = float((err / np.maximum(bound, np.finfo(LD).tiny)).max())
        RATIOS["f16"] = max(RATIOS.get("f16", 0.0), ratio)
        print(f"fp16 256 {'symmetric' if symm else 'general'} L {L} slots {slots}: largest error / bound = {ratio:.4f}")
        assert (err <= bound).all(), f"L {L}, {slots} slots: error / bound = {ratio}"
        assert (got[2] == 0).all()
        if symm:
            assert (got[:, 2] == 0).all() and np.array_equal(_bits(got), _bits(got.T.copy()))
        else:
            assert (got[:, 3] == 0).all()


def test_fp16_256_refuses_rows_that_are_not_16_byte_aligned(gpu_ctx):
    ctx = gpu_ctx
    buf, out = ctx.buffer(64 * 80 * 2 + 16).fill_bytes(0), ctx.buffer(64 * 64 * 4)
    before = ctx.gemm_last_plan()
    with pytest.raises(NotImplementedError):
        ctx.cosine_f16_dev(buf.ptr, 64, buf.ptr, 64, 12, None, None, out.ptr, 64)              # L % 8 != 0
    for shift_a, shift_b in ((2, 0), (0, 8)):
        with pytest.raises(NotImplementedError):
            ctx.cosine_f16_dev(buf.ptr + shift_a, 64, buf.ptr + shift_b, 64, 72, None, None, out.ptr, 64)
    assert ctx.gemm_last_plan() == before                                                       # nothing was launched


# ====================================================================================================== bounded fp16 prefilter
def _clustered(rng, nq, N, L, same):
    """rows around 40 prototypes (the filter's margin separates the best scores from the bulk); a zero row and an exact duplicate in
    the database, one query that IS a database row"""
    proto = rng.standard_normal((40, L)).astype(np.float32)
    db = proto[rng.integers(0, 40, N)] + np.float32(0.6) * rng.standard_normal((N, L)).astype(np.float32)
    db[7] = 0
    db[11] = db[5]
    if same:
        return db, db
    q = db[rng.integers(0, N, nq)] + np.float32(0.3) * rng.standard_normal((nq, L)).astype(np.float32)
    q[1] = db[5]
    return q, db


def _filtered_equals_exact(ctx, what, q, db, same, k, slots, **want):
    nq, L = q.shape
    N = db.shape[0]
    ddb = _up(ctx, db)
    dq = ddb if same else _up(ctx, q)
    didb = ctx.buffer(N * 4)
    ctx.row_inv_norms_dev(ddb.ptr, N, L, didb.ptr)
    diq = didb if same else ctx.buffer(nq * 4)
    if not same:
        ctx.row_inv_norms_dev(dq.ptr, nq, L, diq.ptr)
    f_idx, f_val = ctx.buffer(nq * k * 8).fill_bytes(0xff), ctx.buffer(nq * k * 4).fill_bytes(0xff)
    with ctx.option(_ffi.OPT_GEMM_SLOTS, slots):
        st = ctx.cosine_topk_filtered_dev(dq.ptr, nq, ddb.ptr, N, L, diq.ptr, didb.ptr, k, f_idx.ptr, f_val.ptr)
        assert st["filtered"], f"{what}: the prefilter declined, the test would compare the exact path with itself"
        assert st["redone_exact"] == 0, f"{what}: {st['redone_exact']} queries went to the exact path, whose GEMM hides the prefilter's read-back"
        _expect(ctx, what, **want)
    ctx.sync()
    e_idx, e_val = ctx.buffer(nq * k * 8).fill_bytes(0xff), ctx.buffer(nq * k * 4).fill_bytes(0xff)
    ctx.cosine_topk_dev(dq.ptr, nq, ddb.ptr, N, L, diq.ptr, didb.ptr, k, 0, False, e_idx.ptr, e_val.ptr)
    ctx.sync()
    fi, fv = f_idx.download((nq, k), np.int64), f_val.download((nq, k), np.float32)
    ei, ev = e_idx.download((nq, k), np.int64), e_val.download((nq, k), np.float32)
    assert np.array_equal(fi, ei), f"{what}: {int((fi != ei).any(1).sum())} lists differ"
    assert np.array_equal(_bits(fv), _bits(ev))
    return fi


@pytest.mark.parametrize("L", [200, 264])
def test_prefilter_two_level_256x128_kernel_at_600_by_700(gpu_ctx, L):
    """1 slot: 3 x 6 tiles of 256 x 128 >= 4 slots -> gemm_f16_2lvl.hpp, whole tiles only.  L = 200: partial last k-tile; L = 264: five
    k-tiles, not a multiple of the three LDS buffers."""
    q, db = _clustered(np.random.default_rng(L), 600, 700, L, False)
    idx = _filtered_equals_exact(gpu_ctx, "two-level", q, db, False, 5, 1, model=F16_2LVL, tiles_m=3, tiles_n=6, symm=0, n_main=18,
                                 n_tail=0, accumulate=0)
    assert idx[1, 0] == 5 and idx[1, 1] == 11                           # the duplicated row: equal scores in index order


# 600 x 700 = 5 x 6 tiles of 128 (from 5 slots on the two-level kernel no longer qualifies: 18 < 4 x 5); L = 2568 = three chains
BOUNDED_GENERAL = [(5, 30, 0, 1), (7, 28, 2, 16), (64, 0, 30, 2)]    # the last: two slices, one of two chains
BOUNDED_SELF = [(1, 6, 0, 1), (4, 4, 2, 2), (64, 0, 6, 8)]               # 300 x 300 self: 3 x 3 symmetric


@pytest.mark.parametrize("slots,n_main,n_tail,split", BOUNDED_GENERAL)
def test_prefilter_128_kernel_general_every_plan(gpu_ctx, slots, n_main, n_tail, split):
    L = 2568
    q, db = _clustered(np.random.default_rng(3), 600, 700, L, False)
    _filtered_equals_exact(gpu_ctx, f"bounded 128 general, {slots} slots", q, db, False, 5, slots, model=F16_BOUNDED, tiles_m=5, tiles_n=6,
                           symm=0, n_main=n_main, n_tail=n_tail, split=min(split, 3) if n_tail else 1, nparts=3 if n_tail else 0,
                           accumulate=0)


@pytest.mark.parametrize("slots,n_main,n_tail,split", BOUNDED_SELF)
def test_prefilter_128_kernel_self_every_plan(gpu_ctx, slots, n_main, n_tail, split):
    """Q == DB with one factor array: one symmetric launch.  k = 64 keeps the candidate slots (4 k + 64) above the 300 tied scores of
    the zero row, so no query leaves for the exact path and the read-back stays the prefilter's."""
    L = 2568
    db, _ = _clustered(np.random.default_rng(4), 300, 300, L, True)
    _filtered_equals_exact(gpu_ctx, f"bounded 128 self, {slots} slots", db, db, True, 64, slots, model=F16_BOUNDED, tiles_m=3, tiles_n=3,
                           symm=1, n_main=n_main, n_tail=n_tail, split=min(split, 3) if n_tail else 1, nparts=3 if n_tail else 0,
                           accumulate=0)


@functools.lru_cache(maxsize=None)
def _long_rows():
    db, _ = _clustered(np.random.default_rng(9), 300, 300, 32776, True)
    db.setflags(write=False)
    return db


SEGMENTS = [
    # what, queries, self, k, slots, read-back of the LAST segment (8 k-values, added into the output)
    ("128 kernel, split tail: the reduce adds into the output", 130, False, 5, 4,
     dict(model=F16_BOUNDED, tiles_m=2, tiles_n=3, symm=0, n_main=4, n_tail=2, split=1, nparts=1, accumulate=1)),
    ("128 kernel, self, split tail: the mirrored store carries the sum", 300, True, 64, 4,
     dict(model=F16_BOUNDED, tiles_m=3, tiles_n=3, symm=1, n_main=4, n_tail=2, split=1, nparts=1, accumulate=1)),
    ("two-level kernel adds into the output", 260, False, 5, 1,
     dict(model=F16_2LVL, tiles_m=2, tiles_n=3, symm=0, n_main=6, n_tail=0, accumulate=1)),
]


@pytest.mark.parametrize("case", SEGMENTS, ids=[c[0] for c in SEGMENTS])
def test_prefilter_two_accumulated_segments_at_L_32776(gpu_ctx, case):
    """Rows longer than 32768 go through in segments of 32768 k-values accumulated in the output; L = 32776 is one full segment and
    one of a single 16-byte chunk.  The read-back shows the last launch: the second segment, adding."""
    what, nq, same, k, slots, want = case
    db = _long_rows()
    rng = np.random.default_rng(nq)
    if same:
        q = db
    else:
        q = db[rng.integers(0, 300, nq)] + np.float32(0.3) * rng.standard_normal((nq, db.shape[1])).astype(np.float32)
        q[1] = db[5]
    _filtered_equals_exact(gpu_ctx, what, q, db, same, k, slots, **want)


# ====================================================================================================== row norms
NORM_ROWS = [1, 3, 4, 5, 9]             # four rows per workgroup
NORM_L = [1, 3, 4, 252, 256, 260, 1001]  # 64 lanes x float4 = 256: below, at and above one pass; scalar lengths


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("L", NORM_L)
def test_row_inv_norms_within_L_plus_8_u(gpu_ctx, dtype, L):
    """pvs_row_inv_norms_dev (float4 form when L % 4 == 0 and the rows are 16-byte aligned, scalar form otherwise -- reached by the
    length and by a pointer 4 bytes past a boundary) and pvs_row_inv_norms_f64_dev: |got - 1/sqrt(sum x^2)| <= (L + 8) u |.| against
    long double, u = 2^-24 / 2^-53.  A zero row gives exactly 1; a row whose sum of squares is denormal gives a finite value."""
    ctx = gpu_ctx
    f32 = dtype == np.float32
    u = LD(2.0) ** (-24 if f32 else -53)
    call = ctx.row_inv_norms_dev if f32 else ctx.row_inv_norms_f64_dev
    size = np.dtype(dtype).itemsize
    for rows in NORM_ROWS:
        rng = np.random.default_rng(100 * rows + L)
        x = (rng.standard_normal((rows, L)) * np.exp(rng.uniform(-3, 3, (rows, 1)))).astype(dtype)
        zero, tiny = (1, 2) if rows >= 3 else (None, None)
        if zero is not None:
            x[zero] = 0
            x[tiny] = 0
            x[tiny, 0] = dtype(1e-21 if f32 else 1e-158)               # its square is a denormal
        with np.errstate(divide="ignore"):
            ref = 1 / np.sqrt((x.astype(LD) ** 2).sum(1))
        for shift in (0, size):                                         # size: 4 / 8 bytes past a 16-byte boundary
            buf = ctx.buffer(x.nbytes + 16)
            buf.upload(x, offset=shift)
            assert buf.ptr % 16 == 0
            out = ctx.buffer((rows + 2) * size).fill_bytes(0xff)
            call(buf.ptr + shift, rows, L, out.ptr)
            ctx.sync()
            got = out.download((rows + 2,), dtype)
            _assert_padding_kept(got[rows:])
            got = got[:rows]
            assert np.isfinite(got).all()
            live = np.ones(rows, bool)
            if zero is not None:
                assert got[zero] == 1
                live[[zero, tiny]] = False
            err = np.abs(got[live].astype(LD) - ref[live]) / ref[live]
            print(f"row norms {np.dtype(dtype).name} rows {rows} L {L} shift {shift}: largest error / bound = {float((err / ((L + 8) * u)).max()):.3f}")
            assert (err <= (L + 8) * u).all(), (rows, L, shift, float((err / ((L + 8) * u)).max()))
