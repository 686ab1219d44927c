"""Planted score panels for the ranking kernels of csrc/topk.hip, shared by tests/test_topk_host.py (which asserts, from the twin
alone, that every adversarial panel meets the condition that sends the kernels down the branch it is meant for) and by the GPU
tests that rank them on the device.  Everything is a pure function of its arguments and a seed.

Kernel geometry the panels are built around (csrc/topk.hip): the one-wave threshold filter reads chunks of 2048 columns, keeps
at most 256 survivors and serves k <= 16; the launcher moves from the k-rounds kernel to it at 4096 columns; the radix select and
the rounds read chunks of 8192 columns; one launch ranks at most 1024 deep, deeper lists are paged."""
import numpy as np

import topk_numpy as tk

WAVE_CHUNK, WAVE_LIST, WAVE_KMAX, SWITCH, RADIX_CHUNK, KMAX = 2048, 256, 16, 4096, 8192, 1024
NCOLS = ("k-1", "k", 0, 1, 63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4099, 6151, 8191, 8192, 8197, 16389)
KS = (1, 2, 15, 16, 17, 255, 256, 257, 1023, 1024)
KS_PAGED = (1025, 2048, 2049)
INDEX_LIMIT = 0xfffffffe           # col_offset + ncols may reach this, not exceed it
PLATEAU = 300                      # equal scores of a plateau row, at least
RADIX_HOLES = 7                    # columns 3 .. 9 of the radix-depth row score low, so the cut never sits at a multiple of 256

_NAN_BITS = {np.dtype(np.float32): (0xffc00001, 0x7f800001, 0xffffffff, 0x7fc00000, 0xff800123),
             np.dtype(np.float64): (0xfff8000000000001, 0x7ff0000000000001, 0xffffffffffffffff, 0x7ff8000000000000,
                                    0xfff0000000000123)}


def resolve_ncols(ncols, k):
    return {"k-1": k - 1, "k": k}.get(ncols, ncols)


def _gauss(rng, n, dt):
    return rng.standard_normal(n).astype(dt)


def _put(row, cols, value):
    cols = np.asarray(cols, np.int64)
    row[cols[cols < len(row)]] = value


# ------------------------------------------------------------------------------------------------ rows
def row_ties_across_chunks(rng, n, k, dt):
    """Gaussian; columns 5, 5 + 2048 and 5 + 8192 share the best value, columns 2047, 2048, 8191, 8192 the second best"""
    row = _gauss(rng, n, dt)
    top = dt(np.ceil(np.abs(row).max()) if n else 1.0)
    _put(row, [2047, 2048, RADIX_CHUNK - 1, RADIX_CHUNK], top + dt(0.5))
    _put(row, [5, 5 + WAVE_CHUNK, 5 + RADIX_CHUNK], top + dt(1))
    return row


def row_increasing(rng, n, k, dt):
    return (np.arange(n) - n // 2).astype(dt)


def row_decreasing(rng, n, k, dt):
    return row_increasing(rng, n, k, dt)[::-1].copy()


def row_all_equal(rng, n, k, dt):
    return np.full(n, 0.25, dt)


def row_all_nan(rng, n, k, dt):
    return np.full(n, np.nan, dt)


def row_fewer_numbers_than_k(rng, n, k, dt):
    """k // 2 numbers (none at k = 1), NaN everywhere else"""
    row = np.full(n, np.nan, dt)
    cnt = min(n, k // 2)
    row[rng.choice(n, cnt, replace=False) if cnt else []] = np.round(_gauss(rng, cnt, dt) * 4) / 4
    return row


def row_nan_lanes(rng, n, k, dt):
    """first chunk: every column that lane 0 .. 55 of the wave kernel reads, in its 16-byte layout (lane = (c / 4) % 64) and in its
    4-byte layout (lane = c % 64), is NaN, so those lanes' maxima are NaN; 8 (or 2) lanes keep numbers"""
    row = _gauss(rng, n, dt)
    c = np.arange(min(n, WAVE_CHUNK))
    row[c[(c % 64 < 56) | ((c // 4) % 64 < 56)]] = np.nan
    return row


def row_infinities(rng, n, k, dt):
    row = _gauss(rng, n, dt)
    row[rng.random(n) < 0.2] = -np.inf
    row[rng.random(n) < 0.1] = np.inf
    return row


def row_all_minus_inf(rng, n, k, dt):
    return np.full(n, -np.inf, dt)


def row_signed_zeros(rng, n, k, dt):
    """k + 5 zeros of either sign over strictly negative scores: the cut at k falls among the zeros"""
    row = (-1 - np.abs(_gauss(rng, n, dt))).astype(dt)
    cnt = min(n, k + 5)
    at = rng.choice(n, cnt, replace=False) if cnt else np.zeros(0, np.int64)
    row[at] = np.where(rng.random(cnt) < 0.5, dt(-0.0), dt(0.0))
    return row


def row_denormals(rng, n, k, dt):
    """small integer multiples of the smallest denormal, either sign, many ties"""
    return (rng.integers(-50, 51, n).astype(dt) * np.finfo(dt).smallest_subnormal).astype(dt)


def row_nan_payloads(rng, n, k, dt):
    """a third of the columns are NaN with sign bits and payloads (quiet and signalling)"""
    row = np.round(_gauss(rng, n, dt) * 8) / 8
    at = np.flatnonzero(rng.random(n) < 0.33)
    pat = np.array(_NAN_BITS[np.dtype(dt)], tk.bits(row).dtype)
    tk.bits(row)[at] = pat[np.arange(len(at)) % len(pat)] if len(at) else pat[:0]
    return row


def _plateau(rng, n, k, dt, where):
    """k // 2 distinct better scores, then max(PLATEAU, k) columns at 0.5, everything else distinct-ish and lower.
    where = "first": all of them inside the first chunk (when they fit); "late": the plateau is the row's tail and the better
    scores come before it, in earlier chunks"""
    row = (-1 - np.abs(_gauss(rng, n, dt))).astype(dt)
    b, ln = k // 2, max(PLATEAU, k)
    better = (1 + np.arange(b) / 1024).astype(dt)
    if where == "first":
        span = min(n, max(WAVE_CHUNK, b + ln))
        at = rng.permutation(span)[:min(n, b + ln)]
        row[at[b:]] = 0.5
        row[at[:b]] = better[:len(at[:b])]
    else:
        start = max(0, n - ln)
        row[start:] = 0.5
        nb = min(b, start)
        row[rng.choice(min(start, WAVE_CHUNK), nb, replace=False) if nb else []] = better[:nb]
    return row


def row_plateau_first_chunk(rng, n, k, dt):
    return _plateau(rng, n, k, dt, "first")


def row_plateau_late_chunk(rng, n, k, dt):
    return _plateau(rng, n, k, dt, "late")


def row_radix_depth(rng, n, k, dt):
    """three better columns, RADIX_HOLES low ones, then one value to the end: for k > 3 the k-th and (k+1)-th keys have the same
    score and neighbouring indices k + 6 and k + 7, which differ in the lowest index byte alone"""
    row = np.full(n, 0.25, dt)
    row[:3] = 1.0
    row[3:3 + RADIX_HOLES] = -2.0
    return row


def row_exactly_k_numbers(rng, n, k, dt):
    row = np.full(n, np.nan, dt)
    cnt = min(n, k)
    row[rng.choice(n, cnt, replace=False) if cnt else []] = np.round(_gauss(rng, cnt, dt) * 4) / 4
    return row


GROUPS = {
    "A": (row_ties_across_chunks, row_increasing, row_decreasing, row_all_equal, row_all_nan, row_fewer_numbers_than_k, row_nan_lanes,
          row_infinities, row_all_minus_inf),
    "B": (row_signed_zeros, row_denormals, row_nan_payloads, row_plateau_first_chunk, row_plateau_late_chunk, row_radix_depth,
          row_exactly_k_numbers),
}
ALL_ROWS = GROUPS["A"] + GROUPS["B"]


def panel(group, n, k, dt=np.float32, seed=0):
    """(rows of the group, n): 9 or 7 query rows, neither a multiple of the four rows a workgroup of the wave kernel serves"""
    dt = np.dtype(dt).type
    fns = GROUPS[group]
    out = np.empty((len(fns), n), dt)
    for r, fn in enumerate(fns):
        out[r] = fn(np.random.default_rng([seed, r, n, k]), n, k, dt)
    return out


# ------------------------------------------------------------------------------------------------ branch conditions (twin side)
def mono_key(val, idx):
    """the 64-bit key of csrc/topk.hip for a float32 score and its index, as a Python int: order-preserving image of the score
    (NaN lowest, -0 = +0) in the high half, the complemented index in the low half"""
    v = np.float32(val)
    if np.isnan(v):
        m = 1
    else:
        u = int(tk.bits(np.array([v + np.float32(0)], np.float32))[0])
        m = (~u & 0xffffffff) if u & 0x80000000 else (u | 0x80000000)
    return (m << 32) | (~int(idx) & 0xffffffff)


def cut_keys(row, k):
    """keys of the k-th and (k+1)-th entries of the row's ranking (needs more than k columns)"""
    idx, val = tk.topk(row[None, :], k + 1)
    return mono_key(val[0, k - 1], idx[0, k - 1]), mono_key(val[0, k], idx[0, k])


def wave_overflow_chunks(row, k):
    """2048-column chunks in which more than 256 columns score at or above the k-th best of the row up to that chunk's end.
    The filter's threshold never exceeds the k-th best seen so far, so at least that many columns survive it and the 256-entry
    list overflows whatever it held before: the chunk takes the fallback rounds."""
    out = []
    for c0 in range(0, len(row), WAVE_CHUNK):
        seen = row[:c0 + WAVE_CHUNK]
        if len(seen) < k:
            continue
        _, val = tk.topk(seen[None, :], k)
        kth = val[0, k - 1]
        chunk = row[c0:c0 + WAVE_CHUNK]
        n_ge = len(chunk) if np.isnan(kth) else int((chunk >= kth).sum())       # a NaN threshold is reached by every column
        if n_ge > WAVE_LIST:
            out.append(c0)
    return out


def nan_lane_counts(row):
    """lanes of the first chunk whose columns are all NaN -> (16-byte layout, 4-byte layout)"""
    c = np.arange(min(len(row), WAVE_CHUNK))
    nan = np.isnan(row[:len(c)])
    vec = sum(bool(nan[(c // 4) % 64 == lane].all()) for lane in range(64) if ((c // 4) % 64 == lane).any())
    sca = sum(bool(nan[c % 64 == lane].all()) for lane in range(64) if (c % 64 == lane).any())
    return vec, sca


# ------------------------------------------------------------------------------------------------ geometry, paging
def padded(panel, pad):
    """the panel with `pad` more columns per row (ld = ncols + pad), all +inf: a read past ncols would win the ranking"""
    out = np.full((panel.shape[0], panel.shape[1] + pad), np.inf, panel.dtype)
    out[:, :panel.shape[1]] = panel
    return out


PAGING_NCOLS = (1030, 1500, 2047, 2049, 4099)     # 1500 and 2047 end between two pages of 1024
PAGE_EDGE_ROWS = ((1, KMAX - 1), (2, KMAX), (3, KMAX + 1))   # (row, how many numbers it holds): the rest is NaN


def paging_rows(ncols):
    """seven rows for k > 1024: ties on a grid of quarters; rows 1 - 3 hold 1023, 1024 and 1025 numbers and NaN elsewhere, so the
    first NaN of the ranking ends the first page, starts the second, or follows its first entry; all equal; all NaN; whole numbers"""
    rng = np.random.default_rng([7, ncols])
    rows = np.round(rng.standard_normal((7, ncols)).astype(np.float32) * 4) / 4
    for r, numbers in PAGE_EDGE_ROWS:
        rows[r, rng.permutation(ncols)[numbers:]] = np.nan
    rows[4] = 0.25
    rows[5] = np.nan
    rows[6] = np.round(rows[6])                # a handful of distinct values: long runs of equal scores
    return rows


# ------------------------------------------------------------------------------------------------ merges across panels
def merge_rows(n, k, seed):
    """six query rows over n columns in all: heavy ties on a grid, all equal, a plateau at 0.5 under k // 2 better scores, mostly NaN,
    distinct Gaussians, and k // 3 numbers among NaN (NaN columns belong to the best k: no threshold may pass them over)"""
    rng = np.random.default_rng([seed, n, k])
    f = np.float32
    rows = np.empty((6, n), f)
    rows[0] = np.round(_gauss(rng, n, f) * 4) / 4
    rows[1] = 0.25
    rows[2] = np.where(rng.random(n) < 0.7, f(0.5), (-1 - np.abs(_gauss(rng, n, f))).astype(f))
    rows[2, rng.choice(n, min(n, k // 2), replace=False)] = (1 + np.arange(min(n, k // 2)) / 1024).astype(f)
    rows[3] = np.where(rng.random(n) < 0.66, f(np.nan), np.round(_gauss(rng, n, f) * 2) / 2)
    rows[4] = _gauss(rng, n, f)
    rows[5] = np.nan
    rows[5, rng.choice(n, min(n, k // 3), replace=False)] = np.round(_gauss(rng, min(n, k // 3), f) * 2) / 2
    return rows


def merge_case(name, k, seed=0):
    """-> (panels, offsets) in the order they are handed to pvs_topk_dev; the first without merge, the others with it"""
    if name == "short_then_long":        # fewer than k columns, then a panel the launcher gives to another kernel
        sizes, offsets = [max(k // 2, 1) if k > 1 else 0, 4099], None
    elif name == "two_unequal":
        sizes, offsets = [2049, 333], None
    elif name == "empty_middle":         # an empty panel with merge = 1 hands the running list back as it is
        sizes, offsets = [100, 0, 50], None
    elif name == "empty_last":
        sizes, offsets = [700, 0], None
    elif name == "ties_lower_and_higher":   # the running list comes from global indices 6000 ..; ties arrive from below and above
        sizes, offsets = [777, 4099, 65], [6000, 0, 20000]
    else:
        raise KeyError(name)
    rows = merge_rows(sum(sizes), k, seed)
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    panels = [np.ascontiguousarray(rows[:, cuts[i]:cuts[i + 1]]) for i in range(len(sizes))]
    return panels, (offsets if offsets is not None else [int(c) for c in cuts[:-1]])


MERGE_CASES = ("short_then_long", "two_unequal", "empty_middle", "empty_last", "ties_lower_and_higher")


# ------------------------------------------------------------------------------------------------ list mode
def merge_lists_case(n_lists, k, nq=5, seed=0):
    """-> idx int64 / val float32 (n_lists, nq, k): each list ranked by the rule, scores on a grid of halves so that lists tie with
    each other, ids distinct within a query and spread over [0, 2^32 - 2); odd lists end in unfilled entries, the last query has
    none filled at all, query 1 has exactly k filled entries in all (when there are two lists or more)"""
    rng = np.random.default_rng([seed, n_lists, k])
    idx = np.full((n_lists, nq, k), -1, np.int64)
    val = np.full((n_lists, nq, k), -np.inf, np.float32)
    for q in range(nq - 1):
        ids = rng.choice(0xfffffffe, n_lists * k, replace=False).astype(np.int64).reshape(n_lists, k)
        for l in range(n_lists):
            filled = k - (l * 7 + q) % (k + 1) if l % 2 else k
            if q == 1 and n_lists >= 2:
                filled = k // 2 if l == 0 else (k - k // 2 if l == 1 else 0)
            v = (np.round(rng.standard_normal(filled) * 2) / 2).astype(np.float32)
            if q == 2 and filled:
                v[0] = np.nan
            idx[l, q], val[l, q] = tk.rank_row(ids[l, :filled], v, k)
    return idx, val
