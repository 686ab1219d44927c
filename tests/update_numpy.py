"""NumPy restatement of the index-maintenance entry points (csrc/update.hip, include/pvsim.h "index maintenance").
Everything is integer counting and row movement, so the kernels are held to this twin with np.array_equal (tests/test_gpu_update.py),
and the twin is held to the obvious definitions -- np.cumsum, np.delete, pvsim.compact._sort_into_lists -- in tests/test_update_host.py.
The twin follows the device's structure (tiles, windows, one plan entry per merged row) rather than the one-line definitions."""
import numpy as np

SCAN_TILE = 2048        # PVS_SCAN_TILE


def keep_mask(removed, n: int) -> np.ndarray:
    """pvs_keep_mask_dev: uint8 (n,), 1 everywhere, 0 at the removed indices; indices outside [0, n) are skipped"""
    keep = np.ones(n, np.uint8)
    for i in np.asarray(removed, dtype=np.int64).reshape(-1):
        if 0 <= i < n:
            keep[i] = 0
    return keep


def keep_positions(keep, tile: int = SCAN_TILE) -> np.ndarray:
    """pvs_keep_positions_dev: int64 (n + 1,), pos[i] = kept entries before i, pos[n] = the total.  Three levels, as on the device:
    kept flags per tile, exclusive prefixes of the tile sums inside blocks of `tile` tiles, exclusive prefixes of the block sums."""
    flags = (np.asarray(keep).reshape(-1) != 0).astype(np.int64)
    n = flags.size
    pos = np.zeros(n + 1, np.int64)
    if n == 0:
        return pos
    ntiles = -(-n // tile)
    nblocks = -(-ntiles // tile)
    assert nblocks <= tile, "three levels cover tile^3 flags"
    tile_sum = np.array([flags[t * tile:(t + 1) * tile].sum() for t in range(ntiles)], np.int64)
    tile_ex = np.zeros(ntiles, np.int64)
    block_sum = np.zeros(nblocks, np.int64)
    for b in range(nblocks):
        run = 0
        for t in range(b * tile, min(ntiles, (b + 1) * tile)):
            tile_ex[t] = run
            run += tile_sum[t]
        block_sum[b] = run
    block_ex = np.zeros(nblocks, np.int64)
    run = 0
    for b in range(nblocks):
        block_ex[b] = run
        run += block_sum[b]
    for t in range(ntiles):
        f = flags[t * tile:(t + 1) * tile]
        incl = np.cumsum(f)                                   # the workgroup's scan of its own tile
        pos[t * tile:t * tile + f.size] = block_ex[t // tile] + tile_ex[t] + (incl - f)
    pos[n] = pos[n - 1] + flags[n - 1]
    return pos


def compact_rows(rows, keep, pos) -> np.ndarray:
    """pvs_compact_rows_dev out of place: out[pos[i]] = rows[i] for kept i -> the pos[n] kept rows (what lies beyond is undefined)"""
    rows = np.asarray(rows)
    out = np.empty((int(pos[-1]),) + rows.shape[1:], rows.dtype)
    for i in range(rows.shape[0]):
        if keep[i]:
            out[pos[i]] = rows[i]
    return out


def compact_rows_in_place(buf, keep, pos, first: int = 0, window: int = 64) -> None:
    """pvs_compact_rows_dev with out == rows: rows before `first` are not touched; the kept rows of source window [a, b) are gathered
    into a staging array of at most `window` rows, then written to rows [pos[a], pos[b]).  Asserts the schedule's safety condition."""
    n = len(keep)
    for a in range(first, n, window):
        b = min(n, a + window)
        stage = np.empty((window,) + buf.shape[1:], buf.dtype)
        for i in range(a, b):
            if keep[i]:
                stage[pos[i] - pos[a]] = buf[i]
        assert pos[b] <= b and pos[a] <= a                    # the write ends before the next window's first source row
        buf[pos[a]:pos[b]] = stage[:pos[b] - pos[a]]


def sort_new_rows(new_lists, nlist: int):
    """the host's part of an insert, O(b + nlist): -> (perm int32 (b,): the new rows by (list, arrival); new_off int64 (nlist + 1,))"""
    new_lists = np.asarray(new_lists, dtype=np.int64).reshape(-1)
    counts = np.zeros(nlist, np.int64)
    for l in new_lists:
        counts[l] += 1
    new_off = np.zeros(nlist + 1, np.int64)
    for l in range(nlist):
        new_off[l + 1] = new_off[l] + counts[l]
    fill = new_off[:-1].copy()
    perm = np.zeros(new_lists.size, np.int32)
    for p, l in enumerate(new_lists):
        perm[fill[l]] = p
        fill[l] += 1
    return perm, new_off


def ivf_insert(codes, inv, ids, list_off, new_codes, new_inv, new_off, perm):
    """pvs_ivf_insert_dev -> (codes, inv, ids, list_off) of the n + b merged rows.  One plan entry per merged row j: its list is the
    last l with out_off[l] <= j; inside the list the old rows come first, then the list's new rows in arrival order (ids n + p)."""
    list_off, new_off = np.asarray(list_off, np.int64), np.asarray(new_off, np.int64)
    nlist = list_off.size - 1
    n, b = int(list_off[-1]), int(new_off[-1])
    out_off = list_off + new_off
    m = codes.shape[1] if n else new_codes.shape[1]
    o_codes, o_inv, o_ids = np.zeros((n + b, m), np.uint8), np.zeros(n + b, np.float32), np.zeros(n + b, np.int32)
    for j in range(n + b):
        lo, hi = 0, nlist - 1
        while lo < hi:
            mid = (lo + hi + 1) >> 1
            if out_off[mid] <= j:
                lo = mid
            else:
                hi = mid - 1
        r, old_len = j - out_off[lo], list_off[lo + 1] - list_off[lo]
        if r < old_len:
            s = list_off[lo] + r
            o_codes[j], o_inv[j], o_ids[j] = codes[s], inv[s], ids[s]
        else:
            p = perm[new_off[lo] + (r - old_len)]
            o_codes[j], o_inv[j], o_ids[j] = new_codes[p], new_inv[p], n + p
    return o_codes, o_inv, o_ids, out_off


def ivf_remove(codes, inv, ids, list_off, keep_orig):
    """pvs_ivf_remove_dev -> (codes, inv, ids, list_off) of the survivors: stored row i survives iff keep_orig[ids[i]], its new id is
    pos_orig[ids[i]], stored order is kept, and the new list_off[l] is the stored-order scan read at the old list_off[l]."""
    ids = np.asarray(ids, np.int64)
    pos_orig = keep_positions(keep_orig)
    skeep = np.array([1 if keep_orig[i] else 0 for i in ids], np.uint8)
    spos = keep_positions(skeep)
    o_ids = np.zeros(int(spos[-1]), np.int32)
    for i in range(ids.size):
        if skeep[i]:
            o_ids[spos[i]] = pos_orig[ids[i]]
    return (compact_rows(codes, skeep, spos), compact_rows(inv, skeep, spos), o_ids,
            np.array([spos[o] for o in np.asarray(list_off, np.int64)], np.int64))
