"""NumPy twin of the ASMK maintenance entry points (include/pvsim.h), with the device's structure: entries in
slots with a count per image, a least-significant-digit radix sort over tiles with a digit behind every word for the slots that are
no entries, one plan entry per merged entry for the insert, keep / pos renumbering for the remove.  Plain loops over integers: the
device must agree with this byte for byte, and tests/test_asmk_update_host.py holds it against np.argsort(kind="stable"), np.delete
and list concatenation."""
import numpy as np

SCALE = 1023
TILE_DEFAULT, TILE_MAX, MAX_TILES = 4096, 65536, 65536


def resolve_tile(total, tile_entries=0):
    """the tile the host chooses: tile_entries rounded up to 256 and clamped to 256..65536 (0: 4096), raised so that at most 65536 tiles
    cover `total`"""
    tile = TILE_DEFAULT if tile_entries == 0 else min(max((tile_entries + 255) // 256 * 256, 256), TILE_MAX)
    need = (-(-total // MAX_TILES) + 255) // 256 * 256
    return max(tile, need)


def slot_keys(offsets, count, word, K):
    """key of every slot: the word of an entry, K for a slot beyond its image's count (never read) or a word outside [0, K)"""
    total = int(offsets[-1])
    key = np.full(total, K, np.int64)
    for i in range(len(offsets) - 1):
        lo, rows = int(offsets[i]), int(offsets[i + 1] - offsets[i])
        for t in range(min(max(int(count[i]), 0), rows)):
            w = int(word[lo + t])
            if 0 <= w < K:
                key[lo + t] = w
    return key


def digit(key, K, shift):
    return np.where(key >= K, 256, (key >> shift) & 255)


def radix_pass(key, src, K, shift, tile):
    """one stable pass: digit counts per tile, an exclusive scan over [digit][tile], then every tile walks its items in order"""
    total = len(key)
    ntiles = -(-total // tile)
    d = digit(key, K, shift)
    counts = np.zeros((257, ntiles), np.int64)
    for j in range(total):
        counts[d[j], j // tile] += 1
    flat = counts.reshape(-1)
    base = (np.cumsum(flat) - flat).reshape(257, ntiles)
    out_key, out_src = np.empty_like(key), np.empty_like(src)
    for t in range(ntiles):
        running = base[:, t].copy()
        for j in range(t * tile, min((t + 1) * tile, total)):
            out_key[running[d[j]]], out_src[running[d[j]]] = key[j], src[j]
            running[d[j]] += 1
    return out_key, out_src


def invert(offsets, count, word, sig, K, img_base=0, tile_entries=0):
    """-> (word_off int64 (K + 1,), out_img int32 (E,), out_sig uint32 (E, W)): the defined part of the device's outputs"""
    offsets = np.asarray(offsets, np.int64)
    total = int(offsets[-1])
    sig = np.asarray(sig, np.uint32)                                          # 2-D (total, W), empty ones too
    if total == 0:
        return np.zeros(K + 1, np.int64), np.zeros(0, np.int32), np.zeros((0, sig.shape[1]), np.uint32)
    tile = resolve_tile(total, tile_entries)
    key, src = slot_keys(offsets, count, word, K), np.arange(total, dtype=np.int64)
    for p in range(1 if K <= 256 else 2):
        key, src = radix_pass(key, src, K, 8 * p, tile)
    word_off = np.searchsorted(key, np.arange(K + 1), side="left").astype(np.int64)
    E = int(word_off[K])
    image = np.searchsorted(offsets, src[:E], side="right") - 1               # the last i with offsets[i] <= slot
    return word_off, (img_base + image).astype(np.int32), np.ascontiguousarray(sig[src[:E]])


def weight_sums(offsets, count, word, wt):
    offsets, K = np.asarray(offsets, np.int64), len(wt)
    sums = np.zeros(len(offsets) - 1, np.int64)
    for i in range(len(sums)):
        lo, rows = int(offsets[i]), int(offsets[i + 1] - offsets[i])
        for t in range(min(max(int(count[i]), 0), rows)):
            w = int(word[lo + t])
            if 0 <= w < K:
                sums[i] += SCALE * int(wt[w])
    return sums


def insert(word_off, ent_img, ent_sig, new_off, new_img, new_sig):
    """one plan entry per merged entry j: its word by a binary search of the summed offsets, old entries first"""
    word_off, new_off = np.asarray(word_off, np.int64), np.asarray(new_off, np.int64)
    K, out_off = len(word_off) - 1, word_off + new_off
    total, W = int(out_off[K]), np.asarray(ent_sig).shape[1]                  # signatures are 2-D (E, W), empty ones too
    out_img, out_sig = np.zeros(total, np.int32), np.zeros((total, W), np.uint32)
    for j in range(total):
        lo, hi = 0, K - 1
        while lo < hi:
            mid = (lo + hi + 1) >> 1
            if out_off[mid] <= j:
                lo = mid
            else:
                hi = mid - 1
        r, first = j - int(out_off[lo]), int(word_off[lo])
        old_len = int(word_off[lo + 1]) - first
        if r < old_len:
            out_img[j], out_sig[j] = ent_img[first + r], ent_sig[first + r]
        else:
            s = int(new_off[lo]) + r - old_len
            out_img[j], out_sig[j] = new_img[s], new_sig[s]
    return out_off, out_img, out_sig


def keep_positions(keep):
    pos = np.zeros(len(keep) + 1, np.int64)
    np.cumsum(np.asarray(keep) != 0, out=pos[1:])
    return pos


def remove(word_off, ent_img, ent_sig, keep, pos):
    """keep uint8 (N,), pos int64 (N + 1,) by image id -> the surviving entries in stored order with ids pos[id]"""
    word_off, N, E = np.asarray(word_off, np.int64), len(keep), len(ent_img)
    flag = np.zeros(E + 1, np.int64)
    for e in range(E):
        i = int(ent_img[e])
        flag[e] = 1 if 0 <= i < N and keep[i] else 0
    spos = np.cumsum(flag) - flag
    out_img = np.zeros(int(spos[E]), np.int32)
    out_sig = np.zeros((int(spos[E]), np.asarray(ent_sig).shape[1]), np.uint32)
    for e in range(E):
        if flag[e]:
            out_img[spos[e]], out_sig[spos[e]] = pos[ent_img[e]], ent_sig[e]
    return spos[word_off].astype(np.int64), out_img, out_sig


# ------------------------------------------------------------------------------------------------ inputs shared by the tests
def make_slots(rng, n, E, K, W, flavor="random"):
    """n images holding E entries in all, in slots as pvs_asmk_aggregate_dev leaves them; unused slots hold 0xFF bytes.  With 40
    images, image 0, 20 and 39 have no rows and image 5 has rows but no entries.  flavor: "random"; "distinct" (no word twice in the
    batch, K >= E); "shared" (word K - 1 in every image that has entries); "bad" (a few images also carry a word of -1 and a word of
    K inside their count: both are dropped).  At K = 65536 the words 0 and 65535 are held.
    -> (offsets, count, word, sig, per-image [(words, sigs)] of the entries that count)"""
    hollow = {0, 20, 39, 5} if n == 40 else set()
    full = [i for i in range(n) if i not in hollow]
    share = {i: E // len(full) + (1 if r < E % len(full) else 0) for r, i in enumerate(full)} if full else {}
    assert all(c <= K for c in share.values()) and (full or E == 0)
    pool = rng.permutation(K) if flavor == "distinct" else None
    if pool is not None and K == 65536:
        pool = np.concatenate([[0, 65535], pool[(pool != 0) & (pool != 65535)]])
    at, ents, rows, extra = 0, [], [], {}
    for i in range(n):
        c = share.get(i, 0)
        if flavor == "distinct":
            w, at = pool[at:at + c], at + c
        else:
            w = rng.permutation(K)[:c]
            if flavor == "shared" and c and K - 1 not in w:
                w[0] = K - 1
            if K == 65536 and i == (full[0] if full else -1) and c >= 2:
                w = np.unique(np.concatenate([[0, 65535], w]))[:c]
                w[-1] = 65535
        w = np.sort(np.unique(w)).astype(np.int32)
        assert len(w) == c
        ents.append((w, rng.randint(0, 1 << 32, (c, W), dtype=np.uint64).astype(np.uint32)))
        extra[i] = 2 if flavor == "bad" and c and len(extra) < 8 and i % 2 == 0 else 0
        rows.append(c + extra[i] + (3 if i == 5 and n == 40 else i % 3 if i not in hollow else 0))
    off = np.zeros(n + 1, np.int64)
    np.cumsum(rows, out=off[1:])
    total = int(off[-1])
    word, sig, count = np.full(total, -1, np.int32), np.full((total, W), 0xFFFFFFFF, np.uint32), np.zeros(n, np.int32)
    for i, (w, s) in enumerate(ents):
        lo, c = int(off[i]), len(w)
        if extra[i]:                                                         # -1 in front, K behind: inside the count, dropped
            word[lo], word[lo + c + 1] = -1, K
            sig[lo], sig[lo + c + 1] = 7, 9
            lo += 1
        word[lo:lo + c], sig[lo:lo + c], count[i] = w, s, c + extra[i]
    return off, count, word, sig, ents
