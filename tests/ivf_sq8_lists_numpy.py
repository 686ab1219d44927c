"""NumPy twin of the probed int8 scan by list (csrc/ivf_sq8.hip) on top of ivf_sq8_numpy (imported as it is): the
candidate rows, W, the padding and the result stay that module's; this one restates only who fills which slot.

  base[q][j]   the first slot of probe j in the candidate row of query q: the exclusive prefix sum of the probed lists' lengths in
               probe order; a probe outside [0, nlist) has length 0.  total[q]: the live slots of the row.
  grouping     the pairs (q, j) with a probe in [0, nlist), sorted by list, stably from (q, j) order: (list ascending, query ascending).
               goff[l] .. goff[l + 1]: the pairs of list l; gq[p], gbase[p]: the query and base[q][j] of grouped pair p.
  tiles        a row tile is ROWS consecutive stored rows of one list (a list of length 0 has none), a query tile PAIRS consecutive
               pairs of one group.  Row tile x query tile x (row, pair) writes slot gq W + gbase + (row - list start)."""
import numpy as np

import ivf_sq8_numpy as tw
import sq8_numpy as sq

ROWS = 128
PAIRS = 128
MAX_PAIRS = 1 << 20             # grouped pairs of one query block: 32 MiB of grouping arrays at 32 bytes a pair
CAND_BYTES = 64 << 20           # candidate rows of one query block, 8 bytes a slot (section 14)


def group_probes(probe, list_off):
    """probe int64 (qn, nprobe), list_off int64 (nlist + 1,) -> (base int32 (qn, nprobe), total int32 (qn,), goff int32 (nlist + 1,),
    gq int32 (P,), gbase int32 (P,)) with P = goff[nlist]"""
    probe, list_off = np.asarray(probe, np.int64), np.asarray(list_off, np.int64)
    nlist = len(list_off) - 1
    valid = (probe >= 0) & (probe < nlist)
    safe = np.where(valid, probe, 0)
    length = np.where(valid, list_off[safe + 1] - list_off[safe], 0)
    incl = np.cumsum(length, axis=1)
    base, total = (incl - length).astype(np.int32), incl[:, -1].astype(np.int32)
    key = np.where(valid, probe, nlist).ravel()                       # pairs in (q, j) order
    order = np.argsort(key, kind="stable")
    order = order[key[order] < nlist]
    goff = np.searchsorted(key[order], np.arange(nlist + 1), side="left").astype(np.int32)
    return base, total, goff, (order // probe.shape[1]).astype(np.int32), base.ravel()[order]


def row_tiles(list_off):
    """-> int64 (T, 3): (list, first stored row, rows) of every row tile, in list order"""
    out = []
    for l in range(len(list_off) - 1):
        a, b = int(list_off[l]), int(list_off[l + 1])
        out += [(l, r, min(ROWS, b - r)) for r in range(a, b, ROWS)]
    return np.array(out, np.int64).reshape(-1, 3)


def query_block(nq, W, nprobe, query_block=0):
    """the host rule: the query block of section 14 (64 MiB of 8-byte slots, at most 65535), capped so that QB nprobe <= MAX_PAIRS;
    a positive query_block caps it further"""
    qb = max(1, min(nq, 65535, CAND_BYTES // (8 * W)))
    qb = min(qb, max(1, MAX_PAIRS // nprobe))
    return min(qb, query_block) if query_block > 0 else qb


def fill_counts(probe, list_off, W):
    """how often every slot of the candidate rows (qn, W) is written when the tiles are walked as the kernel walks them"""
    base, total, goff, gq, gbase = group_probes(probe, list_off)
    hit = np.zeros((probe.shape[0], W), np.int64)
    for l, r0, rows in row_tiles(list_off):
        for p0 in range(goff[l], goff[l + 1], PAIRS):
            for p in range(p0, min(p0 + PAIRS, goff[l + 1])):
                s = int(gbase[p]) + (r0 - int(list_off[l]))
                hit[gq[p], s:s + rows] += 1
    return hit, total


def candidate_rows(qcodes, inv_q, probe, list_off, codes, inv_db, ids, scores=sq.scores):
    """the candidate rows of ivf_sq8_numpy.candidate_rows, filled tile by tile"""
    nq, nprobe = probe.shape
    W = tw.width(list_off, nprobe)
    cval, cid = np.full((nq, W), -np.inf, np.float32), np.full((nq, W), -1, np.int32)
    base, total, goff, gq, gbase = group_probes(probe, list_off)
    for l, r0, rows in row_tiles(list_off):
        if goff[l] == goff[l + 1]:
            continue
        qs, bs = gq[goff[l]:goff[l + 1]], gbase[goff[l]:goff[l + 1]].astype(np.int64)
        s = scores(qcodes[qs], inv_q[qs], codes[r0:r0 + rows], inv_db[r0:r0 + rows])
        for t in range(len(qs)):
            at = bs[t] + (r0 - int(list_off[l]))
            cval[qs[t], at:at + rows], cid[qs[t], at:at + rows] = s[t], ids[r0:r0 + rows]
    return cval, cid
