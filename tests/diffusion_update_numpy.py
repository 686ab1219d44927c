"""NumPy twin of graph maintenance after add / remove (include/pvsim.h "graph maintenance").

A mutable graph stores, per row i, its LIST: the first kg rows j != i of row i's ranking in the order of tests/topk_numpy.py (score
descending, index ascending, NaN last, -0 and +0 tie), as nbr int32 (N, kg) and sim (N, kg), the values the ranking returned.  The
functions of the first part work on look-ups into a score matrix S[i][j] (query i, column j; S need not be symmetric, and S[i][i] need
not be the largest of its row): the lists from scratch, `add` by merge, `remove` by damage / remap / re-rank.  The second part restates
the six device entry points element by element."""
import numpy as np

import topk_numpy as tk
from diffusion_numpy import affinity, drop_self


# ------------------------------------------------------------------------------------------------ the order
def before(xv, xid, yv, yid):
    """entry x comes before entry y: numbers before NaNs, the larger number first (-0 and +0 tie), then the smaller id"""
    xn, yn = bool(np.isnan(xv)), bool(np.isnan(yv))
    if xn != yn:
        return yn
    if not xn:
        if xv > yv:
            return True
        if xv < yv:
            return False
    return int(xid) < int(yid)


# ------------------------------------------------------------------------------------------------ lists on a score matrix
def ranked_lists(S, rows, kg):
    """rows `rows` of S ranked against every column to depth kg + 1, self dropped -> (nbr int32 (len(rows), kg), sim (len(rows), kg))"""
    S = np.asarray(S)
    ids = np.arange(S.shape[1], dtype=np.int64)
    out = [tk.rank_row(ids, S[i], kg + 1) for i in rows]
    idx = np.array([o[0] for o in out], np.int64).reshape(len(rows), kg + 1)
    val = np.array([o[1] for o in out], S.dtype).reshape(len(rows), kg + 1)
    nbr, sim = drop_self(idx, val, np.asarray(rows))
    return nbr.astype(np.int32), sim


def lists_from_scratch(S, kg):
    """what a build keeps: the list of every row of the square score matrix S"""
    return ranked_lists(S, np.arange(S.shape[0]), kg)


def first_others(S, i, kg):
    """the definition itself: the first kg columns j != i of row i's complete ranking -> (ids, values)"""
    n = S.shape[1]
    idx, val = tk.rank_row(np.arange(n, dtype=np.int64), S[i], n)
    keep = idx != i
    return idx[keep][:kg].astype(np.int32), val[keep][:kg]


def add_by_merge(nbr, sim, S, kg):
    """(nbr, sim) of the first N rows of S; S (N + b, N + b) is the score matrix with the b new rows and columns at the end.  New rows
    are ranked against everything; an old row is ranked against the new columns alone to depth min(kg, b) and merged with its list"""
    N, M = nbr.shape[0], S.shape[0]
    b = M - N
    c = min(kg, b)
    out_nbr, out_sim = np.empty((M, kg), np.int32), np.empty((M, kg), sim.dtype)
    out_nbr[N:], out_sim[N:] = ranked_lists(S, np.arange(N, M), kg)
    rel = np.arange(b, dtype=np.int64)
    cand = [tk.rank_row(rel, S[i, N:], c) for i in range(N)]
    cidx = np.array([o[0] for o in cand], np.int64).reshape(N, c)
    cval = np.array([o[1] for o in cand], sim.dtype).reshape(N, c)
    out_nbr[:N], out_sim[:N] = merge(nbr, sim, cidx, cval, N, M)
    return out_nbr, out_sim


def remove_by_damage(nbr, sim, S_new, removed, kg):
    """(nbr, sim) of N rows, `removed` the indices that leave, S_new the score matrix of the survivors in surviving order -> (nbr, sim,
    reranked): undamaged lists are renumbered and move up, damaged ones are ranked again by their own new id"""
    N = nbr.shape[0]
    removed = np.unique(np.asarray(removed, np.int64))
    if kg > N - removed.size - 1:
        raise ValueError(f"kg = {kg} neighbours per row need at least {kg + 1} rows, {N - removed.size} would survive")
    keep = np.ones(N, np.uint8)
    keep[removed] = 0
    pos = np.concatenate([[0], np.cumsum(keep != 0)]).astype(np.int64)
    flag = damage(nbr, keep)
    kept = keep != 0
    out_nbr, out_sim = remap(nbr, keep, pos)[kept], sim[kept].copy()
    own = np.flatnonzero(flag[kept])                           # the damaged rows in the new numbering
    if own.size:
        out_nbr[own], out_sim[own] = ranked_lists(S_new, own, kg)
    return out_nbr, out_sim, int(own.size)


# ------------------------------------------------------------------------------------------------ the six entry points
def lists(idx, val, own, N, nbr, sim):
    """pvs_graph_lists_dev: rankings idx int64 / val float32 (b, kg + 1) of the rows `own` (b,) -> rows own of nbr / sim, in place:
    drop self with the similarity kept; an index outside [0, N) is stored as -1; a row whose own lies outside [0, N) is not written"""
    own = np.asarray(own, np.int64)
    i, v = drop_self(np.asarray(idx), np.asarray(val), own)
    ok = (own >= 0) & (own < N)
    nbr[own[ok]] = np.where((i >= 0) & (i < N), i, -1).astype(np.int32)[ok]
    sim[own[ok]] = v[ok]


def merge(nbr, sim, cidx, cval, col_offset, N):
    """pvs_graph_merge_dev: per row a two-way merge of the stored list and the candidates (id = cidx + col_offset, cidx < 0 skipped)
    by `before`, the stored entry first where neither comes before the other, cut after kg entries; values move as they stand"""
    rows, kg = nbr.shape
    c = cidx.shape[1]
    out_nbr, out_sim = np.empty_like(nbr), np.empty_like(sim)
    for i in range(rows):
        p = q = 0
        for t in range(kg):
            while q < c and cidx[i, q] < 0:
                q += 1
            if q < c and before(cval[i, q], cidx[i, q] + col_offset, sim[i, p], nbr[i, p]):
                j = int(cidx[i, q]) + col_offset
                out_nbr[i, t], out_sim[i, t] = (j if 0 <= j < N else -1), cval[i, q]
                q += 1
            else:
                out_nbr[i, t], out_sim[i, t] = nbr[i, p], sim[i, p]
                p += 1
    return out_nbr, out_sim


def damage(nbr, keep):
    """pvs_graph_damage_dev: flag[i] = 1 iff row i is kept and some slot names a row in [0, N) that is not"""
    N = nbr.shape[0]
    valid = (nbr >= 0) & (nbr < N)
    gone = valid & (np.asarray(keep)[np.where(valid, nbr, 0)] == 0)
    return (gone.any(axis=1) & (np.asarray(keep) != 0)).astype(np.uint8)


def remap(nbr, keep, pos, out=None):
    """pvs_graph_remap_dev: the slots of the kept rows through pos, -1 for a removed or invalid neighbour; the rows that are not
    kept keep what `out` held (a copy of nbr where none is given)"""
    N = nbr.shape[0]
    keep = np.asarray(keep)
    out = nbr.copy() if out is None else out
    valid = (nbr >= 0) & (nbr < N)
    j = np.where(valid, nbr, 0)
    new = np.where(valid & (keep[j] != 0), np.asarray(pos)[j], -1).astype(np.int32)
    out[keep != 0] = new[keep != 0]
    return out


def gather_rows(rows, ids):
    """pvs_graph_gather_rows_dev: out[p] = rows[ids[p]], zeros for an id outside [0, n)"""
    rows, ids = np.asarray(rows), np.asarray(ids, np.int64)
    ok = (ids >= 0) & (ids < rows.shape[0])
    out = rows[np.where(ok, ids, 0)].copy()
    out[~ok] = 0
    return out


def affinity_sim(sim, gamma):
    """pvs_graph_affinity_sim_dev: the affinity of diffusion_numpy of the float32 similarities, upcast exactly"""
    return affinity(np.asarray(sim, np.float32), gamma)
