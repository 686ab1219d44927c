"""Workspace slots that grow between calls while carved layouts are in use (csrc/workspace.hpp): one fresh context, a small
neighbour search, a larger one (its panel, list and norm blocks are all re-allocated), a filtered top-k that carves the list block
with another layout, and the first search again."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 15   # checked on the CPU: the smallest relative gap of the float64 references below is 2.7e-4, 1.1e-5 and 1.2e-5 (> 1e-6)


def _rows(rng, n, L):
    """n float32 rows around 40 directions: neighbours and scores are well separated"""
    proto = rng.standard_normal((40, L))
    return (proto[np.arange(n) % 40] + 0.6 * rng.standard_normal((n, L))).astype(np.float32)


def _assert_unambiguous(best_first, k):
    """every gap between consecutive values among the k + 1 best of every query exceeds 1e-6 relative (no query is excluded)"""
    a, b = best_first[:, :k], best_first[:, 1:k + 1]
    gap = np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)
    assert gap.min() > 1e-6, gap.min()


def _knn_ref(x, k):
    x = x.astype(np.float64)
    d = np.concatenate([((x[i:i + 100, None, :] - x[None, :, :]) ** 2).sum(-1) for i in range(0, len(x), 100)])
    order = np.argsort(d, axis=1, kind="stable")[:, :k + 1]
    _assert_unambiguous(np.take_along_axis(d, order, 1), k)
    return order[:, :k]


def _cosine_ref(x, k):
    x = x.astype(np.float64)
    xn = x / np.linalg.norm(x, axis=1, keepdims=True)
    s = xn @ xn.T
    order = np.argsort(-s, axis=1, kind="stable")[:, :k + 1]
    _assert_unambiguous(np.take_along_axis(s, order, 1), k)
    return order[:, :k]


def test_slots_grow_between_calls_with_carved_layouts():
    import pvsim
    rng = np.random.default_rng(SEED)
    small, large, enc = _rows(rng, 300, 32), _rows(rng, 1500, 32), _rows(rng, 600, 64)
    ctx = pvsim.Context(0)   # a context of its own: every slot starts empty

    def knn(x, k):
        n, L = x.shape
        d_x, d_idx, d_dist = ctx.buffer(x.nbytes).upload(x), ctx.buffer(n * k * 8), ctx.buffer(n * k * 8)
        st = ctx.l2_knn_dev(d_x.ptr, n, d_x.ptr, n, L, False, k, d_idx.ptr, d_dist.ptr, stats=True)
        out = d_idx.download((n, k), np.int64), d_dist.download((n, k), np.float64), st
        for b in (d_x, d_idx, d_dist):
            b.free()
        return out

    try:
        idx1, dist1, st1 = knn(small, 3)
        idx2, _, st2 = knn(large, 7)
        n, L, k = enc.shape[0], enc.shape[1], 5
        d_x, d_inv = ctx.buffer(enc.nbytes).upload(enc), ctx.buffer(n * 4)
        d_idx, d_val = ctx.buffer(n * k * 8), ctx.buffer(n * k * 4)
        ctx.row_inv_norms_dev(d_x.ptr, n, L, d_inv.ptr)
        st3 = ctx.cosine_topk_filtered_dev(d_x.ptr, n, d_x.ptr, n, L, d_inv.ptr, d_inv.ptr, k, d_idx.ptr, d_val.ptr)
        ctx.sync()
        idx3 = d_idx.download((n, k), np.int64)
        for b in (d_x, d_inv, d_idx, d_val):
            b.free()
        idx4, dist4, _ = knn(small, 3)
    finally:
        ctx.close()

    assert st1["filtered"] and st2["filtered"], "the float32 path with the carved list block did not run"
    assert st3["filtered"], "the prefilter declined: its list block was never carved"
    assert np.array_equal(idx4, idx1) and np.array_equal(dist4.view(np.int64), dist1.view(np.int64))
    assert np.array_equal(idx1, _knn_ref(small, 3))
    assert np.array_equal(idx2, _knn_ref(large, 7))
    assert np.array_equal(idx3, _cosine_ref(enc, k))
