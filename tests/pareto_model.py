"""Pareto ranking stated on the host (include/rem2d_pareto.h), shared by tests/test_pareto_host.py (numpy alone) and
tests/test_pareto_gpu.py: what novelty_model.py is for the novelty score.  Written from the header, not from the kernels.

* ``rank_model``: (front int32 [G], crowd float64 [G], util int32 [G], n_fronts int32 [M]) from obj [G, K].
* ``local_model``: (local float64 [G], neighbours int32 [G]) from desc [G, B] and fitness [G].

The ``variant`` names state WRONG arithmetic, for the teeth test of test_pareto_host.py.

NaNs: a computed NaN has no defined sign or payload, so ``bits64`` maps every NaN to one pattern before a comparison.
"""
import numpy as np

from novelty_model import bits64, sq_dists  # noqa: F401  (bits64: re-exported; sq_dists: the header's d2, stated once)

f32, f64 = np.float32, np.float64
RANK_VARIANTS = ("weak", "nonstrict", "by_row", "reverse")
LOCAL_VARIANTS = ("self", "high_tie", "le")


def fronts_of(x, adm, variant=None):
    """front int [S] of one block (-1: unadmitted) and F, by the peel: 1 + the greatest front among the dominators"""
    S = x.shape[0]
    ge = (x[:, None, :] >= x[None, :, :]).all(axis=2)       # [i, j]: i >= j in every objective
    gt = (x[:, None, :] > x[None, :, :]).any(axis=2)
    dom = ge & (True if variant == "weak" else gt) & adm[:, None] & adm[None, :]   # [i, j]: i dominates j
    if variant == "weak":
        np.fill_diagonal(dom, False)
    front = np.full(S, -1, np.int64)
    left = adm.copy()
    waiting = dom.sum(axis=0)                               # the dominators of a row that are still left
    r = 0
    while left.any():
        free = left & (waiting == 0)
        if not free.any():                                  # (only the WRONG weak variant: equal rows dominate each other)
            free = left.copy()
        front[free] = r
        left &= ~free
        waiting = waiting - dom[free].sum(axis=0)
        r += 1
    return front, r


def crowd_of(x, front, adm, variant=None):
    """crowd float64 [S] of one block from its fronts"""
    S, K = x.shape
    crowd = np.zeros(S, f64)
    order = range(K - 1, -1, -1) if variant == "reverse" else range(K)
    inf = f64(np.inf)
    for f in np.unique(front[adm]):
        rows = np.flatnonzero(front == f)
        v = x[rows]                                         # [n, K]
        acc = np.zeros(len(rows), f64)
        open_ = np.zeros(len(rows), bool)
        for m in order:
            col = v[:, m]
            if variant == "nonstrict":                      # the neighbours of a sort: an equal value of another row counts
                idx = np.arange(len(rows))
                other = idx[:, None] != idx[None, :]
                lt = (col[None, :] <= col[:, None]) & other
                gtm = (col[None, :] >= col[:, None]) & other
            else:
                lt = col[None, :] < col[:, None]            # [c, j]: j strictly below c
                gtm = col[None, :] > col[:, None]
            below = np.where(lt, col[None, :], -inf).max(axis=1)
            above = np.where(gtm, col[None, :], inf).min(axis=1)
            open_ |= ~lt.any(axis=1) | ~gtm.any(axis=1)
            with np.errstate(all="ignore"):
                acc = acc + ((above - below) / (col.max() - col.min()))
        crowd[rows] = np.where(open_, inf, acc)
    return crowd


def util_of(front, crowd, variant=None):
    """2 L + E - (S - 1) on the order (front ascending, crowd descending, a NaN crowd lowest and level with a NaN)"""
    S = front.shape[0]
    nanc = np.isnan(crowd)
    with np.errstate(invalid="ignore"):
        cgt = (crowd[:, None] > crowd[None, :]) | (~nanc[:, None] & nanc[None, :])      # [c, j]: crowd c above crowd j
    better = (front[:, None] < front[None, :]) | ((front[:, None] == front[None, :]) & cgt)
    level = ~better & ~better.T
    np.fill_diagonal(level, False)
    L, E = better.sum(axis=1), level.sum(axis=1)
    if variant == "by_row":                                 # ties go to the lower row instead of being averaged
        idx = np.arange(S)
        L = L + (level & (idx[:, None] < idx[None, :])).sum(axis=1)
        return 2 * L - (S - 1)
    return 2 * L + E - (S - 1)


def rank_model(obj, group_size, variant=None):
    """-> (front int32 [G], crowd float64 [G], util int32 [G], n_fronts int32 [M])"""
    assert variant is None or variant in RANK_VARIANTS
    obj = np.asarray(obj, f64)
    if obj.ndim == 1:
        obj = obj[:, None]
    G, K = obj.shape
    S = int(group_size)
    assert 1 <= S <= 1024 and G % S == 0 and 1 <= K <= 4
    M = G // S
    front, crowd, util, nf = np.zeros(G, np.int32), np.zeros(G, f64), np.zeros(G, np.int32), np.zeros(M, np.int32)
    for b in range(M):
        x = obj[b * S:(b + 1) * S]
        adm = np.isfinite(x).all(axis=1)
        f, F = fronts_of(x, adm, variant)
        c = crowd_of(x, f, adm, variant)
        f = np.where(adm, f, F)
        front[b * S:(b + 1) * S], crowd[b * S:(b + 1) * S], nf[b] = f, c, F
        util[b * S:(b + 1) * S] = util_of(f, c, variant)
    return front, crowd, util, nf


def below(a, b):
    """a below b in the evolve header's order on fitness: a NaN is below every number and not below a NaN; equal is not below"""
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    with np.errstate(invalid="ignore"):
        return (a < b) | (np.isnan(a) & ~np.isnan(b))


def local_model(desc, fitness, k, group_size, variant=None):
    """-> (local float64 [G], neighbours int32 [G])"""
    assert variant is None or variant in LOCAL_VARIANTS
    desc, fit = np.asarray(desc, f32), np.asarray(fitness, f64)
    G, B = desc.shape
    S, k = int(group_size), int(k)
    assert S >= 1 and G % S == 0 and 1 <= k <= 32 and 1 <= B <= 32 and fit.shape == (G,)
    local, neigh = np.zeros(G, f64), np.zeros(G, np.int32)
    inf = f32(np.inf)
    idx = np.arange(S)
    for b in range(G // S):
        x, f = desc[b * S:(b + 1) * S], fit[b * S:(b + 1) * S]
        d2 = sq_dists(x, x)
        if variant != "self":
            d2[idx, idx] = inf                              # by index, not by value
        d2 = np.where(np.isfinite(d2), d2, inf)
        cols = idx[::-1] if variant == "high_tie" else idx
        order = cols[np.argsort(d2[:, cols], axis=1, kind="stable")][:, :k]            # ascending (d2, row index)
        kept = np.take_along_axis(d2, order, axis=1) < inf
        beaten = (f[order] <= f[:, None]) if variant == "le" else below(f[order], f[:, None])
        cnt = (kept & beaten).sum(axis=1).astype(f64)
        cnt[~np.isfinite(x).all(axis=1)] = np.nan
        local[b * S:(b + 1) * S], neigh[b * S:(b + 1) * S] = cnt, kept.sum(axis=1)
    return local, neigh
