"""Behavioural novelty stated on the host (include/rem2d_novelty.h), shared by tests/test_novelty_host.py (numpy alone) and
tests/test_novelty_gpu.py: what es_model.py is for the evolution strategy.  Written from the header, not from the kernels.

* ``score_model``: novelty float64 [G] from desc [G, B], the archive [M, cap, B] and total [M].
* ``add_model``: the archive and total after an add, and who was added.
* ``describe_update``: one rem2d_worlds_describe call on host arrays of (steps, frozen, px_root, py_root).
* ``rate_threshold``: floor(rate * 2^32), what the Python layer hands to the library.

The ``variant`` names of ``score_model`` state WRONG arithmetic, for the teeth test of test_novelty_host.py.

NaNs: a computed NaN has no defined sign or payload, so ``bits64`` maps every NaN to one pattern before a comparison.
"""
import numpy as np

from evolve_model import philox, rate_threshold, seed_key  # noqa: F401  (rate_threshold: re-exported)

f32, f64 = np.float32, np.float64
u32, u64 = np.uint32, np.uint64
NOVELTY_DOMAIN = 9                                         # counter word 3 of the add; evolve has 0 .. 4, the strategy 5 .. 8
VARIANTS = ("reverse", "acc64", "fma", "self", "no_archive", "descending")


def sq_dists(x, y, variant=None):
    """d2 float32 [len(x), len(y)]: d2 = 0; for i ascending: t = x_i - y_i; d2 = d2 + (t * t), each one float32 operation"""
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    B = x.shape[1]
    order = range(B - 1, -1, -1) if variant == "reverse" else range(B)
    with np.errstate(all="ignore"):
        if variant == "acc64":
            d2 = np.zeros((x.shape[0], y.shape[0]), f64)
            for i in order:
                t = x[:, i, None] - y[None, :, i]
                d2 = d2 + (t * t).astype(f64)
            return d2.astype(f32)
        d2 = np.zeros((x.shape[0], y.shape[0]), f32)
        for i in order:
            t = x[:, i, None] - y[None, :, i]
            assert t.dtype == f32
            if variant == "fma":                           # the exact product (48 bits fit binary64), rounded once with the sum
                d2 = (t.astype(f64) * t.astype(f64) + d2.astype(f64)).astype(f32)
            else:
                d2 = d2 + (t * t)
        assert d2.dtype == f32
    return d2


def live_entries(total, cap):
    return np.minimum(np.maximum(np.asarray(total, np.int64), 0), int(cap))


def score_model(desc, group_size, k, archive=None, total=None, variant=None):
    """novelty float64 [G].  archive [M, cap, B] / total [M] (None: no archive)"""
    assert variant is None or variant in VARIANTS
    desc = np.asarray(desc, f32)
    G, B = desc.shape
    S, k = int(group_size), int(k)
    assert S >= 1 and G % S == 0 and 1 <= k <= 32 and 1 <= B <= 32
    M = G // S
    cap = 0 if archive is None else np.asarray(archive).shape[1]
    live = live_entries(total, cap) if cap else np.zeros(M, np.int64)
    out = np.zeros(G, f64)
    inf = f32(np.inf)
    for b in range(M):
        x = desc[b * S:(b + 1) * S]
        d2 = sq_dists(x, x, variant)
        if variant != "self":
            d2[np.arange(S), np.arange(S)] = inf           # by index, not by value
        if live[b] and variant != "no_archive":
            d2 = np.concatenate([d2, sq_dists(x, np.asarray(archive, f32)[b, :live[b]], variant)], axis=1)
        d2 = np.where(np.isfinite(d2), d2, inf)
        d2.sort(axis=1)
        best = d2[:, :k]
        n = (best < inf).sum(axis=1)                       # k' per row
        with np.errstate(all="ignore"):
            root = np.sqrt(best)                           # float32 sqrt: correctly rounded (test_novelty_host checks it)
        assert root.dtype == f32
        acc = np.zeros(S, f64)
        cols = range(best.shape[1] - 1, -1, -1) if variant == "descending" else range(best.shape[1])
        for j in cols:                                     # in order, one binary64 addition each
            acc = np.where(best[:, j] < inf, acc + root[:, j].astype(f64), acc)
        with np.errstate(all="ignore"):
            nov = np.where(n > 0, acc / np.maximum(n, 1).astype(f64), 0.0)
        nov[~np.isfinite(x).all(axis=1)] = np.nan
        out[b * S:(b + 1) * S] = nov
    return out


def admitted(desc, generation, seed, threshold, mask=None):
    """bool [G]: the rows an add takes"""
    desc = np.asarray(desc, f32)
    G = desc.shape[0]
    x0 = philox((0, np.arange(G, dtype=np.int64), generation, NOVELTY_DOMAIN), seed_key(seed))[0]
    take = np.isfinite(desc).all(axis=1) & (x0.astype(u64) < u64(int(threshold)))
    if mask is not None:
        take &= np.asarray(mask) != 0
    return take


def add_model(desc, group_size, archive, total, generation, seed, threshold, mask=None):
    """-> (archive [M, cap, B] float32, total [M] int64, taken bool [G]); the inputs are not written"""
    desc = np.asarray(desc, f32)
    G, B = desc.shape
    S = int(group_size)
    M = G // S
    total = np.array(total, np.int64)
    archive = np.array(archive, f32).reshape(M, -1, B)
    cap = archive.shape[1]
    take = admitted(desc, generation, seed, threshold, mask)
    for b in range(M):
        rows = np.flatnonzero(take[b * S:(b + 1) * S]) + b * S
        n = len(rows)
        for j, c in enumerate(rows):
            if cap and j >= n - cap:
                archive[b, (int(total[b]) + j) % cap] = desc[c]
        total[b] += n
    return archive, total, take


def describe_update(rows, steps, frozen, px, py, period, n_samples):
    """One describe call: rows float32 [N, 2 K] is written in place.  A creature with frozen != 0 writes nothing; the others
    write (px, py) to every slot k with (k + 1) * period >= steps."""
    K = int(n_samples)
    at = (np.arange(K, dtype=np.int64) + 1) * int(period)
    write = (np.asarray(frozen) == 0)[:, None] & (at[None, :] >= np.asarray(steps, np.int64)[:, None])
    rows[:, 0::2] = np.where(write, np.asarray(px, f32)[:, None], rows[:, 0::2])
    rows[:, 1::2] = np.where(write, np.asarray(py, f32)[:, None], rows[:, 1::2])
    return rows


def combine_util(util_f, util_n, weights):
    """int32 [G]: w_f util_f + w_n util_n in int32 arithmetic"""
    wf, wn = (np.int32(int(w)) for w in weights)
    with np.errstate(over="ignore"):
        return (wf * np.asarray(util_f, np.int32) + wn * np.asarray(util_n, np.int32)).astype(np.int32)


def bits64(a):
    """float64 array -> uint64 words, every NaN mapped to one pattern"""
    a = np.array(a, f64)
    a[np.isnan(a)] = f64("nan")
    return a.view(u64)


def bits32(a):
    a = np.array(a, f32)
    a[np.isnan(a)] = f32("nan")
    return a.view(u32)


def episode_words(px):
    """frozen int32 [T + 1, N] from the root's x after reset and after each of T steps, by the step's own bookkeeping: the wall of
    death advances 0.04 a step (a binary64 running sum), the reward is the root's x, or -100 once the root is left of 0 or behind
    the wall; a reward below -10 or above 100 ends evaluate()'s loop for the creature (REM2D_F_FROZEN), for good"""
    px = np.asarray(px, f32)
    frozen = np.zeros(px.shape, np.int32)
    wod = 0.0
    for t in range(1, px.shape[0]):
        wod += 0.04
        r = px[t].astype(f64)
        rew = np.where((r < 0.0) | (wod > r), -100.0, r)
        frozen[t] = frozen[t - 1] | (rew < -10.0) | (rew > 100.0)
    return frozen
