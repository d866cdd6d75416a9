"""The evolution strategy for device policies stated on the host (include/rem2d_es.h), shared by tests/test_es_host.py (numpy alone)
and tests/test_es_gpu.py: what evolve_model.py is for rem2d_policy_evolve.  Written from the header, not from the kernels.

* ``sample_model``: the four child arrays [M S, ...] from the four mean arrays [M, ...].
* ``shape_model``: util int32 [M S] from fitness, on evolve_model's order on fitness.
* ``update_model``: the four new mean arrays from the mean and util; the weighted sums in int64 numpy arithmetic.
* ``step_for``: the binary32 step the Python layer hands to the library.

The keyword arguments that default to False / None state WRONG variants, for the teeth tests of test_es_host.py.

NaNs: every child word and every new mean word is computed, and a computed NaN has no defined sign or payload, so ``bits`` maps
every NaN to one pattern before a comparison (evolve_model.bits does the same at hit elements).
"""
import numpy as np

from evolve_model import NOISE_BIAS, NOISE_SCALE, greater, philox, seed_key

f32 = np.float32
u32, u64 = np.uint32, np.uint64
ES_DOMAIN0 = 4                                             # counter word 3 is 4 + k, k = 1 .. 4 for w1, b1, w2, b2


def draw_sums(n, anchors, k, seed, generation):
    """s int64 [len(anchors), n]: the centred sum of the six 16-bit halves of x1, x2, x3 for elements 0 .. n-1 of array k (1 .. 4)"""
    i = np.arange(n, dtype=np.int64)[None, :]
    a = np.asarray(anchors, np.int64).reshape(-1, 1)
    _, x1, x2, x3 = philox((i, a, generation, ES_DOMAIN0 + k), seed_key(seed))
    s = np.zeros(x1.shape, np.int64)
    for x in (x1, x2, x3):
        s += (x & u32(0xffff)).astype(np.int64) + (x >> u32(16)).astype(np.int64)
    return s - NOISE_BIAS


def noise_of(s):
    """z float32 = (float)s * C; the conversion is exact"""
    sf = s.astype(f32)
    assert np.array_equal(sf.astype(np.int64), s)
    return sf * NOISE_SCALE


def sample_model(mean, group_size, sigma, seed, generation, same_sign=False, own_counter=False):
    """mean: (w1 [M, D, H], b1 [M, H], w2 [M, H, MB], b2 [M, MB]) -> the four child arrays [M S, ...].
    same_sign: the WRONG odd child that shares the even child's sign; own_counter: the WRONG odd child drawn on its own index"""
    mean = [np.asarray(a, f32) for a in mean]
    M, S = mean[0].shape[0], int(group_size)
    assert S >= 2 and S % 2 == 0
    c = np.arange(M * S, dtype=np.int64)
    anchor = c & ~np.int64(1)                              # b S + 2 q: S is even
    odd = (c & 1) == 1
    kids = []
    for k, a in enumerate(mean):
        flat = a.reshape(M, -1)
        n = flat.shape[1]
        z = noise_of(draw_sums(n, c if own_counter else anchor, k + 1, seed, generation))
        with np.errstate(all="ignore"):
            t = f32(sigma) * z
            if not same_sign:
                t = np.where(odd[:, None], -t, t)
            out = flat[c // S] + t
        assert out.dtype == f32 and t.dtype == f32
        kids.append(out.reshape((M * S,) + a.shape[1:]))
    return kids


PAIRWISE_MAX = 2048                                        # blocks up to here are counted pair by pair, as the header words it


def block_util_sorted(f):
    """2 L + E - (S - 1) of one block by sorting: what the pairwise count gives (test_es_host holds the two together), for blocks
    whose S x S comparisons would not fit in memory"""
    f = np.asarray(f, np.float64)
    S, isn = f.shape[0], np.isnan(f)
    n_nan = int(isn.sum())
    v = np.sort(f[~isn])                                   # (-0 and +0 compare equal: they land in one run)
    lo, hi = np.searchsorted(v, f, "left"), np.searchsorted(v, f, "right")
    L = np.where(isn, 0, n_nan + lo)
    E = np.where(isn, n_nan - 1, hi - lo - 1)
    return 2 * L + E - (S - 1)


def shape_model(fitness, group_size, low_ties=False):
    """util int32 [G]: 2 L + E - (S - 1) within blocks of S.  low_ties: the WRONG ranks whose ties go to the lower index"""
    fit = np.asarray(fitness, np.float64)
    S = int(group_size)
    assert fit.shape[0] % S == 0
    util = np.zeros(fit.shape[0], np.int64)
    for b in range(0, fit.shape[0], S):
        f = fit[b:b + S]
        if S > PAIRWISE_MAX and not low_ties:
            util[b:b + S] = block_util_sorted(f)
            continue
        above = greater(f[:, None], f[None, :])            # [c, o]: c above o
        under = above.T
        level = ~above & ~under
        np.fill_diagonal(level, False)
        L, E = above.sum(axis=1), level.sum(axis=1)
        if low_ties:
            idx = np.arange(S)
            L = L + (level & (idx[None, :] < idx[:, None])).sum(axis=1)
            util[b:b + S] = 2 * L - (S - 1)
        else:
            util[b:b + S] = 2 * L + E - (S - 1)
    return util.astype(np.int32)


def step_for(lr, group_size, sigma):
    S = int(group_size)
    return f32(float(lr) / (2.0 * (S - 1) * S * float(sigma)))


def weighted_sums(util, group_size, n, k, block, seed, generation, acc=np.int64, rows=1 << 12):
    """g [n] of array k (1 .. 4) of block `block`: the sum over the block's pairs of d_q * s_{q,i}, accumulated in ``acc``
    (int64: the header's; int32: the WRONG accumulator that overflows; float32: the WRONG running float sum)"""
    S = int(group_size)
    u = np.asarray(util, np.int32)[block * S:(block + 1) * S]
    d = (u[0::2] - u[1::2]).astype(np.int64)               # int32 arithmetic, modulo 2^32, as the header says
    anchors = block * S + 2 * np.arange(S // 2, dtype=np.int64)
    g = np.zeros(n, acc)
    for q0 in range(0, S // 2, rows):
        live = np.flatnonzero(d[q0:q0 + rows]) + q0
        if not len(live):
            continue
        s = draw_sums(n, anchors[live], k, seed, generation)
        prod = d[live, None] * s
        if acc is np.float32:
            for row in prod:                               # a running sum, one rounding per pair
                g = g + row.astype(f32)
        else:
            with np.errstate(over="ignore"):
                g = g + prod.astype(acc).sum(axis=0, dtype=acc)
    return g


def update_model(mean, util, group_size, step, seed, generation, acc=np.int64):
    """the four new mean arrays: m + (step * ((float)(double)g * C))"""
    mean = [np.asarray(a, f32) for a in mean]
    M = mean[0].shape[0]
    out = []
    for k, a in enumerate(mean):
        flat = a.reshape(M, -1)
        new = np.empty_like(flat)
        for b in range(M):
            g = weighted_sums(util, group_size, flat.shape[1], k + 1, b, seed, generation, acc)
            gf = g.astype(np.float64).astype(f32)
            with np.errstate(all="ignore"):
                new[b] = flat[b] + (f32(step) * (gf * NOISE_SCALE))
        assert new.dtype == f32
        out.append(new.reshape(a.shape))
    return out


def bits(a):
    """float32 array -> uint32 words, every NaN mapped to one pattern"""
    a = np.array(a, f32)
    a[np.isnan(a)] = f32("nan")
    return a.view(u32)
