"""The adaptive evolution strategy for device policies stated on the host (include/rem2d_snes.h), shared by tests/test_snes_host.py
(numpy alone) and tests/test_snes_gpu.py: what es_model.py is for rem2d_es.  Written from the header, not from the kernels.

* ``sample_model``: the four child arrays [M S, ...] from the four mean arrays and the four sigma arrays [M, ...].
* ``second_sums``: h [n] of one array of one block, in wrapping int64 numpy arithmetic.
* ``update_model``: (new mean, new sigma, new m1, new m2), four arrays each (the moments None without ADAM).
* ``scalars`` and its helpers: the binary32 scalars the Python layer hands to the library.

The keyword arguments that default to False / None state WRONG variants, for the teeth test of test_snes_host.py.
"""
import math

import numpy as np

import es_model as ES
from es_model import bits, draw_sums, noise_of  # noqa: F401  (bits: every NaN mapped to one pattern before a comparison)
from evolve_model import NOISE_SCALE

f32 = np.float32
ADAM, NATURAL = 1, 2
MAX_GROUP = 8192
TWO31 = np.int64(1) << np.int64(31)


def sample_model(mean, sigma, group_size, seed, generation):
    """mean, sigma: (w1 [M, D, H], b1 [M, H], w2 [M, H, MB], b2 [M, MB]) each -> the four child arrays [M S, ...]"""
    mean, sigma = [np.asarray(a, f32) for a in mean], [np.asarray(a, f32) for a in sigma]
    M, S = mean[0].shape[0], int(group_size)
    assert S >= 2 and S % 2 == 0
    c = np.arange(M * S, dtype=np.int64)
    anchor, odd = c & ~np.int64(1), (c & 1) == 1
    kids = []
    for k, (a, sg) in enumerate(zip(mean, sigma)):
        flat, sflat = a.reshape(M, -1), sg.reshape(M, -1)
        z = noise_of(draw_sums(flat.shape[1], anchor, k + 1, seed, generation))
        with np.errstate(all="ignore"):
            t = sflat[c // S] * z
            t = np.where(odd[:, None], -t, t)
            out = flat[c // S] + t
        assert out.dtype == f32 and t.dtype == f32
        kids.append(out.reshape((M * S,) + a.shape[1:]))
    return kids


def pair_terms(util, group_size, block):
    """(d, p) int64 [S / 2] of one block: util[a] -+ util[a + 1] in int32 arithmetic, modulo 2^32"""
    S = int(group_size)
    u = np.asarray(util, np.int32)[block * S:(block + 1) * S]
    with np.errstate(over="ignore"):
        return (u[0::2] - u[1::2]).astype(np.int64), (u[0::2] + u[1::2]).astype(np.int64)


def second_sums(util, group_size, n, k, block, seed, generation, acc=np.int64, skip_on_d=False, square32=False, rows=1 << 12):
    """h [n] of array k (1 .. 4) of block `block`: the sum over the block's pairs of p_q * (s_{q,i}^2 - 2^31), wrapping modulo 2^64.
    acc float32: the WRONG running float sum; skip_on_d: the WRONG skip of every pair whose d is 0; square32: the WRONG s * s in
    32 bits"""
    S = int(group_size)
    d, p = pair_terms(util, S, block)
    anchors = block * S + 2 * np.arange(S // 2, dtype=np.int64)
    h = np.zeros(n, acc)
    for q0 in range(0, S // 2, rows):
        dd, pp = d[q0:q0 + rows], p[q0:q0 + rows]
        live = np.flatnonzero(dd != 0 if skip_on_d else (dd != 0) | (pp != 0)) + q0
        if not len(live):
            continue
        s = draw_sums(n, anchors[live], k, seed, generation)
        with np.errstate(over="ignore"):
            sq = s * s
            if square32:
                sq = sq.astype(np.int32).astype(np.int64)
            prod = p[live, None] * (sq - TWO31)            # int64 arrays: numpy wraps modulo 2^64
            if acc is np.float32:
                for row in prod:                           # a running sum, one rounding per pair
                    h = h + row.astype(f32)
            else:
                h = h + prod.sum(axis=0, dtype=np.int64)
    return h


def sstep_for(lr_sigma, group_size):
    S = int(group_size)
    return f32(float(lr_sigma) / (4.0 * (S - 1) * S))


def mstep_for(lr, group_size, sigma, adam=False):
    S = int(group_size)
    return f32(1.0 / (2.0 * (S - 1) * S)) if adam else f32(float(lr) / (2.0 * (S - 1) * S * float(sigma)))


def alpha_for(lr, beta1, beta2, t):
    return f32(float(lr) * math.sqrt(1.0 - float(beta2) ** int(t)) / (1.0 - float(beta1) ** int(t)))


def scalars(group_size, sigma=0.1, lr=0.05, lr_sigma=4.0, adam=None, t=1, sigma_bounds=(1e-6, 10.0)):
    """the ten binary32 scalars of a descriptor, as policy.SeparableES computes them for its update number t = 1, 2, ..."""
    c = dict(mstep=mstep_for(lr, group_size, sigma, adam is not None), sstep=sstep_for(lr_sigma, group_size), beta1=f32(0), omb1=f32(0),
             beta2=f32(0), omb2=f32(0), alpha=f32(0), eps=f32(0), sigma_min=f32(sigma_bounds[0]), sigma_max=f32(sigma_bounds[1]))
    if adam is not None:
        b1, b2, eps = (float(v) for v in adam)
        c.update(beta1=f32(b1), omb1=f32(1.0 - b1), beta2=f32(b2), omb2=f32(1.0 - b2), eps=f32(eps), alpha=alpha_for(lr, b1, b2, t))
    return c


def apply_sums(m, sg, o1, o2, g, h, c, flags, new_sigma_in_natural=False, fused_adam=False, use_exp=False):
    """the header's conversions, sigma update and mean update on arrays of old words m, sg (and o1, o2 with ADAM) and the int64
    sums g, h -> (m', sg', m1', m2'), the moments None without ADAM.  c: the scalars, a dict of binary32"""
    c = {k: f32(v) for k, v in c.items()}
    m, sg = np.asarray(m, f32), np.asarray(sg, f32)
    one, two = f32(1), f32(2)
    with np.errstate(all="ignore"):
        G = np.asarray(g, np.int64).astype(np.float64).astype(f32) * NOISE_SCALE
        Hh = np.asarray(h, np.int64).astype(np.float64).astype(f32) * f32(2.0 ** -31)
        x = c["sstep"] * Hh
        x = np.where(np.isnan(x), f32(0), np.where(x < -one, -one, np.where(x > one, one, x)))
        f = np.exp(x.astype(np.float64)).astype(f32) if use_exp else (two + x) / (two - x)
        sn = sg * f
        sn = np.where(sn < c["sigma_min"], c["sigma_min"], np.where(sn > c["sigma_max"], c["sigma_max"], sn))
        t = ((sn if new_sigma_in_natural else sg) * G) if flags & NATURAL else G
        gh = c["mstep"] * t
        assert G.dtype == f32 and x.dtype == f32 and f.dtype == f32 and sn.dtype == f32 and gh.dtype == f32
        if not flags & ADAM:
            return m + gh, sn, None, None
        o1, o2 = np.asarray(o1, f32), np.asarray(o2, f32)
        if fused_adam:
            a1 = (np.float64(c["beta1"]) * o1.astype(np.float64) + np.float64(c["omb1"]) * gh.astype(np.float64)).astype(f32)
        else:
            a1 = (c["beta1"] * o1) + (c["omb1"] * gh)
        a2 = (c["beta2"] * o2) + (c["omb2"] * (gh * gh))
        new = m + (c["alpha"] * (a1 / (np.sqrt(a2) + c["eps"])))
        assert a1.dtype == f32 and a2.dtype == f32 and new.dtype == f32
        return new, sn, a1, a2


def update_model(mean, sigma, m1, m2, util, group_size, c, flags, seed, generation, acc=np.int64, skip_on_d=False, square32=False,
                 new_sigma_in_natural=False, fused_adam=False, use_exp=False):
    """-> (new mean, new sigma, new m1, new m2): lists of four arrays, the moments None without ADAM.  c: the scalars (a dict of
    binary32).  The WRONG variants: acc / skip_on_d / square32 (second_sums), the NEW sigma in the natural step, beta m + omb g
    rounded once, exp in place of (2 + x) / (2 - x)"""
    mean, sigma = [np.asarray(a, f32) for a in mean], [np.asarray(a, f32) for a in sigma]
    adam = bool(flags & ADAM)
    if adam:
        m1, m2 = [np.asarray(a, f32) for a in m1], [np.asarray(a, f32) for a in m2]
    M = mean[0].shape[0]
    out = ([], [], [], [])
    for k, a in enumerate(mean):
        flat, sflat = a.reshape(M, -1), sigma[k].reshape(M, -1)
        n = flat.shape[1]
        new, nsig, n1, n2 = (np.empty_like(flat) for _ in range(4))
        for b in range(M):
            g = ES.weighted_sums(util, group_size, n, k + 1, b, seed, generation)
            h = second_sums(util, group_size, n, k + 1, b, seed, generation, acc, skip_on_d, square32)
            o1, o2 = (m1[k].reshape(M, -1)[b], m2[k].reshape(M, -1)[b]) if adam else (None, None)
            res = apply_sums(flat[b], sflat[b], o1, o2, g, h.astype(np.int64) if acc is np.int64 else h.astype(np.float64).astype(np.int64),
                             c, flags, new_sigma_in_natural, fused_adam, use_exp)
            new[b], nsig[b] = res[0], res[1]
            if adam:
                n1[b], n2[b] = res[2], res[3]
        for dst, arr in zip(out, (new, nsig, n1, n2)):
            dst.append(arr.reshape(a.shape))
    return out[0], out[1], (out[2] if adam else None), (out[3] if adam else None)
