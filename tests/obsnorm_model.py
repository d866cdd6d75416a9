"""A numpy model of include/rem2d_obsnorm.h: the exact sums (section 1), the tables (section 3) and the application (section 4),
operation by operation -- integers in Python / int64, binary32 and binary64 operations one at a time, each rounded by numpy as the
header says the library rounds it.  The forward passes themselves are policy_model's and recurrent_model's, fed x^."""
import numpy as np

import policy_model as PM
import recurrent_model as RM

f32, f64 = np.float32, np.float64
CLAMP = f32(2048.0)
SCALE = f32(4096.0)
LOW = (1 << 23) - 1
CAPACITY = 1 << 39


def width(MB, R):
    return 8 + 6 * MB + R


def quantise(x):
    """q of every word: clamp to +-2048, times 4096 (exact), round to nearest even; int64.  The words must be finite."""
    x = np.asarray(x, f32)
    c = np.where(x < -CLAMP, -CLAMP, np.where(x > CLAMP, CLAMP, x)).astype(f32)
    with np.errstate(under="ignore"):
        return np.rint((c * SCALE).astype(f32)).astype(np.int64)


class State:
    """count [M], s1 / s2hi / s2lo [M][Dn], int64 (an object array of Python ints where ``exact``: no word can wrap)"""

    def __init__(self, M, Dn, exact=False):
        dt = object if exact else np.int64
        self.M, self.Dn = M, Dn
        self.count = np.zeros(M, dt)
        self.s1, self.s2hi, self.s2lo = (np.zeros((M, Dn), dt) for _ in range(3))
        if exact:
            for a in (self.count, self.s1, self.s2hi, self.s2lo):
                a[...] = 0

    def words(self):
        return [np.asarray(a, np.int64) for a in (self.count, self.s1, self.s2hi, self.s2lo)]

    def copy(self):
        s = State(self.M, self.Dn)
        s.count, s.s1, s.s2hi, s.s2lo = (np.array(a) for a in (self.count, self.s1, self.s2hi, self.s2lo))
        return s


def contributes(rows, mask=None):
    """the rows that contribute: mask byte set (or no mask) and all words finite"""
    ok = np.isfinite(np.asarray(rows, f32)).all(axis=1)
    return ok if mask is None else ok & (np.asarray(mask) != 0)


def accumulate(state, rows, group_size, mask=None):
    """``rows`` [N][Dn] added to ``state`` in place, row r to block r // group_size"""
    rows = np.asarray(rows, f32)
    on = contributes(rows, mask)
    for r in np.nonzero(on)[0]:
        b = int(r) // int(group_size)
        q = quantise(rows[r])
        p = q * q
        state.count[b] += 1
        state.s1[b] += q
        state.s2hi[b] += p >> 23
        state.s2lo[b] += p & LOW
    return state


def moments(n, s1, s2hi, s2lo):
    """(m, v) in binary64 of one block's words, v as the difference leaves it: BEFORE the clamp at 0"""
    nd = f64(n)
    m = np.asarray(s1, np.int64).astype(f64) / nd
    hi = np.asarray(s2hi, np.int64).astype(f64) * f64(8388608.0)
    s2 = (hi + np.asarray(s2lo, np.int64).astype(f64)) / nd
    mm = m * m
    return m, s2 - mm


def freeze(count, s1, s2hi, s2lo, min_count, min_var):
    """(mu, inv) float32 [M][Dn] of a state, the header's formula one operation at a time"""
    count, s1, s2hi, s2lo = (np.asarray(a, np.int64) for a in (count, s1, s2hi, s2lo))
    M, Dn = s1.shape
    mu, inv = np.zeros((M, Dn), f32), np.ones((M, Dn), f32)
    min_var = f32(min_var)
    with np.errstate(all="ignore"):
        for b in range(M):
            n = int(count[b])
            if n < int(min_count):
                continue
            m, v = moments(n, s1[b], s2hi[b], s2lo[b])
            v = np.where(v > 0, v, f64(0.0))
            mu[b] = (m / f64(4096.0)).astype(f32)
            vx = (v / f64(16777216.0)).astype(f32)
            root = np.sqrt(vx).astype(f32)
            inv[b] = np.where(vx >= min_var, (f32(1.0) / root).astype(f32), f32(0.0))
    return mu, inv


def apply(x, mu, inv, clip, group_size):
    """x^ [N][Dn] of rows x [N][Dn] under tables [M][Dn]"""
    x = np.asarray(x, f32)
    blk = np.arange(x.shape[0]) // int(group_size)
    clip = f32(clip)
    with np.errstate(all="ignore"):
        d = (x - mu[blk]).astype(f32)
        t = (d * inv[blk]).astype(f32)
        return np.where(t > clip, clip, np.where(t < -clip, -clip, t)).astype(f32)


def forward(x, mu, inv, clip, group_size, w1, b1, w2, b2, **kw):
    """the law for a feed-forward policy: policy_model.forward_model fed x^"""
    return PM.forward_model(apply(x, mu, inv, clip, group_size), w1, b1, w2, b2, **kw)


def forward_memory(x, memory, mu, inv, clip, group_size, w1, b1, w2, b2, **kw):
    """the law for a policy with memory: recurrent_model.forward_model fed x^; x is [N][Dn], the context words are memory's"""
    return RM.forward_model(apply(x, mu, inv, clip, group_size), memory, w1, b1, w2, b2, **kw)


def tbits(a):
    return np.ascontiguousarray(np.asarray(a, f32)).view(np.uint32)
