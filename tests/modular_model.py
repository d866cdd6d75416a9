"""The modular device policy stated on the host (include/rem2d_modular.h), shared by tests/test_modular_host.py (numpy alone) and
tests/test_modular_gpu.py: what recurrent_model.py is for the recurrent policy, and built on policy_model.py.

* ``tree``: live(b) and par(b) of a topology table holding ANY int32 values, as the header defines them.
* ``gather``: what a body reads from its neighbours in one round: the number of its children, the sum of their messages -- one
  rounded binary32 add per child, in ascending child order, from +0 -- and its parent's message.
* ``body_rows``: the Dm input words of every (row, body) pair.
* ``forward_model``: P rounds and the read-out; rows the kernel skips keep what their outputs held.
* ``topology_model``: the table rem2d_worlds_topology writes for creatures given as parent lists in body order.
* ``forge``: random rows, trees and messages with the awkward values in them.
"""
import numpy as np

import policy_model as PM

f32 = np.float32
HEAD, BODY = 8, 6
MAX_INPUTS, MAX_ROUNDS = 64, 8


def width(n_rays, messages):
    """Dm: the words a body's controller reads"""
    return HEAD + BODY + int(n_rays) + 2 + 2 * int(messages)


def tree(topo):
    """topo int32 [N, MB, 2] -> (live bool [N, MB], par int64 [N, MB], -1 = none)"""
    topo = np.asarray(topo, np.int32)
    N, MB = topo.shape[:2]
    live = topo[:, :, 1] != 0
    p = topo[:, :, 0].astype(np.int64)
    ok = (p >= 0) & (p < MB) & (p != np.arange(MB)[None, :]) & live
    rows = np.arange(N)[:, None].repeat(MB, 1)
    ok &= live[rows, np.clip(p, 0, MB - 1)]
    return live, np.where(ok, p, -1)


def gather(m, live, par):
    """m float32 [N, MB, K] -> (nch int64 [N, MB], cm float32 [N, MB, K], pm float32 [N, MB, K])"""
    N, MB, K = m.shape
    nch = np.zeros((N, MB), np.int64)
    cm = np.zeros((N, MB, K), f32)
    with np.errstate(all="ignore"):
        for c in range(MB):                                     # ascending c: a row has one parent of c, so no index repeats
            rows = np.nonzero(par[:, c] >= 0)[0]
            b = par[rows, c]
            cm[rows, b] = cm[rows, b] + m[rows, c]
            nch[rows, b] += 1
    rows = np.arange(N)[:, None].repeat(MB, 1)
    pm = np.where((par >= 0)[:, :, None], m[rows, np.clip(par, 0, MB - 1)], f32(0.0)).astype(f32)
    return nch, cm, pm


def body_rows(obs, frac, topo, nch, cm, pm):
    """x float32 [N, MB, Dm]: head, body b, rays, shape, children, cm, pm"""
    obs = np.asarray(obs, f32)
    N, MB = topo.shape[:2]
    R = 0 if frac is None else frac.shape[1]
    parts = [np.broadcast_to(obs[:, None, :HEAD], (N, MB, HEAD)), obs[:, HEAD:].reshape(N, MB, BODY)]
    if R:
        parts.append(np.broadcast_to(np.asarray(frac, f32)[:, None, :], (N, MB, R)))
    parts += [topo[:, :, 1].astype(f32)[:, :, None], nch.astype(f32)[:, :, None], cm, pm]
    return np.concatenate(parts, axis=2).astype(f32)


def forward_model(obs, frac, topo, memory, w1, b1, w2, b2, rounds=1, act=PM.SOFTSIGN, scale=PM.DEFAULT_SCALE, index=None, reset=None,
                  row_mask=None, out=None):
    """obs float32 [N, 8 + 6 MB]; frac float32 [N, R] or None; topo int32 [N, MB, 2]; memory float32 [N, MB, K]; w1 [G, Dm, H],
    b1 [G, H], w2 [G, H, 1], b2 [G, 1]; index / reset / row_mask as the kernel takes them; out: the (targets, valid) a skipped row
    keeps (default zeros) -> (targets float64 [N, MB], valid uint8 [N, MB], new memory float32 [N, MB, K])."""
    topo, memory = np.asarray(topo, np.int32), np.asarray(memory, f32)
    w1, b1, w2, b2 = (np.asarray(v, f32) for v in (w1, b1, w2, b2))
    N, MB, K = memory.shape
    G, Dm, H = w1.shape
    R = 0 if frac is None else frac.shape[1]
    assert Dm == width(R, K) and 1 <= K <= H and R + 2 + 2 * K <= MAX_INPUTS and 1 <= rounds <= MAX_ROUNDS and w2.shape == (G, H, 1)
    live, par = tree(topo)
    run = PM.rows_run(N, G, index, row_mask)
    g = np.arange(N) if index is None else np.asarray(index, np.int64)
    g = np.where((g >= 0) & (g < G), g, 0)
    m = memory.copy()
    if reset is not None:
        m[np.asarray(reset) != 0] = f32(0.0)
    m[~live] = f32(0.0)
    rr, bb = np.nonzero(live & run[:, None])                    # the (row, body) pairs that are evaluated
    h = np.zeros((len(rr), H), f32)
    with np.errstate(all="ignore"):
        for _ in range(rounds):
            x = body_rows(obs, frac, topo, *gather(m, live, par))[rr, bb]
            h = PM.hidden_model(x, w1[g[rr]], b1[g[rr]], act)
            assert h.dtype == f32
            m = m.copy()
            m[rr, bb] = h[:, :K]
        w2g = w2[g[rr]]
        y = b2[g[rr]].copy()
        for j in range(H):
            y = y + (h[:, j, None] * w2g[:, j, :])
        t = f32(scale) * PM.softsign(y)
    assert t.dtype == f32
    targets = np.zeros((N, MB), np.float64) if out is None else np.array(out[0], np.float64)
    valid = np.zeros((N, MB), np.uint8) if out is None else np.array(out[1], np.uint8)
    targets[run], valid[run] = 0.0, 0
    targets[rr, bb] = t[:, 0].astype(np.float64)
    valid[rr, bb] = np.isfinite(t[:, 0]).astype(np.uint8)
    new = m
    new.view(np.uint32)[~run] = memory.view(np.uint32)[~run]    # (a skipped row keeps the very bits)
    return targets, valid, new


def mem_bits(memory):
    """float32 -> uint32 words with every NaN mapped to one pattern (policy_model.bits says why)"""
    m = np.array(memory, f32)
    m[np.isnan(m)] = f32("nan")
    return m.view(np.uint32)


def topology_model(parents, shapes, max_bodies):
    """parents: per creature the list of each body's parent BODY index (-1: root), in body order; shapes: the bodies' shape words
    -> int32 [N, max_bodies, 2]"""
    out = np.zeros((len(parents), max_bodies, 2), np.int32)
    out[:, :, 0] = -1
    for r, (ps, ss) in enumerate(zip(parents, shapes)):
        for b, (p, s) in enumerate(zip(ps, ss)):
            if b < max_bodies:
                out[r, b] = (p if 0 <= p < max_bodies else -1, s)
    return out


# ---------------------------------------------------------------------------------------------------------------- forged inputs
def chain(n):
    return [-1] + list(range(n - 1))


def star(n):
    return [-1] + [0] * (n - 1)


def random_tree(rng, n):
    return [-1] + [int(rng.integers(0, b)) for b in range(1, n)]


def forge_topo(rng, N, MB):
    """int32 [N, MB, 2]: chains, stars and random trees of every size up to MB, holes of non-live slots in the middle, and parents
    that are out of range, the body itself, a non-live slot or half of a 2-cycle"""
    topo = np.zeros((N, MB, 2), np.int32)
    topo[:, :, 0] = -1
    for r in range(N):
        n = MB if r < 3 else int(rng.integers(1, MB + 1))
        ps = (chain, star, lambda k: random_tree(rng, k))[r % 3](n)
        topo[r, :n, 0] = ps
        topo[r, :n, 1] = rng.integers(1, 3, n)
        kind = r % 7
        if r >= 3 and MB >= 3:
            b = int(rng.integers(1, MB))
            if kind == 1:
                topo[r, b, 1] = 0                               # a hole: its children lose their parent
            elif kind == 2:
                topo[r, b, 0] = int(rng.choice([MB, MB + 5, -7, 2 ** 31 - 1, -2 ** 31]))
            elif kind == 3:
                topo[r, b, 0] = b
            elif kind == 4:
                a = int(rng.integers(0, MB))
                topo[r, a, 0], topo[r, b, 0] = b, a             # a 2-cycle (a == b: the body itself)
                topo[r, [a, b], 1] = 1
            elif kind == 5:
                topo[r, :, 1] = 0                               # nobody is live
            elif kind == 6:
                topo[r, b, 1] = -3 if rng.integers(2) else 2 ** 30      # any non-zero word is live
    return topo


SPECIALS = np.array([np.nan, np.inf, -np.inf, 1e-40, -1e-42, -0.0, 3e38, -3e38], f32)


def forge(seed, N, MB, H, K, R, G=None, specials=True):
    """-> dict(obs, frac, topo, memory, weights): forged inputs of N rows, G weight sets (default N)"""
    rng = np.random.default_rng([seed, N, MB, H, K, R])
    G = N if G is None else G
    Dm = width(R, K)
    obs = rng.standard_normal((N, HEAD + BODY * MB)).astype(f32)
    frac = rng.random((N, R)).astype(f32) if R else None
    memory = (rng.standard_normal((N, MB, K)) * 0.5).astype(f32)
    W = [(rng.standard_normal(s) * sd).astype(f32) for s, sd in (((G, Dm, H), 0.3), ((G, H), 0.3), ((G, H, 1), 0.5), ((G, 1), 0.3))]
    if specials and N:
        for a in [memory] + W + [obs]:
            flat = a.reshape(-1)
            at = rng.integers(0, flat.size, max(1, flat.size // 97))
            flat[at] = rng.choice(SPECIALS, at.size)
    return dict(obs=obs, frac=frac, topo=forge_topo(rng, N, MB), memory=memory, weights=tuple(W))
