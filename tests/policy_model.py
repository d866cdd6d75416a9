"""The device policy stated on the host (include/rem2d_policy.h), shared by tests/test_policy_host.py (numpy and the oracle alone)
and tests/test_policy_gpu.py: what control_model.py is for observe / control and range_model.py for the rays.

* ``forward_model``: the forward pass in numpy binary32.  The loops over the input index i and the hidden index j are Python loops
  in ascending order; each step is `acc = acc + (x_i * w)` on float32 arrays, which numpy evaluates as one rounded product and one
  rounded sum (it has no fused multiply-add for this expression), vectorised over rows and output units only.  `a / (1 + |a|)` is
  one rounded sum and one correctly rounded division.
* ``loop_weights`` / ``policy_loop_run``: the closed loop on the oracle alone -- observe_model and range_model.cast make the input
  rows, forward_model the targets, OracleLoop.set_targets(mask=valid) writes them -- cached for both test files.

NaNs: IEEE 754 leaves the sign and payload of a NaN result open and the host's and the device's arithmetic choose differently, so
``bits`` maps every NaN target to one pattern before a comparison; everything else, infinities and zeros' signs included, is compared
bit for bit.
"""
import numpy as np

import control_model as M
import range_model as R
import state_forge as F

f32 = np.float32
SOFTSIGN, RELU = "softsign", "relu"
DEFAULT_SCALE = f32(np.pi / 2)
N_POLICY_LOOP = 120
LOOP_BODIES, LOOP_HIDDEN = 16, 32


def softsign(a):
    return a / (f32(1.0) + np.abs(a))


def hidden_model(x, w1, b1, act):
    """h float32 [N, H] of rows x [N, D] under per-row weights w1 [N, D, H], b1 [N, H]"""
    a = b1.copy()
    for i in range(x.shape[1]):
        a = a + (x[:, i, None] * w1[:, i, :])
    if act == RELU:
        return np.where(a > 0, a, f32(0.0)).astype(f32)      # NaN > 0 and -0 > 0 are false: +0
    return softsign(a)


def forward_model(x, w1, b1, w2, b2, act=SOFTSIGN, scale=DEFAULT_SCALE, index=None):
    """x float32 [N, D]; w1 [G, D, H], b1 [G, H], w2 [G, H, MB], b2 [G, MB]; index int [N] or None (row r uses set r)
    -> (targets float64 [N, MB], valid uint8 [N, MB]).  A row whose index lies outside [0, G) is one the kernel skips: what is
    returned for it (computed with set 0) means nothing, see ``rows_run``."""
    x, w1, b1, w2, b2 = (np.asarray(v, f32) for v in (x, w1, b1, w2, b2))
    N, G = x.shape[0], w1.shape[0]
    g = np.arange(N) if index is None else np.asarray(index, np.int64)
    g = np.where((g >= 0) & (g < G), g, 0)
    with np.errstate(all="ignore"):
        h = hidden_model(x, w1[g], b1[g], act)
        w2g = w2[g]
        y = b2[g].copy()
        for j in range(h.shape[1]):
            y = y + (h[:, j, None] * w2g[:, j, :])
        t = f32(scale) * softsign(y)
    assert t.dtype == f32 and h.dtype == f32
    return t.astype(np.float64), np.isfinite(t).astype(np.uint8)


def rows_run(n, n_sets, index=None, row_mask=None):
    """bool [n]: the rows the kernel computes (the others keep what their outputs held)"""
    run = np.ones(n, bool) if index is None else (np.asarray(index) >= 0) & (np.asarray(index) < n_sets)
    return run if row_mask is None else run & (np.asarray(row_mask) != 0)


def bits(targets):
    """float64 targets -> uint64 words with every NaN mapped to one pattern"""
    t = np.array(targets, np.float64)
    t[np.isnan(t)] = np.float64("nan")
    return t.view(np.uint64)


def input_rows(obs, frac):
    return np.concatenate([obs, frac], axis=1).astype(f32) if frac is not None and frac.shape[1] else np.asarray(obs, f32)


# ------------------------------------------------------------------------------------------------------------- the closed loop
def loop_weights(N, K, max_bodies=LOOP_BODIES, hidden=LOOP_HIDDEN, n_rays=10):
    """The per-creature weight sets of a lane bucket of N creatures with K lanes: w1 0.3, b1 0.3, w2 0.5, b2 0.3 times standard
    normals drawn in that order from default_rng([N, K, 9])"""
    rng = np.random.default_rng([N, K, 9])
    D = M.width(max_bodies) + n_rays
    return ((rng.standard_normal((N, D, hidden)) * 0.3).astype(f32), (rng.standard_normal((N, hidden)) * 0.3).astype(f32),
            (rng.standard_normal((N, hidden, max_bodies)) * 0.5).astype(f32), (rng.standard_normal((N, max_bodies)) * 0.3).astype(f32))


_RUNS = {}


def policy_loop_run(O, pop, flags, n_steps=N_POLICY_LOOP, act=SOFTSIGN, morphs=None, terrain=None, key=None):
    """The oracle under the device policy's model, per lane bucket of loop population `pop` (or of `morphs` on `terrain`, cached
    under `key`) -> list of dict(ctx, weights, obs / frac [n_steps + 1], targets / valid [n_steps], caps [n_steps + 1], final,
    root_x, fitness)"""
    key = (pop, flags, n_steps, act) if key is None else key
    if key in _RUNS:
        return _RUNS[key]
    if morphs is None:
        terrain, morphs = M.loop_population(pop)
    T = R.Terrain.of(terrain)
    rays = R.bipedal_rays()
    runs = []
    for morph in morphs:
        loop = M.OracleLoop(O, terrain, morph, flags, pop)
        ctx = loop.ctx
        W = loop_weights(ctx.N, ctx.K)
        run = dict(ctx=ctx, weights=W, max_bodies=LOOP_BODIES, obs=[], frac=[], targets=[], valid=[], caps=[])
        for t in range(n_steps + 1):
            snap = loop.snapshot()
            if t:
                for f in F.LANE_FIELDS + F.SLOT_FIELDS:
                    assert np.isfinite(snap[f]).all(), "oracle state not finite: %s %s step %d" % (pop, f, t)
            run["obs"].append(M.observe_model(ctx, snap, LOOP_BODIES))
            run["frac"].append(R.cast(T, snap["px"][:, 0], snap["py"][:, 0], rays)[0])
            run["caps"].append(np.stack([snap["ccount"].max(axis=1),
                                         ((snap["ctouch"] != 0) & F.masks(ctx, snap)["cedge"]).sum(axis=0).max(axis=1)], 1))
            if t == n_steps:
                break
            tg, valid = forward_model(input_rows(run["obs"][-1], run["frac"][-1]), *W, act=act)
            loop.set_targets(tg, mask=valid)
            run["targets"].append(tg)
            run["valid"].append(valid)
            loop.step()
        run["final"] = snap
        run["root_x"] = loop.root_x()
        run["fitness"] = loop.env["fitness"].copy()
        runs.append(run)
    _RUNS[key] = runs
    return runs
