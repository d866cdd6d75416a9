"""The recurrent device policy stated on the host (include/rem2d_recurrent.h), shared by tests/test_recurrent_host.py (numpy and the
oracle alone) and tests/test_recurrent_gpu.py: what policy_model.py is for the feed-forward policy, and built on it.

* ``forward_model``: one control step.  The input row is ``[x | c]`` with ``c = memory``, or +0 where ``reset`` is set (a
  substitution: NaNs in memory do not get through); the targets and validity bytes are policy_model.forward_model's on that row --
  the header's law, taken literally -- and the new memory is the first K columns of policy_model.hidden_model on the same row.
  Rows the kernel skips keep their memory.
* ``oscillator``: the hand-made weight set of the "memory matters" tests: two context units that rotate by a quarter turn per step.
* ``recurrent_loop_run``: policy_model.policy_loop_run with memory, on control_model.OracleLoop, cached.
"""
import numpy as np

import control_model as M
import policy_model as PM
import range_model as R
import state_forge as F

f32 = np.float32
LOOP_CONTEXT = 8
bits = PM.bits


def forward_model(x, memory, w1, b1, w2, b2, act=PM.SOFTSIGN, scale=PM.DEFAULT_SCALE, index=None, reset=None, row_mask=None):
    """x float32 [N, D - K] (observation words, then ray fractions); memory float32 [N, K]; the weights as policy_model.forward_model
    takes them, w1 [G, D, H]; reset / row_mask uint8 [N] or None
    -> (targets float64 [N, MB], valid uint8 [N, MB], new memory float32 [N, K]).  For a row the kernel skips (policy_model.rows_run)
    the targets and valid bytes mean nothing, as in policy_model; its new memory is its old memory, bit for bit."""
    x, memory, w1, b1 = np.asarray(x, f32), np.asarray(memory, f32), np.asarray(w1, f32), np.asarray(b1, f32)
    N, K, G = x.shape[0], memory.shape[1], w1.shape[0]
    assert memory.shape[0] == N and x.shape[1] + K == w1.shape[1] and 1 <= K <= w1.shape[2]
    c = memory.copy()
    if reset is not None:
        c[np.asarray(reset) != 0] = f32(0.0)
    full = np.concatenate([x, c], axis=1).astype(f32)
    targets, valid = PM.forward_model(full, w1, b1, w2, b2, act=act, scale=scale, index=index)
    g = np.arange(N) if index is None else np.asarray(index, np.int64)
    g = np.where((g >= 0) & (g < G), g, 0)
    with np.errstate(all="ignore"):
        h = PM.hidden_model(full, w1[g], b1[g], act)
    assert h.dtype == f32
    run = PM.rows_run(N, G, index, row_mask)
    new = np.where(run[:, None], h[:, :K], memory).astype(f32)
    new.view(np.uint32)[~run] = memory.view(np.uint32)[~run]      # (np.where may quieten a signalling NaN: keep the very bits)
    return targets, valid, new


def mem_bits(memory):
    """float32 memory -> uint32 words with every NaN mapped to one pattern (policy_model.bits says why)"""
    m = np.array(memory, f32)
    m[np.isnan(m)] = f32("nan")
    return m.view(np.uint32)


def oscillator():
    """(x [1, 14], weights) of a controller that can only move by its memory: MB = 1, R = 0, H = K = 2.  The context rows of w1 are
    [[0, 4], [-4, 0]], everything else in w1 zero, b1 = (0.25, 0), w2 = [[1], [0]], b2 = 0: a_0 = 0.25 - 4 c_1, a_1 = 4 c_0, a
    rotation by a quarter turn with gain 4 under softsign -- the sign of h_0, and with it the target's, has period 4."""
    D = M.width(1) + 2
    w1 = np.zeros((1, D, 2), f32)
    w1[0, D - 2:] = [[0.0, 4.0], [-4.0, 0.0]]
    b1 = np.array([[0.25, 0.0]], f32)
    w2 = np.array([[[1.0], [0.0]]], f32)
    b2 = np.zeros((1, 1), f32)
    x = np.linspace(-1.0, 1.0, M.width(1)).astype(f32)[None]          # a constant input row: w1 ignores it
    return x, (w1, b1, w2, b2)


def oscillator_run(n_steps):
    """-> (targets float64 [n_steps], memories float32 [n_steps + 1, 2]) of the oscillator from zero memory"""
    x, W = oscillator()
    mem = np.zeros((1, 2), f32)
    targets, mems = [], [mem[0].copy()]
    for _ in range(n_steps):
        t, v, mem = forward_model(x, mem, *W)
        assert v.all()
        targets.append(t[0, 0])
        mems.append(mem[0].copy())
    return np.array(targets), np.stack(mems)


# ------------------------------------------------------------------------------------------------------------- the closed loop
def loop_weights(N, K, context=LOOP_CONTEXT):
    """policy_model.loop_weights with `context` more input rows (the same draw as a feed-forward set of 10 + context rays)"""
    return PM.loop_weights(N, K, n_rays=10 + context)


_RUNS = {}


def recurrent_loop_run(O, pop, flags, n_steps=PM.N_POLICY_LOOP, act=PM.SOFTSIGN, context=LOOP_CONTEXT, morphs=None, terrain=None,
                       weights=None, key=None):
    """policy_model.policy_loop_run under the recurrent model, from zero memory: per lane bucket of loop population `pop` (or of
    `morphs` on `terrain` with `weights`, one 4-tuple per bucket, cached under `key`) -> list of dict(ctx, weights, obs / frac
    [n_steps + 1], memory [n_steps + 1] (memory[t]: what step t reads), targets / valid [n_steps], caps, final, root_x, fitness)"""
    key = (pop, flags, n_steps, act, context) if key is None else key
    if key in _RUNS:
        return _RUNS[key]
    if morphs is None:
        terrain, morphs = M.loop_population(pop)
    T = R.Terrain.of(terrain)
    rays = R.bipedal_rays()
    runs = []
    for k, morph in enumerate(morphs):
        loop = M.OracleLoop(O, terrain, morph, flags, pop)
        ctx = loop.ctx
        W = loop_weights(ctx.N, ctx.K, context) if weights is None else tuple(np.asarray(a, f32) for a in weights[k])
        assert W[0].shape == (ctx.N, M.width(PM.LOOP_BODIES) + 10 + context, W[1].shape[1])
        run = dict(ctx=ctx, weights=W, max_bodies=PM.LOOP_BODIES, context=context, obs=[], frac=[], memory=[np.zeros((ctx.N, context), f32)],
                   targets=[], valid=[], caps=[])
        for t in range(n_steps + 1):
            snap = loop.snapshot()
            if t:
                for f in F.LANE_FIELDS + F.SLOT_FIELDS:
                    assert np.isfinite(snap[f]).all(), "oracle state not finite: %s %s step %d" % (pop, f, t)
            run["obs"].append(M.observe_model(ctx, snap, PM.LOOP_BODIES))
            run["frac"].append(R.cast(T, snap["px"][:, 0], snap["py"][:, 0], rays)[0])
            run["caps"].append(np.stack([snap["ccount"].max(axis=1),
                                         ((snap["ctouch"] != 0) & F.masks(ctx, snap)["cedge"]).sum(axis=0).max(axis=1)], 1))
            if t == n_steps:
                break
            tg, valid, mem = forward_model(PM.input_rows(run["obs"][-1], run["frac"][-1]), run["memory"][-1], *W, act=act)
            loop.set_targets(tg, mask=valid)
            run["targets"].append(tg)
            run["valid"].append(valid)
            run["memory"].append(mem)
            loop.step()
        run["final"] = snap
        run["root_x"] = loop.root_x()
        run["fitness"] = loop.env["fitness"].copy()
        runs.append(run)
    _RUNS[key] = runs
    return runs
