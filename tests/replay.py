"""The oracle-replay runner of the bit-exact parity suites: drive a world through a sequence of calls and compare its whole arena
with the oracle's snapshot (state_forge.snapshot) after every call, with `==`: the 8 body columns, joint impulses, motor speed and
limit state, every body's pair list in list order (edge or static index, point count, manifold type, feature keys, normal and tangent
impulses), position-iteration count, TOI events, reward, done, everdone, fitness, wall of death.

A world is a ``BatchedWorld`` (pytest -m gpu) or the oracle-backed twin of the ABI, ``oracle.cpu_twin.CpuWorld``, on which
tests/test_replay_host.py tests this module without a GPU.  The suites keep their protocol facts (settle steps, marks, left-out
caps, what they count); the loop, the comparison and the verdict on the error bits are here, once.
"""
import ctypes as C
import sys

import numpy as np
import pytest

import state_forge as F

# name -> (tile shape for reset, launch options): every launch form a suite steps through; a suite's own ids map into this table
LAUNCH_FORMS = {"step_train": (None, None), "velpost": (None, {"fuse_velpost": 1}), "two_launches": (None, {"fuse_velpost": 0}),
                "fused_step_kernel": (None, {"pipeline": 0}), "train_128_lanes": (1, None),
                "per_step_128_lanes": (1, {"fuse_velpost": 0})}
# test_tick_split_gpu's and test_step_forge_gpu's spelling of the five forms they share
TICK_FORMS = {"step_train": "step_train", "velpost_per_step": "velpost", "two_launches_per_step": "two_launches",
              "train_128_lanes": "train_128_lanes", "per_step_128_lanes": "per_step_128_lanes"}


def need_gpu(world=False):
    """The body of a module's GPU fixture: skip without a GPU, build() -> torch, or BatchedWorld."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd.world import BatchedWorld
    return BatchedWorld if world else torch


def tally(title, order):
    """The body of a module's `tally` fixture: yields {key: [tests, creature-steps compared, creatures left out]} for `count`."""
    t = {}
    yield t
    out = sys.__stdout__
    out.write("\n%s | tests | creature-steps compared | creatures left out\n" % title)
    for k in order:
        if k in t:
            out.write("  %-24s | %3d | %7d | %d\n" % (k, t[k][0], t[k][1], t[k][2]))
    out.write("  %d rows, %d ids, %d creature-steps\n" % (len(t), sum(v[0] for v in t.values()), sum(v[1] for v in t.values())))
    out.flush()


def count(t, key, test_id, compared, gone=0):
    row = t.setdefault(key, [0, 0, 0])
    row[0], row[1], row[2] = row[0] + 1, row[1] + compared, row[2] + gone
    print("%s: %d creature-steps compared, %d creatures left out" % (test_id, compared, gone))


def _arena(w):
    """-> (the whole arena as host bytes, name -> (offset, count, dtype code)): a BatchedWorld's arena is a device tensor read in ONE
    copy, with rem2d_world_field's offsets; a CpuWorld's is numpy, with CpuWorld.field's."""
    if isinstance(w.arena, np.ndarray):
        return w.arena, w.field
    import torch
    from gym_rem2d_amd import _lib
    torch.cuda.synchronize(w.device)

    def field(name):
        off, cnt, dt = C.c_size_t(), C.c_size_t(), C.c_int32()
        w._check(w.L.rem2d_world_field(w.h, _lib.FIELD_ID[name], C.byref(off), C.byref(cnt), C.byref(dt)))
        return off.value, cnt.value, dt.value
    return w.arena.cpu().numpy(), field


def read_state(w):
    """The whole arena -> {field: numpy array shaped like w.view(field)}."""
    from gym_rem2d_amd import _lib
    host, field = _arena(w)
    Lp, out = w.n_envs_padded * w.lanes, {}
    for name in _lib.FIELDS:
        off, cnt, dt = field(name)
        v = np.frombuffer(host, dtype=(np.float32, np.int32, np.float64)[dt], count=cnt, offset=off)
        if cnt == Lp:
            v = v.reshape(w.n_envs_padded, w.lanes)[:w.n_envs]
        elif cnt == Lp * w.contact_slots:
            v = v.reshape(w.contact_slots, w.n_envs_padded, w.lanes)[:, :w.n_envs]
        else:
            v = v[:w.n_envs]
        out[name] = v
    out["cnpt"], out["ctype"] = out["cinfo"] & 0xff, (out["cinfo"] >> 8) & 0xff
    return out


def mismatches(ctx, got, want, keep, slots, where):
    """Every field the oracle exposes under `==`, for the creatures in `keep` -> list of texts (empty: equal)."""
    bad = []
    msk = F.masks(ctx, want)

    def check(f, g, o, m):
        if g.dtype.kind == "i":
            g, o = g.astype(np.int64) & 0xffffffff, o.astype(np.int64) & 0xffffffff
        ne = m & (g != o)
        if ne.any():
            i = tuple(int(x[0]) for x in np.nonzero(ne))
            bad.append("%s %s: %d differ, first at %s: gpu %r oracle %r" % (where, f, int(ne.sum()), i, g[i], o[i]))

    for f in F.LANE_FIELDS:
        check(f, got[f], want[f], msk[f] & keep[:, None])
    # (a kept creature has at most `slots` pairs on a body; the oracle's rows beyond the build's slots are empty for it)
    assert int(want["ccount"][keep].max(initial=0)) <= slots
    for f in F.SLOT_FIELDS:
        check(f, got[f][:slots], want[f][:slots], msk[f][:slots] & keep[None, :, None])
    for f in F.ENV_FIELDS:
        check(f, got[f], want[f], keep)
    return bad


def verdict(ctx, got, want, keep, bits, slots, where):
    """One compared state -> list of texts: `mismatches` for the creatures in `keep`; no error bit on them, REM2D_ERR_HANDOVER on
    nobody, and on everyone else the capacity bits `bits` by which the oracle's own state justifies leaving them out."""
    bad = mismatches(ctx, got, want, keep, slots, where)
    err, gone = got["err"], ~keep
    if (err[keep] != 0).any():
        bad.append("%s: error bits %s on creatures the oracle does not justify" % (where, err[keep][err[keep] != 0]))
    if (err & F.ERR_HANDOVER).any():
        bad.append("%s: REM2D_ERR_HANDOVER" % where)
    if ((err[gone] & bits[gone]) != bits[gone]).any():
        bad.append("%s: left-out creatures without their capacity bit: err %s, oracle %s" % (where, err[gone], bits[gone]))
    return bad


def inject(w, ctx, snap, inj):
    """Write the injection through the arena views: only the entries under the field's mask, like state_forge.apply_to_oracle."""
    import torch
    msk = F.masks(ctx, snap)
    for f, v in inj.items():
        view = w.view(f)
        m = msk[f]
        if v.ndim == 3:
            m, v = m[:view.shape[0]], v[:view.shape[0]]
        m_d = torch.from_numpy(np.ascontiguousarray(m)).to(w.device)
        v_d = torch.from_numpy(np.ascontiguousarray(v)).to(w.device)
        assert v_d.dtype == view.dtype and v_d.shape == view.shape, f
        view.copy_(torch.where(m_d, v_d, view))


def make_world(World, morph, terrain, flags, form, wide):
    """A `World` of the LAUNCH_FORMS form `form` on `terrain`, reset on `morph`."""
    shape, options = LAUNCH_FORMS[form]
    w = World(morph.n_envs, morph.lanes, flags, wide=wide, options=options)
    try:
        w.set_terrain(terrain)
        w.reset(morph, tile_shape=shape)
    except BaseException:
        w.close()
        raise
    return w


def invdt0(st, call, where):
    """replay's `check` for step_ex calls: the arena holds 1.0f / dt of the call."""
    ok = (st["invdt0"] == np.float32(1.0) / np.float32(call[1])).all()
    return [] if ok else ["%s: invdt0 %s" % (where, np.unique(st["invdt0"]))]


def replay(make, ctx, start, calls, expected, pair_slots, settle=0, injections=(), first=None, bits=None, marks=(), check=None):
    """Drive a world from `make()` through `calls` -- n for step(n), (n, dt, vel, pos) for step_ex -- and hold it to expected[c] after
    call c; raises AssertionError with every difference of the first call that has one.  -> (creature-steps compared, creatures left out)

    start: the snapshot after `settle` steps (0: the reset state), equal on every world with nobody left out and no error bit.
    injections {c: injection}: written before call c under the masks of the state then held.  first / bits: creature e is compared
    in the calls before first[e] and must carry bits[e] from then on (state_forge.left_out; default: nobody is left out).  marks:
    call counts at which a second world given the same injections, stepped in ONE launch from mark to mark, is compared as well.
    check(state, call, where) -> texts: a suite's own per-call check."""
    everyone = np.ones(ctx.N, bool)
    first = np.full(ctx.N, len(calls), np.int32) if first is None else first
    bits = np.zeros(ctx.N, np.int32) if bits is None else bits
    assert not len(marks) or all(c == 0 or c in marks for c in injections)     # (the second world is injected between its launches)
    worlds = []
    try:
        for name in ("single", "multi")[:2 if len(marks) else 1]:
            worlds.append((name, make()))
            w = worlds[-1][1]
            assert w.contact_slots == pair_slots
            if settle:
                w.step(settle)
            st = read_state(w)
            # oracle body i is arena lane slots[i]: equal poses (and everything else) before the first call
            bad = mismatches(ctx, st, start, everyone, pair_slots, "%s start" % name)
            assert not bad and int(st["err"].max()) == 0, bad
        compared, snap, mark = 0, start, 0
        for c, call in enumerate(calls):
            for _, w in worlds:
                if c in injections:
                    inject(w, ctx, snap, injections[c])
            if isinstance(call, int):
                n, what = call, "step %d" % (c + 1)
                worlds[0][1].step(n)
            else:
                n, what = call[0], "call %d (%d x dt %.9g, %d / %d)" % ((c,) + tuple(call))
                worlds[0][1].step_ex(*call)
            judged = worlds[:1]
            if c + 1 in marks:
                worlds[1][1].step(sum(calls[mark:c + 1]))
                judged, mark = worlds, c + 1
            keep, snap, bad = first > c, expected[c], []
            for name, w in judged:
                st = read_state(w)
                bad += verdict(ctx, st, snap, keep, bits, pair_slots, "%s %s" % (name, what))
                bad += check(st, call, "%s %s" % (name, what)) if check else []
            assert not bad, "\n".join(bad)
            compared += n * int(keep.sum())
        for name, w in worlds:
            assert w.handover_failures() == 0, "%s world: handover_failures() %d" % (name, w.handover_failures())
        return compared, int((first < len(calls)).sum())
    finally:
        for _, w in worlds:
            w.close()
