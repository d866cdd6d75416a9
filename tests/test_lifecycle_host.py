"""World reuse, host half (no GPU): the populations and the dirt of tests/lifecycle_forge.py are what they claim to be, and the
host-pointer twin (oracle/librem2d_cpu.so) -- whose arena right after a reset is the image the GPU half holds
rem2d_reset_kernel to -- treats a used, scribbled-on world exactly like a fresh one."""
import numpy as np
import pytest

import lifecycle_forge as F
from conftest import oracle_terrain


@pytest.mark.parametrize("lanes", F.LANES)
def test_populations_swap_bodies_and_empty_lanes(lanes):
    """The world shapes of the issue (37 creatures on 48 padded rows; 21 on 24; three 64-lane blocks each) and, in at least a
    quarter of the creatures each, an empty lane of P2 where P1 had a body and a body of P2 where P1 had none."""
    from oracle import cpu_twin
    m1, m2 = F.populations(lanes)
    assert m1.n_envs == m2.n_envs == F.N_ENVS[lanes] == {4: 37, 8: 21}[lanes] and m1.lanes == m2.lanes == lanes
    assert not set(F.SEEDS[lanes][0]) & set(F.SEEDS[lanes][1])
    cfg = cpu_twin.WorldCfg(m1.n_envs, lanes, 0, 0)
    padded = cpu_twin.lib().rem2d_cpu_padded_envs(cfg)
    assert padded == {4: 48, 8: 24}[lanes] and padded * lanes == 3 * 64
    gone, new = F.swap_counts(m1, m2)
    assert 4 * gone >= m1.n_envs and 4 * new >= m1.n_envs, (gone, new)


@pytest.mark.parametrize("lanes", F.LANES)
def test_episode_one_leaves_something_behind(lanes, oracle, rough_terrain):
    """Non-vacuity, from the oracle alone: after episode 1 there are touching manifolds, joint and contact impulses, TOI events,
    creatures that used all 60 position iterations and a wall of death that has moved -- the state a reset has to get rid of."""
    m1, _ = F.populations(lanes)
    w = F.twin_world(lanes, F.FLAG_CONTINUOUS, rough_terrain)
    w.reset(m1)
    w.step(F.EPISODE1)
    left = F.leftovers(F.host_views(w))
    print(lanes, left)
    assert all(v > 0 for v in left.values()), left
    run = oracle.batch_run(oracle_terrain(oracle, rough_terrain), m1.as_dict(), F.EPISODE1, n_threads=4, flags=oracle.FLAG_CONTINUOUS)
    F.assert_like_batch_run(F.host_views(w), run, "episode 1")
    w.close()


@pytest.mark.parametrize("flags", [F.FLAG_CONTINUOUS, F.FLAG_CONTINUOUS | F.FLAG_SKIP_FROZEN], ids=["continuous", "skip-frozen"])
@pytest.mark.parametrize("lanes", F.LANES)
def test_twin_re_reset_equals_twin_fresh(lanes, flags, oracle, rough_terrain):
    """reset(P1), 120 steps, scribble, reset(P2), 60 steps on one twin world == reset(P2), 60 steps on a fresh one, arena byte for
    byte -- right after the reset (the image) and after the steps -- and both == oracle.batch_run."""
    m1, m2 = F.populations(lanes)
    ref = F.reference(lanes, flags, rough_terrain, oracle)
    w = F.twin_world(lanes, flags, rough_terrain)
    w.reset(m1)
    w.step(F.EPISODE1)
    F.scribble(w)
    dirty = F.host_views(w)
    assert dirty["frozen"].min() == 1 and dirty["steps"].max() == 7 and dirty["awake"].max() == 0
    w.reset(m2)
    assert F.differing(F.field_bytes(w), ref["image"]) == []
    for n in F.EPISODE2_CALLS:
        w.step(n)
    assert F.differing(F.field_bytes(w), ref["after_bytes"]) == []
    for views in (F.host_views(w), ref["after"]):
        F.assert_like_batch_run(views, ref["run"], "episode 2")
        assert int(views["steps"].min()) == F.EPISODE2
    w.close()


@pytest.mark.parametrize("lanes", F.LANES)
def test_twin_image_after_reset(lanes, oracle, rough_terrain):
    """The expected image of a reset, field by field over all padded rows: what rem2d_reset_kernel writes by reading it
    (csrc/rem2d_kernels.h) -- padding creatures and empty lanes carry no shape, no parent (-1), the fat AABB of a point at the
    origin and no mass; every pair slot of every lane is empty (edge -1); every per-creature word is 0 except `newfix`."""
    _, m2 = F.populations(lanes)
    ref = F.reference(lanes, F.FLAG_CONTINUOUS, rough_terrain, oracle)
    n, K, Np = m2.n_envs, lanes, {4: 48, 8: 24}[lanes]
    img = {k: np.frombuffer(v, dtype=np.uint8) for k, v in ref["image"].items()}

    def lane(name, dtype):
        return img[name].view(dtype).reshape(Np, K)
    shape = lane("shape", np.int32)
    assert np.array_equal(shape[:n], m2.arrays["shape"].reshape(n, K)) and not shape[n:].any()
    empty = shape == 0
    assert empty[:n].any() and (lane("parent", np.int32)[empty] == -1).all()
    assert np.array_equal(lane("parent", np.int32)[:n][~empty[:n]], m2.arrays["parent"].reshape(n, K)[~empty[:n]])
    ext = np.float32(0.1)
    for name, want in (("fatlx", -ext), ("fatly", -ext), ("fatux", ext), ("fatuy", ext)):
        assert (lane(name, np.float32)[empty] == want).all(), name
    for name in ("px", "py", "ang", "hx", "hy", "invm", "invi", "vx", "vy", "w", "sleept", "jax", "jtorque", "jimpx", "jmotorspeed"):
        assert not img[name].view(np.uint32).reshape(Np, K)[empty].any(), name
    assert (lane("awake", np.int32) == (~empty).astype(np.int32)).all()
    assert (lane("invm", np.float32)[~empty] > 0).all() and not lane("ccount", np.int32).any()
    assert (img["cedge"].view(np.int32) == -1).all() and len(img["cedge"]) == 4 * F.TWIN_SLOTS * Np * K
    for name in ("cinfo", "ckey0", "ckey1", "cn0", "cn1", "ct0", "ct1", "wod", "fitness", "reward", "done", "everdone", "frozen", "steps",
                 "invdt0", "err", "positers", "toievents"):
        assert not img[name].any(), name
    assert (img["newfix"].view(np.int32) == 1).all() and len(img["newfix"]) == 4 * Np


def test_gaps_are_what_the_layout_leaves(rough_terrain):
    """The alignment gaps between the five field groups (256-byte boundaries), from rem2d_cpu_world_field's offsets and counts:
    fields plus gaps tile the arena exactly."""
    for lanes in F.LANES:
        w = F.twin_world(lanes, 0, rough_terrain)
        g = F.gaps(w)
        used = sum(cnt * esz for _, cnt, esz in (F.field_place(w, n) for n in F._fields()))
        assert used + sum(hi - lo for lo, hi in g) == len(w.arena)
        assert all(hi % 256 == 0 and 0 < hi - lo < 256 for lo, hi in g) and len(g) >= 1, g
        w.close()
