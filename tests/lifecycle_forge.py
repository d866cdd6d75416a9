"""World reuse: what the host half (tests/test_lifecycle_host.py, twin and oracle alone) and the GPU half
(tests/test_lifecycle_gpu.py) of the re-reset / dirty-arena / recycled-scratch tests share.

Protocol, one lane bucket at a time: a world runs EPISODE1 steps of population P1, is scribbled on (``scribble``: dirt an episode
alone might not leave), is reset to population P2 of the same world shape and runs EPISODE2 steps in the calls EPISODE2_CALLS.  It
must then be indistinguishable, in every byte of every field over ALL padded rows (``field_bytes``), from a world that saw P2 only.
Rough terrain (seed 4), continuous physics.  Everything is compared with ``==``; there is no tolerance anywhere.

The buckets: lanes 4 with 37 creatures (48 padded: 11 padding creatures, 3 blocks of 64 lanes, the last one mostly padding) and lanes
8 with 21 creatures (24 padded, 3 blocks) -- several blocks, so the step train hands over between blocks.  P1 and P2 come from
disjoint seed ranges of ``synthetic.lsystem_specs(mutate_odd=True)``, picked (SEEDS) so that P2 has empty lanes where P1 had bodies
and bodies where P1 had none, each in at least a quarter of the creatures (``swap_counts``; asserted by the host half).

What episode 1 leaves behind, oracle alone (`python tests/lifecycle_forge.py` prints it; asserted > 0 by the host half):

| bucket  | touching manifolds | joints with impulse | contact points with impulse | TOI events | creatures at 60 position iterations | creatures with wod > 0 |
|---------|--------------------|---------------------|-----------------------------|------------|-------------------------------------|------------------------|
| lanes 4 | 73                 | 91                  | 82                          | 90         | 2                                   | 37                     |
| lanes 8 | 36                 | 101                 | 36                          | 51         | 1                                   | 21                     |
"""
import ctypes as C

import numpy as np

FLAG_CONTINUOUS, FLAG_SKIP_FROZEN, FLAG_RETILE = 1, 8, 16
EPISODE1 = 120
EPISODE2_CALLS = (1, 9, 50)
EPISODE2 = sum(EPISODE2_CALLS)
GRAPH_CALLS = (10, 10, 10)            # the graph replay test's second episode
LANES = (4, 8)
TWIN_SLOTS = 24                       # pair slots per body of the twin (the default build's; the wide build has 32)

# (P1, P2) per lane bucket: seeds of synthetic.lsystem_specs(mutate_odd=True) whose creature falls into the bucket
SEEDS = {
    4: ((4, 5, 10, 11, 13, 18, 25, 30, 33, 49, 52, 68, 71, 77, 81, 83, 87, 89, 93, 99, 103, 106, 124, 128, 131, 136, 141, 148, 151,
         152, 155, 156, 157, 158, 175, 188, 194),
        (1004, 1005, 1008, 1019, 1012, 1026, 1013, 1032, 1035, 1067, 1038, 1068, 1040, 1052, 1055, 1060, 1061, 1082, 1074, 1077,
         1081, 1083, 1086, 1088, 1102, 1094, 1096, 1099, 1107, 1108, 1113, 1114, 1120, 1131, 1121, 1123, 1132)),
    8: ((2, 8, 15, 19, 23, 31, 32, 34, 38, 41, 98, 142, 149, 176, 184, 190, 202, 205, 224, 265, 281),
        (1028, 1058, 1059, 1071, 1072, 1075, 1078, 1080, 1098, 1118, 1103, 1174, 1138, 1253, 1143, 1244, 1133, 1157, 1206, 1246,
         1213)),
}
N_ENVS = {k: len(v[0]) for k, v in SEEDS.items()}

LANE_FIELDS = ("px", "py", "ang", "vx", "vy", "w", "sleept", "hx", "hy", "invm", "invi", "fatlx", "fatly", "fatux", "fatuy", "awake",
               "ccount", "shape")
JOINT_FIELDS = ("jax", "jay", "jbx", "jby", "jtorque", "jlower", "jupper", "jimpx", "jimpy", "jimpz", "jmotorimp", "jmotorspeed",
                "jlimit", "camp", "cphase", "cfreq", "coffset", "cistate", "parent")
ENV_FIELDS = ("wod", "fitness", "reward", "done", "everdone", "frozen", "steps", "invdt0", "positers", "toievents")
# what rem2d_reset_kernel leaves in a pair slot (the wide build's slots beyond the twin's 24 are compared with these)
SLOT_RESET = {"cedge": -1, "cinfo": 0, "ckey0": 0, "ckey1": 0, "cn0": 0.0, "cn1": 0.0, "ct0": 0.0, "ct1": 0.0}

_POPULATIONS = {}


# ---------------------------------------------------------------------------------------------------------------- populations
def populations(lanes):
    """(P1, P2): two Morphology batches of one world shape."""
    if lanes not in _POPULATIONS:
        from gym_rem2d_amd import synthetic
        from gym_rem2d_amd.compiler import Morphology, lanes_for
        out = []
        for seeds in SEEDS[lanes]:
            specs = synthetic.lsystem_specs(seeds, mutate_odd=True)
            assert all(lanes_for(s.n_bodies) == lanes for s in specs)
            out.append(Morphology.from_specs(specs, lanes))
        _POPULATIONS[lanes] = tuple(out)
    return _POPULATIONS[lanes]


def swap_counts(m1, m2):
    """(creatures in which P2 has an empty lane where P1 had a body, creatures in which P2 has a body where P1 had none)."""
    a = m1.arrays["shape"].reshape(m1.n_envs, m1.lanes) != 0
    b = m2.arrays["shape"].reshape(m2.n_envs, m2.lanes) != 0
    return int((a & ~b).any(axis=1).sum()), int((~a & b).any(axis=1).sum())


def hub_population(lanes=8):
    """P1 of the lanes-8 bucket with creature 1 replaced by the five-child hub of tests/test_env_gpu.py (schedule period 5: the
    default build flags its tile REM2D_ERR_SOLVER_OVERFLOW)."""
    from gym_rem2d_amd import synthetic
    from gym_rem2d_amd.compiler import CreatureBuilder, CreatureSpec, Morphology
    b = CreatureBuilder()
    hub = b.add_box(0.25, 0.25, 5.0, 7.0, 0.0)
    for k in range(5):
        ang = 2.0 * np.pi * k / 5
        child = b.add_box(0.1, 0.3, 5.0 + 0.55 * np.cos(ang), 7.0 + 0.55 * np.sin(ang), ang - np.pi / 2)
        b.add_revolute(hub, child, (0.25 * np.cos(ang), 0.25 * np.sin(ang)), (0.0, -0.3), 50.0)
    star = CreatureSpec(b, list(range(6)))
    assert star.period == 5
    specs = synthetic.lsystem_specs(SEEDS[lanes][0], mutate_odd=True)
    specs[1] = star
    return Morphology.from_specs(specs, lanes)


# ---------------------------------------------------------------------------------------------------------------- dirt
def scribble(world):
    """Overwrite, through ``view(name)``, what an episode alone might leave clean: every per-creature int field with 1, the step /
    iteration / event counters with 7, the per-creature floats with 3.5, and on every lane a sleep timer of 0.4 on a sleeping body.
    Works on a BatchedWorld (torch views) and on the twin's CpuWorld (numpy views) alike."""
    for name in ("done", "everdone", "frozen", "err", "newfix"):
        world.view(name)[...] = 1
    for name in ("steps", "positers", "toievents"):
        world.view(name)[...] = 7
    for name in ("wod", "fitness", "reward", "invdt0"):
        world.view(name)[...] = 3.5
    world.view("sleept")[...] = 0.4
    world.view("awake")[...] = 0


# ---------------------------------------------------------------------------------------------------------------- the arena
def _fields():
    from gym_rem2d_amd import _lib
    return _lib.FIELDS


def field_place(world, name):
    """(byte offset, element count over ALL padded rows, bytes per element) of a field, from rem2d_world_field (the twin: its
    counterpart)."""
    if hasattr(world, "field"):                      # oracle.cpu_twin.CpuWorld
        off, cnt, dt = world.field(name)
    else:
        from gym_rem2d_amd import _lib
        o, c, d = C.c_size_t(), C.c_size_t(), C.c_int32()
        _lib.check(world.L.rem2d_world_field(world.h, _lib.FIELD_ID[name], C.byref(o), C.byref(c), C.byref(d)), world.wide)
        off, cnt, dt = o.value, c.value, d.value
    return off, cnt, 8 if dt == 2 else 4


def arena_bytes(world):
    """The whole arena as a host uint8 array (a copy)."""
    a = world.arena
    if isinstance(a, np.ndarray):
        return a.copy()
    import torch
    torch.cuda.synchronize(a.device)
    return a.cpu().numpy()


def field_bytes(world):
    """{field: raw bytes over all padded rows} for every field of _lib.FIELDS -- padding creatures and empty lanes included, which
    ``view(name)`` cuts off."""
    a = arena_bytes(world)
    out = {}
    for name in _fields():
        off, cnt, esz = field_place(world, name)
        out[name] = a[off:off + cnt * esz].tobytes()
    return out


def gaps(world):
    """[(start, end)] byte ranges of the arena that belong to no field: the alignment gaps behind the five field groups, from
    rem2d_world_field's offsets and counts (fields of a group are contiguous; a group starts on a 256-byte boundary)."""
    spans = sorted((off, off + cnt * esz) for off, cnt, esz in (field_place(world, n) for n in _fields()))
    total = len(world.arena) if isinstance(world.arena, np.ndarray) else world.arena.numel()
    out, at = [], 0
    for lo, hi in spans:
        assert lo >= at, "fields overlap"
        if lo > at:
            out.append((at, lo))
        at = hi
    if total > at:
        out.append((at, total))
    return out


def widen_image(image, world):
    """The twin's image (24 pair slots) as the fields of `world` must look right after a reset: the same bytes, and in a build with
    more pair slots (the wide one: 32) the further slots as rem2d_reset_kernel leaves them."""
    slots = getattr(world, "contact_slots", TWIN_SLOTS)
    if slots == TWIN_SLOTS:
        return image
    out = dict(image)
    for name, value in SLOT_RESET.items():
        dtype = np.int32 if name in ("cedge", "cinfo", "ckey0", "ckey1") else np.float32
        have = np.frombuffer(image[name], dtype=dtype)
        more = np.full(len(have) // TWIN_SLOTS * (slots - TWIN_SLOTS), value, dtype=dtype)
        out[name] = np.concatenate([have, more]).tobytes()
    return out


def differing(a, b):
    """Names of the fields whose bytes differ."""
    assert a.keys() == b.keys()
    return [n for n in a if a[n] != b[n]]


def recreate_on(world, arena):
    """Give a BatchedWorld a new handle on `arena` (a 256-byte aligned uint8 device tensor of at least rem2d_state_bytes, with
    whatever it holds) through rem2d_world_create: the ABI lets a caller hand over any memory.  Terrain and options start over."""
    from gym_rem2d_amd import _lib
    nbytes = world.L.rem2d_state_bytes(C.byref(world.cfg))
    assert arena.numel() >= nbytes and arena.data_ptr() % 256 == 0
    world.close()
    world._views = {}
    world.arena = arena
    h = C.c_void_p()
    _lib.check(world.L.rem2d_world_create(C.byref(world.cfg), arena.data_ptr(), nbytes, C.byref(h)), world.wide)
    world.h = h
    return world


def raw_reset(world, morph):
    """rem2d_world_reset alone -- no new tile table, so nothing a captured graph embeds changes: the world keeps the default tiles
    of rem2d_world_create, which are valid for every morphology of its shape."""
    import torch
    from gym_rem2d_amd import _lib
    dev = {k: torch.from_numpy(np.ascontiguousarray(morph.arrays[k])).to(world.device) for k in _lib.MORPH_FIELDS}
    m = _lib.Morph()
    for k in _lib.MORPH_FIELDS:
        setattr(m, k, dev[k].data_ptr())
    world._morph_dev = dev
    _lib.check(world.L.rem2d_world_reset(world.h, C.byref(m), world._stream()), world.wide)


# ---------------------------------------------------------------------------------------------------------------- comparisons
def host_views(world, names=None):
    """{field: host numpy array in view(name)'s shape ([n_envs, lanes], [slots, n_envs, lanes] or [n_envs])}."""
    out = {}
    for name in (names or _fields()):
        v = world.view(name)
        out[name] = v.copy() if isinstance(v, np.ndarray) else v.cpu().numpy()
    return out


def assert_like_oracle(got, ref, what=""):
    """The masked comparisons of tests/test_cpu_twin.py between two sets of host views (``host_views``): `ref` is the twin's, i.e.
    the oracle's state -- bodies and static lane fields on live lanes, joint fields and impulses on jointed lanes, every
    per-creature field the oracle maintains, the pair lists in list order (edge, point count, manifold type, feature keys, impulses)."""
    active = ref["shape"] != 0
    jointed = active & (ref["parent"] >= 0)
    for name in LANE_FIELDS:
        assert np.array_equal(got[name][active], ref[name][active]), (name, what)
    for name in JOINT_FIELDS:
        assert np.array_equal(got[name][jointed], ref[name][jointed]), (name, what)
    for name in ENV_FIELDS:
        assert np.array_equal(got[name], ref[name]), (name, what)
    cc, gi, ci = ref["ccount"], got["cinfo"], ref["cinfo"]
    for k in range(int(cc.max())):
        m = active & (cc > k)
        assert np.array_equal(got["cedge"][k][m], ref["cedge"][k][m]), ("cedge", what)
        assert np.array_equal(gi[k][m] & 0xff, ci[k][m] & 0xff), ("point count", what)
        touching = m & ((ci[k] & 0xff) > 0)
        assert np.array_equal((gi[k][touching] >> 8) & 0xff, (ci[k][touching] >> 8) & 0xff), ("manifold type", what)
        for j, (key, nn, tt) in enumerate((("ckey0", "cn0", "ct0"), ("ckey1", "cn1", "ct1"))):
            mj = m & ((ci[k] & 0xff) > j)
            for name in (key, nn, tt):
                assert np.array_equal(got[name][k][mj], ref[name][k][mj]), (name, what)


def bodies_of(views):
    """[n_envs, lanes, 8] like BatchedWorld.bodies(), from host views."""
    cols = [views[k].astype(np.float32) for k in ("px", "py", "ang", "vx", "vy", "w", "sleept")]
    cols.append(views["awake"].astype(np.float32))
    return np.stack(cols, axis=-1)


def assert_like_batch_run(got, run, what=""):
    """Host views against oracle.batch_run's result: bodies, reward, done (= ever done) and fitness."""
    assert np.array_equal(bodies_of(got), run["bodies"]), ("bodies", what)
    assert np.array_equal(got["reward"], run["reward"].astype(np.float32)), ("reward", what)
    assert np.array_equal(got["everdone"], run["done"]), ("done", what)
    assert np.array_equal(got["fitness"], run["fitness"]), ("fitness", what)


# ---------------------------------------------------------------------------------------------------------------- the reference
_REFERENCE = {}


def twin_world(lanes, flags, terrain):
    from oracle import cpu_twin
    cpu_twin.build()
    w = cpu_twin.CpuWorld(N_ENVS[lanes], lanes, flags)
    w.set_terrain(terrain)
    return w


def leftovers(views):
    """What an episode has left in a world, from host views: the counts of the module docstring's table."""
    active = views["shape"] != 0
    jointed = active & (views["parent"] >= 0)
    cc = views["ccount"]
    slot = (np.arange(views["cinfo"].shape[0])[:, None, None] < cc[None]) & active[None]
    npts = np.where(slot, views["cinfo"] & 0xff, 0)
    imp = ((views["cn0"] != 0) | (views["ct0"] != 0)) & (npts > 0)
    imp1 = ((views["cn1"] != 0) | (views["ct1"] != 0)) & (npts > 1)
    jimp = (views["jimpx"] != 0) | (views["jimpy"] != 0) | (views["jimpz"] != 0) | (views["jmotorimp"] != 0)
    return {"touching manifolds": int((npts > 0).sum()), "joints with impulse": int((jimp & jointed).sum()),
            "contact points with impulse": int(imp.sum() + imp1.sum()), "TOI events": int(views["toievents"].sum()),
            "creatures at 60 position iterations": int((views["positers"] == 60).sum()),
            "creatures with wod > 0": int((views["wod"] > 0).sum())}


def reference(lanes, flags, terrain, oracle):
    """Per (bucket, world flags), made once: ``image`` -- the twin's fields right after reset(P2), the expected image of a GPU
    reset --, ``after`` -- a fresh twin's host views after episode 2 --, ``after30`` -- after GRAPH_CALLS --, and ``run`` /
    ``run30`` -- oracle.batch_run of P2 over the same steps."""
    key = (lanes, flags)
    if key not in _REFERENCE:
        from conftest import oracle_terrain
        _, m2 = populations(lanes)
        w = twin_world(lanes, flags, terrain)
        w.reset(m2)
        ref = {"image": field_bytes(w)}
        for n in EPISODE2_CALLS:
            w.step(n)
        ref["after"], ref["after_bytes"] = host_views(w), field_bytes(w)
        w.close()
        w = twin_world(lanes, flags, terrain)
        w.reset(m2)
        for n in GRAPH_CALLS:
            w.step(n)
        ref["after30"] = host_views(w)
        w.close()
        ot = oracle_terrain(oracle, terrain)
        oflags = oracle.FLAG_CONTINUOUS if flags & FLAG_CONTINUOUS else 0
        ref["run"] = oracle.batch_run(ot, m2.as_dict(), EPISODE2, n_threads=4, flags=oflags)
        ref["run30"] = oracle.batch_run(ot, m2.as_dict(), sum(GRAPH_CALLS), n_threads=4, flags=oflags)
        _REFERENCE[key] = ref
    return _REFERENCE[key]


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from gym_rem2d_amd import make_terrain
    for k in LANES:
        p1, p2 = populations(k)
        tw = twin_world(k, FLAG_CONTINUOUS, make_terrain(4))
        tw.reset(p1)
        tw.step(EPISODE1)
        print("lanes", k, "swap", swap_counts(p1, p2), leftovers(host_views(tw)))
        tw.close()
