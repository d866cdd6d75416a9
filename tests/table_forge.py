"""World tables across the launch split: what the host half (tests/test_world_tables_host.py) and the GPU half
(tests/test_world_tables_gpu.py) share.

Every between-steps call that takes a list of worlds packs them into a kernel-argument table -- CTL_TABLE = 16 worlds, STREAM_TABLE = 8
for rem2d_worlds_refill -- and launches once per table (csrc/rem2d.hip, table_launches: `for (first = 0; first < n_worlds; first +=
table)`), filling the shared CtlTable through control_table(.., first, n) and, for most calls, a second per-world table beside it (SenseTable: the
terrain; NvTable: env4; EpTable / StTable: morphology, env4, feed).  ONE forged list of N_WORLDS = 33 small worlds under one population
index serves all calls: a call with n worlds takes the first n.

What the list guarantees (asserted by the host half on WORLDS alone, before a device is involved):
  * counts: 16, 17, 32, 33 worlds for the CtlTable calls, 8, 9, 16, 17 for refill: a table exactly full, one over, a third launch;
  * lanes per creature 2 .. 64 in an unsorted order; a 64-lane world at slots 15 and 16 (last / first of a chunk of either table), a
    2-lane world at slots 7, 8 (refill's last / first), 0, 32 (first) and 31 (last);
  * 1, 2 and 3 64-lane blocks per world; the chunks' block totals are 29, 30, 3, 1 (CtlTable: worlds 0-15, 16-31, 16 alone, 32) and
    14, 15, 1, 3 (refill: 0-7, 8-15, 8 alone, 16): mod 4 they cover 1, 2, 3, so the last workgroup of a launch has wavefronts past the
    last block, and no two chunks of one call have the same total;
  * padding: 24 of the 33 worlds have creatures that do not fill their last block;
  * terrain: world 16 + i stands on another terrain than world i, of another pitch AND another x0 (PAIR); the obstacle list differs
    wherever hardcore4 is one of the two.  The creatures are PLACED on their own world's terrain (terrain_forge.place);
  * the population index is a permutation of all 33 worlds' creatures (`index`); its `short` form has n_rows below the creature count
    and creatures pointed out of range, a negative index (-2) and one of at least n_rows (n_rows + 3) on either side of each table's
    split (OUT_OF_RANGE: worlds 3 and 20, worlds 9 and 2).

State: reset, then SETTLE = 40 steps of continuous physics (`WorldSet`), so that contacts, joint limits, wall-of-death and step words
are not the reset's.  The step kernels are not under test here.

The expected-arena builders (`expected_control`, `expected_refill`) work on plain byte arrays and a {field: (offset, count, bytes per
element)} table, so that the host half can test them on fabricated arrays.
"""
import ctypes as C

import numpy as np

CTL_TABLE, STREAM_TABLE = 16, 8
CTL_COUNTS, REFILL_COUNTS = (16, 17, 32, 33), (8, 9, 16, 17)
MAX_BODIES, MAX_RAYS, MAX_SAMPLES = 64, 64, 16          # REM2D_CONTROL_MAX_BODIES, REM2D_SENSE_MAX_RAYS, REM2D_NOVELTY_MAX_SAMPLES
WAVE, CTL_WAVES = 64, 4                                  # CTL_THREADS / WAVE
CONT, SETTLE = 1, 40
CTRL_TARGET, CTRL_PARAMS = 0, 1
GUARD = 64

# (lanes per creature, creatures, kind) of world i
WORLDS = (
    (2, 70, "lsystem"), (16, 5, "lsystem"), (4, 16, "lsystem"), (64, 1, "lsystem"), (8, 19, "lsystem"), (32, 2, "lsystem"),
    (16, 3, "lsystem"), (2, 40, "chain"),
    (2, 20, "lsystem"), (8, 8, "lsystem"), (32, 4, "lsystem"), (4, 21, "lsystem"), (16, 9, "lsystem"), (8, 3, "chain"),
    (4, 40, "lsystem"), (64, 2, "lsystem"),
    (64, 3, "lsystem"), (2, 33, "lsystem"), (8, 17, "lsystem"), (16, 2, "lsystem"), (4, 7, "chain"), (32, 6, "lsystem"),
    (2, 10, "lsystem"), (16, 7, "lsystem"), (8, 12, "lsystem"), (64, 1, "lsystem"), (4, 35, "lsystem"), (32, 1, "chain"),
    (8, 5, "lsystem"), (16, 11, "lsystem"), (4, 18, "lsystem"), (2, 30, "lsystem"),
    (2, 9, "lsystem"),
)
N_WORLDS = len(WORLDS)
FIRST = ("saw_fine", "hardcore4", "saw_coarse", "shifted", "rough4")             # world i < 16: FIRST[i % 5]
PAIR = {"saw_fine": "saw_coarse", "saw_coarse": "hardcore4", "shifted": "saw_fine", "hardcore4": "saw_coarse", "rough4": "saw_fine"}
SHORT_BY = 9                         # the short index: n_rows = creatures - 9
OUT_OF_RANGE = ((3, 0, -2), (20, 4, +3), (9, 5, -2), (2, 11, +3))     # (world, creature, index: negative as it is, else n_rows + it)
# bodies per creature a lane count takes from the L-system pool
BODIES = {2: (1, 2), 4: (2, 4), 8: (3, 8), 16: (5, 16), 32: (6, 16), 64: (6, 16)}


def blocks(i):
    K, n, _ = WORLDS[i]
    return (n * K + WAVE - 1) // WAVE


def padded(i):
    """creatures of world i's arena, padding included"""
    K = WORLDS[i][0]
    return blocks(i) * (WAVE // K)


def chunks(n_worlds, table):
    """[(first, n)] of a call with n_worlds worlds"""
    return [(first, min(table, n_worlds - first)) for first in range(0, n_worlds, table)]


def chunk_blocks(n_worlds, table):
    return [sum(blocks(i) for i in range(first, first + n)) for first, n in chunks(n_worlds, table)]


def terrain_name(i):
    if i < CTL_TABLE:
        return FIRST[i % len(FIRST)]
    if i < 2 * CTL_TABLE:
        return PAIR[terrain_name(i - CTL_TABLE)]
    return "rough4"


def terrain(i):
    import terrain_forge as TF
    return TF.profile(terrain_name(i))


def terrain_facts(name):
    """(pitch, x0, obstacles) of a terrain_forge terrain"""
    import terrain_forge as TF
    p = TF.profile(name)
    return float(p.xs[-1] - p.xs[0]) / (len(p.xs) - 1), float(p.xs[0]), len(p.polys)


# ----------------------------------------------------------------------------------------------------------------- creatures
_POOL, _MORPHS = [], {}


def _pool():
    if not _POOL:
        from gym_rem2d_amd import synthetic
        _POOL.extend(synthetic.lsystem_specs(range(300)))
    return _POOL


def morphology(i):
    """The creatures of world i, placed on world i's terrain (cached; treat as read-only)."""
    if i not in _MORPHS:
        import terrain_forge as TF
        from gym_rem2d_amd import synthetic
        from gym_rem2d_amd.compiler import Morphology
        K, n, kind = WORLDS[i]
        if kind == "chain":
            m = synthetic.chain_population(n, min(K, 6), "left", lanes=K)
        else:
            lo, hi = BODIES[K]
            fit = [s for s in _pool() if lo <= s.n_bodies <= hi]
            m = Morphology.from_specs([fit[(7 * i + 3 * e) % len(fit)] for e in range(n)], K)
        name = terrain_name(i)
        prof = TF.profile(name)
        m = TF.place(m, prof, TF.TERRAINS[name][2](prof, n, (0.13 * i + 0.05) % 1.0))
        _MORPHS[i] = m
    return _MORPHS[i]


def roots(i):
    """root px, py float32 [n] of world i's creatures as placed"""
    m = morphology(i)
    return m.arrays["x"].reshape(m.n_envs, m.lanes)[:, 0].copy(), m.arrays["y"].reshape(m.n_envs, m.lanes)[:, 0].copy()


def sense_rays():
    """the ten default rays, their mirror images and three more: 23 rays"""
    import range_model as R
    r = R.bipedal_rays()
    return np.ascontiguousarray(np.concatenate([r, r * [-1.0, 1.0], [[6.0, -0.4], [-5.0, 0.3], [0.1, 0.05]]]), np.float64)


# --------------------------------------------------------------------------------------------------------- the population index
def n_creatures(n_worlds=N_WORLDS):
    return sum(w[1] for w in WORLDS[:n_worlds])


def index(short=False):
    """-> ([int32 rows of world i's creatures], n_rows): a permutation of all creatures; `short`: see the module docstring"""
    total = n_creatures()
    perm = np.random.default_rng(33).permutation(total).astype(np.int32)
    rows, at = [], 0
    for K, n, _ in WORLDS:
        rows.append(perm[at:at + n].copy())
        at += n
    if not short:
        return rows, total
    n_rows = total - SHORT_BY
    for w, e, v in OUT_OF_RANGE:
        rows[w][e] = v if v < 0 else n_rows + v
    return rows, n_rows


# ------------------------------------------------------------------------------------------------------ expected-arena builders
def _lane_f64(arena, places, name, Np, K):
    off, cnt, esz = places[name]
    assert cnt == Np * K and esz == 8, (name, cnt, esz)
    return arena[off:off + cnt * esz].view(np.float64).reshape(Np, K)


def expected_control(before, places, Np, K, live, parent, rows, n_rows, mode, values, mask, max_bodies):
    """The arena rem2d_worlds_control leaves: `before` (uint8) with the controller words of the selected (creature, body) pairs
    replaced -- a live lane with a parent, of body rank 1 .. max_bodies - 1 among its creature's live lanes, of a creature whose row
    lies in [0, n_rows) and whose mask byte (if any) is set -- by 0.0 / values[row, body] (CTRL_TARGET: camp, coffset) or
    values[row, body, 0 .. 3] (CTRL_PARAMS: camp, cphase, cfreq, coffset).  live, parent [n, K]; rows [n].  -> (arena, pairs written)"""
    exp = before.copy()
    live = np.asarray(live, bool)
    body = np.cumsum(live, axis=1) - 1
    r = np.asarray(rows, np.int64)
    sel = live & (np.asarray(parent) >= 0) & (body >= 1) & (body < max_bodies) & ((r >= 0) & (r < n_rows))[:, None]
    e, lane = np.nonzero(sel)
    at = r[e] * max_bodies + body[e, lane]
    if mask is not None:
        keep = np.asarray(mask).reshape(-1)[at] != 0
        e, lane, at = e[keep], lane[keep], at[keep]
    if mode == CTRL_TARGET:
        _lane_f64(exp, places, "camp", Np, K)[e, lane] = 0.0
        _lane_f64(exp, places, "coffset", Np, K)[e, lane] = np.asarray(values, np.float64).reshape(-1)[at]
    else:
        v = np.asarray(values, np.float64).reshape(-1, 4)[at]
        for q, name in enumerate(("camp", "cphase", "cfreq", "coffset")):
            _lane_f64(exp, places, name, Np, K)[e, lane] = v[:, q]
    return exp, len(e)


def expected_refill(before, fresh, places, Np, K, slots, took, retired):
    """The arena rem2d_worlds_refill leaves: `before` with every field element of the creatures `took` (bool [n]) taken from `fresh`
    (the arena of a world reset with the new occupants and never stepped), and the `frozen` word of the creatures `retired` set to 1."""
    exp = before.copy()
    at = np.flatnonzero(took)
    for name, (off, cnt, esz) in places.items():
        dt = np.uint32 if esz == 4 else np.uint64
        e, f = exp[off:off + cnt * esz].view(dt), fresh[off:off + cnt * esz].view(dt)
        if cnt == Np * K:
            e.reshape(Np, K)[at] = f.reshape(Np, K)[at]
        elif cnt == Np * K * slots:
            e.reshape(slots, Np, K)[:, at] = f.reshape(slots, Np, K)[:, at]
        else:
            assert cnt == Np, (name, cnt)
            e[at] = f[at]
    off, cnt, esz = places["frozen"]
    assert cnt == Np and esz == 4
    exp[off:off + cnt * esz].view(np.int32)[np.flatnonzero(retired)] = 1
    return exp


# ------------------------------------------------------------------------------------------------------------- on the device
def world_array(worlds):
    """the `rem2d_world *` array of a list of BatchedWorld; None = a NULL entry"""
    return (C.c_void_p * len(worlds))(*[None if w is None else w.h for w in worlds])


def places_of(world):
    import lifecycle_forge as LF
    from gym_rem2d_amd import _lib
    return {name: LF.field_place(world, name) for name in _lib.FIELDS}


class Guarded:
    """A device buffer of `shape` between two guards of GUARD rows, all prefilled with `fill`; `inner` is what a call is given."""

    def __init__(self, torch, shape, dtype, fill):
        self.shape, self.fill = tuple(shape), fill
        self.raw = torch.full((shape[0] + 2 * GUARD,) + tuple(shape[1:]), fill, dtype=dtype, device="cuda")
        self.inner = self.raw[GUARD:GUARD + shape[0]]

    def host(self):
        """the inner rows on the host, after checking that the guards are whole"""
        a = self.raw.cpu().numpy()
        g = np.concatenate([a[:GUARD].reshape(-1), a[GUARD + self.shape[0]:].reshape(-1)])
        assert (g == a.dtype.type(self.fill)).all(), "a guard row was written"
        return a[GUARD:GUARD + self.shape[0]].copy()


class WorldSet:
    """The first n worlds of WORLDS on the device in one build: reset, SETTLE steps, the population index installed.  `restore()`
    puts back every arena and every world's device morphology as they were after the settle."""

    def __init__(self, torch, n=N_WORLDS, wide=False):
        from gym_rem2d_amd.world import BatchedWorld
        self.torch, self.n, self.wide = torch, n, wide
        self.worlds, self.morphs = [], [morphology(i) for i in range(n)]
        total = n_creatures()
        self.reward, self.done = torch.zeros(total, device="cuda"), torch.zeros(total, dtype=torch.bool, device="cuda")
        try:
            for i, m in enumerate(self.morphs):
                w = BatchedWorld(m.n_envs, m.lanes, CONT, wide=wide)
                self.worlds.append(w)
                assert w.n_envs_padded == padded(i)
                w.set_terrain(terrain(i))
                w.reset(m)
                w.step(SETTLE)
            self.use_index(False)
            torch.cuda.synchronize()
            self._arenas = [w.arena.clone() for w in self.worlds]
            self._morph_dev = [{k: v.clone() for k, v in w._morph_dev.items()} for w in self.worlds]
        except BaseException:
            self.close()
            raise
        self.places = [places_of(w) for w in self.worlds]
        self._states = None

    def use_index(self, short):
        """install the full or the short population index -> n_rows"""
        torch = self.torch
        rows, self.n_rows = index(short)
        self.rows = rows[:self.n]
        self._index_dev = [torch.from_numpy(r).to("cuda") for r in self.rows]
        for w, idx in zip(self.worlds, self._index_dev):
            w.set_outputs(self.reward, self.done, idx)
        return self.n_rows

    def restore(self):
        for w, a, md in zip(self.worlds, self._arenas, self._morph_dev):
            w.arena.copy_(a)
            for k, v in md.items():
                w._morph_dev[k].copy_(v)

    def states(self):
        """replay.read_state of every world as it stands after the settle (cached: call on a restored set)"""
        if self._states is None:
            from replay import read_state
            self._states = [read_state(w) for w in self.worlds]
        return self._states

    def arenas(self, n=None):
        import lifecycle_forge as LF
        return [LF.arena_bytes(w) for w in self.worlds[:n]]

    def close(self):
        for w in self.worlds:
            w.close()
        self.worlds = []
