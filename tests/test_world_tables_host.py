"""The host half of the world-table tests (tests/table_forge.py; the GPU half is tests/test_world_tables_gpu.py): the conditions the
forged list of worlds must meet for the GPU half to mean anything, asserted on its plain description; the expected-arena builders
on fabricated byte arrays; and the constants the forge assumes, read from the headers as text.  No GPU."""
import os
import re

import numpy as np

import range_model as R
import table_forge as TB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(path, name):
    text = open(os.path.join(ROOT, path)).read()
    m = re.findall(r"^#define %s (\d+)\b" % name, text, flags=re.M)
    assert len(m) == 1, "%s: %d definitions of %s" % (path, len(m), name)
    return int(m[0])


# ------------------------------------------------------------------------------------------------------------- the constants
def test_the_constants_are_the_headers():
    """a change of either table size, of the wave / workgroup shape or of a REM2D_*_MAX fails here, not by emptying the GPU half"""
    assert _define("gym_rem2d_amd/csrc/rem2d_control.h", "CTL_TABLE") == TB.CTL_TABLE == 16
    assert _define("gym_rem2d_amd/csrc/rem2d_stream.h", "STREAM_TABLE") == TB.STREAM_TABLE == 8
    assert _define("gym_rem2d_amd/csrc/rem2d_control.h", "CTL_THREADS") == TB.CTL_WAVES * TB.WAVE
    assert _define("include/rem2d_control.h", "REM2D_CONTROL_MAX_BODIES") == TB.MAX_BODIES
    assert _define("include/rem2d_sense.h", "REM2D_SENSE_MAX_RAYS") == TB.MAX_RAYS
    assert _define("include/rem2d_novelty.h", "REM2D_NOVELTY_MAX_SAMPLES") == TB.MAX_SAMPLES
    assert _define("include/rem2d_control.h", "REM2D_CTRL_TARGET") == TB.CTRL_TARGET
    assert _define("include/rem2d_control.h", "REM2D_CTRL_PARAMS") == TB.CTRL_PARAMS
    # the host layer has ONE chunked loop over worlds, in table_launches, stepping by that helper's table-size parameter; the helper
    # is called with one of the two tables, CTL_TABLE by five calls and STREAM_TABLE by one; and the two kernels' second tables are
    # as long
    src = open(os.path.join(ROOT, "gym_rem2d_amd/csrc/rem2d.hip")).read()
    helper = re.search(r"static int table_launches\(int (\w+), rem2d_world \*const \*worlds, int n_worlds, Launch launch\) \{\n(.*?)\n\}\n", src, flags=re.S)
    assert helper and helper.group(1) == "table"
    assert re.findall(r"first \+= *(\w+)", src) == ["table"] and len(re.findall(r"\bfirst *\+=|\+= *(?:CTL|STREAM)_TABLE\b", src)) == 1
    assert re.findall(r"for \(int first = 0; first < n_worlds; first \+= (\w+)\)", helper.group(2)) == ["table"]
    assert "control_table(Tb, worlds, first, n)" in helper.group(2) and "std::min(table, n_worlds - first)" in helper.group(2)
    calls = re.findall(r"\btable_launches\((?!int )([^,]*),", src)
    assert sorted(calls) == ["CTL_TABLE"] * 5 + ["STREAM_TABLE"], calls
    assert len(re.findall(r"\bcontrol_table\(", src)) == 2          # (its definition, and the helper)
    for path, member in (("rem2d_sense.h", r"SenseTerrain t\[CTL_TABLE\]"), ("rem2d_novelty.h", r"char \*env4\[CTL_TABLE\]"),
                         ("rem2d_episode.h", r"EpWorld w\[CTL_TABLE\]"), ("rem2d_stream.h", r"StWorld w\[STREAM_TABLE\]")):
        assert re.search(member, open(os.path.join(ROOT, "gym_rem2d_amd/csrc", path)).read()), path


# ---------------------------------------------------------------------------------------------------------- the world list
def test_counts_lanes_and_slots():
    assert TB.CTL_COUNTS == (TB.CTL_TABLE, TB.CTL_TABLE + 1, 2 * TB.CTL_TABLE, 2 * TB.CTL_TABLE + 1)
    assert TB.REFILL_COUNTS == (TB.STREAM_TABLE, TB.STREAM_TABLE + 1, 2 * TB.STREAM_TABLE, 2 * TB.STREAM_TABLE + 1)
    assert TB.N_WORLDS == max(TB.CTL_COUNTS) >= max(TB.REFILL_COUNTS)
    lanes = [w[0] for w in TB.WORLDS]
    assert set(lanes) == {2, 4, 8, 16, 32, 64}
    assert lanes != sorted(lanes) and lanes != sorted(lanes, reverse=True)
    for n in TB.CTL_COUNTS + TB.REFILL_COUNTS:      # ... and no call's list is sorted either
        assert lanes[:n] != sorted(lanes[:n])
    # a 64-lane and a 2-lane world at a chunk's first and at a chunk's last slot, for either table
    for table, counts in ((TB.CTL_TABLE, TB.CTL_COUNTS), (TB.STREAM_TABLE, TB.REFILL_COUNTS)):
        first = {f for n in counts for f, _ in TB.chunks(n, table) if f > 0}
        last = {f + k - 1 for n in counts for f, k in TB.chunks(n, table) if k == table}
        assert table in first
        for K in (2, 64):
            assert any(lanes[i] == K for i in first), (table, K, "first")
            assert any(lanes[i] == K for i in last), (table, K, "last")
    assert lanes[TB.CTL_TABLE] == 64 and lanes[TB.STREAM_TABLE] == 2
    # refill's shared feeds: worlds 7 / 8 and 15 / 16 hold creatures of one lane count
    assert lanes[7] == lanes[8] and lanes[15] == lanes[16]


def test_blocks_and_padding():
    nb = [TB.blocks(i) for i in range(TB.N_WORLDS)]
    assert set(nb) == {1, 2, 3}
    for table, counts in ((TB.CTL_TABLE, TB.CTL_COUNTS), (TB.STREAM_TABLE, TB.REFILL_COUNTS)):
        mods = set()
        for n in counts:
            totals = TB.chunk_blocks(n, table)
            assert len(totals) == len(TB.chunks(n, table)) == -(-n // table)
            assert len(set(totals)) == len(totals), (n, totals)          # a chunk that kept the previous chunk's blockEnd base shows
            mods |= {t % TB.CTL_WAVES for t in totals}
        assert mods >= {1, 2, 3}, (table, mods)                          # wavefronts past the last block in the last workgroup
    assert TB.chunk_blocks(33, TB.CTL_TABLE) == [29, 30, 1] and TB.chunk_blocks(17, TB.CTL_TABLE) == [29, 3]
    assert TB.chunk_blocks(17, TB.STREAM_TABLE) == [14, 15, 3] and TB.chunk_blocks(9, TB.STREAM_TABLE) == [14, 1]
    short = [i for i, (K, n, _) in enumerate(TB.WORLDS) if (n * K) % TB.WAVE]
    assert len(short) >= 16 and any(i < 8 for i in short) and any(8 <= i < 16 for i in short) and any(i >= 16 for i in short)
    assert all(TB.padded(i) * TB.WORLDS[i][0] == TB.blocks(i) * TB.WAVE for i in range(TB.N_WORLDS))


def test_the_creatures():
    from gym_rem2d_amd.compiler import lanes_for
    kinds = set()
    for i, (K, n, kind) in enumerate(TB.WORLDS):
        m = TB.morphology(i)
        assert (m.n_envs, m.lanes) == (n, K)
        live = (m.arrays["shape"] != 0).reshape(n, K)
        assert live[:, 0].all() and live.sum(axis=1).max() <= K
        assert K >= 32 or lanes_for(int(live.sum(axis=1).max())) == K       # a bucket's creatures need the bucket
        px, _ = TB.roots(i)
        assert len(np.unique(px)) == n                                      # no two creatures of a world stand at one place
        kinds.add(kind)
        xs = TB.terrain(i).xs
        assert ((px >= xs[0] - 3.0) & (px <= xs[-1] + 3.0)).all()
    assert kinds == {"lsystem", "chain"}
    jointed = sum(int(((TB.morphology(i).arrays["parent"] >= 0) & (TB.morphology(i).arrays["shape"] != 0)).sum()) for i in range(TB.N_WORLDS))
    assert jointed > 1000


def test_terrains_differ_across_the_split():
    names = [TB.terrain_name(i) for i in range(TB.N_WORLDS)]
    assert set(names) == {"saw_fine", "saw_coarse", "shifted", "hardcore4", "rough4"}
    obstacles = 0
    for i in range(TB.CTL_TABLE):
        (pa, xa, oa), (pb, xb, ob) = TB.terrain_facts(names[i]), TB.terrain_facts(names[TB.CTL_TABLE + i])
        assert abs(pa - pb) > 0.1 * min(pa, pb) and abs(xa - xb) >= 3.0, (i, names[i], names[TB.CTL_TABLE + i])
        obstacles += (oa != ob)
    assert obstacles >= 6 and TB.terrain_facts("hardcore4")[2] > 20
    # a cast against world i's terrain instead of world 16 + i's own changes at least one ray for at least 90 % of the creatures
    rays = TB.sense_rays()
    assert rays.shape == (23, 2)
    changed = total = 0
    for i in range(TB.CTL_TABLE):
        own, other = R.Terrain.of(TB.terrain(TB.CTL_TABLE + i)), R.Terrain.of(TB.terrain(i))
        px, py = TB.roots(TB.CTL_TABLE + i)
        a, b = R.cast(own, px, py, rays), R.cast(other, px, py, rays)
        assert (a[1] >= 0).any(axis=1).mean() >= 0.9, i                     # (and on its own terrain a creature's rays end somewhere)
        changed += int(((a[0] != b[0]) | (a[1] != b[1])).any(axis=1).sum())
        total += len(px)
    assert changed >= 0.9 * total, (changed, total)
    # ... and so does a cast against the terrain of the chunk's own first world (a SenseTable read at `i` instead of `first + i`
    # gives world 16 the terrain of world 0)
    for i in (TB.CTL_TABLE, 2 * TB.CTL_TABLE):
        px, py = TB.roots(i)
        a, b = R.cast(R.Terrain.of(TB.terrain(i)), px, py, rays), R.cast(R.Terrain.of(TB.terrain(0)), px, py, rays)
        assert ((a[0] != b[0]) | (a[1] != b[1])).any(axis=1).all(), i


def test_the_population_index():
    rows, n_rows = TB.index()
    assert n_rows == TB.n_creatures() == sum(w[1] for w in TB.WORLDS)
    assert [len(r) for r in rows] == [w[1] for w in TB.WORLDS] and all(r.dtype == np.int32 for r in rows)
    flat = np.concatenate(rows)
    assert np.array_equal(np.sort(flat), np.arange(n_rows)) and not np.array_equal(flat, np.arange(n_rows))
    assert all((np.diff(r) < 0).any() and (np.diff(r) > 0).any() for r in rows if len(r) > 2)        # scattered inside a world too
    short, n_short = TB.index(short=True)
    assert n_short == n_rows - TB.SHORT_BY
    differ = [(w, e) for w in range(TB.N_WORLDS) for e in np.flatnonzero(short[w] != rows[w])]
    assert differ == sorted((w, e) for w, e, _ in TB.OUT_OF_RANGE)
    bad = {w: int(short[w][e]) for w, e, _ in TB.OUT_OF_RANGE}
    assert sum(v < 0 for v in bad.values()) == 2 and sum(v >= n_short for v in bad.values()) == 2
    for table in (TB.CTL_TABLE, TB.STREAM_TABLE):          # out of range on either side of either split
        assert any(w < table for w in bad) and any(table <= w < 2 * table + 1 for w in bad)
    # ... and the creatures whose own row lies beyond n_rows are spread over many worlds
    assert len({w for w in range(TB.N_WORLDS) if (rows[w] >= n_short).any()}) >= 4


# ------------------------------------------------------------------------------------------------------------- the builders
def _fabricated(Np, K, slots, rng):
    """an arena of random bytes with five lane fields of 8 bytes, one of 4, a slot field and two per-creature fields, gaps between"""
    places, at = {}, 64
    for name, cnt, esz in (("camp", Np * K, 8), ("cphase", Np * K, 8), ("cfreq", Np * K, 8), ("coffset", Np * K, 8), ("cistate", Np * K, 8),
                           ("px", Np * K, 4), ("cinfo", Np * K * slots, 4), ("frozen", Np, 4), ("wod", Np, 8)):
        places[name] = (at, cnt, esz)
        at += cnt * esz + 40
    return rng.integers(0, 256, at, dtype=np.uint8), places


def test_expected_control_on_fabricated_bytes():
    rng = np.random.default_rng(5)
    Np, K, n, MB, n_rows = 8, 8, 6, 5, 7
    before, places = _fabricated(Np, K, 3, rng)
    live = np.zeros((n, K), bool)
    parent = np.full((n, K), -1)
    # creature 0: lanes 0 2 3 5 (bodies 0 1 2 3), lane 3 without a parent; creature 1: seven bodies (5 and 6 beyond MB); 2: a lone root
    live[0, [0, 2, 3, 5]] = True
    parent[0, [2, 5]] = 0
    live[1, :7] = True
    parent[1, 1:7] = np.arange(6)
    live[2, 0] = True
    live[3, :3] = live[4, :3] = live[5, :3] = True
    parent[3, 1:3] = parent[4, 1:3] = parent[5, 1:3] = 0
    rows = np.array([4, 0, 2, -1, 7, 6])                   # creature 3: negative; creature 4: n_rows
    values = rng.standard_normal((n_rows, MB))
    exp, wrote = TB.expected_control(before, places, Np, K, live, parent, rows, n_rows, TB.CTRL_TARGET, values, None, MB)
    want = {(0, 2): (4, 1), (0, 5): (4, 3), (1, 1): (0, 1), (1, 2): (0, 2), (1, 3): (0, 3), (1, 4): (0, 4), (5, 1): (6, 1), (5, 2): (6, 2)}
    assert wrote == len(want)

    def f64(a, name):
        off, cnt, _ = places[name]
        return a[off:off + cnt * 8].view(np.float64).reshape(Np, K)
    changed = np.zeros(len(before), bool)
    for (e, lane), (r, b) in want.items():
        assert f64(exp, "camp")[e, lane] == 0.0 and f64(exp, "coffset")[e, lane] == values[r, b]
        for name in ("camp", "coffset"):
            at = places[name][0] + 8 * (e * K + lane)
            changed[at:at + 8] = True
    assert np.array_equal(exp[~changed], before[~changed])                                     # nothing else moved by a byte
    # a mask takes pairs away; CTRL_PARAMS writes four words
    mask = np.ones((n_rows, MB), np.uint8)
    mask[4, 3] = mask[0, 2] = 0
    params = rng.standard_normal((n_rows, MB, 4))
    exp2, wrote2 = TB.expected_control(before, places, Np, K, live, parent, rows, n_rows, TB.CTRL_PARAMS, params, mask, MB)
    assert wrote2 == len(want) - 2
    for (e, lane), (r, b) in want.items():
        for q, name in enumerate(("camp", "cphase", "cfreq", "coffset")):
            word = f64(before, name)[e, lane] if (r, b) in ((4, 3), (0, 2)) else params[r, b, q]
            assert f64(exp2, name).view(np.uint64)[e, lane] == np.float64(word).view(np.uint64)
    assert np.array_equal(f64(exp2, "cistate").view(np.uint64), f64(before, "cistate").view(np.uint64))
    assert int((exp2 != before).sum()) > 0 and TB.expected_control(before, places, Np, K, live, parent, rows, 0, 0, values, None, MB)[1] == 0
    # max_bodies 1: no joint has a column
    assert TB.expected_control(before, places, Np, K, live, parent, rows, n_rows, 0, values[:, :1], None, 1)[1] == 0


def test_expected_refill_on_fabricated_bytes():
    rng = np.random.default_rng(6)
    Np, K, slots = 8, 4, 3
    before, places = _fabricated(Np, K, slots, rng)
    fresh = rng.integers(0, 256, len(before), dtype=np.uint8)
    took, retired = np.zeros(6, bool), np.zeros(6, bool)
    took[[1, 4]] = True
    retired[[0, 5]] = True
    exp = TB.expected_refill(before, fresh, places, Np, K, slots, took, retired)
    src = np.zeros(len(before), np.int8)                       # 0: before, 1: fresh, 2: the frozen word of a retired creature
    for name, (off, cnt, esz) in places.items():
        per = cnt // Np
        for e in (1, 4):
            if per == 1:
                src[off + e * esz:off + (e + 1) * esz] = 1
            elif per == K:
                src[off + e * K * esz:off + (e + 1) * K * esz] = 1
            else:
                for s in range(slots):
                    lo = off + (s * Np * K + e * K) * esz
                    src[lo:lo + K * esz] = 1
    off = places["frozen"][0]
    for e in (0, 5):
        src[off + 4 * e:off + 4 * e + 4] = 2
    assert np.array_equal(exp[src == 0], before[src == 0]) and np.array_equal(exp[src == 1], fresh[src == 1])
    assert (exp[off:off + 4 * Np].view(np.int32)[[0, 5]] == 1).all()
    assert (src == 1).sum() == 2 * (5 * K * 8 + K * 4 + slots * K * 4 + 4 + 8) and (src == 2).sum() == 8
    none = TB.expected_refill(before, fresh, places, Np, K, slots, np.zeros(6, bool), np.zeros(6, bool))
    assert np.array_equal(none, before)
