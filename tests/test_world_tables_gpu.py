"""The world-table calls across their launch split on a real MI355X (pytest -m gpu): rem2d_worlds_observe, _control, _sense, _act,
_act_recurrent, _describe and _refill with MORE worlds than one kernel-argument table holds (CTL_TABLE = 16; STREAM_TABLE = 8 for
refill), on the forged list of tests/table_forge.py (its docstring states what the list guarantees; tests/test_world_tables_host.py
asserts it).  rem2d_worlds_reset_where crosses its split in tests/test_episodes_gpu.py.

The reference is always the numpy model of the call -- control_model.observe_model, range_model.cast, policy_model.forward_model,
recurrent_model.forward_model, novelty_model.describe_update, table_forge.expected_control / expected_refill -- applied to state read
back from the device (replay.read_state, lifecycle_forge.arena_bytes), never the library's own output, and every comparison is on
bits: there is no tolerance in this module.  Outputs sit between guard rows; rows nobody owns must keep their fill.

Matrix (default build unless stated):
  observe        16 / 17 / 32 / 33 worlds x max_bodies 1, 5, 64 x {full index, short index};  17 worlds also wide and fma
  control        16 / 17 / 32 / 33 worlds x {target, target + mask, params, params + mask};     17 worlds also wide and fma
  sense          16 / 17 / 32 / 33 worlds x 23 rays x {full, short}, hit_dev given and NULL;    17 worlds also wide and fma
  act            16 / 17 / 32 / 33 worlds, {full, short}: obs, frac, targets, valid, the arenas' controller words
  act_recurrent  the same, plus the memory words, under a reset mask that selects creatures of both chunks
  describe       16 / 17 / 32 / 33 worlds, three calls at forged step words, a third of the creatures frozen
  refill         8 / 9 / 16 / 17 worlds, test_stream_gpu's forged-occupant protocol; worlds 7 + 8 and 15 + 16 share a feed and cursor
                 that runs short in the second of the two launches
  act_normed     17 / 33 worlds x {feed-forward, with memory under such a reset mask}, accumulate = 1, a normaliser of 64-row blocks
                 (they straddle worlds and chunks) frozen after one accumulation: the same buffers and the sums, against
                 obsnorm_model on top of the models above
  act launches   one act / act_recurrent / act_normed over 17 worlds captured into a graph: 7, 7 and 8 kernel nodes
  refusals       9 calls x {NULL world at 16, never-reset world at 17}, refill also a feed of other lanes at 9: the documented text,
                 and no byte of any arena or buffer moved (reset_where included: it shares the contract)
  chains         9 calls x two orders of a list of good / never reset / NULL / no terrain (refill: / feed of other lanes / static
                 tile shape) worlds, walked down fault by fault against tests/golden/world_call_refusals.json: code and text of
                 every link, nothing moved (the host half of the record: tests/test_world_calls_host.py)
  split transparency, inside each id: the n-world call and n one-world calls from the same state leave identical bytes.  For refill
                 the comparison is of what the header specifies (cursors, the ids handed out, how many slots a world refilled and
                 retired): WHICH pending creature lands in which slot of one launch is unspecified (csrc/rem2d_stream.h)
  facade         BatchedModular2D with five lane buckets and step_groups = 4 (17 worlds): 20 closed-loop steps under an MLPPolicy and
                 under a RecurrentPolicy against policy_model.policy_loop_run / recurrent_model.recurrent_loop_run; a streamed env
                 with step_groups = 4 (11 worlds: reset_stream cuts a bucket into a world per step group, and the worlds of a bucket
                 share its feed) through evaluate.run_stream against stream_model.run

60 ids.  Measured on one MI355X: the whole module in 9 s of wall time -- 1.6 s of it the set-up of the 33 worlds (reset and 40 steps
each), 1.4 s the streamed env, 0.8 s the slowest forge id (observe, 16 worlds, which also makes the cached models), 0.6 s the first
act_normed id, every other id below 0.6 s; the nine chain ids together take a fraction of a second.  What the two scratch mutants of the host loop fail is recorded in DESIGN.md section 14, "The world tables across their
launch split".
"""
import ctypes as C

import numpy as np
import pytest

import control_model as CM
import novelty_model as NM
import policy_model as PM
import range_model as R
import recurrent_model as RM
import state_forge as F
import table_forge as TB

pytestmark = pytest.mark.gpu

BUILDS = {"default": False, "wide": True, "fma": "fma"}
OTHER_BUILDS_N = TB.CTL_TABLE + 1
CASES = [(n, "default") for n in TB.CTL_COUNTS] + [(OTHER_BUILDS_N, "wide"), (OTHER_BUILDS_N, "fma")]
f32 = np.float32


def _cid(c):
    return "%d%s" % (c[0], "" if c[1] == "default" else "-" + c[1])


@pytest.fixture(scope="module")
def gpu():
    import replay
    return replay.need_gpu()


@pytest.fixture(scope="module")
def sets(gpu):
    """get(build) -> the build's WorldSet, restored and under the full index: all 33 worlds in the default build, 17 in the others"""
    made = {}

    def get(build="default"):
        if build not in made:
            made[build] = TB.WorldSet(gpu, TB.N_WORLDS if build == "default" else OTHER_BUILDS_N, BUILDS[build])
        s = made[build]
        s.restore()
        s.use_index(False)
        return s
    yield get
    for s in made.values():
        s.close()


# ------------------------------------------------------------------------------------------------------------------ the calls
def call(worlds, name, args, pre=()):
    """rem2d_worlds_<name>(worlds, [pre,] n, args..., stream) -> (return code, rem2d_last_error's text)"""
    w0 = next(w for w in worlds if w is not None)
    rc = getattr(w0.L, "rem2d_worlds_" + name)(TB.world_array(worlds), *pre, len(worlds), *args, w0._stream())
    return rc, (w0.L.rem2d_last_error().decode() if rc else "")


def ok(worlds, name, args, pre=()):
    rc, text = call(worlds, name, args, pre)
    assert rc == 0, "%s: %d %s" % (name, rc, text)


def ptr(t):
    return None if t is None else t.data_ptr()


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def one_by_one(worlds, name, args, pre_of=None):
    for i, w in enumerate(worlds):
        ok([w], name, args, () if pre_of is None else pre_of(i))


# ----------------------------------------------------------------------------------------------------------------- the models
def _cached(s, key, make):
    cache = s.__dict__.setdefault("_models", {})
    if key not in cache:
        cache[key] = make()
    return cache[key]


def ctxs(s):
    return _cached(s, "ctx", lambda: [F.Ctx(m) for m in s.morphs])


def model_obs(s, max_bodies):
    """observe_model of every world's state after the settle -> [float32 [n_i, width]]"""
    return _cached(s, ("obs", max_bodies), lambda: [CM.observe_model(c, st, max_bodies) for c, st in zip(ctxs(s), s.states())])


def model_cast(s, rays, key):
    """range_model.cast of every world's roots against ITS OWN terrain -> [(frac, hit)]"""
    return _cached(s, ("cast", key), lambda: [R.cast(R.Terrain.of(TB.terrain(i)), st["px"][:, 0], st["py"][:, 0], rays)
                                              for i, st in enumerate(s.states())])


def scatter(s, n, per_world, tail, fill, dtype):
    """what a call on the first n worlds leaves in a buffer of s.n_rows rows prefilled with `fill`: row rows[e] = per_world[i][e]"""
    out = np.full((s.n_rows,) + tuple(tail), fill, dtype)
    for i in range(n):
        r = s.rows[i]
        inside = (r >= 0) & (r < s.n_rows)
        out[r[inside]] = per_world[i][inside]
    return out


def same_rows(got, want, s, n, what):
    """bit for bit; a failure names the worlds whose rows differ"""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    g, w = got.reshape(len(got), -1), want.reshape(len(want), -1)
    bits = {4: np.uint32, 8: np.uint64, 1: np.uint8}[g.dtype.itemsize]
    bad = (np.ascontiguousarray(g).view(bits) != np.ascontiguousarray(w).view(bits)).any(axis=1)
    if bad.any():
        owner = np.full(len(got), -1)
        for i in range(len(s.rows)):
            r = s.rows[i]
            owner[r[(r >= 0) & (r < len(got))]] = i
        pytest.fail("%s: %d of %d rows differ, in worlds %s (-1: a row nobody in the call owns); first row %d: device %r model %r" % (
            what, int(bad.sum()), len(bad), sorted(set(owner[bad].tolist())), int(np.argmax(bad)), g[int(np.argmax(bad))][:12], w[int(np.argmax(bad))][:12]))


def same_arenas(got, want, what):
    assert len(got) == len(want)
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a.tobytes() != b.tobytes()]
    assert not bad, "%s: the arenas of worlds %s differ" % (what, bad)


def control_arenas(s, n, before, mode, values, mask, max_bodies):
    """table_forge.expected_control for the first n worlds; the others as they were -> ([arena], pairs written)"""
    out, wrote = [], 0
    for i, (w, st) in enumerate(zip(s.worlds, s.states())):
        if i >= n:
            out.append(before[i])
            continue
        exp, k = TB.expected_control(before[i], s.places[i], w.n_envs_padded, w.lanes, st["shape"] != 0, st["parent"], s.rows[i], s.n_rows,
                                     mode, values, mask, max_bodies)
        out.append(exp)
        wrote += k
    return out, wrote


# -------------------------------------------------------------------------------------------------------------------- observe
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_observe(gpu, sets, case):
    """every row of control_model.observe_model of the device's state, scattered through the index, for max_bodies 1, 5 and 64 (below,
    between and above the lane counts); rows beyond n_rows, of the two creatures pointed out of range and of the worlds not in the call
    keep their fill; no arena moves; one world at a time gives the same bytes"""
    torch = gpu
    n, build = case
    s = sets(build)
    before = s.arenas()
    compared = 0
    for short in (False, True):
        n_rows = s.use_index(short)
        for mb in (1, 5, TB.MAX_BODIES):
            buf = TB.Guarded(torch, (n_rows, CM.width(mb)), torch.float32, 7.5)
            ok(s.worlds[:n], "observe", (mb, ptr(buf.inner), n_rows))
            got = buf.host()
            want = scatter(s, n, model_obs(s, mb), (CM.width(mb),), 7.5, f32)
            same_rows(got, want, s, n, "observe, %d worlds, max_bodies %d%s" % (n, mb, ", short index" if short else ""))
            compared += int((want[:, 7] != 7.5).sum())
            single = TB.Guarded(torch, (n_rows, CM.width(mb)), torch.float32, 7.5)
            one_by_one(s.worlds[:n], "observe", (mb, ptr(single.inner), n_rows))
            assert single.host().tobytes() == got.tobytes(), "observe: %d one-world calls differ from the %d-world call" % (n, n)
    assert compared >= 6 * (TB.n_creatures(n) - TB.SHORT_BY - 4)
    same_arenas(s.arenas(), before, "observe")
    st = s.states()
    assert sum(int((x["ccount"] > 0).sum()) for x in st[:n]) > 100 and sum(int((x["jlimit"] != 0).sum()) for x in st[:n]) > 0
    assert all((x["steps"] == TB.SETTLE).all() for x in st[:n]) and sum(int((x["wod"] > 0).sum()) for x in st[:n]) > 100


# -------------------------------------------------------------------------------------------------------------------- control
CONTROL_FORMS = ((TB.CTRL_TARGET, False, 64, False), (TB.CTRL_TARGET, True, 5, True), (TB.CTRL_PARAMS, False, 16, True),
                 (TB.CTRL_PARAMS, True, 64, False))


@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_control(gpu, sets, case):
    """both modes, with and without a mask (mode, mask, max_bodies, short index: CONTROL_FORMS): every arena afterwards is the arena
    before with exactly the controller words of the selected (creature, body) pairs replaced -- padding lanes, alignment gaps and the
    worlds that were not in the call included -- and one world at a time gives the same bytes"""
    torch = gpu
    n, build = case
    s = sets(build)
    rng = np.random.default_rng(40 + n)
    for mode, masked, mb, short in CONTROL_FORMS:
        s.restore()
        n_rows = s.use_index(short)
        before = s.arenas()
        values = rng.uniform(-1.3, 1.3, (n_rows, mb) + ((4,) if mode == TB.CTRL_PARAMS else ()))
        mask = (rng.random((n_rows, mb)) < 0.6).astype(np.uint8) if masked else None
        vd, md = dev(torch, values), (dev(torch, mask) if masked else None)
        ok(s.worlds[:n], "control", (mode, ptr(vd), mb, n_rows, ptr(md)))
        after = s.arenas()
        want, wrote = control_arenas(s, n, before, mode, values, mask, mb)
        same_arenas(after, want, "control mode %d, mask %s, max_bodies %d, %d worlds" % (mode, masked, mb, n))
        assert wrote > (40 if mb == 5 else 150) and sum(int((a != b).sum()) for a, b in zip(after, before)) > 4 * wrote
        s.restore()
        one_by_one(s.worlds[:n], "control", (mode, ptr(vd), mb, n_rows, ptr(md)))
        same_arenas(s.arenas(), after, "control: one world at a time")


# ---------------------------------------------------------------------------------------------------------------------- sense
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_sense(gpu, sets, case):
    """frac and hit of range_model.cast on each world's OWN terrain (world 16 + i stands on another one than world i: pitch, x0,
    obstacle list), 23 rays; hit_dev NULL gives the same fractions; no arena moves; one world at a time gives the same bytes"""
    torch = gpu
    n, build = case
    s = sets(build)
    rays = TB.sense_rays()
    rd = dev(torch, rays)
    before = s.arenas()
    model = model_cast(s, rays, "23")
    for short in (False, True):
        n_rows = s.use_index(short)
        bufs = []
        for k in range(3):         # the n-world call, the same without hit_dev, one world at a time
            frac = TB.Guarded(torch, (n_rows, len(rays)), torch.float32, 7.5)
            hit = None if k == 1 else TB.Guarded(torch, (n_rows, len(rays)), torch.int32, -7)
            args = (ptr(rd), len(rays), ptr(frac.inner), None if hit is None else ptr(hit.inner), n_rows)
            if k < 2:
                ok(s.worlds[:n], "sense", args)
            else:
                one_by_one(s.worlds[:n], "sense", args)
            bufs.append((frac.host(), None if hit is None else hit.host()))
        want_f = scatter(s, n, [m[0] for m in model], (len(rays),), 7.5, f32)
        want_h = scatter(s, n, [m[1] for m in model], (len(rays),), -7, np.int32)
        what = "sense, %d worlds%s" % (n, ", short index" if short else "")
        same_rows(bufs[0][0], want_f, s, n, what + ": frac")
        same_rows(bufs[0][1], want_h, s, n, what + ": hit")
        assert bufs[1][0].tobytes() == bufs[0][0].tobytes(), what + ": hit_dev NULL"
        assert bufs[2][0].tobytes() == bufs[0][0].tobytes() and bufs[2][1].tobytes() == bufs[0][1].tobytes(), what + ": one world at a time"
    hits = np.concatenate([m[1] for m in model[:n]])
    assert (hits >= 0).mean() > 0.3 and (hits < 0).mean() > 0.1
    same_arenas(s.arenas(), before, "sense")


# -------------------------------------------------------------------------------------------------- act and act_recurrent
ACT_BODIES, ACT_HIDDEN, ACT_CONTEXT = 16, 32, 8
FILL = dict(obs=0.25, frac=1.0, targets=-3.0, valid=9, memory=0.5)


def act_buffers(torch, n_rows, recurrent):
    b = dict(obs=TB.Guarded(torch, (n_rows, CM.width(ACT_BODIES)), torch.float32, FILL["obs"]),
             frac=TB.Guarded(torch, (n_rows, 10), torch.float32, FILL["frac"]),
             targets=TB.Guarded(torch, (n_rows, ACT_BODIES), torch.float64, FILL["targets"]),
             valid=TB.Guarded(torch, (n_rows, ACT_BODIES), torch.uint8, FILL["valid"]))
    if recurrent:
        b["memory"] = TB.Guarded(torch, (n_rows, ACT_CONTEXT), torch.float32, FILL["memory"])
    return b


def run_act(torch, s, n, pol, rays, recurrent, mem0, reset, single, owned=False):
    """the call on the first n worlds of a restored set (or n one-world calls) -> ({name: host rows}, [arena]).  owned: under a row
    mask of the rows the call's worlds own -- one call's forward pass then leaves every other row, its context words included, alone"""
    b = act_buffers(torch, s.n_rows, recurrent)
    name = "act_recurrent" if recurrent else "act"
    keep = [dev(torch, reset)] if recurrent else []
    if recurrent:
        b["memory"].inner.copy_(dev(torch, mem0))

    def desc(worlds):
        mask = None
        if owned:
            own = np.zeros(s.n_rows, np.uint8)
            for i in worlds:
                r = s.rows[i]
                own[r[(r >= 0) & (r < s.n_rows)]] = 1
            mask = dev(torch, own)
            keep.append(mask)
        bufs = (b["obs"].inner, b["frac"].inner, b["targets"].inner, b["valid"].inner)
        return pol.descriptor(*bufs, b["memory"].inner, keep[0], mask) if recurrent else pol.descriptor(*bufs, mask)
    if single:
        for i in range(n):
            ok([s.worlds[i]], name, (C.byref(desc([i])), ptr(rays)))
    else:
        ok(s.worlds[:n], name, (C.byref(desc(range(n))), ptr(rays)))
    return {k: v.host() for k, v in b.items()}, s.arenas()


@pytest.mark.parametrize("recurrent", [False, True], ids=["act", "act_recurrent"])
@pytest.mark.parametrize("n", TB.CTL_COUNTS)
def test_act(gpu, sets, n, recurrent):
    """the composition observe_model -> cast -> forward_model -> the control write, per creature under its own weight set: obs, frac,
    targets, valid, (memory,) and every arena's controller words.  The forward pass runs over every row, so a row nobody in the call
    owns is the model's on the buffers' fill.  The recurrent call's reset mask selects creatures of both chunks."""
    torch = gpu
    from gym_rem2d_amd import policy
    s = sets()
    rays = dev(torch, R.bipedal_rays())
    cast = model_cast(s, R.bipedal_rays(), "10")
    for short in (False, True):
        s.restore()
        n_rows = s.use_index(short)
        before = s.arenas()
        rng = np.random.default_rng(60 + n)
        mem0 = reset = None
        if recurrent:
            pol = policy.RecurrentPolicy.random(n_rows, ACT_BODIES, ACT_HIDDEN, ACT_CONTEXT, seed=71 + n).to("cuda")
            mem0 = rng.uniform(-0.9, 0.9, (n_rows, ACT_CONTEXT)).astype(f32)
            reset = (rng.random(n_rows) < 0.3).astype(np.uint8)
            for i in (1, 4, n - 1):                             # creatures of the first and of the last chunk, for certain
                r = s.rows[i]
                reset[r[(r >= 0) & (r < n_rows)][:2]] = 1
            picked = [int(reset[r[(r >= 0) & (r < n_rows)]].sum()) for r in s.rows[:n]]
            assert sum(picked[:TB.CTL_TABLE]) >= 4 and (n == TB.CTL_TABLE or sum(picked[TB.CTL_TABLE:]) >= 2)
        else:
            pol = policy.MLPPolicy.random(n_rows, ACT_BODIES, ACT_HIDDEN, seed=71 + n).to("cuda")
        W = tuple(t.cpu().numpy() for t in pol.weights)
        got, after = run_act(torch, s, n, pol, rays, recurrent, mem0, reset, False)
        obs = scatter(s, n, model_obs(s, ACT_BODIES), (CM.width(ACT_BODIES),), FILL["obs"], f32)
        frac = scatter(s, n, [m[0] for m in cast], (10,), FILL["frac"], f32)
        x = PM.input_rows(obs, frac)
        if recurrent:
            tg, valid, mem = RM.forward_model(x, mem0, *W, reset=reset)
        else:
            tg, valid = PM.forward_model(x, *W)
        what = "%s, %d worlds%s" % ("act_recurrent" if recurrent else "act", n, ", short index" if short else "")
        same_rows(got["obs"], obs, s, n, what + ": obs")
        same_rows(got["frac"], frac, s, n, what + ": frac")
        same_rows(PM.bits(got["targets"]), PM.bits(tg), s, n, what + ": targets")
        same_rows(got["valid"], valid, s, n, what + ": valid")
        if recurrent:
            same_rows(RM.mem_bits(got["memory"]), RM.mem_bits(mem), s, n, what + ": memory")
            carried = RM.forward_model(x, mem0, *W)[2]
            assert (RM.mem_bits(carried)[reset != 0] != RM.mem_bits(mem)[reset != 0]).any(axis=1).all()      # the mask mattered
        want, wrote = control_arenas(s, n, before, TB.CTRL_TARGET, tg, valid, ACT_BODIES)
        same_arenas(after, want, what + ": the arenas")
        assert wrote > 150 and valid.all()
        # one world at a time.  A call's forward pass runs over every row, which the feed-forward policy may do any number of times;
        # a recurrent one would advance its context n times, so both sides of its comparison run under a row mask of the rows their
        # worlds own
        s.restore()
        many = run_act(torch, s, n, pol, rays, recurrent, mem0, reset, False, owned=True) if recurrent else (got, after)
        s.restore()
        got1, after1 = run_act(torch, s, n, pol, rays, recurrent, mem0, reset, True, owned=recurrent)
        assert all(got1[k].tobytes() == many[0][k].tobytes() for k in got), what + ": one world at a time"
        same_arenas(after1, many[1], what + ": one world at a time")
        if recurrent:       # under the mask the rows the call's worlds own are the unmasked call's, every other row kept its fill
            own = scatter(s, n, [np.ones(len(r), np.uint8) for r in s.rows], (), 0, np.uint8) != 0
            assert all(many[0][k][own].tobytes() == got[k][own].tobytes() for k in got) and own.sum() > 200
            assert all((many[0][k][~own] == np.asarray(FILL[k], many[0][k].dtype)).all() for k in ("targets", "valid", "obs", "frac"))
            assert many[0]["memory"][~own].tobytes() == mem0[~own].tobytes()
            same_arenas(many[1], after, what + ": under a row mask")


# ----------------------------------------------------------------------------------------------------------------- act_normed
NORM_GROUP = 64


def normed_call(worlds, nd, p, rays, accumulate):
    """rem2d_worlds_act_normed(worlds, n, &nd, &p, rays, accumulate) on the current stream, which travels in nd -> (code, text)"""
    w0 = next(w for w in worlds if w is not None)
    nd.stream = w0._stream()
    rc = w0.L.rem2d_worlds_act_normed(TB.world_array(worlds), len(worlds), C.byref(nd), C.byref(p), ptr(rays), accumulate)
    return rc, (w0.L.rem2d_last_error().decode() if rc else "")


def run_act_normed(torch, s, n, pol, norm, sums0, rays, memory, mem0, reset, single, owned=False):
    """test_act's run_act for rem2d_worlds_act_normed with accumulate = 1, from the sums `sums0`
    -> ({name: host rows}, [count, s1, s2hi, s2lo], [arena])"""
    import test_obsnorm_gpu as TO
    b = act_buffers(torch, s.n_rows, memory)
    for name, a in zip(("count", "s1", "s2hi", "s2lo"), sums0):
        getattr(norm, name).copy_(dev(torch, a))
    keep = [dev(torch, reset)] if memory else []
    if memory:
        b["memory"].inner.copy_(dev(torch, mem0))

    def one(worlds):
        mask = None
        if owned:
            own = np.zeros(s.n_rows, np.uint8)
            for i in worlds:
                r = s.rows[i]
                own[r[(r >= 0) & (r < s.n_rows)]] = 1
            mask = dev(torch, own)
            keep.append(mask)
        bufs = (b["obs"].inner, b["frac"].inner, b["targets"].inner, b["valid"].inner)
        nd = norm.descriptor()
        if memory:
            q = pol.descriptor(*bufs, b["memory"].inner, keep[0], mask)
            nd.context, nd.memory, nd.reset, p = q.context, q.memory, q.reset, q.p
        else:
            p = pol.descriptor(*bufs, mask)
        rc, text = normed_call([s.worlds[i] for i in worlds], nd, p, rays, 1)
        assert rc == 0, "act_normed: %d %s" % (rc, text)
    if single:
        for i in range(n):
            one([i])
    else:
        one(range(n))
    return {k: v.host() for k, v in b.items()}, TO.get_state(norm), s.arenas()


@pytest.mark.parametrize("memory", [False, True], ids=["feed_forward", "memory"])
@pytest.mark.parametrize("n", (TB.CTL_TABLE + 1, 2 * TB.CTL_TABLE + 1))
def test_act_normed(gpu, sets, n, memory):
    """test_act for rem2d_worlds_act_normed, accumulate = 1, feed-forward and with memory under a reset mask that selects creatures of
    both chunks.  The normaliser's blocks are 64 rows, so they straddle worlds and chunks, and its tables were frozen after one
    accumulation of forged rows, so every block has its own.  obs, frac, targets, valid, (memory,) the sums and the arenas against
    observe_model -> cast -> obsnorm_model.accumulate / forward(_memory) -> the control write; then, both under a row mask of the
    rows their worlds own, one call against one world at a time (the sums are exact, so n masked calls add up to the one)."""
    torch = gpu
    import obsnorm_model as OM
    import test_obsnorm_gpu as TO
    from gym_rem2d_amd import policy
    s = sets()
    rays = dev(torch, R.bipedal_rays())
    cast = model_cast(s, R.bipedal_rays(), "10")
    for short in (False, True):
        s.restore()
        n_rows = s.use_index(short)
        before = s.arenas()
        rng = np.random.default_rng(160 + n)
        mem0 = reset = None
        if memory:
            pol = policy.RecurrentPolicy.random(n_rows, ACT_BODIES, ACT_HIDDEN, ACT_CONTEXT, seed=171 + n).to("cuda")
            mem0 = rng.uniform(-0.9, 0.9, (n_rows, ACT_CONTEXT)).astype(f32)
            reset = (rng.random(n_rows) < 0.3).astype(np.uint8)
            for i in (1, 4, n - 1):
                r = s.rows[i]
                reset[r[(r >= 0) & (r < n_rows)][:2]] = 1
            picked = [int(reset[r[(r >= 0) & (r < n_rows)]].sum()) for r in s.rows[:n]]
            assert sum(picked[:TB.CTL_TABLE]) >= 4 and sum(picked[TB.CTL_TABLE:]) >= 2
        else:
            pol = policy.MLPPolicy.random(n_rows, ACT_BODIES, ACT_HIDDEN, seed=171 + n).to("cuda")
        W = tuple(t.cpu().numpy() for t in pol.weights)
        norm = policy.ObsNormalizer(-(-n_rows // NORM_GROUP), NORM_GROUP, ACT_BODIES, 10, min_count=2, device="cuda")
        prior = (rng.standard_normal((n_rows, norm.width)) * np.linspace(0.2, 3.0, norm.n_blocks).repeat(NORM_GROUP)[:n_rows, None]).astype(f32)
        norm.accumulate(*TO.split(torch, prior, ACT_BODIES))
        norm.freeze()
        sums0 = TO.get_state(norm)
        mu, inv = (t.cpu().numpy().copy() for t in norm.tables)
        assert len({mu[b].tobytes() for b in range(norm.n_blocks)}) == norm.n_blocks > 4 and (inv != 1).all()
        got, sums, after = run_act_normed(torch, s, n, pol, norm, sums0, rays, memory, mem0, reset, False)
        obs = scatter(s, n, model_obs(s, ACT_BODIES), (CM.width(ACT_BODIES),), FILL["obs"], f32)
        frac = scatter(s, n, [m[0] for m in cast], (10,), FILL["frac"], f32)
        x = PM.input_rows(obs, frac)
        if memory:
            tg, valid, mem = OM.forward_memory(x, mem0, mu, inv, norm.clip, NORM_GROUP, *W, reset=reset)
        else:
            tg, valid = OM.forward(x, mu, inv, norm.clip, NORM_GROUP, *W)
        what = "act_normed%s, %d worlds%s" % (" with memory" if memory else "", n, ", short index" if short else "")
        same_rows(got["obs"], obs, s, n, what + ": obs")
        same_rows(got["frac"], frac, s, n, what + ": frac")
        same_rows(PM.bits(got["targets"]), PM.bits(tg), s, n, what + ": targets")
        same_rows(got["valid"], valid, s, n, what + ": valid")
        if memory:
            same_rows(RM.mem_bits(got["memory"]), RM.mem_bits(mem), s, n, what + ": memory")
        st = OM.State(norm.n_blocks, norm.width)
        st.count, st.s1, st.s2hi, st.s2lo = (a.copy() for a in sums0)
        OM.accumulate(st, x, NORM_GROUP)
        for name, g, w in zip(("count", "s1", "s2hi", "s2lo"), sums, st.words()):
            assert np.array_equal(g, w.reshape(g.shape)), "%s: `%s`" % (what, name)
        assert (sums[0] > sums0[0]).all()
        assert np.array_equal(OM.tbits(norm.mu.cpu().numpy()), OM.tbits(mu)) and np.array_equal(OM.tbits(norm.inv.cpu().numpy()), OM.tbits(inv))
        want, wrote = control_arenas(s, n, before, TB.CTRL_TARGET, tg, valid, ACT_BODIES)
        same_arenas(after, want, what + ": the arenas")
        assert wrote > 150 and valid.all()
        plain = (RM.forward_model(x, mem0, *W, reset=reset) if memory else PM.forward_model(x, *W))[0]
        assert (PM.bits(plain) != PM.bits(tg)).any(axis=1).mean() > 0.9                                  # the tables mattered
        # one world at a time, both sides under a row mask of the rows their worlds own
        s.restore()
        many = run_act_normed(torch, s, n, pol, norm, sums0, rays, memory, mem0, reset, False, owned=True)
        s.restore()
        ones = run_act_normed(torch, s, n, pol, norm, sums0, rays, memory, mem0, reset, True, owned=True)
        assert all(ones[0][k].tobytes() == many[0][k].tobytes() for k in got), what + ": one world at a time"
        assert all(a.tobytes() == b.tobytes() for a, b in zip(ones[1], many[1])), what + ": the sums, one world at a time"
        same_arenas(ones[2], many[2], what + ": one world at a time")
        own = scatter(s, n, [np.ones(len(r), np.uint8) for r in s.rows], (), 0, np.uint8) != 0
        assert all(many[0][k][own].tobytes() == got[k][own].tobytes() for k in got) and own.sum() > 200
        assert int((many[1][0] - sums0[0]).sum()) == int(own.sum())
        same_arenas(many[2], after, what + ": under a row mask")


# ------------------------------------------------------------------------------------------- the launches of one act call
def captured_nodes(torch, queue):
    """queue(stream) captured on a side stream through the process's own HIP runtime -> the node count of the graph; nothing runs"""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = C.CDLL(path)
    side = torch.cuda.Stream()
    st, graph, count = C.c_void_p(side.cuda_stream), C.c_void_p(), C.c_size_t()
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(st, 2) == 0                # hipStreamCaptureModeRelaxed: the mode is of no concern here
    try:
        with torch.cuda.stream(side):
            queue()
    finally:
        assert hip.hipStreamEndCapture(st, C.byref(graph)) == 0
    try:
        assert hip.hipGraphGetNodes(graph, None, C.byref(count)) == 0
    finally:
        hip.hipGraphDestroy(graph)
    return count.value


def test_act_launches(gpu, sets):
    """one act call over 17 worlds, captured: observe and sense, the forward pass and control are 2 + 2 + 1 + 2 kernel nodes -- a
    launch per table of 16 worlds and call, one forward pass -- and the normalised call's accumulation is one more.  These are the
    counts of the library as it was when every act call went through the public observe / sense / control; no buffer is written."""
    torch = gpu
    from gym_rem2d_amd import policy
    s = sets()
    n, n_rows = TB.CTL_TABLE + 1, s.n_rows
    rays = dev(torch, R.bipedal_rays())
    arenas = s.arenas()
    for name, nodes in (("act", 7), ("act_recurrent", 7), ("act_normed", 8)):
        rec = name == "act_recurrent"
        b = act_buffers(torch, n_rows, rec)
        bufs = (b["obs"].inner, b["frac"].inner, b["targets"].inner, b["valid"].inner)
        if rec:
            pol = policy.RecurrentPolicy.random(n_rows, ACT_BODIES, ACT_HIDDEN, ACT_CONTEXT, seed=5).to("cuda")
            desc = pol.descriptor(*bufs, b["memory"].inner)
        else:
            pol = policy.MLPPolicy.random(n_rows, ACT_BODIES, ACT_HIDDEN, seed=5).to("cuda")
            desc = pol.descriptor(*bufs)
        norm = policy.ObsNormalizer(-(-n_rows // NORM_GROUP), NORM_GROUP, ACT_BODIES, 10, device="cuda")
        held = [v.raw.clone() for v in b.values()]

        def queue():
            if name == "act_normed":
                rc, text = normed_call(s.worlds[:n], norm.descriptor(), desc, rays, 1)
            else:
                rc, text = call(s.worlds[:n], name, (C.byref(desc), ptr(rays)))
            assert rc == 0, text
        assert captured_nodes(torch, queue) == nodes, name
        torch.cuda.synchronize()
        assert all(torch.equal(v.raw, h) for v, h in zip(b.values(), held)) and int(norm.count.sum()) == 0
    same_arenas(s.arenas(), arenas, "captured act calls")


# ------------------------------------------------------------------------------------------------------------------- describe
@pytest.mark.parametrize("n", TB.CTL_COUNTS)
def test_describe(gpu, sets, n):
    """three calls of period 15 x 4 samples on forged step words (so that sample slots fill call by call) with a third of the
    creatures frozen, against novelty_model.describe_update on the words read back; NvTable carries env4, where `steps` and `frozen`
    live; no arena moves; one world at a time gives the same bytes"""
    torch = gpu
    from replay import read_state
    s = sets()
    period, samples = 15, 4
    rng = np.random.default_rng(80 + n)
    for short in (False, True):
        s.restore()
        n_rows = s.use_index(short)
        buf = TB.Guarded(torch, (n_rows, 2 * samples), torch.float32, -5.0)
        single = TB.Guarded(torch, (n_rows, 2 * samples), torch.float32, -5.0)
        want = np.full((n_rows, 2 * samples), -5.0, f32)
        wrote = kept = 0
        for k, top in enumerate((14, 40, 75)):
            for i, w in enumerate(s.worlds[:n]):
                w.view("steps").copy_(dev(torch, rng.integers(max(0, top - 30), top + 1, w.n_envs).astype(np.int32)))
                w.view("frozen").copy_(dev(torch, (rng.random(w.n_envs) < (0.33 if k else 0.1)).astype(np.int32)))
                w.view("px")[:, 0] += float(k)            # the creatures have moved between two calls
            before = s.arenas()
            ok(s.worlds[:n], "describe", (period, samples, ptr(buf.inner), n_rows))
            one_by_one(s.worlds[:n], "describe", (period, samples, ptr(single.inner), n_rows))
            same_arenas(s.arenas(), before, "describe")
            for i, w in enumerate(s.worlds[:n]):
                st = read_state(w)
                r = s.rows[i]
                inside = (r >= 0) & (r < n_rows)
                sub = want[r[inside]]
                was = sub.copy()
                NM.describe_update(sub, st["steps"][inside], st["frozen"][inside], st["px"][inside, 0], st["py"][inside, 0], period, samples)
                want[r[inside]] = sub
                wrote, kept = wrote + int((sub != was).sum()), kept + int((sub == was).sum())
            what = "describe, %d worlds, call %d%s" % (n, k, ", short index" if short else "")
            same_rows(buf.host(), want, s, n, what)
            assert single.host().tobytes() == buf.host().tobytes(), what + ": one world at a time"
        assert wrote > 1000 and kept > 1000 and (want[:, 0] != want[:, 2 * samples - 2]).sum() > 50     # slots filled at different calls


# --------------------------------------------------------------------------------------------------------------------- refill
N_IDS, LIMIT, OLD_ID0 = 6000, 1000, 3000
SHARED = {7: "a", 8: "a", 15: "b", 16: "b"}


def morph_struct(devs):
    from gym_rem2d_amd import _lib
    m = _lib.Morph()
    for k in _lib.MORPH_FIELDS:
        setattr(m, k, devs[k].data_ptr())
    return m


def forge_refill(torch, s, n):
    """test_stream_gpu's forged-occupant protocol on the first n worlds of a restored set: per world the first and the last creature
    and its whole first wavefront have ended (step word LIMIT + i), nobody of its second, 40 % of the rest; every fourth slot from
    the second on is empty (-1), half of those carry an ended step word all the same.  A world's feed is its own creatures in reverse
    order, under a cursor of its own -- but worlds 7 + 8 and 15 + 16 share a feed (both worlds' creatures) and its cursor, with two /
    one pending creatures more than the first world's ended slots: fewer than both worlds' ended slots, so the second launch draws the
    last ones and retires the rest."""
    from gym_rem2d_amd import _lib
    from gym_rem2d_amd.compiler import Morphology
    rng = np.random.default_rng(90)
    occ0 = np.full(s.n_rows, -1, np.int32)
    ended, keys = [], []
    for i, w in enumerate(s.worlds[:n]):
        nn, per = w.n_envs, TB.WAVE // w.lanes
        loc = rng.random(nn) < 0.4
        if nn > per:
            loc[:per] = True
        if nn > 2 * per:
            loc[per:2 * per] = False
        loc[0] = loc[nn - 1] = True
        empty = np.zeros(nn, bool)
        empty[np.arange(1, nn - 1)[::4]] = True
        forged = loc.copy()
        forged[np.flatnonzero(empty)[::2]] = True
        w.view("steps")[dev(torch, np.flatnonzero(forged))] = LIMIT + i
        w.view("frozen").zero_()                                     # (forged too: a retired slot must show as 0 -> 1)
        occ = OLD_ID0 + s.rows[i].astype(np.int32)
        occ[empty] = -1
        if i == 0:
            occ[nn - 1] = N_IDS + 5                                  # ended and refilled, but no row of `out` is its own
        occ0[s.rows[i]] = occ
        ended.append(loc & ~empty)
        keys.append(SHARED.get(i, i))
    order = list(dict.fromkeys(keys))
    cursors = torch.zeros(len(order), dtype=torch.int32, device="cuda")
    feeds, host, keep = {}, {}, []
    for j, key in enumerate(order):
        members = [i for i in range(n) if keys[i] == key]
        own = Morphology.concat([s.morphs[i] for i in members])
        pending = own.take(np.arange(own.n_envs)[::-1])
        n_ended = [int(ended[i].sum()) for i in members]
        if key in ("a", "b"):
            count = n_ended[0] + (2 if key == "a" else 1) if len(members) == 2 else n_ended[0] - 1
            assert 0 < count < sum(n_ended) and count <= pending.n_envs, (key, count, n_ended)
        else:
            count = pending.n_envs
        d = {f: dev(torch, pending.arrays[f]) for f in _lib.MORPH_FIELDS}
        d["id"] = torch.arange(100 * j, 100 * j + pending.n_envs, dtype=torch.int32, device="cuda")
        f = _lib.Feed()
        f.M, f.id, f.count, f.lanes, f.cursor = morph_struct(d), d["id"].data_ptr(), count, own.lanes, cursors[j:j + 1].data_ptr()
        feeds[key], host[key] = f, dict(pending=pending, count=count, id0=100 * j, slot=j, members=members, ended=sum(n_ended))
        keep.append(d)
    out = _lib.StreamOut()
    raw = dict(steps=TB.Guarded(torch, (N_IDS,), torch.int32, -77), finished=TB.Guarded(torch, (N_IDS,), torch.uint8, 0xA5))
    out.steps, out.finished = ptr(raw["steps"].inner), ptr(raw["finished"].inner)
    return dict(occ0=occ0, occupant=dev(torch, occ0), ended=ended, keys=keys, feeds=feeds, host=host, cursors=cursors, out=out, raw=raw,
                keep=keep)


def refill_args(s, n, fg, pick=None):
    """(pre, args) of the call on worlds `pick` (default: the first n)"""
    from gym_rem2d_amd import _lib
    pick = list(range(n)) if pick is None else pick
    morphs = (_lib.Morph * len(pick))(*[morph_struct(s.worlds[i]._morph_dev) for i in pick])
    feeds = (_lib.Feed * len(pick))(*[fg["feeds"][fg["keys"][i]] for i in pick])
    return (morphs,), (feeds, ptr(fg["occupant"]), _lib.WHEN["steps"], LIMIT, C.byref(fg["out"]), N_IDS, s.n_rows)


def check_refill(torch, s, n, fg, before, morph_before):
    """everything the header promises of the call, from `occupant` as the record -> per world (slots refilled, slots retired)"""
    from gym_rem2d_amd import _lib
    from gym_rem2d_amd.compiler import Morphology
    from gym_rem2d_amd.world import BatchedWorld
    import lifecycle_forge as LF
    occ1, cur = fg["occupant"].cpu().numpy(), fg["cursors"].cpu().numpy()
    after = s.arenas()
    handed = {key: [] for key in fg["host"]}
    counts, moved, changed = [], 0, 0
    for i, w in enumerate(s.worlds[:n]):
        h, r, ended = fg["host"][fg["keys"][i]], s.rows[i], fg["ended"][i]
        now = occ1[r]
        assert np.array_equal(now[~ended], fg["occ0"][r][~ended]), "world %d: the occupant of a slot that had not ended moved" % i
        took, retired = ended & (now >= 0), ended & (now < 0)
        q = now[took] - h["id0"]
        assert (now[retired] == -1).all() and (q >= 0).all() and (q < h["count"]).all(), "world %d" % i
        handed[fg["keys"][i]] += now[took].tolist()
        counts.append((int(took.sum()), int(retired.sum())))
        # the arena: a fresh world of the creatures now in the slots, never stepped; retired slots differ in `frozen` only
        pick = np.arange(w.n_envs)
        pick[took] = w.n_envs + q
        new = Morphology.concat([s.morphs[i], h["pending"]]).take(pick)
        fresh = BatchedWorld(w.n_envs, w.lanes, TB.CONT, wide=s.wide)
        try:
            fresh.set_terrain(TB.terrain(i))
            fresh.reset(new)
            fresh_bytes = LF.arena_bytes(fresh)
        finally:
            fresh.close()
        off, cnt, esz = s.places[i]["frozen"]
        assert not before[i][off:off + cnt * esz].view(np.int32)[np.flatnonzero(retired)].any()
        exp = TB.expected_refill(before[i], fresh_bytes, s.places[i], w.n_envs_padded, w.lanes, w.contact_slots, took, retired)
        assert after[i].tobytes() == exp.tobytes(), "world %d (%d lanes): the arena after refill" % (i, w.lanes)
        moved += int((exp != before[i]).sum())
        # the world's device morphology: the new occupants' words at the refilled slots, nothing else
        lanes = np.repeat(took, w.lanes)
        for f in _lib.MORPH_FIELDS:
            m_now = w._morph_dev[f].cpu().numpy()
            assert m_now.tobytes() == new.arrays[f].tobytes(), "world %d: device morphology `%s`" % (i, f)
            assert m_now[~lanes].tobytes() == morph_before[i][f][~lanes].tobytes()
            changed += int((m_now != morph_before[i][f]).sum())
    same_arenas(after[n:], before[n:], "refill: worlds that were not in the call")
    for key, h in fg["host"].items():
        assert cur[h["slot"]] == h["ended"], "feed %r: cursor %d for %d ended slots" % (key, cur[h["slot"]], h["ended"])
        want = list(range(h["id0"], h["id0"] + min(h["ended"], h["count"])))
        assert sorted(handed[key]) == want, "feed %r: ids lost or handed out twice" % (key,)
    assert moved > 1000 and changed > 100
    # the harvest: the ids that finished, between guards
    steps, fin = fg["raw"]["steps"].host(), fg["raw"]["finished"].host()
    done = np.zeros(N_IDS, bool)
    for i in range(n):
        ids = fg["occ0"][s.rows[i]][fg["ended"][i]]
        done[ids[ids < N_IDS]] = True
        assert (steps[ids[ids < N_IDS]] == LIMIT + i).all()
    assert (fin[done] == 1).all() and (fin[~done] == 0xA5).all() and (steps[~done] == -77).all()
    return counts, {key: sorted(v) for key, v in handed.items()}, cur.copy()


@pytest.mark.parametrize("n", TB.REFILL_COUNTS)
def test_refill(gpu, sets, n):
    """forge_refill's protocol, then check_refill: per feed the ids drawn are distinct, min(count, ended) in number, and the cursor
    ends at the number of ended slots -- for the two feeds shared across a launch boundary too; every refilled slot is a fresh world's
    bytes of the creature `occupant` names; retired slots differ in REM2D_F_FROZEN only; the device morphology changed at the refilled
    slots and nowhere else.  One world at a time hands out the same ids and refills and retires as many slots in every world."""
    torch = gpu
    s = sets()
    results = []
    for single in (False, True):
        s.restore()
        fg = forge_refill(torch, s, n)
        before = s.arenas()
        morph_before = [{k: v.cpu().numpy().copy() for k, v in w._morph_dev.items()} for w in s.worlds[:n]]
        if single:
            for i in range(n):
                pre, args = refill_args(s, n, fg, [i])
                ok([s.worlds[i]], "refill", args, pre)
        else:
            pre, args = refill_args(s, n, fg)
            ok(s.worlds[:n], "refill", args, pre)
        results.append(check_refill(torch, s, n, fg, before, morph_before))
    (counts, handed, cur), (counts1, handed1, cur1) = results
    assert counts == counts1 and handed == handed1 and np.array_equal(cur, cur1)
    for first, second in ((7, 8), (15, 16)):             # the shared feeds ran short in the second world
        if n > second:
            assert counts[first][1] == 0 and counts[second][0] == (2 if first == 7 else 1) and counts[second][1] > 0, (counts[first], counts[second])
        elif n > first:
            assert counts[first][1] == 1


# ------------------------------------------------------------------------------------------------------------------ refusals
REFUSED = ("observe", "control", "sense", "act", "act_recurrent", "act_normed", "describe", "reset_where", "refill")
N_REFUSED = TB.CTL_TABLE + 2


def refusal_call(torch, s, name):
    """-> (run(worlds, feed_lanes=None) -> (rc, text), [device tensors the call could write])"""
    from gym_rem2d_amd import _lib, policy
    n, n_rows = N_REFUSED, s.n_rows
    rays = dev(torch, R.bipedal_rays())
    if name == "observe":
        out = torch.full((n_rows, CM.width(16)), 7.5, dtype=torch.float32, device="cuda")
        return (lambda ws, _=None: call(ws, name, (16, ptr(out), n_rows))), [out]
    if name == "control":
        values = torch.full((n_rows, 16), 0.5, dtype=torch.float64, device="cuda")
        return (lambda ws, _=None: call(ws, name, (TB.CTRL_TARGET, ptr(values), 16, n_rows, None))), [values]
    if name == "sense":
        frac = torch.full((n_rows, 10), 7.5, dtype=torch.float32, device="cuda")
        hit = torch.full((n_rows, 10), -7, dtype=torch.int32, device="cuda")
        return (lambda ws, _=None: call(ws, name, (ptr(rays), 10, ptr(frac), ptr(hit), n_rows))), [frac, hit]
    if name in ("act", "act_recurrent"):
        rec = name == "act_recurrent"
        b = act_buffers(torch, n_rows, rec)
        if rec:
            pol = policy.RecurrentPolicy.random(n_rows, ACT_BODIES, ACT_HIDDEN, ACT_CONTEXT, seed=5).to("cuda")
            desc = pol.descriptor(b["obs"].inner, b["frac"].inner, b["targets"].inner, b["valid"].inner, b["memory"].inner)
        else:
            pol = policy.MLPPolicy.random(n_rows, ACT_BODIES, ACT_HIDDEN, seed=5).to("cuda")
            desc = pol.descriptor(b["obs"].inner, b["frac"].inner, b["targets"].inner, b["valid"].inner)
        return (lambda ws, _=None: call(ws, name, (C.byref(desc), ptr(rays)))), [v.raw for v in b.values()] + list(pol.weights)
    if name == "act_normed":
        b = act_buffers(torch, n_rows, False)
        pol = policy.MLPPolicy.random(n_rows, ACT_BODIES, ACT_HIDDEN, seed=5).to("cuda")
        norm = policy.ObsNormalizer(-(-n_rows // NORM_GROUP), NORM_GROUP, ACT_BODIES, 10, min_count=2, device="cuda")
        desc = pol.descriptor(b["obs"].inner, b["frac"].inner, b["targets"].inner, b["valid"].inner)
        return ((lambda ws, _=None: normed_call(ws, norm.descriptor(), desc, rays, 1)),
                [v.raw for v in b.values()] + list(pol.weights) + [norm.count, norm.s1, norm.s2hi, norm.s2lo, norm.mu, norm.inv])
    if name == "describe":
        out = torch.full((n_rows, 8), -5.0, dtype=torch.float32, device="cuda")
        return (lambda ws, _=None: call(ws, name, (15, 4, ptr(out), n_rows))), [out]
    some = s.worlds[0]._morph_dev

    def morphs_of(ws):
        return (_lib.Morph * len(ws))(*[morph_struct(some if w is None or w._morph_dev is None else w._morph_dev) for w in ws])
    if name == "reset_where":
        mask = torch.ones(n_rows, dtype=torch.uint8, device="cuda")
        ended = torch.full((n_rows,), 0xA5, dtype=torch.uint8, device="cuda")
        out = _lib.EpisodeOut()
        out.ended = ptr(ended)
        return (lambda ws, _=None: call(ws, name, (ptr(mask), 0, 0, C.byref(out), n_rows), (morphs_of(ws),))), [mask, ended]
    for w in s.worlds[:n]:
        w.view("steps")[...] = LIMIT                          # everybody has ended: a launch would show in every arena
    fg = forge_refill(torch, s, n)

    def run(ws, feed_lanes=None):
        feeds = (_lib.Feed * len(ws))(*[fg["feeds"][fg["keys"][i]] for i in range(len(ws))])
        if feed_lanes is not None:
            feeds[feed_lanes[0]].lanes = feed_lanes[1]
        return call(ws, name, (feeds, ptr(fg["occupant"]), _lib.WHEN["steps"], LIMIT, C.byref(fg["out"]), N_IDS, n_rows), (morphs_of(ws),))
    return run, [fg["occupant"], fg["cursors"], fg["raw"]["steps"].raw, fg["raw"]["finished"].raw] + [w._morph_dev[f] for w in s.worlds[:n]
                                                                                                     for f in ("shape", "x", "amp")]


@pytest.mark.parametrize("name", REFUSED)
def test_refusals_across_the_split(gpu, sets, name):
    """18 worlds: a NULL world at index 16, a world that was never reset at index 17 and (refill) a feed of other lanes at index 9 are
    refused with their documented texts -- the NULL world and the feed by their index; the text of a world before its reset names no
    world -- and after each refusal every arena, worlds 0 .. 15 included, and every buffer of the call holds the bytes it held: nothing
    was launched for the chunks that came before the bad world.  The same list without the fault is then taken."""
    torch = gpu
    from gym_rem2d_amd import _lib
    from gym_rem2d_amd.world import BatchedWorld
    s = sets()
    run, buffers = refusal_call(torch, s, name)
    good = s.worlds[:N_REFUSED]
    raw = BatchedWorld(s.worlds[17].n_envs, s.worlds[17].lanes, TB.CONT)
    try:
        raw.set_terrain(TB.terrain(17))
        raw._morph_dev = None
        cases = [("NULL world", good[:16] + [None] + good[17:], None, -1, "%s: world 16 is NULL" % name),
                 ("never reset", good[:17] + [raw], None, -3, "%s: rem2d_world_reset (or adopt) must be called first" % name)]
        if name == "refill":
            K = good[9].lanes
            cases.append(("feed of other lanes", good, (9, 2 * K), -1,
                          "refill: feed 9 holds creatures of %d lanes, its world creatures of %d" % (2 * K, K)))
        torch.cuda.synchronize()
        arenas = s.arenas()
        held = [b.clone() for b in buffers]
        for what, worlds, feed_lanes, code, text in cases:
            rc, said = run(worlds, feed_lanes)
            assert rc == code and said == text, "%s, %s: %d %r" % (name, what, rc, said)
            torch.cuda.synchronize()
            same_arenas(s.arenas(), arenas, "%s refused (%s)" % (name, what))
            assert all(torch.equal(b, h) for b, h in zip(buffers, held)), "%s refused (%s): a buffer was written" % (name, what)
        rc, said = run(good, None)
        assert rc == 0, said
        torch.cuda.synchronize()
        if name not in ("observe", "sense", "describe"):
            assert sum(a.tobytes() != b.tobytes() for a, b in zip(s.arenas(), arenas)) >= 12      # ... and it had something to do
        else:
            assert not all(torch.equal(b, h) for b, h in zip(buffers, held))
    finally:
        raw.close()


# ------------------------------------------------------------------------------------------------------------ refusal chains
# The GPU half of tests/test_world_calls_host.py: which of several faulty WORLDS of one list a call names first.  The list is five
# 2-lane one-block worlds' worth of faults -- a good world, one that was never reset, a NULL, one without terrain; for refill also a
# good world whose feed holds creatures of other lanes and a world on the static tile shape 4 -- in two orders, so that a check
# that runs world by world and one that runs in a loop of its own tell apart.  A link: call, record code and text, take the world
# the text names out of the list (the first one with that fault); the chain ends, without a call, when the list holds nothing the
# call refuses.  Every link is refused before a launch: after each one every arena and every buffer holds the bytes it held.
LEFT_OUT = ("a world of more than 64 lanes per creature: rem2d_world_create takes 2, 4, 8, 16, 32 or 64 lanes, so the library cannot make one",)
CHAIN_CALLS = ("observe", "control", "sense", "act", "act_recurrent", "act_normed", "describe", "reset_where", "refill")
CHAIN_ORDERS = {"a": ("good", "raw", "null", "bare", "lanes", "static"), "b": ("good", "static", "lanes", "bare", "null", "raw")}
CHAIN_FAULTS = (("is NULL", "null"), ("rem2d_world_set_terrain must be called first", "bare"),
                ("rem2d_world_reset (or adopt) must be called first", "raw"), ("lanes, its world creatures of", "lanes"),
                ("is on the static tile shape", "static"))
NEEDS_TERRAIN = ("sense", "act", "act_recurrent", "act_normed")


class ChainWorlds:
    """good / raw (terrain, never reset) / bare (reset, no terrain) / lanes (good; its feed is of 4 lanes) / static (tile shape 4)"""

    def __init__(self, torch):
        from gym_rem2d_amd.world import BatchedWorld
        self.torch, self.w = torch, {}
        m = self.morph = TB.morphology(32)
        assert (m.lanes, TB.blocks(32)) == (2, 1)
        try:
            for kind in ("good", "raw", "bare", "lanes", "static"):
                w = self.w[kind] = BatchedWorld(m.n_envs, m.lanes, TB.CONT)
                if kind != "bare":
                    w.set_terrain(TB.terrain(32))
                if kind != "raw":
                    w.reset(m, tile_shape=4 if kind == "static" else None)
            self.w["null"] = None
            self.n_rows = 5 * m.n_envs
            self.index = [torch.arange(k * m.n_envs, (k + 1) * m.n_envs, dtype=torch.int32, device="cuda") for k in range(5)]
            self.reward, self.done = torch.zeros(self.n_rows, device="cuda"), torch.zeros(self.n_rows, dtype=torch.bool, device="cuda")
            for w, idx in zip(self.real(), self.index):
                w.set_outputs(self.reward, self.done, idx)
            torch.cuda.synchronize()
        except BaseException:
            self.close()
            raise

    def real(self):
        return [w for w in self.w.values() if w is not None]

    def arenas(self):
        return [w.arena.clone() for w in self.real()]

    def close(self):
        for w in self.real():
            w.close()


def chain_call(torch, cw, name):
    """-> (run(kinds) -> (code, text), [device tensors the call could write])"""
    from gym_rem2d_amd import _lib, policy
    n_rows = cw.n_rows
    rays = dev(torch, R.bipedal_rays())
    some = {f: dev(torch, cw.morph.arrays[f]) for f in _lib.MORPH_FIELDS}

    def ws(kinds):
        return [cw.w[k] for k in kinds]

    def morphs_of(kinds):
        return (_lib.Morph * len(kinds))(*[morph_struct(some) for _ in kinds])
    if name == "observe":
        out = torch.full((n_rows, CM.width(4)), 7.5, dtype=torch.float32, device="cuda")
        return (lambda kinds: call(ws(kinds), name, (4, ptr(out), n_rows))), [out]
    if name == "control":
        values = torch.full((n_rows, 4), 0.5, dtype=torch.float64, device="cuda")
        return (lambda kinds: call(ws(kinds), name, (TB.CTRL_TARGET, ptr(values), 4, n_rows, None))), [values]
    if name == "sense":
        frac = torch.full((n_rows, 10), 7.5, dtype=torch.float32, device="cuda")
        return (lambda kinds: call(ws(kinds), name, (ptr(rays), 10, ptr(frac), None, n_rows))), [frac]
    if name == "describe":
        out = torch.full((n_rows, 8), -5.0, dtype=torch.float32, device="cuda")
        return (lambda kinds: call(ws(kinds), name, (15, 4, ptr(out), n_rows))), [out]
    if name in ("act", "act_recurrent", "act_normed"):
        rec = name == "act_recurrent"
        b = act_buffers(torch, n_rows, rec)
        bufs = (b["obs"].inner, b["frac"].inner, b["targets"].inner, b["valid"].inner)
        held = [v.raw for v in b.values()]
        if rec:
            pol = policy.RecurrentPolicy.random(n_rows, ACT_BODIES, ACT_HIDDEN, ACT_CONTEXT, seed=5).to("cuda")
            desc = pol.descriptor(*bufs, b["memory"].inner)
        else:
            pol = policy.MLPPolicy.random(n_rows, ACT_BODIES, ACT_HIDDEN, seed=5).to("cuda")
            desc = pol.descriptor(*bufs)
        if name == "act_normed":
            norm = policy.ObsNormalizer(1, n_rows, ACT_BODIES, 10, device="cuda")
            return ((lambda kinds: normed_call(ws(kinds), norm.descriptor(), desc, rays, 1)),
                    held + list(pol.weights) + [norm.count, norm.s1, norm.s2hi, norm.s2lo, norm.mu, norm.inv])
        return (lambda kinds: call(ws(kinds), name, (C.byref(desc), ptr(rays)))), held + list(pol.weights)
    if name == "reset_where":
        mask = torch.ones(n_rows, dtype=torch.uint8, device="cuda")
        return (lambda kinds: call(ws(kinds), name, (ptr(mask), 0, 0, None, n_rows), (morphs_of(kinds),))), [mask] + list(some.values())
    cursor = torch.zeros(1, dtype=torch.int32, device="cuda")
    occupant = torch.arange(n_rows, dtype=torch.int32, device="cuda")
    ids = torch.arange(cw.morph.n_envs, dtype=torch.int32, device="cuda")

    def run(kinds):
        feeds = (_lib.Feed * len(kinds))()
        for f, k in zip(feeds, kinds):
            f.M, f.id, f.count, f.cursor, f.lanes = morph_struct(some), ptr(ids), cw.morph.n_envs, ptr(cursor), 4 if k == "lanes" else 2
        return call(ws(kinds), name, (feeds, ptr(occupant), _lib.WHEN["steps"], 1, None, n_rows, n_rows), (morphs_of(kinds),))
    return run, [cursor, occupant, ids] + list(some.values())


def chain_kinds(name, order):
    return [k for k in CHAIN_ORDERS[order] if name == "refill" or k not in ("lanes", "static")]


def refused(name, kinds):
    """what the call refuses of a list, by the headers: NULL and never-reset worlds always, a world without terrain where rays are
    cast, the feed of other lanes and the static tile shape in refill"""
    return [k for k in kinds if k in ("null", "raw") or (k == "bare" and name in NEEDS_TERRAIN) or (k in ("lanes", "static") and name == "refill")]


def walk_chain(torch, cw, name, order, check=None):
    """[[code, text], ...] down to a list the call would take; check(): called after every link"""
    run, _ = chain_call(torch, cw, name) if check is None else check[0]
    kinds, out = chain_kinds(name, order), []
    while refused(name, kinds) and len(out) < 8:
        rc, text = run(kinds)
        out.append([rc, text])
        if check is not None:
            check[1](kinds)
        gone = [k for needle, k in CHAIN_FAULTS if needle in text and k in kinds]
        if rc == 0 or len(gone) != 1:
            break
        kinds.remove(gone[0])
    return out


def record_chains(torch):
    """for tests/test_world_calls_host.py --record: {call: {order: chain}}"""
    cw = ChainWorlds(torch)
    try:
        return {name: {order: walk_chain(torch, cw, name, order) for order in CHAIN_ORDERS} for name in CHAIN_CALLS}
    finally:
        cw.close()


@pytest.fixture(scope="module")
def chain_worlds(gpu):
    cw = ChainWorlds(gpu)
    yield cw
    cw.close()


@pytest.mark.parametrize("name", CHAIN_CALLS)
def test_refusal_chains(gpu, chain_worlds, name):
    """both orders of the list, link by link against tests/golden/world_call_refusals.json (recorded before the calls were put on
    shared helpers): code, text, and no byte of any arena or buffer moved.  The chains are no vacuous ones: each ends with nothing
    left that the call refuses, and every fault the call knows was named once."""
    import json
    import test_world_calls_host as H
    torch = gpu
    cw = chain_worlds
    with open(H.GOLDEN) as f:
        record = json.load(f)
    want = record["gpu"][name]
    assert sorted(record["gpu"]) == sorted(CHAIN_CALLS) and record["gpu_left_out"] == list(LEFT_OUT)
    run, buffers = chain_call(torch, cw, name)
    torch.cuda.synchronize()
    arenas, held = cw.arenas(), [b.clone() for b in buffers]

    def untouched(kinds):
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(cw.arenas(), arenas)), "%s refused (%s): an arena moved" % (name, kinds)
        assert all(torch.equal(b, h) for b, h in zip(buffers, held)), "%s refused (%s): a buffer was written" % (name, kinds)
    for order in CHAIN_ORDERS:
        got = walk_chain(torch, cw, name, order, ((run, buffers), untouched))
        for i, (a, b) in enumerate(zip(got, want[order])):
            assert a == b, "%s, order %s, link %d: %r, the record has %r" % (name, order, i, a, b)
        assert len(got) == len(want[order]) == len(refused(name, chain_kinds(name, order))), (name, order, got)
        assert all(rc in (-1, -3) and text.startswith(name + ": ") for rc, text in got)
    # (the calls that look at a world's faults world by world name them in the list's order; the act calls and reset_where run a
    # loop per fault, so the two orders give them one chain)
    assert ([t for _, t in want["a"]] != [t for _, t in want["b"]]) == (name in ("observe", "control", "describe", "sense", "refill"))


# ---------------------------------------------------------------------------------------------------------- through the facade
FACADE_STEPS = 20
_FACADE = []


def facade_population():
    """(terrain, [Morphology], rows): the smallest population that gives BatchedModular2D five lane buckets and, with step_groups = 4,
    more than 16 worlds -- four buckets of just enough creatures for a world in each of the four groups (25 of 8 lanes, 16 each of 16,
    32 and 64 lanes) and one creature of 2 lanes: 74 creatures, 17 worlds -- in an interleaved population order"""
    if not _FACADE:
        from gym_rem2d_amd import make_terrain
        from gym_rem2d_amd.compiler import Morphology
        pool = TB._pool()
        small, mid, big = ([s for s in pool if lo <= s.n_bodies <= hi] for lo, hi in ((2, 2), (3, 8), (9, 16)))
        assert len(small) >= 1 and len(mid) >= 25 and len(big) >= 32
        morphs = [Morphology.from_specs(small[:1], 2), Morphology.from_specs(mid[:25], 8), Morphology.from_specs(big[:16], 16),
                  Morphology.from_specs(big[8:24], 32), Morphology.from_specs(big[16:32], 64)]
        n = sum(m.n_envs for m in morphs)
        order = np.random.default_rng(7).permutation(n)
        rows = np.split(order, np.cumsum([m.n_envs for m in morphs])[:-1])
        _FACADE.append((make_terrain(4), morphs, rows))
    return _FACADE[0]


def facade_env(morphs, rows):
    from gym_rem2d_amd.env import BatchedModular2D
    env = BatchedModular2D(seed=4, flags=TB.CONT)
    env.step_groups = 4
    env._upload(list(zip(morphs, rows)), sum(m.n_envs for m in morphs))
    assert len({w.lanes for w, _ in env.worlds}) == 5 and len(env.groups) == 4 and len(env.worlds) > TB.CTL_TABLE, len(env.worlds)
    return env


@pytest.mark.parametrize("recurrent", [False, True], ids=["policy", "recurrent"])
def test_policy_loop_through_the_facade(gpu, oracle, recurrent):
    """BatchedModular2D with five lane buckets and step_groups = 4 holds 17 worlds: 20 closed-loop steps under a device policy, every
    creature under its own weight set.  Before every step act()'s targets and validity bytes (and the context words) equal the
    model's on the ORACLE's state -- policy_model.policy_loop_run / recurrent_model.recurrent_loop_run -- and after the last step so
    do observe()'s rows and sense_terrain()'s fractions: each of them one library call over all 17 worlds."""
    torch = gpu
    from env_harness import population_rows
    from gym_rem2d_amd import _lib, policy
    import test_policy_gpu as TP
    import test_recurrent_gpu as TR
    terrain, morphs, rows = facade_population()
    if recurrent:
        runs = RM.recurrent_loop_run(oracle, "tables", TB.CONT, n_steps=FACADE_STEPS, morphs=morphs, terrain=terrain, key=("tables", "recurrent"))
    else:
        runs = PM.policy_loop_run(oracle, "tables", TB.CONT, n_steps=FACADE_STEPS, morphs=morphs, terrain=terrain, key=("tables", "policy"))
    env = facade_env(morphs, rows)
    try:
        n, Mb = env.n_envs, PM.LOOP_BODIES
        first_pop = np.zeros(n, np.int64)
        for run, r in zip(runs, rows):
            first_pop[r] = CM.left_out_first(run, *_lib.capacity(False)[:2])[0]
        assert (first_pop > FACADE_STEPS).mean() >= 1.0 - F.LEFT_OUT_CAP
        if recurrent:
            env.set_policy(TR.population_policy(torch, policy, runs, rows, n, RM.LOOP_CONTEXT))
        else:
            env.set_policy(TP.population_policy(torch, policy, runs, rows, n))
        for t in range(FACADE_STEPS):
            targets, valid = env.act()
            keep = first_pop > t
            want_t, want_v = population_rows(runs, rows, "targets", t, Mb), population_rows(runs, rows, "valid", t, Mb)
            ne = (PM.bits(targets.cpu().numpy()) != PM.bits(want_t)) & keep[:, None]
            assert not ne.any(), "act() before step %d: %d targets differ, rows %s" % (t, int(ne.sum()), np.flatnonzero(ne.any(axis=1))[:8])
            assert np.array_equal(valid.cpu().numpy()[keep], want_v[keep])
            if recurrent:
                got_m, want_m = env.policy_memory.cpu().numpy(), TR._population_memory(runs, rows, t + 1, n)
                assert np.array_equal(got_m.view(np.uint32)[keep], want_m.view(np.uint32)[keep]), "memory after act() before step %d" % t
            env.step(1)
        keep = first_pop > FACADE_STEPS
        obs = env.observe(Mb).cpu().numpy()
        assert np.array_equal(obs.view(np.uint32)[keep], population_rows(runs, rows, "obs", FACADE_STEPS, Mb).view(np.uint32)[keep])
        frac = env.sense_terrain().cpu().numpy()
        want_f = np.zeros((n, 10), f32)
        for run, r in zip(runs, rows):
            want_f[r] = run["frac"][FACADE_STEPS]
        assert np.array_equal(frac.view(np.uint32)[keep], want_f.view(np.uint32)[keep])
        assert env.handover_failures() == 0 and not env.errors()[keep].any()
    finally:
        env.close()


def test_streamed_env_with_step_groups(gpu, oracle):
    """reset_stream cuts a lane bucket into a world per step group like every upload, so with step_groups = 4 the L-system loop
    population (119 creatures) in 100 slots is held in 11 worlds -- more than STREAM_TABLE -- and every refill() of run_stream is two
    launches, the worlds of a bucket sharing its feed across them: every id's fitness is stream_model.run's, bit for bit; everybody
    finished, every pending creature was handed out once, every slot retired."""
    from gym_rem2d_amd import evaluate
    from gym_rem2d_amd.env import BatchedModular2D
    import stream_model as SM
    import test_stream_gpu as TS
    batches, ids = TS.population()
    slots = 100
    env = BatchedModular2D(seed=4, flags=evaluate.EVAL_FLAGS)
    env.step_groups = 4
    try:
        fit = evaluate.run_stream(env, batches, TS.N_TOTAL, slots, max_steps=SM.MAX_STEPS, chunk=SM.CHUNK, on_error="fallback")
        st = env.stream
        assert env.n_envs == slots and len(env.worlds) > TB.STREAM_TABLE, len(env.worlds)
        assert max(sum(w.lanes == K for w, _ in env.worlds) for K in (4, 8, 16)) >= 3            # a feed shared by several worlds
        model = SM.run(oracle, "lsystem")
        assert not any(o.any() for o in model["over"])
        got, want = st.fitness.cpu().numpy(), SM.by_id(model["fitness"], ids, TS.N_TOTAL)
        assert fit.cpu().numpy().tobytes() == got.tobytes()
        assert got.tobytes() == want.tobytes(), "ids %s differ from the model" % np.flatnonzero(got != want)[:8]
        assert bool(st.finished.all()) and not st.err.any() and env.handover_failures() == 0
        assert st.handed_out() == st.pending and sum(st.pending) == TS.N_TOTAL - slots
        assert (st.occupant.cpu().numpy() == -1).all() and (st.cursors.cpu().numpy() >= np.array(st.pending)).all()
        by_limit = SM.by_id(model["how"], ids, TS.N_TOTAL) == "steps"
        assert (st.steps.cpu().numpy()[by_limit] == SM.MAX_STEPS).all() and by_limit.sum() >= 40
    finally:
        env.close()
