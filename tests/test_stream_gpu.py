"""Streaming evaluation on a real MI355X (pytest -m gpu): rem2d_worlds_refill / BatchedModular2D.reset_stream, refill, the `stream`
record and evaluate.run_stream (include/rem2d_stream.h).

Yardsticks, all exact.  GPU against GPU: a population streamed through a third as many slots gets, id by id, the fitness of the same
population uploaded as a whole; a refilled slot holds, and goes on holding, what a freshly reset env of its new creature holds, and
nobody else changes by a byte.  GPU against tests/stream_model.py (oracle alone): every creature's fitness and way of ending.

Populations: the L-system loop population (119 creatures of 2 / 4 / 8 / 16 lanes) and test_episodes_gpu.byte_population()'s six worlds
(K = 2 ... 64, two of them of 8 lanes: they share a feed and its cursor; no creature count a multiple of 64 / K)."""
import ctypes as C

import numpy as np
import pytest

import control_model as M
import lifecycle_forge as LF
import stream_model as SM
import test_episodes_gpu as EG

pytestmark = pytest.mark.gpu

CONT = 1
GUARD = 64
SENT = dict(fitness=-12345.678, steps=-77, err=-99, finished=0xA5)
N_TOTAL, SLOTS = 119, 40


@pytest.fixture(scope="module")
def gpu():
    import replay
    return replay.need_gpu()


_POP = []


def population():
    """(batches [(Morphology, ids)], ids per bucket) of the L-system loop population under an interleaved id order"""
    if not _POP:
        terrain, morphs = M.loop_population("lsystem")
        assert [(m.lanes, m.n_envs) for m in morphs] == [(2, 16), (4, 40), (8, 23), (16, 40)]
        order = np.random.default_rng(11).permutation(N_TOTAL)
        ids, at = [], 0
        for m in morphs:
            ids.append(order[at:at + m.n_envs])
            at += m.n_envs
        _POP.append(([(m, i) for m, i in zip(morphs, ids)], ids))
    return _POP[0]


# ------------------------------------------------------------------------------------------------------- 1. streamed equals plain
@pytest.mark.parametrize("form", list(EG.FORMS))
def test_streamed_equals_plain(gpu, oracle, form):
    """The 119 creatures through 40 slots (5 / 14 / 8 / 13: about three occupants per slot), max_steps 125 in chunks of 25: for every
    id, stream.fitness == the fitness of the same population uploaded as a whole and run by evaluate._episode(env, 125, 25) in the
    same launch form, and (the bit-exact builds) == the stream model's; everybody finished, no error bit, every pending creature
    handed out once, every slot retired; steps == 125 for the creatures the model ends by the limit and below the boundary for
    those it freezes earlier (a creature frozen in the last chunk may or may not have been stepped on: not compared).  A refill
    that drops, duplicates or mis-copies a creature fails here.  Measured with the oracle: 69 creatures freeze (12 of them before the last boundary), 50 run into the limit."""
    torch = gpu
    from gym_rem2d_amd import evaluate
    from gym_rem2d_amd.env import BatchedModular2D, stream_slots
    wide, options = EG.FORMS[form]
    batches, ids = population()
    plain = BatchedModular2D(seed=4, flags=evaluate.EVAL_FLAGS, wide=wide, options=options)
    env = BatchedModular2D(seed=4, flags=evaluate.EVAL_FLAGS, wide=wide, options=options)
    try:
        plain.reset_batches(batches, N_TOTAL)
        evaluate._episode(plain, SM.MAX_STEPS, SM.CHUNK, compact=False)
        want = plain.fitness.cpu().numpy()
        assert not plain.errors().any() and plain.handover_failures() == 0
        fit = evaluate.run_stream(env, batches, N_TOTAL, SLOTS, max_steps=SM.MAX_STEPS, chunk=SM.CHUNK, on_error="fallback")
        st = env.stream
        got = st.fitness.cpu().numpy()
        assert env.n_envs == SLOTS and sorted(w.n_envs for w, _ in env.worlds) == sorted(stream_slots([16, 40, 23, 40], [2, 4, 8, 16], SLOTS))
        assert fit.cpu().numpy().tobytes() == got.tobytes()
        differ = np.flatnonzero(got != want)
        assert differ.size == 0, "%s: fitness of ids %s differs: streamed %s, plain %s" % (form, differ[:8], got[differ[:8]], want[differ[:8]])
        assert (want != 0).sum() >= 60 and len(set(want.tolist())) >= 30
        assert bool(st.finished.all()) and not st.err.any() and env.handover_failures() == 0
        assert st.handed_out() == st.pending == [11, 26, 15, 27]
        assert (st.occupant.cpu().numpy() == -1).all() and (st.cursors.cpu().numpy() >= np.array(st.pending)).all()
        rep = env.last_episode
        assert rep is not None and not rep.codes.any() and rep.handover == rep.overflow == rep.unresolved == []
        model = SM.run(oracle, "lsystem")
        assert not any(o.any() for o in model["over"])
        how = SM.by_id(model["how"], ids, N_TOTAL)
        bound = SM.by_id(model["steps"], ids, N_TOTAL)
        steps = st.steps.cpu().numpy()
        by_limit = how == "steps"
        assert by_limit.sum() >= 40 and (~by_limit).sum() >= 40
        assert (steps[by_limit] == SM.MAX_STEPS).all()
        early = ~by_limit & (bound < SM.MAX_STEPS)
        assert early.sum() >= 10 and (steps[early] <= bound[early]).all() and (steps[early] > 0).all()      # (the oracle: 2 by step 75, 10 by step 100)
        if wide != "fma":
            mfit = SM.by_id(model["fitness"], ids, N_TOTAL)
            assert got.tobytes() == mfit.tobytes(), "%s: ids %s differ from the model" % (form, np.flatnonzero(got != mfit)[:8])
    finally:
        plain.close()
        env.close()


# -------------------------------------------------------------------------------------------------------- 2. the image of one call
def guarded(torch, n, name, dtype):
    return torch.full((n + 2 * GUARD,), SENT[name], dtype=dtype, device="cuda")


def inner(buf, name):
    a = buf.cpu().numpy()
    assert (a[:GUARD] == a.dtype.type(SENT[name])).all() and (a[-GUARD:] == a.dtype.type(SENT[name])).all(), "guards of `%s`" % name
    return a[GUARD:-GUARD].copy()


def morph_struct(dev):
    from gym_rem2d_amd import _lib
    m = _lib.Morph()
    for k in _lib.MORPH_FIELDS:
        setattr(m, k, dev[k].data_ptr())
    return m


def refill_call(worlds, feeds, occupant, when, max_steps, out, n_ids, n_rows):
    """rem2d_worlds_refill itself on a list of BatchedWorld; feeds: one _lib.Feed per world"""
    from gym_rem2d_amd import _lib
    morphs = (_lib.Morph * len(worlds))(*[morph_struct(w._morph_dev) for w in worlds])
    arr = (_lib.Feed * len(worlds))(*feeds)
    w0 = worlds[0]
    _lib.check(w0.L.rem2d_worlds_refill(_lib.world_array(worlds), morphs, len(worlds), arr, occupant.data_ptr(), when, max_steps,
                                        None if out is None else C.byref(out), n_ids, n_rows, w0._stream()), w0.wide)


N_IDS, LIMIT, OLD_ID0 = 600, 1000, 300
FEED_ID0 = {2: 0, 4: 20, 8: 70, 16: 120, 64: 170}
SHORT = 3            # pending creatures of the 16-lane feed: fewer than its world's ended creatures


@pytest.mark.parametrize("build", list(EG.BUILDS))
def test_image(gpu, build):
    """Six worlds, 60 steps, then ONE call on a forged occupant array and forged step words (when = steps): per world the first and
    the last creature and one whole wavefront have ended, one wavefront has nobody ended, some slots are empty (-1; half of those
    carry an ended step word too and must still be left alone), one ended slot carries an id beyond n_ids.  The feed of a lane count
    is its own bucket in reverse order; the two 8-lane worlds share one feed and one cursor; the 16-lane feed has 3 pending
    creatures for more than 5 ended slots.  Afterwards every byte of every arena -- padding creatures and gaps included -- is the
    snapshot taken before the call, except the slots that took a creature, which are those of a fresh env that was reset with the
    creature `occupant` now names and never stepped, and the retired slots, which differ in REM2D_F_FROZEN only.  The worlds' device
    morphology is the new occupants' at the refilled slots and unchanged elsewhere; per feed the ids handed out are exactly
    id[0 : min(cursor, count)], each once, and the cursor advanced by the number of ended creatures; the harvest sits between guards,
    sentinels untouched for ids that did not finish; the set_outputs arrays did not move."""
    torch = gpu
    from gym_rem2d_amd import _lib
    from gym_rem2d_amd.compiler import Morphology
    wide = EG.BUILDS[build]
    terrain, morphs = EG.byte_population()
    a, rows = EG.make_env(morphs, wide)
    b = None
    try:
        assert len(a.worlds) == len(morphs) and all(w.n_envs == m.n_envs and w.lanes == m.lanes for (w, _), m in zip(a.worlds, morphs))
        n_rows = a.n_envs
        a.step(EG.SETTLE)
        mask = EG.make_mask(a)                       # first and last creature, a whole first wavefront, none of the second
        rng = np.random.default_rng(17)
        occ0 = np.full(n_rows, -1, np.int32)
        ended_w, empty_w, forged_empty = [], [], 0
        for wi, ((w, _), r) in enumerate(zip(a.worlds, rows)):
            n, per = w.n_envs, 64 // w.lanes
            loc = mask[r] != 0
            cand = np.arange(1, n - 1) if n <= per else np.arange(2 * per if n > 2 * per else per, n - 1)
            empty = np.zeros(n, bool)
            empty[cand[::4]] = True
            assert empty.any() and not empty[0] and not empty[n - 1]
            forged = loc.copy()
            forged[np.flatnonzero(empty)[::2]] = True                    # an empty slot whose step word says "ended"
            forged_empty += int((forged & empty).sum())
            st = w.view("steps")
            st[torch.from_numpy(np.flatnonzero(forged)).to("cuda")] = LIMIT + wi
            occ = OLD_ID0 + r.astype(np.int32)
            occ[empty] = -1
            if wi == 0:
                occ[n - 1] = N_IDS + 5                                   # ended, refilled, but no row of `out` is its own
            occ0[r] = occ
            ended_w.append(loc & ~empty)
            empty_w.append(empty)
        assert forged_empty >= 6
        # the feeds: a lane count's own creatures in reverse order
        feeds, feed_dev, feed_host, cursors = {}, {}, {}, torch.zeros(8, dtype=torch.int32, device="cuda")
        for k, K in enumerate(sorted(FEED_ID0)):
            own = Morphology.concat([m for m in morphs if m.lanes == K])
            rev = own.take(np.arange(own.n_envs)[::-1])
            count = SHORT if K == 16 else rev.n_envs
            dev = {f: torch.from_numpy(rev.arrays[f].copy()).to("cuda") for f in _lib.MORPH_FIELDS}
            dev["id"] = torch.arange(FEED_ID0[K], FEED_ID0[K] + rev.n_envs, dtype=torch.int32, device="cuda")
            f = _lib.Feed()
            f.M, f.id, f.count, f.lanes, f.cursor = morph_struct(dev), dev["id"].data_ptr(), count, K, cursors[k:k + 1].data_ptr()
            feeds[K], feed_dev[K], feed_host[K] = f, dev, (rev, count, k)
        n_ended = {K: sum(int(e.sum()) for e, (w, _) in zip(ended_w, a.worlds) if w.lanes == K) for K in FEED_ID0}
        assert n_ended[16] >= 5 > SHORT and all(n_ended[K] < feed_host[K][1] for K in (2, 4, 8, 64)) and sum(w.lanes == 8 for w, _ in a.worlds) == 2
        occupant = torch.from_numpy(occ0).to("cuda")
        raw = {name: guarded(torch, N_IDS, name, dt) for name, dt in (("fitness", torch.float64), ("steps", torch.int32), ("err", torch.int32),
                                                                        ("finished", torch.uint8))}
        out = _lib.StreamOut()
        for name in raw:
            setattr(out, name, raw[name][GUARD:].data_ptr())
        before = EG.arenas(a)
        pre = {f: EG.pop_field(a, f) for f in ("fitness", "steps", "err")}
        morph_before = [{f: w._morph_dev[f].cpu().numpy().copy() for f in _lib.MORPH_FIELDS} for w, _ in a.worlds]
        out_before = (a._reward.clone(), a._done.clone(), [idx.clone() for _, idx in a.worlds])
        worlds = [w for w, _ in a.worlds]
        refill_call(worlds, [feeds[w.lanes] for w in worlds], occupant, _lib.WHEN["steps"], LIMIT, out, N_IDS, n_rows)
        after = EG.arenas(a)
        occ1 = occupant.cpu().numpy()
        cur = cursors.cpu().numpy()
        # who got what: occupant is the record
        new_morphs, took_w, retired_w, handed = [], [], [], {K: [] for K in FEED_ID0}
        for (w, _), r, m, ended, empty in zip(a.worlds, rows, morphs, ended_w, empty_w):
            K = w.lanes
            rev, count, _ = feed_host[K]
            now = occ1[r]
            assert np.array_equal(now[~ended], occ0[r][~ended]), "%d-lane world: occupant of a slot that had not ended moved" % K
            took = ended & (now >= 0)
            retired = ended & (now < 0)
            q = now[took] - FEED_ID0[K]
            assert (now[retired] == -1).all() and (q >= 0).all() and (q < count).all()
            handed[K] += now[took].tolist()
            pick = np.arange(w.n_envs)
            pick[took] = w.n_envs + q
            new_morphs.append(Morphology.concat([m, rev]).take(pick))
            took_w.append(took)
            retired_w.append(retired)
        for K, (rev, count, k) in feed_host.items():
            assert cur[k] == n_ended[K], "cursor of the %d-lane feed: %d for %d ended creatures" % (K, cur[k], n_ended[K])
            assert sorted(handed[K]) == list(range(FEED_ID0[K], FEED_ID0[K] + min(int(cur[k]), count))), "%d-lane feed: ids lost or handed out twice" % K
        assert sum(int(x.sum()) for x in retired_w) == n_ended[16] - SHORT and retired_w[3].sum() == n_ended[16] - SHORT
        assert all(t.any() for t in took_w) and (cur[5:] == 0).all()
        # the arenas: fresh worlds of the creatures now in the slots, never stepped
        b, _ = EG.make_env(new_morphs, wide)
        moved = 0
        for (w, _), bef, fre, aft, took, retired in zip(a.worlds, before, EG.arenas(b), after, took_w, retired_w):
            exp = EG.expected_arena(w, bef, fre, took)
            off, cnt, esz = LF.field_place(w, "frozen")
            fz = exp[off:off + cnt * esz].view(np.int32)
            assert not fz[np.flatnonzero(retired)].any()
            fz[np.flatnonzero(retired)] = 1
            assert aft.tobytes() == exp.tobytes(), "%d-lane world: %s" % (w.lanes, EG.differing_fields(w, aft, exp))
            moved += int((exp != bef).sum())
        assert moved > 1000
        # the worlds' device morphology: the new occupants' words at the refilled slots, nothing else
        changed = 0
        for (w, _), m_old, m_new, took in zip(a.worlds, morph_before, new_morphs, took_w):
            lanes = np.repeat(took, w.lanes)
            for f in _lib.MORPH_FIELDS:
                now = w._morph_dev[f].cpu().numpy()
                assert now.tobytes() == m_new.arrays[f].tobytes(), "%d-lane world: device morphology `%s`" % (w.lanes, f)
                assert now[~lanes].tobytes() == m_old[f][~lanes].tobytes()
                changed += int((now != m_old[f]).sum())
        assert changed > 500
        # the harvest
        h = {name: inner(raw[name], name) for name in raw}
        fin = np.zeros(N_IDS, bool)
        for r, ended in zip(rows, ended_w):
            rr = r[ended & (occ0[r] < N_IDS)]
            ids = occ0[rr]
            fin[ids] = True
            assert h["fitness"][ids].tobytes() == pre["fitness"][rr].tobytes() and np.array_equal(h["err"][ids], pre["err"][rr])
            assert np.array_equal(h["steps"][ids], pre["steps"][rr]) and (h["steps"][ids] >= LIMIT).all()
        assert fin.sum() == sum(n_ended.values()) - 1 and (h["finished"][fin] == 1).all() and (h["finished"][~fin] == SENT["finished"]).all()
        assert (h["fitness"][~fin] == SENT["fitness"]).all() and (h["steps"][~fin] == SENT["steps"]).all() and (h["err"][~fin] == SENT["err"]).all()
        assert (pre["fitness"] != 0).sum() >= 20
        # the set_outputs arrays
        assert torch.equal(a._reward, out_before[0]) and torch.equal(a._done, out_before[1])
        assert all(torch.equal(idx, old) for (_, idx), old in zip(a.worlds, out_before[2]))
    finally:
        a.close()
        if b is not None:
            b.close()


# ------------------------------------------------------------------------------------------------ 3. reset_where on a refilled slot
def envs_of_occupants(env, batches, flags):
    """a fresh env that holds, slot for slot, the creatures env.stream.occupant names (all slots occupied)"""
    from gym_rem2d_amd.compiler import Morphology
    from gym_rem2d_amd.env import BatchedModular2D
    occ = env.stream.occupant.cpu().numpy()
    assert (occ >= 0).all()
    where = {}
    for m, ids in batches:
        for e, i in enumerate(np.asarray(ids).tolist()):
            where[i] = (m, e)
    new = []
    for w, idx in env.worlds:
        r = idx.cpu().numpy()
        parts = [where[int(i)] for i in occ[r]]
        assert all(m.lanes == w.lanes for m, _ in parts)
        new.append((Morphology.concat([m.take([e]) for m, e in parts]), r))
    fresh = BatchedModular2D(seed=4, flags=flags)
    fresh._upload(new, env.n_envs)
    assert [(w.n_envs, w.lanes) for w, _ in fresh.worlds] == [(w.n_envs, w.lanes) for w, _ in env.worlds]
    return fresh


def test_reset_where_restarts_the_new_occupant(gpu):
    """reset_stream, 25 steps, refill at a 25-step limit: all 40 slots hand on.  12 steps later reset_where(mask) on every other slot,
    then 25 steps: the masked slots are, in every byte of every field, where a fresh env of the creatures `occupant` names is after
    25 steps, the others where it is after 37 -- reset_where restarts the slot's CURRENT creature, from the device morphology
    refill() rewrote."""
    torch = gpu
    batches, ids = population()
    from gym_rem2d_amd.env import BatchedModular2D
    env = BatchedModular2D(seed=4, flags=CONT)
    fresh = late = None
    try:
        env.reset_stream(batches, N_TOTAL, SLOTS)
        first = env.stream.occupant.cpu().numpy().copy()
        env.step(25)
        st = env.refill(when=("steps",), max_steps=25)
        occ = st.occupant.cpu().numpy()
        assert st is env.stream and (occ >= 0).all() and not np.intersect1d(occ, first).size and len(set(occ.tolist())) == SLOTS
        assert st.finished.cpu().numpy()[first].all() and int(st.finished.sum()) == SLOTS and st.handed_out() == [5, 14, 8, 13]
        assert (st.steps.cpu().numpy()[first] == 25).all()
        env.step(12)
        mask = np.zeros(SLOTS, np.uint8)
        mask[::2] = 1
        ended = env.reset_where(torch.from_numpy(mask).to("cuda"))
        assert np.array_equal(ended.cpu().numpy(), mask != 0)
        env.step(25)
        fresh, late = envs_of_occupants(env, batches, CONT), envs_of_occupants(env, batches, CONT)
        fresh.step(25)
        late.step(37)
        n = EG.same_creatures(env, fresh, mask != 0, "reset_where on a refilled slot against a fresh env of its occupant")
        n += EG.same_creatures(env, late, mask == 0, "a refilled slot against a fresh env of its occupant")
        assert n == SLOTS and np.array_equal(st.occupant.cpu().numpy(), occ)
        assert EG.pop_field(env, "steps")[mask != 0].tolist() == [25] * int(mask.sum())
        assert all(e.handover_failures() == 0 for e in (env, fresh, late))
        with pytest.raises(ValueError, match="compact: this env streams"):
            env.compact()
        env.reset_batches(batches, N_TOTAL)                   # an upload drops the record
        with pytest.raises(ValueError, match="reset_stream first"):
            env.refill(max_steps=25)
    finally:
        for e in (env, fresh, late):
            if e is not None:
                e.close()


# ------------------------------------------------------------------------------------------------------- 4. nobody has ended
def test_nobody_ended_changes_nothing(gpu):
    """10 steps after reset_stream nobody is frozen and nobody is near the limit: refill() changes no byte of any arena, no cursor,
    no occupant, no row of the record, and no word of the worlds' device morphology"""
    torch = gpu
    from gym_rem2d_amd import _lib, evaluate
    from gym_rem2d_amd.env import BatchedModular2D
    batches, ids = population()
    env = BatchedModular2D(seed=4, flags=evaluate.EVAL_FLAGS)
    try:
        env.reset_stream(batches, N_TOTAL, SLOTS)
        st = env.stream
        env.step(10)
        assert not env.frozen.any()
        before, occ = EG.arenas(env), st.occupant.clone()
        morph = [{f: w._morph_dev[f].clone() for f in _lib.MORPH_FIELDS} for w, _ in env.worlds]
        for kw in (dict(when=("frozen", "steps"), max_steps=SM.MAX_STEPS), dict(when=("frozen", "done")), dict(when="steps", max_steps=11)):
            assert env.refill(**kw) is st
            assert all(x.tobytes() == y.tobytes() for x, y in zip(before, EG.arenas(env))), kw
            assert not st.cursors.any() and torch.equal(st.occupant, occ) and not st.finished.any()
            assert not st.fitness.any() and not st.steps.any() and not st.err.any()
            assert all(torch.equal(w._morph_dev[f], m[f]) for (w, _), m in zip(env.worlds, morph) for f in _lib.MORPH_FIELDS)
        assert st.handed_out() == [0, 0, 0, 0]
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------------- 5. refused worlds
def test_worlds_the_call_refuses(gpu):
    """a world that was never reset (REM2D_E_STATE), and a world on the static tile shape 4 -- through the library on real handles"""
    torch = gpu
    from gym_rem2d_amd import _lib, make_terrain, synthetic
    from gym_rem2d_amd.world import BatchedWorld
    m = synthetic.chain_population(5, 8, "left")
    w = BatchedWorld(m.n_envs, m.lanes, CONT)
    try:
        w.set_terrain(make_terrain(4))
        cursor = torch.zeros(1, dtype=torch.int32, device="cuda")
        occupant = torch.arange(5, dtype=torch.int32, device="cuda")
        feed = _lib.Feed()
        feed.count, feed.lanes, feed.cursor = 0, 8, cursor.data_ptr()
        w._morph_dev = {f: torch.from_numpy(m.arrays[f]).to("cuda") for f in _lib.MORPH_FIELDS}
        with pytest.raises(_lib.Rem2dError, match="rem2d_world_reset .* must be called first"):
            refill_call([w], [feed], occupant, _lib.WHEN["steps"], 5, None, 5, 5)
        w.reset(m, tile_shape=4)
        with pytest.raises(_lib.Rem2dError, match="static tile shape 4.*planned from the joints"):
            refill_call([w], [feed], occupant, _lib.WHEN["steps"], 5, None, 5, 5)
        w.reset(m, tile_shape=3)
        w.step(6)
        refill_call([w], [feed], occupant, _lib.WHEN["steps"], 5, None, 5, 5)       # an empty feed: every slot is retired
        assert (occupant.cpu().numpy() == -1).all() and int(cursor.item()) == 5 and (w.view("frozen").cpu().numpy() == 1).all()
    finally:
        w.close()
