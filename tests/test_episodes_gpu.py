"""Episode boundaries on a real MI355X (pytest -m gpu): rem2d_worlds_reset_where / BatchedModular2D.reset_where, set_autoreset and
the `episodes` record (include/rem2d_episode.h).

Two yardsticks, both exact.  GPU against GPU, on bytes: a creature reset in place must hold, and go on holding, what the same creature
holds in an env that was reset as a whole -- and nobody else may change by a byte.  GPU against tests/episode_model.py (oracle
alone): who ends when, with which fitness after how many steps, and the state everybody is in at the finish (replay.verdict).

Populations: the four lane buckets of the L-system loop population (16 / 40 / 23 / 40 creatures of 2 / 4 / 8 / 16 lanes; for the byte
tests the last one is cut to 39 so that its last 64-lane block holds a padding creature too), the 8-module chains (12 creatures, 8
lanes) and five L-system creatures in a 64-lane bucket (one creature per wavefront): K = 2, with 32 creatures of mixed fate in one
wavefront, through K = 64."""
import ctypes as C

import numpy as np
import pytest

import control_model as M
import episode_model as EM
import lifecycle_forge as LF
import state_forge as F
from replay import read_state, verdict

pytestmark = pytest.mark.gpu

CONT = 1
GUARD = 64
SENT = dict(reward=-7.5, done=0xA5, ended=0xA5, fitness=-12345.678, steps=-77, count=1234567)
BUILDS = {"default": False, "wide": True, "fma": "fma"}
# launch forms of the continuation test: (build, launch options)
FORMS = {"step_train": (False, None), "velpost": (False, {"fuse_velpost": 1}), "two_launches": (False, {"fuse_velpost": 0}),
         "fused_step_kernel": (False, {"pipeline": 0}), "wide": (True, None), "fma": ("fma", None)}
SETTLE, AFTER = 60, 50


@pytest.fixture(scope="module")
def gpu():
    import replay
    return replay.need_gpu()


# ------------------------------------------------------------------------------------------------------------ populations, envs
_BYTE_POP = []


def byte_population():
    """(terrain, [Morphology]) of the byte tests: no world's creature count is a multiple of 64 / K (K = 64 aside)"""
    if not _BYTE_POP:
        from gym_rem2d_amd import synthetic
        from gym_rem2d_amd.compiler import Morphology
        terrain, ls = M.loop_population("lsystem")
        assert [(m.lanes, m.n_envs) for m in ls] == [(2, 16), (4, 40), (8, 23), (16, 40)]
        morphs = ls[:3] + [ls[3].take(np.arange(39))] + M.loop_population("chain8")[1]
        big = [s for s in synthetic.lsystem_specs(range(300)) if 9 <= s.n_bodies <= 16][:5]
        morphs.append(Morphology.from_specs(big, 64))
        assert all(m.lanes == 64 or m.n_envs % (64 // m.lanes) for m in morphs) and morphs[-1].lanes == 64
        _BYTE_POP.append((terrain, morphs))
    return _BYTE_POP[0]


def make_env(morphs, wide=False, options=None, flags=CONT, seed=5):
    """BatchedModular2D holding `morphs` in an interleaved population order -> (env, rows per morph)"""
    from gym_rem2d_amd.env import BatchedModular2D
    n = sum(m.n_envs for m in morphs)
    order = np.random.default_rng(seed).permutation(n)
    rows, at = [], 0
    for m in morphs:
        rows.append(order[at:at + m.n_envs])
        at += m.n_envs
    env = BatchedModular2D(seed=4, flags=flags, wide=wide, options=options)
    env._upload([(m, r) for m, r in zip(morphs, rows)], n)
    return env, rows


def world_rows(env):
    return [idx.cpu().numpy() for _, idx in env.worlds]


def make_mask(env, seed=3):
    """About 40 % of the population: each world's first and last creature, all of each world's first wavefront, and (worlds of three
    or more wavefronts) none of its second -> uint8 [N]"""
    rng = np.random.default_rng(seed)
    mask = np.zeros(env.n_envs, np.uint8)
    whole = none = 0
    for (w, _), rows in zip(env.worlds, world_rows(env)):
        per, n = 64 // w.lanes, w.n_envs
        loc = rng.random(n) < 0.3
        if n > per:
            loc[:per] = True
            whole += 1
        if n > 2 * per:
            loc[per:2 * per] = False
            none += 1
        loc[0] = loc[n - 1] = True
        mask[rows[loc]] = 1
    assert whole >= 3 and none >= 3 and 0.3 < mask.mean() < 0.55, (whole, none, mask.mean())
    return mask


def guarded_episodes(torch, env):
    """env.episodes with every buffer between two guards and prefilled with SENT (count: zero) -> {name: whole buffer}"""
    from gym_rem2d_amd.env import Episodes
    dev, n = env.worlds[0][0].device, env.n_envs
    ep, raw = Episodes(1, dev), {}
    for name, dtype in (("reward", torch.float32), ("done", torch.uint8), ("ended", torch.uint8), ("fitness", torch.float64),
                        ("steps", torch.int32), ("count", torch.int32)):
        raw[name] = torch.full((n + 2 * GUARD,), SENT[name], dtype=dtype, device=dev)
        inner = raw[name][GUARD:GUARD + n]
        if name == "count":
            inner.zero_()
        setattr(ep, name, inner.view(torch.bool) if dtype == torch.uint8 else inner)
    env._episodes, env._episode_args = ep, None
    return raw


def harvest(raw):
    """{name: inner host array}, after checking the guards"""
    out = {}
    for name, buf in raw.items():
        a = buf.cpu().numpy()
        assert (a[:GUARD] == a.dtype.type(SENT[name])).all() and (a[-GUARD:] == a.dtype.type(SENT[name])).all(), "guards of `%s`" % name
        out[name] = a[GUARD:-GUARD].copy()
    return out


def pop_field(env, name):
    """a per-creature field of every world in population order (host)"""
    out = None
    for (w, _), rows in zip(env.worlds, world_rows(env)):
        v = w.view(name).cpu().numpy()
        out = np.zeros(env.n_envs, v.dtype) if out is None else out
        out[rows] = v
    return out


def arenas(env):
    """the whole arena of every world still in use (compact() releases those it has emptied), as host bytes"""
    return [LF.arena_bytes(w) for wi, (w, _) in enumerate(env.worlds) if wi not in env._inactive]


def expected_arena(w, before, fresh, loc):
    """`before` with every field element of the creatures `loc` (bool [n_envs]) taken from `fresh`: whole-arena bytes"""
    from gym_rem2d_amd import _lib
    exp = before.copy()
    at = np.flatnonzero(loc)
    Np, K = w.n_envs_padded, w.lanes
    for name in _lib.FIELDS:
        off, cnt, esz = LF.field_place(w, name)
        dt = np.uint32 if esz == 4 else np.uint64
        e, f = exp[off:off + cnt * esz].view(dt), fresh[off:off + cnt * esz].view(dt)
        if cnt == Np * K:
            e.reshape(Np, K)[at] = f.reshape(Np, K)[at]
        elif cnt == Np * K * w.contact_slots:
            e.reshape(w.contact_slots, Np, K)[:, at] = f.reshape(w.contact_slots, Np, K)[:, at]
        else:
            assert cnt == Np
            e[at] = f[at]
    return exp


def differing_fields(w, a, b):
    from gym_rem2d_amd import _lib
    out = []
    for name in _lib.FIELDS:
        off, cnt, esz = LF.field_place(w, name)
        if a[off:off + cnt * esz].tobytes() != b[off:off + cnt * esz].tobytes():
            out.append(name)
    for lo, hi in LF.gaps(w):
        if a[lo:hi].tobytes() != b[lo:hi].tobytes():
            out.append("gap %d..%d" % (lo, hi))
    return out


def same_creatures(env_a, env_b, pick, what):
    """every state field of the creatures `pick` (bool [N], population order) byte for byte; -> creatures compared"""
    from gym_rem2d_amd import _lib
    n = 0
    for (wa, _), (wb, _), rows in zip(env_a.worlds, env_b.worlds, world_rows(env_a)):
        sa, sb = read_state(wa), read_state(wb)
        loc = pick[rows]
        for f in _lib.FIELDS:
            a, b = (sa[f][:, loc], sb[f][:, loc]) if sa[f].ndim == 3 else (sa[f][loc], sb[f][loc])
            assert a.tobytes() == b.tobytes(), "%s: field %s of the %d-lane world differs" % (what, f, wa.lanes)
        n += int(loc.sum())
    return n


# ------------------------------------------------------------------------------------------------------------------- 5. image
def image_and_on(torch, wide, options, go_on):
    terrain, morphs = byte_population()
    envs = [make_env(morphs, wide, options)[0] for _ in range(3 if go_on else 2)]
    a, b = envs[0], envs[1]
    try:
        assert len(a.worlds) >= len(morphs) and {w.lanes for w, _ in a.worlds} == {2, 4, 8, 16, 64}
        mask = make_mask(a)
        a.step(SETTLE)
        before, fresh = arenas(a), arenas(b)
        pre = {f: pop_field(a, f) for f in ("reward", "done", "fitness", "steps")}
        out_before = (a._reward.clone(), a._done.clone(), [idx.clone() for _, idx in a.worlds])
        raw = guarded_episodes(torch, a)
        mask_dev = torch.from_numpy(mask).to(a.worlds[0][0].device)
        ended = a.reset_where(mask_dev if wide else mask_dev.view(torch.bool))      # (both mask dtypes are taken)
        assert ended.data_ptr() == a.episodes.ended.data_ptr() and ended.dtype == torch.bool
        after = arenas(a)
        moved = 0
        for (w, _), rows, bef, fre, aft in zip(a.worlds, world_rows(a), before, fresh, after):
            loc = mask[rows] != 0
            exp = expected_arena(w, bef, fre, loc)
            assert aft.tobytes() == exp.tobytes(), "%d-lane world: %s" % (w.lanes, differing_fields(w, aft, exp))
            moved += int((exp != bef).sum())
        assert moved > 1000                                                             # the call had something to undo
        assert torch.equal(a._reward, out_before[0]) and torch.equal(a._done, out_before[1])
        assert all(torch.equal(idx, old) for (_, idx), old in zip(a.worlds, out_before[2]))
        h = harvest(raw)
        sel = mask != 0
        assert np.array_equal(h["ended"], mask) and np.array_equal(h["count"], mask.astype(np.int32))
        assert h["reward"].tobytes() == pre["reward"].tobytes() and np.array_equal(h["done"], (pre["done"] != 0).astype(np.uint8))
        assert h["fitness"][sel].tobytes() == pre["fitness"][sel].tobytes() and np.array_equal(h["steps"][sel], pre["steps"][sel])
        assert (h["fitness"][~sel] == SENT["fitness"]).all() and (h["steps"][~sel] == SENT["steps"]).all()
        assert (pre["steps"] == SETTLE).all() and (pre["fitness"][sel] != 0).any()
        if not go_on:
            return
        c = envs[2]
        a.step(AFTER)
        b.step(AFTER)
        c.step(SETTLE)
        c.step(AFTER)
        n = same_creatures(a, b, sel, "reset in place against a fresh env")
        n += same_creatures(a, c, ~sel, "untouched against an env that never saw the call")
        assert n == a.n_envs
        assert pop_field(a, "steps")[sel].tolist() == [AFTER] * int(sel.sum())
        assert all(env.handover_failures() == 0 for env in envs)
    finally:
        for env in envs:
            env.close()


@pytest.mark.parametrize("build", list(BUILDS))
def test_image(gpu, build):
    """60 steps, then reset_where(mask) on about 40 %: every byte of every arena -- padding creatures and alignment gaps included --
    is the snapshot taken before the call, except the fields of the selected creatures, which are those of an env that was reset and
    never stepped.  The set_outputs arrays do not move; the harvest is the pre-call fields, between guards that stay whole."""
    image_and_on(gpu, BUILDS[build], None, False)


# ------------------------------------------------------------------------------------------------------------ 6. continuation
@pytest.mark.parametrize("form", list(FORMS))
def test_continuation(gpu, form):
    """... and 50 steps later the selected creatures are, in every byte of every field, where a fresh env is after 50 steps, the
    others where an env that never saw the call is after 110; no failed hand-over.  Six launch forms."""
    image_and_on(gpu, FORMS[form][0], FORMS[form][1], True)


def model_masks(mask, rows):
    return [mask[r] for r in rows]


def check_against_model(env, model, what):
    """the final state of every world against the model's worlds (replay.verdict, state_forge's left-out rule)"""
    from gym_rem2d_amd import _lib
    pair, solver = _lib.capacity(env.wide)[:2]
    over = model.over_capacity(pair, solver)
    assert sum(int(o.sum()) for o in over) <= int(F.LEFT_OUT_CAP * env.n_envs)
    bad = []
    for (w, _), loop, snap, o in zip(env.worlds, model.loops, model.snapshots(), over):
        bits = np.zeros(loop.ctx.N, np.int32)
        bad += verdict(loop.ctx, read_state(w), snap, ~o, bits, pair, "%s K=%d" % (what, loop.ctx.K))
    assert not bad, "\n".join(bad)
    assert env.handover_failures() == 0


def test_continuation_against_the_model(gpu, oracle):
    """the same protocol on the L-system loop population, default build, against the episode model: the whole visible state"""
    torch = gpu
    from env_harness import make_env as loop_env
    env, rows, _ = loop_env("lsystem")
    try:
        mask = make_mask(env)
        model = EM.EpisodeModel(oracle, "lsystem")
        model.step(SETTLE)
        env.step(SETTLE)
        want = model.reset_where(model_masks(mask, rows))
        ended = env.reset_where(torch.from_numpy(mask).to("cuda")).cpu().numpy()
        for r, e in zip(rows, want):
            assert np.array_equal(ended[r], e)
        model.step(AFTER)
        env.step(AFTER)
        check_against_model(env, model, "after reset_where")
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------- 7. / 8. device conditions
def by_rows(per_bucket, rows, n):
    out = np.zeros(n, per_bucket[0].dtype)
    for v, r in zip(per_bucket, rows):
        out[r] = v
    return out


def follow_model(torch, env, rows, run, n_steps, step, what):
    """n_steps x step(env) -> ended; after every one `ended` equals the model's, and at every end fitness and steps do (==)"""
    n, ends = env.n_envs, 0
    ep = env.episodes
    for t in range(n_steps):
        ended = step(env).cpu().numpy()
        want = by_rows(run["ended"][t], rows, n)
        assert np.array_equal(ended, want), "%s step %d: ended differs at rows %s" % (what, t + 1, np.flatnonzero(ended != want)[:8])
        if want.any():
            fit, steps = ep.fitness.cpu().numpy(), ep.steps.cpu().numpy()
            assert fit[want].tobytes() == by_rows(run["fitness"][t], rows, n)[want].tobytes(), "%s step %d: fitness" % (what, t + 1)
            assert np.array_equal(steps[want], by_rows(run["steps"][t], rows, n)[want]), "%s step %d: steps" % (what, t + 1)
            ends += int(want.sum())
    assert np.array_equal(ep.count.cpu().numpy(), by_rows(run["count"], rows, n))
    return ends


def test_done_condition_open_loop(gpu, oracle):
    """320 x (step(1), reset_where(when=("done",))) on the L-system loop population: the model's `ended` after every step, its
    fitness and steps at every end, its episode counts and its worlds' state at the finish"""
    torch = gpu
    from env_harness import make_env as loop_env
    run = EM.run(oracle, "lsystem", EM.N_OPEN, ("done",))
    env, rows, _ = loop_env("lsystem")
    try:
        def step(env):
            env.step(1)
            return env.reset_where(when=("done",))
        ends = follow_model(torch, env, rows, run, EM.N_OPEN, step, "done")
        count = env.episodes.count.cpu().numpy()
        assert ends == int(count.sum()) and (count >= 1).all() and (count >= 2).sum() >= 100
        check_against_model(env, run["model"], "done, 320 steps")
    finally:
        env.close()


def test_steps_condition(gpu, oracle):
    """when = ("steps",), max_steps 60, 130 steps: everyone has ended exactly twice and stands 10 steps into a third episode"""
    torch = gpu
    from env_harness import make_env as loop_env
    run = EM.run(oracle, "lsystem", EM.N_TIMED, ("steps",), EM.TIMED_STEPS)
    env, rows, _ = loop_env("lsystem")
    try:
        def step(env):
            env.step(1)
            return env.reset_where(when=("steps",), max_steps=EM.TIMED_STEPS)
        follow_model(torch, env, rows, run, EM.N_TIMED, step, "steps")
        assert (env.episodes.count.cpu().numpy() == 2).all() and (env.episodes.steps.cpu().numpy() == EM.TIMED_STEPS).all()
        assert (pop_field(env, "steps") == 10).all()
        check_against_model(env, run["model"], "steps, 130 steps")
    finally:
        env.close()


def test_conditions_under_a_mask(gpu, oracle):
    """when = ("done", "steps"), max_steps 100, and a mask that exempts every third creature: the others follow the model, the exempt
    ones are, byte for byte, where a plain 320-step run leaves them"""
    torch = gpu
    from env_harness import make_env as loop_env
    env, rows, _ = loop_env("lsystem")
    plain, _, _ = loop_env("lsystem")
    try:
        mask = (np.arange(env.n_envs) % 3 != 0).astype(np.uint8)
        run = EM.run(oracle, "lsystem", EM.N_OPEN, ("done", "steps"), 100, masks=model_masks(mask, rows))
        mask_dev = torch.from_numpy(mask).to("cuda")

        def step(env):
            env.step(1)
            return env.reset_where(mask_dev, when=("done", "steps"), max_steps=100)
        follow_model(torch, env, rows, run, EM.N_OPEN, step, "masked")
        count = env.episodes.count.cpu().numpy()
        assert (count[mask == 0] == 0).all() and (count[mask != 0] >= 3).all()
        plain.step(EM.N_OPEN)
        assert same_creatures(env, plain, mask == 0, "exempt creatures against a plain run") == int((mask == 0).sum())
        assert (pop_field(env, "steps")[mask == 0] == EM.N_OPEN).all()
        check_against_model(env, run["model"], "masked, 320 steps")
    finally:
        env.close()
        plain.close()


def test_frozen_condition_under_eval_flags(gpu, oracle):
    """when = ("frozen",) under evaluate.EVAL_FLAGS (REM2D_FLAG_SKIP_FROZEN): each time a creature ends, the harvested fitness is
    oracle.batch_run's fitness of that creature, after the model's number of steps.  (Fitness and steps only: the oracle does not
    define the state of a frozen creature under SKIP_FROZEN -- but none stays frozen here beyond the call that follows its step.)"""
    torch = gpu
    from env_harness import make_env as loop_env
    from gym_rem2d_amd import evaluate
    run = EM.run(oracle, "lsystem", EM.N_OPEN, ("frozen",))
    env, rows, morphs = loop_env("lsystem", flags=evaluate.EVAL_FLAGS)
    try:
        ot = F.oracle_terrain(oracle, M.loop_population("lsystem")[0])
        final = by_rows([oracle.batch_run(ot, m.as_dict(), EM.N_OPEN, n_threads=4, flags=CONT)["fitness"] for m in morphs], rows, env.n_envs)
        seen = np.zeros(env.n_envs, int)

        def step(env):
            env.step(1)
            ended = env.reset_where(when=("frozen",))
            e = ended.cpu().numpy()
            if e.any():
                assert env.episodes.fitness.cpu().numpy()[e].tobytes() == final[e].tobytes()
                seen[e] += 1
            return ended
        follow_model(torch, env, rows, run, EM.N_OPEN, step, "frozen")
        assert (seen >= 1).all() and (seen >= 2).sum() >= 100
        assert env.handover_failures() == 0
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------------------- 9. auto-reset
def world_bytes(env):
    from gym_rem2d_amd import _lib
    out = []
    for wi, (w, idx) in enumerate(env.worlds):
        if wi not in env._inactive:
            st = read_state(w)
            out.append((w.lanes, idx.cpu().numpy(), {f: st[f] for f in _lib.FIELDS}))
    return out


def same_worlds(a, b, what):
    assert len(a) == len(b), what
    for (la, ia, fa), (lb, ib, fb) in zip(a, b):
        assert la == lb and np.array_equal(ia, ib), what
        for f in fa:
            assert fa[f].tobytes() == fb[f].tobytes(), "%s: field %s of the %d-lane world differs" % (what, f, la)


def same_episodes(a, b, what):
    from gym_rem2d_amd.env import Episodes
    for f in Episodes.FIELDS:
        x, y = getattr(a.episodes, f).cpu().numpy(), getattr(b.episodes, f).cpu().numpy()
        assert x.tobytes() == y.tobytes(), "%s: episodes.%s differs" % (what, f)


def test_autoreset_is_the_loop_by_hand(gpu):
    """set_autoreset + step_policy(90) == 90 x (act(), step(1), reset_where()) in every field of every world and every `episodes`
    buffer, on the permuted four-bucket x three-step-group population of test_policy_gpu's three-ways test; the values returned are
    the terminal step's (-100 / True where `done` ended the episode) while the arena already holds the new episode's zeros; with
    set_autoreset(None) step_policy is act + step again."""
    torch = gpu
    from gym_rem2d_amd import policy, synthetic
    from gym_rem2d_amd.env import BatchedModular2D
    specs = synthetic.lsystem_specs(range(260))
    n = len(specs)
    perm = np.random.default_rng(9).permutation(n)
    pol = policy.MLPPolicy.random(n, 16, 32, seed=21).take(perm)
    WHEN, LIMIT = ("done", "steps"), 80

    def make():
        env = BatchedModular2D(seed=4, flags=CONT)
        env.step_groups = 3
        env.reset_specs([specs[i] for i in perm])
        env.set_policy(pol)
        return env
    envs = [make() for _ in range(4)]
    a, b, c, d = envs
    try:
        assert len(a.groups) >= 2 and len({w.lanes for w, _ in a.worlds}) >= 3
        a.set_autoreset(WHEN, LIMIT)
        r, dn = a.step_policy(90)
        assert r.data_ptr() == a.episodes.reward.data_ptr() and dn.data_ptr() == a.episodes.done.data_ptr() and dn.dtype == torch.bool
        terminal = by_done = 0
        for t in range(90):
            b.act()
            b.step(1)
            ended = b.reset_where(when=WHEN, max_steps=LIMIT).cpu().numpy()
            done, reward = b.episodes.done.cpu().numpy(), b.episodes.reward.cpu().numpy()
            hit = ended & done
            assert (reward[hit] == -100.0).all() and not (pop_field(b, "done")[ended] != 0).any() and (pop_field(b, "reward")[ended] == 0).all()
            assert not (done & ~ended).any() and (b.episodes.steps.cpu().numpy()[ended & ~done] == LIMIT).all()
            assert (pop_field(b, "steps")[~ended] < LIMIT).all()
            terminal, by_done = terminal + int(ended.sum()), by_done + int(hit.sum())
        print("auto-reset: %d episodes ended, %d of them by `done`" % (terminal, by_done))
        assert by_done >= 1 and terminal >= n
        same_worlds(world_bytes(a), world_bytes(b), "step_policy under auto-reset against the loop by hand")
        same_episodes(a, b, "auto-reset")
        assert r.cpu().numpy().tobytes() == b.episodes.reward.cpu().numpy().tobytes() and torch.equal(dn.cpu(), b.episodes.done.cpu())
        # ... and switched off (or never on): act + step, as before
        a.set_autoreset(None)
        c.set_autoreset(WHEN, LIMIT)
        c.set_autoreset(None)
        for env in (c, d):
            assert env._autoreset is None
        rc = c.step_policy(30)
        for _ in range(30):
            d.act()
            rd = d.step(1)
        same_worlds(world_bytes(c), world_bytes(d), "step_policy without auto-reset")
        assert torch.equal(rc[0], rd[0]) and torch.equal(rc[1], rd[1]) and c._episodes is None
        assert (pop_field(c, "steps") == 30).all()
    finally:
        for env in envs:
            env.close()


def population_policy(torch, policy_mod, weights, rows, n):
    """the buckets' per-creature weight sets (policy_model.loop_weights) as one policy in population order"""
    arrays = []
    for k in range(4):
        a = np.zeros((n,) + weights[0][k].shape[1:], np.float32)
        for W, r in zip(weights, rows):
            a[r] = W[k]
        arrays.append(torch.from_numpy(a))
    return policy_mod.MLPPolicy(*arrays)


def test_autoreset_against_the_policy_model(gpu, oracle):
    """200 x step_policy(1) under set_autoreset(("done", "steps"), 150) on the L-system loop population, every creature under its own
    MLP: `ended`, fitness and steps of the policy form of the model, ==; the state at the finish"""
    torch = gpu
    from env_harness import make_env as loop_env
    from gym_rem2d_amd import policy
    run = EM.run(oracle, "lsystem", EM.N_POLICY, ("done", "steps"), 150, policy=True)
    env, rows, _ = loop_env("lsystem")
    try:
        env.set_policy(population_policy(torch, policy, run["model"].weights, rows, env.n_envs))
        env.set_autoreset(("done", "steps"), 150)

        def step(env):
            r, d = env.step_policy(1)
            assert d.data_ptr() == env.episodes.done.data_ptr()
            return env.episodes.ended
        ends = follow_model(torch, env, rows, run, EM.N_POLICY, step, "policy")
        assert ends >= env.n_envs
        check_against_model(env, run["model"], "policy, 200 steps")
    finally:
        env.close()


# --------------------------------------------------------------------------------------------- 10. nothing selected, the edges
def test_nothing_selected_changes_nothing(gpu):
    """a zero mask, and when = ("done",) right after a reset and after 20 steps in which nobody ends: no byte of any arena moves and
    `ended` is 0 everywhere; after compact() the call raises and changes nothing"""
    torch = gpu
    terrain, morphs = byte_population()
    env, _ = make_env(morphs)
    try:
        n = env.n_envs
        zero = torch.zeros(n, dtype=torch.uint8, device="cuda")
        for stage in range(2):
            before = arenas(env)
            raw = guarded_episodes(torch, env)
            for kw in (dict(mask=zero), dict(when=("done",)), dict(mask=zero, when=("done", "frozen", "steps"), max_steps=1)):
                ended = env.reset_where(**kw)
                assert not ended.any()
                assert all(x.tobytes() == y.tobytes() for x, y in zip(before, arenas(env))), (stage, kw)
            h = harvest(raw)
            assert not h["ended"].any() and not h["count"].any() and (h["steps"] == SENT["steps"]).all()
            assert h["reward"].tobytes() == pop_field(env, "reward").tobytes()
            env.step(20)
        for w, _ in env.worlds:
            w.view("frozen")[::2] = 1
        env.compact(min_envs=1, max_alive=1.0)
        before = arenas(env)
        with pytest.raises(ValueError, match=r"compact\(\)"):
            env.reset_where(when=("frozen",))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(before, arenas(env)))
    finally:
        env.close()


def abi_call(torch, worlds, mask, when, max_steps, out, n_rows):
    """rem2d_worlds_reset_where itself on a list of BatchedWorld"""
    from gym_rem2d_amd import _lib
    morphs = (_lib.Morph * len(worlds))()
    for m, w in zip(morphs, worlds):
        for k in _lib.MORPH_FIELDS:
            setattr(m, k, w._morph_dev[k].data_ptr())
    w0 = worlds[0]
    _lib.check(w0.L.rem2d_worlds_reset_where(_lib.world_array(worlds), morphs, len(worlds), None if mask is None else mask.data_ptr(),
                                             when, max_steps, None if out is None else C.byref(out), n_rows, w0._stream()), w0.wide)


def test_fewer_rows_than_creatures_and_more_worlds_than_a_table(gpu):
    """Through the ABI: 19 small worlds (more than the 16 of one launch's table; chains of 8 lanes, 3 creatures each, and 5 L-system
    creatures of 4 lanes in every third) under one population index, 30 steps, all-ones mask, n_rows = 40 of 69 -- the creatures of
    rows below 40 are a fresh world's, those beyond have not moved by a byte and nothing was harvested for them; no `out` at all and
    members left NULL are fine."""
    torch = gpu
    from gym_rem2d_amd import _lib, make_terrain, synthetic
    from gym_rem2d_amd.compiler import Morphology
    from gym_rem2d_amd.world import BatchedWorld
    terrain = make_terrain(4)
    small = Morphology.from_specs([s for s in synthetic.lsystem_specs(range(60)) if 3 <= s.n_bodies <= 4][:5], 4)
    morphs = [small if i % 3 == 2 else synthetic.chain_population(3, 8, "left") for i in range(19)]
    n = sum(m.n_envs for m in morphs)
    assert n == 69
    order = np.random.default_rng(2).permutation(n)
    reward, done = torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.bool, device="cuda")

    def make():
        worlds, rows, at = [], [], 0
        for m in morphs:
            w = BatchedWorld(m.n_envs, m.lanes, CONT)
            w.set_terrain(terrain)
            w.reset(m)
            rows.append(order[at:at + m.n_envs])
            w.set_outputs(reward, done, torch.from_numpy(rows[-1].astype(np.int32)).to("cuda"))
            worlds.append(w)
            at += m.n_envs
        return worlds, rows
    stepped, rows = make()
    fresh, _ = make()
    try:
        for w in stepped:
            w.step(30)
        before = [LF.arena_bytes(w) for w in stepped]
        N_ROWS = 40
        ones = torch.ones(n, dtype=torch.uint8, device="cuda")
        out = _lib.EpisodeOut()
        ended = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
        steps = torch.full((n,), -77, dtype=torch.int32, device="cuda")
        out.ended, out.steps = ended.data_ptr(), steps.data_ptr()                       # the other four stay NULL
        abi_call(torch, stepped, ones, 0, 0, out, N_ROWS)
        for w, f, r, bef in zip(stepped, fresh, rows, before):
            exp = expected_arena(w, bef, LF.arena_bytes(f), r < N_ROWS)
            aft = LF.arena_bytes(w)
            assert aft.tobytes() == exp.tobytes(), differing_fields(w, aft, exp)
        e, s = ended.cpu().numpy(), steps.cpu().numpy()
        assert (e[:N_ROWS] == 1).all() and (e[N_ROWS:] == 0xA5).all() and (s[:N_ROWS] == 30).all() and (s[N_ROWS:] == -77).all()
        # no `out`: the same selection by condition -- everybody below row 40 stands at step 0 now, so nobody is selected
        before = [LF.arena_bytes(w) for w in stepped]
        abi_call(torch, stepped, None, _lib.WHEN["steps"], 30, None, N_ROWS)
        assert all(LF.arena_bytes(w).tobytes() == b.tobytes() for w, b in zip(stepped, before))
        abi_call(torch, stepped, None, _lib.WHEN["steps"], 30, None, n)              # ... and with every row in range the rest follows
        for w, f in zip(stepped, fresh):
            assert LF.arena_bytes(w).tobytes() == expected_arena(w, LF.arena_bytes(w), LF.arena_bytes(f), np.ones(w.n_envs, bool)).tobytes()
        assert all(int(w.view("steps").max()) == 0 for w in stepped)
    finally:
        for w in stepped + fresh:
            w.close()


def test_graph_replay_after_reset_where(gpu):
    """REM2D_STEP_GRAPH: a step call replayed as a captured graph after a reset_where gives the bytes of the unreplayed call"""
    torch = gpu
    terrain, morphs = byte_population()
    envs = [make_env(morphs)[0] for _ in range(2)]
    a, b = envs
    try:
        a.use_graph = True
        assert len(a.worlds) > 1 and not b.use_graph
        mask = torch.from_numpy(make_mask(a)).to("cuda")
        for env in envs:
            env.step(10)                      # a: captured
            env.step(10)                      # a: replayed
            env.reset_where(mask)
            env.step(10)                      # a: replayed again, on creatures that were reset in between
            env.reset_where(when=("steps",), max_steps=10)
            env.step(10)
        same_worlds(world_bytes(a), world_bytes(b), "graph replay")
        same_episodes(a, b, "graph replay")
        assert sorted(set(pop_field(a, "steps").tolist())) == [10]
        assert all(env.handover_failures() == 0 for env in envs)
    finally:
        for env in envs:
            env.close()
