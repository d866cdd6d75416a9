"""Device policies on a real MI355X (pytest -m gpu): the forward kernel against tests/policy_model.py on forged inputs, in the three
builds, and the closed loop `act()` / `step_policy()` against the oracle (include/rem2d_policy.h).  Every comparison is on bits:
``view(uint64)`` of the targets (NaNs mapped to one pattern first: policy_model.bits says why), bytes of `valid`."""
import numpy as np
import pytest

import control_model as M
import policy_model as PM
import state_forge as F

pytestmark = pytest.mark.gpu

CONT = 1
f32 = np.float32
BUILDS = (False, True, "fma")
SHAPES = [(1, 0, 1), (4, 3, 5), (16, 10, 32), (16, 0, 33), (64, 64, 128)]       # (MB, R, H)
ROWS = (1, 63, 64, 65, 257)
GUARD = 64                                   # guard words in front of and behind every output buffer
T_SENTINEL, V_SENTINEL = -12345.678, 0xA5


@pytest.fixture(scope="module")
def gpu():
    import replay
    return replay.need_gpu()


# ------------------------------------------------------------------------------------------------------------------ the forge
def _sprinkle(rng, a, share, values):
    """put `values` at a `share` of the entries of a (in place)"""
    flat = a.reshape(-1)
    at = rng.choice(flat.size, size=max(1, int(share * flat.size)), replace=False)
    flat[at] = rng.choice(np.asarray(values, f32), size=len(at))
    return a


TINY = [1e-20, -3e-23, 1e-38, 2e-42, -1.4e-45, 7e-30]                    # products and sums of these are denormals
ODD = [-0.0, 0.0, 1e-39, -5e-41]                                         # -0 and denormals themselves


def forge(MB, R, H, N, mode, seed):
    """Inputs of one forge case: x [N, D], the weight arrays [G, ...], index or None, row mask or None.  A normal bulk; in x, the
    weights and the biases -0 and denormals everywhere, tiny values whose products are denormals, and NaN / +-inf where they poison
    a row, a unit or an output column rather than everything (shared sets serve every row)."""
    rng = np.random.default_rng([MB, R, H, N, seed])
    D = M.width(MB) + R
    G = {"per_row": N, "shared": 1, "indexed": 7}[mode]
    x = rng.standard_normal((N, D)).astype(f32)
    w1, b1 = (rng.standard_normal((G, D, H)) * 0.3).astype(f32), (rng.standard_normal((G, H)) * 0.3).astype(f32)
    w2, b2 = (rng.standard_normal((G, H, MB)) * 0.5).astype(f32), (rng.standard_normal((G, MB)) * 0.3).astype(f32)
    for a in (x, w1, b1, w2, b2):
        _sprinkle(rng, a, 0.03, ODD)
        _sprinkle(rng, a, 0.03, TINY)
    special = [np.nan, np.inf, -np.inf]
    for r in range(0, N, 5):                                             # every fifth row senses something that is not a number
        x[r, rng.integers(D)] = special[(r // 5) % 3]
    for r in range(2, N, 9):                                             # a row of tiny inputs: denormal products all the way
        x[r] = (x[r] * f32(1e-22)).astype(f32)
    if mode == "per_row":                                                # a creature's own weights may be anything
        for g in range(1, G, 4):
            (w1, b1, w2, b2)[(g // 4) % 4][g].reshape(-1)[rng.integers(min(H, MB))] = special[(g // 4) % 3]
    else:                                                                # shared sets: one output column each
        for g in range(G):                                               # (with a single column: every other set, never the only one)
            if MB > 1 or (g % 2 == 1):
                w2[g, rng.integers(H), rng.integers(MB)] = special[g % 3]
            if MB > 1:
                b2[g, (g + 1) % MB] = special[(g + 1) % 3]
    index = mask = None
    if mode == "shared":
        index = np.zeros(N, np.int32)                                    # every row names the one set
    if mode == "indexed":
        index = rng.integers(0, G, N).astype(np.int32)                   # 7 sets: repeats from 8 rows on
        if N >= 3:
            index[rng.choice(N, 2, replace=False)] = (-1, G)             # two values that name no set
        mask = (rng.random(N) < 0.7).astype(np.uint8)
    return x, (w1, b1, w2, b2), index, mask


def _guarded(torch, n, dtype, fill, dev):
    """a buffer of n words between two guards, all `fill`"""
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _offset_copy(torch, a, off, dev):
    """`a` on the device, its base `off` words behind a fresh allocation's (4 bytes: no 16-byte load can be used on it)"""
    flat = torch.zeros(a.size + off, dtype=torch.float32, device=dev)
    flat[off:] = torch.from_numpy(a.reshape(-1)).to(dev)
    return flat[off:].view(*a.shape)


def run_forward(torch, policy_mod, MB, R, act, x, W, index, mask, wide, off):
    """-> (targets uint64 [N, MB], valid [N, MB]) after two calls that must agree, guards checked"""
    dev = torch.device("cuda:0")
    N = x.shape[0]
    w = [_offset_copy(torch, a, off, dev) for a in W]
    assert all(t.data_ptr() % 16 == (4 * off) % 16 for t in w)
    rays = None if R in (0, 10) else np.zeros((R, 2)) + 1.0
    pol = policy_mod.MLPPolicy(*w, activation=act, index=None if index is None else torch.from_numpy(index).to(dev), rays=rays)
    assert (pol.max_bodies, pol.n_rays, pol.hidden) == (MB, R, W[0].shape[2])
    xd = torch.from_numpy(x).to(dev)
    obs = xd[:, :M.width(MB)].contiguous()
    frac = xd[:, M.width(MB):].contiguous() if R else None
    md = None if mask is None else torch.from_numpy(mask).to(dev)
    outs = []
    for rep in range(2):
        tbuf, t = _guarded(torch, N * MB, torch.float64, T_SENTINEL, dev)
        vbuf, v = _guarded(torch, N * MB, torch.uint8, V_SENTINEL, dev)
        got = pol.forward(obs, frac, out=(t.view(N, MB), v.view(N, MB)), row_mask=md, wide=wide)
        assert got[0].data_ptr() == t.data_ptr()
        tb, vb = tbuf.cpu().numpy(), vbuf.cpu().numpy()
        for g in (tb[:GUARD], tb[-GUARD:]):
            assert (g == T_SENTINEL).all(), "guard words of `targets` overwritten"
        for g in (vb[:GUARD], vb[-GUARD:]):
            assert (g == V_SENTINEL).all(), "guard bytes of `valid` overwritten"
        outs.append((PM.bits(tb[GUARD:-GUARD].reshape(N, MB)), vb[GUARD:-GUARD].reshape(N, MB).copy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]), "two calls differ"
    return outs[0]


@pytest.mark.parametrize("act", [PM.SOFTSIGN, PM.RELU])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "MB%d-R%d-H%d" % s)
def test_forward_forge(gpu, shape, act):
    """rem2d_policy_forward == the model, bit for bit: five shapes x both activations (the ids), each over five row counts, three
    ways to own weights (per row; one shared set; 7 sets through an index with repeats, two out-of-range values and a row mask), the
    three builds, and weight bases 16-byte aligned and 4 bytes off.  Skipped rows keep the prefilled sentinel; guards stay whole."""
    torch = gpu
    from gym_rem2d_amd import policy
    MB, R, H = shape
    compared = invalid = skipped = 0
    for N in ROWS:
        for mode in ("per_row", "shared", "indexed"):
            x, W, index, mask = forge(MB, R, H, N, mode, 1)
            want_t, want_v = PM.forward_model(x, *W, act=act, index=index)
            run = PM.rows_run(N, W[0].shape[0], index, mask)
            want_t, want_v = PM.bits(want_t), want_v.copy()
            want_t[~run], want_v[~run] = np.array([T_SENTINEL]).view(np.uint64)[0], V_SENTINEL
            first = None
            for wide in BUILDS:
                for off in (0, 1):
                    got_t, got_v = run_forward(torch, policy, MB, R, act, x, W, index, mask, wide, off)
                    what = "N=%d %s build=%s offset=%d" % (N, mode, wide, off)
                    ne = got_t != want_t
                    assert not ne.any(), "%s: %d targets differ, first at %s: gpu %#x model %#x" % (
                        what, int(ne.sum()), tuple(np.argwhere(ne)[0]), got_t[tuple(np.argwhere(ne)[0])], want_t[tuple(np.argwhere(ne)[0])])
                    assert np.array_equal(got_v, want_v), what + ": validity bytes differ"
                    first = (got_t, got_v) if first is None else first
                    assert np.array_equal(got_t, first[0]) and np.array_equal(got_v, first[1]), what + ": the builds differ"
            compared += int(run.sum()) * MB
            invalid += int((want_v[run] == 0).sum())
            skipped += int((~run).sum())
    print("%s %s: %d targets per build compared, %d of them invalid, %d rows skipped" % (shape, act, compared, invalid, skipped))
    # the forge is no vacuous one: invalid targets, valid ones and skipped rows all occur
    assert 0 < invalid < compared and skipped > 0


# ------------------------------------------------------------------------------------------------- the closed loop and the oracle
PARITY = [("lsystem", False, None), ("cppn", False, None), ("direct", False, None), ("lsystem", True, None), ("direct", False, {"pipeline": 0})]


def _pid(c):
    return "%s%s%s" % (c[0], "-wide" if c[1] else "", "".join("-%s%d" % kv for kv in sorted((c[2] or {}).items())))


def population_policy(torch, policy_mod, runs, rows, n, act=PM.SOFTSIGN):
    """The buckets' per-creature weight sets as one policy in population order"""
    arrays = []
    for k in range(4):
        a = np.zeros((n,) + runs[0]["weights"][k].shape[1:], f32)
        for run, r in zip(runs, rows):
            a[r] = run["weights"][k]
        arrays.append(torch.from_numpy(a))
    return policy_mod.MLPPolicy(*arrays, activation=act)


@pytest.mark.parametrize("case", PARITY, ids=_pid)
def test_closed_loop_parity(gpu, oracle, case):
    """Both sides from reset, 120 steps: before every step act()'s targets and validity bytes equal the model on the ORACLE's state
    (so both sides' joints are told the same), at the end the whole visible state equals the oracle's, as test_control_gpu.py
    compares it, with its left-out rule; no failed hand-over."""
    torch = gpu
    pop, wide, options = case
    from gym_rem2d_amd import _lib, policy
    from env_harness import check_final, make_env, population_rows
    runs = PM.policy_loop_run(oracle, pop, CONT)
    env, rows, morphs = make_env(pop, wide, options)
    try:
        firsts = [M.left_out_first(run, *_lib.capacity(wide)[:2]) for run in runs]
        gone = sum(int((f < len(run["obs"])).sum()) for (f, _), run in zip(firsts, runs))
        assert gone <= int(F.LEFT_OUT_CAP * env.n_envs)
        Mb = PM.LOOP_BODIES
        first_pop = np.zeros(env.n_envs, np.int64)
        for (f, _), r in zip(firsts, rows):
            first_pop[r] = f
        env.set_policy(population_policy(torch, policy, runs, rows, env.n_envs))
        assert env.policy.max_bodies == Mb and env.policy.device.type == "cuda"
        compared = 0
        for t in range(PM.N_POLICY_LOOP):
            targets, valid = env.act()
            keep = first_pop > t
            want_t, want_v = population_rows(runs, rows, "targets", t, Mb), population_rows(runs, rows, "valid", t, Mb)
            got_t, got_v = PM.bits(targets.cpu().numpy()), valid.cpu().numpy()
            ne = (got_t != PM.bits(want_t)) & keep[:, None]
            assert not ne.any(), "act() before step %d: %d targets differ, first at %s" % (t, int(ne.sum()), tuple(np.argwhere(ne)[0]))
            assert np.array_equal(got_v[keep], want_v[keep])
            compared += int(keep.sum()) * Mb
            env.step(1)
        check_final(env, runs, firsts, _pid(case))
        assert env.handover_failures() == 0
        print("%s: %d targets compared over %d steps, %d creatures left out" % (_pid(case), compared, PM.N_POLICY_LOOP, gone))
    finally:
        env.close()


# --------------------------------------------------------------------------------------------------------- the same three ways
def _world_bytes(env):
    """every state field of every active world, as host arrays (one copy per world)"""
    from gym_rem2d_amd import _lib
    from replay import read_state
    out = []
    for wi, (w, idx) in enumerate(env.worlds):
        if wi in env._inactive:
            continue
        st = read_state(w)
        out.append((w.lanes, idx.cpu().numpy(), {f: st[f] for f in _lib.FIELDS}))
    return out


def _same_worlds(a, b, what):
    assert len(a) == len(b), what
    for (la, ia, fa), (lb, ib, fb) in zip(a, b):
        assert la == lb and np.array_equal(ia, ib), what
        for f in fa:
            assert fa[f].tobytes() == fb[f].tobytes(), "%s: field %s of the %d-lane world differs" % (what, f, la)


def test_three_ways_to_the_same_state(gpu):
    """step_policy(n) == n x (act(), step(1)) == n x (observe, sense_terrain, MLPPolicy.forward, set_joint_targets(mask=valid),
    step(1)): every state field of every world, byte for byte -- on a permuted population of four lane buckets x three step groups,
    30 steps, a compact() that retires every third creature, 30 steps more.  The unpermuted population under the unpermuted policy
    ends with the same observation rows, permuted."""
    torch = gpu
    from gym_rem2d_amd import policy, synthetic
    from gym_rem2d_amd.env import BatchedModular2D
    specs = synthetic.lsystem_specs(range(260))
    n = len(specs)
    perm = np.random.default_rng(9).permutation(n)
    base = policy.MLPPolicy.random(n, 16, 32, seed=21)

    def make(order, pol):
        env = BatchedModular2D(seed=4, flags=CONT)
        env.step_groups = 3
        env.reset_specs([specs[i] for i in order])
        env.set_policy(pol)
        return env

    def by_hand(env, steps):
        pol = env.policy
        for _ in range(steps):
            obs, frac = env.observe(pol.max_bodies), env.sense_terrain(pol.rays)
            targets, valid = pol.forward(obs, frac, out=hand_out, row_mask=hand_mask[0])
            env.set_joint_targets(targets, mask=valid)
            env.step(1)
    envs = [make(perm, base.take(perm)) for _ in range(3)] + [make(np.arange(n), base)]
    a, b, c, d = envs
    hand_out = (torch.zeros((n, 16), dtype=torch.float64, device="cuda"), torch.zeros((n, 16), dtype=torch.uint8, device="cuda"))
    hand_mask = [None]
    try:
        assert len(a.groups) >= 2 and len({w.lanes for w, _ in a.worlds}) >= 3
        for half in range(2):
            r, dn = a.step_policy(30)
            assert r.shape == (n,) and dn.shape == (n,)
            for _ in range(30):
                b.act()
                b.step(1)
            by_hand(c, 30)
            d.step_policy(30)
            wa = _world_bytes(a)
            _same_worlds(wa, _world_bytes(b), "act + step, half %d" % half)
            _same_worlds(wa, _world_bytes(c), "by hand, half %d" % half)
            oa, od = a.observe().cpu().numpy(), d.observe().cpu().numpy()
            assert np.array_equal(oa.view(np.uint32), od[perm].view(np.uint32))
            ta = a.act()[0].cpu().numpy()                    # (what act() computes is a function of the state: one more changes nothing)
            if half == 1:
                break
            for env, order in ((a, perm), (b, perm), (c, perm), (d, np.arange(n))):
                for w, idx in env.worlds:
                    w.view("frozen")[torch.from_numpy(order).to(idx.device)[idx] % 3 == 0] = 1
            alive = [env.compact(min_envs=1, max_alive=1.0) for env in envs]
            assert len(set(alive)) == 1 and alive[0] <= n - len(range(0, n, 3))
            live = np.zeros(n, np.uint8)
            for wi, (w, idx) in enumerate(c.worlds):
                if wi not in c._inactive:
                    live[idx.cpu().numpy()] = 1
            hand_mask[0] = torch.from_numpy(live).to("cuda")
            # after compact() the rows no live world holds are masked out of act()'s forward pass: they keep their last targets
            before = a._policy["targets"].clone()
            a._policy["targets"][torch.from_numpy(live == 0).to("cuda")] = 77.0
            got = a.act()[0].cpu().numpy()
            assert (got[live == 0] == 77.0).all() and (got[live == 1] != 77.0).all() and int((live == 0).sum()) >= n // 3
            a._policy["targets"].copy_(before)
            a.act()
            assert np.array_equal(PM.bits(ta[live == 1]), PM.bits(a._policy["targets"].cpu().numpy()[live == 1]))
    finally:
        for env in envs:
            env.close()


def _observe_rows(env):
    return env.observe().clone().cpu().numpy().view(np.uint32)


def test_nan_weight_leaves_the_creature_to_its_oscillators(gpu):
    """One NaN in one creature's weight set: all its targets are invalid, its joints stay under their own oscillators -- it ends
    where it ends without any policy -- and everybody else ends where they end under the clean policy."""
    torch = gpu
    from gym_rem2d_amd import policy, synthetic
    from gym_rem2d_amd.env import BatchedModular2D
    specs = [s for s in synthetic.lsystem_specs(range(200)) if s.n_bodies >= 3][:48]
    n, victim = len(specs), 17
    clean = policy.MLPPolicy.random(n, 16, 32, seed=5)
    w1 = clean.w1.clone()
    w1[victim, 40, 7] = float("nan")
    dirty = policy.MLPPolicy(w1, clean.b1, clean.w2, clean.b2)
    envs = []
    try:
        for pol in (clean, dirty, None):
            env = BatchedModular2D(seed=4, flags=CONT)
            env.reset_specs(specs)
            env.set_policy(pol)
            envs.append(env)
        a, b, c = envs
        a.step_policy(50)
        b.step_policy(50)
        c.step(50)
        valid = b.act()[1].cpu().numpy()
        assert not valid[victim].any() and valid[np.arange(n) != victim].all()
        oa, ob, oc = (_observe_rows(e) for e in envs)
        others = np.arange(n) != victim
        assert np.array_equal(ob[others], oa[others]) and np.array_equal(ob[victim], oc[victim])
        assert not np.array_equal(oa[victim], oc[victim]) and (oa[others] != oc[others]).any(axis=1).mean() > 0.9
        # its controller words are its oscillator's still: nothing was written to them
        seen = 0
        for (wb, ib), (wc, ic) in zip(b.worlds, c.worlds):
            assert np.array_equal(ib.cpu().numpy(), ic.cpu().numpy())
            for e in np.flatnonzero(ib.cpu().numpy() == victim):
                for f in ("camp", "cphase", "cfreq", "coffset"):
                    assert wb.view(f)[e].cpu().numpy().tobytes() == wc.view(f)[e].cpu().numpy().tobytes(), f
                assert (wb.view("camp")[e].cpu().numpy() != 0).any()
                seen += 1
        assert seen == 1
    finally:
        for env in envs:
            env.close()


def test_run_policy_episode_gives_the_oracles_fitness(gpu, oracle):
    """evaluate.run_policy_episode on 64 L-system creatures, 150 steps in chunks of 50: the fitness of the oracle loop"""
    torch = gpu
    from gym_rem2d_amd import evaluate, make_terrain, policy, synthetic
    from gym_rem2d_amd.compiler import Morphology, lanes_for
    from gym_rem2d_amd.env import BatchedModular2D
    specs = [s for s in synthetic.lsystem_specs(range(120)) if s.n_bodies >= 2][:64]
    groups = {}
    for e, s in enumerate(specs):
        groups.setdefault(lanes_for(s.n_bodies), []).append(e)
    batches = [(Morphology.from_specs([specs[e] for e in groups[k]], k), groups[k]) for k in sorted(groups)]
    terrain = make_terrain(4)
    steps = 150
    runs = PM.policy_loop_run(oracle, "episode64", CONT, n_steps=steps, morphs=[m for m, _ in batches], terrain=terrain,
                              key=("episode64", steps))
    rows = [np.asarray(idx) for _, idx in batches]
    env = BatchedModular2D(seed=4, flags=evaluate.EVAL_FLAGS)
    try:
        env.reset_batches(batches, len(specs))
        env.set_policy(population_policy(torch, policy, runs, rows, len(specs)))
        fit = evaluate.run_policy_episode(env, max_steps=steps, chunk=50).cpu().numpy()
        want = np.zeros(len(specs))
        gone = np.zeros(len(specs), bool)
        for run, r in zip(runs, rows):
            want[r] = run["fitness"]
            gone[r] = M.left_out_first(run)[0] < len(run["obs"])
        assert not gone.any() and fit.dtype == np.float64
        assert np.array_equal(fit.view(np.uint64), want.view(np.uint64)) and (want > 0).sum() >= 8
        assert env.last_episode is None and int(env.steps.max()) == steps
    finally:
        env.close()


def test_gym_facade_with_a_policy(gpu):
    """Modular2D(closed_loop=True, policy=...): step(None) acts by the policy -- the joints carry the model's targets of the
    observation just returned -- and an explicit action still wins."""
    import copy
    import random
    torch = gpu
    import range_model as R
    from gym_rem2d_amd import get_module_list, policy
    from gym_rem2d_amd.compiler import build_creature
    from gym_rem2d_amd.encodings import DirectEncoding
    from gym_rem2d_amd.env import Modular2D
    Mb = 16
    for seed in range(40):
        random.seed(seed)
        ml = get_module_list()
        tree = copy.deepcopy(DirectEncoding(ml).create(6))
        if 3 <= build_creature(copy.deepcopy(tree).getNodes(), ml)[0].n_bodies <= Mb:
            break
    else:
        raise AssertionError("no suitable tree")
    pol = policy.MLPPolicy.random(1, Mb, 32, seed=8)
    W = tuple(t.numpy() for t in (pol.w1, pol.b1, pol.w2, pol.b2))
    env = Modular2D(closed_loop=True, max_bodies=Mb, policy=pol)
    try:
        env.seed(4)
        obs = env.reset(tree=tree, module_list=ml)
        batch, world = env._batch, env._batch.worlds[0][0]
        T = R.Terrain.of(batch._terrain())
        nb = len(env.robot.components)
        lanes = np.flatnonzero(world.view("shape")[0].cpu().numpy() != 0)
        for t in range(20):
            frac = R.cast(T, obs[0:1], obs[1:2], R.bipedal_rays())[0]
            want, valid = PM.forward_model(PM.input_rows(obs[None], frac), *W)
            assert valid.all()
            obs, r, d, info = env.step(None)
            amp, off = world.view("camp")[0].cpu().numpy(), world.view("coffset")[0].cpu().numpy()
            assert (amp[lanes[1:]] == 0.0).all() and np.array_equal(off[lanes[1:]].view(np.uint64), want[0, 1:nb].view(np.uint64))
        action = np.linspace(-1.0, 1.0, Mb)
        env.step(action)
        assert np.array_equal(world.view("coffset")[0].cpu().numpy()[lanes[1:]], action[1:nb])
    finally:
        env.close()
