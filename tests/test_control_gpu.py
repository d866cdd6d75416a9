"""Closed-loop control on a real MI355X (pytest -m gpu): `observe`, `set_joint_targets` and `set_controllers` against the oracle,
every comparison with `==` (include/rem2d_control.h, tests/control_model.py).

Closed-loop parity: both sides start from reset; before every step the targets of control_model.policy (a host function of the
step and of the MODEL's observation rows, binary64) are written on both sides -- the oracle through World.set_controller(q, 0,
phase, freq, target, i_state), the GPU through set_joint_targets.  `observe()` must equal the model of the oracle's state after
reset and after each of the control_model.N_LOOP = 300 steps (so the policy would have computed the same targets from the GPU's
rows), and at the end the whole visible state is compared as the injected-state tests compare it: poses, velocities, joint and
contact impulses, pair lists, reward, done, fitness, wall of death.

As there, a creature leaves the comparison from the step on at which the ORACLE shows one of its bodies beyond the build's pair /
solver slots (tests/test_control_host.py caps them at 2 % of a population); it must then carry that capacity bit, and nobody else
any error bit.
"""
import numpy as np
import pytest

import control_model as M
import state_forge as F
from env_harness import check_final, make_env, population_rows
from replay import need_gpu, read_state

pytestmark = pytest.mark.gpu

CONT = 1
# (population, build, launch options): rough terrain for all but cppn, which runs the hardcore track; continuous physics
PARITY = [("lsystem", False, None), ("direct", False, None), ("chain8", False, None), ("cppn", False, None),
          ("lsystem", True, None), ("cppn", True, None), ("lsystem", False, {"fuse_velpost": 0}), ("direct", False, {"pipeline": 0})]


def _pid(c):
    return "%s%s%s" % (c[0], "-wide" if c[1] else "", "".join("-%s%d" % kv for kv in sorted((c[2] or {}).items())))


@pytest.fixture(scope="module")
def gpu():
    return need_gpu()


@pytest.mark.parametrize("case", PARITY, ids=_pid)
def test_closed_loop_parity(gpu, oracle, case):
    torch = gpu
    pop, wide, options = case
    from gym_rem2d_amd import _lib
    runs = M.closed_loop_run(oracle, pop, CONT)          # the oracle first (cached over the builds and launch forms)
    env, rows, morphs = make_env(pop, wide, options)
    try:
        firsts = [M.left_out_first(run, *_lib.capacity(wide)[:2]) for run in runs]
        gone = sum(int((f < len(run["obs"])).sum()) for (f, _), run in zip(firsts, runs))
        assert gone <= int(F.LEFT_OUT_CAP * env.n_envs)
        Mb = max(m.lanes for m in morphs)
        first_pop = np.zeros(env.n_envs, np.int64)
        for (f, _), r in zip(firsts, rows):
            first_pop[r] = f
        compared = 0
        for t in range(M.N_LOOP + 1):
            got = env.observe().cpu().numpy()
            assert got.shape == (env.n_envs, M.width(Mb)) and got.dtype == np.float32
            want = population_rows(runs, rows, "obs", t, Mb)
            keep = first_pop > t
            ne = (got.view(np.uint32) != want.view(np.uint32)) & keep[:, None]     # bit for bit (a -0.0 is not a 0.0)
            assert not ne.any(), "observe() after step %d: %d words differ, first at %s: gpu %r model %r" % (
                t, int(ne.sum()), tuple(np.argwhere(ne)[0]), got[tuple(np.argwhere(ne)[0])], want[tuple(np.argwhere(ne)[0])])
            compared += int(keep.sum())
            if t == M.N_LOOP:
                break
            targets = population_rows(runs, rows, "targets", t, Mb)
            assert np.array_equal(M.policy(t, got, Mb)[keep], M.policy(t, want, Mb)[keep])   # the GPU's rows give the same policy output
            env.set_joint_targets(torch.from_numpy(targets))
            env.step(1)
        check_final(env, runs, firsts, _pid(case))
        print("%s: %d observation rows compared over %d steps, %d creatures left out" % (_pid(case), compared, M.N_LOOP, gone))
    finally:
        env.close()


def _params(ctx):
    rng = np.random.default_rng([ctx.N, ctx.K, 77])
    p = np.zeros((ctx.N, ctx.K, 4))
    p[..., 0], p[..., 1] = rng.uniform(0.0, 1.0, (ctx.N, ctx.K)), rng.uniform(-1.0, 1.0, (ctx.N, ctx.K))
    p[..., 2], p[..., 3] = rng.uniform(0.0, 0.3, (ctx.N, ctx.K)), rng.uniform(-0.3, 0.3, (ctx.N, ctx.K))
    return p


def test_params_mode_parity(gpu, oracle):
    """REM2D_CTRL_PARAMS: 60 closed-loop steps, then amp, phase, freq and offset of every joint are replaced on both sides and the
    oscillators run 100 steps from the i_state they have; final state equal."""
    torch = gpu
    at, n = 60, 160
    runs = M.closed_loop_run(oracle, "direct", CONT, n_steps=n, params_at=(at, _params))
    env, rows, morphs = make_env("direct")
    try:
        Mb = max(m.lanes for m in morphs)
        firsts = [M.left_out_first(run) for run in runs]
        keep = np.zeros(env.n_envs, bool)
        for (f, _), run, r in zip(firsts, runs, rows):
            keep[r] = f >= len(run["obs"])
        assert keep.mean() >= 1.0 - F.LEFT_OUT_CAP
        for t in range(n):
            if t < at:
                env.set_joint_targets(torch.from_numpy(population_rows(runs, rows, "targets", t, Mb)))
            elif t == at:
                params = np.zeros((env.n_envs, Mb, 4))
                for run, r in zip(runs, rows):
                    params[r, :run["ctx"].K] = run["params"]
                env.set_controllers(torch.from_numpy(params))
            env.step(1)
        got = env.observe().cpu().numpy()
        assert np.array_equal(got.view(np.uint32)[keep], population_rows(runs, rows, "obs", n, Mb).view(np.uint32)[keep])
        check_final(env, runs, firsts, "params")
    finally:
        env.close()


def test_fma_build_observes_the_same_bits(gpu):
    """The -ffp-contract=fast build on an IDENTICAL injected state: the arena of a default-build world after 80 steps, copied byte
    for byte (same slot counts, same layout).  Every observed difference is one __fsub_rn, so nothing can be contracted."""
    torch = gpu
    from gym_rem2d_amd import control
    from gym_rem2d_amd.world import BatchedWorld
    terrain, morphs = F.population("lsystem")
    for morph in morphs:
        a = BatchedWorld(morph.n_envs, morph.lanes, CONT)
        b = BatchedWorld(morph.n_envs, morph.lanes, CONT, wide="fma")
        try:
            for w in (a, b):
                w.set_terrain(terrain)
            a.reset(morph)
            a.step(80)
            assert a.arena.numel() == b.arena.numel()
            b.arena.copy_(a.arena)
            b.adopt(morph)
            outs = []
            for w in (a, b):
                out = torch.full((morph.n_envs, control.width(morph.lanes)), 7.0, dtype=torch.float32, device=w.device)
                control.observe([w], morph.lanes, out)
                outs.append(out.cpu().numpy())
            assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
            assert (outs[0][:, 7] >= 1).all() and np.abs(outs[0][:, control.OBS_HEAD:]).max() > 0.1
        finally:
            a.close()
            b.close()


def _controller_words(env):
    """{population row: (live lanes' body index b [K], amp, phase, freq, offset, istate [K] each)} read from every active world."""
    out = {}
    for wi, (w, idx) in enumerate(env.worlds):
        if wi in env._inactive:
            continue
        st = read_state(w)
        live = st["shape"] != 0
        body = np.cumsum(live, axis=1) - 1
        for e, row in enumerate(idx.cpu().numpy()):
            out[int(row)] = (np.where(live[e], body[e], -1), st["parent"][e].copy()) + tuple(
                st[f][e].copy() for f in ("camp", "cphase", "cfreq", "coffset", "cistate"))
    return out


def test_population_plumbing(gpu):
    """Several lane buckets x several step groups, creatures in an arbitrary order: observe() rows follow the population order
    (permute the population and the rows permute with it), before and after a compact() that retires creatures, whose rows keep
    their last observation; a mask leaves the masked-off joints' controller words bit-identical; i_state keeps integrating."""
    torch = gpu
    from gym_rem2d_amd import control, synthetic
    from gym_rem2d_amd.env import BatchedModular2D
    specs = synthetic.lsystem_specs(range(260))            # lane buckets 2 / 4 / 8 / 16, lone roots included
    n = len(specs)
    perm = np.random.default_rng(9).permutation(n)

    def make(order):
        env = BatchedModular2D(seed=4, flags=CONT)
        env.step_groups = 3
        env.reset_specs([specs[i] for i in order])
        return env
    a, b = make(np.arange(n)), make(perm)
    try:
        buckets = len({w.lanes for w, _ in a.worlds})
        assert len(a.groups) >= 2 and buckets >= 3 and len(a.worlds) > buckets        # several step groups x several lane buckets
        Mb = a.max_bodies
        lay = control.layout(Mb)
        n_bodies = np.array([s.n_bodies for s in specs])
        tg = np.random.default_rng(10).uniform(-1.2, 1.2, (n, Mb))
        for env, order in ((a, np.arange(n)), (b, perm)):
            env.step(25)
            env.set_joint_targets(torch.from_numpy(tg[order]).to(torch.float32))       # float32 input: converted exactly
            env.step(15)
        oa, ob = a.observe().clone().cpu().numpy(), b.observe().clone().cpu().numpy()
        assert np.array_equal(ob.view(np.uint32), oa[perm].view(np.uint32))
        assert np.array_equal(oa[:, lay.head["n_bodies"]], n_bodies.astype(np.float32))
        dead = np.arange(Mb)[None, :] >= n_bodies[:, None]
        assert not lay.bodies(oa)[dead].any()                                          # body slots beyond a creature's count are 0
        # a narrower and a wider row than the lanes of any bucket; a caller's buffer; rows beyond it are skipped
        o4 = a.observe(max_bodies=4).clone().cpu().numpy()
        assert np.array_equal(o4.view(np.uint32), oa[:, :control.width(4)].view(np.uint32))
        big = torch.full((n - 7, control.width(40)), 3.0, dtype=torch.float32, device=a.worlds[0][0].device)
        assert a.observe(max_bodies=40, out=big) is big
        big = big.cpu().numpy()
        assert np.array_equal(big[:, :control.width(Mb)].view(np.uint32), oa[:n - 7].view(np.uint32)) and not big[:, control.width(Mb):].any()

        # ---- mask: masked-off joints keep their four words bit for bit; i_state is never written and keeps integrating ----
        before = _controller_words(a)
        rng = np.random.default_rng(12)
        mask = rng.random((n, Mb)) < 0.5
        tg2 = rng.uniform(-1.0, 1.0, (n, Mb))
        a.set_joint_targets(torch.from_numpy(tg2), mask=torch.from_numpy(mask))
        after = _controller_words(a)
        a.step(1)
        stepped = _controller_words(a)
        written = kept = 0
        for row in range(n):
            body, parent, amp0, ph0, fr0, of0, is0 = before[row]
            _, _, amp1, ph1, fr1, of1, is1 = after[row]
            for k in np.flatnonzero(body >= 0):
                bb = int(body[k])
                words0 = np.array([amp0[k], ph0[k], fr0[k], of0[k], is0[k]]).view(np.uint64)
                words1 = np.array([amp1[k], ph1[k], fr1[k], of1[k], is1[k]]).view(np.uint64)
                if parent[k] >= 0 and bb < Mb and mask[row, bb]:
                    assert amp1[k] == 0.0 and of1[k] == tg2[row, bb] and np.array_equal(words0[[1, 2, 4]], words1[[1, 2, 4]])
                    written += 1
                else:
                    assert np.array_equal(words0, words1), (row, k)
                    kept += 1
                if parent[k] >= 0:
                    assert stepped[row][6][k] == is1[k] + fr1[k]
        assert written > 200 and kept > 200

        # ---- compact(): retire every third creature of the population on both sides ----
        b.set_joint_targets(torch.from_numpy(tg2[perm]), mask=torch.from_numpy(mask[perm]))      # (b catches up with a)
        b.step(1)
        for env, order in ((a, np.arange(n)), (b, perm)):
            for w, idx in env.worlds:
                w.view("frozen")[torch.from_numpy(order).to(idx.device)[idx] % 3 == 0] = 1
        last = a.observe().clone().cpu().numpy()
        assert np.array_equal(b.observe().cpu().numpy().view(np.uint32), last[perm].view(np.uint32))
        alive = [env.compact(min_envs=1, max_alive=1.0) for env in (a, b)]
        assert alive[0] == alive[1] <= n - len(range(0, n, 3))
        for env in (a, b):
            env.step(10)
        ca, cb = a.observe().cpu().numpy(), b.observe().cpu().numpy()
        assert np.array_equal(cb.view(np.uint32), ca[perm].view(np.uint32))
        retired = np.ones(n, bool)
        for wi, (w, idx) in enumerate(a.worlds):
            if wi not in a._inactive:
                retired[idx.cpu().numpy()] = False
        assert retired[::3].all() and int((~retired).sum()) == alive[0]
        assert np.array_equal(ca[retired].view(np.uint32), last[retired].view(np.uint32))     # they keep their last observation
        moved = (ca[~retired] != last[~retired]).any(axis=1)
        assert moved.mean() > 0.9
        # targets after compact() reach the survivors only
        a.set_joint_targets(torch.from_numpy(tg))
        words = _controller_words(a)
        assert sorted(words) == sorted(np.flatnonzero(~retired).tolist())
        for row, (body, parent, amp, _, _, off, _) in words.items():
            k = np.flatnonzero((body >= 1) & (parent >= 0) & (body < Mb))
            assert (amp[k] == 0.0).all() and np.array_equal(off[k], tg[row, body[k]])
    finally:
        a.close()
        b.close()


def test_single_world_follows_the_population_order(gpu):
    """One lane bucket, one world, creatures sorted by schedule inside it: rows are the caller's order all the same."""
    torch = gpu
    from gym_rem2d_amd import synthetic
    from gym_rem2d_amd.env import BatchedModular2D
    specs = [s for s in synthetic.lsystem_specs(range(120)) if 5 <= s.n_bodies <= 8][:12]
    envs = []
    try:
        for order in (list(range(len(specs))), list(reversed(range(len(specs))))):
            env = BatchedModular2D(seed=4, flags=CONT)
            env.reset_specs([specs[i] for i in order])
            assert len(env.worlds) == 1
            env.step(30)
            envs.append(env)
        oa, ob = envs[0].observe().cpu().numpy(), envs[1].observe().cpu().numpy()
        assert np.array_equal(ob.view(np.uint32), oa[::-1].view(np.uint32))
        assert np.array_equal(oa[:, 7], np.float32([s.n_bodies for s in specs]))
    finally:
        for env in envs:
            env.close()


def test_gym_facade(gpu):
    """Modular2D(closed_loop=True): reset() and step() return the row BatchedModular2D.observe() holds for the creature, the
    spaces have the real widths, actions reach the joints; closed_loop=False is the reference's surface: observation 0."""
    import copy
    import random
    torch = gpu
    from gym_rem2d_amd import control, get_module_list, gymshim
    from gym_rem2d_amd.encodings import DirectEncoding
    from gym_rem2d_amd.env import Modular2D
    from gym_rem2d_amd.compiler import build_creature
    Mb = 16
    for seed in range(40):      # the first direct-encoding tree with 3 .. Mb bodies
        random.seed(seed)
        ml = get_module_list()
        tree = copy.deepcopy(DirectEncoding(ml).create(6))
        if 3 <= build_creature(copy.deepcopy(tree).getNodes(), ml)[0].n_bodies <= Mb:
            break
    else:
        raise AssertionError("no suitable tree")
    env = gymshim.make("Modular2DLocomotionControl-v0", max_bodies=Mb)
    plain = Modular2D()
    try:
        assert isinstance(env.unwrapped, Modular2D) and env.closed_loop
        assert env.observation_space.shape == (control.width(Mb),) and env.action_space.shape == (Mb,)
        assert plain.observation_space.shape == (24,) and plain.action_space.shape == (4,)
        env.seed(4)
        plain.seed(4)
        obs = env.reset(tree=tree, module_list=ml)
        assert plain.reset(tree=tree, module_list=ml) is None
        nb = len(env.robot.components)
        assert 3 <= nb <= Mb and obs.dtype == np.float32 and obs.shape == (control.width(Mb),) and obs[7] == nb
        batch = env.unwrapped._batch
        assert np.array_equal(obs, batch.observe(Mb)[0].cpu().numpy())
        world = batch.worlds[0][0]
        lanes = np.flatnonzero(world.view("shape")[0].cpu().numpy() != 0)       # body b = lane lanes[b]
        assert len(lanes) == nb
        differ = False
        for t in range(40):
            action = M.policy(t, obs[None], Mb)[0]
            assert env.action_space.contains(action.astype(np.float32))
            obs, r, d, info = env.step(action)
            assert isinstance(obs, np.ndarray) and np.array_equal(obs.view(np.uint32), batch.observe(Mb)[0].cpu().numpy().view(np.uint32))
            amp, off = world.view("camp")[0].cpu().numpy(), world.view("coffset")[0].cpu().numpy()
            assert (amp[lanes[1:]] == 0.0).all() and np.array_equal(off[lanes[1:]], action[1:nb])
            o2, r2, d2, i2 = plain.step(action)
            assert o2 == 0 and not isinstance(o2, np.ndarray) and i2 == 0
            differ = differ or r != r2 or obs[0] != float(plain.world.view("px")[0, 0])
        assert differ                                           # the actions did something the ignored ones did not
        obs2, _, _, _ = env.step(None)                          # None: the joints keep their last targets
        assert np.array_equal(world.view("coffset")[0].cpu().numpy()[lanes[1:]], action[1:nb])
        with pytest.raises(ValueError):
            env.step(np.zeros(Mb + 1))
    finally:
        env.close()
        plain.close()
