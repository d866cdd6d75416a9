"""Terrain range sensing on a real MI355X (pytest -m gpu): rem2d_worlds_sense / BatchedModular2D.sense_terrain against the host
model (tests/range_model.py), `frac` with == and `hit` exactly, on the root positions read back from the GPU.  The model is a
brute force over every static proxy, so equality also shows that the kernel's edge window and its box reject lose no hit.
tests/test_sense_host.py keeps the main grid from being a vacuous yardstick (how many of its rays end on edges, boxes, nowhere).
"""
import numpy as np
import pytest

import control_model as M
import range_model as R
import state_forge as F
import terrain_forge as TF

pytestmark = pytest.mark.gpu

CONT = 1
f32 = np.float32


@pytest.fixture(scope="module")
def gpu():
    import replay
    return replay.need_gpu()


def same(got, want, what, keep=None):
    """frac with ==, hit exactly"""
    (gf, gh), (wf, wh) = got, want
    assert gf.dtype == np.float32 and gh.dtype == np.int32 and gf.shape == wf.shape == gh.shape == wh.shape, what
    ne = (gf != wf) | (gh != wh)
    if keep is not None:
        ne &= keep[:, None]
    assert not ne.any(), "%s: %d of %d rays differ, first at %s: gpu %r / %d model %r / %d" % (
        what, int(ne.sum()), ne.size, tuple(np.argwhere(ne)[0]), gf[tuple(np.argwhere(ne)[0])], gh[tuple(np.argwhere(ne)[0])],
        wf[tuple(np.argwhere(ne)[0])], wh[tuple(np.argwhere(ne)[0])])


class Probe:
    """A world of n 4-lane chains whose creatures are moved as a whole to given root positions; casts a ray table from them."""

    def __init__(self, torch, profile, n, wide=False):
        from gym_rem2d_amd import synthetic
        from gym_rem2d_amd.world import BatchedWorld
        self.torch, self.n = torch, n
        self.morph = synthetic.chain_population(n, 4, "left")
        self.w = BatchedWorld(n, 4, CONT, wide=wide)
        self.w.set_terrain(profile)
        self.w.reset(self.morph)
        self.T = R.Terrain.of(profile)

    def move(self, px, py):
        torch, w = self.torch, self.w
        x, y = w.view("px"), w.view("py")
        dx = torch.from_numpy(np.asarray(px, f32)).to(w.device) - x[:, 0]
        dy = torch.from_numpy(np.asarray(py, f32)).to(w.device) - y[:, 0]
        x += dx[:, None]
        y += dy[:, None]
        x[:, 0] = torch.from_numpy(np.asarray(px, f32)).to(w.device)       # (the root exactly where it was asked to be)
        y[:, 0] = torch.from_numpy(np.asarray(py, f32)).to(w.device)

    def roots(self):
        return self.w.view("px")[:, 0].cpu().numpy(), self.w.view("py")[:, 0].cpu().numpy()

    def cast(self, rays, hits=True, fill=7.0):
        from gym_rem2d_amd import sense
        torch, w = self.torch, self.w
        rays = np.ascontiguousarray(rays, np.float64)
        frac = torch.full((self.n, len(rays)), fill, dtype=torch.float32, device=w.device)
        hit = torch.full((self.n, len(rays)), -7, dtype=torch.int32, device=w.device) if hits else None
        sense.sense([w], torch.from_numpy(rays).to(w.device), frac, hit)
        return frac.cpu().numpy(), (hit.cpu().numpy() if hits else None)

    def close(self):
        self.w.close()


@pytest.mark.parametrize("name", ["hardcore4", "rough4"])
def test_main_grid(gpu, name):
    """268 origins per pass over and beyond the whole track at three heights, the 10 default rays; between the passes the world
    is stepped.  Then a NaN and an infinite root: 1.0 / -1, the neighbours' rows untouched."""
    prof = TF.profile(name)
    passes = R.grid(prof)
    p = Probe(gpu, prof, len(passes[0][0]))
    rays = R.bipedal_rays()
    try:
        edge = box = none = 0
        for px, py in passes:
            p.w.step(1)
            p.move(px, py)
            gx, gy = p.roots()
            assert np.array_equal(gx, px) and np.array_equal(gy, py)
            got, want = p.cast(rays), R.cast(p.T, gx, gy, rays)
            same(got, want, name)
            edge, box, none = edge + int((got[1] >= p.T.n_poly).sum()), box + int(((got[1] >= 0) & (got[1] < p.T.n_poly)).sum()), none + int((got[1] < 0).sum())
            assert np.array_equal(p.cast(rays, hits=False)[0], got[0])                     # hit_dev = NULL: the same fractions
        print("%s: %d rays on edges, %d on boxes, %d nowhere" % (name, edge, box, none))
        assert edge >= 804 and none >= 804 and (box >= 804 or name == "rough4")
        # non-finite roots in a world that is not stepped afterwards
        before = got
        p.w.view("px")[5, 0] = float("nan")
        p.w.view("py")[9, 0] = float("inf")
        p.w.view("px")[11, 0] = float("-inf")
        after = p.cast(rays)
        for e in (5, 9, 11):
            assert (after[0][e] == 1.0).all() and (after[1][e] == -1).all()
        others = np.ones(p.n, bool)
        others[[5, 9, 11]] = False
        same(after, before, name + " beside a non-finite root", keep=others)
    finally:
        p.close()


def test_long_upward_zero_and_64_rays(gpu):
    """A 400 m horizontal ray either way (the window is the whole track), upward rays, a zero-length ray, 64 rays in all."""
    prof = TF.profile("hardcore4")
    px, py = R.grid(prof)[1]
    ang = np.linspace(0.0, 2 * np.pi, 59, endpoint=False)
    rays = np.concatenate([[[400.0, 0.0], [-400.0, 0.0], [0.0, 0.0], [0.0, 30.0], [250.0, -9.0]],
                           np.stack([np.cos(ang), np.sin(ang)], axis=1) * np.linspace(0.2, 40.0, 59)[:, None]])
    assert rays.shape == (64, 2)
    p = Probe(gpu, prof, len(px))
    try:
        p.move(px, py)
        got, want = p.cast(rays), R.cast(p.T, *p.roots(), rays)
        same(got, want, "ray table")
        assert (got[1][:, 2] == -1).all() and (got[1][:, 3] == -1).sum() > 200                # zero length; straight up
        # the long rays end on edges dozens of edges away from their origins (the model says so: the window must reach them)
        pitch = float(prof.xs[1] - prof.xs[0])
        for k in (0, 1, 4):
            on_edge = want[1][:, k] >= p.T.n_poly
            assert np.abs((want[1][on_edge, k] - p.T.n_poly) - px[on_edge] / pitch).max() > 60
        with pytest.raises(ValueError):
            p.cast(np.zeros((65, 2)))
    finally:
        p.close()


def test_shared_vertex_lowest_index_wins(gpu):
    """Straight down through the vertex edges k - 1 and k share, numbers chosen so that both fractions are 0.25 exactly."""
    from gym_rem2d_amd.terrain import TerrainProfile
    prof = TerrainProfile(np.arange(9.0), np.ones(9), [])
    p = Probe(gpu, prof, 7)
    try:
        px = np.arange(1.0, 8.0).astype(f32)
        p.move(px, np.full(7, 2.0, f32))
        got = p.cast([[0.0, -4.0], [0.0, 4.0]])
        same(got, R.cast(p.T, *p.roots(), [[0.0, -4.0], [0.0, 4.0]]), "shared vertex")
        assert np.array_equal(got[1][:, 0], np.arange(0, 7)) and (got[0][:, 0] == 0.25).all() and (got[1][:, 1] == -1).all()
    finally:
        p.close()


def _env_on(profile, batches, n, **kw):
    from gym_rem2d_amd.env import BatchedModular2D
    env = BatchedModular2D(seed=4, flags=CONT, **kw)
    env.terrain = profile
    env._upload(batches, n)
    return env


def _roots(env):
    """root px, py in population order, of the worlds still stepped"""
    px, py = np.full(env.n_envs, np.nan, f32), np.full(env.n_envs, np.nan, f32)
    for wi, (w, idx) in enumerate(env.worlds):
        if wi not in env._inactive:
            i = idx.cpu().numpy()
            px[i], py[i] = w.view("px")[:, 0].cpu().numpy(), w.view("py")[:, 0].cpu().numpy()
    return px, py


@pytest.mark.parametrize("name", list(TF.TERRAINS))
def test_every_terrain(gpu, name):
    """terrain_forge's terrains with its placed creatures (all lane buckets in one call, rows interleaved), after reset and after
    30 steps: pitch / 4 with x0 = -3, 3 x pitch with x0 = 1000, shifted xs and a short track with creatures beyond both ends
    stress the window."""
    prof, morphs = TF.placed(name, TF.TERRAINS[name][1][0])
    n = sum(m.n_envs for m in morphs)
    order = np.random.default_rng(3).permutation(n)
    rows = np.split(order, np.cumsum([m.n_envs for m in morphs])[:-1])
    env = _env_on(prof, list(zip(morphs, rows)), n)
    T = R.Terrain.of(prof)
    pitch = float(prof.xs[1] - prof.xs[0])
    rays = np.concatenate([R.bipedal_rays(), R.bipedal_rays() * [-1.0, 1.0], [[40 * pitch, -0.2], [-40 * pitch, 0.3], [0.1, 0.05]]])
    try:
        hits = 0
        for steps in (0, 30):
            if steps:
                env.step(steps)
            frac, hit = env.sense_terrain(rays, hits=True)
            got = frac.cpu().numpy(), hit.cpu().numpy()
            same(got, R.cast(T, *_roots(env), rays), "%s after %d steps" % (name, steps))
            hits += int((got[1] >= 0).sum())
        assert hits > 0.2 * 2 * n * len(rays)
        assert len(env._sense_rays) == 1                                                    # one upload for both calls
    finally:
        env.close()


def test_population_order_step_groups_and_compact(gpu):
    """Lane buckets 2 / 4 / 8 / 16 x three step groups in one call; a permuted population permutes the rows; after compact() the
    retired creatures' rows keep their last value; a caller's buffer is written in place."""
    torch = gpu
    from gym_rem2d_amd import synthetic
    from gym_rem2d_amd.env import BatchedModular2D
    specs = synthetic.lsystem_specs(range(260))
    n = len(specs)
    perm = np.random.default_rng(9).permutation(n)

    def make(order):
        env = BatchedModular2D(seed=4, flags=CONT)
        env.step_groups = 3
        env.reset_specs([specs[i] for i in order])
        return env
    a, b = make(np.arange(n)), make(perm)
    T = R.Terrain.of(a._terrain())
    rays = R.bipedal_rays()
    try:
        assert len(a.groups) >= 2 and sorted({w.lanes for w, _ in a.worlds}) == [2, 4, 8, 16] and len(a.worlds) > 4
        for env in (a, b):
            env.step(40)
        fa = a.sense_terrain().cpu().numpy()
        assert fa.shape == (n, 10) and a.sense_terrain() is a.sense_terrain()              # the persistent buffer
        fb, hb = b.sense_terrain(hits=True)
        assert np.array_equal(fb.cpu().numpy(), fa[perm])
        same((fb.cpu().numpy(), hb.cpu().numpy()), R.cast(T, *_roots(b), rays), "permuted population")
        mine = torch.full((n, 10), 3.0, dtype=torch.float32, device=fb.device)
        assert a.sense_terrain(out=mine) is mine and np.array_equal(mine.cpu().numpy(), fa)
        # compact(): retire every third creature
        for w, idx in a.worlds:
            w.view("frozen")[idx % 3 == 0] = 1
        last = a.sense_terrain(hits=True)
        last = last[0].clone().cpu().numpy(), last[1].clone().cpu().numpy()
        alive = a.compact(min_envs=1, max_alive=1.0)
        a.step(10)
        got = a.sense_terrain(hits=True)
        got = got[0].cpu().numpy(), got[1].cpu().numpy()
        px, py = _roots(a)
        retired = np.isnan(px)
        assert retired[::3].all() and int((~retired).sum()) == alive
        same(got, last, "retired rows", keep=retired)
        same(got, R.cast(T, np.nan_to_num(px), np.nan_to_num(py), rays), "survivors", keep=~retired)
        assert (got[0][~retired] != last[0][~retired]).any(axis=1).mean() > 0.5
    finally:
        a.close()
        b.close()


def test_three_builds_write_the_same_bits(gpu):
    """The default, the wide and the -ffp-contract=fast build on the same root positions: the same bits, those of the model."""
    prof = TF.profile("hardcore4")
    px, py = R.grid(prof)[0]
    rays = np.concatenate([R.bipedal_rays(), [[3.0, 1.0], [-2.0, -2.5]]])
    outs = []
    for wide in (False, True, "fma"):
        p = Probe(gpu, prof, len(px), wide=wide)
        try:
            p.move(px, py)
            assert np.array_equal(p.roots()[0], px)
            outs.append(p.cast(rays))
        finally:
            p.close()
    want = R.cast(R.Terrain.of(prof), px, py, rays)
    for got, what in zip(outs, ("default", "wide", "fma")):
        same(got, want, what)
        assert np.array_equal(got[0].view(np.uint32), outs[0][0].view(np.uint32))


def test_state_errors(gpu):
    from gym_rem2d_amd import _lib, sense, synthetic
    from gym_rem2d_amd.world import BatchedWorld
    torch = gpu
    w = BatchedWorld(8, 4, CONT)
    try:
        rays = torch.from_numpy(R.bipedal_rays()).to(w.device)
        frac = torch.ones((8, 10), dtype=torch.float32, device=w.device)
        with pytest.raises(_lib.Rem2dError, match="set_terrain"):
            sense.sense([w], rays, frac)
        w.set_terrain(TF.profile("rough4"))
        with pytest.raises(_lib.Rem2dError, match="reset"):
            sense.sense([w], rays, frac)
        w.reset(synthetic.chain_population(8, 4, "left"))
        sense.sense([w], rays, frac)
        assert (frac.cpu().numpy()[:, 0] < 1.0).all()
        for bad in (frac.double(), frac[:, :9], frac.t()):
            with pytest.raises(ValueError):
                sense.sense([w], rays, bad)
    finally:
        w.close()


def test_gym_facade(gpu):
    """Modular2D(closed_loop=True, lidar=True): the observe words, then sense_terrain's row; lidar=False has the old width."""
    import copy
    import random
    from gym_rem2d_amd import control, get_module_list, gymshim
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
    env = gymshim.make("Modular2DLocomotionLidar-v0", max_bodies=Mb)
    old = Modular2D(closed_loop=True, max_bodies=Mb)
    try:
        W = control.width(Mb)
        assert env.lidar and env.observation_space.shape == (W + 10,) and old.observation_space.shape == (W,)
        env.seed(4)
        old.seed(4)
        obs, obs_old = env.reset(tree=tree, module_list=ml), old.reset(tree=tree, module_list=ml)
        assert obs.shape == (W + 10,) and obs.dtype == np.float32 and obs_old.shape == (W,)
        assert np.array_equal(obs[:W].view(np.uint32), obs_old.view(np.uint32))
        batch = env.unwrapped._batch
        T = R.Terrain.of(batch._terrain())
        for t in range(30):
            action = M.policy(t, obs[None, :W], Mb)[0]
            obs, r, d, info = env.step(action)
            obs_old = old.step(action)[0]
            assert obs.shape == (W + 10,) and np.array_equal(obs[:W].view(np.uint32), obs_old.view(np.uint32))
            assert np.array_equal(obs[:W].view(np.uint32), batch.observe(Mb)[0].cpu().numpy().view(np.uint32))
            assert np.array_equal(obs[W:], batch.sense_terrain()[0].cpu().numpy())
            assert np.array_equal(obs[W:], R.cast(T, obs[0:1], obs[1:2], R.bipedal_rays())[0][0])
        assert obs[W] < 1.0 and obs[W] > 0.0                                               # the ground under the root
    finally:
        env.close()
        old.close()


LIDAR_GAIN = 0.6
N_LIDAR_LOOP = 100


def lidar_policy(t, obs, frac, max_bodies):
    """control_model.policy plus a term on the smallest forward fraction (rays 5 .. 9 of the fan): the fractions feed back"""
    near = 1.0 - frac[:, 5:].astype(np.float64).min(axis=1)
    return np.clip(M.policy(t, obs, max_bodies) + LIDAR_GAIN * near[:, None], -np.pi / 2, np.pi / 2)


def test_closed_loop_with_lidar_on_the_hardcore_track(gpu, oracle):
    """100 closed-loop steps of the CPPN creatures on hardcore4: GPU and oracle are both driven by the targets the policy makes of
    the MODEL's observation rows and fractions; the GPU's fractions must equal the model's at every step (so its own would have
    made the same targets) and the final state the oracle's, as in test_control_gpu.py."""
    torch = gpu
    from gym_rem2d_amd import _lib
    from env_harness import check_final, make_env, population_rows
    terrain, morphs = M.loop_population("cppn")
    T = R.Terrain.of(terrain)
    rays = R.bipedal_rays()
    runs = []
    for morph in morphs:                                                                    # the oracle's side
        loop = M.OracleLoop(oracle, terrain, morph, CONT, "cppn")
        ctx, K = loop.ctx, morph.lanes
        run = dict(ctx=ctx, max_bodies=K, obs=[], frac=[], targets=[], caps=[])
        for t in range(N_LIDAR_LOOP + 1):
            snap = loop.snapshot()
            run["obs"].append(M.observe_model(ctx, snap, K))
            run["frac"].append(R.cast(T, snap["px"][:, 0], snap["py"][:, 0], rays))
            run["caps"].append(np.stack([snap["ccount"].max(axis=1), ((snap["ctouch"] != 0) & F.masks(ctx, snap)["cedge"]).sum(axis=0).max(axis=1)], 1))
            if t == N_LIDAR_LOOP:
                break
            tg = lidar_policy(t, run["obs"][-1], run["frac"][-1][0], K)
            loop.set_targets(tg)
            run["targets"].append(tg)
            loop.step()
        run["final"] = snap
        runs.append(run)
    assert max(np.ptp(np.stack([f[0] for f in run["frac"]])[:, :, 5:].min(axis=2)) for run in runs) > 0.3     # the term is alive
    env, rows, morphs = make_env("cppn")
    try:
        firsts = [M.left_out_first(run, *_lib.capacity(False)[:2]) for run in runs]
        assert sum(int((f < len(run["obs"])).sum()) for (f, _), run in zip(firsts, runs)) <= int(F.LEFT_OUT_CAP * env.n_envs)
        Mb = max(m.lanes for m in morphs)
        first_pop = np.zeros(env.n_envs, np.int64)
        for (f, _), r in zip(firsts, rows):
            first_pop[r] = f
        for t in range(N_LIDAR_LOOP + 1):
            frac, hit = env.sense_terrain(hits=True)
            want_f, want_h = np.zeros((env.n_envs, 10), f32), np.zeros((env.n_envs, 10), np.int32)
            for run, r in zip(runs, rows):
                want_f[r], want_h[r] = run["frac"][t]
            same((frac.cpu().numpy(), hit.cpu().numpy()), (want_f, want_h), "step %d" % t, keep=first_pop > t)
            if t == N_LIDAR_LOOP:
                break
            env.set_joint_targets(torch.from_numpy(population_rows(runs, rows, "targets", t, Mb)))
            env.step(1)
        check_final(env, runs, firsts, "lidar loop")
    finally:
        env.close()
