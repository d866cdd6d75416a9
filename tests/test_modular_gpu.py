"""Modular device policies on the GPU (include/rem2d_modular.h) against tests/modular_model.py, bit for bit, in the three builds:
the forward pass on forged rows, trees and messages; law (a) against RecurrentPolicy.forward; the topology table against the
creatures' trees; ONE weight set driving a population of mixed morphologies through set_policy / act() / step_policy(); messages
that travel one edge per round; the search operators; the three calls under a capture and behind test_caller_stream_gpu's gate;
the refusals."""
import numpy as np
import pytest

import modular_model as MM
import policy_model as PM
import test_caller_stream_gpu as TCS
import test_policy_gpu as TP
from test_caller_stream_gpu import gate  # noqa: F401  (the fixture: the gate's cycle count, proved by its control)

pytestmark = pytest.mark.gpu

f32 = np.float32
CONT = 1
BUILDS = (False, True, "fma")
GUARD = TP.GUARD
T_SENT, V_SENT = TP.T_SENTINEL, TP.V_SENTINEL
nan = f32("nan")


@pytest.fixture(scope="module")
def gpu():
    import replay
    return replay.need_gpu()


def _rays(R):
    return None if R in (0, 10) else np.zeros((R, 2)) + 1.0


def _guarded(torch, shape, dtype, fill):
    """a contiguous tensor of `shape` inside a buffer with GUARD words in front of and behind it -> (view, whole buffer)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf[GUARD:GUARD + n].view(*shape), buf


def _guards_intact(buf, fill, what):
    g = np.concatenate([buf[:GUARD].cpu().numpy(), buf[-GUARD:].cpu().numpy()])
    assert g.tobytes() == np.full(2 * GUARD, fill, g.dtype).tobytes(), "guard words around `%s` were written" % what


def run_forward(torch, policy_mod, f, K, P, act, wide, index=None, row_mask=None, reset=None):
    """one rem2d_modular_forward on forged inputs, outputs under sentinels and between guards -> (targets, valid, memory) as numpy"""
    N, MB = f["topo"].shape[:2]
    R = 0 if f["frac"] is None else f["frac"].shape[1]
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    pol = policy_mod.ModularPolicy(*[dev(w) for w in f["weights"]], messages=K, rounds=P, max_bodies=MB, activation=act,
                                   index=None if index is None else dev(index.astype(np.int32)), rays=_rays(R))
    tg, tg_buf = _guarded(torch, (N, MB), torch.float64, T_SENT)
    va, va_buf = _guarded(torch, (N, MB), torch.uint8, V_SENT)
    mem, mem_buf = _guarded(torch, (N, MB, K), torch.float32, 7.5)
    mem.copy_(dev(f["memory"]))
    pol.forward(dev(f["obs"]), dev(f["frac"]), dev(f["topo"]), mem, reset=dev(reset), out=(tg, va), row_mask=dev(row_mask), wide=wide)
    torch.cuda.synchronize()
    _guards_intact(tg_buf, T_SENT, "targets")
    _guards_intact(va_buf, V_SENT, "valid")
    _guards_intact(mem_buf, 7.5, "memory")
    return tg.cpu().numpy(), va.cpu().numpy(), mem.cpu().numpy()


def check_forward(torch, policy_mod, f, K, P, act, wide, what, index=None, row_mask=None, reset=None):
    N, MB = f["topo"].shape[:2]
    got = run_forward(torch, policy_mod, f, K, P, act, wide, index, row_mask, reset)
    sent = (np.full((N, MB), T_SENT, np.float64), np.full((N, MB), V_SENT, np.uint8))
    want = MM.forward_model(f["obs"], f["frac"], f["topo"], f["memory"], *f["weights"], rounds=P, act=act, index=index, reset=reset,
                            row_mask=row_mask, out=sent)
    for name, g, w in zip(("targets", "valid", "memory"), (PM.bits(got[0]), got[1], MM.mem_bits(got[2])),
                          (PM.bits(want[0]), want[1], MM.mem_bits(want[2]))):
        ne = g != w
        assert not ne.any(), "%s: %d words of `%s` differ from the model, first at %r" % (what, int(ne.sum()), name, tuple(np.argwhere(ne)[0]))
    run = PM.rows_run(N, f["weights"][0].shape[0], index, row_mask)
    if not run.all():                                             # skipped rows keep their sentinel bytes in all three outputs
        assert (got[0][~run] == T_SENT).all() and (got[1][~run] == V_SENT).all()
        assert got[2][~run].tobytes() == f["memory"][~run].tobytes()
    return got


# (MB, H, K, R, P, N): every MB, H, K, R, P and N of the issue; 26 / 10 and 31 / 0 are the R + 2 + 2 K = 64 corner; MB = 64 holds the
# chain of depth 63 and the star of 63 children (forge_topo's rows 0 and 1)
SHAPES = [(1, 1, 1, 0, 1, 1), (2, 32, 8, 10, 2, 65), (3, 33, 1, 10, 8, 65), (12, 128, 8, 10, 1, 65), (64, 32, 8, 10, 2, 65),
          (64, 128, 31, 0, 1, 9), (12, 32, 26, 10, 2, 65), (3, 8, 8, 0, 8, 1), (64, 33, 8, 10, 1, 9), (12, 1, 1, 10, 2, 65)]


@pytest.mark.parametrize("build", BUILDS, ids=TCS._bid)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "MB%d-H%d-K%d-R%d-P%d-N%d" % s)
def test_forward_forge(gpu, shape, build):
    """per-row sets under softsign; shared sets through an index with values outside [0, G), a row mask and a reset mask over NaN
    memory under relu"""
    torch = gpu
    from gym_rem2d_amd import policy
    MB, H, K, R, P, N = shape
    f = MM.forge(11, N, MB, H, K, R)
    if MB == 64:
        live, par = MM.tree(f["topo"])
        assert par[0].tolist() == [-1] + list(range(63)) and par[1].tolist() == [-1] + [0] * 63 and live[:2].all()
    check_forward(torch, policy, f, K, P, PM.SOFTSIGN, build, "per-row sets")
    rng = np.random.default_rng([5, N, MB])
    G = 5
    g = MM.forge(12, N, MB, H, K, R, G=G)
    index = rng.integers(0, G, N)
    bad = rng.random(N) < 0.15
    index[bad] = rng.choice([-1, G, G + 3, 2 ** 31 - 1, -2 ** 31], int(bad.sum()))
    row_mask = (rng.random(N) < 0.8).astype(np.uint8)
    reset = (rng.random(N) < 0.4).astype(np.uint8)
    if N > 1:
        index[0], row_mask[0], reset[0] = 1, 1, 1                  # row 0 runs, from zero messages
        index[1], row_mask[1], reset[1] = 2, 1, 0                  # row 1 runs on what memory holds
        index[2], row_mask[2] = G, 1                                # row 2 names no set
        row_mask[3] = 0
    g["memory"][reset != 0] = nan                                   # a NaN does not survive a reset
    check_forward(torch, policy, g, K, P, PM.RELU, build, "shared sets", index=index.astype(np.int64), row_mask=row_mask, reset=reset)


@pytest.mark.parametrize("build", BUILDS, ids=TCS._bid)
def test_no_rows(gpu, build):
    torch = gpu
    from gym_rem2d_amd import policy
    f = MM.forge(13, 0, 12, 32, 8, 10, G=2)
    got = run_forward(torch, policy, f, 8, 2, PM.SOFTSIGN, build, index=np.zeros(0, np.int64))
    assert got[0].shape == (0, 12) and got[2].shape == (0, 12, 8)


@pytest.mark.parametrize("MB", [2, 12])
def test_the_law(gpu, MB):
    """law (a) on the device: one round equals RecurrentPolicy.forward on the flattened (row, body) rows, in every build"""
    torch = gpu
    from gym_rem2d_amd import policy
    H, K, R, N = 32, 8, 10, 33
    f = MM.forge(17, N, MB, H, K, R, G=4)
    index = np.arange(N) % 4
    live, par = MM.tree(f["topo"])
    m0 = f["memory"].copy()
    m0[~live] = 0
    nch, cm, pm = MM.gather(m0, live, par)
    x = MM.body_rows(f["obs"], f["frac"], f["topo"], nch, cm, pm)
    rr, bb = np.nonzero(live)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    for build in BUILDS:
        tg, va, mem = run_forward(torch, policy, f, K, 1, PM.SOFTSIGN, build, index=index)
        rec = policy.RecurrentPolicy(*[dev(w) for w in f["weights"]], K, index=dev(index[rr].astype(np.int32)), rays=np.zeros((R + 2 + K, 2)) + 1.0)
        assert rec.max_bodies == 1 and rec.n_rays == R + 2 + K
        flat_mem = dev(pm[rr, bb])
        t1, v1 = rec.forward(dev(x[rr, bb, :14]), dev(x[rr, bb, 14:14 + R + 2 + K]), flat_mem, wide=build)
        torch.cuda.synchronize()
        assert np.array_equal(PM.bits(t1.cpu().numpy()[:, 0]), PM.bits(tg[rr, bb])) and np.array_equal(v1.cpu().numpy()[:, 0], va[rr, bb])
        assert np.array_equal(MM.mem_bits(flat_mem.cpu().numpy()), MM.mem_bits(mem[rr, bb]))


# ------------------------------------------------------------------------------------------------------------ the topology
def _mixed_specs():
    """48 L-system creatures: 1-, 2-, 5- and 12-module ones among them, boxes and circles, lane buckets 2, 4, 8 and 16"""
    from gym_rem2d_amd import synthetic
    from gym_rem2d_amd.compiler import lanes_for
    specs = synthetic.lsystem_specs(range(48))
    counts = {s.n_bodies for s in specs}
    assert {1, 2, 5, 12} <= counts and max(counts) == 16
    assert {b.shape for s in specs for b in s.bodies} == {1, 2} and len({lanes_for(s.n_bodies) for s in specs}) >= 2
    return specs


def _host_topology(specs, max_bodies):
    """the table from the creatures' own joints: body index = rank of the body's lane among the creature's lanes"""
    parents, shapes = [], []
    for s in specs:
        rank = {slot: i for i, slot in enumerate(sorted(b.slot for b in s.bodies))}
        ps = [-1] * len(rank)
        for j in s.joints:
            ps[rank[j["child"]]] = rank[j["parent"]]
        sh = [0] * len(rank)
        for b in s.bodies:
            sh[rank[b.slot]] = b.shape
        parents.append(ps)
        shapes.append(sh)
    return MM.topology_model(parents, shapes, max_bodies)


@pytest.mark.parametrize("build", BUILDS, ids=TCS._bid)
def test_topology(gpu, build):
    torch = gpu
    from gym_rem2d_amd.env import BatchedModular2D
    specs = _mixed_specs()
    env = BatchedModular2D(seed=4, flags=CONT, wide=build)
    try:
        env.reset_specs(specs)
        assert len(env.worlds) >= 2
        for MB in (12, 16, 20, 1, 64):                               # below, at and above the largest count
            got = env.topology(MB)
            assert got.dtype == torch.int32 and tuple(got.shape) == (len(specs), MB, 2)
            want = _host_topology(specs, MB)
            assert np.array_equal(got.cpu().numpy(), want), "max_bodies %d" % MB
        assert (_host_topology(specs, 12)[:, :, 0] < 12).all()
        out, buf = _guarded(torch, (len(specs), 16, 2), torch.int32, -77)
        assert env.topology(16, out=out) is out
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), _host_topology(specs, 16))
        _guards_intact(buf, -77, "topo")
        assert env.topology().shape[1] == env.max_bodies
        with pytest.raises(ValueError, match="max_bodies"):
            env.topology(65)
    finally:
        env.close()


# --------------------------------------------------------------------------------------------------------- the closed loop
def _model_of_act(env, W, P, prev_mem, reset):
    """the model on what the last act() observed (its persistent obs / frac buffers) and on topology(), from prev_mem under `reset`"""
    B = env._policy
    topo = env.topology(B["policy"].max_bodies).cpu().numpy()
    return MM.forward_model(B["obs"].cpu().numpy(), B["frac"].cpu().numpy(), topo, prev_mem, *W, rounds=P, index=np.zeros(env.n_envs, np.int64),
                            reset=reset)


def _same(a, b, what):
    assert np.array_equal(a, b), what


@pytest.mark.parametrize("build", BUILDS, ids=TCS._bid)
def test_one_set_drives_a_mixed_population(gpu, build):
    """ONE shared weight set (index = 0 everywhere) drives 48 creatures of mixed morphologies.  After every act() the targets, the
    validity bytes and policy_memory equal the model fed with observe(), sense_terrain() and topology(); a second env driven by
    hand with the MODEL's targets through set_joint_targets ends with the same bytes in every state field of every world -- the
    controller words of every joint among them.  After reset_where() on some rows, and under set_autoreset, the restarted rows read
    zero messages and nobody else's memory moves."""
    torch = gpu
    from gym_rem2d_amd import policy
    from gym_rem2d_amd.env import BatchedModular2D
    specs = _mixed_specs()
    n, MB, K, P = len(specs), 16, 8, 2
    pol = policy.ModularPolicy.random(1, 32, K, rounds=P, max_bodies=MB, seed=23, index=torch.zeros(n, dtype=torch.int32))
    W = tuple(t.numpy() for t in pol.weights)
    envs = []
    try:
        for _ in range(2):
            env = BatchedModular2D(seed=4, flags=CONT, wide=build)
            env.reset_specs(specs)
            envs.append(env)
        a, b = envs
        a.set_policy(pol)
        assert type(a.policy) is policy.ModularPolicy and tuple(a.policy_memory.shape) == (n, MB, K) and not bool(a.policy_memory.any())
        assert np.array_equal(a.policy_topology.cpu().numpy(), _host_topology(specs, MB))

        def check_act(prev_mem, reset, what):
            wt, wv, wm = _model_of_act(a, W, P, prev_mem, reset)
            B = a._policy
            _same(PM.bits(B["targets"].cpu().numpy()), PM.bits(wt), what + ": targets")
            _same(B["valid"].cpu().numpy(), wv, what + ": valid")
            _same(MM.mem_bits(a.policy_memory.cpu().numpy()), MM.mem_bits(wm), what + ": policy_memory")
            # the model's inputs are what observe() and sense_terrain() give now (act() observed the same state)
            _same(a.observe(MB).cpu().numpy().view(np.uint32), B["obs"].cpu().numpy().view(np.uint32), what + ": obs")
            _same(a.sense_terrain(a.policy.rays).cpu().numpy().view(np.uint32), B["frac"].cpu().numpy().view(np.uint32), what + ": frac")
            return wt, wv, wm

        def hand(wt, wv):
            b.set_joint_targets(torch.from_numpy(wt).to("cuda"), mask=torch.from_numpy(wv).to("cuda"))

        mem = np.zeros((n, MB, K), f32)
        for i in range(3):                                           # act() by act()
            a.act()
            wt, wv, mem = check_act(mem, None, "act %d" % i)
            hand(wt, wv)
            a.step(1)
            b.step(1)
        TP._same_worlds(TP._world_bytes(a), TP._world_bytes(b), "act() against the model's targets set by hand")
        live = _host_topology(specs, MB)[:, :, 1] != 0
        assert (mem[live] != 0).any() and not mem[~live].any() and wv[live].all()
        # step_policy(3) is three of those
        before = mem
        a.step_policy(3)
        after = a.policy_memory.cpu().numpy()
        assert (after != before).any()
        # reset_where on every third row: the next act() reads zero messages there, and only there
        mask = torch.zeros(n, dtype=torch.bool, device="cuda")
        mask[torch.arange(0, n, 3)] = True
        m = mask.cpu().numpy()
        a.reset_where(mask=mask)
        mem0 = a.policy_memory.cpu().numpy().copy()
        _same(mem0.view(np.uint32), after.view(np.uint32), "reset_where leaves the memory alone")
        a.act()
        _, _, want1 = check_act(mem0, m.astype(np.uint8), "the act() after reset_where")
        _, _, carried = _model_of_act(a, W, P, mem0, None)
        assert (carried[m].view(np.uint32) != want1[m].view(np.uint32)).any() and np.array_equal(carried[~m].view(np.uint32), want1[~m].view(np.uint32))
        a.act()
        check_act(want1, None, "the act() after that")               # the mask is this one call's
        # auto-reset: every act() reads the `ended` of the reset before it
        a.set_autoreset(("steps",), 4)
        fresh = 0
        for i in range(9):
            prev_mem = a.policy_memory.cpu().numpy().copy()
            prev_ended = a.episodes.ended.cpu().numpy().astype(np.uint8) if i else None      # (the manual reset's mask has been used)
            a.step_policy(1)                                         # act, step, reset_where
            w = _model_of_act(a, W, P, prev_mem, prev_ended)
            _same(MM.mem_bits(a.policy_memory.cpu().numpy()), MM.mem_bits(w[2]), "auto-reset act %d: policy_memory" % i)
            _same(PM.bits(a._policy["targets"].cpu().numpy()), PM.bits(w[0]), "auto-reset act %d: targets" % i)
            if i:
                f = prev_ended != 0
                _, _, carried = _model_of_act(a, W, P, prev_mem, None)
                assert np.array_equal(carried[~f].view(np.uint32), w[2][~f].view(np.uint32))
                fresh += int(f.sum())
        assert fresh >= n
        # a new upload drops the policy, its memory and its table; attaching it again makes them again
        a.reset_specs(specs[::-1])
        assert a.policy is None and a.policy_memory is None and a.policy_topology is None
        a.set_policy(pol)
        assert not bool(a.policy_memory.any()) and np.array_equal(a.policy_topology.cpu().numpy(), _host_topology(specs[::-1], MB))
    finally:
        for env in envs:
            env.close()


def test_a_body_is_its_words_not_its_column(gpu):
    """what the modular policy is for: an MLPPolicy's set is tied to body columns; a modular set's result for a body depends on the
    body's own words and on its neighbours', whatever its column"""
    torch = gpu
    from gym_rem2d_amd import policy
    H, K, R, MB = 32, 8, 10, 12
    f = MM.forge(29, 2, MB, H, K, R, G=1, specials=False)
    # the same two-body creature, once in columns 0, 1 and once in columns 0, 5 with non-live slots between them
    f["topo"][:] = [-1, 0]
    f["obs"][1] = f["obs"][0]
    f["frac"][1] = f["frac"][0]
    f["memory"][:] = 0
    f["topo"][0, 0], f["topo"][0, 1] = (-1, 1), (0, 2)
    f["topo"][1, 0], f["topo"][1, 5] = (-1, 1), (0, 2)
    f["obs"][1, 8 + 6 * 5:8 + 6 * 6] = f["obs"][0, 8 + 6:8 + 12]
    tg, va, mem = run_forward(torch, policy, f, K, 2, PM.SOFTSIGN, False, index=np.zeros(2, np.int64))
    assert PM.bits(tg[0, :2]).tolist() == PM.bits(tg[1, [0, 5]]).tolist() and np.array_equal(mem[0, 1], mem[1, 5]) and va[1].tolist() == [1, 0, 0, 0, 0, 1] + [0] * 6


def test_gym_facade_with_a_modular_policy(gpu):
    """Modular2D(closed_loop=True, policy=ModularPolicy): step(None) acts by it -- the observations are those of a one-creature
    batch env under the same policy, the messages move, and reset() zeroes them"""
    torch = gpu
    from gym_rem2d_amd import policy, synthetic
    from gym_rem2d_amd.env import BatchedModular2D, Modular2D
    tree = synthetic.chain_tree(4)
    pol = policy.ModularPolicy.random(1, 8, 2, rounds=2, max_bodies=8, seed=3)
    env = Modular2D(closed_loop=True, max_bodies=8, policy=pol)
    batch = BatchedModular2D(seed=4)
    try:
        env.seed(4)
        env.reset(tree=tree, module_list=[0])
        batch.reset([tree], [[0]])
        batch.set_policy(pol)
        for t in range(3):
            obs, r, d, info = env.step(None)
            batch.act()
            batch.step(1)
            assert np.array_equal(obs[:8 + 6 * 8].view(np.uint32), batch.observe(8)[0].cpu().numpy().view(np.uint32)), "step %d" % t
            assert torch.equal(env._batch.policy_memory, batch.policy_memory)
        mem = batch.policy_memory.cpu().numpy()
        assert mem.shape == (1, 8, 2) and mem[0, :4].any() and not mem[0, 4:].any()
        assert env._batch.policy_topology.cpu().numpy()[0, :, 0].tolist() == [-1, 0, 1, 2, -1, -1, -1, -1]
        env.reset(tree=tree, module_list=[0])
        assert type(env._batch.policy) is policy.ModularPolicy and not bool(env._batch.policy_memory.any())
    finally:
        env.close()
        batch.close()


# -------------------------------------------------------------------------------------------------------- messages matter
@pytest.mark.parametrize("build", BUILDS, ids=TCS._bid)
def test_messages_travel_one_edge_per_round(gpu, build):
    """a hand-made set (K = 1, relu: h = touching + the children's messages) on a 3-chain.  A round makes a body's message from its
    own words and the messages of the round before, so the touching word of the root's child is in the root's message after exactly
    two acts and not after one -- with P = 2 after one act -- and the leaf's, two edges away, after exactly three (P = 3: one)."""
    torch = gpu
    from gym_rem2d_amd import policy
    import test_modular_host as TH
    W = TH.relay_weights()
    topo = MM.topology_model([MM.chain(3)], [[1, 1, 1]], 3)

    def acts(body, P, n):
        obs = np.zeros((1, 8 + 6 * 3), f32)
        obs[0, 8 + 6 * body + 3] = 1.0
        f = dict(obs=obs, frac=None, topo=topo, memory=np.zeros((1, 3, 1), f32), weights=W)
        root = []
        for _ in range(n):
            tg, va, mem = check_forward(torch, policy, f, 1, P, PM.RELU, build, "relay")
            f["memory"] = mem
            root.append(float(mem[0, 0, 0]))
        return root
    assert acts(1, 1, 3) == [0.0, 1.0, 1.0]
    assert acts(1, 2, 1) == [1.0]
    assert acts(2, 1, 4) == [0.0, 0.0, 1.0, 1.0]
    assert acts(2, 2, 2) == [0.0, 1.0]
    assert acts(2, 3, 1) == [1.0]


# ------------------------------------------------------------------------------------------- the operators take it as it is
def _words(p):
    return [t.cpu().numpy().view(np.uint32).copy() for t in p.weights]


def test_the_operators_take_it_as_it_is(gpu):
    """G = 32 sets of (H, K, R) = (5, 2, 3) in blocks of 16: evolve, es_sample + es_update, SeparableES.sample + update and
    EliteGrid.insert + emit each return a ModularPolicy of the same K, P and max_bodies whose weight bits are what the same calls
    give on the MLPPolicy(max_bodies = 1, n_rays = R + 2 + 2 K) view of the same arrays"""
    torch = gpu
    from gym_rem2d_amd import policy
    from gym_rem2d_amd.elites import EliteGrid
    G, S, K, P, MB, R = 32, 16, 2, 3, 12, 3
    mod = policy.ModularPolicy.random(G, 5, K, rounds=P, max_bodies=MB, n_rays=R, seed=41).to("cuda")
    ff = policy.MLPPolicy(mod.w1.clone(), mod.b1.clone(), mod.w2.clone(), mod.b2.clone(), rays=np.zeros((R + 2 + 2 * K, 2)) + 1.0)
    assert mod.d == ff.d == 14 + 9 and ff.max_bodies == 1 and ff.n_rays == R + 2 + 2 * K

    def same(m, f, what):
        assert type(m) is policy.ModularPolicy and (m.messages, m.rounds, m.max_bodies, m.n_rays, m.weight_bodies) == (K, P, MB, R, 1), what
        assert type(f) is policy.MLPPolicy, what
        for x, y in zip(_words(m), _words(f)):
            assert np.array_equal(x, y), what + ": weight bits differ"
    rng = np.random.default_rng(41)
    fit = torch.from_numpy(rng.standard_normal(G)).to("cuda")
    kids = [p.evolve(fit, 3, seed=5, rate=0.3, sigma=0.2, group_size=S, elite=1) for p in (mod, ff)]
    same(*kids, "evolve")
    assert torch.equal(kids[0].parents, kids[1].parents) and not np.array_equal(_words(kids[0])[0], _words(mod)[0])
    means = [p.take([0, S]) for p in (mod, ff)]
    kids = [m.es_sample(2, seed=6, sigma=0.1, group_size=S) for m in means]
    same(*kids, "es_sample")
    new = [m.es_update(fit, 2, seed=6, sigma=0.1, lr=0.5, group_size=S) for m in means]
    same(*new, "es_update")
    assert not np.array_equal(_words(new[0])[0], _words(means[0])[0])
    es = [policy.SeparableES(m, S, sigma=0.1, lr=0.05, adam=(0.9, 0.999, 1e-8)) for m in means]
    same(*[e.sample(1, seed=7) for e in es], "SeparableES.sample")
    same(*[e.update(fit, 1, seed=7) for e in es], "SeparableES.update")
    desc = torch.from_numpy(rng.random((G, 2)).astype(f32)).to("cuda")
    grids = [EliteGrid(2, [(0, 0.0, 1.0, 4), (1, 0.0, 1.0, 4)], 2, p, device="cuda") for p in (mod, ff)]
    for g, p in zip(grids, (mod, ff)):
        g.insert(p, fit, desc, group_size=S)
    assert torch.equal(grids[0].count, grids[1].count) and int(grids[0].n_filled.min()) >= 4
    same(grids[0].elites(1), grids[1].elites(1), "EliteGrid.elites")
    kids = [g.emit(4, seed=8, rate=0.3, sigma=0.2, n_children=G) for g in grids]
    same(*kids, "EliteGrid.emit")
    # what comes back runs
    f = MM.forge(43, G, MB, 5, K, R, specials=False)
    f["weights"] = tuple(t.cpu().numpy() for t in kids[0].weights)
    check_forward(torch, policy, f, K, P, PM.SOFTSIGN, False, "the emitted children")


# ------------------------------------------------------------------------------------------------------ the caller's stream
ST = (12, 8, 2, 3, 2, 65)                     # (MB, H, K, R, P, N): V = 4, two passes of bodies


def case_forward(torch, wide):
    from gym_rem2d_amd import policy
    MB, H, K, R, P, N = ST
    c = TCS.Case(torch)
    sets = []
    for s in (1, 2, 3):
        f = MM.forge(50 + s, N, MB, H, K, R, specials=s != 3)
        f["topo"] = MM.forge(50, N, MB, H, K, R)["topo"] if s != 2 else f["topo"]
        sets.append(f)
    obs, frac = c.inp("obs", *(s["obs"] for s in sets)), c.inp("frac", *(s["frac"] for s in sets))
    topo, mem = c.inp("topo", *(s["topo"] for s in sets)), c.inp("memory", *(s["memory"] for s in sets))
    w = [c.inp(n, *(s["weights"][i] for s in sets)) for i, n in enumerate(TCS.NAMES4)]
    pol = policy.ModularPolicy(*w, messages=K, rounds=P, max_bodies=MB, rays=np.zeros((R, 2)) + 1.0)
    out = (c.out("targets", (N, MB), torch.float64, TCS.F_SENT), c.out("valid", (N, MB), torch.uint8, 0xA5))
    c.inout("memory")
    c.call = lambda: pol.forward(obs, frac, topo, mem, out=out, wide=wide)

    def want(key):
        d = c.data[key]
        tg, v, new = MM.forward_model(d["obs"], d["frac"], d["topo"], d["memory"], d["w1"], d["b1"], d["w2"], d["b2"], rounds=P)
        return [PM.bits(tg), v.astype(np.uint8), MM.mem_bits(new)]
    c.want = want
    c.norm = lambda key, got: [PM.bits(got[0]), got[1], MM.mem_bits(got[2])]
    c.insensitive = {"valid"}
    return c


def _shape_words(w, host):
    """the `shape` words of a world's lanes inside its arena bytes"""
    import ctypes as C
    from gym_rem2d_amd import _lib
    off, cnt, dt = C.c_size_t(), C.c_size_t(), C.c_int32()
    _lib.check(w.L.rem2d_world_field(w.h, _lib.FIELD_ID["shape"], C.byref(off), C.byref(cnt), C.byref(dt)), w.wide)
    assert dt.value == 1
    return host[off.value:off.value + cnt.value * 4].view(np.int32)


def forge_shapes(w, arena, key):
    """the table is the same in every recorded state: the decoy (and data set B, in part) swaps boxes and circles, which the call
    reports and which moves no lane into or out of a creature"""
    a = _shape_words(w, arena)
    pick = (a != 0) if key == "decoy" else (a != 0) & (np.arange(a.size) % 3 == 0) if key == "B" else np.zeros(a.size, bool)
    a[pick] = 3 - a[pick]


def mk_topology(c, env, rig):
    out = c.out("topo", (env.n_envs, 16, 2), c.torch.int32, TCS.I_SENT)
    c.call = lambda: env.topology(16, out=out)


ACT_HIDDEN, ACT_K, ACT_BODIES = 5, 2, 8


def prep_act_modular(env):
    from gym_rem2d_amd import policy
    env.set_policy(policy.ModularPolicy.random(TCS.N_POP, ACT_HIDDEN, ACT_K, rounds=2, max_bodies=ACT_BODIES, seed=3))


def mk_act_modular(c, env, rig):
    B = env._policy
    c.bind("memory", B["memory"], *TCS._sets(lambda s, fin: TCS._rng(s, 2).standard_normal((TCS.N_POP, ACT_BODIES, ACT_K)).astype(f32)))
    c.out_existing("obs", B["obs"], TCS.F_SENT)
    c.out_existing("frac", B["frac"], TCS.F_SENT)
    c.out_existing("targets", B["targets"], TCS.F_SENT)
    c.out_existing("valid", B["valid"], 0xA5)
    c.insensitive = {"valid"}
    c.inout("memory")
    c.call = lambda: env.act()


STREAM_CASES = {
    "forward": case_forward,
    "topology": lambda torch, wide: TCS._world_case(torch, wide, mk_topology, False, tag="modular_topology", forge=forge_shapes),
    "act": lambda torch, wide: TCS._world_case(torch, wide, mk_act_modular, True, tag="modular_act", prepare=prep_act_modular),
}
_CASES = {}


def _stream_case(torch, which, build):
    if (which, build) not in _CASES:
        c = STREAM_CASES[which](torch, build)
        memo, model = {}, c.want
        c.want = lambda key: memo[key] if key in memo else memo.setdefault(key, model(key))
        _CASES[(which, build)] = c
    return _CASES[(which, build)]


@pytest.fixture(scope="module", autouse=True)
def _cases_released():
    yield
    _CASES.clear()
    for key in [k for k in TCS._RIGS if k[0].startswith("modular_")]:
        TCS._RIGS.pop(key).close()


STREAM_IDS = [pytest.param(w, b, id="%s-%s" % (w, TCS._bid(b))) for w in STREAM_CASES for b in BUILDS]


@pytest.mark.parametrize("which,build", STREAM_IDS)
def test_capture_and_replay(gpu, which, build):
    """The call alone captured on a caller's stream (the stream travels in the descriptor): the capture succeeds, nothing ran during
    it, and each replay computes the reference of what the inputs hold then: data set A, then B written in place"""
    torch = gpu
    c = _stream_case(torch, which, build)
    what = "modular %s (%s build)" % (which, TCS._bid(build))
    c.load("A")
    torch.cuda.synchronize()
    before = c.read()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.call()
    torch.cuda.synchronize()
    c.untouched("A", before, what + " during capture")
    g.replay()
    torch.cuda.synchronize()
    c.compare("A", what + " first replay")
    c.load("B")
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    c.compare("B", what + " second replay")
    del g


@pytest.mark.parametrize("which,build", STREAM_IDS)
def test_behind_a_gate(gpu, gate, which, build):  # noqa: F811
    """test_caller_stream_gpu's gate leg, as it is: the call on a caller's stream behind a spin and the copies that bring its real
    inputs; a launch that went to any other stream reads the decoy"""
    torch = gpu
    c = _stream_case(torch, which, build)
    c.reads_decoy()
    TCS._gated(torch, c, gate)
    what = "modular %s (%s build) behind the gate" % (which, TCS._bid(build))
    got, decoy = c.norm("decoy", c.read()), c.want("decoy")
    for n, g, d in zip(c.names(), got, decoy):
        assert n in c.insensitive or (np.asarray(g).reshape(-1) != np.asarray(d).reshape(-1)).any(), \
            "%s: `%s` holds the DECOY's result: a launch did not wait for the caller's stream" % (what, n)
    c.compare("A", what)


# ----------------------------------------------------------------------------------------------------------- the refusals
def test_refusals(gpu):
    """normalizer=, a streamed evaluation and refill() under a ModularPolicy; the descriptors the library refuses write nothing"""
    torch = gpu
    import ctypes as C
    from gym_rem2d_amd import _lib, policy
    from gym_rem2d_amd.env import BatchedModular2D
    import test_modular_host as TH
    specs = _mixed_specs()[:16]
    pol = policy.ModularPolicy.random(16, 8, 2, max_bodies=16, seed=1)
    env = BatchedModular2D(seed=4, flags=CONT)
    try:
        env.reset_specs(specs)
        norm = policy.ObsNormalizer(1, 16, 16, 10)
        with pytest.raises(ValueError, match="a ModularPolicy takes no normalizer"):
            env.set_policy(pol, normalizer=norm)
        assert env.policy is None
        env.set_policy(pol)
        env._stream_rec = object()                                   # (as if a streamed evaluation were in place under it)
        with pytest.raises(ValueError, match="refill: a ModularPolicy is attached"):
            env.refill()
        env._stream_rec = None
        env.reset_stream(TCS._batches(32), 32, 16)
        with pytest.raises(ValueError, match="cannot be attached to a streamed evaluation"):
            env.set_policy(pol)
    finally:
        env.close()
    # every REM2D_E_INVALID case of the header, on real device buffers under sentinels: nothing is written
    f = MM.forge(3, 3, 16, 32, 8, 10)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    p = policy.ModularPolicy(*[dev(w) for w in f["weights"]], messages=8, max_bodies=16)
    tg = torch.full((3, 16), T_SENT, dtype=torch.float64, device="cuda")
    va = torch.full((3, 16), V_SENT, dtype=torch.uint8, device="cuda")
    mem = dev(f["memory"])
    good = p.descriptor(dev(f["obs"]), dev(f["frac"]), tg, va, dev(f["topo"]), mem)
    L = _lib.lib()
    for kw, msg in TH.BAD:
        q = _lib.Modular()
        C.memmove(C.byref(q), C.byref(good), C.sizeof(q))
        for k, v in kw.items():
            setattr(q if k in TH.MOD_FIELDS else q.p, k, v)
        assert L.rem2d_modular_forward(C.byref(q)) == -1 and msg in L.rem2d_last_error(), kw
    torch.cuda.synchronize()
    assert bool((tg == T_SENT).all()) and bool((va == V_SENT).all()) and mem.cpu().numpy().tobytes() == f["memory"].tobytes()
