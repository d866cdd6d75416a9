"""Recurrent device policies on a real MI355X (pytest -m gpu): the recurrent forward kernel against tests/recurrent_model.py on forged
inputs and forged memory, in the three builds; the law that ties it to rem2d_policy_forward; the closed loop `act()` with
`env.policy_memory` against the oracle; episode boundaries; the evolutionary operators, which take a recurrent weight set as it is;
one ES loop end to end; the gym facade; and the oscillator of the host tests (include/rem2d_recurrent.h).  Every comparison is on
bits: ``view(uint64)`` of the targets and ``view(uint32)`` of the memory (NaNs mapped to one pattern first: policy_model.bits says
why), bytes of `valid`."""
import numpy as np
import pytest

import control_model as M
import policy_model as PM
import recurrent_model as RM
import state_forge as F
import test_policy_gpu as TP

pytestmark = pytest.mark.gpu

CONT = 1
f32 = np.float32
BUILDS = (False, True, "fma")
# (MB, R, K, H): the smallest; odd sizes; the loop's shape; K = H; the dword path (H no multiple of 4); K = 64 - R at the widest layer
SHAPES = [(1, 0, 1, 1), (4, 3, 2, 5), (16, 10, 7, 32), (16, 10, 32, 32), (16, 0, 33, 33), (64, 10, 54, 128)]
ROWS = (1, 9, 64, 65, 257)                   # 9: past a wavefront's 8 rows at 8 lanes per row
GUARD = TP.GUARD
T_SENTINEL, V_SENTINEL, M_SENTINEL = TP.T_SENTINEL, TP.V_SENTINEL, 4242.5


@pytest.fixture(scope="module")
def gpu():
    import replay
    return replay.need_gpu()


# ------------------------------------------------------------------------------------------------------------------ the forge
def _rays(R):
    return None if R in (0, 10) else np.zeros((R, 2)) + 1.0


def _resets(N):
    """the reset masks of the three consecutive calls: everyone, NULL, every third row"""
    third = np.zeros(N, np.uint8)
    third[::3] = 1
    return [np.ones(N, np.uint8), None, third]


def model_calls(x, W, index, mask, act, K):
    """the three calls on the host, from NaN-filled memory -> [(targets bits, valid, memory) per call], rows_run"""
    N = x.shape[0]
    run = PM.rows_run(N, W[0].shape[0], index, mask)
    mem = np.full((N, K), np.nan, f32)
    out = []
    for reset in _resets(N):
        t, v, mem = RM.forward_model(x, mem, *W, act=act, index=index, reset=reset, row_mask=mask)
        t, v = PM.bits(t), v.copy()
        t[~run], v[~run] = np.array([T_SENTINEL]).view(np.uint64)[0], V_SENTINEL
        out.append((t, v, mem))
    return out, run


def run_calls(torch, policy_mod, shape, act, x, W, index, mask, wide, off):
    """the three calls on the device, memory and weights `off` words off a 16-byte boundary, guards checked
    -> [(targets bits, valid, memory float32) per call]"""
    MB, R, K, H = shape
    dev = torch.device("cuda:0")
    N = x.shape[0]
    w = [TP._offset_copy(torch, a, off, dev) for a in W]
    pol = policy_mod.RecurrentPolicy(*w, K, activation=act, index=None if index is None else torch.from_numpy(index).to(dev), rays=_rays(R))
    assert (pol.max_bodies, pol.n_rays, pol.context, pol.hidden) == (MB, R, K, H)
    xd = torch.from_numpy(x).to(dev)
    obs = xd[:, :M.width(MB)].contiguous()
    frac = xd[:, M.width(MB):].contiguous() if R else None
    md = None if mask is None else torch.from_numpy(mask).to(dev)
    mbuf = torch.full((N * K + off + 2 * GUARD,), M_SENTINEL, dtype=torch.float32, device=dev)
    mem = mbuf[GUARD + off:GUARD + off + N * K].view(N, K)
    assert mem.data_ptr() % 16 == (4 * off) % 16 and all(t.data_ptr() % 16 == (4 * off) % 16 for t in w) and mem.is_contiguous()
    mem.fill_(float("nan"))
    tbuf, t = TP._guarded(torch, N * MB, torch.float64, T_SENTINEL, dev)
    vbuf, v = TP._guarded(torch, N * MB, torch.uint8, V_SENTINEL, dev)
    outs = []
    for reset in _resets(N):
        t.fill_(T_SENTINEL)
        v.fill_(V_SENTINEL)
        rd = None if reset is None else torch.from_numpy(reset).to(dev)
        got = pol.forward(obs, frac, mem, reset=rd, out=(t.view(N, MB), v.view(N, MB)), row_mask=md, wide=wide)
        assert got[0].data_ptr() == t.data_ptr()
        tb, vb, mb = tbuf.cpu().numpy(), vbuf.cpu().numpy(), mbuf.cpu().numpy()
        assert (tb[:GUARD] == T_SENTINEL).all() and (tb[-GUARD:] == T_SENTINEL).all(), "guard words of `targets` overwritten"
        assert (vb[:GUARD] == V_SENTINEL).all() and (vb[-GUARD:] == V_SENTINEL).all(), "guard bytes of `valid` overwritten"
        assert (mb[:GUARD + off] == M_SENTINEL).all() and (mb[GUARD + off + N * K:] == M_SENTINEL).all(), "guard words of `memory` overwritten"
        outs.append((PM.bits(tb[GUARD:-GUARD].reshape(N, MB)), vb[GUARD:-GUARD].reshape(N, MB).copy(),
                     mb[GUARD + off:GUARD + off + N * K].reshape(N, K).copy()))
    return outs


@pytest.mark.parametrize("act", [PM.SOFTSIGN, PM.RELU])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "MB%d-R%d-K%d-H%d" % s)
def test_forward_forge(gpu, shape, act):
    """rem2d_recurrent_forward == the model, bit for bit: six shapes x both activations (the ids), each over five row counts, the
    three ways to own weights of test_policy_gpu.forge, the three builds, weight AND memory bases 16-byte aligned and 4 bytes off, and
    three consecutive calls on the same memory: reset everywhere over NaN-filled memory, no reset mask, a reset on every third row.
    After each call targets, valid and memory equal the model; skipped rows keep the sentinel and their memory's very bits; the guards
    around all three buffers stay whole."""
    torch = gpu
    from gym_rem2d_amd import policy
    MB, R, K, H = shape
    compared = invalid = skipped = mem_words = moved = 0
    nan_bits = np.full(1, np.nan, f32).view(np.uint32)[0]
    for N in ROWS:
        for mode in ("per_row", "shared", "indexed"):
            xf, W, index, mask = TP.forge(MB, R + K, H, N, mode, 1)
            x = np.ascontiguousarray(xf[:, :M.width(MB) + R])
            want, run = model_calls(x, W, index, mask, act, K)
            first = None
            for wide in BUILDS:
                for off in (0, 1):
                    got = run_calls(torch, policy, shape, act, x, W, index, mask, wide, off)
                    for c, ((gt, gv, gm), (wt, wv, wm)) in enumerate(zip(got, want)):
                        what = "N=%d %s build=%s offset=%d call %d" % (N, mode, wide, off, c)
                        ne = gt != wt
                        assert not ne.any(), "%s: %d targets differ, first at %s: gpu %#x model %#x" % (
                            what, int(ne.sum()), tuple(np.argwhere(ne)[0]), gt[tuple(np.argwhere(ne)[0])], wt[tuple(np.argwhere(ne)[0])])
                        assert np.array_equal(gv, wv), what + ": validity bytes differ"
                        ne = RM.mem_bits(gm) != RM.mem_bits(wm)
                        assert not ne.any(), "%s: %d memory words differ, first at %s: gpu %r model %r" % (
                            what, int(ne.sum()), tuple(np.argwhere(ne)[0]), gm[tuple(np.argwhere(ne)[0])], wm[tuple(np.argwhere(ne)[0])])
                        assert (gm.view(np.uint32)[~run] == nan_bits).all(), what + ": a skipped row's memory was written"
                    first = got if first is None else first
                    for (gt, gv, gm), (ft, fv, fm) in zip(got, first):
                        assert np.array_equal(gt, ft) and np.array_equal(gv, fv) and np.array_equal(RM.mem_bits(gm), RM.mem_bits(fm)), \
                            "N=%d %s build=%s offset=%d: the builds differ" % (N, mode, wide, off)
            # the three calls are three different computations: the memory moved between them
            moved += int((RM.mem_bits(want[0][2])[run] != RM.mem_bits(want[1][2])[run]).sum())
            compared += 3 * int(run.sum()) * MB
            invalid += sum(int((wv[run] == 0).sum()) for _, wv, _ in want)
            skipped += int((~run).sum())
            mem_words += 3 * int(run.sum()) * K
    print("%s %s: %d targets and %d memory words per build compared, %d targets invalid, %d rows skipped" % (
        shape, act, compared, mem_words, invalid, skipped))
    # the forge is no vacuous one: invalid targets, valid ones and skipped rows all occur
    assert 0 < invalid < compared and skipped > 0 and moved > 0


# ------------------------------------------------------------------------------------------------------------------ the law
@pytest.mark.parametrize("shape", [(4, 3, 2, 5), (16, 10, 32, 32)], ids=lambda s: "MB%d-R%d-K%d-H%d" % s)
def test_the_law(gpu, shape):
    """RecurrentPolicy.forward == MLPPolicy.forward on the same arrays with R + K ray columns and frac' = cat(frac, context), N = 65,
    both activations: targets and validity bytes, bit for bit -- and the memory it leaves is not what it read."""
    torch = gpu
    from gym_rem2d_amd import policy
    MB, R, K, H = shape
    N = 65
    for act in (PM.SOFTSIGN, PM.RELU):
        xf, W, _, _ = TP.forge(MB, R + K, H, N, "per_row", 2)
        w = [torch.from_numpy(a).to("cuda") for a in W]
        rec = policy.RecurrentPolicy(*w, K, activation=act, rays=_rays(R))
        ff = policy.MLPPolicy(*w, activation=act, rays=np.zeros((R + K, 2)) + 1.0)
        assert (ff.n_rays, rec.n_rays, rec.d) == (R + K, R, ff.d)
        xd = torch.from_numpy(xf).to("cuda")
        obs, frac2 = xd[:, :M.width(MB)].contiguous(), xd[:, M.width(MB):].contiguous()
        frac, mem = frac2[:, :R].contiguous(), frac2[:, R:].contiguous()
        before = mem.clone()
        t1, v1 = rec.forward(obs, frac, mem)
        t2, v2 = ff.forward(obs, frac2)
        assert np.array_equal(PM.bits(t1.cpu().numpy()), PM.bits(t2.cpu().numpy())) and torch.equal(v1, v2)
        assert 0 < int((v1 == 0).sum()) < v1.numel() and not torch.equal(mem, before)
        wt, wv, wm = RM.forward_model(xf[:, :M.width(MB) + R], xf[:, M.width(MB) + R:], *W, act=act)
        assert np.array_equal(PM.bits(t1.cpu().numpy()), PM.bits(wt)) and np.array_equal(RM.mem_bits(mem.cpu().numpy()), RM.mem_bits(wm))


# ------------------------------------------------------------------------------------------------- the closed loop and the oracle
def population_policy(torch, policy_mod, runs, rows, n, context, act=PM.SOFTSIGN):
    """The buckets' per-creature weight sets as one recurrent policy in population order"""
    arrays = []
    for k in range(4):
        a = np.zeros((n,) + runs[0]["weights"][k].shape[1:], f32)
        for run, r in zip(runs, rows):
            a[r] = run["weights"][k]
        arrays.append(torch.from_numpy(a))
    return policy_mod.RecurrentPolicy(*arrays, context, activation=act)


def _population_memory(runs, rows, t, n):
    out = np.zeros((n, runs[0]["context"]), f32)
    for run, r in zip(runs, rows):
        out[r] = run["memory"][t]
    return out


@pytest.mark.parametrize("case", [("lsystem", False), ("direct", True)], ids=lambda c: "%s%s" % (c[0], "-wide" if c[1] else ""))
def test_closed_loop_parity(gpu, oracle, case):
    """Both sides from reset, 120 steps: before every step act()'s targets, validity bytes and env.policy_memory equal the model on
    the ORACLE's state, at the end the whole visible state equals the oracle's with test_control_gpu.py's left-out rule; no failed
    hand-over."""
    torch = gpu
    pop, wide = case
    from gym_rem2d_amd import _lib, policy
    from env_harness import check_final, make_env, population_rows
    runs = RM.recurrent_loop_run(oracle, pop, CONT)
    env, rows, morphs = make_env(pop, wide, None)
    try:
        firsts = [M.left_out_first(run, *_lib.capacity(wide)[:2]) for run in runs]
        gone = sum(int((f < len(run["obs"])).sum()) for (f, _), run in zip(firsts, runs))
        assert gone <= int(F.LEFT_OUT_CAP * env.n_envs)
        Mb = PM.LOOP_BODIES
        first_pop = np.zeros(env.n_envs, np.int64)
        for (f, _), r in zip(firsts, rows):
            first_pop[r] = f
        env.set_policy(population_policy(torch, policy, runs, rows, env.n_envs, RM.LOOP_CONTEXT))
        assert type(env.policy) is policy.RecurrentPolicy and env.policy.context == RM.LOOP_CONTEXT
        assert tuple(env.policy_memory.shape) == (env.n_envs, RM.LOOP_CONTEXT) and not bool(env.policy_memory.any())
        compared = 0
        for t in range(PM.N_POLICY_LOOP):
            targets, valid = env.act()
            keep = first_pop > t
            want_t, want_v = population_rows(runs, rows, "targets", t, Mb), population_rows(runs, rows, "valid", t, Mb)
            got_t, got_v = PM.bits(targets.cpu().numpy()), valid.cpu().numpy()
            ne = (got_t != PM.bits(want_t)) & keep[:, None]
            assert not ne.any(), "act() before step %d: %d targets differ, first at %s" % (t, int(ne.sum()), tuple(np.argwhere(ne)[0]))
            assert np.array_equal(got_v[keep], want_v[keep])
            got_m, want_m = env.policy_memory.cpu().numpy(), _population_memory(runs, rows, t + 1, env.n_envs)
            assert np.array_equal(got_m.view(np.uint32)[keep], want_m.view(np.uint32)[keep]), "memory after act() before step %d" % t
            compared += int(keep.sum()) * Mb
            env.step(1)
        check_final(env, runs, firsts, "recurrent-%s" % pop)
        assert env.handover_failures() == 0
        print("%s: %d targets compared over %d steps, %d creatures left out" % (pop, compared, PM.N_POLICY_LOOP, gone))
    finally:
        env.close()


# --------------------------------------------------------------------------------------------------------- episode boundaries
def _boundary_env(torch, pol, specs):
    from gym_rem2d_amd.env import BatchedModular2D
    env = BatchedModular2D(seed=4, flags=CONT)
    env.reset_specs(specs)
    env.set_policy(pol)
    return env


def _model_of_act(env, W, prev_mem, reset):
    """the model on what the last act() observed (its persistent obs / frac buffers), from prev_mem under `reset`"""
    P = env._policy
    x = PM.input_rows(P["obs"].cpu().numpy(), P["frac"].cpu().numpy())
    return RM.forward_model(x, prev_mem, *W, reset=reset)


def _specs64():
    from gym_rem2d_amd import synthetic
    specs = [s for s in synthetic.lsystem_specs(range(160)) if 2 <= s.n_bodies <= 16][:64]
    assert len(specs) == 64
    return specs


def test_autoreset_zeroes_the_context_of_who_restarts(gpu):
    """64 creatures, two episode phases (every other creature is restarted by hand after 3 steps), then set_autoreset(("steps",), 7)
    and 30 x step_policy(1).  After each act() the memory rows of the creatures that just restarted equal the model from ZERO context
    on their fresh observation and all others the model continued from their own; so do targets and validity bytes.  At the end every
    state field of every world is byte-equal to a second env stepped by hand -- observe, sense, RecurrentPolicy.forward on a memory
    tensor of its own with the restarted rows zeroed explicitly, set_joint_targets, step, reset_where -- that never calls act()."""
    torch = gpu
    from gym_rem2d_amd import policy
    specs = _specs64()
    n = len(specs)
    pol = policy.RecurrentPolicy.random(n, 16, 32, 8, seed=31)
    W = tuple(t.numpy() for t in (pol.w1, pol.b1, pol.w2, pol.b2))
    even = torch.zeros(n, dtype=torch.uint8, device="cuda")
    even[::2] = 1
    a, b = _boundary_env(torch, pol, specs), _boundary_env(torch, pol, specs)
    try:
        # ---- a: act() and auto-reset
        a.step_policy(3)
        assert bool(a.policy_memory.any())
        a.reset_where(mask=even)
        a.set_autoreset(("steps",), 7)
        fresh_rows = kept_rows = 0
        for i in range(30):
            prev_mem, prev_ended = a.policy_memory.cpu().numpy().copy(), a.episodes.ended.cpu().numpy().astype(np.uint8)
            a.step_policy(1)                                   # act (reads `ended` of the reset before it), step, reset_where
            wt, wv, wm = _model_of_act(a, W, prev_mem, prev_ended)
            got_m = a.policy_memory.cpu().numpy()
            assert np.array_equal(got_m.view(np.uint32), wm.view(np.uint32)), "memory after act() %d" % i
            assert np.array_equal(PM.bits(a._policy["targets"].cpu().numpy()), PM.bits(wt)) and np.array_equal(a._policy["valid"].cpu().numpy(), wv)
            if prev_ended.any():                               # who restarted did NOT continue from their own memory
                _, _, carried = _model_of_act(a, W, prev_mem, None)
                f = prev_ended != 0
                assert (carried[f].view(np.uint32) != wm[f].view(np.uint32)).any(axis=1).all()
                assert np.array_equal(carried[~f].view(np.uint32), wm[~f].view(np.uint32))
            fresh_rows += int(prev_ended.sum())
            kept_rows += int((prev_ended == 0).sum())
        assert fresh_rows >= 4 * (n // 2) and kept_rows >= 20 * n // 2 and int(a.episodes.count.min()) >= 4
        # ---- b: by hand, with explicit zeroing
        mem = pol.to("cuda").new_memory(n)
        polb = b.policy
        out = (torch.zeros((n, 16), dtype=torch.float64, device="cuda"), torch.zeros((n, 16), dtype=torch.uint8, device="cuda"))

        def hand_step():
            obs, frac = b.observe(16), b.sense_terrain(polb.rays)
            polb.forward(obs, frac, mem, out=out)
            b.set_joint_targets(out[0], mask=out[1])
            b.step(1)
        for _ in range(3):
            hand_step()
        mem[b.reset_where(mask=even)] = 0.0
        for _ in range(30):
            hand_step()
            mem[b.reset_where(when=("steps",), max_steps=7)] = 0.0
        TP._same_worlds(TP._world_bytes(a), TP._world_bytes(b), "auto-reset against the hand-stepped env")
        assert torch.equal(a.episodes.count, b.episodes.count)
        assert not bool(b.policy_memory.any())                  # b's own act() memory was never touched
    finally:
        a.close()
        b.close()


def test_manual_reset_zeroes_the_next_act_only(gpu):
    """Without auto-reset: after reset_where(mask) the NEXT act() reads zero context for those rows -- and only for those -- and the
    act() after it reads what that one left, for everybody."""
    torch = gpu
    from gym_rem2d_amd import policy
    specs = _specs64()
    n = len(specs)
    pol = policy.RecurrentPolicy.random(n, 16, 32, 8, seed=32)
    W = tuple(t.numpy() for t in (pol.w1, pol.b1, pol.w2, pol.b2))
    env = _boundary_env(torch, pol, specs)
    try:
        env.step_policy(5)
        mask = torch.zeros(n, dtype=torch.bool, device="cuda")
        mask[torch.arange(0, n, 3)] = True
        m = mask.cpu().numpy()
        ended = env.reset_where(mask=mask)
        assert torch.equal(ended, mask)
        mem0 = env.policy_memory.cpu().numpy().copy()
        assert (mem0[m] != 0).any(axis=1).all()                 # reset_where itself leaves the memory alone
        env.act()
        mem1 = env.policy_memory.cpu().numpy().copy()
        _, _, want1 = _model_of_act(env, W, mem0, m.astype(np.uint8))
        _, _, carried = _model_of_act(env, W, mem0, None)
        assert np.array_equal(mem1.view(np.uint32), want1.view(np.uint32))
        assert (carried[m].view(np.uint32) != want1[m].view(np.uint32)).any(axis=1).all()
        env.act()                                               # (no step in between: the same observation, the mask still in `ended`)
        assert torch.equal(env.episodes.ended, mask)
        _, _, want2 = _model_of_act(env, W, mem1, None)
        _, _, zeroed = _model_of_act(env, W, mem1, m.astype(np.uint8))
        mem2 = env.policy_memory.cpu().numpy()
        assert np.array_equal(mem2.view(np.uint32), want2.view(np.uint32))
        assert (zeroed[m].view(np.uint32) != want2[m].view(np.uint32)).any(axis=1).all()
        # attaching the policy again zeroes the memory again
        env.set_policy(pol)
        assert not bool(env.policy_memory.any())
    finally:
        env.close()


# ------------------------------------------------------------------------------------------- the operators take it as it is
def _words(p):
    return [t.cpu().numpy().view(np.uint32).copy() for t in (p.w1, p.b1, p.w2, p.b2)]


def _same_sets(rec, ff, what, policy_mod):
    assert type(rec) is policy_mod.RecurrentPolicy and rec.context == 2 and rec.n_rays == 3, what
    assert type(ff) is policy_mod.MLPPolicy and ff.n_rays == 5, what
    for a, b in zip(_words(rec), _words(ff)):
        assert np.array_equal(a, b), what + ": weight bits differ"


def test_the_operators_take_it_as_it_is(gpu):
    """G = 32 sets of (MB, R, K, H) = (4, 3, 2, 5) in blocks of 16: evolve, es_sample + es_update, SeparableES.sample + update and
    EliteGrid.insert + emit each return a RecurrentPolicy with K = 2 whose weight bits are what the same calls give on an MLPPolicy
    of the same arrays with 5 ray columns."""
    torch = gpu
    from gym_rem2d_amd import policy
    from gym_rem2d_amd.elites import EliteGrid
    G, S = 32, 16
    rec = policy.RecurrentPolicy.random(G, 4, 5, 2, n_rays=3, seed=41).to("cuda")
    ff = policy.MLPPolicy(rec.w1.clone(), rec.b1.clone(), rec.w2.clone(), rec.b2.clone(), rays=np.zeros((5, 2)) + 1.0)
    assert rec.d == ff.d == 37
    rng = np.random.default_rng(41)
    fit = torch.from_numpy(rng.standard_normal(G)).to("cuda")
    # tournament GA
    kids = [p.evolve(fit, 3, seed=5, rate=0.3, sigma=0.2, group_size=S, elite=1) for p in (rec, ff)]
    _same_sets(*kids, "evolve", policy)
    assert torch.equal(kids[0].parents, kids[1].parents) and not np.array_equal(_words(kids[0])[0], _words(rec)[0])
    # ES around the first set of each block as the mean
    means = [p.take([0, S]) for p in (rec, ff)]
    kids = [m.es_sample(2, seed=6, sigma=0.1, group_size=S) for m in means]
    _same_sets(*kids, "es_sample", policy)
    assert kids[0].n_sets == G
    new = [m.es_update(fit, 2, seed=6, sigma=0.1, lr=0.5, group_size=S) for m in means]
    _same_sets(*new, "es_update", policy)
    assert not np.array_equal(_words(new[0])[0], _words(means[0])[0])
    # separable NES with Adam
    es = [policy.SeparableES(m, S, sigma=0.1, lr=0.05, adam=(0.9, 0.999, 1e-8)) for m in means]
    kids = [e.sample(1, seed=7) for e in es]
    _same_sets(*kids, "SeparableES.sample", policy)
    new = [e.update(fit, 1, seed=7) for e in es]
    _same_sets(*new, "SeparableES.update", policy)
    assert type(es[0].mean) is policy.RecurrentPolicy and es[0].mean.context == 2
    # MAP-Elites
    desc = torch.from_numpy(rng.random((G, 2)).astype(f32)).to("cuda")
    grids = [EliteGrid(2, [(0, 0.0, 1.0, 4), (1, 0.0, 1.0, 4)], 2, p, device="cuda") for p in (rec, ff)]
    for g, p in zip(grids, (rec, ff)):
        g.insert(p, fit, desc, group_size=S)
    assert torch.equal(grids[0].count, grids[1].count) and int(grids[0].n_filled.min()) >= 4
    _same_sets(grids[0].elites(1), grids[1].elites(1), "EliteGrid.elites", policy)
    kids = [g.emit(4, seed=8, rate=0.3, sigma=0.2, n_children=G) for g in grids]
    _same_sets(*kids, "EliteGrid.emit", policy)
    assert torch.equal(kids[0].parents, kids[1].parents) and int(kids[0].parents.min()) >= 0
    # what comes back runs: one recurrent forward pass on the emitted children
    obs = torch.from_numpy(rng.standard_normal((G, M.width(4))).astype(f32)).to("cuda")
    frac = torch.from_numpy(rng.random((G, 3)).astype(f32)).to("cuda")
    mem = kids[0].new_memory(G)
    t, v = kids[0].forward(obs, frac, mem)
    wt, wv, wm = RM.forward_model(np.concatenate([obs.cpu().numpy(), frac.cpu().numpy()], 1), np.zeros((G, 2), f32),
                                  *[t_.cpu().numpy() for t_ in (kids[0].w1, kids[0].b1, kids[0].w2, kids[0].b2)])
    assert np.array_equal(PM.bits(t.cpu().numpy()), PM.bits(wt)) and np.array_equal(mem.cpu().numpy().view(np.uint32), wm.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------- a loop end to end
def test_an_es_loop_end_to_end(gpu, oracle):
    """evaluate.run_policy_es on 32 L-system creatures in blocks of 16 around 2 recurrent means, 2 generations of 60-step episodes:
    the result equals the same loop written out by hand with set_policy / reset_where / step_policy, and generation 1's fitness ==
    the oracle replay of its children through recurrent_loop_run."""
    torch = gpu
    from gym_rem2d_amd import evaluate, make_terrain, policy, synthetic
    from gym_rem2d_amd.compiler import Morphology, lanes_for
    from gym_rem2d_amd.env import BatchedModular2D
    specs = [s for s in synthetic.lsystem_specs(range(120)) if s.n_bodies >= 2][:32]
    n, steps, S, K = len(specs), 60, 16, RM.LOOP_CONTEXT
    groups = {}
    for e, s in enumerate(specs):
        groups.setdefault(lanes_for(s.n_bodies), []).append(e)
    batches = [(Morphology.from_specs([specs[e] for e in groups[k]], k), groups[k]) for k in sorted(groups)]
    morphs, rows = [m for m, _ in batches], [np.asarray(idx) for _, idx in batches]
    terrain = make_terrain(4)
    sigma, lr, seed = 0.1, 0.5, 7
    first = policy.RecurrentPolicy(*[torch.from_numpy(a.copy()) for a in RM.loop_weights(n // S, 16, K)], K).to("cuda")
    seen = []
    env = BatchedModular2D(seed=4, flags=evaluate.EVAL_FLAGS)
    hand = BatchedModular2D(seed=4, flags=evaluate.EVAL_FLAGS)
    try:
        env.reset_batches(batches, n)
        last, fit, history = evaluate.run_policy_es(
            env, first, 2, seed=seed, sigma=sigma, lr=lr, group_size=S, max_steps=steps, chunk=30,
            on_generation=lambda g, k, f, m: seen.append((g, [t.cpu().numpy().copy() for t in (k.w1, k.b1, k.w2, k.b2)], f.cpu().numpy().copy())))
        assert type(last) is policy.RecurrentPolicy and last.context == K and type(env.policy) is policy.RecurrentPolicy
        assert [s[0] for s in seen] == [1, 2] and bool(env.policy_memory.any())
        # the same loop, written out
        hand.reset_batches(batches, n)
        everyone = torch.ones(n, dtype=torch.uint8, device="cuda")
        mean, fits = first, []
        for gen in (1, 2):
            kids = mean.es_sample(gen, seed=seed, sigma=sigma, group_size=S)
            hand.set_policy(kids)
            hand.reset_where(mask=everyone)
            for _ in range(steps):
                hand.step_policy(1)
            fits.append(hand.fitness.clone())
            mean = mean.es_update(fits[-1], gen, seed=seed, sigma=sigma, lr=lr, group_size=S)
        for (g, _, got), want in zip(seen, fits):
            assert np.array_equal(got.view(np.uint64), want.cpu().numpy().view(np.uint64)), "generation %d: the written-out loop differs" % g
        assert torch.equal(fit, fits[1]) and all(np.array_equal(a, b) for a, b in zip(_words(last), _words(mean)))
        # generation 1 on the oracle
        runs = RM.recurrent_loop_run(oracle, "es32", CONT, n_steps=steps, context=K, morphs=morphs, terrain=terrain,
                                     weights=[tuple(a[r] for a in seen[0][1]) for r in rows], key=("es32", steps, K))
        want = np.zeros(n)
        for run, r in zip(runs, rows):
            want[r] = run["fitness"]
            assert not (M.left_out_first(run)[0] < len(run["obs"])).any()
        assert np.array_equal(seen[0][2].view(np.uint64), want.view(np.uint64)) and len(set(want.tolist())) > n // 2
        assert (seen[0][2] != seen[1][2]).any()
    finally:
        env.close()
        hand.close()


# ------------------------------------------------------------------------------------------------------------------ the facade
def test_gym_facade_with_a_recurrent_policy(gpu):
    """Modular2D(closed_loop=True, policy=RecurrentPolicy): three step(None) calls give the observations of a one-creature batch env
    under the same policy, the memory moves, and reset() zeroes it."""
    import copy
    import random
    torch = gpu
    from gym_rem2d_amd import get_module_list, policy
    from gym_rem2d_amd.compiler import build_creature
    from gym_rem2d_amd.encodings import DirectEncoding
    from gym_rem2d_amd.env import BatchedModular2D, Modular2D
    Mb = 16
    for seed in range(40):
        random.seed(seed)
        ml = get_module_list()
        tree = copy.deepcopy(DirectEncoding(ml).create(6))
        if 3 <= build_creature(copy.deepcopy(tree).getNodes(), ml)[0].n_bodies <= Mb:
            break
    else:
        raise AssertionError("no suitable tree")
    pol = policy.RecurrentPolicy.random(1, Mb, 32, 8, seed=8)
    env = Modular2D(closed_loop=True, max_bodies=Mb, policy=pol)
    batch = BatchedModular2D(seed=4)
    try:
        env.seed(4)
        obs0 = env.reset(tree=copy.deepcopy(tree), module_list=ml)
        batch.reset([copy.deepcopy(tree)], [ml])
        batch.set_policy(pol)
        assert np.array_equal(obs0.view(np.uint32), batch.observe(Mb)[0].cpu().numpy().view(np.uint32))
        assert not bool(env._batch.policy_memory.any())
        mems = []
        for t in range(3):
            obs, r, d, info = env.step(None)
            batch.act()
            batch.step(1)
            assert np.array_equal(obs.view(np.uint32), batch.observe(Mb)[0].cpu().numpy().view(np.uint32)), "step %d" % t
            assert torch.equal(env._batch.policy_memory, batch.policy_memory)
            mems.append(batch.policy_memory.cpu().numpy().copy())
        assert mems[0].any() and not np.array_equal(mems[0], mems[2])
        env.reset(tree=copy.deepcopy(tree), module_list=ml)
        assert type(env._batch.policy) is policy.RecurrentPolicy and not bool(env._batch.policy_memory.any())
    finally:
        env.close()
        batch.close()


# -------------------------------------------------------------------------------------------------------------- the oscillator
def test_oscillator_on_the_device(gpu):
    """The host test's hand-made set through RecurrentPolicy.forward alone, 64 calls on a constant input row: every call's target and
    memory equal the model's, and the target's sign has period 4 once it has run in."""
    torch = gpu
    from gym_rem2d_amd import policy
    x, W = RM.oscillator()
    pol = policy.RecurrentPolicy(*(torch.from_numpy(a) for a in W), 2).to("cuda")
    obs = torch.from_numpy(x).to("cuda")
    mem = pol.new_memory(1)
    want_t, want_m = RM.oscillator_run(64)
    got = []
    for i in range(64):
        t, v = pol.forward(obs, None, mem)
        assert int(v[0, 0]) == 1
        got.append(float(t[0, 0]))
        assert np.array_equal(mem.cpu().numpy()[0].view(np.uint32), want_m[i + 1].view(np.uint32)), "memory after call %d" % i
    got = np.array(got)
    assert np.array_equal(got.view(np.uint64), want_t.view(np.uint64))
    tail = np.sign(got[32:])
    assert np.array_equal(tail[:-4], tail[4:]) and int((tail[1:] != tail[:-1]).sum()) >= 14
