"""Evolving device policies on a real MI355X (pytest -m gpu): the selection and the variation kernel against tests/evolve_model.py, in
the three builds, MLPPolicy.evolve, and two generations of evaluate.run_policy_generations against the host replay
(include/rem2d_evolve.h).  Every comparison is on bits: ``view(uint32)`` of the weights -- the NaNs at HIT elements mapped to one
pattern first (evolve_model.bits says why), everything else, a copied NaN's payload included, as it is -- and int32 parents."""
import ctypes as C

import numpy as np
import pytest

import evolve_model as EM
import policy_model as PM

pytestmark = pytest.mark.gpu

CONT = 1
f32 = np.float32
BUILDS = (False, True, "fma")
GUARD = 64                                   # guard words in front of and behind every child buffer
SENTINEL = -12345.678                        # what guards and not-yet-written child words hold
SHAPES = [(1, 0, 1), (4, 3, 5), (16, 10, 32)]          # (MB, R, H): per-set lengths 14 1 1 1 / 175 5 20 4 / 3648 32 512 16
SPECIAL = np.array([0x7fc00000, 0xffc01234, 0x7f800001, 0x7f800000, 0xff800000, 0x00000001, 0x807fffff, 0x00400000, 0x80000000,
                    0x00000000], np.uint32).view(f32)  # NaNs with payloads (one signalling), +-inf, denormals, +-0


@pytest.fixture(scope="module")
def gpu():
    import replay
    return replay.need_gpu()


def lengths(MB, R, H):
    D = 8 + 6 * MB + R
    return D, ((D, H), (H,), (H, MB), (MB,))


def forge_weights(MB, R, H, G, seed):
    """G parent sets: a normal bulk, and in every array of every set a few of SPECIAL (all of them where the array is long enough)"""
    rng = np.random.default_rng([MB, R, H, G, seed])
    D, shapes = lengths(MB, R, H)
    W = [(rng.standard_normal((G,) + s) * 0.3).astype(f32) for s in shapes]
    for a in W:
        flat = a.reshape(G, -1)
        n = flat.shape[1]
        for g in range(G):
            at = rng.choice(n, size=min(n, len(SPECIAL)), replace=False)
            flat[g, at] = rng.permutation(SPECIAL)[:len(at)]
    return W


def descriptor(_lib, MB, R, H, G, S, T, elite, thr, sigma, seed, gen, fitness=None, parents=None, kids=None, parent=None):
    D, _ = lengths(MB, R, H)
    e = _lib.Evolve()
    e.d, e.hidden, e.max_bodies, e.n_sets, e.group_size, e.tournsize, e.elite = D, H, MB, G, S, T, elite
    e.generation, e.rate_threshold, e.seed, e.sigma, e.reserved = gen, thr, seed, sigma, 0
    e.fitness = None if fitness is None else fitness.data_ptr()
    if parents is not None:
        e.w1, e.b1, e.w2, e.b2 = (t.data_ptr() for t in parents)
        e.child_w1, e.child_b1, e.child_w2, e.child_b2 = (t.data_ptr() for t in kids)
    e.parent = parent.data_ptr()
    return e


def call(torch, _lib, name, e, wide):
    L = _lib.lib(wide)
    _lib.check(getattr(L, name)(C.byref(e), C.c_void_p(torch.cuda.current_stream().cuda_stream)), wide)


# ------------------------------------------------------------------------------------------------------------------ select
def fitness_cases(G, rng):
    """fitness vectors with what the order has to get right: ties, all equal, NaN, +-inf, +-0"""
    nan, inf = np.nan, np.inf
    few = rng.integers(0, 3, G).astype(np.float64)                                   # three values: ties everywhere
    mixed = rng.choice(np.array([nan, -inf, inf, -0.0, 0.0, 1.5, -2.0, 1e-310]), G)   # every special, repeated
    spread = rng.standard_normal(G)
    spread[rng.integers(G)] = nan
    spread[rng.integers(G)] = inf
    return {"ties": few, "equal": np.full(G, 2.5), "nan": np.full(G, nan), "mixed": mixed, "spread": spread,
            "zeros": np.where(rng.random(G) < 0.5, -0.0, 0.0)}


def run_select(torch, _lib, fit, S, T, elite, seed, gen, wide):
    G = len(fit)
    buf = torch.full((G + 2 * GUARD,), -7, dtype=torch.int32, device="cuda")
    e = descriptor(_lib, 4, 3, 5, G, S, T, elite, 0, 0.0, seed, gen, fitness=torch.from_numpy(fit).to("cuda"), parent=buf[GUARD:])
    call(torch, _lib, "rem2d_policy_select", e, wide)
    got = buf.cpu().numpy()
    assert (got[:GUARD] == -7).all() and (got[GUARD + G:] == -7).all(), "guard words of `parent` overwritten"
    return got[GUARD:GUARD + G]


@pytest.mark.parametrize("G", [1, 5, 64, 65, 130, 200])
def test_select(gpu, G):
    """rem2d_policy_select == the model: every S of {1, 5, 65, G} that divides G (blocks inside a wavefront, across wavefronts and
    longer than one), T = 1 .. 4, elite 0 and 1, six kinds of fitness; G = 65 with S = 65 and G = 130 also in the wide and fma builds"""
    torch = gpu
    from gym_rem2d_amd import _lib
    rng = np.random.default_rng([G, 77])
    cases = fitness_cases(G, rng)
    compared = elites = 0
    for S in sorted({s for s in (1, 5, 65, G) if G % s == 0}):
        for T in (1, 2, 3, 4):
            for elite in (0, 1):
                for name, fit in cases.items():
                    seed, gen = int(rng.integers(0, 2 ** 63)) * 2 + 1, int(rng.integers(0, 2 ** 32))
                    want = EM.select_model(fit, S, T, elite, seed, gen)
                    builds = BUILDS if G in (65, 130) and S == 65 else (False,)
                    for wide in builds:
                        got = run_select(torch, _lib, fit, S, T, elite, seed, gen, wide)
                        ne = got != want
                        assert not ne.any(), "G=%d S=%d T=%d elite=%d %s build=%s: %d parents differ, first child %d: gpu %d model %d" % (
                            G, S, T, elite, name, wide, int(ne.sum()), int(np.argmax(ne)), got[np.argmax(ne)], want[np.argmax(ne)])
                    assert ((want >= (np.arange(G) // S) * S) & (want < (np.arange(G) // S + 1) * S)).all()
                    compared += G
                    elites += elite * (G // S)
    print("G=%d: %d parents compared, %d of them elite scans" % (G, compared, elites))


# -------------------------------------------------------------------------------------------------------------------- vary
def guarded(torch, shape, off):
    """a child buffer of `shape` between two guards, everything SENTINEL; off: words its base lies behind a 16-byte boundary"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD + off,), SENTINEL, dtype=torch.float32, device="cuda")
    return buf, buf[GUARD + off:GUARD + off + n].view(*shape)


def offset_copy(torch, a, off):
    flat = torch.zeros(a.size + off, dtype=torch.float32, device="cuda")
    flat[off:] = torch.from_numpy(a.reshape(-1)).to("cuda")
    return flat[off:].view(*a.shape)


def run_vary(torch, _lib, shape, W, parent, S, elite, thr, sigma, seed, gen, wide, off, name="rem2d_policy_vary", fitness=None, T=4):
    """-> (children as uint32 arrays, parent int32 [G]) of one call; guards and the parents' own words checked"""
    MB, R, H = shape
    G = W[0].shape[0]
    src = [offset_copy(torch, a, off) for a in W]
    bufs, kids = zip(*[guarded(torch, a.shape, off) for a in W])
    assert all(t.data_ptr() % 16 == (4 * off) % 16 for t in src + list(kids))
    pd = torch.from_numpy(np.asarray(parent, np.int32)).to("cuda")
    e = descriptor(_lib, MB, R, H, G, S, T, elite, thr, sigma, seed, gen, parents=src, kids=kids, parent=pd,
                   fitness=None if fitness is None else torch.from_numpy(fitness).to("cuda"))
    call(torch, _lib, name, e, wide)
    out = []
    for buf, a, s in zip(bufs, W, src):
        b = buf.cpu().numpy()
        sent = np.array([SENTINEL], f32).view(np.uint32)[0]
        assert (b[:GUARD + off].view(np.uint32) == sent).all() and (b[GUARD + off + a.size:].view(np.uint32) == sent).all(), \
            "guard words of a child buffer overwritten"
        assert np.array_equal(s.cpu().numpy().view(np.uint32), a.view(np.uint32)), "a parent buffer was written"
        out.append(b[GUARD + off:GUARD + off + a.size].reshape(a.shape))
    return out, pd.cpu().numpy()


def check_children(got, want, hits, what):
    for k, name in enumerate(("w1", "b1", "w2", "b2")):
        g, w = EM.bits(got[k], hits[k]), EM.bits(want[k], hits[k])
        ne = g != w
        assert not ne.any(), "%s: %d words of %s differ, first at %s: gpu %#x model %#x" % (
            what, int(ne.sum()), name, tuple(np.argwhere(ne)[0]), g[tuple(np.argwhere(ne)[0])], w[tuple(np.argwhere(ne)[0])])


def forge_parent(G, rng, out_of_range):
    parent = rng.integers(0, G, G)
    if out_of_range and G >= 3:
        parent[rng.choice(G, 2, replace=False)] = (-1, G)
        if G > 8:
            parent[rng.choice(np.flatnonzero((parent >= 0) & (parent < G)), 2, replace=False)] = (-2 ** 31, 2 ** 31 - 1)
    return parent


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "MB%d-R%d-H%d" % s)
def test_vary(gpu, shape):
    """rem2d_policy_vary == the model: G of 3, 64, 67 x four thresholds (0; 2^32; rates 0.01, 0.5) x sigma 0, 0.1, +inf, the parents
    full of NaN payloads, infinities, denormals and signed zeros, a caller-filled `parent` with repeats and out-of-range entries
    (those children keep the sentinel), elite on and off with blocks of 1 and of G, buffer bases 16-byte aligned and 4 bytes off
    (MB 16, R 10, H 32 aligned is the dwordx4 path).  G = 67 at rate 0.5 also in the wide and the fma build."""
    torch = gpu
    from gym_rem2d_amd import _lib
    rng = np.random.default_rng([shape[2], 5])
    sent = np.array([SENTINEL], f32)
    n_hit = n_nan = n_words = n_skipped = combo = 0
    for G in (3, 64, 67):
        W = forge_weights(*shape, G, 1)
        for thr in (0, 1 << 32, EM.rate_threshold(0.01), EM.rate_threshold(0.5)):
            for sigma in (0.0, 0.1, float("inf")):
                combo += 1
                elite, S = combo % 2, (1 if combo % 4 == 1 else G)
                off = 1 if combo % 3 == 0 else 0
                parent = forge_parent(G, rng, out_of_range=combo % 2 == 0)
                seed, gen = int(rng.integers(0, 2 ** 63)) * 2 + 1, int(rng.integers(0, 2 ** 32))
                before = [np.full(a.shape, sent[0], f32) for a in W]
                want, hits, written = EM.vary_model(W, parent, S, elite, thr, sigma, seed, gen, before=before)
                builds = BUILDS if G == 67 and thr == EM.rate_threshold(0.5) else (False,)
                for wide in builds:
                    what = "G=%d thr=%#x sigma=%s S=%d elite=%d off=%d build=%s" % (G, thr, sigma, S, elite, off, wide)
                    got, pd = run_vary(torch, _lib, shape, W, parent, S, elite, thr, sigma, seed, gen, wide, off)
                    assert np.array_equal(pd, parent.astype(np.int32)), what + ": `parent` was written"
                    check_children(got, want, hits, what)
                    for k in range(4):                                          # (what check_children already implies, said once more)
                        assert (got[k][~written].view(np.uint32) == sent.view(np.uint32)[0]).all(), what + ": a skipped child was touched"
                n_hit += sum(int(h.sum()) for h in hits)
                n_nan += sum(int((np.isnan(w) & h).sum()) for w, h in zip(want, hits))
                n_words += sum(a.size for a in W)
                n_skipped += int((~written).sum())
    print("%s: %d words compared per build, %d hit, %d of the hits NaN, %d children skipped" % (shape, n_words, n_hit, n_nan, n_skipped))
    assert 0 < n_hit < n_words and n_nan > 0 and n_skipped > 0


# ------------------------------------------------------------------------------------------------------------------ evolve
def test_evolve_is_select_then_vary(gpu):
    """rem2d_policy_evolve == rem2d_policy_select followed by rem2d_policy_vary == the model, in the three builds (MB 4, R 3, H 5
    and the dwordx4 shape)"""
    torch = gpu
    from gym_rem2d_amd import _lib
    for shape, G, S in (((4, 3, 5), 65, 5), ((16, 10, 32), 64, 16)):
        W = forge_weights(*shape, G, 2)
        rng = np.random.default_rng([G, 3])
        fit = rng.integers(0, 6, G).astype(np.float64)
        fit[rng.integers(G)] = np.nan
        thr, sigma, seed, gen, T, elite = EM.rate_threshold(0.05), 0.1, 0xfedcba9876543210, 4000000000, 3, 1
        want, hits, wparent = EM.evolve_model(W, fit, S, T, elite, thr, sigma, seed, gen)
        for wide in BUILDS:
            what = "%s build=%s" % (shape, wide)
            got, pd = run_vary(torch, _lib, shape, W, np.full(G, -1), S, elite, thr, sigma, seed, gen, wide, 0, "rem2d_policy_evolve", fit, T)
            assert np.array_equal(pd, wparent), what + ": evolve's parents differ from the model's"
            check_children(got, want, hits, what)
            two = run_select(torch, _lib, fit, S, T, elite, seed, gen, wide)
            assert np.array_equal(two, pd), what
            again, _ = run_vary(torch, _lib, shape, W, two, S, elite, thr, sigma, seed, gen, wide, 0)
            for k in range(4):
                assert np.array_equal(again[k].view(np.uint32), got[k].view(np.uint32)), what + ": select + vary != evolve"


def _words(p):
    return [t.cpu().numpy().view(np.uint32) for t in (p.w1, p.b1, p.w2, p.b2)]


def test_mlp_policy_evolve(gpu):
    """MLPPolicy.evolve: the model's children and parents; the same call twice gives the same bits, another generation or seed
    others; parents= skips selection; the child keeps activation, scale and rays"""
    torch = gpu
    from gym_rem2d_amd import policy
    G = 48
    p = policy.MLPPolicy.random(G, 4, 5, n_rays=3, seed=3, activation="relu", scale=1.25).to("cuda")
    W = [t.cpu().numpy() for t in (p.w1, p.b1, p.w2, p.b2)]
    fit = torch.from_numpy(np.random.default_rng(1).standard_normal(G)).to("cuda")
    kw = dict(seed=11, rate=0.25, sigma=0.5, tournsize=2, group_size=12, elite=1)
    a = p.evolve(fit, 7, **kw)
    want, hits, wparent = EM.evolve_model(W, fit.cpu().numpy(), 12, 2, 1, EM.rate_threshold(0.25), 0.5, 11, 7)
    assert a.parents.dtype == torch.int32 and np.array_equal(a.parents.cpu().numpy(), wparent)
    check_children([t.cpu().numpy() for t in (a.w1, a.b1, a.w2, a.b2)], want, hits, "MLPPolicy.evolve")
    assert (a.activation, a.scale, a.n_sets, a.index) == ("relu", 1.25, G, None) and np.array_equal(a.rays, p.rays)
    assert all(np.array_equal(x, y.view(np.uint32)) for x, y in zip(_words(p), W)), "the parents were written"
    b = p.evolve(fit, 7, **kw)
    assert all(np.array_equal(x, y) for x, y in zip(_words(a), _words(b))) and torch.equal(a.parents, b.parents)
    for other in (p.evolve(fit, 8, **kw), p.evolve(fit, 7, **dict(kw, seed=12)), p.evolve(fit, 7, **dict(kw, seed=11 + 2 ** 32))):
        assert not torch.equal(other.parents, a.parents) and (_words(other)[0] != _words(a)[0]).mean() > 0.1
    # the defaults: one population, tournaments of 4, no elite
    d = p.evolve(fit, 1)
    assert np.array_equal(d.parents.cpu().numpy(), EM.select_model(fit.cpu().numpy(), G, 4, 0, 0, 1))
    # parents=: the caller's selection; a child without a parent keeps the zeros of its fresh buffer
    mine = torch.arange(G, dtype=torch.int32, device="cuda").flip(0).contiguous()
    mine[5] = -1
    c = p.evolve(fit, 7, parents=mine, **kw)
    wantc, hitsc, written = EM.vary_model(W, mine.cpu().numpy(), 12, 1, EM.rate_threshold(0.25), 0.5, 11, 7)
    assert c.parents is mine and not written[5] and float(c.w1[5].abs().max()) == 0.0
    check_children([t.cpu().numpy() for t in (c.w1, c.b1, c.w2, c.b2)], wantc, hitsc, "parents=")


def test_double_buffering(gpu):
    """out=: three generations through two sets of buffers equal three generations of fresh allocations, and allocate nothing"""
    torch = gpu
    from gym_rem2d_amd import policy
    G = 64
    first = policy.MLPPolicy.random(G, 16, 32, seed=4).to("cuda")
    fits = [torch.from_numpy(np.random.default_rng(g).standard_normal(G)).to("cuda") for g in range(3)]
    kw = dict(seed=5, rate=0.05, sigma=0.1, group_size=16, elite=1)
    fresh = [first]
    for g in range(3):
        fresh.append(fresh[-1].evolve(fits[g], g + 1, **kw))
    start = policy.MLPPolicy(first.w1.clone(), first.b1.clone(), first.w2.clone(), first.b2.clone())
    spare = policy.MLPPolicy.random(G, 16, 32, seed=9).to("cuda")
    spare.parents = torch.zeros(G, dtype=torch.int32, device="cuda")
    start.parents = torch.zeros(G, dtype=torch.int32, device="cuda")
    cur = start
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    for g in range(3):
        child = cur.evolve(fits[g], g + 1, out=spare, **kw)
        assert child is spare and torch.cuda.memory_allocated() == held, "evolve(out=) allocated device memory"
        assert all(np.array_equal(x, y) for x, y in zip(_words(child), _words(fresh[g + 1]))), "generation %d" % (g + 1)
        assert torch.equal(child.parents, fresh[g + 1].parents)
        spare, cur = cur, child
    assert len({t.w1.data_ptr() for t in (cur, spare)}) == 2


# ------------------------------------------------------------------------------------------------------------- generations
def test_two_generations_give_the_replays_fitness(gpu, oracle):
    """evaluate.run_policy_generations on 64 L-system creatures, blocks of 16, two generations of episodes capped at 60 steps: each
    generation's fitness is the host replay's -- evolve_model for the weights, the oracle's closed loop for the episode -- and so
    are the final weights and the history rows."""
    torch = gpu
    from gym_rem2d_amd import evaluate, make_terrain, policy, synthetic
    from gym_rem2d_amd.compiler import Morphology, lanes_for
    from gym_rem2d_amd.env import BatchedModular2D
    specs = [s for s in synthetic.lsystem_specs(range(120)) if s.n_bodies >= 2][:64]
    n, steps, S = len(specs), 60, 16
    groups = {}
    for e, s in enumerate(specs):
        groups.setdefault(lanes_for(s.n_bodies), []).append(e)
    batches = [(Morphology.from_specs([specs[e] for e in groups[k]], k), groups[k]) for k in sorted(groups)]
    morphs, rows = [m for m, _ in batches], [np.asarray(idx) for _, idx in batches]
    terrain = make_terrain(4)
    D, shapes = lengths(PM.LOOP_BODIES, 10, PM.LOOP_HIDDEN)
    W = [np.zeros((n,) + s, f32) for s in shapes]
    for m, r in zip(morphs, rows):
        for k, a in enumerate(PM.loop_weights(len(r), m.lanes)):
            W[k][r] = a
    kw = dict(seed=7, rate=0.05, sigma=0.1, tournsize=4, group_size=S, elite=1)
    # the host's generations
    want_fit, want_W = [], [W]
    for gen in range(3):
        fit, gone = EM.episode_replay(oracle, terrain, morphs, rows, want_W[-1], CONT, steps, PM.LOOP_BODIES)
        assert not gone.any()
        want_fit.append(fit)
        if gen < 2:
            want_W.append(EM.evolve_model(want_W[-1], fit, S, 4, 1, EM.rate_threshold(0.05), 0.1, 7, gen + 1)[0])
    assert all((f > 0).sum() >= 8 and len(set(f.tolist())) > n // 2 for f in want_fit)
    assert any((a != b).any() for a, b in zip(want_fit[1:], want_fit[:-1]))
    env = BatchedModular2D(seed=4, flags=evaluate.EVAL_FLAGS)
    seen = []
    try:
        env.reset_batches(batches, n)
        first = policy.MLPPolicy(*[torch.from_numpy(a) for a in W])
        last, fit, history = evaluate.run_policy_generations(env, first, 2, max_steps=steps, chunk=30,
                                                             on_generation=lambda g, p, f: seen.append((g, f.clone().cpu().numpy())), **kw)
        assert [g for g, _ in seen] == [0, 1, 2] and fit.dtype == torch.float64 and fit.device.type == "cuda"
        for (g, got), want in zip(seen, want_fit):
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), "generation %d: the fitness differs from the replay's" % g
        assert np.array_equal(fit.cpu().numpy().view(np.uint64), want_fit[2].view(np.uint64))
        for got, want in zip(_words(last), want_W[2]):
            assert np.array_equal(got, want.view(np.uint32)), "the final weights differ from the model's"
        assert env.policy is last and last.device.type == "cuda"
        assert [h[0] for h in history] == [1, 2]
        for h, want in zip(history, want_fit[1:]):
            assert h[1] == want.min() and h[2] == want.max() and abs(h[3] - want.mean()) <= 1e-12 * abs(want.mean())
    finally:
        env.close()


def test_generations_reuse_two_sets_of_buffers(gpu):
    """run_policy_generations over three generations: the caller's policy is never written, generations 1 and 3 share their buffers,
    and every generation's fitness and the final weights equal the same loop written out with fresh allocations"""
    torch = gpu
    from gym_rem2d_amd import evaluate, policy, synthetic
    from gym_rem2d_amd.env import BatchedModular2D
    specs = [s for s in synthetic.lsystem_specs(range(60)) if s.n_bodies >= 2][:32]
    n, steps = len(specs), 20
    kw = dict(seed=3, rate=0.1, sigma=0.2, tournsize=2, group_size=8, elite=0)
    first = policy.MLPPolicy.random(n, 16, 32, seed=6).to("cuda")
    before = _words(first)
    seen = []
    a, b = BatchedModular2D(seed=4, flags=evaluate.EVAL_FLAGS), BatchedModular2D(seed=4, flags=evaluate.EVAL_FLAGS)
    try:
        a.reset_specs(specs)
        last, fit, history = evaluate.run_policy_generations(
            a, first, 3, max_steps=steps, chunk=steps, on_generation=lambda g, p, f: seen.append((p.w1.data_ptr(), f.clone())), **kw)
        ptrs = [p for p, _ in seen]
        assert ptrs[0] == first.w1.data_ptr() and ptrs[3] == ptrs[1] and len({ptrs[0], ptrs[1], ptrs[2]}) == 3
        assert all(np.array_equal(x, y) for x, y in zip(_words(first), before)), "the caller's policy was written"
        b.reset_specs(specs)
        everyone = torch.ones(n, dtype=torch.uint8, device="cuda")
        p = first
        for g in range(4):
            if g:
                p = p.evolve(seen[g - 1][1], g, **kw)
                b.reset_where(mask=everyone)
            b.set_policy(p)
            f = evaluate.run_policy_episode(b, max_steps=steps, chunk=steps, compact=False)
            assert torch.equal(f.view(torch.int64), seen[g][1].view(torch.int64)), "generation %d" % g
        assert all(np.array_equal(x, y) for x, y in zip(_words(last), _words(p))) and torch.equal(last.parents, p.parents)
        assert [h[0] for h in history] == [1, 2, 3] and history[2][2] == float(fit.max())
    finally:
        a.close()
        b.close()
