"""Behavioural novelty on a real MI355X (pytest -m gpu): rem2d_novelty_score / _add / _step and rem2d_worlds_describe against
tests/novelty_model.py, every comparison by bits under `==` with NaNs mapped to one pattern, every output between guard words,
every input verified unchanged; the three builds; NoveltyArchive, BatchedModular2D.describe, evaluate.run_behaviour_episode and two
generations of evaluate.run_policy_nses against the host replay (es_model for the weights, the oracle's closed loop for the
episodes and the positions, novelty_model for the rest).

Shapes: widths on both sides of every padded register width (1, 2, 8, 31, 32), blocks below, at and above the wavefront and the
256-row tile (1, 2, 63, 64, 65, 257), one and three blocks, k from 1 to 32 (beyond the candidates where blocks are short), archives
of 0, 1, 5 and 300 entries (one tile and a bit) that are empty, part full, full and wrapped."""
import ctypes as C

import numpy as np
import pytest

import control_model as CM
import es_model as ES
import novelty_model as NM
import policy_model as PM
from replay import need_gpu

pytestmark = pytest.mark.gpu

CONT = 1
f32 = np.float32
BUILDS = (False, True, "fma")
GUARD = 16
WIDTHS = (1, 2, 8, 31, 32)
SIZES = (1, 2, 63, 64, 65, 257)
KS = (1, 2, 15, 32)
CAPS = (0, 1, 5, 300)
CONTENTS = ("random", "dups", "grid", "special")


@pytest.fixture(scope="module")
def gpu():
    return need_gpu()


# ----------------------------------------------------------------------------------------------------------------- buffers
class Buf:
    """A device array between guard words, at an aligned or a 4-byte-offset base (float32 arrays; 8-byte types stay aligned)"""

    def __init__(self, torch, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        self.shape, self.dtype = arr.shape, arr.dtype
        self.n, self.at = arr.size, GUARD + (int(offset) if arr.dtype.itemsize == 4 else 0)
        flat = np.full(self.n + 2 * GUARD + 1, 0, arr.dtype)
        flat[:] = self.pattern(len(flat))
        flat[self.at:self.at + self.n] = arr.ravel()
        self.host = flat.copy()
        self.t = torch.from_numpy(flat).to("cuda")

    def pattern(self, n):
        if self.dtype == np.float32:
            return np.full(n, 0xFFC0DE77, np.uint32).view(f32)       # (a NaN with a payload: == on bits)
        if self.dtype == np.float64:
            return np.full(n, 0xFFF8C0DE000000AA, np.uint64).view(np.float64)
        return np.full(n, 0x5A, self.dtype)

    @property
    def ptr(self):
        return self.t.data_ptr() + self.at * self.dtype.itemsize

    def read(self):
        """the array; the guards must be as they were"""
        flat = self.t.cpu().numpy()
        raw, was = flat.view(np.uint8), self.host.view(np.uint8)
        i0, i1 = self.at * self.dtype.itemsize, (self.at + self.n) * self.dtype.itemsize
        assert np.array_equal(raw[:i0], was[:i0]) and np.array_equal(raw[i1:], was[i1:]), "guard words were written"
        return flat[self.at:self.at + self.n].reshape(self.shape).copy()

    def unchanged(self):
        return np.array_equal(self.t.cpu().numpy().view(np.uint8), self.host.view(np.uint8))


def make_desc(kind, G, B, rng):
    if kind == "random":
        return rng.standard_normal((G, B)).astype(f32)
    if kind == "grid":                                      # a coarse integer grid: many equal d2, many exact twins
        return rng.integers(0, 3, (G, B)).astype(f32)
    if kind == "dups":                                      # whole rows duplicated
        d = rng.standard_normal((G, B)).astype(f32)
        return d[rng.integers(0, max(1, G // 3), G)]
    d = rng.standard_normal((G, B)).astype(f32)            # special: NaN, +-inf, denormals, +-0 and words that make d2 overflow
    pool = np.array([np.nan, np.inf, -np.inf, 1e-45, -3e-42, 0.0, -0.0, 1e19, -1e19, 3e38], f32)
    hit = rng.random((G, B)) < 0.08
    d[hit] = rng.choice(pool, int(hit.sum()))
    d[rng.random(G) < 0.1] = f32(0.0)
    return d


def totals_for(cap, M, which):
    """total [M] for an archive of cap entries: one of 0, 1, cap - 1, cap, 3 cap + 2 per block, rotated by `which`"""
    menu = [0, 1, max(cap - 1, 0), cap, 3 * cap + 2]
    return np.array([menu[(which + b) % len(menu)] for b in range(M)], np.int64)


def descriptor(bufs, B, G, S, k, cap, generation=0, seed=0, threshold=0):
    from gym_rem2d_amd import _lib
    n = _lib.Novelty()
    n.width, n.n_rows, n.group_size, n.k, n.capacity = B, G, S, k, cap
    n.generation, n.seed, n.add_threshold, n.reserved = generation, seed, threshold, 0
    n.desc, n.total = bufs["desc"].ptr, bufs["total"].ptr
    n.archive = bufs["archive"].ptr if cap else None
    n.novelty = bufs["novelty"].ptr if "novelty" in bufs else None
    n.add_mask = bufs["mask"].ptr if "mask" in bufs else None
    return n


def call(torch, wide, name, n):
    from gym_rem2d_amd import _lib
    _lib.check(getattr(_lib.lib(wide), name)(C.byref(n), None), wide)
    torch.cuda.synchronize()


def cases_for(B):
    """(S, M, k, cap, which total, content, offset): every S twice with this width; both M and every k, cap and content with every width,
    the totals and bases in rotation"""
    out = []
    i = WIDTHS.index(B)
    for s, S in enumerate(SIZES):
        for rep in range(2):
            out.append((S, (1, 3)[(s + rep) % 2], KS[(s // 2 + rep + i) % 4], CAPS[(s + 2 * rep + i) % 4], (s + 3 * rep + i) % 5,
                        CONTENTS[(s + rep + 2 * i) % 4], (s + i) % 2))
    return out


def same64(got, want, what):
    g, w = NM.bits64(got), NM.bits64(want)
    ne = g != w
    assert not ne.any(), "%s: %d scores differ, first at %d: gpu %r model %r" % (what, int(ne.sum()), int(np.argmax(ne)), got[np.argmax(ne)], want[np.argmax(ne)])


# ------------------------------------------------------------------------------------------------------------------- score
@pytest.mark.parametrize("B", WIDTHS)
def test_score(gpu, B):
    """rem2d_novelty_score == novelty_model.score_model, bit for bit, in the three builds, twice alike"""
    torch = gpu
    seen_short = seen_nan = 0
    for ci, (S, M, k, cap, which, content, offset) in enumerate(cases_for(B)):
        rng = np.random.default_rng([B, S, M, k, cap, which])
        G = M * S
        desc = make_desc(content, G, B, rng)
        arch = make_desc(content if content != "dups" else "random", M * cap, B, rng).reshape(M, cap, B)
        total = totals_for(cap, M, which)
        want = NM.score_model(desc, S, k, arch if cap else None, total)
        seen_short += int(S - 1 + min(int(total.max()), cap) < k)
        seen_nan += int(np.isnan(want).any())
        what = "B %d S %d M %d k %d cap %d total %s %s offset %d" % (B, S, M, k, cap, total.tolist(), content, offset)
        for wide in BUILDS:
            bufs = dict(desc=Buf(torch, desc, offset), archive=Buf(torch, arch, offset), total=Buf(torch, total),
                        novelty=Buf(torch, np.zeros(G, np.float64)))
            n = descriptor(bufs, B, G, S, k, cap)
            call(torch, wide, "rem2d_novelty_score", n)
            got = bufs["novelty"].read()
            same64(got, want, "%s build %s" % (what, wide))
            call(torch, wide, "rem2d_novelty_score", n)
            assert np.array_equal(bufs["novelty"].read().view(np.uint64), got.view(np.uint64)), what
            assert all(bufs[b].unchanged() for b in ("desc", "archive", "total")), what
    assert seen_short >= 1, "no case with k beyond the candidates"
    print("B = %d: %d cases x 3 builds, %d with k beyond the candidates, %d with NaN scores" % (B, ci + 1, seen_short, seen_nan))


# --------------------------------------------------------------------------------------------------------------------- add
@pytest.mark.parametrize("B", WIDTHS)
def test_add(gpu, B):
    """rem2d_novelty_add == novelty_model.add_model: archive and totals by bits; rates 0, 0.3 and 1, with and without a mask"""
    torch = gpu
    wrapped = flooded = 0
    for ci, (S, M, k, cap, which, content, offset) in enumerate(cases_for(B)):
        rng = np.random.default_rng([B, S, M, cap, which, 2])
        G = M * S
        desc = make_desc(content, G, B, rng)
        arch = rng.standard_normal((M, cap, B)).astype(f32)
        total = totals_for(cap, M, which)
        rate = (0.0, 0.3, 1.0)[(ci + WIDTHS.index(B)) % 3]
        mask = (rng.random(G) < 0.7).astype(np.uint8) if ci % 2 else None
        gen, seed = 3 + ci, (1 << 40) + ci
        thr = NM.rate_threshold(rate)
        wa, wt, took = NM.add_model(desc, S, arch, total, gen, seed, thr, mask)
        assert not took[~np.isfinite(desc).all(axis=1)].any()
        per = took.reshape(M, S).sum(axis=1)
        wrapped += int(cap > 0 and ((total % max(cap, 1)) + per > cap).any())
        flooded += int(cap > 0 and (per > cap).any())
        what = "B %d S %d M %d cap %d total %s %s rate %s mask %s" % (B, S, M, cap, total.tolist(), content, rate, mask is not None)
        for wide in BUILDS:
            bufs = dict(desc=Buf(torch, desc, offset), archive=Buf(torch, arch, offset), total=Buf(torch, total))
            if mask is not None:
                bufs["mask"] = Buf(torch, mask)
            n = descriptor(bufs, B, G, S, k, cap, gen, seed, thr)
            call(torch, wide, "rem2d_novelty_add", n)
            ga, gt = bufs["archive"].read(), bufs["total"].read()
            assert np.array_equal(gt, wt), "%s build %s: totals %s, model %s" % (what, wide, gt.tolist(), wt.tolist())
            assert np.array_equal(ga.view(np.uint32), wa.view(np.uint32)), "%s build %s: the archive differs" % (what, wide)
            assert bufs["desc"].unchanged() and (mask is None or bufs["mask"].unchanged()), what
    # another generation or seed gives other choices
    desc = np.zeros((512, B), f32)
    picks = [NM.admitted(desc, g, s, NM.rate_threshold(0.3)) for g, s in ((1, 5), (2, 5), (1, 6))]
    for (g, s), want in zip(((1, 5), (2, 5), (1, 6)), picks):
        bufs = dict(desc=Buf(torch, desc), archive=Buf(torch, np.zeros((1, 0, B), f32)), total=Buf(torch, np.zeros(1, np.int64)))
        call(torch, False, "rem2d_novelty_add", descriptor(bufs, B, 512, 512, 1, 0, g, s, NM.rate_threshold(0.3)))
        assert bufs["total"].read().tolist() == [int(want.sum())]
    assert (picks[0] != picks[1]).any() and (picks[0] != picks[2]).any()
    assert wrapped >= 1 and flooded >= 1, (wrapped, flooded)
    print("B = %d: %d cases x 3 builds, %d wrap the ring, %d add more than cap rows" % (B, ci + 1, wrapped, flooded))


def test_step_is_score_then_add(gpu):
    """rem2d_novelty_step == rem2d_novelty_score, then rem2d_novelty_add; the score is blind to the rows the call adds"""
    torch = gpu
    B, S, M, k, cap = 8, 65, 3, 15, 5
    G = M * S
    rng = np.random.default_rng(17)
    desc, arch, total = make_desc("random", G, B, rng), rng.standard_normal((M, cap, B)).astype(f32), np.array([0, 3, 12], np.int64)
    thr = NM.rate_threshold(0.3)
    want = NM.score_model(desc, S, k, arch, total)
    wa, wt, took = NM.add_model(desc, S, arch, total, 4, 9, thr)
    after = NM.score_model(desc, S, k, wa, wt)
    assert took.sum() > cap and (NM.bits64(after) != NM.bits64(want)).mean() > 0.5      # seeing the added rows would show
    for wide in BUILDS:
        one = dict(desc=Buf(torch, desc), archive=Buf(torch, arch), total=Buf(torch, total), novelty=Buf(torch, np.zeros(G, np.float64)))
        two = dict(desc=Buf(torch, desc), archive=Buf(torch, arch), total=Buf(torch, total), novelty=Buf(torch, np.zeros(G, np.float64)))
        call(torch, wide, "rem2d_novelty_step", descriptor(one, B, G, S, k, cap, 4, 9, thr))
        call(torch, wide, "rem2d_novelty_score", descriptor(two, B, G, S, k, cap, 4, 9, thr))
        call(torch, wide, "rem2d_novelty_add", descriptor(two, B, G, S, k, cap, 4, 9, thr))
        for bufs in (one, two):
            same64(bufs["novelty"].read(), want, "step, build %s" % (wide,))
            assert np.array_equal(bufs["archive"].read().view(np.uint32), wa.view(np.uint32)) and np.array_equal(bufs["total"].read(), wt)
            assert bufs["desc"].unchanged()


def test_novelty_archive(gpu):
    """novelty.NoveltyArchive: score / add / step give the model's bits, out= is written in place and nothing else is allocated, a
    checkpoint restores the ring"""
    torch = gpu
    from gym_rem2d_amd import novelty
    B, S, M, k, cap = 8, 64, 2, 15, 40
    rng = np.random.default_rng(23)
    a = novelty.NoveltyArchive(M, cap, B, device="cuda")
    arch, total = np.zeros((M, cap, B), f32), np.zeros(M, np.int64)
    out = torch.zeros(M * S, dtype=torch.float64, device="cuda")
    mask = torch.from_numpy(rng.random(M * S) < 0.8).to("cuda")
    descs = [torch.from_numpy(make_desc("random", M * S, B, rng)).to("cuda") for _ in range(4)]
    torch.cuda.synchronize()
    mem = []
    for gen, d in enumerate(descs, 1):
        got = a.step(d, gen, k=k, seed=5, rate=0.3, mask=mask, out=out)
        assert got is out
        want = NM.score_model(d.cpu().numpy(), S, k, arch, total)
        arch, total, _ = NM.add_model(d.cpu().numpy(), S, arch, total, gen, 5, NM.rate_threshold(0.3), mask.cpu().numpy())
        same64(out.cpu().numpy(), want, "NoveltyArchive.step, generation %d" % gen)
        assert np.array_equal(a.entries.cpu().numpy().view(np.uint32), arch.view(np.uint32)) and a.total.cpu().tolist() == total.tolist()
        mem.append(torch.cuda.memory_allocated())
    assert len(set(mem)) == 1 and total.max() > cap
    state = a.state_dict()
    same64(a.score(descs[0], k=3).cpu().numpy(), NM.score_model(descs[0].cpu().numpy(), S, 3, arch, total), "score")
    assert a.add(descs[0], 9, rate=1.0) is a.total and a.total.cpu().tolist() == (total + S).tolist()
    a.load_state_dict(state)
    assert np.array_equal(a.entries.cpu().numpy().view(np.uint32), arch.view(np.uint32)) and a.total.cpu().tolist() == total.tolist()
    same64(a.score(descs[1], k=k, wide="fma").cpu().numpy(), NM.score_model(descs[1].cpu().numpy(), S, k, arch, total), "score, fma build")


# ---------------------------------------------------------------------------------------------------------------- describe
def loop_env(pop, wide):
    """env_harness.make_env on three step groups"""
    from gym_rem2d_amd.env import BatchedModular2D
    terrain, morphs = CM.loop_population(pop)
    n = sum(m.n_envs for m in morphs)
    order = np.random.default_rng(5).permutation(n)
    rows, at = [], 0
    for m in morphs:
        rows.append(order[at:at + m.n_envs])
        at += m.n_envs
    env = BatchedModular2D(hardcore=(pop == "cppn"), seed=4, flags=CONT, wide=wide)
    env.step_groups = 3
    env._upload([(m, r) for m, r in zip(morphs, rows)], n)
    return env, rows, morphs


@pytest.mark.parametrize("wide", [False, True], ids=["default", "wide"])
def test_describe(gpu, oracle, wide):
    """rem2d_worlds_describe == novelty_model.describe_update fed with the oracle's closed-loop trajectory (lsystem: the oracle shows
    nobody beyond the default slots in these 120 steps), on a permuted population of four lane buckets on several step groups, for
    K in {1, 4, 16} x period in {1, 7}, each called every step and every period; every row is compared after every step, so an ended
    creature's row is held byte for byte while its wavefront neighbours go on.  Then reset_where of a few creatures, ended ones among
    them: their rows start again from the start position and nobody else's row moves."""
    torch = gpu
    from gym_rem2d_amd import novelty
    from env_harness import population_rows
    n_steps = 120
    runs = CM.closed_loop_run(oracle, "lsystem", CONT)
    assert all((CM.left_out_first(run)[0] > n_steps).all() for run in runs)              # nobody leaves the comparison
    env, rows, morphs = loop_env("lsystem", wide)
    try:
        n, Mb = env.n_envs, max(m.lanes for m in morphs)
        assert len(env.groups) >= 2 and len({w.lanes for w, _ in env.worlds}) >= 2
        px, py = np.zeros((n_steps + 1, n), f32), np.zeros((n_steps + 1, n), f32)
        for run, r in zip(runs, rows):
            for t in range(n_steps + 1):
                px[t, r], py[t, r] = run["obs"][t][:, 0], run["obs"][t][:, 1]
        frozen = NM.episode_words(px)
        assert 5 <= int(frozen[n_steps].sum()) < n - 5                                   # some end on the way, some last
        forms = [(K, p, every) for K in (1, 4, 16) for p in (1, 7) for every in (1, p)]
        want = [np.full((n, 2 * K), -7.0, f32) for K, _, _ in forms]
        bufs = [Buf(torch, w) for w in want]
        gots = [torch.as_strided(b.t, (n, 2 * K), (2 * K, 1), b.at) for b, (K, _, _) in zip(bufs, forms)]
        env.set_descriptor(7, 16)                                                        # the env's own: form (16, 7, every 7)
        own, own_want = forms.index((16, 7, 7)), np.zeros((n, 32), f32)
        compared = 0
        for t in range(n_steps + 1):
            worlds = env._control_worlds()
            for (K, p, every), w, g in zip(forms, want, gots):
                if t % every == 0:
                    NM.describe_update(w, np.full(n, t), frozen[t], px[t], py[t], p, K)
                    novelty.describe(worlds, p, K, g)
            if t % 7 == 0:
                NM.describe_update(own_want, np.full(n, t), frozen[t], px[t], py[t], 7, 16)
                assert env.describe() is env.behaviour
            for form, w, b in zip(forms, want, bufs):
                assert np.array_equal(b.read().view(np.uint32), w.view(np.uint32)), "step %d, (K, period, every) = %s" % (t, form)
                compared += n
            assert np.array_equal(env.behaviour.cpu().numpy().view(np.uint32), own_want.view(np.uint32)), "step %d, env.describe()" % t
            if t == n_steps:
                break
            env.set_joint_targets(torch.from_numpy(population_rows(runs, rows, "targets", t, Mb)))
            env.step(1)
        assert np.array_equal(env.frozen.cpu().numpy() != 0, frozen[n_steps] != 0) and (env.steps.cpu().numpy() == n_steps).all()
        assert np.array_equal(want[own], own_want)
        # a masked reset in the middle of it all
        pick = np.zeros(n, bool)
        pick[np.flatnonzero(frozen[n_steps] != 0)[:3]] = True
        pick[np.flatnonzero(frozen[n_steps] == 0)[:3]] = True
        ended = env.reset_where(mask=torch.from_numpy(pick).to("cuda"))
        assert np.array_equal(ended.cpu().numpy() != 0, pick)
        before = env.behaviour.cpu().numpy().copy()
        got = env.describe().cpu().numpy()
        assert (got[pick, 0::2] == px[0, pick, None]).all() and (got[pick, 1::2] == py[0, pick, None]).all()
        assert np.array_equal(got[~pick].view(np.uint32), before[~pick].view(np.uint32)) and (got[pick] != before[pick]).any()
        print("describe (%s build): %d rows compared over %d steps in %d forms; %d creatures ended on the way"
              % ("wide" if wide else "default", compared, n_steps, len(forms), int(frozen[n_steps].sum())))
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------------------- generations
def behaviour_replay(O, terrain, morphs, rows, weights, flags, n_steps, max_bodies, period, samples):
    """evolve_model.episode_replay that also describes: the oracle's closed loop under the weight sets, from reset, with
    describe_update at step 0 and after every `period` steps -> (fitness float64 [n], behaviour float32 [n, 2 samples], gone)"""
    import range_model as R
    T = R.Terrain.of(terrain)
    rays = R.bipedal_rays()
    n = sum(len(r) for r in rows)
    fitness, gone, beh = np.zeros(n, np.float64), np.zeros(n, bool), np.zeros((n, 2 * samples), f32)
    for morph, r in zip(morphs, rows):
        loop = CM.OracleLoop(O, terrain, morph, flags, "replay")
        ctx = loop.ctx
        W = [a[np.asarray(r)] for a in weights]
        run = dict(ctx=ctx, caps=[], obs=[])
        mine = np.zeros((ctx.N, 2 * samples), f32)
        for t in range(n_steps + 1):
            snap = loop.snapshot()
            run["obs"].append(None)
            run["caps"].append(np.stack([snap["ccount"].max(axis=1),
                                         ((snap["ctouch"] != 0) & CM.F.masks(ctx, snap)["cedge"]).sum(axis=0).max(axis=1)], 1))
            if t % period == 0 and t <= period * samples:
                NM.describe_update(mine, loop.env["steps"], loop.env["frozen"], snap["px"][:, 0], snap["py"][:, 0], period, samples)
            if t == n_steps:
                break
            obs = CM.observe_model(ctx, snap, max_bodies)
            frac = R.cast(T, snap["px"][:, 0], snap["py"][:, 0], rays)[0]
            tg, valid = PM.forward_model(PM.input_rows(obs, frac), *W)
            loop.set_targets(tg, mask=valid)
            loop.step()
        fitness[r], beh[r] = loop.env["fitness"], mine
        gone[r] = CM.left_out_first(run)[0] < len(run["obs"])
    return fitness, beh, gone


def _arrays(p):
    return [t.cpu().numpy() for t in (p.w1, p.b1, p.w2, p.b2)]


def same_bits(got, want, what):
    for k, name in enumerate(("w1", "b1", "w2", "b2")):
        assert np.array_equal(ES.bits(got[k]), ES.bits(want[k])), "%s: %s differs" % (what, name)


NSES = dict(steps=60, S=16, K=4, period=15, k=5, cap=6, rate=0.3, sigma=0.1, lr=0.5, seed=7)


def nses_host_generations(oracle):
    """-> (batches, W, want): the population, the first mean and the host's two generations under weights (1, 1)"""
    from gym_rem2d_amd import make_terrain, synthetic
    from gym_rem2d_amd.compiler import Morphology, lanes_for
    specs = [s for s in synthetic.lsystem_specs(range(120)) if s.n_bodies >= 2][:64]
    n, steps, S, K, period, k, cap, rate = (len(specs),) + tuple(NSES[q] for q in ("steps", "S", "K", "period", "k", "cap", "rate"))
    sigma, lr, seed = NSES["sigma"], NSES["lr"], NSES["seed"]
    M = n // S
    groups = {}
    for e, s in enumerate(specs):
        groups.setdefault(lanes_for(s.n_bodies), []).append(e)
    batches = [(Morphology.from_specs([specs[e] for e in groups[g]], g), groups[g]) for g in sorted(groups)]
    morphs, rows = [m for m, _ in batches], [np.asarray(idx) for _, idx in batches]
    terrain = make_terrain(4)
    W = list(PM.loop_weights(M, 16))
    step = ES.step_for(lr, S, sigma)
    want, mean = [], W
    arch, total = np.zeros((M, cap, 2 * K), f32), np.zeros(M, np.int64)
    for gen in (1, 2):
        kids = ES.sample_model(mean, S, sigma, seed, gen)
        fit, beh, gone = behaviour_replay(oracle, terrain, morphs, rows, kids, CONT, steps, PM.LOOP_BODIES, period, K)
        assert not gone.any()
        nov = NM.score_model(beh, S, k, arch, total)
        arch, total, _ = NM.add_model(beh, S, arch, total, gen, seed, NM.rate_threshold(rate))
        util = NM.combine_util(ES.shape_model(fit, S), ES.shape_model(nov, S), (1, 1))
        mean = ES.update_model(mean, util, S, step, seed, gen)
        want.append(dict(kids=kids, fit=fit, beh=beh, nov=nov, arch=arch.copy(), total=total.copy(), util=util, mean=mean))
    # the replay is worth comparing with: most creatures move, a ring wraps, novelty changes the ranks
    assert (want[0]["beh"][:, 0::2].std(axis=1) > 0).sum() > n // 2 and total.max() > cap
    assert (want[1]["util"] != 2 * ES.shape_model(want[1]["fit"], S)).any() and np.isfinite(want[1]["nov"]).all()
    return batches, W, want


def test_two_generations_of_nses(gpu, oracle):
    """evaluate.run_policy_nses on 64 L-system creatures in blocks of 16 around 4 means, episodes of 60 steps described 4 times:
    two generations under weights (1, 1) give the host replay's children, fitness, behaviour, novelty, archive, totals, util and mean;
    three under (1, 0) are run_policy_es bit for bit, and the third allocates nothing."""
    torch = gpu
    from gym_rem2d_amd import evaluate, novelty, policy
    from gym_rem2d_amd.env import BatchedModular2D
    batches, W, want = nses_host_generations(oracle)
    n = sum(m.n_envs for m, _ in batches)
    steps, S, K, period, k, cap, rate, sigma, lr, seed = (NSES[q] for q in ("steps", "S", "K", "period", "k", "cap", "rate", "sigma", "lr", "seed"))
    M = n // S
    env = BatchedModular2D(seed=4, flags=evaluate.EVAL_FLAGS)
    try:
        env.reset_batches(batches, n)
        first = policy.MLPPolicy(*[torch.from_numpy(a.copy()) for a in W]).to("cuda")
        archive = novelty.NoveltyArchive(M, cap, 2 * K, device="cuda")
        seen = []

        def keep(g, kids, f, m, b, nv, u):
            seen.append(dict(kids=_arrays(kids), fit=f.cpu().numpy(), beh=b.cpu().numpy(), nov=nv.cpu().numpy(), util=u.cpu().numpy(),
                             mean=_arrays(m), arch=archive.entries.cpu().numpy(), total=archive.total.cpu().numpy()))
        last, fit, history = evaluate.run_policy_nses(env, first, 2, archive, k=k, rate=rate, weights=(1, 1), period=period, samples=K,
                                                      seed=seed, sigma=sigma, lr=lr, group_size=S, max_steps=steps, on_generation=keep)
        assert len(seen) == 2 and [h[0] for h in history] == [1, 2]
        for g, (got, w) in enumerate(zip(seen, want), 1):
            same_bits(got["kids"], w["kids"], "children of generation %d" % g)
            assert np.array_equal(got["fit"].view(np.uint64), w["fit"].view(np.uint64)), "generation %d: fitness" % g
            assert np.array_equal(got["beh"].view(np.uint32), w["beh"].view(np.uint32)), "generation %d: behaviour" % g
            same64(got["nov"], w["nov"], "generation %d: novelty" % g)
            assert np.array_equal(got["arch"].view(np.uint32), w["arch"].view(np.uint32)) and np.array_equal(got["total"], w["total"])
            assert np.array_equal(got["util"], w["util"]), "generation %d: util" % g
            same_bits(got["mean"], w["mean"], "mean after generation %d" % g)
        same_bits(_arrays(last), want[1]["mean"], "the final mean")
        # weights (1, 0): run_policy_es, bit for bit; the third generation allocates nothing
        es_seen, ns_seen, mem = [], [], []
        evaluate.run_policy_es(env, first, 3, seed=seed, sigma=sigma, lr=lr, group_size=S, max_steps=steps, chunk=30,
                               on_generation=lambda g, kids, f, m: es_seen.append((_arrays(kids), f.cpu().numpy(), _arrays(m), m.util.cpu().numpy())))
        archive2 = novelty.NoveltyArchive(M, cap, 2 * K, device="cuda")

        def keep0(g, kids, f, m, b, nv, u):
            ns_seen.append((_arrays(kids), f.cpu().numpy(), _arrays(m), u.cpu().numpy()))
            torch.cuda.synchronize()
            mem.append(torch.cuda.memory_allocated())
        evaluate.run_policy_nses(env, first, 3, archive2, k=k, rate=rate, weights=(1, 0), period=period, samples=K, seed=seed, sigma=sigma,
                                 lr=lr, group_size=S, max_steps=steps, on_generation=keep0)
        assert len(es_seen) == len(ns_seen) == 3
        for g, (a, b) in enumerate(zip(es_seen, ns_seen), 1):
            same_bits(a[0], b[0], "(1, 0) children, generation %d" % g)
            assert np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)) and np.array_equal(a[3], b[3])
            same_bits(a[2], b[2], "(1, 0) mean, generation %d" % g)
        assert mem[2] == mem[1], mem
        assert archive2.total.cpu().numpy().sum() > 0
    finally:
        env.close()
