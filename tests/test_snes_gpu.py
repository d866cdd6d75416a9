"""The adaptive evolution strategy for device policies on a real MI355X (pytest -m gpu): the sample and update kernels against
tests/snes_model.py, in the three builds, their reductions to rem2d_es_*, policy.SeparableES, and two generations of
evaluate.run_policy_snes against the host replay (include/rem2d_snes.h).  Every comparison is on bits, every NaN mapped to one
pattern first (es_model.bits says why); every written buffer lies between guard words, and the inputs are read back unchanged."""
import ctypes as C

import numpy as np
import pytest

import es_model as ES
import evolve_model as EM
import policy_model as PM
import snes_model as SN
from test_es_gpu import BUILDS, SHAPES, SPECIAL, forge_mean, guarded, offset_copy, same_bits, unguard

pytestmark = pytest.mark.gpu

CONT = 1
f32 = np.float32
ARRAYS = ("w1", "b1", "w2", "b2")
NAMES = ("mean", "sigma", "m1", "m2")
BOUNDS = (1e-6, 10.0)
ADAM3 = (0.9, 0.999, 1e-8)


@pytest.fixture(scope="module")
def gpu():
    import replay
    return replay.need_gpu()


def plant(rng, arrays, words):
    """a few of `words` at random places of every set of every array (all of them where the array is long enough)"""
    words = np.asarray(words, f32)
    for a in arrays:
        flat = a.reshape(a.shape[0], -1)
        n = flat.shape[1]
        for g in range(flat.shape[0]):
            at = rng.choice(n, size=min(n, len(words)), replace=False)
            flat[g, at] = rng.permutation(words)[:len(at)]
    return arrays


def forge_state(MB, R, H, M, seed):
    """sigma, m1, m2 of the mean's shapes: sigma positive with NaN, +-inf, denormals, +-0, a negative word and words AT both clamp
    bounds; m1 any sign with the special words; m2 small and positive with a negative and a denormal word among the special ones"""
    rng = np.random.default_rng([MB, R, H, M, seed, 3])
    like = forge_mean(MB, R, H, M, seed, special=False)
    sigma = [(np.abs(rng.standard_normal(a.shape)) * 0.1 + 0.01).astype(f32) for a in like]
    m1 = [(rng.standard_normal(a.shape) * 0.01).astype(f32) for a in like]
    m2 = [(rng.standard_normal(a.shape) ** 2 * 1e-4).astype(f32) for a in like]
    plant(rng, sigma, np.concatenate([SPECIAL, np.array([-0.25, BOUNDS[0], BOUNDS[1]], f32)]))
    plant(rng, m1, SPECIAL)
    plant(rng, m2, np.concatenate([np.array([-1e-4], f32), np.array([0x00000001, 0x00400000], np.uint32).view(f32), SPECIAL]))
    return sigma, m1, m2


def snes_descriptor(_lib, shape, M, S, seed, gen, flags=0, c=None, pair_chunk=0, fitness=None, util=None, scratch=None, **buffers):
    """buffers: prefix ("", "sigma_", "child_", "new_m1_", ...) with the trailing underscore dropped -> four tensors"""
    MB, R, H = shape
    e = _lib.Snes()
    e.d, e.hidden, e.max_bodies, e.n_means, e.group_size, e.pair_chunk = 8 + 6 * MB + R, H, MB, M, S, pair_chunk
    e.generation, e.flags, e.seed = gen, flags, seed
    for k, v in (c or SN.scalars(S)).items():
        setattr(e, k, float(v))
    e.fitness = None if fitness is None else fitness.data_ptr()
    e.util = None if util is None else util.data_ptr()
    for prefix, tensors in buffers.items():
        for k, t in zip(ARRAYS, tensors):
            setattr(e, (prefix + "_" + k) if prefix != "mean" else k, t.data_ptr())
    if scratch is not None:
        e.scratch, e.scratch_bytes = scratch.data_ptr(), scratch.numel() * 8
    return e


def call(torch, _lib, name, e, wide):
    _lib.check(getattr(_lib.lib(wide), name)(C.byref(e), C.c_void_p(torch.cuda.current_stream().cuda_stream)), wide)


def unchanged(src, W, what):
    for s, a in zip(src, W):
        assert np.array_equal(s.cpu().numpy().view(np.uint32), a.view(np.uint32)), what + " was written"


# ------------------------------------------------------------------------------------------------------------------ sample
def run_sample(torch, _lib, shape, W, sigma, S, seed, gen, wide, off):
    M = W[0].shape[0]
    src, sg = [offset_copy(torch, a, off) for a in W], [offset_copy(torch, a, off) for a in sigma]
    kid_shapes = [(M * S,) + a.shape[1:] for a in W]
    bufs, kids = zip(*[guarded(torch, s, off) for s in kid_shapes])
    assert all(t.data_ptr() % 16 == (4 * off) % 16 for t in src + sg + list(kids))
    e = snes_descriptor(_lib, shape, M, S, seed, gen, mean=src, sigma=sg, child=kids)
    call(torch, _lib, "rem2d_snes_sample", e, wide)
    unchanged(src, W, "the mean")
    unchanged(sg, sigma, "sigma")
    return [unguard(b, s, off, "a child buffer") for b, s in zip(bufs, kid_shapes)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "MB%d-R%d-H%d" % s)
def test_sample(gpu, shape):
    """rem2d_snes_sample == the model: M of 1, 3 x S of 2, 6, 66, the mean and sigma full of NaN payloads, infinities, denormals,
    signed zeros and a negative sigma, the bases 16-byte aligned and, every third case, 4 bytes off (the V = 1 path on misaligned
    bases).  M = 3, S = 6 also in the wide and the fma build."""
    torch = gpu
    from gym_rem2d_amd import _lib
    rng = np.random.default_rng([shape[2], 15])
    combo = n_nan = 0
    for M in (1, 3):
        W = forge_mean(*shape, M, 1)
        sigma = forge_state(*shape, M, 1)[0]
        for S in (2, 6, 66):
            combo += 1
            off = 1 if combo % 3 == 0 else 0
            seed, gen = int(rng.integers(0, 2 ** 63)) * 2 + 1, int(rng.integers(0, 2 ** 32))
            want = SN.sample_model(W, sigma, S, seed, gen)
            for wide in (BUILDS if (M, S) == (3, 6) else (False,)):
                got = run_sample(torch, _lib, shape, W, sigma, S, seed, gen, wide, off)
                same_bits(got, want, "M=%d S=%d off=%d build=%s" % (M, S, off, wide))
            n_nan += sum(int(np.isnan(a).sum()) for a in want)
    assert n_nan > 0


# ------------------------------------------------------------------------------------------------------------------ update
def util_cases(M, S, rng):
    """model-made util (random fitness, ties) and caller-filled: all zeros, the extreme d, LEVEL pairs (util[a] == util[a + 1] =
    +-(S - 1): d = 0 and p != 0), any int32"""
    G = M * S
    ext = np.empty(G, np.int32)
    ext[0::2], ext[1::2] = S - 1, -(S - 1)
    level = np.repeat(np.where(rng.random(G // 2) < 0.5, S - 1, -(S - 1)).astype(np.int32), 2)
    return {"ranks": ES.shape_model(rng.standard_normal(G), S), "ties": ES.shape_model(rng.integers(0, 3, G).astype(np.float64), S),
            "zeros": np.zeros(G, np.int32), "extreme": ext, "level": level, "any": rng.integers(-2 ** 31, 2 ** 31, G).astype(np.int32)}


def run_update(torch, _lib, shape, state, util, S, c, flags, seed, gen, wide, off, pair_chunk, name="rem2d_snes_update", fitness=None):
    """state: (mean, sigma, m1, m2) -> (the new (mean, sigma, m1, m2) -- the moments None without ADAM --, util after the call, the
    scratch bytes the library asked for)"""
    W = state[0]
    M = W[0].shape[0]
    adam = bool(flags & SN.ADAM)
    n_in = 4 if adam else 2
    src = [[offset_copy(torch, a, off) for a in arrays] for arrays in state[:n_in]]
    outs = [list(zip(*[guarded(torch, a.shape, off) for a in W])) for _ in range(n_in)]
    ud = torch.from_numpy(np.asarray(util, np.int32).copy()).to("cuda")
    fd = None if fitness is None else torch.from_numpy(fitness).to("cuda")
    buffers = dict(mean=src[0], sigma=src[1], new=outs[0][1], new_sigma=outs[1][1])
    if adam:
        buffers.update(m1=src[2], m2=src[3], new_m1=outs[2][1], new_m2=outs[3][1])
    e = snes_descriptor(_lib, shape, M, S, seed, gen, flags, c, pair_chunk, fd, ud, **buffers)
    need = int(_lib.lib(wide).rem2d_snes_scratch_bytes(C.byref(e)))
    assert need >= 0 and need % 16 == 0
    sbuf = None
    if need:
        sbuf, scratch = guarded(torch, (need // 8,), 0, torch.int64, -99)
        e.scratch, e.scratch_bytes = scratch.data_ptr(), need
    call(torch, _lib, name, e, wide)
    if sbuf is not None:
        unguard(sbuf, (need // 8,), 0, "scratch")
    if fd is not None:
        assert np.array_equal(fd.cpu().numpy().view(np.uint64), fitness.view(np.uint64)), "fitness was written"
    for s, arrays, what in zip(src, state, NAMES):
        unchanged(s, arrays, what)
    got = [[unguard(b, a.shape, off, "the new " + what) for b, a in zip(bufs, W)] for (bufs, _), what in zip(outs, NAMES)]
    return got + [None] * (4 - n_in), ud.cpu().numpy(), need


def same_state(got, want, what):
    for g, w, name in zip(got, want, NAMES):
        assert (g is None) == (w is None), what
        if w is not None:
            same_bits(g, w, what + " new " + name)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "MB%d-R%d-H%d" % s)
def test_update(gpu, shape):
    """rem2d_snes_update == the model: M of 1, 3 x S of 2, 6, 64, 66, six kinds of util, pair_chunk 0, 1, 2 and S / 2 -- with and
    without the split through scratch -- all equal to each other and to the model; the four flag combinations in turn, and all four
    on every util at M = 3, S = 6, which also runs in the wide and fma builds.  The state carries the special words."""
    torch = gpu
    from gym_rem2d_amd import _lib
    rng = np.random.default_rng([shape[2], 16])
    combo = split = 0
    seen = set()
    for M in (1, 3):
        W = forge_mean(*shape, M, 2)
        state = (W,) + forge_state(*shape, M, 2)
        for S in (2, 6, 64, 66):
            cases = util_cases(M, S, rng)
            names = list(cases) if S in (6, 66) else ["ranks", "level"]
            for name in names:
                util = cases[name]
                combo += 1
                off = 1 if combo % 3 == 0 else 0
                seed, gen = int(rng.integers(0, 2 ** 63)) * 2 + 1, int(rng.integers(0, 2 ** 32))
                for flags in (range(4) if (M, S) == (3, 6) else (combo % 4,)):
                    c = SN.scalars(S, adam=ADAM3 if flags & SN.ADAM else None, t=1 + combo % 3, sigma_bounds=BOUNDS)
                    want = SN.update_model(*state, util, S, c, flags, seed, gen)
                    seen.add((name, flags))
                    for wide in (BUILDS if (M, S) == (3, 6) else (False,)):
                        for chunk in sorted({0, 1, 2, S // 2}):
                            what = "M=%d S=%d util=%s flags=%d off=%d chunk=%d build=%s" % (M, S, name, flags, off, chunk, wide)
                            got, after, need = run_update(torch, _lib, shape, state, util, S, c, flags, seed, gen, wide, off, chunk)
                            assert np.array_equal(after, util), what + ": util was written"
                            same_state(got, want, what)
                            assert (need > 0) == (chunk != 0 and chunk < S // 2), what
                            split += need > 0
    assert split > 0 and {f for _, f in seen} == {0, 1, 2, 3} and {n for n, _ in seen} == set(util_cases(1, 2, rng))


def test_update_of_a_large_block(gpu):
    """One block of S = 8192 children of the 17-word policy, level pairs and ranks: |h| passes 2^40; the library's own split, no
    split and chunks of 1000 pairs give the model's bits"""
    torch = gpu
    from gym_rem2d_amd import _lib
    shape, S = (1, 0, 1), SN.MAX_GROUP
    W = forge_mean(*shape, 1, 3, special=False)
    sigma, m1, m2 = ([np.full_like(a, v) for a in W] for v in (0.1, 0.0, 0.0))
    rng = np.random.default_rng(S)
    level = np.repeat(np.where(rng.random(S // 2) < 0.75, S - 1, -(S - 1)).astype(np.int32), 2)
    seed, gen = 0x123456789abcdef1, 9
    flags = SN.ADAM | SN.NATURAL
    for name, util, c in (("level", level, dict(SN.scalars(S, adam=ADAM3, t=2), sstep=f32(2.0 ** -22))),
                          ("ranks", ES.shape_model(rng.standard_normal(S), S), SN.scalars(S, adam=ADAM3, t=2))):
        h = SN.second_sums(util, S, 14, 1, 0, seed, gen)
        assert np.abs(h).max() > 2 ** 40
        want = SN.update_model(W, sigma, m1, m2, util, S, c, flags, seed, gen)
        assert (SN.bits(want[1][0]) != SN.bits(sigma[0])).mean() > 0.9
        needs = []
        for chunk in (0, S // 2, 1000):
            got, _, need = run_update(torch, _lib, shape, (W, sigma, m1, m2), util, S, c, flags, seed, gen, False, 0, chunk)
            same_state(got, want, "S=%d util=%s chunk=%d" % (S, name, chunk))
            needs.append(need)
        assert needs[1] == 0 and needs[2] > 0 and needs[0] > 0
        print("S=%d %s: max |h| = 2^%.1f, scratch of the library's choice %d bytes" % (S, name, np.log2(float(np.abs(h).max())), needs[0]))


# ----------------------------------------------------------------------------------------------------- against rem2d_es_*
def test_reductions_to_the_plain_strategy(gpu):
    """A sigma array of one value: rem2d_snes_sample writes rem2d_es_sample's bits.  flags 0 and sstep = 0: the new mean is
    rem2d_es_update's and the new sigma is sigma; likewise rem2d_snes_step against rem2d_es_step, util included"""
    torch = gpu
    from gym_rem2d_amd import _lib
    import test_es_gpu as TG
    for shape, M, S, chunk in (((4, 3, 5), 3, 66, 0), ((16, 10, 32), 2, 16, 3)):
        W = forge_mean(*shape, M, 4)
        rng = np.random.default_rng([M, S, 1])
        seed, gen, step = 0xfedcba9876543210, 4000000000, ES.step_for(0.05, S, 0.1)
        sigma = [np.full_like(a, 0.1) for a in W]
        es_kids = TG.run_sample(torch, _lib, shape, W, S, 0.1, seed, gen, False, 0)
        kids = run_sample(torch, _lib, shape, W, sigma, S, seed, gen, False, 0)
        for a, b in zip(kids, es_kids):
            assert np.array_equal(ES.bits(a), ES.bits(b)), "snes_sample != es_sample"
        fit = rng.integers(0, 9, M * S).astype(np.float64)
        fit[rng.integers(M * S)] = np.nan
        c = dict(SN.scalars(S), mstep=step, sstep=f32(0.0))
        varied = [(np.abs(rng.standard_normal(a.shape)) * 0.1 + 0.01).astype(f32) for a in W]
        for name, es_name, util in (("rem2d_snes_update", "rem2d_es_update", ES.shape_model(fit, S)), ("rem2d_snes_step", "rem2d_es_step", np.full(M * S, -7))):
            es_new, es_util, _ = TG.run_update(torch, _lib, shape, W, util, S, step, seed, gen, False, 0, chunk, es_name, fit)
            got, after, _ = run_update(torch, _lib, shape, (W, varied, None, None), util, S, c, 0, seed, gen, False, 0, chunk, name, fit)
            assert np.array_equal(after, es_util) and np.array_equal(after, ES.shape_model(fit, S)), name
            for a, b in zip(got[0], es_new):
                assert np.array_equal(ES.bits(a), ES.bits(b)), name + ": the new mean is not the ES's"
            for a, b in zip(got[1], varied):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name + ": sigma moved with sstep = 0"


# ------------------------------------------------------------------------------------------------------------------ Python
def _arrays(ts):
    return [t.cpu().numpy() for t in ts]


def _weights(p):
    return _arrays((p.w1, p.b1, p.w2, p.b2))


def test_separable_es_on_the_device(gpu):
    """policy.SeparableES with Adam, natural: three generations equal the model driven by the same fitness, t and the folded alpha
    included; after generation 2 every buffer is one seen before and nothing is allocated; state() -> load_state() continues with the
    same bits; util= skips the ranking"""
    torch = gpu
    from gym_rem2d_amd import policy
    M, S, seed = 3, 16, 11
    kw = dict(sigma=0.2, lr=0.03, lr_sigma=3.0, adam=ADAM3, natural=True, sigma_bounds=(1e-4, 5.0))
    first = policy.MLPPolicy.random(M, 4, 5, n_rays=3, seed=3, activation="relu", scale=1.25).to("cuda")
    before = _weights(first)
    es = policy.SeparableES(first, S, **kw)
    mean, sigma = _weights(first), [np.full_like(a, 0.2) for a in before]
    m1, m2 = [np.zeros_like(a) for a in before], [np.zeros_like(a) for a in before]
    fits = [torch.from_numpy(np.random.default_rng(g).standard_normal(M * S)).to("cuda") for g in range(4)]
    seen, held, saved = [], None, None
    for g in range(1, 4):
        kids = es.sample(g, seed=seed)
        same_bits(_weights(kids), SN.sample_model(mean, sigma, S, seed, g), "children of generation %d" % g)
        assert (kids.activation, kids.scale, kids.n_sets, kids.index) == ("relu", 1.25, M * S, None) and np.array_equal(kids.rays, first.rays)
        new = es.update(fits[g - 1], g, seed=seed, pair_chunk=3)
        assert new is es.mean and es.t == g
        util = ES.shape_model(fits[g - 1].cpu().numpy(), S)
        c = SN.scalars(S, t=g, **{k: v for k, v in kw.items() if k != "natural"})
        assert np.array_equal(new.util.cpu().numpy(), util)
        mean, sigma, m1, m2 = SN.update_model(mean, sigma, m1, m2, util, S, c, SN.ADAM | SN.NATURAL, seed, g)
        same_state((_weights(new), _arrays(es.sigma), _arrays(es.m1), _arrays(es.m2)), (mean, sigma, m1, m2), "generation %d" % g)
        ptrs = tuple(t.data_ptr() for t in (new.w1, es.sigma[0], es.m1[1], es.m2[2], new.util, kids.w1, es._scratch))
        if g == 1:
            torch.cuda.synchronize()
            held = torch.cuda.memory_allocated()
        else:
            assert torch.cuda.memory_allocated() == held, "generation %d allocated device memory" % g
        if g == 3:
            assert ptrs == seen[0] and ptrs != seen[1]
        seen.append(ptrs)
        if g == 2:
            saved = es.state()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(_weights(first), before)), "the caller's mean was written"
    # a checkpoint taken after generation 2, loaded into a fresh object, gives generation 3's bits
    assert saved["t"] == 2 and all(t.device.type == "cpu" for k in NAMES for t in saved[k])
    other = policy.SeparableES(first, S, **kw)
    other.load_state(saved)
    same_bits(_weights(other.sample(3, seed=seed)), _weights(es._children), "the children after load_state")
    again = other.update(fits[2], 3, seed=seed)
    assert other.t == 3
    same_state((_weights(again), _arrays(other.sigma), _arrays(other.m1), _arrays(other.m2)), (mean, sigma, m1, m2), "after load_state")
    # util=: the caller's utilities, no ranking
    mine = torch.from_numpy(np.random.default_rng(2).integers(-S, S, M * S).astype(np.int32)).to("cuda")
    new = es.update(None, 4, seed=seed, util=mine)
    assert new.util is mine and es.t == 4
    c = SN.scalars(S, t=4, **{k: v for k, v in kw.items() if k != "natural"})
    want = SN.update_model(mean, sigma, m1, m2, mine.cpu().numpy(), S, c, SN.ADAM | SN.NATURAL, seed, 4)
    same_state((_weights(new), _arrays(es.sigma), _arrays(es.m1), _arrays(es.m2)), want, "util=")


# ------------------------------------------------------------------------------------------------------------- generations
def test_two_generations_give_the_replays_fitness(gpu, oracle):
    """evaluate.run_policy_snes on 16 L-system creatures in blocks of 8 around 2 means, two generations of episodes capped at 60
    steps: each generation's fitness is the host replay's -- snes_model for the weights, the oracle's closed loop for the episode --
    and so are the means, sigma and the history rows"""
    torch = gpu
    from gym_rem2d_amd import evaluate, make_terrain, policy, synthetic
    from gym_rem2d_amd.compiler import Morphology, lanes_for
    from gym_rem2d_amd.env import BatchedModular2D
    specs = [s for s in synthetic.lsystem_specs(range(60)) if s.n_bodies >= 2][:16]
    n, steps, S = len(specs), 60, 8
    M = n // S
    groups = {}
    for e, s in enumerate(specs):
        groups.setdefault(lanes_for(s.n_bodies), []).append(e)
    batches = [(Morphology.from_specs([specs[e] for e in groups[k]], k), groups[k]) for k in sorted(groups)]
    morphs, rows = [m for m, _ in batches], [np.asarray(idx) for _, idx in batches]
    terrain = make_terrain(4)
    W = list(PM.loop_weights(M, 16))
    sigma0, lr, seed = 0.1, 0.5, 7
    c = SN.scalars(S, sigma=sigma0, lr=lr, lr_sigma=4.0)
    want_fit, want_kids, want_mean, want_sigma = [], [], [W], [[np.full_like(a, sigma0) for a in W]]
    for gen in (1, 2):
        want_kids.append(SN.sample_model(want_mean[-1], want_sigma[-1], S, seed, gen))
        fit, gone = EM.episode_replay(oracle, terrain, morphs, rows, want_kids[-1], CONT, steps, PM.LOOP_BODIES)
        assert not gone.any()
        want_fit.append(fit)
        new = SN.update_model(want_mean[-1], want_sigma[-1], None, None, ES.shape_model(fit, S), S, c, 0, seed, gen)
        want_mean.append(new[0])
        want_sigma.append(new[1])
    assert (want_fit[0] != want_fit[1]).any() and (ES.bits(want_sigma[1][0]) != ES.bits(want_sigma[2][0])).mean() > 0.5
    env = BatchedModular2D(seed=4, flags=evaluate.EVAL_FLAGS)
    seen = []
    try:
        env.reset_batches(batches, n)
        first = policy.MLPPolicy(*[torch.from_numpy(a.copy()) for a in W]).to("cuda")
        es = policy.SeparableES(first, S, sigma=sigma0, lr=lr, lr_sigma=4.0)
        last, fit, history = evaluate.run_policy_snes(
            env, es, 2, seed=seed, max_steps=steps, chunk=30,
            on_generation=lambda g, k, f, m: seen.append((g, _weights(k), f.clone().cpu().numpy(), _weights(m), _arrays(es.sigma), m.util.cpu().numpy())))
        assert [s[0] for s in seen] == [1, 2] and fit.dtype == torch.float64 and fit.device.type == "cuda" and es.t == 2
        for (g, kids, got, mean, sigma, util), wk, wf, wm, ws in zip(seen, want_kids, want_fit, want_mean[1:], want_sigma[1:]):
            same_bits(kids, wk, "children of generation %d" % g)
            assert np.array_equal(got.view(np.uint64), wf.view(np.uint64)), "generation %d: the fitness differs from the replay's" % g
            assert np.array_equal(util, ES.shape_model(wf, S))
            same_bits(mean, wm, "mean after generation %d" % g)
            same_bits(sigma, ws, "sigma after generation %d" % g)
        assert last is es.mean and last.n_sets == M and env.policy.n_sets == n
        same_bits(_weights(last), want_mean[2], "the final mean")
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(_weights(first), W)), "the caller's mean was written"
        assert [h[0] for h in history] == [1, 2]
        for h, want in zip(history, want_fit):
            assert h[1] == want.min() and h[2] == want.max() and abs(h[3] - want.mean()) <= 1e-12 * abs(want.mean())
    finally:
        env.close()
