"""The evolution strategy for device policies on a real MI355X (pytest -m gpu): the sample, shape and update kernels against
tests/es_model.py, in the three builds, MLPPolicy.es_sample / es_update, and two generations of evaluate.run_policy_es against the
host replay (include/rem2d_es.h).  Every comparison is on bits: ``view(uint32)`` of the weights -- every NaN mapped to one pattern
first (es_model.bits says why) -- and int32 util."""
import ctypes as C

import numpy as np
import pytest

import es_model as ES
import evolve_model as EM
import policy_model as PM

pytestmark = pytest.mark.gpu

CONT = 1
f32 = np.float32
BUILDS = (False, True, "fma")
GUARD = 64                                   # guard words in front of and behind every written buffer
SENTINEL = -12345.678                        # what guards and not-yet-written words hold
SHAPES = [(1, 0, 1), (4, 3, 5), (16, 10, 32)]          # (MB, R, H): per-set lengths 14 1 1 1 (all dword) / 175 5 20 4 (mixed) /
#                                                        3648 32 512 16 (all dwordx4 when the bases are aligned)
TILE = 256                                   # ES_TILE of csrc/rem2d_es.h
SPECIAL = np.array([0x7fc00000, 0xffc01234, 0x7f800001, 0x7f800000, 0xff800000, 0x00000001, 0x807fffff, 0x00400000, 0x80000000,
                    0x00000000], np.uint32).view(f32)  # NaNs with payloads (one signalling), +-inf, denormals, +-0


@pytest.fixture(scope="module")
def gpu():
    import replay
    return replay.need_gpu()


def lengths(MB, R, H):
    D = 8 + 6 * MB + R
    return D, ((D, H), (H,), (H, MB), (MB,))


def forge_mean(MB, R, H, M, seed, special=True):
    """M mean sets: a normal bulk, and in every array of every set a few of SPECIAL (all of them where the array is long enough)"""
    rng = np.random.default_rng([MB, R, H, M, seed])
    D, shapes = lengths(MB, R, H)
    W = [(rng.standard_normal((M,) + s) * 0.3).astype(f32) for s in shapes]
    if special:
        for a in W:
            flat = a.reshape(M, -1)
            n = flat.shape[1]
            for g in range(M):
                at = rng.choice(n, size=min(n, len(SPECIAL)), replace=False)
                flat[g, at] = rng.permutation(SPECIAL)[:len(at)]
    return W


def descriptor(_lib, MB, R, H, M, S, seed, gen, sigma=0.0, step=0.0, pair_chunk=0, fitness=None, util=None, mean=None, kids=None,
               new=None, scratch=None):
    D, _ = lengths(MB, R, H)
    e = _lib.Es()
    e.d, e.hidden, e.max_bodies, e.n_means, e.group_size, e.pair_chunk = D, H, MB, M, S, pair_chunk
    e.generation, e.reserved, e.seed, e.sigma, e.step = gen, 0, seed, sigma, step
    e.fitness = None if fitness is None else fitness.data_ptr()
    e.util = None if util is None else util.data_ptr()
    if mean is not None:
        e.w1, e.b1, e.w2, e.b2 = (t.data_ptr() for t in mean)
    if kids is not None:
        e.child_w1, e.child_b1, e.child_w2, e.child_b2 = (t.data_ptr() for t in kids)
    if new is not None:
        e.new_w1, e.new_b1, e.new_w2, e.new_b2 = (t.data_ptr() for t in new)
    if scratch is not None:
        e.scratch, e.scratch_bytes = scratch.data_ptr(), scratch.numel() * 8
    return e


def call(torch, _lib, name, e, wide):
    L = _lib.lib(wide)
    _lib.check(getattr(L, name)(C.byref(e), C.c_void_p(torch.cuda.current_stream().cuda_stream)), wide)


def guarded(torch, shape, off, dtype=None, fill=SENTINEL):
    """a buffer of `shape` between two guards, everything `fill`; off: words its base lies behind a 16-byte boundary"""
    dtype = dtype or torch.float32
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD + off,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD + off:GUARD + off + n].view(*shape)


def unguard(buf, shape, off, what):
    """the words between the guards, the guards checked"""
    b = buf.cpu().numpy()
    n = int(np.prod(shape))
    raw = b.view(np.uint32 if b.dtype.itemsize == 4 else np.uint64)
    assert (raw[:GUARD + off] == raw[0]).all() and (raw[GUARD + off + n:] == raw[0]).all(), "guard words of %s overwritten" % what
    return b[GUARD + off:GUARD + off + n].reshape(shape)


def offset_copy(torch, a, off):
    flat = torch.zeros(a.size + off, dtype=torch.float32, device="cuda")
    flat[off:] = torch.from_numpy(a.reshape(-1)).to("cuda")
    return flat[off:].view(*a.shape)


def same_bits(got, want, what):
    for k, name in enumerate(("w1", "b1", "w2", "b2")):
        g, w = ES.bits(got[k]), ES.bits(want[k])
        ne = g != w
        assert not ne.any(), "%s: %d words of %s differ, first at %s: gpu %#x model %#x" % (
            what, int(ne.sum()), name, tuple(np.argwhere(ne)[0]), g[tuple(np.argwhere(ne)[0])], w[tuple(np.argwhere(ne)[0])])


# ------------------------------------------------------------------------------------------------------------------- shape
def fitness_cases(G, rng):
    nan, inf = np.nan, np.inf
    spread = rng.standard_normal(G)
    return {"random": spread, "ties": rng.integers(0, 3, G).astype(np.float64), "equal": np.full(G, 2.5), "nan": np.full(G, nan),
            "mixed": rng.choice(np.array([nan, -inf, inf, -0.0, 0.0, 1.5, -2.0, 1e-310]), G)}


def run_shape(torch, _lib, fit, M, S, wide, name="rem2d_es_shape"):
    G = M * S
    buf, util = guarded(torch, (G,), 0, torch.int32, -7)
    fd = torch.from_numpy(fit).to("cuda")
    e = descriptor(_lib, 4, 3, 5, M, S, 1, 1, fitness=fd, util=util)
    call(torch, _lib, name, e, wide)
    assert np.array_equal(fd.cpu().numpy().view(np.uint64), fit.view(np.uint64)), "fitness was written"
    return unguard(buf, (G,), 0, "util")


@pytest.mark.parametrize("S", [2, 6, 62, 64, 66, 130, TILE + 2])
def test_shape(gpu, S):
    """rem2d_es_shape == the model for M of 1 and 3 blocks (blocks that share a wavefront, straddle workgroups and are longer
    than the LDS tile) and five kinds of fitness; S = 66 also in the wide and fma builds"""
    torch = gpu
    from gym_rem2d_amd import _lib
    rng = np.random.default_rng([S, 77])
    for M in (1, 3):
        for name, fit in fitness_cases(M * S, rng).items():
            want = ES.shape_model(fit, S)
            assert (want.reshape(M, S).sum(axis=1) == 0).all()
            for wide in (BUILDS if S == 66 else (False,)):
                got = run_shape(torch, _lib, fit, M, S, wide)
                ne = got != want
                assert not ne.any(), "M=%d S=%d %s build=%s: %d util differ, first child %d: gpu %d model %d" % (
                    M, S, name, wide, int(ne.sum()), int(np.argmax(ne)), got[np.argmax(ne)], want[np.argmax(ne)])


# ------------------------------------------------------------------------------------------------------------------ sample
def run_sample(torch, _lib, shape, W, S, sigma, seed, gen, wide, off):
    MB, R, H = shape
    M = W[0].shape[0]
    src = [offset_copy(torch, a, off) for a in W]
    kid_shapes = [(M * S,) + a.shape[1:] for a in W]
    bufs, kids = zip(*[guarded(torch, s, off) for s in kid_shapes])
    assert all(t.data_ptr() % 16 == (4 * off) % 16 for t in src + list(kids))
    e = descriptor(_lib, MB, R, H, M, S, seed, gen, sigma=sigma, mean=src, kids=kids)
    call(torch, _lib, "rem2d_es_sample", e, wide)
    for s, a in zip(src, W):
        assert np.array_equal(s.cpu().numpy().view(np.uint32), a.view(np.uint32)), "the mean was written"
    return [unguard(b, s, off, "a child buffer") for b, s in zip(bufs, kid_shapes)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "MB%d-R%d-H%d" % s)
def test_sample(gpu, shape):
    """rem2d_es_sample == the model: M of 1, 3 x S of 2, 6, 64, 66 x sigma 0, 0.1, +inf, the means full of NaN payloads, infinities,
    denormals and signed zeros, buffer bases 16-byte aligned and 4 bytes off (MB 16, R 10, H 32 aligned is the dwordx4 path, MB 4
    the mixed one).  M = 3, S = 6 also in the wide and the fma build."""
    torch = gpu
    from gym_rem2d_amd import _lib
    rng = np.random.default_rng([shape[2], 5])
    combo = n_words = n_nan = 0
    for M in (1, 3):
        W = forge_mean(*shape, M, 1)
        for S in (2, 6, 64, 66):
            for sigma in (0.0, 0.1, float("inf")):
                combo += 1
                off = 1 if combo % 3 == 0 else 0
                seed, gen = int(rng.integers(0, 2 ** 63)) * 2 + 1, int(rng.integers(0, 2 ** 32))
                want = ES.sample_model(W, S, sigma, seed, gen)
                for wide in (BUILDS if (M, S) == (3, 6) else (False,)):
                    got = run_sample(torch, _lib, shape, W, S, sigma, seed, gen, wide, off)
                    same_bits(got, want, "M=%d S=%d sigma=%s off=%d build=%s" % (M, S, sigma, off, wide))
                if sigma == 0.0:                                        # the finite words of the mean come through as they are
                    rep = np.repeat(W[0], S, axis=0)
                    assert (want[0][np.isfinite(rep)] == rep[np.isfinite(rep)]).all()
                n_words += sum(a.size for a in want)
                n_nan += sum(int(np.isnan(a).sum()) for a in want)
    print("%s: %d child words compared per build, %d of them NaN" % (shape, n_words, n_nan))
    assert n_nan > 0


# ------------------------------------------------------------------------------------------------------------------ update
def util_cases(M, S, rng):
    """model-made util (random fitness, ties) and caller-filled: all zeros, the extremes +-(S - 1), anything"""
    G = M * S
    ext = np.empty(G, np.int32)
    ext[0::2], ext[1::2] = S - 1, -(S - 1)
    flip = ext.copy()
    flip[rng.random(G) < 0.5] *= -1                                      # pairs with d = 0 among pairs with d = +-2 (S - 1)
    return {"ranks": ES.shape_model(rng.standard_normal(G), S), "ties": ES.shape_model(rng.integers(0, 3, G).astype(np.float64), S),
            "zeros": np.zeros(G, np.int32), "extreme": ext, "flipped": flip,
            "any": rng.integers(-2 ** 31, 2 ** 31, G).astype(np.int32)}


def run_update(torch, _lib, shape, W, util, S, step, seed, gen, wide, off, pair_chunk, name="rem2d_es_update", fitness=None):
    """-> (the new mean's four arrays, util after the call)"""
    MB, R, H = shape
    M = W[0].shape[0]
    src = [offset_copy(torch, a, off) for a in W]
    bufs, new = zip(*[guarded(torch, a.shape, off) for a in W])
    ud = torch.from_numpy(np.asarray(util, np.int32).copy()).to("cuda")
    fd = None if fitness is None else torch.from_numpy(fitness).to("cuda")       # (held until the call has run)
    e = descriptor(_lib, MB, R, H, M, S, seed, gen, step=step, pair_chunk=pair_chunk, util=ud, mean=src, new=new, fitness=fd)
    need = int(_lib.lib(wide).rem2d_es_scratch_bytes(C.byref(e)))
    assert need >= 0 and need % 8 == 0
    sbuf = None
    if need:
        sbuf, scratch = guarded(torch, (need // 8,), 0, torch.int64, -99)
        e.scratch, e.scratch_bytes = scratch.data_ptr(), need
    call(torch, _lib, name, e, wide)
    if sbuf is not None:
        unguard(sbuf, (need // 8,), 0, "scratch")
    if fd is not None:
        assert np.array_equal(fd.cpu().numpy().view(np.uint64), fitness.view(np.uint64)), "fitness was written"
    for s, a in zip(src, W):
        assert np.array_equal(s.cpu().numpy().view(np.uint32), a.view(np.uint32)), "the mean was written"
    return [unguard(b, a.shape, off, "the new mean") for b, a in zip(bufs, W)], ud.cpu().numpy(), need


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "MB%d-R%d-H%d" % s)
def test_update(gpu, shape):
    """rem2d_es_update == the model: M of 1, 3 x S of 2, 6, 64, 66, model-made and caller-filled util (all zeros, the extremes,
    any int32), pair_chunk 0, 1, 2 and S / 2 -- with and without the split through scratch -- all equal to each other and to the
    model; guard words around the new mean and the scratch, the mean and util unchanged.  M = 3, S = 6 also in the wide and fma
    builds."""
    torch = gpu
    from gym_rem2d_amd import _lib
    rng = np.random.default_rng([shape[2], 6])
    combo = split = 0
    for M in (1, 3):
        W = forge_mean(*shape, M, 2)
        for S in (2, 6, 64, 66):
            cases = util_cases(M, S, rng)
            names = list(cases) if S in (6, 66) else ["ranks", "flipped"]
            for name in names:
                util = cases[name]
                combo += 1
                off = 1 if combo % 3 == 0 else 0
                seed, gen = int(rng.integers(0, 2 ** 63)) * 2 + 1, int(rng.integers(0, 2 ** 32))
                step = ES.step_for(0.05, S, 0.1) if name != "any" else f32(1e-12)
                want = ES.update_model(W, util, S, step, seed, gen)
                for wide in (BUILDS if (M, S) == (3, 6) else (False,)):
                    for chunk in sorted({0, 1, 2, S // 2}):
                        what = "M=%d S=%d util=%s off=%d chunk=%d build=%s" % (M, S, name, off, chunk, wide)
                        got, after, need = run_update(torch, _lib, shape, W, util, S, step, seed, gen, wide, off, chunk)
                        assert np.array_equal(after, util), what + ": util was written"
                        same_bits(got, want, what)
                        assert (need > 0) == (chunk != 0 and chunk < S // 2), what
                        split += need > 0
    print("%s: %d util patterns, %d calls through the split path" % (shape, combo, split))
    assert split > 0


@pytest.mark.parametrize("S", [4096, 65536])
def test_update_of_a_large_block(gpu, S):
    """One block of S children of the smallest policy (MB 1, R 0, H 1: 17 words): the sums pass 2^31 (2^40 at S = 65536 on the
    extreme pattern), which a 32-bit product or accumulator fails; the library's own split, no split and chunks of 1000 pairs give
    the model's bits"""
    torch = gpu
    from gym_rem2d_amd import _lib
    shape = (1, 0, 1)
    W = forge_mean(*shape, 1, 3, special=False)
    rng = np.random.default_rng(S)
    ext = np.empty(S, np.int32)
    ext[0::2], ext[1::2] = S - 1, -(S - 1)
    seed, gen = 0x123456789abcdef1, 9
    for name, util, step in (("extreme", ext, f32(2.0 ** -11 / S)), ("ranks", ES.shape_model(rng.standard_normal(S), S), ES.step_for(0.05, S, 0.1))):
        g = ES.weighted_sums(util, S, 14, 1, 0, seed, gen)
        assert np.abs(g).max() > 2 ** 31
        want = ES.update_model(W, util, S, step, seed, gen)
        assert (ES.bits(want[0]) != ES.bits(W[0])).mean() > 0.9
        needs = []
        for chunk in (0, S // 2, 1000):
            got, _, need = run_update(torch, _lib, shape, W, util, S, step, seed, gen, False, 0, chunk)
            same_bits(got, want, "S=%d util=%s chunk=%d" % (S, name, chunk))
            needs.append(need)
        assert needs[1] == 0 and needs[2] > 0 and needs[0] > 0            # (one block of more than 64 pairs: the library splits it)
        print("S=%d %s: max |g| = 2^%.1f, scratch of the library's choice %d bytes" % (S, name, np.log2(float(np.abs(g).max())), needs[0]))


def test_es_step_is_shape_then_update(gpu):
    """rem2d_es_step == rem2d_es_shape followed by rem2d_es_update == the model, in the three builds, without and with the split"""
    torch = gpu
    from gym_rem2d_amd import _lib
    for shape, M, S, chunk in (((4, 3, 5), 3, 66, 0), ((16, 10, 32), 2, 16, 3)):
        W = forge_mean(*shape, M, 4)
        rng = np.random.default_rng([M, S])
        fit = rng.integers(0, 9, M * S).astype(np.float64)
        fit[rng.integers(M * S)] = np.nan
        seed, gen, step = 0xfedcba9876543210, 4000000000, ES.step_for(0.05, S, 0.1)
        wutil = ES.shape_model(fit, S)
        want = ES.update_model(W, wutil, S, step, seed, gen)
        for wide in BUILDS:
            what = "%s build=%s" % (shape, wide)
            got, util, _ = run_update(torch, _lib, shape, W, np.full(M * S, -7), S, step, seed, gen, wide, 0, chunk, "rem2d_es_step", fit)
            assert np.array_equal(util, wutil), what + ": es_step's util differs from the model's"
            same_bits(got, want, what)
            two = run_shape(torch, _lib, fit, M, S, wide)
            assert np.array_equal(two, util), what
            again, _, _ = run_update(torch, _lib, shape, W, two, S, step, seed, gen, wide, 0, chunk)
            for k in range(4):
                assert np.array_equal(again[k].view(np.uint32), got[k].view(np.uint32)), what + ": shape + update != step"


# ------------------------------------------------------------------------------------------------------------------ Python
def _words(p):
    return [t.cpu().numpy().view(np.uint32) for t in (p.w1, p.b1, p.w2, p.b2)]


def _arrays(p):
    return [t.cpu().numpy() for t in (p.w1, p.b1, p.w2, p.b2)]


def test_mlp_policy_es(gpu):
    """MLPPolicy.es_sample / es_update: the model's children, util and new mean; the same call twice gives the same bits, another
    generation or seed others; util= skips the ranking; children and new mean keep activation, scale and rays"""
    torch = gpu
    from gym_rem2d_amd import policy
    M, S = 3, 16
    p = policy.MLPPolicy.random(M, 4, 5, n_rays=3, seed=3, activation="relu", scale=1.25).to("cuda")
    W = _arrays(p)
    kw = dict(seed=11, sigma=0.5, group_size=S)
    kids = p.es_sample(7, **kw)
    same_bits(_arrays(kids), ES.sample_model(W, S, 0.5, 11, 7), "es_sample")
    assert (kids.activation, kids.scale, kids.n_sets, kids.index) == ("relu", 1.25, M * S, None) and np.array_equal(kids.rays, p.rays)
    again = p.es_sample(7, **kw)
    assert all(np.array_equal(x, y) for x, y in zip(_words(kids), _words(again)))
    for other in (p.es_sample(8, **kw), p.es_sample(7, **dict(kw, seed=12)), p.es_sample(7, **dict(kw, seed=11 + 2 ** 32))):
        assert (_words(other)[0] != _words(kids)[0]).mean() > 0.9
    fit = torch.from_numpy(np.random.default_rng(1).standard_normal(M * S)).to("cuda")
    new = p.es_update(fit, 7, lr=0.05, **kw)
    wutil = ES.shape_model(fit.cpu().numpy(), S)
    want = ES.update_model(W, wutil, S, ES.step_for(0.05, S, 0.5), 11, 7)
    assert new.util.dtype == torch.int32 and np.array_equal(new.util.cpu().numpy(), wutil)
    same_bits(_arrays(new), want, "es_update")
    assert (new.activation, new.scale, new.n_sets, new.index) == ("relu", 1.25, M, None) and np.array_equal(new.rays, p.rays)
    assert all(np.array_equal(x, y.view(np.uint32)) for x, y in zip(_words(p), W)), "the mean was written"
    twice = p.es_update(fit, 7, lr=0.05, **kw)
    assert all(np.array_equal(x, y) for x, y in zip(_words(new), _words(twice))) and torch.equal(new.util, twice.util)
    for chunk in (1, 3, 8):
        assert all(np.array_equal(x, y) for x, y in zip(_words(new), _words(p.es_update(fit, 7, lr=0.05, pair_chunk=chunk, **kw))))
    for other in (p.es_update(fit, 8, lr=0.05, **kw), p.es_update(fit, 7, lr=0.05, **dict(kw, seed=12))):
        assert (_words(other)[0] != _words(new)[0]).mean() > 0.9 and torch.equal(other.util, new.util)
    mine = torch.from_numpy(np.random.default_rng(2).integers(-S, S, M * S).astype(np.int32)).to("cuda")
    c = p.es_update(None, 7, lr=0.05, util=mine, **kw)
    assert c.util is mine
    same_bits(_arrays(c), ES.update_model(W, mine.cpu().numpy(), S, ES.step_for(0.05, S, 0.5), 11, 7), "util=")
    # the children move the mean towards the better half: the update along (children - mean) weighted by util is positive
    move = (new.w1 - p.w1).double().flatten(1)
    pull = ((kids.w1.view(M, S, -1) - p.w1.view(M, 1, -1)).double() * new.util.view(M, S, 1).double()).sum(dim=1)
    assert bool(((move * pull).sum(dim=1) > 0).all())


def test_buffer_reuse(gpu):
    """out= / scratch=: three generations through one child policy, two sets of mean buffers and one scratch equal three
    generations of fresh allocations, and allocate nothing"""
    torch = gpu
    from gym_rem2d_amd import policy
    M, S, chunk = 2, 32, 4
    first = policy.MLPPolicy.random(M, 16, 32, seed=4).to("cuda")
    fits = [torch.from_numpy(np.random.default_rng(g).standard_normal(M * S)).to("cuda") for g in range(3)]
    kw = dict(seed=5, sigma=0.1, group_size=S)
    fresh_means, fresh_kids = [first], []
    for g in range(3):
        fresh_kids.append(fresh_means[-1].es_sample(g + 1, **kw))
        fresh_means.append(fresh_means[-1].es_update(fits[g], g + 1, lr=0.1, pair_chunk=chunk, **kw))
    cur = policy.MLPPolicy(first.w1.clone(), first.b1.clone(), first.w2.clone(), first.b2.clone())
    spare = policy.MLPPolicy.random(M, 16, 32, seed=9).to("cuda")
    kids = policy.MLPPolicy.random(M * S, 16, 32, seed=8).to("cuda")
    spare.util = torch.zeros(M * S, dtype=torch.int32, device="cuda")
    cur.util = torch.zeros(M * S, dtype=torch.int32, device="cuda")
    need = first.es_scratch_bytes(S, chunk)
    assert need == M * (S // 2 // chunk) * (first.weight_bytes() // 4) * 8
    scratch = torch.empty(need // 8, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    for g in range(3):
        k = cur.es_sample(g + 1, out=kids, **kw)
        new = cur.es_update(fits[g], g + 1, lr=0.1, pair_chunk=chunk, out=spare, scratch=scratch, **kw)
        assert k is kids and new is spare and torch.cuda.memory_allocated() == held, "es_sample / es_update(out=) allocated device memory"
        assert all(np.array_equal(x, y) for x, y in zip(_words(k), _words(fresh_kids[g]))), "children of generation %d" % (g + 1)
        assert all(np.array_equal(x, y) for x, y in zip(_words(new), _words(fresh_means[g + 1]))), "mean after generation %d" % (g + 1)
        assert torch.equal(new.util, fresh_means[g + 1].util)
        spare, cur = cur, new
    assert len({t.w1.data_ptr() for t in (cur, spare)}) == 2 and cur.util is not spare.util


# ------------------------------------------------------------------------------------------------------------- generations
def test_two_generations_give_the_replays_fitness(gpu, oracle):
    """evaluate.run_policy_es on 64 L-system creatures in blocks of 16 around 4 means, two generations of episodes capped at 60
    steps: each generation's fitness is the host replay's -- es_model for the weights, the oracle's closed loop for the episode -- and
    so are the means and the history rows.  The caller's mean is never written."""
    torch = gpu
    from gym_rem2d_amd import evaluate, make_terrain, policy, synthetic
    from gym_rem2d_amd.compiler import Morphology, lanes_for
    from gym_rem2d_amd.env import BatchedModular2D
    specs = [s for s in synthetic.lsystem_specs(range(120)) if s.n_bodies >= 2][:64]
    n, steps, S = len(specs), 60, 16
    M = n // S
    groups = {}
    for e, s in enumerate(specs):
        groups.setdefault(lanes_for(s.n_bodies), []).append(e)
    batches = [(Morphology.from_specs([specs[e] for e in groups[k]], k), groups[k]) for k in sorted(groups)]
    morphs, rows = [m for m, _ in batches], [np.asarray(idx) for _, idx in batches]
    terrain = make_terrain(4)
    W = list(PM.loop_weights(M, 16))
    sigma, lr, seed = 0.1, 0.5, 7
    step = ES.step_for(lr, S, sigma)
    # the host's generations
    want_fit, want_kids, want_mean = [], [], [W]
    for gen in (1, 2):
        want_kids.append(ES.sample_model(want_mean[-1], S, sigma, seed, gen))
        fit, gone = EM.episode_replay(oracle, terrain, morphs, rows, want_kids[-1], CONT, steps, PM.LOOP_BODIES)
        assert not gone.any()
        want_fit.append(fit)
        want_mean.append(ES.update_model(want_mean[-1], ES.shape_model(fit, S), S, step, seed, gen))
    assert all((f > 0).sum() >= 8 and len(set(f.tolist())) > n // 2 for f in want_fit)
    assert (want_fit[0] != want_fit[1]).any() and (ES.bits(want_mean[1][0]) != ES.bits(want_mean[2][0])).mean() > 0.5
    env = BatchedModular2D(seed=4, flags=evaluate.EVAL_FLAGS)
    seen = []
    try:
        env.reset_batches(batches, n)
        first = policy.MLPPolicy(*[torch.from_numpy(a.copy()) for a in W]).to("cuda")
        before = _words(first)
        last, fit, history = evaluate.run_policy_es(
            env, first, 2, seed=seed, sigma=sigma, lr=lr, group_size=S, max_steps=steps, chunk=30,
            on_generation=lambda g, k, f, m: seen.append((g, _arrays(k), f.clone().cpu().numpy(), _arrays(m), m.util.cpu().numpy())))
        assert [s[0] for s in seen] == [1, 2] and fit.dtype == torch.float64 and fit.device.type == "cuda"
        for (g, kids, got, mean, util), wk, wf, wm in zip(seen, want_kids, want_fit, want_mean[1:]):
            same_bits(kids, wk, "children of generation %d" % g)
            assert np.array_equal(got.view(np.uint64), wf.view(np.uint64)), "generation %d: the fitness differs from the replay's" % g
            assert np.array_equal(util, ES.shape_model(wf, S))
            same_bits(mean, wm, "mean after generation %d" % g)
        assert np.array_equal(fit.cpu().numpy().view(np.uint64), want_fit[1].view(np.uint64))
        same_bits(_arrays(last), want_mean[2], "the final mean")
        assert last.n_sets == M and last.device.type == "cuda" and env.policy.n_sets == n
        assert all(np.array_equal(x, y) for x, y in zip(_words(first), before)), "the caller's mean was written"
        assert last.w1.data_ptr() != first.w1.data_ptr()
        assert [h[0] for h in history] == [1, 2]
        for h, want in zip(history, want_fit):
            assert h[1] == want.min() and h[2] == want.max() and abs(h[3] - want.mean()) <= 1e-12 * abs(want.mean())
    finally:
        env.close()
