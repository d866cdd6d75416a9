"""Pareto ranking on a real MI355X (pytest -m gpu): rem2d_pareto_rank and rem2d_pareto_local against tests/pareto_model.py, every
comparison by bits under `==` with NaNs mapped to one pattern, every output between guard words, every input verified unchanged;
the three builds; pareto.rank / local_competition, and two generations each of evaluate.run_policy_pareto_es and run_policy_nslc
replayed by the host models from the device's own fitness and behaviour.

Shapes.  Rank: blocks below, at and above the wavefront and on both sides of the switch between the 256-thread workgroup that
packs whole blocks and the 1024-thread one (1, 2, 3, 16, 63, 64, 65, 100, 256 | 257, 1024); 1, 3 and 67 blocks, so that packed
workgroups are full, partial and many; one to four objectives.  Local competition: widths on both sides of every padded register
width, blocks below, at and above the wavefront and the 256-row tile, k from 1 to 32 (beyond the candidates where blocks are
short)."""
import ctypes as C

import numpy as np
import pytest

import es_model as ES
import evolve_model as EM
import novelty_model as NM
import pareto_model as PA
import policy_model as PM
from replay import need_gpu

pytestmark = pytest.mark.gpu

f32, f64, i32 = np.float32, np.float64, np.int32
BUILDS = (False, True, "fma")
GUARD = 16
RANK_SIZES = (1, 2, 3, 16, 63, 64, 65, 100, 256, 257, 1024)
RANK_BLOCKS = (1, 3, 67)
RANK_CONTENTS = ("normal", "ints", "equal", "chain", "antichain", "special", "huge", "none")
RANK_OUT = ("front", "crowd", "util", "n_fronts")
WIDTHS = (1, 2, 8, 31, 32)
LOCAL_SIZES = (1, 2, 63, 64, 65, 257, 1024)
KS = (1, 2, 15, 32)
DESC_CONTENTS = ("random", "dups", "grid", "special")


@pytest.fixture(scope="module")
def gpu():
    return need_gpu()


# ----------------------------------------------------------------------------------------------------------------- buffers
class Buf:
    """A device array between guard words, at an aligned or a 4-byte-offset base (float32 arrays; the others stay aligned)"""

    def __init__(self, torch, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        self.shape, self.dtype = arr.shape, arr.dtype
        self.n, self.at = arr.size, GUARD + (int(offset) if arr.dtype == f32 else 0)
        flat = np.zeros(self.n + 2 * GUARD + 1, arr.dtype)
        flat[:] = self.pattern(len(flat))
        flat[self.at:self.at + self.n] = arr.ravel()
        self.host = flat.copy()
        self.t = torch.from_numpy(flat).to("cuda")

    def pattern(self, n):
        if self.dtype == f32:
            return np.full(n, 0xFFC0DE77, np.uint32).view(f32)         # (a NaN with a payload: == on bits)
        if self.dtype == f64:
            return np.full(n, 0xFFF8C0DE000000AA, np.uint64).view(f64)
        return np.full(n, 0x5A5A5A5A, np.uint32).view(i32)

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


def call(torch, wide, name, p):
    from gym_rem2d_amd import _lib
    _lib.check(getattr(_lib.lib(wide), name)(C.byref(p), None), wide)
    torch.cuda.synchronize()


def same(got, want, what):
    for name, g, w in zip(RANK_OUT + ("local", "neighbours"), got, want):
        if g is None:
            continue
        gb, wb = (PA.bits64(g), PA.bits64(w)) if w.dtype == f64 else (g, w)
        ne = gb != wb
        assert not ne.any(), "%s: %d words of %s differ, first at %d: gpu %r model %r" % (
            what, int(ne.sum()), name, int(np.argmax(ne)), g[np.argmax(ne)], w[np.argmax(ne)])


# -------------------------------------------------------------------------------------------------------------------- rank
def make_obj(kind, M, S, K, rng):
    G = M * S
    if kind == "normal":
        return rng.standard_normal((G, K))
    if kind == "ints":                                      # heavy ties, duplicate vectors
        return rng.integers(0, 3, (G, K)).astype(f64)
    if kind == "equal":
        return np.tile(rng.standard_normal((1, K)), (G, 1))
    if kind == "chain":                                     # S fronts of one row: the deepest peel
        v = np.concatenate([rng.permutation(S) for _ in range(M)]).astype(f64)
        return np.tile(v[:, None], (1, K))
    if kind == "antichain":                                 # one front on a line (K = 1: a line is a chain)
        v = np.concatenate([rng.permutation(S) for _ in range(M)]).astype(f64)
        o = np.zeros((G, K))
        o[:, 0] = v
        if K > 1:
            o[:, 1] = -v
        return o
    if kind == "special":                                   # NaN, +-inf, +-0 among normal and tied values
        o = np.where(rng.random((G, K)) < 0.5, rng.standard_normal((G, K)), rng.integers(-1, 2, (G, K)).astype(f64))
        hit = rng.random((G, K)) < 0.1
        o[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324]), int(hit.sum()))
        return o
    if kind == "huge":                                      # hi - lo and above - below overflow: inf and NaN crowding
        o = rng.choice(np.array([-1.7e308, -1e308, -1.0, 0.0, 1.0, 1e308, 1.7e308]), (G, K))
        if K > 1:
            line = rng.random(G) < 0.5                      # half of the rows on an anti-chain, so that fronts are long
            o[line, 1] = -o[line, 0]
        return o
    assert kind == "none"                                   # block 0 has no admitted row
    o = rng.standard_normal((G, K))
    o[np.arange(S), rng.integers(0, K, S)] = rng.choice(np.array([np.nan, np.inf, -np.inf]), S)
    return o


def rank_descriptor(bufs, G, S, K, skip=None):
    from gym_rem2d_amd import _lib
    p = _lib.Pareto()
    p.n_rows, p.group_size, p.n_obj, p.reserved = G, S, K, 0
    p.obj = bufs["obj"].ptr
    for name in RANK_OUT:
        setattr(p, name, None if name == skip else bufs[name].ptr)
    return p


def rank_bufs(torch, obj, G, M):
    return dict(obj=Buf(torch, obj), front=Buf(torch, np.zeros(G, i32)), crowd=Buf(torch, np.zeros(G, f64)),
                util=Buf(torch, np.zeros(G, i32)), n_fronts=Buf(torch, np.zeros(M, i32)))


@pytest.mark.parametrize("content", RANK_CONTENTS)
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_rank(gpu, K, content):
    """rem2d_pareto_rank == pareto_model.rank_model, bit for bit, in the three builds, twice alike, with every output present and
    with each output NULL in turn"""
    torch = gpu
    ci0 = RANK_CONTENTS.index(content)
    seen = dict(nan=0, fronts=0, out=0)
    for si, S in enumerate(RANK_SIZES):
        M = RANK_BLOCKS[(si + ci0 + K) % 3]
        if S == 1024:                                       # (67 blocks of 1024 once: the host model is what takes long)
            M = 67 if (content, K) == ("normal", 2) else min(M, 3)
        G = M * S
        rng = np.random.default_rng([K, ci0, S, M])
        obj = make_obj(content, M, S, K, rng)
        want = PA.rank_model(obj, S)
        assert (want[2].reshape(M, S).sum(axis=1) == 0).all()
        seen["nan"] += int(np.isnan(want[1]).any())
        seen["fronts"] = max(seen["fronts"], int(want[3].max()))
        seen["out"] += int((want[3] == 0).any())
        what = "K %d S %d M %d %s" % (K, S, M, content)
        for wide in BUILDS:
            bufs = rank_bufs(torch, obj, G, M)
            p = rank_descriptor(bufs, G, S, K)
            call(torch, wide, "rem2d_pareto_rank", p)
            got = [bufs[name].read() for name in RANK_OUT]
            same(got, want, "%s build %s" % (what, wide))
            call(torch, wide, "rem2d_pareto_rank", p)
            again = [bufs[name].read() for name in RANK_OUT]
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, again)), what
            assert bufs["obj"].unchanged(), what
            if wide is not False:
                continue
            for skip in RANK_OUT:                           # each output NULL in turn: it is not written, the others are
                bufs = rank_bufs(torch, obj, G, M)
                call(torch, wide, "rem2d_pareto_rank", rank_descriptor(bufs, G, S, K, skip))
                assert bufs[skip].unchanged() and bufs["obj"].unchanged(), (what, skip)
                same([None if name == skip else bufs[name].read() for name in RANK_OUT], want, "%s without %s" % (what, skip))
    if content == "chain":
        assert seen["fronts"] == 1024                       # the deepest peel a block can hold
    if content == "huge" and K > 1:
        assert seen["nan"] >= 1, "no NaN crowding in the overflow cases"
    if content == "none":
        assert seen["out"] == len(RANK_SIZES)
    print("K = %d, %s: %d sizes x 3 builds; up to %d fronts, %d cases with a NaN crowd, %d with a block of no admitted row"
          % (K, content, len(RANK_SIZES), seen["fronts"], seen["nan"], seen["out"]))


def test_rank_of_blocks_one_by_one(gpu):
    """A rank over G rows equals the ranks of its blocks called one by one: nothing depends on the launch shape"""
    torch = gpu
    from gym_rem2d_amd import _lib
    for S, M, K in ((100, 5, 3), (16, 19, 2), (300, 4, 4)):
        G = M * S
        obj = make_obj("special", M, S, K, np.random.default_rng([S, M, K]))
        want = PA.rank_model(obj, S)
        whole = rank_bufs(torch, obj, G, M)
        call(torch, False, "rem2d_pareto_rank", rank_descriptor(whole, G, S, K))
        parts = rank_bufs(torch, obj, G, M)
        for b in range(M):
            p = _lib.Pareto()
            p.n_rows, p.group_size, p.n_obj, p.reserved = S, S, K, 0
            p.obj = parts["obj"].ptr + b * S * K * 8
            p.front, p.crowd, p.util, p.n_fronts = (parts["front"].ptr + b * S * 4, parts["crowd"].ptr + b * S * 8,
                                                    parts["util"].ptr + b * S * 4, parts["n_fronts"].ptr + b * 4)
            call(torch, False, "rem2d_pareto_rank", p)
        for bufs in (whole, parts):
            same([bufs[name].read() for name in RANK_OUT], want, "S %d M %d K %d" % (S, M, K))


# ------------------------------------------------------------------------------------------------------- local competition
def make_desc(kind, G, B, rng):
    if kind == "random":
        return rng.standard_normal((G, B)).astype(f32)
    if kind == "grid":                                      # a coarse integer grid: many equal d2, twins at distance 0
        return rng.integers(0, 3, (G, B)).astype(f32)
    if kind == "dups":                                      # whole rows duplicated
        return rng.standard_normal((G, B)).astype(f32)[rng.integers(0, max(1, G // 3), G)]
    d = rng.standard_normal((G, B)).astype(f32)            # special: NaN, +-inf, denormals, +-0 and words that make d2 overflow
    hit = rng.random((G, B)) < 0.08
    d[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e-45, -3e-42, 0.0, -0.0, 1e19, -1e19, 3e38], f32), int(hit.sum()))
    d[rng.random(G) < 0.1] = f32(0.0)
    return d


def make_fitness(G, rng):
    """ties and NaNs, an infinity now and then"""
    fit = rng.integers(0, 5, G).astype(f64)
    fit[rng.random(G) < 0.15] = np.nan
    fit[rng.random(G) < 0.03] = np.inf
    fit[rng.random(G) < 0.03] = -0.0
    return fit


def local_cases(B):
    """(S, M, k, content, offset): every S twice with this width; both M and every k and content with every width"""
    i = WIDTHS.index(B)
    return [(S, (1, 3)[(s + rep) % 2], KS[(s // 2 + rep + i) % 4], DESC_CONTENTS[(s + rep + 2 * i) % 4], (s + i + rep) % 2)
            for s, S in enumerate(LOCAL_SIZES) for rep in range(2)]


def local_descriptor(bufs, G, S, B, k, neighbours=True):
    from gym_rem2d_amd import _lib
    p = _lib.Pareto()
    p.n_rows, p.group_size, p.width, p.k, p.reserved = G, S, B, k, 0
    p.desc, p.fitness, p.local = bufs["desc"].ptr, bufs["fitness"].ptr, bufs["local"].ptr
    p.neighbours = bufs["neighbours"].ptr if neighbours else None
    return p


@pytest.mark.parametrize("B", WIDTHS)
def test_local(gpu, B):
    """rem2d_pareto_local == pareto_model.local_model, bit for bit, in the three builds, twice alike, with and without neighbours"""
    torch = gpu
    short = nans = ties = 0
    for S, M, k, content, offset in local_cases(B):
        rng = np.random.default_rng([B, S, M, k])
        G = M * S
        desc, fit = make_desc(content, G, B, rng), make_fitness(G, rng)
        want = PA.local_model(desc, fit, k, S)
        short += int(k > S - 1)
        nans += int(np.isnan(want[0]).any())
        ties += int((PA.bits64(PA.local_model(desc, fit, k, S, variant="high_tie")[0]) != PA.bits64(want[0])).any())
        what = "B %d S %d M %d k %d %s offset %d" % (B, S, M, k, content, offset)
        for wide in BUILDS:
            bufs = dict(desc=Buf(torch, desc, offset), fitness=Buf(torch, fit), local=Buf(torch, np.zeros(G, f64)),
                        neighbours=Buf(torch, np.zeros(G, i32)))
            p = local_descriptor(bufs, G, S, B, k)
            call(torch, wide, "rem2d_pareto_local", p)
            got = (bufs["local"].read(), bufs["neighbours"].read())
            same((None,) * 4 + got, (None,) * 4 + want, "%s build %s" % (what, wide))
            call(torch, wide, "rem2d_pareto_local", p)
            assert np.array_equal(bufs["local"].read().view(np.uint64), got[0].view(np.uint64)) and np.array_equal(bufs["neighbours"].read(), got[1])
            assert bufs["desc"].unchanged() and bufs["fitness"].unchanged(), what
            bufs["local"], bufs["neighbours"] = Buf(torch, np.zeros(G, f64)), Buf(torch, np.zeros(G, i32))
            call(torch, wide, "rem2d_pareto_local", local_descriptor(bufs, G, S, B, k, neighbours=False))
            same((None,) * 4 + (bufs["local"].read(), None), (None,) * 4 + want, "%s build %s, no neighbours" % (what, wide))
            assert bufs["neighbours"].unchanged(), what
    assert short >= 1 and ties >= 1, (short, ties)
    print("B = %d: %d cases x 3 builds, %d with k beyond the candidates, %d with NaN scores, %d in which the tie-break shows"
          % (B, len(local_cases(B)), short, nans, ties))


# ------------------------------------------------------------------------------------------------------------ Python layer
def test_python_layer(gpu):
    """pareto.rank / local_competition: the model's bits; out= is written in place and nothing else is allocated"""
    torch = gpu
    from gym_rem2d_amd import pareto
    rng = np.random.default_rng(31)
    S, M, K, B, k = 65, 3, 3, 8, 15
    G = S * M
    obj = make_obj("special", M, S, K, rng)
    want = PA.rank_model(obj, S)
    o = torch.from_numpy(obj).to("cuda")
    got = pareto.rank(o, group_size=S)
    assert isinstance(got, pareto.ParetoRank) and [t.dtype for t in got] == [torch.int32, torch.float64, torch.int32, torch.int32]
    same([t.cpu().numpy() for t in got], want, "pareto.rank")
    out = pareto.ParetoRank(*(torch.zeros_like(t) for t in got))
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    back = pareto.rank(o, group_size=S, out=out, wide="fma")
    assert all(a is b for a, b in zip(back, out)) and torch.cuda.memory_allocated() == mem
    same([t.cpu().numpy() for t in out], want, "pareto.rank(out=)")
    only = pareto.rank(o, group_size=S, out=(None, None, torch.zeros_like(got.util), None))
    assert only.front is None and only.crowd is None and only.n_fronts is None and np.array_equal(only.util.cpu().numpy(), want[2])
    one = pareto.rank(o[:, 0].contiguous(), group_size=S, wide=True)                   # a [G] tensor is one objective
    same([t.cpu().numpy() for t in one], PA.rank_model(obj[:, 0], S), "pareto.rank of [G]")
    whole = pareto.rank(o[:S].contiguous())                                            # default: one block
    same([t.cpu().numpy() for t in whole], PA.rank_model(obj[:S], S), "pareto.rank, one block")
    desc, fit = make_desc("grid", G, B, rng), make_fitness(G, rng)
    d, f = torch.from_numpy(desc).to("cuda"), torch.from_numpy(fit).to("cuda")
    wl = PA.local_model(desc, fit, k, S)[0]
    assert np.array_equal(PA.bits64(pareto.local_competition(d, f, k=k, group_size=S).cpu().numpy()), PA.bits64(wl))
    lo = torch.zeros(G, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    assert pareto.local_competition(d, f, k=k, group_size=S, out=lo, wide=True) is lo and torch.cuda.memory_allocated() == mem
    assert np.array_equal(PA.bits64(lo.cpu().numpy()), PA.bits64(wl))
    assert np.array_equal(PA.bits64(pareto.local_competition(d, f).cpu().numpy()), PA.bits64(PA.local_model(desc, fit, 15, G)[0]))


# ------------------------------------------------------------------------------------------------------------- generations
LOOP = dict(n=32, steps=60, S=16, K=4, period=15, k=5, cap=6, rate=0.3, sigma=0.1, lr=0.5, seed=7, mut=0.25, tourn=3)


def loop_env():
    """32 L-system creatures, two blocks of 16: half of the population of test_novelty_gpu's generations"""
    from gym_rem2d_amd import evaluate, synthetic
    from gym_rem2d_amd.compiler import Morphology, lanes_for
    from gym_rem2d_amd.env import BatchedModular2D
    specs = [s for s in synthetic.lsystem_specs(range(120)) if s.n_bodies >= 2][:LOOP["n"]]
    groups = {}
    for e, s in enumerate(specs):
        groups.setdefault(lanes_for(s.n_bodies), []).append(e)
    batches = [(Morphology.from_specs([specs[e] for e in groups[g]], g), groups[g]) for g in sorted(groups)]
    env = BatchedModular2D(seed=4, flags=evaluate.EVAL_FLAGS)
    env.reset_batches(batches, len(specs))
    return env


def _arrays(p):
    return [t.cpu().numpy() for t in (p.w1, p.b1, p.w2, p.b2)]


def test_two_generations_of_pareto_es(gpu):
    """evaluate.run_policy_pareto_es on 32 creatures around 2 means: the children are es_model's, and from the device's own fitness
    and behaviour the host models give the device's novelty, archive, utilities and new mean, bit for bit; the third generation
    allocates nothing"""
    torch = gpu
    from gym_rem2d_amd import evaluate, novelty, policy
    n, steps, S, K, period, k, cap, rate, sigma, lr, seed = (LOOP[q] for q in ("n", "steps", "S", "K", "period", "k", "cap", "rate", "sigma", "lr", "seed"))
    M = n // S
    env = loop_env()
    try:
        W = list(PM.loop_weights(M, 16))
        first = policy.MLPPolicy(*[torch.from_numpy(a.copy()) for a in W]).to("cuda")
        archive = novelty.NoveltyArchive(M, cap, 2 * K, device="cuda")
        seen, mem = [], []

        def keep(g, kids, f, m, b, nv, u):
            seen.append(dict(kids=_arrays(kids), fit=f.cpu().numpy(), beh=b.cpu().numpy(), nov=nv.cpu().numpy(), util=u.cpu().numpy(),
                             mean=_arrays(m), arch=archive.entries.cpu().numpy(), total=archive.total.cpu().numpy()))
            torch.cuda.synchronize()
            mem.append(torch.cuda.memory_allocated())
        last, fit, history = evaluate.run_policy_pareto_es(env, first, 3, archive, k=k, rate=rate, period=period, samples=K, seed=seed,
                                                           sigma=sigma, lr=lr, group_size=S, max_steps=steps, on_generation=keep)
        assert len(seen) == 3 and [h[0] for h in history] == [1, 2, 3] and mem[2] == mem[1] == mem[0], mem
        step = ES.step_for(lr, S, sigma)
        mean, arch, total = W, np.zeros((M, cap, 2 * K), f32), np.zeros(M, np.int64)
        differs = 0
        for gen, got in enumerate(seen, 1):
            for a, b in zip(got["kids"], ES.sample_model(mean, S, sigma, seed, gen)):
                assert np.array_equal(ES.bits(a), ES.bits(b)), "children of generation %d" % gen
            nov = NM.score_model(got["beh"], S, k, arch, total)
            arch, total, _ = NM.add_model(got["beh"], S, arch, total, gen, seed, NM.rate_threshold(rate))
            assert np.array_equal(PA.bits64(got["nov"]), PA.bits64(nov)), "generation %d: novelty" % gen
            assert np.array_equal(got["arch"].view(np.uint32), arch.view(np.uint32)) and np.array_equal(got["total"], total)
            util = PA.rank_model(np.stack([got["fit"], nov], axis=1), S)[2]
            assert np.array_equal(got["util"], util), "generation %d: util" % gen
            differs += int((util != ES.shape_model(got["fit"], S)).any())
            mean = ES.update_model(mean, util, S, step, seed, gen)
            for a, b in zip(got["mean"], mean):
                assert np.array_equal(ES.bits(a), ES.bits(b)), "mean after generation %d" % gen
        assert differs >= 1 and (seen[0]["beh"][:, 0::2].std(axis=1) > 0).sum() > n // 2          # the replay is worth comparing with
        for a, b in zip(_arrays(last), mean):
            assert np.array_equal(ES.bits(a), ES.bits(b))
        assert np.array_equal(fit.cpu().numpy().view(np.uint64), seen[2]["fit"].view(np.uint64))
    finally:
        env.close()


def test_two_generations_of_nslc(gpu):
    """evaluate.run_policy_nslc on 32 creatures in two blocks: from the device's own fitness and behaviour the host models give the
    device's novelty, local competition and utilities, and evolve_model on those utilities gives the next generation's parents and
    weights, bit for bit"""
    torch = gpu
    from gym_rem2d_amd import evaluate, novelty, policy
    n, steps, S, K, period, k, cap, rate, sigma, seed, mut, tourn = (
        LOOP[q] for q in ("n", "steps", "S", "K", "period", "k", "cap", "rate", "sigma", "seed", "mut", "tourn"))
    M = n // S
    env = loop_env()
    try:
        W = list(PM.loop_weights(n, 16))
        first = policy.MLPPolicy(*[torch.from_numpy(a.copy()) for a in W]).to("cuda")
        archive = novelty.NoveltyArchive(M, cap, 2 * K, device="cuda")
        seen = []

        def keep(g, p, f, b, nv, lc, u):
            seen.append(dict(gen=g, w=_arrays(p), parents=None if getattr(p, "parents", None) is None else p.parents.cpu().numpy(),
                             fit=f.cpu().numpy(), beh=b.cpu().numpy(), nov=nv.cpu().numpy(), loc=lc.cpu().numpy(), util=u.cpu().numpy()))
        last, fit, history = evaluate.run_policy_nslc(env, first, 2, archive, k=k, rate=rate, period=period, samples=K, seed=seed,
                                                      mut_rate=mut, sigma=sigma, tournsize=tourn, group_size=S, elite=1, max_steps=steps,
                                                      on_generation=keep)
        assert [s["gen"] for s in seen] == [0, 1, 2] and [h[0] for h in history] == [1, 2]
        arch, total = np.zeros((M, cap, 2 * K), f32), np.zeros(M, np.int64)
        weights, plain = W, 0
        for got in seen:
            gen = got["gen"]
            if gen:
                kids, hits, parent = EM.evolve_model(weights, util.astype(f64), S, tourn, 1, EM.rate_threshold(mut), sigma, seed, gen)
                assert np.array_equal(got["parents"], parent), "generation %d: parents" % gen
                for name, a, b, h in zip(("w1", "b1", "w2", "b2"), got["w"], kids, hits):
                    assert np.array_equal(EM.bits(a, h), EM.bits(b, h)), "generation %d: %s" % (gen, name)
                weights = got["w"]
            else:
                for a, b in zip(got["w"], W):
                    assert np.array_equal(ES.bits(a), ES.bits(b))
            nov = NM.score_model(got["beh"], S, k, arch, total)
            arch, total, _ = NM.add_model(got["beh"], S, arch, total, gen, seed, NM.rate_threshold(rate))
            loc = PA.local_model(got["beh"], got["fit"], k, S)[0]
            assert np.array_equal(PA.bits64(got["nov"]), PA.bits64(nov)), "generation %d: novelty" % gen
            assert np.array_equal(PA.bits64(got["loc"]), PA.bits64(loc)), "generation %d: local competition" % gen
            util = PA.rank_model(np.stack([nov, loc], axis=1), S)[2]
            assert np.array_equal(got["util"], util), "generation %d: util" % gen
            plain += int((util != ES.shape_model(got["fit"], S)).any())
        assert plain >= 1 and np.array_equal(archive.total.cpu().numpy(), total)
        for a, b in zip(_arrays(last), seen[2]["w"]):
            assert np.array_equal(ES.bits(a), ES.bits(b))
    finally:
        env.close()
