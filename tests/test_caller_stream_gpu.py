"""The caller-stream contract on a real MI355X (pytest -m gpu): every `queued` row of tests/caller_stream.py, in the three builds,
at the smallest shape of its tier's forge that still has a 16-byte (V = 4) and a 4-byte (V = 1) array and two blocks.

Two legs, the same rows and shapes:

  capture   the call alone inside ``torch.cuda.graph`` (global capture-error mode): a call that synchronises, allocates through HIP
            or touches the legacy stream makes the capture raise.  After the capture nothing has run -- every output still holds its
            sentinel --, a replay computes the reference of data set A, and after the inputs were overwritten IN PLACE with data set
            B a second replay computes the reference of B.
  gate      on a fresh stream s: a spin of GATE cycles, then ``inp.copy_(real)`` for every input, then the call.  Until the spin
            ends the inputs hold a finite decoy whose result differs from the real one in every output, so a launch that went to
            any other stream reads the decoy.  Stream order alone makes a correct library pass; the gate's length is proved once
            per session by a control that makes the call under a second stream and MUST read the decoy.

The reference of an array function is its tier's numpy model, on bits, as in the tier's own suite; of a world-taking function the
same call made plainly on the default stream on a second population brought to the identical state (and so for the geometry
self-test in the fma build, which no model states).  The ids are the queued rows of the table: a row without a case fails."""
import ctypes as C

import numpy as np
import pytest

import caller_stream as CS
import elites_model as QM
import es_model as ES
import evolve_model as EM
import novelty_model as NM
import pareto_model as PA
import policy_model as PM
import recurrent_model as RM
import snes_model as SN
import test_es_gpu as TES
import test_evolve_gpu as TEV
import test_policy_gpu as TPO

pytestmark = pytest.mark.gpu

f32 = np.float32
BUILDS = (False, True, "fma")
SHAPE = (4, 3, 5)                            # (MB, R, H): per-set lengths 175 5 20 4 -- w1 and b1 are 4-byte arrays, w2 and b2 16-byte ones
F_SENT, I_SENT = -12345.678, -7              # what a not-yet-written float / integer output word holds
GATE_MS = 20.0                               # the gate outlasts the host's queueing of copies and call by more than 20 x
KEYS = ("A", "B", "decoy")
DEVICE = "cuda:0"


@pytest.fixture(scope="module")
def gpu():
    import replay
    return replay.need_gpu()


# ---------------------------------------------------------------------------------------------------------------------- a case
class Case:
    """One row at one shape in one build: the device tensors the call reads (`inputs`, each with its three data sets resident on
    the device), the ones it writes (`outputs`, each with its sentinel), `call()` on the current stream, and `want(key)`: the
    reference's outputs for a data set, as comparable words."""

    def __init__(self, torch):
        self.torch, self.dev = torch, torch.device(DEVICE)
        self.inputs, self.outputs, self.data = [], [], {k: {} for k in KEYS}
        self.call = self.want = None
        self.norm = lambda key, got: [np.ascontiguousarray(g).reshape(-1).view(np.uint8) for g in got]
        self.derived = []                    # (name, read() -> tensor): outputs the library holds itself, read through it
        self.after_load = None               # queued on the current stream behind the inputs, before the call (not part of it)
        self.insensitive = set()             # outputs the decoy is not asked to change (stated where a case names one)

    def inp(self, name, a, b, decoy):
        """an input tensor; its data sets as host arrays in self.data[key][name]"""
        torch = self.torch
        arrs = [np.ascontiguousarray(v) for v in (a, b, decoy)]
        assert all(v.shape == arrs[0].shape and v.dtype == arrs[0].dtype for v in arrs)
        assert arrs[2].dtype.kind != "f" or np.isfinite(arrs[2]).all(), "a decoy must be finite"
        t = torch.empty(arrs[0].shape, dtype=getattr(torch, str(arrs[0].dtype)), device=self.dev)
        sets = {}
        for key, v in zip(KEYS, arrs):
            self.data[key][name] = v
            sets[key] = torch.from_numpy(v).to(self.dev)
        self.inputs.append((name, t, sets))
        return t

    def bind(self, name, t, a, b, decoy):
        """as inp(), for a tensor that exists already (a world's arena)"""
        torch = self.torch
        sets = {}
        for key, v in zip(KEYS, (a, b, decoy)):
            self.data[key][name] = np.ascontiguousarray(v)
            sets[key] = torch.from_numpy(self.data[key][name]).to(self.dev).view(t.dtype).reshape(t.shape)
        self.inputs.append((name, t, sets))
        return t

    def out(self, name, shape, dtype, sentinel):
        t = self.torch.full(tuple(shape), sentinel, dtype=dtype, device=self.dev)
        self.outputs.append((name, t, t.clone()))
        return t

    def out_existing(self, name, t, sentinel):
        """as out(), for a buffer the package owns (bool: through its bytes)"""
        t = t.view(self.torch.uint8) if t.dtype == self.torch.bool else t
        t.fill_(sentinel)
        self.outputs.append((name, t, t.clone()))
        return t

    def names(self):
        return [n for n, _, _ in self.outputs] + [n for n, _ in self.derived]

    def inout(self, name):
        """an input the call also rewrites in place: compared as an output too; its `sentinel` is the data set it holds"""
        t = [x for n, x, _ in self.inputs if n == name][0]
        self.outputs.append((name, t, None))
        return t

    def load(self, key):
        """sentinels into the outputs, then data set `key` into the inputs, on the current stream"""
        for _, t, sent in self.outputs:
            if sent is not None:
                t.copy_(sent)
        for _, t, sets in self.inputs:
            t.copy_(sets[key])
        if self.after_load is not None:
            self.after_load()

    def read(self):
        return [t.cpu().numpy() for _, t, _ in self.outputs] + [fn().cpu().numpy() for _, fn in self.derived]

    def untouched(self, key, before, what):
        """every output still holds its sentinel (an in-place one: data set `key`; a derived one: what `before` read)"""
        got = self.read()
        for (name, t, sent), g in zip(self.outputs, got):
            ref = sent if sent is not None else [s[key] for n, _, s in self.inputs if n == name][0]
            assert g.tobytes() == ref.cpu().numpy().tobytes(), "%s: `%s` was written" % (what, name)
        for name, g, b in zip(self.names(), got, before):
            assert g.tobytes() == b.tobytes(), "%s: `%s` changed" % (what, name)

    def compare(self, key, what):
        got, want = self.norm(key, self.read()), self.want(key)
        assert len(got) == len(want) == len(self.names())
        for name, g, w in zip(self.names(), got, want):
            g, w = np.asarray(g).reshape(-1), np.asarray(w).reshape(-1)
            assert g.shape == w.shape and g.dtype == w.dtype, "%s: `%s` %s %s against %s %s" % (what, name, g.dtype, g.shape, w.dtype, w.shape)
            ne = g != w
            assert not ne.any(), "%s: %d of %d words of `%s` differ from the reference of data set %s, first at %d: gpu %r reference %r" % (
                what, int(ne.sum()), ne.size, name, key, int(np.argmax(ne)), g[np.argmax(ne)], w[np.argmax(ne)])

    def reads_decoy(self):
        """the decoy's result, as the reference states it, differs from the real one in at least one word of every output"""
        for name, a, d in zip(self.names(), self.want("A"), self.want("decoy")):
            assert name in self.insensitive or (np.asarray(a).reshape(-1) != np.asarray(d).reshape(-1)).any(), \
                "the decoy leaves `%s` as the real data does" % name


def _against_plain_call(torch, c, ref):
    """c's reference becomes what `ref` -- the same case built a second time, on tensors of its own -- leaves when its call is made
    plainly: after a drain, on the default stream, drained again"""
    def want(key):
        torch.cuda.synchronize()
        ref.load(key)
        torch.cuda.synchronize()
        ref.call()
        torch.cuda.synchronize()
        return ref.norm(key, ref.read())
    c.want = want
    c.keep_ref = ref


def _sets(make):
    """(A, B, decoy) of one input from make(seed, finite)"""
    return make(1, False), make(2, False), make(3, True)


def _finite(a, rng):
    """`a` with every word that is not an ordinary number redrawn (a decoy is finite)"""
    a = np.array(a)
    if a.dtype.kind == "f":
        bad = ~np.isfinite(a)
        a[bad] = rng.standard_normal(int(bad.sum())).astype(a.dtype)
    return a


def _lib_call(torch, name, desc, wide):
    from gym_rem2d_amd import _lib
    _lib.check(getattr(_lib.lib(wide), name)(C.byref(desc), C.c_void_p(torch.cuda.current_stream().cuda_stream)), wide)


# ------------------------------------------------------------------------------------------------------- policies: forward passes
N_ROWS = 65                                  # two wavefronts' worth of rows, the second with one row


def _forward_inputs(R_all, seed, finite):
    MB, _, H = SHAPE
    x, W, _, _ = TPO.forge(MB, R_all, H, N_ROWS, "per_row", seed)
    arrs = [x] + list(W)
    if finite:
        rng = np.random.default_rng([seed, 99])
        arrs = [_finite(a, rng) for a in arrs]
    return arrs


def case_policy_forward(torch, wide):
    from gym_rem2d_amd import policy
    MB, R, H = SHAPE
    c = Case(torch)
    sets = [_forward_inputs(R, s, s == 3) for s in (1, 2, 3)]
    wd = TPO.M.width(MB)
    obs, frac = c.inp("obs", *(s[0][:, :wd] for s in sets)), c.inp("frac", *(s[0][:, wd:] for s in sets))
    w = [c.inp(n, *(s[1 + i] for s in sets)) for i, n in enumerate(NAMES4)]
    pol = policy.MLPPolicy(*w, rays=np.zeros((R, 2)) + 1.0)
    out = (c.out("targets", (N_ROWS, MB), torch.float64, F_SENT), c.out("valid", (N_ROWS, MB), torch.uint8, 0xA5))
    c.call = lambda: pol.forward(obs, frac, out=out, wide=wide)

    def want(key):
        d = c.data[key]
        tg, v = PM.forward_model(np.concatenate([d["obs"], d["frac"]], axis=1), d["w1"], d["b1"], d["w2"], d["b2"])
        return [PM.bits(tg), v.astype(np.uint8)]
    c.want = want
    c.norm = lambda key, got: [PM.bits(got[0]), got[1]]
    return c


CONTEXT = 2


def case_recurrent_forward(torch, wide):
    from gym_rem2d_amd import policy
    MB, R, H = SHAPE
    c = Case(torch)
    sets = [_forward_inputs(R + CONTEXT, s, s == 3) for s in (1, 2, 3)]
    wd = TPO.M.width(MB)
    obs = c.inp("obs", *(s[0][:, :wd] for s in sets))
    frac = c.inp("frac", *(s[0][:, wd:wd + R] for s in sets))
    mem = c.inp("memory", *(s[0][:, wd + R:] for s in sets))
    w = [c.inp(n, *(s[1 + i] for s in sets)) for i, n in enumerate(("w1", "b1", "w2", "b2"))]
    pol = policy.RecurrentPolicy(*w, CONTEXT, rays=np.zeros((R, 2)) + 1.0)
    out = (c.out("targets", (N_ROWS, MB), torch.float64, F_SENT), c.out("valid", (N_ROWS, MB), torch.uint8, 0xA5))
    c.inout("memory")
    c.call = lambda: pol.forward(obs, frac, mem, out=out, wide=wide)

    def want(key):
        d = c.data[key]
        tg, v, new = RM.forward_model(np.concatenate([d["obs"], d["frac"]], axis=1), d["memory"], d["w1"], d["b1"], d["w2"], d["b2"])
        return [PM.bits(tg), v.astype(np.uint8), RM.mem_bits(new)]
    c.want = want
    c.norm = lambda key, got: [PM.bits(got[0]), got[1], RM.mem_bits(got[2])]
    return c


# --------------------------------------------------------------------------------------------------- evolve: select, vary, evolve
EV_G, EV_S, EV_T, EV_ELITE = 10, 5, 3, 1     # two blocks of five sets
EV_RATE, EV_SIGMA, EV_SEED, EV_GEN = 0.25, 0.25, 0x1234567887654321, 7     # (0.25: exact as binary32 and as a 32-bit threshold)
NAMES4 = ("w1", "b1", "w2", "b2")


def _weights(forge, n_sets, seed, finite):
    W = forge(*SHAPE, n_sets, seed)
    return [_finite(a, np.random.default_rng([seed, 98])) for a in W] if finite else W


def _fitness(n, seed, finite):
    rng = np.random.default_rng([n, seed, 97])
    f = rng.standard_normal(n)
    if not finite:
        f[rng.integers(n)] = np.nan
        f[rng.integers(n)] = f[rng.integers(n)]          # a tie
    return f


def case_policy_select(torch, wide):
    from gym_rem2d_amd import _lib
    c = Case(torch)
    fit = c.inp("fitness", *_sets(lambda s, fin: _fitness(EV_G, s, fin)))
    parent = c.out("parent", (EV_G,), torch.int32, I_SENT)
    e = TEV.descriptor(_lib, *SHAPE, EV_G, EV_S, EV_T, EV_ELITE, 0, 0.0, EV_SEED, EV_GEN, fitness=fit, parent=parent)
    c.call = lambda: _lib_call(torch, "rem2d_policy_select", e, wide)
    c.want = lambda key: [EM.select_model(c.data[key]["fitness"], EV_S, EV_T, EV_ELITE, EV_SEED, EV_GEN).astype(np.int32)]
    c.norm = lambda key, got: got
    return c


def _evolve_case(torch, wide, vary):
    from gym_rem2d_amd import policy
    MB, R, H = SHAPE
    c = Case(torch)
    sets = [_weights(TEV.forge_weights, EV_G, s, s == 3) for s in (1, 2, 3)]
    w = [c.inp(n, *(s[i] for s in sets)) for i, n in enumerate(NAMES4)]
    fit = c.inp("fitness", *_sets(lambda s, fin: _fitness(EV_G, s, fin)))
    rays = np.zeros((R, 2)) + 1.0
    pol = policy.MLPPolicy(*w, rays=rays)
    kids = [c.out("child_" + n, t.shape, torch.float32, F_SENT) for n, t in zip(NAMES4, w)]
    child = policy.MLPPolicy(*kids, rays=rays)
    thr = EM.rate_threshold(EV_RATE)
    if vary:       # the caller's parents: every set of the other block, one that names no set (its child keeps the sentinel)
        def parents(seed, fin):
            p = np.random.default_rng([seed, 96]).integers(0, EV_G, EV_G).astype(np.int32)
            p[seed] = -1
            return p
        pd = c.inp("parent", *_sets(parents))
        c.call = lambda: pol.evolve(fit, EV_GEN, EV_SEED, EV_RATE, EV_SIGMA, EV_T, EV_S, EV_ELITE, parents=pd, out=child, wide=wide)
    else:
        child.parents = c.out("parent", (EV_G,), torch.int32, I_SENT)
        c.call = lambda: pol.evolve(fit, EV_GEN, EV_SEED, EV_RATE, EV_SIGMA, EV_T, EV_S, EV_ELITE, out=child, wide=wide)
    memo = {}

    def model(key):
        if key not in memo:
            d = c.data[key]
            W = [d[n] for n in NAMES4]
            if vary:
                before = [np.full(a.shape, F_SENT, f32) for a in W]
                k, h, _ = EM.vary_model(W, d["parent"], EV_S, EV_ELITE, thr, EV_SIGMA, EV_SEED, EV_GEN, before=before)
                memo[key] = (k, h, None)
            else:
                memo[key] = EM.evolve_model(W, d["fitness"], EV_S, EV_T, EV_ELITE, thr, EV_SIGMA, EV_SEED, EV_GEN)
        return memo[key]

    def want(key):
        k, h, p = model(key)
        return [EM.bits(a, hit) for a, hit in zip(k, h)] + ([] if vary else [np.asarray(p, np.int32)])
    c.want = want
    c.norm = lambda key, got: [EM.bits(a, hit) for a, hit in zip(got[:4], model(key)[1])] + list(got[4:])
    return c


def case_policy_vary(torch, wide):
    return _evolve_case(torch, wide, True)


def case_policy_evolve(torch, wide):
    return _evolve_case(torch, wide, False)


# ------------------------------------------------------------------------------------------------------- the evolution strategy
ES_M, ES_S, ES_SIGMA, ES_LR, ES_SEED, ES_GEN = 2, 6, 0.25, 0.5, 0x0fedcba987654321, 11     # two means of six children


def case_es_sample(torch, wide):
    from gym_rem2d_amd import policy
    MB, R, H = SHAPE
    c = Case(torch)
    sets = [_weights(TES.forge_mean, ES_M, s, s == 3) for s in (1, 2, 3)]
    w = [c.inp(n, *(s[i] for s in sets)) for i, n in enumerate(NAMES4)]
    rays = np.zeros((R, 2)) + 1.0
    pol = policy.MLPPolicy(*w, rays=rays)
    kids = [c.out("child_" + n, (ES_M * ES_S,) + tuple(t.shape[1:]), torch.float32, F_SENT) for n, t in zip(NAMES4, w)]
    child = policy.MLPPolicy(*kids, rays=rays)
    c.call = lambda: pol.es_sample(ES_GEN, ES_SEED, ES_SIGMA, ES_S, out=child, wide=wide)
    c.want = lambda key: [ES.bits(a) for a in ES.sample_model([c.data[key][n] for n in NAMES4], ES_S, ES_SIGMA, ES_SEED, ES_GEN)]
    c.norm = lambda key, got: [ES.bits(a) for a in got]
    return c


def case_es_shape(torch, wide):
    from gym_rem2d_amd import _lib
    c = Case(torch)
    fit = c.inp("fitness", *_sets(lambda s, fin: _fitness(ES_M * ES_S, s, fin)))
    util = c.out("util", (ES_M * ES_S,), torch.int32, I_SENT)
    e = TES.descriptor(_lib, *SHAPE, ES_M, ES_S, 1, 1, fitness=fit, util=util)
    c.call = lambda: _lib_call(torch, "rem2d_es_shape", e, wide)
    c.want = lambda key: [ES.shape_model(c.data[key]["fitness"], ES_S)]
    c.norm = lambda key, got: got
    return c


def _es_update_case(torch, wide, step):
    from gym_rem2d_amd import policy
    MB, R, H = SHAPE
    G = ES_M * ES_S
    c = Case(torch)
    sets = [_weights(TES.forge_mean, ES_M, s, s == 3) for s in (1, 2, 3)]
    w = [c.inp(n, *(s[i] for s in sets)) for i, n in enumerate(NAMES4)]
    rays = np.zeros((R, 2)) + 1.0
    pol = policy.MLPPolicy(*w, rays=rays)
    new = policy.MLPPolicy(*[c.out("new_" + n, t.shape, torch.float32, F_SENT) for n, t in zip(NAMES4, w)], rays=rays)
    need = pol.es_scratch_bytes(ES_S, 0, wide)
    scratch = torch.zeros(max(1, need // 8), dtype=torch.int64, device=c.dev) if need else None
    if step:
        fit = c.inp("fitness", *_sets(lambda s, fin: _fitness(G, s, fin)))
        new.util = c.out("util", (G,), torch.int32, I_SENT)
        c.call = lambda: pol.es_update(fit, ES_GEN, ES_SEED, ES_SIGMA, ES_LR, ES_S, out=new, scratch=scratch, wide=wide)
        util_of = lambda key: ES.shape_model(c.data[key]["fitness"], ES_S)
    else:
        ut = c.inp("util", *_sets(lambda s, fin: ES.shape_model(_fitness(G, s + 10, fin), ES_S)))
        c.call = lambda: pol.es_update(None, ES_GEN, ES_SEED, ES_SIGMA, ES_LR, ES_S, out=new, scratch=scratch, util=ut, wide=wide)
        util_of = lambda key: c.data[key]["util"]

    def want(key):
        u = util_of(key)
        m = ES.update_model([c.data[key][n] for n in NAMES4], u, ES_S, ES.step_for(ES_LR, ES_S, ES_SIGMA), ES_SEED, ES_GEN)
        return [ES.bits(a) for a in m] + ([np.asarray(u, np.int32)] if step else [])
    c.want = want
    c.norm = lambda key, got: [ES.bits(a) for a in got[:4]] + list(got[4:])
    return c


def case_es_update(torch, wide):
    return _es_update_case(torch, wide, False)


def case_es_step(torch, wide):
    return _es_update_case(torch, wide, True)


# ---------------------------------------------------------------------------------------------------- the adaptive strategy
def _snes_case(torch, wide, which):
    """which: "sample", "update" (the caller's util) or "step" (fitness in, util out), through policy.SeparableES on the object's own
    buffers; update and step with Adam, so that all four state arrays are read and written, and with pair_chunk 1, the split through
    scratch: two or three launches.  SeparableES.update swaps the object's current and spare buffers when it returns -- host
    bookkeeping, no device work --, so the case puts them back before every call: each call, and each replay, is the object's
    second update from the same buffers."""
    from gym_rem2d_amd import policy
    import test_snes_gpu as TSN
    M, S, G = ES_M, ES_S, ES_M * ES_S
    c = Case(torch)

    def state(seed, fin):
        st = [TES.forge_mean(*SHAPE, M, seed)] + list(TSN.forge_state(*SHAPE, M, seed))
        rng = np.random.default_rng([seed, 95])
        return [[_finite(a, rng) for a in arrs] for arrs in st] if fin else st
    sts = [state(s, s == 3) for s in (1, 2, 3)]
    groups = ("mean", "sigma") + (("m1", "m2") if which != "sample" else ())
    rays = np.zeros((SHAPE[1], 2)) + 1.0
    zero = policy.MLPPolicy(*[torch.zeros(a.shape, dtype=torch.float32, device=c.dev) for a in sts[0][0]], rays=rays)
    # (sigma 0.1, lr 0.05, lr_sigma 4: the defaults of SeparableES and of snes_model.scalars alike)
    es = policy.SeparableES(zero, S, adam=None if which == "sample" else TSN.ADAM3, sigma_bounds=TSN.BOUNDS)
    four = lambda p: [p.w1, p.b1, p.w2, p.b2]
    own = {"mean": four(es.mean), "sigma": es.sigma, "m1": es.m1, "m2": es.m2}
    spare = {"mean": four(es._spare_mean), "sigma": es._spare_sigma, "m1": es._spare_m1, "m2": es._spare_m2}
    for gi, g in enumerate(groups):
        for i, n in enumerate(NAMES4):
            c.bind("%s_%s" % (g, n), own[g][i], *(st[gi][i] for st in sts))
    if which == "sample":
        kids = [c.out("child_" + n, (G,) + tuple(x.shape[1:]), torch.float32, F_SENT) for n, x in zip(NAMES4, own["mean"])]
        child = policy.MLPPolicy(*kids, rays=rays)
        c.call = lambda: es.sample(ES_GEN, ES_SEED, out=child, wide=wide)
        c.want = lambda key: [ES.bits(a) for a in SN.sample_model([c.data[key]["mean_" + n] for n in NAMES4],
                                                                  [c.data[key]["sigma_" + n] for n in NAMES4], S, ES_SEED, ES_GEN)]
        c.norm = lambda key, got: [ES.bits(a) for a in got]
        return c
    flags = SN.ADAM
    cc = SN.scalars(S, adam=TSN.ADAM3, t=2, sigma_bounds=TSN.BOUNDS)
    assert es.flags == flags and all(f32(cc[k]) == f32(v) for k, v in es.scalars(2).items())
    for g in groups:
        for i, n in enumerate(NAMES4):
            c.out_existing("new_%s_%s" % (g, n), spare[g][i], F_SENT)
    before = (es.mean, es._spare_mean, es.sigma, es._spare_sigma, es.m1, es._spare_m1, es.m2, es._spare_m2)

    def rewind():
        (es.mean, es._spare_mean, es.sigma, es._spare_sigma, es.m1, es._spare_m1, es.m2, es._spare_m2), es.t = before, 1
    need = es.scratch_bytes(1, wide)
    assert need > 0, "pair_chunk 1 of %d pairs goes through scratch" % (S // 2)
    scratch = torch.zeros(need // 8, dtype=torch.int64, device=c.dev)
    if which == "step":
        fit = c.inp("fitness", *_sets(lambda s, fin: _fitness(G, s, fin)))
        util = c.out("util", (G,), torch.int32, I_SENT)
        es._util = [torch.empty_like(util), util]             # (the object's two util buffers; its second update writes the second)
        util_of = lambda key: ES.shape_model(c.data[key]["fitness"], S)

        def call():
            rewind()
            es.update(fit, ES_GEN, ES_SEED, scratch=scratch, pair_chunk=1, wide=wide)
    else:
        ut = c.inp("util", *_sets(lambda s, fin: ES.shape_model(_fitness(G, s + 10, fin), S)))
        util_of = lambda key: c.data[key]["util"]

        def call():
            rewind()
            es.update(None, ES_GEN, ES_SEED, util=ut, scratch=scratch, pair_chunk=1, wide=wide)
    c.call = call

    def want(key):
        d, u = c.data[key], util_of(key)
        st = SN.update_model(*[[d["%s_%s" % (g, n)] for n in NAMES4] for g in groups], u, S, cc, flags, ES_SEED, ES_GEN)
        return [ES.bits(a) for arrs in st for a in arrs] + ([np.asarray(u, np.int32)] if which == "step" else [])
    c.want = want
    c.norm = lambda key, got: [ES.bits(a) for a in got[:16]] + list(got[16:])
    return c


# ------------------------------------------------------------------------------------------------------------- novelty, Pareto
NV_B, NV_S, NV_M, NV_K, NV_CAP, NV_RATE, NV_GEN, NV_SEED = 2, 65, 2, 3, 5, 0.5, 4, (1 << 40) + 9     # two blocks of 65 rows


def _novelty_case(torch, wide, which):
    from gym_rem2d_amd import novelty
    import test_novelty_gpu as TNV
    G = NV_M * NV_S
    c = Case(torch)
    arch = novelty.NoveltyArchive(NV_M, NV_CAP, NV_B, device=c.dev)
    rngs = [np.random.default_rng([s, 94]) for s in (1, 2, 3)]
    desc = c.inp("desc", *(TNV.make_desc("random", G, NV_B, r) for r in rngs))
    c.bind("archive", arch.entries, *(r.standard_normal((NV_M, NV_CAP, NV_B)).astype(f32) for r in rngs))
    c.bind("total", arch.total, *(TNV.totals_for(NV_CAP, NV_M, w) for w in (2, 4, 1)))          # [4, 5], [17, 0], [1, 4]
    thr = NM.rate_threshold(NV_RATE)
    if which != "add":
        out = c.out("novelty", (G,), torch.float64, F_SENT)
    if which != "score":
        c.inout("archive")
        c.inout("total")
    c.call = {"score": lambda: arch.score(desc, NV_K, NV_S, out=out, wide=wide),
              "add": lambda: arch.add(desc, NV_GEN, NV_SEED, NV_RATE, group_size=NV_S, wide=wide),
              "step": lambda: arch.step(desc, NV_GEN, NV_K, NV_SEED, NV_RATE, group_size=NV_S, out=out, wide=wide)}[which]

    def want(key):
        d = c.data[key]
        res = []
        if which != "add":
            res.append(NM.bits64(NM.score_model(d["desc"], NV_S, NV_K, d["archive"], d["total"])))
        if which != "score":
            wa, wt, took = NM.add_model(d["desc"], NV_S, d["archive"], d["total"], NV_GEN, NV_SEED, thr)
            assert 0 < took.sum() < G
            res += [wa.view(np.uint32), np.asarray(wt, np.int64)]
        return res
    c.want = want
    c.norm = lambda key, got: ([NM.bits64(got[0])] if which != "add" else []) + [g.view(np.uint32) if g.dtype == f32 else g
                                                                              for g in got[0 if which == "add" else 1:]]
    return c


PA_S, PA_M, PA_K, PA_B, PA_NEAR = 65, 2, 3, 2, 3


def case_pareto_rank(torch, wide):
    from gym_rem2d_amd import pareto
    import test_pareto_gpu as TPA
    G = PA_M * PA_S
    c = Case(torch)
    rngs = [np.random.default_rng([s, 93]) for s in (1, 2, 3)]
    obj = c.inp("obj", *(TPA.make_obj(kind, PA_M, PA_S, PA_K, r) for kind, r in zip(("special", "ints", "normal"), rngs)))
    out = (c.out("front", (G,), torch.int32, I_SENT), c.out("crowd", (G,), torch.float64, F_SENT), c.out("util", (G,), torch.int32, I_SENT),
           c.out("n_fronts", (PA_M,), torch.int32, I_SENT))
    c.call = lambda: pareto.rank(obj, PA_S, out=out, wide=wide)

    def want(key):
        front, crowd, util, n_fronts = PA.rank_model(c.data[key]["obj"], PA_S)
        return [np.asarray(front, np.int32), PA.bits64(crowd), np.asarray(util, np.int32), np.asarray(n_fronts, np.int32)]
    c.want = want
    c.norm = lambda key, got: [got[0], PA.bits64(got[1]), got[2], got[3]]
    return c


def case_pareto_local(torch, wide):
    from gym_rem2d_amd import pareto
    import test_pareto_gpu as TPA
    G = PA_M * PA_S
    c = Case(torch)
    rngs = [np.random.default_rng([s, 92]) for s in (1, 2, 3)]
    desc = c.inp("desc", *(TPA.make_desc(kind, G, PA_B, r) for kind, r in zip(("special", "grid", "random"), rngs)))
    fit = c.inp("fitness", TPA.make_fitness(G, rngs[0]), TPA.make_fitness(G, rngs[1]), rngs[2].integers(0, 5, G).astype(np.float64))
    out = c.out("local", (G,), torch.float64, F_SENT)
    c.call = lambda: pareto.local_competition(desc, fit, PA_NEAR, PA_S, out=out, wide=wide)
    c.want = lambda key: [PA.bits64(PA.local_model(c.data[key]["desc"], c.data[key]["fitness"], PA_NEAR, PA_S)[0])]
    c.norm = lambda key, got: [PA.bits64(got[0])]
    return c


# -------------------------------------------------------------------------------------------------------------------- elites
EL_B, EL_BINS, EL_M, EL_S, EL_S2 = 2, [2, 2], 2, 5, 6           # two blocks of four cells; five rows in, six children out, per block
EL_RATE, EL_SIGMA, EL_GEN, EL_SEED = 0.25, 0.25, 13, (7 << 33) + 1


def _elites_case(torch, wide, which):
    """through elites.EliteGrid, on the grid's own tensors (the cell map is test_elites_gpu's, which the model and EliteGrid both
    build from the same (word, lo, hi, bins))"""
    from gym_rem2d_amd import elites, policy
    import test_elites_gpu as TEL
    D = 8 + 6 * SHAPE[0] + SHAPE[1]
    shapes = ((D, SHAPE[2]), (SHAPE[2],), (SHAPE[2], SHAPE[0]), (SHAPE[0],))
    M, S, G = EL_M, EL_S, EL_M * EL_S
    c = Case(torch)
    cmap, dims = TEL.make_map(EL_B, EL_BINS, np.random.default_rng(91))
    C_ = cmap.n_cells
    grids, pops = [], []
    for s, kind in zip((1, 2, 3), ("partly", "partly", "full")):
        rng = np.random.default_rng([s, 90])
        g = TEL.make_grid(kind, M, C_, EL_B, shapes, rng)
        desc, fitness = TEL.make_rows("random", cmap, dims, M, S, EL_B, rng)
        weights = [rng.standard_normal((G,) + sh).astype(f32) for sh in shapes]
        if s == 3:
            g.fitness, fitness = _finite(g.fitness, rng), _finite(fitness, rng)
        else:
            weights[0][rng.random(weights[0].shape) < 0.01] = f32(np.nan)
        grids.append(g)
        pops.append((desc, fitness, weights))
    n = M * EL_S2
    thr = EM.rate_threshold(EL_RATE)
    rays = np.zeros((SHAPE[1], 2)) + 1.0
    like = policy.MLPPolicy(*[torch.zeros((1,) + sh, dtype=torch.float32, device=c.dev) for sh in shapes], rays=rays)
    grid = elites.EliteGrid(M, dims, EL_B, like=like, device=c.dev)
    assert np.array_equal(np.array(grid.inv, f32), np.array(cmap.inv, f32)) and grid.n_cells == C_ and elites.rate_threshold(EL_RATE) == thr
    c.bind("count", grid.count, *(g.count for g in grids))
    if which != "sample":
        for k, name in enumerate(NAMES4):
            c.bind("elite_" + name, getattr(grid, name), *(g.weights[k] for g in grids))
    if which == "insert":
        c.bind("elite_fitness", grid.fitness, *(g.fitness for g in grids))
        c.bind("elite_desc", grid.desc, *(g.desc for g in grids))
        desc = c.inp("desc", *(p[0] for p in pops))
        fit = c.inp("fitness", *(p[1] for p in pops))
        pop = policy.MLPPolicy(*[c.inp(name, *(p[2][k] for p in pops)) for k, name in enumerate(NAMES4)], rays=rays)
        grid.cell = c.out("cell", (G,), torch.int32, I_SENT)      # (insert() makes it at first use; here it is there already)
        c.out_existing("winner", grid.winner, I_SENT)
        for name in ("elite_fitness", "elite_desc", "count") + tuple("elite_" + x for x in NAMES4):
            c.inout(name)
        c.call = lambda: grid.insert(pop, fit, desc, group_size=S, wide=wide)
    else:
        parent = c.out("parent", (n,), torch.int32, I_SENT)
        c.out_existing("n_filled", grid.filled, I_SENT)
        if which == "sample":
            c.call = lambda: grid.sample(EL_GEN, EL_SEED, n, out=parent, wide=wide)
        else:
            child = policy.MLPPolicy(*[c.out("child_" + name, (n,) + shapes[k], torch.float32, F_SENT) for k, name in enumerate(NAMES4)],
                                     rays=rays)
            child.parents = parent
            c.call = lambda: grid.emit(EL_GEN, EL_SEED, EL_RATE, EL_SIGMA, n, out=child, wide=wide)
    memo = {}

    def model(key):
        if key not in memo:
            d = c.data[key]
            g = QM.Grid(M, C_, EL_B, shapes)
            g.count[:] = d["count"]
            if which == "insert":
                g.fitness[:], g.desc[:] = d["elite_fitness"], d["elite_desc"]
            if which != "sample":
                for k, name in enumerate(NAMES4):
                    g.weights[k].view(np.uint32)[:] = d["elite_" + name].view(np.uint32)
            if which == "insert":
                memo[key] = QM.insert_model(cmap, g, [d[x] for x in NAMES4], d["fitness"], d["desc"], S)
            elif which == "sample":
                memo[key] = QM.sample_model(g.count, n, EL_SEED, EL_GEN)
            else:
                memo[key] = QM.emit_model(g, n, thr, EL_SIGMA, EL_SEED, EL_GEN, before=[np.full((n,) + sh, F_SENT, f32) for sh in shapes])
        return memo[key]

    def want(key):
        if which == "insert":
            g, cell, winner = model(key)
            return [np.asarray(cell, np.int32), np.asarray(winner, np.int32), TEL.bits(g.fitness), TEL.bits(g.desc), np.asarray(g.count, np.int32)] \
                + [TEL.bits(w) for w in g.weights]
        if which == "sample":
            n_filled, parent = model(key)
            return [np.asarray(parent, np.int32), np.asarray(n_filled, np.int32)]
        kids, hits, parent, n_filled = model(key)
        return [np.asarray(parent, np.int32), np.asarray(n_filled, np.int32)] + [EM.bits(a, h) for a, h in zip(kids, hits)]
    c.want = want

    def norm(key, got):
        if which == "insert":
            return got[:2] + [TEL.bits(got[2]), TEL.bits(got[3]), got[4]] + [TEL.bits(w) for w in got[5:]]
        if which == "sample":
            return got
        return got[:2] + [EM.bits(a, h) for a, h in zip(got[2:], model(key)[1])]
    c.norm = norm
    return c


# --------------------------------------------------------------------------------------------------- the others (ctypes: no wrapper)
DV_N = 40


def case_tree_diversity(torch, wide):
    from gym_rem2d_amd import _lib
    from gym_rem2d_amd.diversity import MAX_NODES, pack_positions
    from oracle import diversity_oracle as D
    c = Case(torch)
    grid = [(float(x), float(y)) for x in range(-3, 4) for y in range(-3, 4)]
    pops = []
    for s in (1, 2, 3):
        rng = np.random.RandomState(s)
        pops.append([[grid[i] for i in rng.randint(0, len(grid), size=int(rng.randint(0, MAX_NODES + 1)))] for _ in range(DV_N)])
    packed = [pack_positions(p) for p in pops]
    pos = c.inp("pos", *(np.asarray(p[0], np.float64) for p in packed))
    cnt = c.inp("count", *(np.asarray(p[1], np.int32) for p in packed))
    out = c.out("out", (DV_N,), torch.int64, I_SENT)
    L = _lib.lib(wide)
    c.call = lambda: _lib.check(L.rem2d_tree_diversity(pos.data_ptr(), cnt.data_ptr(), DV_N, MAX_NODES, out.data_ptr(), 0,
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)), wide)
    c.want = lambda key: [np.asarray(D.tree_edit_distance(pops[KEYS.index(key)]), np.int64)]
    c.norm = lambda key, got: got
    return c


SC_N = 300


def case_selftest_scalar(torch, wide):
    """ordinary numbers (lo <= hi, no zero, no NaN): there the device's one-instruction forms and the oracle's comparisons give the same
    bits (tests/test_parity_gpu.py::test_scalar_helpers_special_values says where else they may not)"""
    from gym_rem2d_amd import _lib
    from oracle import oracle as O
    O.build()
    c = Case(torch)

    def draw(seed, k):
        rng = np.random.default_rng([seed, k, 89])
        return (rng.standard_normal(SC_N) * 10 ** rng.uniform(-3, 3, SC_N)).astype(f32)
    a = c.inp("a", *(draw(s, 0) for s in (1, 2, 3)))
    b = c.inp("b", *(draw(s, 1) for s in (1, 2, 3)))
    cc = c.inp("c", *(np.maximum(draw(s, 1), draw(s, 2)) for s in (1, 2, 3)))
    out = c.out("out", (5, SC_N), torch.float32, F_SENT)
    L = _lib.lib(wide)
    c.call = lambda: _lib.check(L.rem2d_selftest_scalar(a.data_ptr(), b.data_ptr(), cc.data_ptr(), SC_N, out.data_ptr(), 0,
                                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), wide)

    def want(key):
        d = c.data[key]
        sc = np.array([O.sincosf(float(v)) for v in d["a"]], f32).T
        return [np.concatenate([O.kat_scalar(d["a"], d["b"], d["c"]), sc]).astype(f32).view(np.uint32)]
    c.want = want
    c.norm = lambda key, got: [got[0].view(np.uint32)]
    return c


GE_N = 64


def case_selftest_geometry(torch, wide, plain=False):
    """gjk_distance on three runs of tests/geometry_forge.py's table, every output word == the oracle's, as tests/test_geometry_gpu.py
    compares it (floats with ==; -0 == +0).  librem2d_fma.so is the labelled tolerance build for engine arithmetic and is held to
    the oracle's bits nowhere: there the reference is the same call made plainly on the default stream on buffers of its own."""
    from gym_rem2d_amd import _lib
    import geometry_forge as GF
    import test_geometry_gpu as TGE
    spec, _, fo, io = TGE.cases("distance")
    assert len(spec) >= 3 * GE_N
    c = Case(torch)
    L = _lib.lib(wide)
    tables = [np.ascontiguousarray(GF.device_table(spec[k * GE_N:(k + 1) * GE_N], GF.library_static_box(L))) for k in range(3)]
    tab = c.inp("cases", *tables)
    fout = c.out("fout", (GE_N, GF.OUT_WORDS), torch.float32, TGE.CANARY_F)
    iout = c.out("iout", (GE_N, GF.OUT_WORDS), torch.int32, TGE.CANARY_I)
    c.call = lambda: _lib.check(L.rem2d_selftest_geometry(TGE.OPS["distance"], GE_N, tab.data_ptr(), GF.DEVICE_WORDS, fout.data_ptr(),
                                                          iout.data_ptr(), 0, C.c_void_p(torch.cuda.current_stream().cuda_stream)), wide)
    zero = lambda a: np.where(a == 0, f32(0.0), a).astype(f32).view(np.uint32)          # (-0 == +0, as `==` has it)
    c.want = lambda key: [zero(fo[KEYS.index(key) * GE_N:][:GE_N]), np.asarray(io[KEYS.index(key) * GE_N:][:GE_N], np.int32)]
    c.norm = lambda key, got: [zero(got[0]), got[1]]
    if wide == "fma" and not plain:
        _against_plain_call(torch, c, case_selftest_geometry(torch, wide, plain=True))
    return c


# ------------------------------------------------------------------------------------------------------- world-taking functions
CONT = 1
N_POP = 64                                   # one 64-creature L-system population: several lane buckets, so several worlds per call
SNAP_STEPS = (("decoy", 20), ("A", 20), ("B", 30))       # the states the arenas are given: after 20, 40 and 70 steps
_RIGS = {}


def _batches(n):
    from gym_rem2d_amd import synthetic
    from gym_rem2d_amd.compiler import Morphology, lanes_for
    specs = synthetic.lsystem_specs(range(n))
    groups = {}
    for e, s in enumerate(specs):
        groups.setdefault(lanes_for(s.n_bodies), []).append(e)
    return [(Morphology.from_specs([specs[e] for e in groups[k]], k), np.asarray(groups[k])) for k in sorted(groups)]


class Rig:
    """Two envs of one build holding the same creatures: `test` is driven on the caller's stream, `ref` plainly on the default one.
    Neither is stepped by a case: a case copies one of three recorded states -- whole arenas, the bytes that are all a world carries
    from step to step -- into both and makes its call.  prepare(env): what the row needs attached (a policy, a descriptor);
    stream_of: the population is that many creatures streamed through N_POP slots (refill)."""

    def __init__(self, torch, wide, prepare, stream_of):
        from gym_rem2d_amd.env import BatchedModular2D
        self.envs = []
        for _ in range(2):
            env = BatchedModular2D(seed=4, flags=CONT, wide=wide)
            if stream_of:
                env.reset_stream(_batches(stream_of), stream_of, N_POP)
            else:
                env.reset_batches(_batches(N_POP))
            assert env.n_envs == N_POP and len(env.worlds) > 1 and not env._inactive
            if prepare is not None:
                prepare(env)
            self.envs.append(env)
        self.test, self.ref = self.envs
        fresh = [w.arena.clone() for w, _ in self.ref.worlds]
        self.snaps = {}
        for key, n in SNAP_STEPS:
            self.ref.step(n)
            torch.cuda.synchronize()
            self.snaps[key] = [w.arena.cpu().numpy().copy() for w, _ in self.ref.worlds]
        assert self.ref.handover_failures() == 0
        for (w, _), a in zip(self.ref.worlds, fresh):
            w.arena.copy_(a)
        torch.cuda.synchronize()

    def close(self):
        for env in self.envs:
            env.close()


def _rig(torch, wide, tag, prepare=None, stream_of=0):
    if (tag, wide) not in _RIGS:
        _RIGS[(tag, wide)] = Rig(torch, wide, prepare, stream_of)
    return _RIGS[(tag, wide)]


def _biggest(env):
    """the env's world of most creatures"""
    return max(range(len(env.worlds)), key=lambda i: env.worlds[i][0].n_envs)


def _field(w, host, name):
    """the words of the per-creature field `name` inside a world's arena as host bytes"""
    from gym_rem2d_amd import _lib
    off, cnt, dt = C.c_size_t(), C.c_size_t(), C.c_int32()
    _lib.check(w.L.rem2d_world_field(w.h, _lib.FIELD_ID[name], C.byref(off), C.byref(cnt), C.byref(dt)), w.wide)
    dtype = (np.float32, np.int32, np.float64)[dt.value]
    assert cnt.value >= w.n_envs
    return host[off.value:off.value + cnt.value * np.dtype(dtype).itemsize].view(dtype)[:w.n_envs]


def _world_case(torch, wide, make, writes_world, tag="plain", prepare=None, stream_of=0, forge=None):
    """make(case, env, rig): registers the row's inputs and outputs beside the arenas and sets case.call -- run for the test env and
    for the reference env alike.  The reference of a data set is what the same call leaves, made plainly, after a drain, on the
    default stream.  forge(world, arena bytes, key): words the row wants in a state that the recorded ones do not hold, written into
    both envs' copies alike."""
    rig = _rig(torch, wide, tag, prepare, stream_of)
    sides = []
    for env in (rig.test, rig.ref):
        c = Case(torch)
        for i, (w, _) in enumerate(env.worlds):
            states = [rig.snaps[k][i].copy() for k in KEYS]
            if forge is not None:
                for k, a in zip(KEYS, states):
                    forge(w, a, k)
            c.bind("arena%d" % i, w.arena, *states)
        make(c, env, rig)
        if writes_world:
            for i in range(len(env.worlds)):
                c.inout("arena%d" % i)
        sides.append(c)
    c, ref = sides
    _against_plain_call(torch, c, ref)
    return c


def _rng(seed, tag):
    return np.random.default_rng([seed, tag, 88])


def mk_observe(c, env, rig):
    from gym_rem2d_amd import control
    out = c.out("obs", (env.n_envs, control.width(env.max_bodies)), c.torch.float32, F_SENT)
    c.call = lambda: env.observe(out=out)


def mk_control(c, env, rig):
    tg = c.inp("targets", *_sets(lambda s, fin: _rng(s, 1).uniform(-1.5, 1.5, (env.n_envs, env.max_bodies))))
    c.call = lambda: env.set_joint_targets(tg)           # (float64 on the env's device, no mask: the wrapper queues nothing of its own)


def prep_sense(env):
    env.sense_terrain()                                  # (the ray table is uploaded and cached, the persistent buffers made)


def mk_sense(c, env, rig):
    out = c.out("frac", (env.n_envs, 10), c.torch.float32, F_SENT)
    c.call = lambda: env.sense_terrain(out=out)


ACT_BODIES, ACT_HIDDEN = 8, 5


def prep_act(env):
    from gym_rem2d_amd import policy
    env.set_policy(policy.MLPPolicy.random(N_POP, ACT_BODIES, ACT_HIDDEN, seed=3))


def prep_act_recurrent(env):
    from gym_rem2d_amd import policy
    env.set_policy(policy.RecurrentPolicy.random(N_POP, ACT_BODIES, ACT_HIDDEN, CONTEXT, seed=3))


def mk_act(c, env, rig):
    """the four launches each leave a trace: the observation rows, the ray fractions, targets and validity bytes, the joints' words"""
    P = env._policy
    if P["memory"] is not None:
        c.bind("memory", P["memory"], *_sets(lambda s, fin: _rng(s, 2).standard_normal((N_POP, CONTEXT)).astype(f32)))
    c.out_existing("obs", P["obs"], F_SENT)
    c.out_existing("frac", P["frac"], F_SENT)
    c.out_existing("targets", P["targets"], F_SENT)
    c.out_existing("valid", P["valid"], 0xA5)
    c.insensitive = {"valid"}                # (every target is finite in all three states: the bytes are 1 throughout)
    if P["memory"] is not None:
        c.inout("memory")
    c.call = lambda: env.act()


def mk_reset_where(c, env, rig):
    ep = env.episodes
    mask = c.inp("mask", *_sets(lambda s, fin: (_rng(s, 3).random(N_POP) < 0.5).astype(np.uint8)))
    c.bind("count", ep.count, *_sets(lambda s, fin: _rng(s, 4).integers(0, 5, N_POP).astype(np.int32)))
    c.out_existing("reward", ep.reward, F_SENT)
    c.out_existing("done", ep.done, 0xA5)
    c.out_existing("ended", ep.ended, 0xA5)
    c.out_existing("fitness", ep.fitness, F_SENT)
    c.out_existing("steps", ep.steps, I_SENT)
    c.inout("count")
    c.insensitive = {"done"}                 # (nobody has met the wall of death after 70 steps: `done` is 0 in every state)
    c.call = lambda: env.reset_where(mask)


STREAM_TOTAL, REFILL_AFTER = 96, 100         # 96 creatures through 64 slots; an episode is over after 100 steps


def forge_refill(w, arena, key):
    """ONE creature per world has reached the step limit, another one in A than in B, nobody in the decoy.  Which pending creature a
    slot takes is decided by an atomic cursor per lane bucket: with two finished slots in a bucket the outcome depends on who comes
    first, and no reference could be held to on bits."""
    steps = _field(w, arena, "steps")
    assert steps.dtype == np.int32
    steps[:] = 5
    if key != "decoy":
        steps[min(KEYS.index(key), len(steps) - 1)] = REFILL_AFTER


def mk_refill(c, env, rig):
    rec = env.stream
    assert len({w.lanes for w, _ in env.worlds}) == len(env.worlds)     # (a lane bucket's cursor serves one world)
    occ, cur = rec.occupant.cpu().numpy().copy(), rec.cursors.cpu().numpy().copy()
    c.bind("occupant", rec.occupant, occ, occ, occ)
    c.bind("cursors", rec.cursors, cur, cur, cur)
    c.out_existing("fitness", rec.fitness, F_SENT)
    c.out_existing("steps", rec.steps, I_SENT)
    c.out_existing("err", rec.err, I_SENT)
    c.out_existing("finished", rec.finished, 0xA5)
    c.inout("occupant")
    c.inout("cursors")
    c.call = lambda: env.refill(when=("steps",), max_steps=REFILL_AFTER)


DESC_PERIOD, DESC_SAMPLES = 10, 4


def prep_describe(env):
    env.set_descriptor(DESC_PERIOD, DESC_SAMPLES)


def mk_describe(c, env, rig):
    c.bind("behaviour", env.behaviour, *_sets(lambda s, fin: _rng(s, 5).standard_normal((N_POP, 2 * DESC_SAMPLES)).astype(f32)))
    c.inout("behaviour")
    c.call = lambda: env.describe()


def mk_gather(c, env, rig):
    """both kernels of the call: an 8-byte field and a 4-byte one, of the env's largest world (the other worlds' rows keep the sentinel)"""
    w = env.worlds[_biggest(env)][0]
    fit = c.out("fitness", (N_POP,), c.torch.float64, F_SENT)
    steps = c.out("steps", (N_POP,), c.torch.int32, I_SENT)

    def call():
        w.gather("fitness", fit)
        w.gather("steps", steps)
    c.call = call


def _orders(w, dtype):
    def make(seed, fin):
        full = np.arange(w.n_envs_padded, dtype=dtype)
        full[:w.n_envs] = _rng(seed, 6).permutation(w.n_envs)
        return full
    return _sets(make)


def _install_order(w, order):
    from gym_rem2d_amd import _lib
    return lambda: _lib.check(w.L.rem2d_world_set_order(w.h, order.data_ptr(), w._stream()), w.wide)


def mk_read_order(c, env, rig):
    """(ctypes: BatchedWorld.order() allocates what it returns.)  What the call reads is the library's own array: each data set is
    installed by rem2d_world_set_order on the stream of the inputs, behind them.  So this row rests on rem2d_world_set_order
    honouring its stream, which has a row of its own: where both fail, look at that one first."""
    from gym_rem2d_amd import _lib
    w = env.worlds[_biggest(env)][0]
    order = c.inp("order", *_orders(w, np.int32))
    out = c.out("read", (2, w.n_envs_padded), c.torch.int32, I_SENT)
    c.after_load = _install_order(w, order)
    c.call = lambda: _lib.check(w.L.rem2d_world_read_order(w.h, out.data_ptr(), w._stream()), w.wide)


def mk_set_order(c, env, rig):
    w = env.worlds[_biggest(env)][0]
    order = c.inp("order", *(a[:w.n_envs] for a in _orders(w, np.int64)))
    c.derived.append(("order", w.order))
    c.call = lambda: w.set_order(order, check=False)


def forge_make_order(w, arena, key):
    """position-iteration counts on both sides of the thresholds, others in every state (after a few quiet steps they are all alike)"""
    it = _field(w, arena, "positers")
    assert it.dtype == np.int32
    it[:] = _rng(KEYS.index(key), 8).integers(0, 8, len(it))


def mk_make_order(c, env, rig):
    """from the identity, with a threshold of 4 position iterations: creatures at or above it first, those with 3 next, then the rest.
    The identity is installed by rem2d_world_set_order on the stream of the inputs and the result is read by rem2d_world_read_order
    after a drain: the row rests on those two, which have rows of their own -- where they fail too, look at them first."""
    w = env.worlds[_biggest(env)][0]
    ident = c.torch.arange(w.n_envs_padded, dtype=c.torch.int32, device=c.dev)
    c.keep = ident
    c.after_load = _install_order(w, ident)
    c.derived.append(("order", w.order))
    c.call = lambda: w.make_order(4)


def mk_world_reset(c, env, rig):
    """(ctypes: BatchedWorld.reset() plans and uploads tiles first, which blocks.)  The morphology arrays on the device are the input:
    the world's own creatures in three orders."""
    from gym_rem2d_amd import _lib
    i = _biggest(env)
    w, host = env.worlds[i][0], env._world_morph[i]
    takes = [host.take(_rng(s, 7).permutation(host.n_envs)) for s in (1, 2, 3)]
    m = _lib.Morph()
    for k in _lib.MORPH_FIELDS:
        c.bind("morph_" + k, w._morph_dev[k], *(tk.arrays[k] for tk in takes))
        setattr(m, k, w._morph_dev[k].data_ptr())
    c.keep = m
    c.call = lambda: _lib.check(w.L.rem2d_world_reset(w.h, C.byref(m), w._stream()), w.wide)


def _w(make, writes_world, **kw):
    return lambda torch, wide: _world_case(torch, wide, make, writes_world, **kw)


WORLD_CASES = {
    "rem2d_worlds_observe": _w(mk_observe, False),
    "rem2d_worlds_control": _w(mk_control, True),
    "rem2d_worlds_sense": _w(mk_sense, False, tag="sense", prepare=prep_sense),
    "rem2d_worlds_act": _w(mk_act, True, tag="act", prepare=prep_act),
    "rem2d_worlds_act_recurrent": _w(mk_act, True, tag="act_recurrent", prepare=prep_act_recurrent),
    "rem2d_worlds_reset_where": _w(mk_reset_where, True),
    "rem2d_worlds_refill": _w(mk_refill, True, tag="refill", stream_of=STREAM_TOTAL, forge=forge_refill),
    "rem2d_worlds_describe": _w(mk_describe, False, tag="describe", prepare=prep_describe),
    "rem2d_world_gather": _w(mk_gather, False),
    "rem2d_world_read_order": _w(mk_read_order, False),
    "rem2d_world_set_order": _w(mk_set_order, False),
    "rem2d_world_make_order": _w(mk_make_order, False, forge=forge_make_order),
    "rem2d_world_reset": _w(mk_world_reset, True, tag="reset"),
}


# ------------------------------------------------------------------------------------------------------------------ the table
CASES = {
    "rem2d_policy_forward": case_policy_forward,
    "rem2d_recurrent_forward": case_recurrent_forward,
    "rem2d_policy_select": case_policy_select,
    "rem2d_policy_vary": case_policy_vary,
    "rem2d_policy_evolve": case_policy_evolve,
    "rem2d_es_sample": case_es_sample,
    "rem2d_es_shape": case_es_shape,
    "rem2d_es_update": case_es_update,
    "rem2d_es_step": case_es_step,
    "rem2d_snes_sample": lambda torch, wide: _snes_case(torch, wide, "sample"),
    "rem2d_snes_update": lambda torch, wide: _snes_case(torch, wide, "update"),
    "rem2d_snes_step": lambda torch, wide: _snes_case(torch, wide, "step"),
    "rem2d_novelty_score": lambda torch, wide: _novelty_case(torch, wide, "score"),
    "rem2d_novelty_add": lambda torch, wide: _novelty_case(torch, wide, "add"),
    "rem2d_novelty_step": lambda torch, wide: _novelty_case(torch, wide, "step"),
    "rem2d_pareto_rank": case_pareto_rank,
    "rem2d_pareto_local": case_pareto_local,
    "rem2d_elites_insert": lambda torch, wide: _elites_case(torch, wide, "insert"),
    "rem2d_elites_sample": lambda torch, wide: _elites_case(torch, wide, "sample"),
    "rem2d_elites_emit": lambda torch, wide: _elites_case(torch, wide, "emit"),
    "rem2d_tree_diversity": case_tree_diversity,
    "rem2d_selftest_scalar": case_selftest_scalar,
    "rem2d_selftest_geometry": case_selftest_geometry,
}
CASES.update(WORLD_CASES)
_MEMO = {}


def _case(torch, name, build):
    """the case, built once per (row, build) and shared by the two legs; its models are memoised by data set"""
    if (name, build) not in _MEMO:
        c = CASES[name](torch, build)
        memo, model = {}, c.want
        c.want = lambda key: memo[key] if key in memo else memo.setdefault(key, model(key))
        _MEMO[(name, build)] = c
    return _MEMO[(name, build)]


def _bid(b):
    return {False: "default", True: "wide", "fma": "fma"}[b]


def _ids():
    """every queued row of the table in the three builds; a row without a case here fails as a KeyError"""
    return [pytest.param(n, b, id="%s-%s" % (n, _bid(b))) for n in CS.rows(CS.QUEUED) for b in BUILDS]


@pytest.fixture(scope="module", autouse=True)
def _released():
    """whatever was selected and however it ended: the cases' buffers and the rigs' worlds are given back with the module"""
    yield
    _MEMO.clear()
    for rig in _RIGS.values():
        rig.close()
    _RIGS.clear()


def test_cases_are_the_queued_rows(gpu):
    assert sorted(CASES) == CS.rows(CS.QUEUED), sorted(set(CASES) ^ set(CS.rows(CS.QUEUED)))


# ----------------------------------------------------------------------------------------------------------- capture and replay
@pytest.mark.parametrize("name,build", _ids())
def test_capture_and_replay(gpu, name, build):
    """The call alone captured on a caller's stream: the capture succeeds (nothing synchronised, allocated through HIP or touched
    the legacy stream), nothing ran during it, and each replay computes the reference of what the inputs hold then."""
    torch = gpu
    c = _case(torch, name, build)
    what = "%s (%s build)" % (name, _bid(build))
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
    c.load("B")                                   # in place: the graph holds the addresses
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    c.compare("B", what + " second replay")
    del g


# ------------------------------------------------------------------------------------------------------------- behind a gate
SECOND_STREAMS = 8                           # how many fresh second streams the control may go through


def _gated(torch, c, cycles, astray=False):
    """decoy in, sentinels out, device drained; then on a fresh stream: the spin, the real inputs, the call.  astray (the control):
    the call is made under a second stream instead, which does not wait for the first -> (what the outputs hold in the end, whether
    the spin was still running when the second stream had run dry: an event recorded right behind the spin).  The outputs are read
    after a drain of the whole device, not of the second stream: the control must not rest on the call honouring the stream it is
    given, which is what the leg is there to find out."""
    c.load("decoy")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        opened = torch.cuda.Event()
        opened.record()
        for _, t, sets in c.inputs:
            t.copy_(sets["A"])
        if c.after_load is not None:
            c.after_load()
        if not astray:
            c.call()
    if astray:
        s2 = torch.cuda.Stream()
        with torch.cuda.stream(s2):
            c.call()
        s2.synchronize()
        still = not opened.query()
        torch.cuda.synchronize()
        return c.read(), still
    s.synchronize()
    return None


@pytest.fixture(scope="module")
def gate(gpu):
    """-> the gate's cycle count: doubled until an event pair around the spin reads GATE_MS; then proved by the control -- the same
    arrangement for MLPPolicy.forward with the call under a second stream, which must compute the decoy's result while the spin is
    still running.  Two HIP streams may share a hardware queue, and then the second does wait for the first: a second stream that
    runs dry only after the spin proves nothing about the gate either way, and the control goes on to the next fresh one, up to
    SECOND_STREAMS.  The control is passed only by the decoy's result from beside a running spin; if no second stream gives it, the
    leg is inconclusive: it errors out, it does not pass."""
    torch = gpu
    cycles, ms = 1 << 20, 0.0
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= GATE_MS:
            break
        assert cycles < 1 << 40, "the spin does not lengthen with its cycle count: %d cycles read %.3f ms" % (cycles, ms)
        cycles *= 2
    print("gate: %d cycles read %.2f ms" % (cycles, ms))
    c = _case(torch, "rem2d_policy_forward", False)
    c.reads_decoy()
    same = lambda got, want: all((np.asarray(g).reshape(-1) == np.asarray(w).reshape(-1)).all() for g, w in zip(got, want))
    seen = []
    for attempt in range(SECOND_STREAMS):
        raw, still = _gated(torch, c, cycles, astray=True)
        got = c.norm("decoy", raw)
        if still and same(got, c.want("decoy")) and not same(got, c.want("A")):
            print("gate: the control read the decoy on second stream %d" % (attempt + 1))
            return cycles
        # (a second stream that waited for the first one's spin shares its queue; one that left the real data's result ran behind
        # the copies, whatever the event said a moment later: neither proves anything about the gate, the next fresh stream may)
        seen.append("%s, spin %s" % ("the decoy's result" if same(got, c.want("decoy")) else "the real data's result"
                                     if same(got, c.want("A")) else "neither result", "running" if still else "over"))
    raise RuntimeError("the gate leg is inconclusive: none of %d fresh second streams left the decoy's result beside a running %d-cycle "
                       "(%.2f ms) spin on the first: %s" % (SECOND_STREAMS, cycles, ms, "; ".join(seen)))


@pytest.mark.parametrize("name,build", _ids())
def test_behind_a_gate(gpu, gate, name, build):
    """The call on a caller's stream behind a spin and the copies that bring its real inputs: every launch that is ordered on that
    stream sees them; one that went anywhere else reads the decoy, whose result the reference shows to differ in every output."""
    torch = gpu
    c = _case(torch, name, build)
    c.reads_decoy()
    _gated(torch, c, gate)
    what = "%s (%s build) behind the gate" % (name, _bid(build))
    got, decoy = c.norm("decoy", c.read()), c.want("decoy")
    for n, g, d in zip(c.names(), got, decoy):
        assert n in c.insensitive or (np.asarray(g).reshape(-1) != np.asarray(d).reshape(-1)).any(), \
            "%s: `%s` holds the DECOY's result: a launch did not wait for the caller's stream" % (what, n)
    c.compare("A", what)
