"""The evolution strategy for device policies without a GPU (include/rem2d_es.h): the header's util example, a host model with
teeth, the strategy climbing a quadratic, and the header, the ctypes binding and the three libraries in agreement; the argument
checks of the five entry points and the value errors of MLPPolicy.es_sample / es_update.

The GPU half (tests/test_es_gpu.py) compares the kernels with tests/es_model.py bit for bit; this half makes sure that the model is
no vacuous yardstick."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import es_model as ES
import evolve_model as EM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
nan, inf = np.nan, np.inf


def small_mean(M, seed, MB=1, R=0, H=2):
    rng = np.random.default_rng([M, seed])
    D = 8 + 6 * MB + R
    return [(rng.standard_normal(s) * 0.3).astype(f32) for s in ((M, D, H), (M, H), (M, H, MB), (M, MB))]


# ------------------------------------------------------------------------------------------------------------------ shape
def test_the_headers_util_example():
    assert ES.shape_model([nan, 1.0, 1.0, -0.0, 0.0, inf], 6).tolist() == [-5, 2, 2, -2, -2, 5]
    # two blocks: each on its own
    assert ES.shape_model([3.0, 1.0, nan, nan], 2).tolist() == [1, -1, 0, 0]


def test_util_sums_to_zero_and_level_blocks_give_zeros():
    rng = np.random.default_rng(1)
    for S in (2, 6, 64, 130):
        fit = np.concatenate([rng.standard_normal(S), rng.integers(0, 3, S).astype(np.float64), np.full(S, 2.5), np.full(S, nan),
                              rng.choice(np.array([nan, -inf, inf, -0.0, 0.0, 1e-310]), S)])
        u = ES.shape_model(fit, S).astype(np.int64).reshape(5, S)
        assert (u.sum(axis=1) == 0).all() and (np.abs(u) <= S - 1).all()
        assert (u[2] == 0).all() and (u[3] == 0).all()
        assert sorted(u[0].tolist()) == list(range(-(S - 1), S, 2))               # no ties: every centred rank once
        assert ((u[0][:, None] > u[0][None, :]) == EM.greater(fit[:S][:, None], fit[:S][None, :])).all()


def test_the_sorted_count_is_the_pairwise_count(monkeypatch):
    """es_model counts blocks above 2048 sets by sorting: the same util as the header's pairwise wording"""
    rng = np.random.default_rng(4)
    S = 258
    fit = np.concatenate([rng.standard_normal(S), rng.integers(0, 3, S).astype(np.float64), np.full(S, nan),
                          rng.choice(np.array([nan, -inf, inf, -0.0, 0.0, 1e-310, 1.5]), S)])
    pairwise = ES.shape_model(fit, S)
    monkeypatch.setattr(ES, "PAIRWISE_MAX", 0)
    assert np.array_equal(ES.shape_model(fit, S), pairwise)
    assert ES.shape_model([nan, 1.0, 1.0, -0.0, 0.0, inf], 6).tolist() == [-5, 2, 2, -2, -2, 5]


# ------------------------------------------------------------------------------------------------------------------- teeth
def test_the_model_has_teeth():
    """What a kernel could get wrong shows in bits or signs: the odd child sharing the even child's sign, util with ties to the
    lower index, a float32 running sum instead of the integer sum, the odd child's own index as the counter"""
    M, S, sigma, seed, gen = 2, 64, 0.1, 5, 3
    mean = small_mean(M, 1)
    kids = ES.sample_model(mean, S, sigma, seed, gen)
    # the pairs are antithetic about the mean: even - mean == -(odd - mean) up to the rounding of the sum, and of opposite sign
    dev = kids[0].astype(np.float64) - np.repeat(mean[0], S, axis=0)
    assert (np.sign(dev[0::2]) == -np.sign(dev[1::2])).mean() > 0.99 and np.abs(dev[0::2] + dev[1::2]).max() < 1e-7
    same = ES.sample_model(mean, S, sigma, seed, gen, same_sign=True)
    own = ES.sample_model(mean, S, sigma, seed, gen, own_counter=True)
    for wrong in (same, own):
        assert np.array_equal(ES.bits(wrong[0][0::2]), ES.bits(kids[0][0::2]))      # the even children are right in both
        assert (ES.bits(wrong[0][1::2]) != ES.bits(kids[0][1::2])).mean() > 0.9     # the odd ones are not
    devs = same[0].astype(np.float64) - np.repeat(mean[0], S, axis=0)
    assert (np.sign(devs[0::2]) == np.sign(devs[1::2])).mean() > 0.99
    # ties
    fit = np.random.default_rng(2).integers(0, 3, M * S).astype(np.float64)
    util, low = ES.shape_model(fit, S), ES.shape_model(fit, S, low_ties=True)
    assert (util != low).mean() > 0.5 and low.reshape(M, S).sum(axis=1).tolist() == [0, 0]
    assert all(len(set(util[b * S:(b + 1) * S][fit[b * S:(b + 1) * S] == v])) == 1 for b in range(M) for v in (0.0, 1.0, 2.0))
    # the float sum: other words of the new mean, once the products no longer fit 24 bits (S = 1024: |d s| up to 4 10^8)
    big, one = 1024, small_mean(1, 2)
    ranks = ES.shape_model(np.random.default_rng(3).standard_normal(big), big)
    exact = ES.update_model(one, ranks, big, ES.step_for(0.05, big, sigma), seed, gen)
    flt = ES.update_model(one, ranks, big, ES.step_for(0.05, big, sigma), seed, gen, acc=np.float32)
    share = float((ES.bits(exact[0]) != ES.bits(flt[0])).mean())
    print("float32 running sum: %.1f %% of w1's words differ" % (100 * share))
    assert share > 0.05
    step = ES.step_for(0.05, S, sigma)
    new = ES.update_model(mean, util, S, step, seed, gen)
    # the update reads the anchors' draws: the new mean moves towards the children that util favours
    assert all(a.dtype == f32 and a.shape == m.shape for a, m in zip(new, mean))
    assert np.array_equal(ES.bits(ES.update_model(mean, np.zeros(M * S, np.int32), S, step, seed, gen)[0]), ES.bits(mean[0]))


def test_an_int32_accumulator_overflows_at_4096():
    S, seed, gen = 4096, 1, 1
    util = np.empty(S, np.int32)
    util[0::2], util[1::2] = S - 1, -(S - 1)                                        # the extreme pattern: d_q = 2 (S - 1) everywhere
    g64 = ES.weighted_sums(util, S, 17, 1, 0, seed, gen)
    g32 = ES.weighted_sums(util, S, 17, 1, 0, seed, gen, acc=np.int32)
    print("S = 4096: max |g| = %.3g" % np.abs(g64).max())
    assert g64.dtype == np.int64 and np.abs(g64).max() > 2 ** 31 and np.abs(g64).max() <= S * S * 2 ** 18
    assert (g32.astype(np.int64) != g64).any() and np.array_equal(g32, g64.astype(np.int32))
    # shape's own util on a sorted block: the same order of magnitude
    ranks = ES.shape_model(np.arange(S, dtype=np.float64), S)
    assert np.abs(ES.weighted_sums(ranks, S, 17, 1, 0, seed, gen)).max() <= S * S * 2 ** 18


# ------------------------------------------------------------------------------------------------------------------- climb
def test_the_strategy_climbs():
    """f(theta) = -|theta - theta*|^2 on the 33 words of one (MB 1, R 0, H 2) set, S = 64, sigma 0.1, lr 0.05, mean 0, theta*
    standard normal, seeds 0 .. 19: the first update points towards theta* for every seed, and 40 generations at least halve the
    distance for every seed"""
    S, sigma, lr = 64, 0.1, 0.05
    step = ES.step_for(lr, S, sigma)
    worst_cos, worst = 1.0, (0.0, 0.0)
    for seed in range(20):
        star = np.random.default_rng(seed).standard_normal(33)
        mean = [np.zeros(s, f32) for s in ((1, 14, 2), (1, 2), (1, 2, 1), (1, 1))]
        flat = lambda W: np.concatenate([a.reshape(a.shape[0], -1) for a in W], axis=1).astype(np.float64)
        d0 = float(np.linalg.norm(star - flat(mean)[0]))
        for gen in range(1, 41):
            kids = ES.sample_model(mean, S, sigma, seed, gen)
            fit = -((flat(kids) - star[None, :]) ** 2).sum(axis=1)
            new = ES.update_model(mean, ES.shape_model(fit, S), S, step, seed, gen)
            if gen == 1:
                move, want = flat(new)[0] - flat(mean)[0], star - flat(mean)[0]
                cos = float(move @ want / (np.linalg.norm(move) * np.linalg.norm(want)))
                worst_cos = min(worst_cos, cos)
                assert cos > 0.0, (seed, cos)
            mean = new
        d1 = float(np.linalg.norm(star - flat(mean)[0]))
        if d1 / d0 > worst[1] / max(worst[0], 1e-30):
            worst = (d0, d1)
        assert d1 <= 0.5 * d0, (seed, d0, d1)
    print("worst first-update cosine %.2f, worst distance %.2f -> %.2f" % (worst_cos, worst[0], worst[1]))


# -------------------------------------------------------------------------------------------- header, binding, libraries
EXPORTS = ["rem2d_es_abi_version", "rem2d_es_scratch_bytes", "rem2d_es_sample", "rem2d_es_shape", "rem2d_es_update", "rem2d_es_step"]


def test_header_binding_and_libraries_agree():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    with open(os.path.join(ROOT, "include", "rem2d_es.h")) as f:
        text = f.read()
    declared = re.findall(r"^\s*(?:int|int64_t)\s+(rem2d_\w+)\s*\(", text, flags=re.M)
    assert declared == EXPORTS
    assert int(re.search(r"#define REM2D_ES_ABI_VERSION (\d+)", text).group(1)) == _lib.ES_ABI_VERSION == 1
    for const in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "0x37B504F3", "196605"):
        assert const in text, const
    assert ES.ES_DOMAIN0 == 4 and ES.ES_DOMAIN0 + 1 > 4                           # evolve's domains are 0 .. 4
    # the struct: the header's members in the header's order, with the header's types
    body = re.search(r"typedef struct rem2d_es \{(.*?)\} rem2d_es;", text, flags=re.S).group(1)
    members = re.findall(r"^\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+);", body, flags=re.M)
    assert [m[2] for m in members] == [n for n, _ in _lib.Es._fields_], members
    ctype = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}
    for (tname, star, name), (_, ct) in zip(members, _lib.Es._fields_):
        assert ct is (C.c_void_p if star else ctype[tname]), name
    assert C.sizeof(_lib.Es) == 8 * 4 + 8 + 2 * 4 + 15 * 8 + 8
    for path in (_lib.LIB_PATH, _lib.WIDE_LIB_PATH, _lib.FMA_LIB_PATH):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for name in declared:
            assert (" T " + name) in syms, (path, name)
    for wide in (False, True, "fma"):
        assert _lib.lib(wide).rem2d_es_abi_version() == _lib.ES_ABI_VERSION
        assert _lib.lib(wide).rem2d_abi_version() == 11 and _lib.lib(wide).rem2d_evolve_abi_version() == 1
    # the older headers know nothing of it
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if header == "rem2d_es.h":
            continue
        with open(os.path.join(ROOT, "include", header)) as f:
            other = f.read()
        for name in declared + ["REM2D_ES_", "rem2d_es"]:
            assert name not in other, (header, name)


POINTERS = ("fitness", "util", "w1", "b1", "w2", "b2", "child_w1", "child_b1", "child_w2", "child_b2", "new_w1", "new_b1", "new_w2",
            "new_b2", "scratch")
W1_BYTES = 4 * 114 * 32 * 4            # the mean's w1 of _desc: M = 4 sets
CHILD_W1_BYTES = 16 * W1_BYTES         # its children's: S = 16


def _desc(**kw):
    """a good descriptor at the workload's shape, 4 means of 16 children; the "device pointers" are never dereferenced: the checks
    come first.  The fifteen buffers lie 64 MB apart, further than any of them is long."""
    from gym_rem2d_amd import _lib
    e = _lib.Es()
    e.d, e.hidden, e.max_bodies, e.n_means, e.group_size, e.pair_chunk = 114, 32, 16, 4, 16, 0
    e.generation, e.reserved, e.seed, e.sigma, e.step = 3, 0, 2 ** 64 - 1, 0.1, 0.01
    for i, k in enumerate(POINTERS):
        setattr(e, k, (i + 1) << 26)
    e.scratch_bytes = 1 << 26
    for k, v in kw.items():
        setattr(e, k, v)
    return e


SHAPE_CASES = [(dict(max_bodies=0, d=8), b"max_bodies"), (dict(max_bodies=65, d=398), b"max_bodies"), (dict(hidden=0), b"hidden"),
               (dict(hidden=129), b"hidden"), (dict(d=103), b"d must be"), (dict(d=169), b"d must be"), (dict(n_means=0), b"n_means"),
               (dict(n_means=-4), b"n_means"), (dict(group_size=0), b"group_size"), (dict(group_size=1), b"group_size"),
               (dict(group_size=-2), b"group_size"), (dict(group_size=7), b"group_size"),
               (dict(n_means=2 ** 16, group_size=2 ** 15), b"2^31 - 1"), (dict(n_means=1, group_size=2 ** 31 - 1), b"group_size"),
               (dict(pair_chunk=-1), b"pair_chunk"), (dict(reserved=1), b"reserved")]
E_WORDS = 114 * 32 + 32 + 32 * 16 + 16
NEED = 4 * 4 * E_WORDS * 8             # scratch: 4 means x 4 chunks of 2 pairs x E words x 8 bytes
SCRATCH_CASES = ((dict(scratch=None), b"scratch"), (dict(scratch_bytes=NEED - 1), b"are needed"), (dict(scratch_bytes=0), b"are needed"),
                 (dict(scratch=(15 << 26) + 4), b"8-byte aligned"))


def _overlaps(prefix, sets_bytes):
    """overlaps of a destination buffer with the mean, named as evolve names them"""
    w1 = 3 << 26
    return ([(dict([(prefix + "_" + k, None)]), b"NULL device pointer") for k in ("w1", "b1", "w2", "b2")]
            + [(dict([(k, None)]), b"NULL device pointer") for k in ("w1", "b1", "w2", "b2")]
            + [(dict([(prefix + "_w1", w1)]), b"%s_w1 overlaps the mean's w1" % prefix.encode()),
               (dict([(prefix + "_w1", w1 + W1_BYTES - 4)]), b"%s_w1 overlaps the mean's w1" % prefix.encode()),
               (dict([(prefix + "_w1", w1 - sets_bytes + 4)]), b"%s_w1 overlaps the mean's w1" % prefix.encode()),
               (dict([(prefix + "_b2", (5 << 26) + 8)]), b"%s_b2 overlaps the mean's w2" % prefix.encode()),
               (dict([(prefix + "_w2", (4 << 26) - 4)]), b"%s_w2 overlaps the mean's b1" % prefix.encode())])


def test_bad_arguments_are_refused_before_anything_is_dereferenced():
    """Every REM2D_E_INVALID of include/rem2d_es.h, in the three builds, on a machine without a GPU: nothing is launched"""
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        err = L.rem2d_last_error
        calls = {"sample": (L.rem2d_es_sample, b"es_sample: "), "shape": (L.rem2d_es_shape, b"es_shape: "),
                 "update": (L.rem2d_es_update, b"es_update: "), "step": (L.rem2d_es_step, b"es_step: ")}
        every = [(lambda e, fn=fn: fn(e, None), prefix) for fn, prefix in calls.values()]
        every.append((lambda e: L.rem2d_es_scratch_bytes(e), b"es_scratch_bytes: "))
        for fn, prefix in every:
            assert fn(None) == -1 and b"NULL descriptor" in err() and err().startswith(prefix)
            for kw, msg in SHAPE_CASES:
                e = _desc(**kw)
                assert fn(C.byref(e)) == -1 and msg in err() and err().startswith(prefix), (kw, err())
        for name in ("shape", "step"):
            fn, prefix = calls[name]
            e = _desc(fitness=None)
            assert fn(C.byref(e), None) == -1 and b"fitness" in err() and err().startswith(prefix)
        for name in ("shape", "update", "step"):
            fn, prefix = calls[name]
            e = _desc(util=None)
            assert fn(C.byref(e), None) == -1 and b"util" in err() and err().startswith(prefix)
        fn, prefix = calls["sample"]
        for kw, msg in _overlaps("child", CHILD_W1_BYTES):
            e = _desc(**kw)
            assert fn(C.byref(e), None) == -1 and msg in err() and err().startswith(prefix), (kw, err())
        for name in ("update", "step"):
            fn, prefix = calls[name]
            for kw, msg in _overlaps("new", W1_BYTES):
                e = _desc(**kw)
                assert fn(C.byref(e), None) == -1 and msg in err() and err().startswith(prefix), (kw, err())
            assert L.rem2d_es_scratch_bytes(C.byref(_desc(pair_chunk=2))) == NEED
            for kw, msg in SCRATCH_CASES:
                e = _desc(pair_chunk=2, **kw)
                assert fn(C.byref(e), None) == -1 and msg in err() and err().startswith(prefix), (kw, err())
        # the split that pair_chunk names, and the library's choice
        assert L.rem2d_es_scratch_bytes(C.byref(_desc())) == 0 and L.rem2d_es_scratch_bytes(C.byref(_desc(pair_chunk=8))) == 0
        assert L.rem2d_es_scratch_bytes(C.byref(_desc(pair_chunk=100))) == 0
        assert L.rem2d_es_scratch_bytes(C.byref(_desc(pair_chunk=3))) == 4 * 3 * E_WORDS * 8
        big = L.rem2d_es_scratch_bytes(C.byref(_desc(n_means=1, group_size=65536)))
        assert big > 0 and big % (E_WORDS * 8) == 0 and big <= 1 << 24
        # buffers that touch without overlapping are fine, and so is every limit itself: es_ok is the whole validator, so a
        # descriptor it passes is one whose refusals above came from the named field alone -- checked through a refusal that comes
        # last: b2's destination ON the mean's b2
        for kw in (dict(child_w1=(3 << 26) + W1_BYTES), dict(child_w1=(3 << 26) - CHILD_W1_BYTES),
                   dict(max_bodies=64, d=392 + 64, hidden=128, n_means=1, group_size=2), dict(max_bodies=1, d=14, hidden=1, n_means=1, group_size=2),
                   dict(n_means=1, group_size=2 ** 31 - 2, child_w1=1 << 60, child_b1=1 << 61, child_w2=3 << 60)):
            e = _desc(child_b2=6 << 26, **kw)
            assert L.rem2d_es_sample(C.byref(e), None) == -1 and b"child_b2 overlaps the mean's b2" in err(), (kw, err())
        # (the update's last refusal is the scratch's size)
        for kw in (dict(new_w1=(3 << 26) + W1_BYTES), dict(new_w1=(3 << 26) - W1_BYTES), dict(child_w1=3 << 26, fitness=None)):
            e = _desc(pair_chunk=2, scratch_bytes=4 * 4 * E_WORDS * 8 - 8, **kw)
            assert L.rem2d_es_update(C.byref(e), None) == -1 and b"are needed" in err(), (kw, err())
        for kw in (dict(scratch=None, scratch_bytes=0), dict(pair_chunk=2, scratch_bytes=4 * 4 * E_WORDS * 8)):
            e = _desc(new_b2=6 << 26, **kw)
            assert L.rem2d_es_update(C.byref(e), None) == -1 and b"new_b2 overlaps the mean's b2" in err(), (kw, err())


def test_es_value_errors():
    """Every ValueError of MLPPolicy.es_sample and es_update, none of which needs a GPU: they come before anything is allocated or
    launched"""
    import torch
    from gym_rem2d_amd import policy
    M, S = 3, 4
    p = policy.MLPPolicy.random(M, 4, 5, n_rays=0, seed=1)
    kids = policy.MLPPolicy.random(M * S, 4, 5, n_rays=0, seed=2)
    q = policy.MLPPolicy.random(M, 4, 5, n_rays=0, seed=3)
    fit = torch.zeros(M * S, dtype=torch.float64)
    util = torch.zeros(M * S, dtype=torch.int32)
    assert p.util is None
    shared = policy.MLPPolicy(p.w1, p.b1, p.w2, p.b2, index=[0, 1, 2])
    view = policy.MLPPolicy(p.w1, q.b1, q.w2, q.b2)                        # w1 is p's own memory
    cases = [
        ("index", lambda: shared.es_sample(1, group_size=S)), ("index", lambda: shared.es_update(fit, 1, group_size=S)),
        ("group_size", lambda: p.es_sample(1)), ("group_size", lambda: p.es_sample(1, group_size=3)),
        ("group_size", lambda: p.es_sample(1, group_size=0)), ("group_size", lambda: p.es_update(fit, 1, group_size=5)),
        ("group_size", lambda: p.es_update(fit, 1)), ("2\\^31 - 1", lambda: p.es_sample(1, group_size=2 ** 30)),
        ("generation", lambda: p.es_sample(-1, group_size=S)), ("generation", lambda: p.es_sample(2 ** 32, group_size=S)),
        ("generation", lambda: p.es_sample(1, seed=2 ** 64, group_size=S)), ("generation", lambda: p.es_update(fit, 1, seed=-1, group_size=S)),
        ("pair_chunk", lambda: p.es_update(fit, 1, group_size=S, pair_chunk=-1)),
        ("another MLPPolicy", lambda: p.es_sample(1, group_size=S, out=p)),
        ("another MLPPolicy", lambda: p.es_sample(1, group_size=S, out=(kids.w1, kids.b1, kids.w2, kids.b2))),
        ("sets of this policy's shapes", lambda: p.es_sample(1, group_size=S, out=q)),
        ("sets of this policy's shapes", lambda: p.es_sample(1, group_size=S, out=policy.MLPPolicy.random(M * S, 4, 6, n_rays=0))),
        ("sets of this policy's shapes", lambda: p.es_sample(1, group_size=S, out=policy.MLPPolicy(kids.w1, kids.b1, kids.w2, kids.b2, index=[0]))),
        ("float64", lambda: p.es_update(fit.to(torch.float32), 1, group_size=S)), ("float64", lambda: p.es_update(fit.numpy(), 1, group_size=S)),
        ("one entry per child", lambda: p.es_update(fit[:M], 1, group_size=S)),
        ("one entry per child", lambda: p.es_update(torch.zeros((M * S, 1), dtype=torch.float64), 1, group_size=S)),
        ("one entry per child", lambda: p.es_update(torch.zeros(2 * M * S, dtype=torch.float64)[::2], 1, group_size=S)),
        ("fitness must be on", lambda: p.es_update(fit.to("meta"), 1, group_size=S)),
        ("util", lambda: p.es_update(None, 1, group_size=S, util=util.to(torch.int64))),
        ("util", lambda: p.es_update(None, 1, group_size=S, util=util[:5])), ("util", lambda: p.es_update(None, 1, group_size=S, util=[0] * 12)),
        ("sigma", lambda: p.es_update(fit, 1, group_size=S, sigma=0.0)), ("sigma", lambda: p.es_update(fit, 1, group_size=S, sigma=float("inf"))),
        ("sigma", lambda: p.es_update(fit, 1, group_size=S, sigma=float("nan"))),
        ("scratch", lambda: p.es_update(fit, 1, group_size=S, pair_chunk=1, scratch=torch.zeros(10, dtype=torch.int64))),
        ("scratch", lambda: p.es_update(fit, 1, group_size=S, pair_chunk=1, scratch=torch.zeros(1 << 12, dtype=torch.float64))),
        ("another MLPPolicy", lambda: p.es_update(fit, 1, group_size=S, out=p)),
        ("sets of this policy's shapes", lambda: p.es_update(fit, 1, group_size=S, out=kids)),
        ("shares memory", lambda: p.es_update(fit, 1, group_size=S, out=view)),
        ("GPU", lambda: p.es_sample(1, group_size=S)), ("GPU", lambda: p.es_sample(1, group_size=S, out=kids)),   # all else being right
        ("GPU", lambda: p.es_update(fit, 1, group_size=S, out=q)), ("GPU", lambda: p.es_update(None, 1, group_size=S, util=util)),
        ("GPU", lambda: p.es_update(fit, 1, group_size=S, pair_chunk=1, scratch=torch.zeros(1 << 12, dtype=torch.int64))),
    ]
    for match, bad in cases:
        with pytest.raises(ValueError, match=match):
            bad()
    # out sharing memory with the mean, for es_sample: children whose w1 IS a view that starts inside the mean's storage
    base = torch.zeros(M * S * p.w1[0].numel() + 8)
    inside = policy.MLPPolicy(base[:M * p.w1[0].numel()].view_as(p.w1), p.b1, p.w2, p.b2)
    over = policy.MLPPolicy(base[4:4 + M * S * p.w1[0].numel()].view(M * S, *p.w1.shape[1:]), kids.b1, kids.w2, kids.b2)
    with pytest.raises(ValueError, match="shares memory"):
        inside.es_sample(1, group_size=S, out=over)
    assert p.es_scratch_bytes(S) == 0 and p.es_scratch_bytes(S, pair_chunk=1) == M * 2 * (p.weight_bytes() // 4) * 8


def test_run_policy_es_checks_the_env():
    from gym_rem2d_amd import evaluate, policy
    from gym_rem2d_amd.env import BatchedModular2D
    env = BatchedModular2D()
    with pytest.raises(ValueError, match="reset first"):
        evaluate.run_policy_es(env, policy.MLPPolicy.random(3, 16, 32), 1, group_size=2)
