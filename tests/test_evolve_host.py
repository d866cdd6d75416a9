"""Evolving device policies without a GPU (include/rem2d_evolve.h): the random stream's known answers, the statistics of the noise
and of the hit test, a host model with teeth, and the header, the ctypes binding and the three libraries in agreement; the argument
checks of the three entry points and the value errors of MLPPolicy.evolve.

The GPU half (tests/test_evolve_gpu.py) compares the kernels with tests/evolve_model.py bit for bit; this half makes sure that the
model is no vacuous yardstick."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import evolve_model as EM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
N_DRAWS = 1 << 21


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def test_philox_known_answers():
    """Philox4x32-10 of Random123: the zero, the all-ones and the pi-digits vectors"""
    ones = 0xffffffff
    assert _hex(EM.philox((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(EM.philox((ones,) * 4, (ones, ones))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(EM.philox((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    # vectorised over counters == one at a time; the key is (seed lo, seed hi)
    i = np.arange(5)
    many = EM.philox((i, 9, 2, 3), EM.seed_key(0x1234567890abcdef))
    for n in range(5):
        assert [int(v[n]) for v in many] == [int(v) for v in EM.philox((n, 9, 2, 3), (0x90abcdef, 0x12345678))]


@pytest.fixture(scope="module")
def draws():
    """2^21 draws: the elements of one (oversized) array of child 7, generation 3, seed 5"""
    return EM.draws(N_DRAWS, 7, 1, 5, 3)


def test_noise_statistics(draws):
    z = EM.noise(*draws[1:])
    assert z.dtype == f32
    mean, std = float(z.astype(np.float64).mean()), float(z.astype(np.float64).std())
    print("noise: mean %.5f std %.5f min %.3f max %.3f" % (mean, std, z.min(), z.max()))
    assert abs(mean) <= 0.005 and abs(std - 1.0) <= 0.005
    assert np.abs(z).max() <= 4.25                                       # support +-3 * 65535 * C = +-4.2426


@pytest.mark.parametrize("rate", [0.01, 0.05, 0.5])
def test_hit_share(draws, rate):
    hit = draws[0].astype(np.uint64) < np.uint64(EM.rate_threshold(rate))
    dev = (hit.sum() - N_DRAWS * rate) / np.sqrt(N_DRAWS * rate * (1.0 - rate))
    print("rate %g: %d hits, %.2f binomial standard deviations" % (rate, int(hit.sum()), dev))
    assert abs(dev) <= 5.0


def test_rate_threshold_ends():
    assert EM.rate_threshold(0.0) == 0 and EM.rate_threshold(1.0) == 1 << 32 and EM.rate_threshold(0.5) == 1 << 31
    w = np.linspace(-1, 1, 64).astype(f32)
    none, hit0 = EM.mutate_set(w, 0, 1, 0, 0.1, 0, 0)
    every, hit1 = EM.mutate_set(w, 0, 1, 1 << 32, 0.1, 0, 0)
    assert not hit0.any() and hit1.all() and np.array_equal(none.view(np.uint32), w.view(np.uint32)) and (every != w).mean() > 0.9


def test_the_model_has_teeth(draws):
    """What a kernel could get wrong shows: a contracted fma(sigma, z, w) and a re-associated (sigma * C) * s differ from the model
    in at least 5 % of the hit elements"""
    n = 1 << 16
    rng = np.random.default_rng(11)
    w = (rng.standard_normal(n) * 0.3).astype(f32)
    sigma = f32(0.1)
    x1, x2, x3 = (x[:n] for x in draws[1:])
    z = EM.noise(x1, x2, x3)
    want = w + (sigma * z)
    model, hit = EM.mutate_set(w, 7, 1, 1 << 32, sigma, 5, 3)
    assert hit.all() and np.array_equal(model.view(np.uint32), want.view(np.uint32))
    fused = (sigma.astype(np.float64) * z.astype(np.float64) + w.astype(np.float64)).astype(f32)   # one rounding (test_policy_host._fma)
    s = np.rint(z.astype(np.float64) / float(EM.NOISE_SCALE)).astype(f32)                           # the integer sum, recovered
    assert np.array_equal(s * EM.NOISE_SCALE, z)
    reassoc = w + ((sigma * EM.NOISE_SCALE) * s)
    share = {k: float((v.view(np.uint32) != want.view(np.uint32)).mean()) for k, v in (("fused", fused), ("reassociated", reassoc))}
    print(share)
    assert all(v >= 0.05 for v in share.values()), share


def test_tournament_ties_go_to_the_earlier_aspirant():
    rng = np.random.default_rng(3)
    fit = rng.integers(0, 3, 200).astype(np.float64)                      # three values: ties everywhere
    a = EM.select_model(fit, 200, 4, 0, 1, 1)
    b = EM.select_model(fit, 200, 4, 0, 1, 1, late_ties=True)
    assert (a != b).any() and np.array_equal(fit[a], fit[b])              # other winners of the same fitness
    assert np.array_equal(a, EM.select_model(fit, 200, 4, 0, 1, 1))
    assert (a != EM.select_model(fit, 200, 4, 0, 1, 2)).any() and (a != EM.select_model(fit, 200, 4, 0, 2, 1)).any()
    # tournsize 1: the first aspirant, whatever its fitness
    x0 = EM.philox((0, np.arange(200), 1, 0), (1, 0))[0]
    assert np.array_equal(EM.select_model(fit, 200, 1, 0, 1, 1), ((x0.astype(np.uint64) * np.uint64(200)) >> np.uint64(32)).astype(np.int32))


def test_the_order_on_fitness():
    nan, inf = np.nan, np.inf
    assert not EM.greater(nan, nan) and not EM.greater(nan, -inf) and EM.greater(-inf, nan) and EM.greater(0.0, nan)
    assert not EM.greater(0.0, -0.0) and not EM.greater(-0.0, 0.0) and EM.greater(inf, 1e308) and not EM.greater(1.0, 1.0)
    # the elite: the lowest index of the block's maximum; a block of NaNs has its first set as its best
    fit = np.array([nan, 1.0, 3.0, 3.0, -0.0, 0.0, -inf, nan, nan, nan, nan, nan], np.float64)
    p = EM.select_model(fit, 4, 4, 1, 0, 0)
    assert (p[0], p[4], p[8]) == (2, 4, 8)
    assert all(4 * (c // 4) <= p[c] < 4 * (c // 4) + 4 for c in range(12))
    assert EM.select_model(fit, 12, 2, 1, 0, 0)[0] == 2 and (EM.select_model(fit, 1, 3, 0, 9, 9) == np.arange(12)).all()


def test_vary_model_copies_and_skips():
    rng = np.random.default_rng(5)
    G, D, H, MB = 6, 14, 3, 1
    W = [rng.standard_normal(s).astype(f32) for s in ((G, D, H), (G, H), (G, H, MB), (G, MB))]
    W[0].reshape(-1)[:4] = np.array([0x7fc01234, 0xff800000, 0x80000000, 0x00000001], np.uint32).view(f32)
    parent = np.array([0, 0, 5, -1, 6, 2])
    before = [np.full_like(a, 7.0) for a in W]
    kids, hits, written = EM.vary_model(W, parent, 3, 1, 1 << 31, 0.1, 4, 2, before=before)
    assert written.tolist() == [True, True, True, False, False, True]
    for k in range(4):
        assert np.array_equal(kids[k][0].view(np.uint32), W[k][0].view(np.uint32)) and not hits[k][0].any()    # child 0: elite
        assert (kids[k][3] == 7.0).all() and (kids[k][4] == 7.0).all()                                       # skipped: untouched
        miss = ~hits[k][1]
        assert np.array_equal(kids[k][1][miss].view(np.uint32), W[k][0][miss].view(np.uint32))
    assert hits[0][1].any() and not hits[0][1].all() and (kids[0][1][hits[0][1]] != W[0][0][hits[0][1]]).any()
    assert np.isnan(kids[0][1].reshape(-1)[0])                                                               # NaN stays NaN, hit or not
    # children 1 and 2 of the same parent would differ: the child index is in the counter
    k2, _, _ = EM.vary_model(W, np.array([0, 0, 0, 0, 0, 0]), 6, 0, 1 << 32, 0.1, 4, 2)
    assert (k2[0][1] != k2[0][2]).mean() > 0.9


# -------------------------------------------------------------------------------------------- header, binding, libraries
EXPORTS = {"rem2d_evolve_abi_version", "rem2d_policy_select", "rem2d_policy_vary", "rem2d_policy_evolve"}


def test_header_binding_and_libraries_agree():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    with open(os.path.join(ROOT, "include", "rem2d_evolve.h")) as f:
        text = f.read()
    declared = re.findall(r"^\s*int\s+(rem2d_\w+)\s*\(", text, flags=re.M)
    assert set(declared) == EXPORTS and len(declared) == 4
    for name, value in (("REM2D_EVOLVE_ABI_VERSION", _lib.EVOLVE_ABI_VERSION), ("REM2D_EVOLVE_MAX_TOURNSIZE", _lib.EVOLVE_MAX_TOURNSIZE)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value, name
    assert (_lib.EVOLVE_ABI_VERSION, _lib.EVOLVE_MAX_TOURNSIZE) == (1, 4)
    # the constants of the stream and of the noise, as the header states them
    for const in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "0x37B504F3", "196605"):
        assert const in text, const
    assert (int(EM.M0), int(EM.M1), EM.W0, EM.W1, EM.NOISE_BIAS) == (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 196605)
    assert EM.NOISE_SCALE == f32(np.sqrt(f32(2.0))) * f32(2.0 ** -16) and EM.NOISE_SCALE.view(np.uint32) == 0x37B504F3
    # the struct: the header's members in the header's order, with the header's types
    body = re.search(r"typedef struct rem2d_evolve \{(.*?)\} rem2d_evolve;", text, flags=re.S).group(1)
    members = re.findall(r"^\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+);", body, flags=re.M)
    assert [m[2] for m in members] == [n for n, _ in _lib.Evolve._fields_], members
    ctype = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}
    for (tname, star, name), (_, ct) in zip(members, _lib.Evolve._fields_):
        assert ct is (C.c_void_p if star else ctype[tname]), name
    assert C.sizeof(_lib.Evolve) == 8 * 4 + 2 * 8 + 2 * 4 + 10 * 8
    for path in (_lib.LIB_PATH, _lib.WIDE_LIB_PATH, _lib.FMA_LIB_PATH):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for name in declared:
            assert (" T " + name) in syms, (path, name)
    for wide in (False, True, "fma"):
        assert _lib.lib(wide).rem2d_evolve_abi_version() == _lib.EVOLVE_ABI_VERSION
        assert _lib.lib(wide).rem2d_abi_version() == 11
    # the pinned headers know nothing of it
    for header in ("rem2d.h", "rem2d_control.h", "rem2d_sense.h", "rem2d_policy.h", "rem2d_episode.h", "rem2d_stream.h"):
        with open(os.path.join(ROOT, "include", header)) as f:
            other = f.read()
        for name in declared + ["REM2D_EVOLVE_", "rem2d_evolve"]:
            assert name not in other, (header, name)


def _desc(**kw):
    """a good descriptor at the workload's shape; the "device pointers" are never dereferenced: the checks come first.  The ten
    buffers lie 64 MB apart, further than any of them is long."""
    from gym_rem2d_amd import _lib
    e = _lib.Evolve()
    e.d, e.hidden, e.max_bodies, e.n_sets, e.group_size, e.tournsize, e.elite = 114, 32, 16, 64, 16, 4, 1
    e.generation, e.rate_threshold, e.seed, e.sigma, e.reserved = 3, 1 << 32, 2 ** 64 - 1, 0.1, 0
    for i, k in enumerate(("fitness", "w1", "b1", "w2", "b2", "child_w1", "child_b1", "child_w2", "child_b2", "parent")):
        setattr(e, k, (i + 1) << 26)
    for k, v in kw.items():
        setattr(e, k, v)
    return e


W1_BYTES = 64 * 114 * 32 * 4
SHAPE_CASES = [(dict(max_bodies=0, d=8), b"max_bodies"), (dict(max_bodies=65, d=398), b"max_bodies"), (dict(hidden=0), b"hidden"),
               (dict(hidden=129), b"hidden"), (dict(d=103), b"d must be"), (dict(d=169), b"d must be"), (dict(n_sets=0), b"n_sets"),
               (dict(n_sets=-64), b"n_sets"), (dict(group_size=0), b"group_size"), (dict(group_size=-1), b"group_size"),
               (dict(group_size=5), b"group_size"), (dict(group_size=128), b"group_size"), (dict(tournsize=0), b"tournsize"),
               (dict(tournsize=5), b"tournsize"), (dict(elite=2), b"elite"), (dict(elite=-1), b"elite"),
               (dict(rate_threshold=(1 << 32) + 1), b"rate_threshold"), (dict(rate_threshold=2 ** 64 - 1), b"rate_threshold"),
               (dict(parent=None), b"NULL device pointer")]
WEIGHT_CASES = ([(dict([(k, None)]), b"NULL device pointer") for k in ("w1", "b1", "w2", "b2", "child_w1", "child_b1", "child_w2", "child_b2")]
                + [(dict(child_w1=1 << 27), b"child_w1 overlaps the parents' w1"),                                  # the same buffer
                   (dict(child_w1=(1 << 27) + W1_BYTES - 4), b"child_w1 overlaps the parents' w1"),                  # its first word on w1's last
                   (dict(child_w1=(1 << 27) - W1_BYTES + 4), b"child_w1 overlaps the parents' w1"),                  # its last word on w1's first
                   (dict(child_b2=(4 << 26) + 8), b"child_b2 overlaps the parents' w2"),                             # b2's child inside w2
                   (dict(child_w2=(3 << 26) - 4), b"child_w2 overlaps the parents' b1")])                            # w2's child over b1


def test_bad_arguments_are_refused_before_anything_is_dereferenced():
    """Every REM2D_E_INVALID of include/rem2d_evolve.h, in the three builds, on a machine without a GPU: nothing is launched"""
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        err = L.rem2d_last_error
        calls = ((L.rem2d_policy_select, b"select: "), (L.rem2d_policy_vary, b"vary: "), (L.rem2d_policy_evolve, b"evolve: "))
        for fn, prefix in calls:
            assert fn(None, None) == -1 and b"NULL descriptor" in err() and err().startswith(prefix)
            for kw, msg in SHAPE_CASES:
                e = _desc(**kw)
                assert fn(C.byref(e), None) == -1 and msg in err() and err().startswith(prefix), (kw, err())
        for fn, prefix in calls[1:]:
            for kw, msg in WEIGHT_CASES:
                e = _desc(**kw)
                assert fn(C.byref(e), None) == -1 and msg in err() and err().startswith(prefix), (kw, err())
        for fn, prefix in (calls[0], calls[2]):
            e = _desc(fitness=None)
            assert fn(C.byref(e), None) == -1 and b"fitness" in err() and err().startswith(prefix)
        # buffers that touch without overlapping are fine, and so is every limit itself: evolve_ok is the whole validator, so a
        # descriptor it passes is one whose refusals above came from the named field alone -- checked through a refusal that comes last
        for kw in (dict(child_w1=(1 << 27) + W1_BYTES), dict(child_w1=(1 << 27) - W1_BYTES), dict(rate_threshold=0),
                   dict(max_bodies=64, d=392 + 64, hidden=128, n_sets=2, group_size=1, tournsize=1, elite=0),
                   dict(max_bodies=1, d=14, hidden=1, n_sets=1, group_size=1)):
            e = _desc(child_b2=5 << 26, **kw)                            # ... b2's child ON b2: the last check of all
            assert L.rem2d_policy_vary(C.byref(e), None) == -1 and b"child_b2 overlaps the parents' b2" in err(), (kw, err())


def test_evolve_value_errors():
    """Every ValueError of MLPPolicy.evolve, none of which needs a GPU: they come before anything is allocated or launched"""
    import torch
    from gym_rem2d_amd import policy
    p = policy.MLPPolicy.random(6, 4, 5, n_rays=0, seed=1)
    q = policy.MLPPolicy.random(6, 4, 5, n_rays=0, seed=2)
    fit = torch.zeros(6, dtype=torch.float64)
    par = torch.zeros(6, dtype=torch.int32)
    assert p.parents is None
    shared = policy.MLPPolicy(p.w1, p.b1, p.w2, p.b2, index=[0, 1, 2])
    view = policy.MLPPolicy(p.w1, q.b1, q.w2, q.b2)                        # w1 is p's own memory
    cases = [
        ("index", lambda: shared.evolve(fit, 1)),
        ("float64", lambda: p.evolve(fit.to(torch.float32), 1)), ("float64", lambda: p.evolve(fit.numpy(), 1)),
        ("one entry per weight set", lambda: p.evolve(torch.zeros(5, dtype=torch.float64), 1)),
        ("one entry per weight set", lambda: p.evolve(torch.zeros((6, 1), dtype=torch.float64), 1)),
        ("one entry per weight set", lambda: p.evolve(torch.zeros(12, dtype=torch.float64)[::2], 1)),
        ("fitness must be on", lambda: p.evolve(fit.to("meta"), 1)),
        ("group_size", lambda: p.evolve(fit, 1, group_size=4)), ("group_size", lambda: p.evolve(fit, 1, group_size=0)),
        ("tournsize", lambda: p.evolve(fit, 1, tournsize=0)), ("tournsize", lambda: p.evolve(fit, 1, tournsize=5)),
        ("elite", lambda: p.evolve(fit, 1, elite=2)),
        ("rate", lambda: p.evolve(fit, 1, rate=1.5)), ("rate", lambda: p.evolve(fit, 1, rate=-0.1)), ("rate", lambda: p.evolve(fit, 1, rate=float("nan"))),
        ("generation", lambda: p.evolve(fit, -1)), ("generation", lambda: p.evolve(fit, 2 ** 32)), ("generation", lambda: p.evolve(fit, 1, seed=2 ** 64)),
        ("parents", lambda: p.evolve(fit, 1, parents=par.to(torch.int64))), ("parents", lambda: p.evolve(fit, 1, parents=par[:5])),
        ("parents", lambda: p.evolve(fit, 1, parents=[0] * 6)),
        ("another MLPPolicy", lambda: p.evolve(fit, 1, out=p)), ("another MLPPolicy", lambda: p.evolve(fit, 1, out=(q.w1, q.b1, q.w2, q.b2))),
        ("shapes", lambda: p.evolve(fit, 1, out=policy.MLPPolicy.random(6, 4, 6, n_rays=0))),
        ("shapes", lambda: p.evolve(fit, 1, out=policy.MLPPolicy.random(5, 4, 5, n_rays=0))),
        ("shapes", lambda: p.evolve(fit, 1, out=policy.MLPPolicy(q.w1, q.b1, q.w2, q.b2, index=[0]))),
        ("shares memory", lambda: p.evolve(fit, 1, out=view)),
        ("GPU", lambda: p.evolve(fit, 1)), ("GPU", lambda: p.evolve(fit, 1, out=q, parents=par)),   # all else being right: host weights
    ]
    for match, bad in cases:
        with pytest.raises(ValueError, match=match):
            bad()


def test_run_policy_generations_checks_the_env():
    from gym_rem2d_amd import evaluate, policy
    from gym_rem2d_amd.env import BatchedModular2D
    env = BatchedModular2D()
    with pytest.raises(ValueError, match="reset first"):
        evaluate.run_policy_generations(env, policy.MLPPolicy.random(3, 16, 32), 1)
