"""The adaptive evolution strategy for device policies without a GPU (include/rem2d_snes.h): the header's worked example, a host
model with teeth, the bound on the second sum at the largest group, the strategy beating the plain ES on an ill-conditioned
quadratic, and the header, the ctypes binding and the three libraries in agreement; the argument checks of the entry points and
the value errors of policy.SeparableES.

The GPU half (tests/test_snes_gpu.py) compares the kernels with tests/snes_model.py bit for bit; this half makes sure that the
model is no vacuous yardstick."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import es_model as ES
import snes_model as SN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
u32 = np.uint32


def small_set(M, seed, MB=1, R=0, H=2, scale=0.3):
    rng = np.random.default_rng([M, seed])
    D = 8 + 6 * MB + R
    return [(rng.standard_normal(s) * scale).astype(f32) for s in ((M, D, H), (M, H), (M, H, MB), (M, MB))]


def word(x):
    return int(np.asarray(x, f32).reshape(-1).view(u32)[0])


# ----------------------------------------------------------------------------------------------------------- header example
def test_the_headers_example():
    """S = 2, util = [3, 1], s = 1000: the numbers the header works by hand"""
    d, p = SN.pair_terms([3, 1], 2, 0)
    assert d.tolist() == [2] and p.tolist() == [4]
    g, h = 2 * 1000, 4 * (1000 * 1000 - 2 ** 31)
    assert h == -8585934592 and int(f32(np.float64(h))) == -8585934848
    c = dict(SN.scalars(2), sstep=f32(0.125), mstep=f32(1.0))
    new, sg, _, _ = SN.apply_sums([0.0], [f32(0.1)], None, None, [g], [h], c, 0)
    assert word(sg) == 0x3D75D22F and word(new) == 0x3D30C6D5
    x = f32(0.125) * (f32(np.float64(h)) * f32(2.0 ** -31))
    assert float(x) == -0.4997671842575073 and word((f32(2) + x) / (f32(2) - x)) == 0x3F19A35D
    # the clamp of x and of sigma, and the NaN rules
    for hh, want in ((2 ** 62, 3.0), (-2 ** 62, 1.0 / 3.0)):
        _, sg, _, _ = SN.apply_sums([0.0], [f32(1.0)], None, None, [0], [hh], c, 0)
        assert word(sg) == word(f32(1.0) * (f32(want) if want == 3.0 else f32(1) / f32(3)))
    _, sg, _, _ = SN.apply_sums([0.0] * 3, [f32(9.0), f32(2e-6), f32(np.nan)], None, None, [0] * 3, [2 ** 62, -2 ** 62, 0], c, 0)
    assert word(sg[0]) == word(f32(10.0)) and word(sg[1]) == word(f32(1e-6)) and np.isnan(sg[2])
    _, sg, _, _ = SN.apply_sums([0.0], [f32(0.5)], None, None, [0], [5], dict(c, sstep=f32(np.nan)), 0)       # a NaN x is 0
    assert word(sg) == word(f32(0.5))
    # E[s^2] over the 2^96 equally likely (x1, x2, x3): six halves of variance (2^32 - 1) / 12 each
    assert 6 * (2 ** 32 - 1) / 12 == 2 ** 31 - 0.5


# -------------------------------------------------------------------------------------------------------------------- teeth
def test_the_model_has_teeth():
    """What a kernel could get wrong shows in bits: skipping a pair on d == 0 alone, s * s in 32 bits, a float running sum for h,
    the NEW sigma in the natural step, beta m + omb g rounded once, exp in place of the Pade form"""
    M, S, seed, gen = 2, 64, 5, 3
    mean, sigma = small_set(M, 1), [np.abs(a) + f32(0.05) for a in small_set(M, 2)]
    m1, m2 = small_set(M, 3, scale=0.01), [np.abs(a) for a in small_set(M, 4, scale=1e-4)]
    rng = np.random.default_rng(7)
    util = ES.shape_model(rng.integers(0, 5, M * S).astype(np.float64), S)        # ties: pairs with d == 0 and p != 0 among them
    d, p = SN.pair_terms(util, S, 0)
    assert ((d == 0) & (p != 0)).any()
    c = SN.scalars(S, adam=(0.9, 0.999, 1e-8), t=3)
    both = SN.ADAM | SN.NATURAL
    right = SN.update_model(mean, sigma, m1, m2, util, S, c, both, seed, gen)
    again = SN.update_model(mean, sigma, m1, m2, util, S, c, both, seed, gen)
    assert all(np.array_equal(SN.bits(a), SN.bits(b)) for x, y in zip(right, again) for a, b in zip(x, y))

    def differs(wrong, which, least):
        share = float(np.mean([(SN.bits(a) != SN.bits(b)).mean() for a, b in zip(right[which], wrong[which])]))
        return share > least, share

    names = ("mean", "sigma", "m1", "m2")
    for kw, which, least in ((dict(skip_on_d=True), 1, 0.5), (dict(square32=True), 1, 0.5), (dict(acc=np.float32), 1, 0.05),
                             (dict(new_sigma_in_natural=True), 0, 0.5), (dict(fused_adam=True), 2, 0.05), (dict(use_exp=True), 1, 0.3)):
        ok, share = differs(SN.update_model(mean, sigma, m1, m2, util, S, c, both, seed, gen, **kw), which, least)
        print("%s: %.1f %% of the new %s's words differ" % (kw, 100 * share, names[which]))
        assert ok, (kw, share)
    # the flags matter, and the sums alone decide: all-zero util leaves the mean and sigma as they are (without Adam)
    plain = SN.update_model(mean, sigma, None, None, util, S, c, 0, seed, gen)
    assert plain[2] is None and (SN.bits(plain[0][0]) != SN.bits(right[0][0])).mean() > 0.5
    still = SN.update_model(mean, sigma, None, None, np.zeros(M * S, np.int32), S, c, SN.NATURAL, seed, gen)
    assert all(np.array_equal(SN.bits(a), SN.bits(b)) for a, b in zip(still[0] + still[1], mean + sigma))
    # the sample: sigma word by word
    kids = SN.sample_model(mean, sigma, S, seed, gen)
    flat = [np.full_like(a, 0.1) for a in mean]
    assert all(np.array_equal(SN.bits(a), SN.bits(b)) for a, b in zip(SN.sample_model(mean, flat, S, seed, gen), ES.sample_model(mean, S, 0.1, seed, gen)))
    assert (SN.bits(kids[0]) != SN.bits(ES.sample_model(mean, S, 0.1, seed, gen)[0])).mean() > 0.9


def test_wrapping_sums_with_any_util():
    """h wraps modulo 2^64 for a caller's util, as Python's integers say"""
    S, seed, gen = 6, 9, 2
    util = np.array([2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31, 5, 123456789, -987654321], np.int32)
    h = SN.second_sums(util, S, 14, 1, 0, seed, gen)
    s = ES.draw_sums(14, [0, 2, 4], 1, seed, gen)
    for i in range(14):
        tot = 0
        for q in range(3):
            a, b = int(util[2 * q]), int(util[2 * q + 1])
            pq = ((a + b + 2 ** 31) % 2 ** 32) - 2 ** 31
            tot += pq * (int(s[q, i]) ** 2 - 2 ** 31)
        assert int(h[i]) == ((tot + 2 ** 63) % 2 ** 64) - 2 ** 63


def test_the_second_sum_stays_below_2_63_at_8192():
    """p = 2 (S - 1) on every pair (the level-pairs pattern at its extreme) and the model's own draws: |h| < 2^63 at S = 8192,
    inside the header's bound, and wide enough that a 32-bit anything fails"""
    S, seed, gen = SN.MAX_GROUP, 1, 1
    util = np.full(S, S - 1, np.int32)
    h = SN.second_sums(util, S, 17, 1, 0, seed, gen)
    s = ES.draw_sums(17, 2 * np.arange(S // 2), 1, seed, gen)
    exact = [sum(2 * (S - 1) * (int(v) ** 2 - 2 ** 31) for v in s[:, i]) for i in range(17)]      # Python integers: no wrap
    assert h.tolist() == exact
    worst = max(abs(v) for v in exact)
    print("S = 8192: max |h| = 2^%.1f" % np.log2(float(worst)))
    assert 2 ** 40 < worst < 2 ** 63 and worst <= S * S * 2 ** 35.1
    # the bound itself: |s^2 - 2^31| <= max(2^31, 196605^2 - 2^31) < 2^35.1, S / 2 pairs of |p| <= 2 (S - 1)
    assert max(2 ** 31, 196605 ** 2 - 2 ** 31) < 2 ** 35.1 and (S // 2) * 2 * (S - 1) * 2 ** 35.1 < 2 ** 62
    assert (2 * S // 2) * 2 * (2 * S - 1) * (196605 ** 2 - 2 ** 31) > 2 ** 63                      # twice the size: no longer


# -------------------------------------------------------------------------------------------------------------------- climb
def test_adaptive_sigma_beats_the_plain_strategy():
    """f(theta) = -sum c_i (theta_i - theta*_i)^2, c_i = 10^(-4 i / 32), on the 33 words of one (MB 1, R 0, H 2) set, S = 64,
    mean 0, theta* standard normal from default_rng(1000 + seed), sigma 0.1, lr 0.05, 60 generations, seeds 0 .. 9: the model with
    lr_sigma = 4 (no Adam, not natural, bounds 1e-6 .. 10) ends with a smaller loss than es_model alone, for every seed"""
    S, sigma, lr, gens = 64, 0.1, 0.05, 60
    curv = 10.0 ** (-4.0 * np.arange(33) / 32.0)
    shapes = ((1, 14, 2), (1, 2), (1, 2, 1), (1, 1))
    flat = lambda W: np.concatenate([a.reshape(a.shape[0], -1) for a in W], axis=1).astype(np.float64)
    loss = lambda W, star: float((curv * (flat(W)[0] - star) ** 2).sum())
    step, c = ES.step_for(lr, S, sigma), SN.scalars(S, sigma=sigma, lr=lr, lr_sigma=4.0)
    ratios = []
    for seed in range(10):
        star = np.random.default_rng(1000 + seed).standard_normal(33)
        plain = [np.zeros(s, f32) for s in shapes]
        mean, sg = [np.zeros(s, f32) for s in shapes], [np.full(s, sigma, f32) for s in shapes]
        for gen in range(1, gens + 1):
            fit = -(curv[None, :] * (flat(ES.sample_model(plain, S, sigma, seed, gen)) - star[None, :]) ** 2).sum(axis=1)
            plain = ES.update_model(plain, ES.shape_model(fit, S), S, step, seed, gen)
            fit = -(curv[None, :] * (flat(SN.sample_model(mean, sg, S, seed, gen)) - star[None, :]) ** 2).sum(axis=1)
            mean, sg, _, _ = SN.update_model(mean, sg, None, None, ES.shape_model(fit, S), S, c, 0, seed, gen)
        ratios.append(loss(plain, star) / loss(mean, star))
        print("seed %d: plain ES %.4g, adaptive %.4g (ratio %.2f), sigma %.3g .. %.3g" % (
            seed, loss(plain, star), loss(mean, star), ratios[-1], min(a.min() for a in sg), max(a.max() for a in sg)))
    assert all(r > 1.0 for r in ratios), ratios


# -------------------------------------------------------------------------------------------- header, binding, libraries
EXPORTS = ["rem2d_snes_abi_version", "rem2d_snes_scratch_bytes", "rem2d_snes_sample", "rem2d_snes_update", "rem2d_snes_step"]
ARRAYS = ("w1", "b1", "w2", "b2")
IN_PREFIXES, OUT_PREFIXES = ("", "sigma_", "m1_", "m2_"), ("child_", "new_", "new_sigma_", "new_m1_", "new_m2_")


def test_header_binding_and_libraries_agree():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    with open(os.path.join(ROOT, "include", "rem2d_snes.h")) as f:
        text = f.read()
    declared = re.findall(r"^\s*(?:int|int64_t)\s+(rem2d_\w+)\s*\(", text, flags=re.M)
    assert declared == EXPORTS
    assert int(re.search(r"#define REM2D_SNES_ABI_VERSION (\d+)", text).group(1)) == _lib.SNES_ABI_VERSION == 1
    assert int(re.search(r"#define REM2D_SNES_MAX_GROUP (\d+)", text).group(1)) == _lib.SNES_MAX_GROUP == SN.MAX_GROUP == 8192
    assert int(re.search(r"#define REM2D_SNES_ADAM (\d+)u", text).group(1)) == _lib.SNES_ADAM == SN.ADAM
    assert int(re.search(r"#define REM2D_SNES_NATURAL (\d+)u", text).group(1)) == _lib.SNES_NATURAL == SN.NATURAL
    for const in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "0x37B504F3", "196605", "2^31 - 1/2", "0x3F19A35D", "0x3D75D22F"):
        assert const in text, const
    body = re.search(r"typedef struct rem2d_snes \{(.*?)\} rem2d_snes;", text, flags=re.S).group(1)
    members = re.findall(r"^\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+);", body, flags=re.M)
    assert [m[2] for m in members] == [n for n, _ in _lib.Snes._fields_], members
    ctype = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}
    for (tname, star, name), (_, ct) in zip(members, _lib.Snes._fields_):
        assert ct is (C.c_void_p if star else ctype[tname]), name
    assert C.sizeof(_lib.Snes) == 8 * 4 + 8 + 10 * 4 + 39 * 8 + 8 == 400
    assert _lib.Snes.seed.offset == 32 and _lib.Snes.mstep.offset == 40 and _lib.Snes.fitness.offset == 80
    assert _lib.Snes.w1.offset == 96 and _lib.Snes.child_w1.offset == 96 + 16 * 8 and _lib.Snes.scratch.offset == 384
    for path in (_lib.LIB_PATH, _lib.WIDE_LIB_PATH, _lib.FMA_LIB_PATH):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for name in declared + ES_EXPORTS:
            assert (" T " + name) in syms, (path, name)
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        assert L.rem2d_snes_abi_version() == _lib.SNES_ABI_VERSION
        assert L.rem2d_abi_version() == 11 and L.rem2d_es_abi_version() == 1 and L.rem2d_evolve_abi_version() == 1
    # the older headers know nothing of it
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if header == "rem2d_snes.h":
            continue
        with open(os.path.join(ROOT, "include", header)) as f:
            other = f.read()
        for name in declared + ["REM2D_SNES_", "rem2d_snes"]:
            assert name not in other, (header, name)


ES_EXPORTS = ["rem2d_es_abi_version", "rem2d_es_scratch_bytes", "rem2d_es_sample", "rem2d_es_shape", "rem2d_es_update", "rem2d_es_step"]
SET_BYTES = {"w1": 4 * 114 * 32 * 4, "b1": 4 * 32 * 4, "w2": 4 * 32 * 16 * 4, "b2": 4 * 16 * 4}     # M = 4 sets of _desc
E_WORDS = 114 * 32 + 32 + 32 * 16 + 16
POINTERS = (["fitness", "util"] + [pre + k for pre in IN_PREFIXES + OUT_PREFIXES for k in ARRAYS] + ["scratch"])


def _desc(**kw):
    """a good descriptor at the workload's shape, 4 means of 16 children, both flags; the "device pointers" are never dereferenced:
    the checks come first.  The 39 buffers lie 64 MB apart, further than any of them is long."""
    from gym_rem2d_amd import _lib
    e = _lib.Snes()
    e.d, e.hidden, e.max_bodies, e.n_means, e.group_size, e.pair_chunk = 114, 32, 16, 4, 16, 0
    e.generation, e.flags, e.seed = 3, 3, 2 ** 64 - 1
    e.mstep, e.sstep, e.beta1, e.omb1, e.beta2, e.omb2, e.alpha, e.eps = 0.01, 0.01, 0.9, 0.1, 0.999, 0.001, 0.05, 1e-8
    e.sigma_min, e.sigma_max = 1e-6, 10.0
    for i, k in enumerate(POINTERS):
        setattr(e, k, (i + 1) << 26)
    e.scratch_bytes = 1 << 26
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def _at(name):
    return (POINTERS.index(name) + 1) << 26


SHAPE_CASES = [(dict(max_bodies=0, d=8), b"max_bodies"), (dict(max_bodies=65, d=398), b"max_bodies"), (dict(hidden=0), b"hidden"),
               (dict(hidden=129), b"hidden"), (dict(d=103), b"d must be"), (dict(d=169), b"d must be"), (dict(n_means=0), b"n_means"),
               (dict(n_means=-4), b"n_means"), (dict(group_size=0), b"group_size"), (dict(group_size=1), b"group_size"),
               (dict(group_size=-2), b"group_size"), (dict(group_size=7), b"group_size"), (dict(group_size=8194), b"at most 8192"),
               (dict(n_means=1, group_size=65536), b"at most 8192"), (dict(n_means=2 ** 19, group_size=2 ** 12), b"2^31 - 1"),
               (dict(pair_chunk=-1), b"pair_chunk"), (dict(flags=4), b"flags"), (dict(flags=2 ** 31 + 1), b"flags")]
NEED = 2 * 4 * 4 * E_WORDS * 8                                      # 4 means x 4 chunks of 2 pairs x 2 sums x E words x 8 bytes
SAMPLE_OVERLAPS = ((dict(child_w1=_at("w1")), b"child_w1 overlaps the mean's w1"),
                   (dict(child_w1=_at("w1") + SET_BYTES["w1"] - 4), b"child_w1 overlaps the mean's w1"),
                   (dict(child_w1=_at("w1") - 16 * SET_BYTES["w1"] + 4), b"child_w1 overlaps the mean's w1"),
                   (dict(child_b2=_at("sigma_w2") + 8), b"child_b2 overlaps sigma_w2"),
                   (dict(child_w2=_at("child_w1") + 64), b"child_w2 overlaps child_w1"))
UPDATE_OVERLAPS = [(dict(new_w1=_at("w1")), b"new_w1 overlaps the mean's w1"), (dict(new_w1=_at("w1") + SET_BYTES["w1"] - 4), b"new_w1 overlaps the mean's w1"),
                   (dict(new_w1=_at("w1") - SET_BYTES["w1"] + 4), b"new_w1 overlaps the mean's w1"),
                   (dict(new_sigma_b1=_at("sigma_b1")), b"new_sigma_b1 overlaps sigma_b1"), (dict(new_sigma_w2=_at("m2_w2") + 4), b"new_sigma_w2 overlaps m2_w2"),
                   (dict(new_m1_w1=_at("m1_w1")), b"new_m1_w1 overlaps m1_w1"), (dict(new_m2_b2=_at("b2")), b"new_m2_b2 overlaps the mean's b2"),
                   (dict(new_b2=_at("util") + 4 * 63), b"new_b2 overlaps util"), (dict(new_m2_w1=_at("new_w1")), b"new_m2_w1 overlaps new_w1"),
                   (dict(new_sigma_b2=_at("new_b2") + 4), b"new_sigma_b2 overlaps new_b2"),
                   (dict(pair_chunk=2, scratch=_at("sigma_w1") + 8), b"scratch overlaps sigma_w1"),
                   (dict(pair_chunk=2, scratch=_at("new_m1_w2") - NEED + 8), b"scratch overlaps new_m1_w2")]
STEP_OVERLAPS = [(dict(new_b1=_at("fitness") + 8 * 63), b"new_b1 overlaps fitness")]
SIGMA_BOUNDS = ((0.0, 1.0), (-1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (1.0, float("nan")), (1.0, float("inf")), (float("inf"), float("inf")),
                (-float("inf"), 1.0))
SCRATCH_CASES = ((dict(scratch=None), b"scratch"), (dict(scratch_bytes=NEED - 1), b"are needed"), (dict(scratch_bytes=0), b"are needed"),
                 (dict(scratch=_at("scratch") + 4), b"8-byte aligned"))


def test_bad_arguments_are_refused_before_anything_is_dereferenced():
    """Every REM2D_E_INVALID of include/rem2d_snes.h, in the three builds, on a machine without a GPU: nothing is launched"""
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    nan, inf = float("nan"), float("inf")
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        err = L.rem2d_last_error
        calls = {"sample": (L.rem2d_snes_sample, b"snes_sample: "), "update": (L.rem2d_snes_update, b"snes_update: "),
                 "step": (L.rem2d_snes_step, b"snes_step: ")}
        every = [(lambda e, fn=fn: fn(e, None), prefix) for fn, prefix in calls.values()]
        every.append((lambda e: L.rem2d_snes_scratch_bytes(e), b"snes_scratch_bytes: "))
        for fn, prefix in every:
            assert fn(None) == -1 and b"NULL descriptor" in err() and err().startswith(prefix)
            for kw, msg in SHAPE_CASES:
                e = _desc(**kw)
                assert fn(C.byref(e)) == -1 and msg in err() and err().startswith(prefix), (kw, err())
        # what each call needs
        fn, prefix = calls["step"]
        assert fn(C.byref(_desc(fitness=None)), None) == -1 and b"fitness" in err() and err().startswith(prefix)
        for name in ("update", "step"):
            fn, prefix = calls[name]
            assert fn(C.byref(_desc(util=None)), None) == -1 and b"util" in err() and err().startswith(prefix)
        needs = {"sample": ("", "sigma_", "child_"), "update": IN_PREFIXES + OUT_PREFIXES[1:], "step": IN_PREFIXES + OUT_PREFIXES[1:]}
        need = NEED
        for name, (fn, prefix) in calls.items():
            for pre in needs[name]:
                for k in ARRAYS:
                    e = _desc(**{pre + k: None})
                    assert fn(C.byref(e), None) == -1 and b"NULL device pointer" in err() and err().startswith(prefix), (name, pre + k, err())
            # without ADAM the moments are not looked at: the call gets as far as its last refusal, the scratch's size
            if name != "sample":
                e = _desc(flags=2, pair_chunk=2, scratch_bytes=need - 8, **{pre + k: None for pre in ("m1_", "m2_", "new_m1_", "new_m2_") for k in ARRAYS})
                assert fn(C.byref(e), None) == -1 and b"are needed" in err(), (name, err())
        # overlaps: an output with an input, an output with another output
        fn, prefix = calls["sample"]
        for kw, msg in SAMPLE_OVERLAPS:
            e = _desc(**kw)
            assert fn(C.byref(e), None) == -1 and msg in err() and err().startswith(prefix), (kw, err())
        # (the moments and the new state are nothing to sample: the same descriptor with them in a heap passes every check but the last)
        e = _desc(child_b2=_at("b2"), new_w1=_at("w1"), m1_w1=_at("w1"), new_m2_b2=None, util=None, fitness=None, sigma_min=nan)
        assert fn(C.byref(e), None) == -1 and b"child_b2 overlaps the mean's b2" in err(), err()
        for name in ("update", "step"):
            fn, prefix = calls[name]
            for kw, msg in UPDATE_OVERLAPS + (STEP_OVERLAPS if name == "step" else []):
                e = _desc(**kw)
                assert fn(C.byref(e), None) == -1 and msg in err() and err().startswith(prefix), (kw, err())
            for lo, hi in SIGMA_BOUNDS:
                e = _desc(sigma_min=lo, sigma_max=hi)
                assert fn(C.byref(e), None) == -1 and b"sigma_min" in err() and err().startswith(prefix), (lo, hi, err())
            # scratch
            assert L.rem2d_snes_scratch_bytes(C.byref(_desc(pair_chunk=2))) == need
            for kw, msg in SCRATCH_CASES:
                e = _desc(pair_chunk=2, **kw)
                assert fn(C.byref(e), None) == -1 and msg in err() and err().startswith(prefix), (kw, err())
            # without ADAM an output ON a moment is no overlap; buffers that touch are fine; the limits themselves are fine: each
            # gets as far as a refusal that comes last, new_sigma_b2 on new_b2
            for kw in (dict(flags=0, new_w1=_at("m1_w1")), dict(flags=2, new_m1_w1=_at("w1"), m2_b2=_at("new_b1")), dict(new_w1=_at("w1") + SET_BYTES["w1"]),
                       dict(new_w1=_at("w1") - SET_BYTES["w1"]), dict(sigma_min=1e-30, sigma_max=1e-30), dict(sigma_min=3e38, sigma_max=3e38),
                       dict(n_means=1, group_size=8192, scratch_bytes=1 << 40), dict(max_bodies=64, d=392 + 64, hidden=128, n_means=1, group_size=2),
                       dict(max_bodies=1, d=14, hidden=1, n_means=1, group_size=2), dict(scratch=None, scratch_bytes=0)):
                e = _desc(new_sigma_b2=_at("new_b2"), **kw)
                assert fn(C.byref(e), None) == -1 and b"new_sigma_b2 overlaps new_b2" in err(), (name, kw, err())
        # the split that pair_chunk names, and the library's choice: twice what the ES's update needs
        sb = lambda **kw: L.rem2d_snes_scratch_bytes(C.byref(_desc(**kw)))
        assert sb() == 0 and sb(pair_chunk=8) == 0 and sb(pair_chunk=100) == 0 and sb(pair_chunk=3) == 2 * 4 * 3 * E_WORDS * 8
        big = sb(n_means=1, group_size=8192)
        es = _lib.Es()
        es.d, es.hidden, es.max_bodies, es.n_means, es.group_size = 114, 32, 16, 1, 8192
        assert big > 0 and big == 2 * L.rem2d_es_scratch_bytes(C.byref(es))


# --------------------------------------------------------------------------------------------------------------- the class
def test_separable_es_value_errors():
    """Every ValueError of policy.SeparableES, none of which needs a GPU: they come before anything is allocated or launched"""
    import torch
    from gym_rem2d_amd import policy
    M, S = 3, 4
    p = policy.MLPPolicy.random(M, 4, 5, n_rays=0, seed=1)
    kids = policy.MLPPolicy.random(M * S, 4, 5, n_rays=0, seed=2)
    fit = torch.zeros(M * S, dtype=torch.float64)
    util = torch.zeros(M * S, dtype=torch.int32)
    shared = policy.MLPPolicy(p.w1, p.b1, p.w2, p.b2, index=[0, 1, 2])
    new = lambda **kw: policy.SeparableES(p, **dict(dict(group_size=S), **kw))
    es, adam = new(), new(adam=(0.9, 0.999, 1e-8))
    many = policy.MLPPolicy(torch.zeros(2 ** 18, 14, 1), torch.zeros(2 ** 18, 1), torch.zeros(2 ** 18, 1, 1), torch.zeros(2 ** 18, 1))
    nan, inf = float("nan"), float("inf")
    cases = [
        ("MLPPolicy", lambda: policy.SeparableES((p.w1, p.b1, p.w2, p.b2), S)), ("index", lambda: policy.SeparableES(shared, S)),
        ("group_size", lambda: new(group_size=None)), ("group_size", lambda: new(group_size=3)), ("group_size", lambda: new(group_size=0)),
        ("group_size", lambda: new(group_size=8194)), ("group_size", lambda: new(group_size=-2)),
        ("2\\^31 - 1", lambda: policy.SeparableES(many, 8192)),
        ("sigma must", lambda: new(sigma=0.0)), ("sigma must", lambda: new(sigma=inf)), ("sigma must", lambda: new(sigma=nan)),
        ("lr must", lambda: new(lr=nan)), ("lr must", lambda: new(lr=inf)), ("lr_sigma", lambda: new(lr_sigma=-1.0)), ("lr_sigma", lambda: new(lr_sigma=nan)),
        ("adam", lambda: new(adam=(0.9, 0.999))), ("adam", lambda: new(adam=0.9)), ("adam", lambda: new(adam=(1.0, 0.999, 1e-8))),
        ("adam", lambda: new(adam=(0.9, -0.1, 1e-8))), ("adam", lambda: new(adam=(0.9, 0.999, 0.0))), ("adam", lambda: new(adam=(0.9, nan, 1e-8))),
        ("sigma_bounds", lambda: new(sigma_bounds=(0.0, 1.0))), ("sigma_bounds", lambda: new(sigma_bounds=(2.0, 1.0))),
        ("sigma_bounds", lambda: new(sigma_bounds=(1e-6, inf))), ("sigma_bounds", lambda: new(sigma_bounds=(nan, 1.0))),
        ("sigma_bounds", lambda: new(sigma_bounds=1.0)), ("outside sigma_bounds", lambda: new(sigma=0.1, sigma_bounds=(0.2, 1.0))),
        ("generation", lambda: es.sample(-1)), ("generation", lambda: es.sample(2 ** 32)), ("generation", lambda: es.sample(1, seed=2 ** 64)),
        ("generation", lambda: es.update(fit, 1, seed=-1)), ("pair_chunk", lambda: es.update(fit, 1, pair_chunk=-1)),
        ("another MLPPolicy", lambda: es.sample(1, out=es.mean)), ("another MLPPolicy", lambda: es.sample(1, out=(kids.w1, kids.b1, kids.w2, kids.b2))),
        ("sets of this policy's shapes", lambda: es.sample(1, out=p)),
        ("sets of this policy's shapes", lambda: es.sample(1, out=policy.MLPPolicy.random(M * S, 4, 6, n_rays=0))),
        ("float64", lambda: es.update(fit.to(torch.float32), 1)), ("float64", lambda: es.update(fit.numpy(), 1)),
        ("one entry per child", lambda: es.update(fit[:M], 1)), ("one entry per child", lambda: es.update(torch.zeros(2 * M * S, dtype=torch.float64)[::2], 1)),
        ("fitness must be on", lambda: es.update(fit.to("meta"), 1)),
        ("util", lambda: es.update(None, 1, util=util.to(torch.int64))), ("util", lambda: es.update(None, 1, util=util[:5])),
        ("util", lambda: es.update(None, 1, util=[0] * 12)),
        ("scratch", lambda: es.update(fit, 1, pair_chunk=1, scratch=torch.zeros(10, dtype=torch.int64))),
        ("scratch", lambda: es.update(fit, 1, pair_chunk=1, scratch=torch.zeros(1 << 12, dtype=torch.float64))),
        ("GPU", lambda: es.sample(1)), ("GPU", lambda: es.sample(1, out=kids)), ("GPU", lambda: es.update(fit, 1)),     # all else being right
        ("GPU", lambda: adam.update(None, 1, util=util)), ("GPU", lambda: es.update(fit, 1, pair_chunk=1, scratch=torch.zeros(1 << 12, dtype=torch.int64))),
        ("state must be a dict", lambda: es.load_state(None)), ("state must be a dict", lambda: adam.load_state(es.state())),
        ("t must be", lambda: es.load_state(dict(es.state(), t=-1))), ("t must be", lambda: es.load_state(dict(es.state(), t=1.5))),
        ("sigma must be four", lambda: es.load_state(dict(es.state(), sigma=es.state()["sigma"][:3]))),
        ("mean must be four", lambda: es.load_state(dict(es.state(), mean=[t.double() for t in es.state()["mean"]]))),
        ("m2 must be four", lambda: adam.load_state(dict(adam.state(), m2=kids.w1))),
    ]
    for match, bad in cases:
        with pytest.raises(ValueError, match=match):
            bad()
    # children whose w1 starts inside sigma's storage
    n1 = M * p.w1[0].numel()
    base = torch.zeros(S * n1 + 8)
    es.sigma[0] = base[:n1].view_as(p.w1)
    over = policy.MLPPolicy(base[4:4 + S * n1].view(M * S, *p.w1.shape[1:]), kids.b1, kids.w2, kids.b2)
    with pytest.raises(ValueError, match="shares memory with sigma"):
        es.sample(1, out=over)
    # nothing above moved the object: the caller's mean is a copy, t is 0, and the state round-trips on the host
    assert es.t == 0 and adam.t == 0 and es.mean.w1.data_ptr() != p.w1.data_ptr() and torch.equal(es.mean.w1, p.w1)
    assert es.scratch_bytes() == 0 and es.scratch_bytes(pair_chunk=1) == 2 * M * 2 * (p.weight_bytes() // 4) * 8
    assert es.flags == 0 and adam.flags == 1 and new(natural=True, adam=(0.5, 0.5, 1.0)).flags == 3
    st = adam.state()
    assert sorted(st) == ["m1", "m2", "mean", "sigma", "t"] and all(float(t.min()) == float(t.max()) == float(f32(0.1)) for t in st["sigma"])
    st["t"], st["m1"][1][0, 0] = 7, 0.25
    adam.load_state(st)
    assert adam.t == 7 and float(adam.m1[1][0, 0]) == 0.25 and float(adam.state()["m1"][1][0, 0]) == 0.25
    # the scalars: computed in Python floats, rounded once, what the model's helpers give
    for obj, kw in ((new(lr=0.07, lr_sigma=3.0, sigma=0.2), dict(lr=0.07, lr_sigma=3.0, sigma=0.2)),
                    (new(lr=0.01, adam=(0.9, 0.999, 1e-8), sigma_bounds=(1e-3, 2.0)), dict(lr=0.01, adam=(0.9, 0.999, 1e-8), sigma_bounds=(1e-3, 2.0)))):
        for t in (1, 2, 50):
            got, want = obj.scalars(t), SN.scalars(S, t=t, **kw)
            assert sorted(got) == sorted(want) and all(f32(got[k]) == want[k] and isinstance(got[k], float) for k in want), (t, got, want)


def test_run_policy_snes_checks_the_env():
    from gym_rem2d_amd import evaluate, policy
    from gym_rem2d_amd.env import BatchedModular2D
    env = BatchedModular2D()
    es = policy.SeparableES(policy.MLPPolicy.random(3, 16, 32), 2)
    with pytest.raises(ValueError, match="reset first"):
        evaluate.run_policy_snes(env, es, 1)
