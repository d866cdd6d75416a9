"""Observation normalisation without a GPU (include/rem2d_obsnorm.h): the numpy model (tests/obsnorm_model.py) against plain numpy
statistics within a tolerance derived from the quantisation step, the model's invariants (split calls, the bounds at the clamp, an
empty block, constants, a variance that rounds negative), header / binding / library agreement, every REM2D_E_INVALID of the header
on descriptors whose "device pointers" are never dereferenced, the capacity guard and the checkpoint round trip of
``policy.ObsNormalizer``."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import obsnorm_model as OM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
nan, inf = float("nan"), float("inf")
H = 2.0 ** -12                                  # the quantisation step of a word


# --------------------------------------------------------------------------------------------- the model against plain numpy
@pytest.mark.parametrize("name,make", [("80 +- 1", lambda rng, n: 80.0 + rng.standard_normal(n)),
                                       ("1500 +- 0.01", lambda rng, n: 1500.0 + 0.01 * rng.standard_normal(n)),
                                       ("{0, 1, 2}", lambda rng, n: rng.integers(0, 3, n).astype(np.float64)),
                                       ("+- 0.3", lambda rng, n: 0.3 * rng.standard_normal(n))])
def test_model_against_numpy(name, make):
    """mu and inv of benign data against numpy's mean and 1 / std (binary64, ddof = 0).  The bounds, derived:
    every word moves by at most H / 2 when it is quantised, so the mean moves by at most H / 2, and the standard deviation -- the
    2-norm of the centred vector over sqrt(n), a norm -- by at most H / 2 too (triangle inequality).  On top: the binary64 rounding
    of s2, m m (2^-53 relative each, on numbers of size s2 while v may be far smaller: 2^-51 (m^2 + v) / v relative on v, half of
    that on the root) and the binary32 roundings of mu (2^-24 relative) and of vx, its root and the quotient (3 2^-24 relative)."""
    rng = np.random.default_rng(len(name))
    n = 4000
    x = make(rng, n).astype(f32)
    st = OM.accumulate(OM.State(1, 1), x[:, None], n)
    assert int(st.count[0]) == n
    mu, inv = OM.freeze(*st.words(), min_count=1, min_var=2.0 ** -40)
    mean, std = float(np.mean(x.astype(f64))), float(np.std(x.astype(f64)))
    assert abs(float(mu[0, 0]) - mean) <= H / 2 + 2.0 ** -24 * abs(mean) + 2.0 ** -50 * abs(mean), name
    assert std > H, name
    rel64 = 2.0 ** -51 * ((mean / H) ** 2 + (std / H) ** 2) / ((std - H / 2) / H) ** 2 / 2
    lo, hi = 1.0 / (std + H / 2), 1.0 / (std - H / 2)
    slack = 3 * 2.0 ** -24 + rel64
    assert lo * (1 - slack) <= float(inv[0, 0]) <= hi * (1 + slack), (name, float(inv[0, 0]), 1 / std)


# ------------------------------------------------------------------------------------------------------ the model's invariants
def _rows(rng, n, Dn):
    x = (rng.standard_normal((n, Dn)) * rng.choice([0.01, 1.0, 300.0, 5000.0], Dn)).astype(f32)
    x[rng.integers(n), rng.integers(Dn)] = nan
    x[rng.integers(n), rng.integers(Dn)] = -inf
    return x


def test_split_calls_equal_one_call():
    rng = np.random.default_rng(1)
    Dn, S, n = 14, 5, 23
    x, mask = _rows(rng, n, Dn), (rng.random(n) < 0.8).astype(np.uint8)
    one = OM.accumulate(OM.State(5, Dn), x, S, mask)
    two = OM.State(5, Dn)
    # the second call's rows are rows 10 .. of the same population: block = r // S of the WHOLE row number
    OM.accumulate(two, np.concatenate([x[:10], np.full((n - 10, Dn), nan, f32)]), S, mask)
    OM.accumulate(two, np.concatenate([np.full((10, Dn), nan, f32), x[10:]]), S, mask)
    for a, b in zip(one.words(), two.words()):
        assert np.array_equal(a, b)
    assert int(one.count.sum()) == int(OM.contributes(x, mask).sum()) < n


def test_bounds_at_the_clamp():
    """|q| <= 2^23 whatever the word; at the lifetime capacity of 2^39 rows no sum passes 2^62, in exact integers"""
    x = np.array([[2048.0, -2048.0, 1e30, -1e30, 2048.0 - H, 3.4e38]], f32)       # (2048 - 2^-13, the last float below, is a tie: up)
    q = OM.quantise(x)[0]
    assert q.tolist() == [1 << 23, -(1 << 23), 1 << 23, -(1 << 23), (1 << 23) - 1, 1 << 23]
    st = OM.accumulate(OM.State(1, 6, exact=True), x, 1)
    n = OM.CAPACITY
    for a in (st.s1, st.s2hi, st.s2lo):
        assert all(abs(int(v)) * n <= 1 << 62 for v in a[0])
    assert int(st.s2hi[0, 0]) == 1 << 23 and int(st.s2lo[0, 0]) == 0 and int(st.s2lo[0, 4]) < 1 << 23
    # rint ties go to even, -0 and the subnormals give 0
    t = np.array([[0.5 * H, 1.5 * H, 2.5 * H, -0.5 * H, -1.5 * H, -0.0, 1e-40, -1e-45]], f32)
    assert OM.quantise(t)[0].tolist() == [0, 2, 2, 0, -2, 0, 0, 0]


def test_empty_blocks_constants_and_a_negative_variance():
    Dn = 3
    st = OM.State(2, Dn)
    mu, inv = OM.freeze(*st.words(), min_count=1, min_var=2.0 ** -20)           # n = 0 < min_count: the identity
    assert np.array_equal(OM.tbits(mu), OM.tbits(np.zeros((2, Dn), f32))) and np.array_equal(OM.tbits(inv), OM.tbits(np.ones((2, Dn), f32)))
    x = np.tile(np.array([[7.0, -1234.56, 0.0]], f32), (50, 1))
    OM.accumulate(st, x, 50)
    mu, inv = OM.freeze(*st.words(), min_count=50, min_var=2.0 ** -20)
    assert np.array_equal(inv[0], np.zeros(Dn, f32)) and np.array_equal(inv[1], np.ones(Dn, f32))
    assert np.allclose(mu[0], x[0], atol=H, rtol=0) and np.array_equal(mu[1], np.zeros(Dn, f32))
    mu, inv = OM.freeze(*st.words(), min_count=51, min_var=2.0 ** -20)           # one row short
    assert np.array_equal(inv, np.ones((2, Dn), f32))
    # a constant word over so many rows that s1 and s2 round on their way to binary64: for these (q, n) -- found by a search, each a
    # state that n rows of one value leave -- the difference s2 - m m comes out NEGATIVE, and is cut to 0
    for q, n in ((3941643, 19501544874), (6957222, 377218338355), (8247938, 357969085319), ((1 << 23) - 1, (1 << 39) - 7)):
        p = q * q
        words = (np.array([n]), np.array([[n * q]]), np.array([[n * (p >> 23)]]), np.array([[n * (p & OM.LOW)]]))
        _, v = OM.moments(n, words[1][0], words[2][0], words[3][0])
        assert v[0] < 0 or q == (1 << 23) - 1, (q, n, v)
        mu, inv = OM.freeze(*words, min_count=1, min_var=2.0 ** -20)
        assert float(inv[0, 0]) == 0.0 and abs(float(mu[0, 0]) - q * H) <= 2.0 ** -24 * 2048
    # and a forged state whose s2 is below m m outright
    mu, inv = OM.freeze(np.array([1]), np.array([[5]]), np.array([[0]]), np.array([[24]]), min_count=1, min_var=2.0 ** -20)
    assert float(inv[0, 0]) == 0.0 and float(mu[0, 0]) == 5 * H


def test_apply_is_two_roundings_and_a_clip():
    x = np.array([[1.0, 3.0, -100.0, nan, inf, -inf, inf, -0.0]], f32)
    mu = np.array([[0.25, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]], f32)
    inv = np.array([[3.0, 0.0, 1.0, 1.0, 0.0, 2.0, 1.0, 1.0]], f32)
    got = OM.apply(x, mu, inv, 5.0, 1)[0]
    assert got[:3].tolist() == [2.25, 0.0, -5.0] and np.isnan(got[3]) and np.isnan(got[4])          # inf * 0 is a NaN
    assert got[5:7].tolist() == [-5.0, 5.0] and OM.tbits(got[7:])[0] == 0x80000000                  # -0 - 0 = -0, times 1
    free = OM.apply(x, np.zeros_like(mu), np.ones_like(inv), inf, 1)
    same = ~np.isnan(x)
    assert np.array_equal(OM.tbits(free)[same], OM.tbits(x)[same])                                 # the identity, bit for bit


# ---------------------------------------------------------------------------------------- header, binding and the libraries
EXPORTS = ["rem2d_obsnorm_abi_version", "rem2d_obsnorm_accumulate", "rem2d_obsnorm_freeze", "rem2d_obsnorm_forward",
           "rem2d_obsnorm_forward_memory", "rem2d_worlds_act_normed"]


def test_header_binding_and_libraries_agree():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib, policy
    with open(os.path.join(ROOT, "include", "rem2d_obsnorm.h")) as f:
        text = f.read()
    declared = re.findall(r"^\s*(?:int|int64_t)\s+(rem2d_\w+)\s*\(", text, flags=re.M)
    assert declared == EXPORTS
    assert not re.search(r"\bvoid\s*\*\s*stream\b[^;]*\)\s*;", text)                          # the stream is a member, not a parameter
    assert int(re.search(r"#define REM2D_OBSNORM_ABI_VERSION (\d+)", text).group(1)) == _lib.OBSNORM_ABI_VERSION == 1
    assert int(re.search(r"#define REM2D_OBSNORM_MAX_CHUNK (\d+)", text).group(1)) == _lib.OBSNORM_MAX_CHUNK
    assert int(re.search(r"#define REM2D_OBSNORM_CAPACITY_LOG2 (\d+)", text).group(1)) == _lib.OBSNORM_CAPACITY_LOG2 == 39
    assert policy.ObsNormalizer.CAPACITY == OM.CAPACITY == 1 << 39
    body = re.search(r"typedef struct rem2d_obsnorm \{(.*?)\} rem2d_obsnorm;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = re.findall(r"^\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+);", body, flags=re.M)
    assert [m[2] for m in members] == [n for n, _ in _lib.Obsnorm._fields_], members
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
    for (tname, star, name), (_, ct) in zip(members, _lib.Obsnorm._fields_):
        assert ct is (C.c_void_p if star else ctype[tname]), name
    assert C.sizeof(_lib.Obsnorm) == 6 * 4 + 2 * 4 + 2 * 8 + 11 * 8 + 8 + 8 and _lib.Obsnorm.min_count.offset == 32
    assert _lib.Obsnorm.stream.offset == C.sizeof(_lib.Obsnorm) - 8
    for path in (_lib.LIB_PATH, _lib.WIDE_LIB_PATH, _lib.FMA_LIB_PATH):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert sorted(re.findall(r" T (rem2d_\w*(?:obsnorm|normed)\w*)", syms)) == sorted(EXPORTS), path
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        assert L.rem2d_obsnorm_abi_version() == _lib.OBSNORM_ABI_VERSION
        assert L.rem2d_abi_version() == 11 and L.rem2d_policy_abi_version() == 1 and L.rem2d_recurrent_abi_version() == 1
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):                         # the older headers know nothing of it
        if header == "rem2d_obsnorm.h":
            continue
        with open(os.path.join(ROOT, "include", header)) as f:
            other = f.read()
        for name in declared + ["REM2D_OBSNORM_", "rem2d_obsnorm"]:
            assert name not in other, (header, name)
    with open(os.path.join(ROOT, "__graft_entry__.py")) as f:
        entry = f.read()
    assert all('"%s"' % name in entry for name in declared)


# ----------------------------------------------------------------------------------------------------------- the refusals
POINTERS = ("obs", "frac", "row_mask", "count", "s1", "s2hi", "s2lo", "mu", "inv", "memory", "reset")
AT = {k: (i + 1) << 26 for i, k in enumerate(POINTERS)}      # the "device pointers", 64 MB apart
PAT = {k: (i + 20) << 26 for i, k in enumerate(("w1", "b1", "w2", "b2", "index", "row_mask", "obs", "frac", "targets", "valid"))}
MB_, R_, H_, M_, S_, K_ = 16, 10, 32, 4, 16, 8


def _norm(**kw):
    """a good descriptor: 4 blocks of 16 rows of the workload's row; the pointers are never dereferenced: the checks come first"""
    from gym_rem2d_amd import _lib
    n = _lib.Obsnorm()
    n.max_bodies, n.n_rays, n.n_blocks, n.group_size, n.row_chunk, n.context = MB_, R_, M_, S_, 0, 0
    n.clip, n.min_var, n.min_count, n.n_rows, n.reserved, n.stream = 5.0, 2.0 ** -20, 16, M_ * S_ - 3, 0, None
    for k in POINTERS:
        setattr(n, k, AT[k])
    for k, v in kw.items():
        setattr(n, k, v)
    return n


def _pol(context=0, **kw):
    from gym_rem2d_amd import _lib
    p = _lib.Policy()
    p.d, p.max_bodies, p.n_rays, p.hidden, p.activation, p.scale = 8 + 6 * MB_ + R_ + context, MB_, R_, H_, 0, 1.5
    p.n_sets, p.reserved, p.n_rows = M_ * S_, 0, M_ * S_
    for k, v in PAT.items():
        setattr(p, k, v)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


SHAPES = [(dict(max_bodies=0), b"max_bodies must be 1..64"), (dict(max_bodies=65), b"max_bodies must be 1..64"), (dict(n_rays=-1), b"n_rays must be 0..64"),
          (dict(n_rays=65), b"n_rays must be 0..64"), (dict(n_blocks=0), b"n_blocks must be at least 1"), (dict(group_size=0), b"group_size must be at least 1"),
          (dict(n_blocks=2 ** 16, group_size=2 ** 15), b"n_blocks * group_size must be at most 2^31 - 1"),
          (dict(n_blocks=2 ** 25, group_size=1), b"n_blocks times the words of a row must be at most 2^31 - 1"),
          (dict(row_chunk=-1), b"row_chunk must be 0..65536"), (dict(row_chunk=65537), b"row_chunk must be 0..65536"), (dict(reserved=1), b"reserved must be 0")]
STATE = ([(dict(**{k: None}), ("NULL device pointer (%s)" % k).encode()) for k in ("count", "s1", "s2hi", "s2lo")]
         + [(dict(**{k: AT[k] + 4}), ("%s must be 8-byte aligned" % k).encode()) for k in ("count", "s1", "s2hi", "s2lo")])
TABLES = [(dict(mu=None), b"NULL device pointer (mu)"), (dict(inv=None), b"NULL device pointer (inv)")]
ACCUMULATE = SHAPES + STATE + [(dict(n_rows=-1), b"negative row count"), (dict(n_rows=M_ * S_ + 1), b"65 rows are more than n_blocks * group_size = 64"),
                               (dict(obs=None), b"NULL device pointer (obs)"), (dict(frac=None), b"NULL device pointer (frac)")]
FREEZE = SHAPES + STATE + TABLES + [(dict(min_count=0), b"min_count must be at least 1"), (dict(min_var=0.0), b"min_var must be positive and finite"),
                                    (dict(min_var=inf), b"min_var must be positive and finite"), (dict(min_var=nan), b"min_var must be positive and finite")]
APPLY = SHAPES + TABLES + [(dict(clip=0.0), b"clip must be greater than 0"), (dict(clip=-1.0), b"clip must be greater than 0"), (dict(clip=nan), b"clip must be greater than 0"),
                           (dict(context=-1), b"context must be at least 0")]


def test_bad_arguments_are_refused_before_anything_is_dereferenced():
    """Every REM2D_E_INVALID of include/rem2d_obsnorm.h, in the three builds, on a machine without a GPU: nothing is launched"""
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        err = L.rem2d_last_error
        for fn, prefix, cases in ((L.rem2d_obsnorm_accumulate, b"obsnorm_accumulate: ", ACCUMULATE), (L.rem2d_obsnorm_freeze, b"obsnorm_freeze: ", FREEZE)):
            assert fn(None) == -1 and err() == prefix + b"NULL descriptor"
            for kw, msg in cases:
                assert fn(C.byref(_norm(**kw))) == -1 and msg in err() and err().startswith(prefix), (prefix, kw, err())
        # what a call does not look at may be anything
        assert L.rem2d_obsnorm_accumulate(C.byref(_norm(n_rays=0, frac=None, n_rows=2 ** 40))) == -1 and b"rows are more than" in err()
        assert L.rem2d_obsnorm_freeze(C.byref(_norm(n_rows=-5, obs=None, clip=nan, context=-3, min_count=0))) == -1 and b"min_count" in err()
        fwd, mem, act = L.rem2d_obsnorm_forward, L.rem2d_obsnorm_forward_memory, L.rem2d_worlds_act_normed
        worlds = (C.c_void_p * 1)(None)
        calls = ((lambda n, p: fwd(n, p), b"obsnorm_forward: ", 0), (lambda n, p: mem(n, p), b"obsnorm_forward_memory: ", K_),
                 (lambda n, p: act(worlds, 1, n, p, C.c_void_p(8), 1), b"act_normed: ", 0), (lambda n, p: act(worlds, 1, n, p, C.c_void_p(8), 0), b"act_normed: ", K_))
        for call, prefix, K in calls:
            good = dict(context=K)
            assert call(None, C.byref(_pol(K))) == -1 and err() == prefix + b"NULL descriptor"
            assert call(C.byref(_norm(**good)), None) == -1 and err() == prefix + b"NULL policy"
            for kw, msg in APPLY:
                if "context" in kw and prefix == b"obsnorm_forward_memory: ":
                    continue
                assert call(C.byref(_norm(**dict(good, **kw))), C.byref(_pol(K))) == -1 and msg in err() and err().startswith(prefix), (prefix, kw, err())
            for n_kw, p_kw, msg in ((dict(max_bodies=15), {}, b"the policy has max_bodies 16 and n_rays 10, the normaliser 15 and 10"),
                                    (dict(n_rays=9), {}, b"the policy has max_bodies 16 and n_rays 10, the normaliser 16 and 9"),
                                    (dict(n_blocks=3), {}, b"64 rows are more than n_blocks * group_size = 48"),
                                    ({}, dict(hidden=129), b"hidden must be 1..128"), ({}, dict(d=7), b"d must be 8 + 6 max_bodies + n_rays"),
                                    ({}, dict(targets=None), b"NULL device pointer"), ({}, dict(n_rows=-1), b"negative row count"),
                                    ({}, dict(index=None, n_sets=5), b"without an index n_sets must be n_rows")):
                assert call(C.byref(_norm(**dict(good, **n_kw))), C.byref(_pol(K, **p_kw))) == -1 and msg in err() and err().startswith(prefix), (prefix, n_kw, p_kw, err())
        # the two passes want the context they are made for; with memory, the rules of the header of policies with memory
        assert fwd(C.byref(_norm(context=1)), C.byref(_pol(0))) == -1 and b"context must be 0 for a feed-forward policy" in err()
        assert mem(C.byref(_norm(context=0)), C.byref(_pol(0))) == -1 and b"context must be 1..hidden" in err()
        assert mem(C.byref(_norm(context=H_ + 1)), C.byref(_pol(H_ + 1))) == -1 and b"context must be 1..hidden" in err()
        assert mem(C.byref(_norm(context=K_, memory=None)), C.byref(_pol(K_))) == -1 and b"NULL device pointer (memory)" in err()
        assert mem(C.byref(_norm(context=K_)), C.byref(_pol(K_ - 1))) == -1 and b"d must be 8 + 6 max_bodies + n_rays + context" in err()
        # act: the accumulation's refusals only when it accumulates, then rem2d_worlds_act's own, before any world is looked at twice
        n = _norm(count=None)
        assert act(worlds, 1, C.byref(n), C.byref(_pol()), C.c_void_p(8), 1) == -1 and err() == b"act_normed: NULL device pointer (count)"
        assert act(worlds, 1, C.byref(n), C.byref(_pol()), C.c_void_p(8), 0) == -1 and err() == b"act_normed: world 0 is NULL"
        assert act(None, 1, C.byref(_norm()), C.byref(_pol()), C.c_void_p(8), 0) == -1 and err() == b"act_normed: no worlds"
        assert act(worlds, 1, C.byref(_norm()), C.byref(_pol()), None, 0) == -1 and err() == b"act_normed: NULL device pointer (ray offsets)"


# --------------------------------------------------------------------------------------------------------- the Python layer
def test_python_layer_errors_capacity_and_checkpoints():
    import torch
    from gym_rem2d_amd import policy
    N = policy.ObsNormalizer
    for kw, msg in ((dict(n_blocks=0), "n_blocks and group_size"), (dict(group_size=0), "n_blocks and group_size"), (dict(max_bodies=65), "max_bodies must be"),
                    (dict(n_rays=65), "max_bodies must be"), (dict(clip=0.0), "clip must be"), (dict(clip=nan), "clip must be"), (dict(min_count=0), "min_count must be"),
                    (dict(min_count=2.5), "min_count must be"), (dict(min_var=0.0), "min_var must be"), (dict(min_var=inf), "min_var must be")):
        with pytest.raises(ValueError, match=msg):
            N(**dict(dict(n_blocks=2, group_size=3, max_bodies=2, n_rays=1, device="cpu"), **kw))
    nz = N(2, 3, 2, 1, device="cpu")
    assert nz.width == 21 and nz.min_count == 3 and nz.clip == 5.0 and nz.min_var == 2.0 ** -20 and nz.offered == 0
    assert N(2, 1, 2, 1, device="cpu").min_count == 2 and N(2, 3, 2, 1, clip=inf, device="cpu").clip == inf
    mu, inv = nz.tables
    assert mu.shape == inv.shape == (2, 21) and not mu.any() and bool((inv == 1).all())
    obs, frac = torch.zeros((5, 20)), torch.zeros((5, 1))
    for args, msg in (((torch.zeros((5, 19)), frac), "obs must be"), ((obs.double(), frac), "obs must be"), ((obs, None), "frac must be"),
                      ((obs, torch.zeros((4, 1))), "frac must be"), ((obs, frac, torch.zeros(5)), "row_mask must be"),
                      ((torch.zeros((7, 20)), torch.zeros((7, 1))), "7 rows are more than n_blocks \\* group_size = 6")):
        with pytest.raises(ValueError, match=msg):
            nz.accumulate(*args)
    with pytest.raises(ValueError, match="row_chunk must be"):
        nz.accumulate(obs, frac, row_chunk=65537)
    with pytest.raises(ValueError, match="the normaliser is on cpu"):          # everything else was fine: only now the device
        nz.accumulate(obs, frac)
    assert nz.offered == 0
    # the capacity: an upper bound of what one block can have been given, counted per call, checked BEFORE the call
    nz.offered = N.CAPACITY - 2                                               # 5 rows can give one block min(5, group_size 3) = 3 more
    with pytest.raises(OverflowError, match="2\\^39"):
        nz.accumulate(obs, frac)
    assert nz.offered == N.CAPACITY - 2
    nz.offered = N.CAPACITY - 3
    with pytest.raises(ValueError, match="the normaliser is on cpu"):          # exactly at the capacity is allowed
        nz.accumulate(obs[:3], frac[:3])
    # checkpoints
    rng = np.random.default_rng(0)
    nz.count.copy_(torch.tensor([5, 1 << 38]))
    nz.s1.copy_(torch.from_numpy(rng.integers(-2 ** 61, 2 ** 61, (2, 21))))
    nz.s2hi.copy_(torch.from_numpy(rng.integers(0, 2 ** 61, (2, 21))))
    nz.mu.copy_(torch.from_numpy(rng.standard_normal((2, 21)).astype(f32)))
    saved = nz.state()
    other = N(2, 3, 2, 1, device="cpu")
    other.load_state(saved)
    for k in ("count", "s1", "s2hi", "s2lo", "mu", "inv"):
        assert torch.equal(getattr(other, k), getattr(nz, k)) and saved[k].data_ptr() != getattr(nz, k).data_ptr(), k
    assert other.offered == nz.offered == N.CAPACITY - 3
    nz.reset()
    assert nz.offered == 0 and not nz.count.any() and not nz.s1.any() and not nz.mu.any() and bool((nz.inv == 1).all())
    assert int(other.count[1]) == 1 << 38                                      # (a state is a copy)
    for bad, msg in (({}, "state must be a dict"), (dict(saved, offered=-1), "offered must be"), (dict(saved, offered=True), "offered must be"),
                     (dict(saved, s1=saved["s1"][:, :20]), "s1 must be"), (dict(saved, mu=saved["mu"].double()), "mu must be")):
        with pytest.raises(ValueError, match=msg):
            other.load_state(bad)
    # set_policy's and forward's checks of the pair
    pol = policy.MLPPolicy.random(6, 2, 4, n_rays=1, rays=np.zeros((1, 2)) + 1.0)
    for norm, msg in ((N(2, 3, 3, 1, device="cpu"), "the policy has max_bodies 2 and 1 rays, the normaliser 3 and 1"), (N(1, 3, 2, 1, device="cpu"), "6 rows are more than")):
        with pytest.raises(ValueError, match=msg):
            norm.forward(pol, torch.zeros((6, 20)), torch.zeros((6, 1)))
    with pytest.raises(ValueError, match="the normaliser is on cpu"):
        N(2, 3, 2, 1, device="cpu").forward(pol, torch.zeros((6, 20)), torch.zeros((6, 1)))
