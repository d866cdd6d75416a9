"""Device policies without a GPU (include/rem2d_policy.h): the host model has teeth, the closed loop under it matters on the oracle
alone, and the header, the ctypes binding, policy.py and the three libraries agree; the argument checks of both entry points and the
shape and value errors of MLPPolicy / set_policy.

The GPU half (tests/test_policy_gpu.py) compares the kernel with tests/policy_model.py bit for bit and the closed loop with the
oracle runs made here; this half makes sure that neither is a vacuous yardstick."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import control_model as M
import policy_model as PM
import state_forge as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
CONT = 1
LOOP_POPULATIONS = ("lsystem", "cppn", "direct", "chain8")


def _fma(a, b, c):
    """fl32(a * b + c) with ONE rounding: the product of two binary32 numbers is exact in binary64, and the binary64 sum that follows
    is rounded to 53 bits before it is rounded to 24 -- a double rounding that differs from the single one only when the binary64
    sum lands exactly on a binary32 tie, which random data does not do; enough to show what a contracting kernel would compute."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _hidden_variants(x, w1, b1):
    """the hidden pre-activation of the model's order, and of three ways a kernel could go wrong"""
    seq = b1.copy()
    for i in range(x.shape[1]):
        seq = seq + (x[:, i, None] * w1[:, i, :])
    rev = b1.copy()
    for i in reversed(range(x.shape[1])):
        rev = rev + (x[:, i, None] * w1[:, i, :])
    ein = (np.einsum("ni,nij->nj", x, w1) + b1).astype(f32)
    fused = b1.copy()
    for i in range(x.shape[1]):
        fused = _fma(np.broadcast_to(x[:, i, None], fused.shape), w1[:, i, :], fused)
    return seq, rev, ein, fused


@pytest.mark.parametrize("D,H", [(35, 5), (114, 32)])
def test_the_model_has_teeth(D, H):
    """On the forge shapes (MB 4, R 3, H 5 and MB 16, R 10, H 32) the sequential sum differs from the reversed order, from einsum and
    from a fused multiply-add in many output words: a kernel that reorders or contracts cannot pass by luck."""
    rng = np.random.default_rng([D, H])
    N = 64
    x = rng.standard_normal((N, D)).astype(f32)
    w1, b1 = (rng.standard_normal((N, D, H)) * 0.3).astype(f32), (rng.standard_normal((N, H)) * 0.3).astype(f32)
    seq, rev, ein, fused = _hidden_variants(x, w1, b1)
    assert seq.dtype == f32
    share = {k: float((v.view(np.uint32) != seq.view(np.uint32)).mean()) for k, v in (("reversed", rev), ("einsum", ein), ("fused", fused))}
    print(D, H, share)
    assert all(s >= 0.25 for s in share.values()), share
    # ... and the model's own hidden layer is that sequential sum
    h = PM.hidden_model(x, w1, b1, PM.SOFTSIGN)
    assert np.array_equal(h.view(np.uint32), (seq / (f32(1.0) + np.abs(seq))).view(np.uint32))
    # numpy's binary32 quotient is the correctly rounded one: the binary64 quotient of two binary32 numbers rounds to it
    q64 = (seq.astype(np.float64) / (1.0 + np.abs(seq).astype(np.float64))).astype(f32)
    den = f32(1.0) + np.abs(seq)
    assert np.array_equal((seq / den).view(np.uint32), (seq.astype(np.float64) / den.astype(np.float64)).astype(f32).view(np.uint32))
    assert np.abs(q64 - h).max() < 1e-6


def test_model_edge_values():
    """relu sends NaN and -0 to +0; a non-finite target is invalid; skipped rows are named by rows_run"""
    x = np.array([[np.nan], [-0.0], [2.0], [-3.0]], f32)
    w1, b1 = np.ones((4, 1, 1), f32), np.zeros((4, 1), f32)
    b1[1] = -0.0
    h = PM.hidden_model(x, w1, b1, PM.RELU)
    assert np.array_equal(h.view(np.uint32).ravel(), np.array([0.0, 0.0, 2.0, 0.0], f32).view(np.uint32))
    hs = PM.hidden_model(x, w1, b1, PM.SOFTSIGN)
    assert np.isnan(hs[0, 0]) and np.signbit(hs[1, 0]) and hs[2, 0] == f32(2.0) / f32(3.0)
    # MB = 1, R = 0: D = 14
    xr = np.zeros((3, 14), f32)
    xr[:, 0] = (1.0, np.inf, 1e30)
    W = (np.ones((1, 14, 1), f32), np.zeros((1, 1), f32), np.ones((1, 1, 1), f32), np.zeros((1, 1), f32))
    t, valid = PM.forward_model(xr, *W, act=PM.RELU, index=[0, 0, 0])
    assert valid.ravel().tolist() == [1, 0, 1] and np.isnan(t[1, 0])          # inf / (1 + inf)
    assert t[0, 0] == float(PM.DEFAULT_SCALE * (f32(1.0) / f32(2.0))) and t[2, 0] == float(PM.DEFAULT_SCALE)
    assert PM.rows_run(4, 2, [0, 1, 2, -1], [1, 0, 1, 1]).tolist() == [True, False, False, False]
    assert np.array_equal(PM.bits(np.array([np.nan, -np.nan, 1.0]))[:2], PM.bits(np.array([np.nan, np.nan])))


@pytest.mark.parametrize("pop", LOOP_POPULATIONS)
def test_the_policy_loop_matters(oracle, pop):
    """The GPU tests' closed loop, on the oracle alone: 120 steps of continuous physics under per-creature policies (MB 16,
    BipedalWalker's 10 rays, H 32, softsign).  All state stays finite (policy_loop_run asserts it), at most LEFT_OUT_CAP of the
    creatures outgrow the default build's 24 pair / 6 solver slots, at least 90 % end at another root x than under their own
    oscillators, and the targets are not saturated."""
    terrain, morphs = M.loop_population(pop)
    runs = PM.policy_loop_run(oracle, pop, CONT)
    ot = F.oracle_terrain(oracle, terrain)
    moved = total = gone = 0
    mags = []
    for morph, run in zip(morphs, runs):
        open_loop = oracle.batch_run(ot, morph.as_dict(), PM.N_POLICY_LOOP, n_threads=2, flags=CONT)["bodies"][:, 0, 0]
        moved += int((run["root_x"] != open_loop).sum())
        total += run["ctx"].N
        gone += int((M.left_out_first(run)[0] < len(run["obs"])).sum())
        assert all(v.all() for v in run["valid"])                      # finite state, finite weights: every target is valid
        mags.append(np.abs(np.stack(run["targets"])).mean())
        assert np.ptp(np.stack(run["frac"])) > 0.05                    # the rays see something that changes
    print(pop, "moved %d of %d, left out %d, mean |target| %.3f" % (moved, total, gone, float(np.mean(mags))))
    assert moved >= 0.9 * total, "%s: only %d of %d creatures end elsewhere" % (pop, moved, total)
    assert gone <= int(F.LEFT_OUT_CAP * total), "%s: %d of %d creatures outgrow the default slots" % (pop, gone, total)
    assert 0.2 < float(np.mean(mags)) < 1.4                            # of a possible 1.57: neither dead nor saturated


def test_cppn_has_a_bucket_wider_than_the_policy():
    """The cppn loop population has a 32-lane bucket: with MB = 16 its joints 16 .. stay under their oscillators"""
    _, morphs = M.loop_population("cppn")
    assert max(m.lanes for m in morphs) == 32 > PM.LOOP_BODIES
    wide = [m for m in morphs if m.lanes == 32][0]
    assert ((wide.arrays["shape"].reshape(wide.n_envs, 32) != 0).sum(axis=1) > PM.LOOP_BODIES).any()


def test_header_binding_and_libraries_agree():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib, control, policy, sense
    with open(os.path.join(ROOT, "include", "rem2d_policy.h")) as f:
        text = f.read()
    declared = re.findall(r"^\s*int\s+(rem2d_\w+)\s*\(", text, flags=re.M)
    assert set(declared) == {"rem2d_policy_abi_version", "rem2d_policy_forward", "rem2d_worlds_act"}
    for name, value in (("REM2D_POLICY_ABI_VERSION", _lib.POLICY_ABI_VERSION), ("REM2D_POLICY_MAX_HIDDEN", policy.MAX_HIDDEN),
                        ("REM2D_POLICY_SOFTSIGN", policy.ACTIVATIONS.index("softsign")),
                        ("REM2D_POLICY_RELU", policy.ACTIVATIONS.index("relu"))):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value, name
    assert (policy.ABI_VERSION, policy.MAX_HIDDEN, policy.ACTIVATIONS) == (1, 128, (PM.SOFTSIGN, PM.RELU))
    assert policy.DEFAULT_SCALE == float(PM.DEFAULT_SCALE) and policy.input_width(16, 10) == M.width(16) + 10 == 114
    # the struct: the header's members in the header's order
    body = re.search(r"typedef struct rem2d_policy \{(.*?)\} rem2d_policy;", text, flags=re.S).group(1)
    members = re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(\w+);", body, flags=re.M)
    assert members == [n for n, _ in _lib.Policy._fields_], members
    assert C.sizeof(_lib.Policy) == 8 * 4 + 10 * 8 + 8
    for path in (_lib.LIB_PATH, _lib.WIDE_LIB_PATH, _lib.FMA_LIB_PATH):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for name in declared:
            assert (" T " + name) in syms, (path, name)
    for wide in (False, True, "fma"):
        assert _lib.lib(wide).rem2d_policy_abi_version() == _lib.POLICY_ABI_VERSION
    # the pinned headers know nothing of it
    for header in ("rem2d.h", "rem2d_control.h", "rem2d_sense.h"):
        with open(os.path.join(ROOT, "include", header)) as f:
            other = f.read()
        for name in declared + ["REM2D_POLICY_", "rem2d_policy"]:
            assert name not in other, (header, name)
    assert (control.MAX_BODIES, sense.MAX_RAYS) == (64, 64)


def _desc(**kw):
    from gym_rem2d_amd import _lib
    p = _lib.Policy()
    p.d, p.max_bodies, p.n_rays, p.hidden, p.activation, p.scale, p.n_sets, p.reserved = 114, 16, 10, 32, 0, 1.5, 3, 0
    for k in ("w1", "b1", "w2", "b2", "obs", "frac", "targets", "valid"):
        setattr(p, k, 256)                       # "device pointers" that are never dereferenced: the checks come first
    p.index, p.row_mask, p.n_rows = None, None, 3
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD_POLICIES = [(dict(max_bodies=0, d=18), b"max_bodies"), (dict(max_bodies=65, d=408), b"max_bodies"), (dict(n_rays=-1, d=103), b"n_rays"),
                (dict(n_rays=65, d=169), b"n_rays"), (dict(hidden=0), b"hidden"), (dict(hidden=129), b"hidden"), (dict(d=113), b"d must be"),
                (dict(d=104), b"d must be"), (dict(activation=2), b"activation"), (dict(activation=-1), b"activation"),
                (dict(n_sets=0), b"n_sets"), (dict(n_sets=-4), b"n_sets"), (dict(n_rows=-1), b"row count"),
                (dict(w1=None), b"NULL device pointer"), (dict(b1=None), b"NULL device pointer"), (dict(w2=None), b"NULL device pointer"),
                (dict(b2=None), b"NULL device pointer"), (dict(obs=None), b"NULL device pointer"), (dict(frac=None), b"NULL device pointer"),
                (dict(targets=None), b"NULL device pointer"), (dict(valid=None), b"NULL device pointer"),
                (dict(n_sets=2), b"without an index"), (dict(n_rows=4), b"without an index")]


def test_bad_arguments_are_refused_before_anything_is_dereferenced():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        err = L.rem2d_last_error
        fake = (C.c_void_p * 1)(C.c_void_p(8))    # a "world" that is never dereferenced
        null = (C.c_void_p * 1)(None)
        two = (C.c_void_p * 2)(C.c_void_p(8), None)
        buf = C.c_void_p(256)
        assert L.rem2d_policy_forward(None, None) == -1 and b"NULL policy" in err()
        assert L.rem2d_worlds_act(fake, 1, None, buf, None) == -1 and b"NULL policy" in err()
        for kw, msg in BAD_POLICIES:
            p = _desc(**kw)
            assert L.rem2d_policy_forward(C.byref(p), None) == -1 and msg in err() and err().startswith(b"policy: "), (kw, err())
            assert L.rem2d_worlds_act(fake, 1, C.byref(p), buf, None) == -1 and msg in err() and err().startswith(b"act: "), (kw, err())
        good = _desc()
        assert L.rem2d_worlds_act(None, 1, C.byref(good), buf, None) == -1 and b"no worlds" in err()
        assert L.rem2d_worlds_act(fake, 0, C.byref(good), buf, None) == -1 and b"no worlds" in err()
        assert L.rem2d_worlds_act(fake, -2, C.byref(good), buf, None) == -1 and b"no worlds" in err()
        assert L.rem2d_worlds_act(fake, 1, C.byref(good), None, None) == -1 and b"ray offsets" in err()
        assert L.rem2d_worlds_act(null, 1, C.byref(good), buf, None) == -1 and b"world 0 is NULL" in err()
        assert L.rem2d_worlds_act(two, 2, C.byref(good), buf, None) == -1 and b"world 1 is NULL" in err()    # before world 0 is looked at
        # what is allowed to be NULL: frac and the ray offsets without rays, index with one set per row, the row mask -- checked on
        # an empty population, which launches nothing
        empty = _desc(n_rays=0, d=104, frac=None, n_rows=0, n_sets=1, index=256)
        assert L.rem2d_policy_forward(C.byref(empty), None) == 0


def test_mlp_policy_shapes_and_values():
    import torch
    from gym_rem2d_amd import policy, sense
    P = policy.MLPPolicy
    p = P.random(5, 16, 32, seed=3)
    assert (p.n_sets, p.d, p.hidden, p.max_bodies, p.n_rays) == (5, 114, 32, 16, 10) and p.activation == "softsign"
    assert p.scale == policy.DEFAULT_SCALE and np.array_equal(p.rays, sense.bipedal_rays()) and p.index is None
    assert p.weight_bytes() == 4 * (114 * 32 + 32 + 32 * 16 + 16) == 16832
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (p.w1, p.b1, p.w2, p.b2))
    # random() is the documented draw
    rng = np.random.default_rng(3)
    assert np.array_equal(p.w1.numpy(), (rng.standard_normal((5, 114, 32)) * 0.3).astype(f32))
    assert np.array_equal(p.b1.numpy(), (rng.standard_normal((5, 32)) * 0.3).astype(f32))
    assert np.array_equal(p.w2.numpy(), (rng.standard_normal((5, 32, 16)) * 0.5).astype(f32))
    # take(): selection with repeats; through an index
    q = p.take([4, 4, 0])
    assert q.n_sets == 3 and torch.equal(q.w1[1], p.w1[4]) and torch.equal(q.b2[2], p.b2[0]) and q.activation == p.activation
    shared = P(p.w1, p.b1, p.w2, p.b2, index=[0, 1, 1, 4, 2, 3, 3])
    assert shared.index.dtype == torch.int32 and torch.equal(shared.take([2, 3]).w2, p.w2[[1, 4]]) and shared.take([2, 3]).index is None
    with pytest.raises(ValueError):
        P(p.w1, p.b1, p.w2, p.b2, index=[0, 9]).take([1])
    # one set without its leading axis; no rays; other ray counts want their table
    one = P(p.w1[0], p.b1[0], p.w2[0], p.b2[0], activation="relu", scale=1.0)
    assert one.n_sets == 1 and one.activation == "relu" and one.scale == 1.0
    blind = P.random(2, 4, 5, n_rays=0)
    assert blind.n_rays == 0 and blind.rays is None and blind.d == 32
    three = P.random(2, 4, 5, n_rays=3)
    assert three.n_rays == 3 and three.d == 35 and three.rays.shape == (3, 2)
    assert p.to("cpu") is p
    z = torch.zeros
    for bad in (lambda: P(z(2, 114, 32), z(2, 31), z(2, 32, 16), z(2, 16)),                 # b1 does not fit
                lambda: P(z(2, 114, 32), z(2, 32), z(3, 32, 16), z(2, 16)),                 # another G
                lambda: P(z(2, 114, 32), z(2, 32), z(2, 32, 16), z(2, 15)),                 # b2 does not fit
                lambda: P(z(2, 103, 32), z(2, 32), z(2, 32, 16), z(2, 16)),                 # D < 8 + 6 MB
                lambda: P(z(2, 400, 32), z(2, 32), z(2, 32, 16), z(2, 16)),                 # more than 64 rays
                lambda: P(z(2, 107, 32), z(2, 32), z(2, 32, 16), z(2, 16)),                 # 3 rays and no table
                lambda: P(z(2, 107, 32), z(2, 32), z(2, 32, 16), z(2, 16), rays=np.zeros((4, 2))),
                lambda: P(z(2, 104, 32), z(2, 32), z(2, 32, 16), z(2, 16), rays=np.zeros((4, 2))),      # rays nobody reads
                lambda: P(z(2, 114, 129), z(2, 129), z(2, 129, 16), z(2, 16)),              # H > 128
                lambda: P(z(2, 8 + 6 * 65, 8), z(2, 8), z(2, 8, 65), z(2, 65)),             # 65 bodies
                lambda: P(z(0, 114, 32), z(0, 32), z(0, 32, 16), z(0, 16)),                 # no set at all
                lambda: P(z(2, 114, 32), z(2, 32), z(2, 32, 16), z(2, 16), activation="tanh"),
                lambda: P(z(2, 114, 32), z(2, 32), z(2, 32, 16), z(2, 16), index=np.zeros(2)),          # a float index
                lambda: P(z(2, 114, 32, dtype=torch.int32), z(2, 32), z(2, 32, 16), z(2, 16)),
                lambda: P(z(114, 32), z(2, 32), z(2, 32, 16), z(2, 16))):
        with pytest.raises(ValueError):
            bad()
    # the kernel alone refuses host weights, and buffers of another shape, before anything is launched
    with pytest.raises(ValueError, match="GPU"):
        p.forward(z(5, 104), z(5, 10))


def test_set_policy_checks_the_population():
    """set_policy's errors need no GPU: they come before anything is allocated"""
    from gym_rem2d_amd import policy
    from gym_rem2d_amd.env import BatchedModular2D, Modular2D
    env = BatchedModular2D()
    with pytest.raises(ValueError, match="reset first"):
        env.set_policy(policy.MLPPolicy.random(3, 16, 32))
    env.set_policy(None)
    with pytest.raises(ValueError, match="no policy"):
        env.act()
    env.worlds, env.n_envs = [(None, None)], 4          # a population of four, as far as the checks look
    with pytest.raises(ValueError, match="3 weight sets for 4"):
        env.set_policy(policy.MLPPolicy.random(3, 16, 32))
    with pytest.raises(ValueError, match="5 index entries for 4"):
        env.set_policy(policy.MLPPolicy.random(1, 16, 32, index=[0] * 5))
    env.worlds = []
    from gym_rem2d_amd import evaluate
    with pytest.raises(ValueError, match="on_error"):
        evaluate.run_policy_episode(env, on_error="fallback")
    with pytest.raises(ValueError, match="no policy"):
        evaluate.run_policy_episode(env)
    # the gym facade: one set, the env's own max_bodies, closed loop only
    one = policy.MLPPolicy.random(1, 16, 32)
    assert Modular2D(closed_loop=True, max_bodies=16, policy=one)._policy is one
    for bad in (lambda: Modular2D(policy=one), lambda: Modular2D(closed_loop=True, max_bodies=8, policy=one),
                lambda: Modular2D(closed_loop=True, max_bodies=16, policy=policy.MLPPolicy.random(2, 16, 32))):
        with pytest.raises(ValueError):
            bad()
