"""Recurrent device policies without a GPU (include/rem2d_recurrent.h): the header, the ctypes binding, policy.py and the three
libraries agree; bad descriptors are refused by name before anything is dereferenced; RecurrentPolicy checks its shapes and stays
what it is through take / to / _like; and the host model (tests/recurrent_model.py) has teeth -- a reset byte beats NaN memory, a
hand-made set oscillates by its memory alone where the feed-forward model stands still, and the oracle loop's memory is alive.

The GPU half (tests/test_recurrent_gpu.py) compares the kernel and the closed loop with this model bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import control_model as M
import policy_model as PM
import recurrent_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
CONT = 1
EXPORTS = ["rem2d_recurrent_abi_version", "rem2d_recurrent_forward", "rem2d_worlds_act_recurrent"]


def test_header_binding_and_libraries_agree():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib, policy
    with open(os.path.join(ROOT, "include", "rem2d_recurrent.h")) as f:
        text = f.read()
    declared = re.findall(r"^\s*int\s+(rem2d_\w+)\s*\(", text, flags=re.M)
    assert declared == EXPORTS
    assert int(re.search(r"#define REM2D_RECURRENT_ABI_VERSION (\d+)", text).group(1)) == _lib.RECURRENT_ABI_VERSION == 1
    assert _lib.RECURRENT_MAX_INPUTS == _lib.SENSE_MAX_RAYS == 64
    # the struct: the header's members in the header's order, a rem2d_policy first
    body = re.search(r"typedef struct rem2d_recurrent \{(.*?)\} rem2d_recurrent;", text, flags=re.S).group(1)
    members = re.findall(r"^\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+);", body, flags=re.M)
    assert [m[2] for m in members] == [n for n, _ in _lib.Recurrent._fields_] == ["p", "context", "reserved", "memory", "reset"]
    assert members[0][0] == "rem2d_policy" and _lib.Recurrent._fields_[0][1] is _lib.Policy
    for (tname, star, name), (_, ct) in list(zip(members, _lib.Recurrent._fields_))[1:]:
        assert ct is (C.c_void_p if star else {"int32_t": C.c_int32}[tname]), name
    P = C.sizeof(_lib.Policy)
    assert P == 8 * 4 + 10 * 8 + 8 and C.sizeof(_lib.Recurrent) == P + 2 * 4 + 2 * 8
    assert [getattr(_lib.Recurrent, n).offset for n, _ in _lib.Recurrent._fields_] == [0, P, P + 4, P + 8, P + 16]
    for path in (_lib.LIB_PATH, _lib.WIDE_LIB_PATH, _lib.FMA_LIB_PATH):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert sorted(re.findall(r" T (rem2d_\w*recurrent\w*)", syms)) == sorted(EXPORTS), path
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        assert L.rem2d_recurrent_abi_version() == _lib.RECURRENT_ABI_VERSION
        assert L.rem2d_abi_version() == 11 and L.rem2d_policy_abi_version() == 1       # the older versions are what they were
        assert L.rem2d_recurrent_forward.argtypes == [C.POINTER(_lib.Recurrent), C.c_void_p]
    # the older headers know nothing of it, and the CPU twin has no counterpart
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if header == "rem2d_recurrent.h":
            continue
        with open(os.path.join(ROOT, "include", header)) as f:
            other = f.read()
        for name in declared + ["REM2D_RECURRENT_", "rem2d_recurrent"]:
            assert name not in other, (header, name)
    for name in os.listdir(os.path.join(ROOT, "oracle")):
        if name.endswith((".c", ".h", ".py")):
            with open(os.path.join(ROOT, "oracle", name)) as f:
                assert "recurrent" not in f.read(), name
    with open(os.path.join(ROOT, "__graft_entry__.py")) as f:
        entry = f.read()
    assert all('"%s"' % name in entry for name in declared)
    assert issubclass(policy.RecurrentPolicy, policy.MLPPolicy)


def _desc(**kw):
    """a good descriptor: MB 16, R 10, K 8, H 32, three rows with a set each; the "device pointers" are never dereferenced"""
    from gym_rem2d_amd import _lib
    q = _lib.Recurrent()
    p = q.p
    p.d, p.max_bodies, p.n_rays, p.hidden, p.activation, p.scale, p.n_sets, p.reserved = 122, 16, 10, 32, 0, 1.5, 3, 0
    for k in ("w1", "b1", "w2", "b2", "obs", "frac", "targets", "valid"):
        setattr(p, k, 256)
    p.index, p.row_mask, p.n_rows = None, None, 3
    q.context, q.reserved, q.memory, q.reset = 8, 0, 256, None
    for k, v in kw.items():
        setattr(q if k in ("context", "reserved", "memory", "reset") else p, k, v)
    return q


# (what is wrong, the field the message must name)
BAD = [(dict(context=0, d=114), b"context"), (dict(context=-3, d=111), b"context"), (dict(context=33, d=147), b"context"),   # K = 0, K = H + 1
       (dict(n_rays=10, context=55, hidden=64, d=169), b"n_rays + context"),                                    # R + K = 65
       (dict(n_rays=64, context=1, d=169), b"n_rays + context"),
       (dict(d=121), b"d must be"), (dict(d=114), b"d must be"), (dict(d=123), b"d must be"),                   # wrong d (114: the feed-forward rule)
       (dict(memory=None), b"memory"), (dict(reserved=1), b"reserved"),
       # ... and what rem2d_policy_forward refuses
       (dict(max_bodies=0, d=26), b"max_bodies"), (dict(n_rays=-1, d=111), b"n_rays"), (dict(n_rays=65, d=177), b"n_rays"),
       (dict(hidden=0), b"hidden"), (dict(hidden=129), b"hidden"), (dict(activation=2), b"activation"), (dict(n_sets=0), b"n_sets"),
       (dict(n_rows=-1), b"row count"), (dict(w1=None), b"NULL device pointer"), (dict(obs=None), b"NULL device pointer"),
       (dict(frac=None), b"NULL device pointer"), (dict(targets=None), b"NULL device pointer"), (dict(n_sets=2), b"without an index")]


def test_bad_descriptors_are_refused_by_name():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        err = L.rem2d_last_error
        fake = (C.c_void_p * 1)(C.c_void_p(8))    # a "world" that is never dereferenced
        null = (C.c_void_p * 1)(None)
        buf = C.c_void_p(256)
        assert L.rem2d_recurrent_forward(None, None) == -1 and b"NULL recurrent policy" in err()
        assert L.rem2d_worlds_act_recurrent(fake, 1, None, buf, None) == -1 and b"NULL recurrent policy" in err()
        for kw, msg in BAD:
            q = _desc(**kw)
            assert L.rem2d_recurrent_forward(C.byref(q), None) == -1 and msg in err() and err().startswith(b"recurrent: "), (kw, err())
            assert (L.rem2d_worlds_act_recurrent(fake, 1, C.byref(q), buf, None) == -1 and msg in err()
                    and err().startswith(b"act_recurrent: ")), (kw, err())
        good = _desc()
        assert L.rem2d_worlds_act_recurrent(None, 1, C.byref(good), buf, None) == -1 and b"no worlds" in err()
        assert L.rem2d_worlds_act_recurrent(fake, 0, C.byref(good), buf, None) == -1 and b"no worlds" in err()
        assert L.rem2d_worlds_act_recurrent(fake, 1, C.byref(good), None, None) == -1 and b"ray offsets" in err()
        assert L.rem2d_worlds_act_recurrent(null, 1, C.byref(good), buf, None) == -1 and b"world 0 is NULL" in err()
        # the edges that are allowed: K = H, R + K = 64, a reset mask, no rays -- checked on an empty population, which launches nothing
        for kw in (dict(context=32, d=146), dict(n_rays=10, context=54, hidden=64, d=168), dict(reset=256),
                   dict(n_rays=0, frac=None, context=64, hidden=64, d=168)):
            q = _desc(n_rows=0, n_sets=1, index=256, **kw)
            assert L.rem2d_recurrent_forward(C.byref(q), None) == 0, (kw, err())
        # the feed-forward entry point still refuses what the operators' host tests pin: d = 169 at MB = 16
        p = _desc(n_rays=65, d=169).p
        assert L.rem2d_policy_forward(C.byref(p), None) == -1 and b"n_rays" in err()


def test_recurrent_policy_shapes_and_values():
    import torch
    from gym_rem2d_amd import policy, sense
    RP = policy.RecurrentPolicy
    p = RP.random(5, 16, 32, 8, seed=3)
    assert (p.n_sets, p.d, p.hidden, p.max_bodies, p.n_rays, p.context) == (5, 122, 32, 16, 10, 8)
    assert np.array_equal(p.rays, sense.bipedal_rays()) and p.activation == "softsign" and p.scale == policy.DEFAULT_SCALE
    # random() is MLPPolicy.random's draw at R + K rays: the same arrays
    ff = policy.MLPPolicy.random(5, 16, 32, n_rays=18, seed=3)
    assert all(torch.equal(a, b) for a, b in zip((p.w1, p.b1, p.w2, p.b2), (ff.w1, ff.b1, ff.w2, ff.b2))) and ff.n_rays == 18
    assert p.weight_bytes() == ff.weight_bytes()
    mem = p.new_memory(7)
    assert mem.dtype == torch.float32 and tuple(mem.shape) == (7, 8) and not mem.any()
    # class and K survive take / to / _like
    for q in (p.take([4, 4, 0]), p.to("cpu"), p._like(p.w1, p.b1, p.w2, p.b2, None),
              RP(p.w1, p.b1, p.w2, p.b2, 8, index=[0, 1, 1, 4]).take([2, 3])):
        assert type(q) is RP and q.context == 8 and q.n_rays == 10 and q.index is None
    assert p.take([4, 4, 0]).n_sets == 3 and torch.equal(p.take([4, 4, 0]).w1[1], p.w1[4])
    # the edges: K = H, K = 64 - R, no rays, other ray counts want their table
    assert RP.random(1, 16, 32, 32).context == 32 and RP.random(1, 64, 128, 54).d == 8 + 6 * 64 + 64
    blind = RP.random(2, 4, 5, 2, n_rays=0)
    assert blind.n_rays == 0 and blind.rays is None and blind.d == 34
    three = RP.random(2, 4, 5, 2, n_rays=3)
    assert (three.n_rays, three.d, three.context) == (3, 37, 2) and three.rays.shape == (3, 2)
    z = torch.zeros
    for bad in (lambda: RP(z(2, 122, 32), z(2, 32), z(2, 32, 16), z(2, 16), 0),                  # K = 0
                lambda: RP(z(2, 122, 32), z(2, 32), z(2, 32, 16), z(2, 16), -1),
                lambda: RP(z(2, 122, 32), z(2, 32), z(2, 32, 16), z(2, 16), 2.0),                # not an integer
                lambda: RP(z(2, 122, 32), z(2, 32), z(2, 32, 16), z(2, 16), True),
                lambda: RP(z(2, 147, 32), z(2, 32), z(2, 32, 16), z(2, 16), 33),                 # K = H + 1
                lambda: RP(z(2, 169, 64), z(2, 64), z(2, 64, 16), z(2, 16), 55),                 # R + K = 65 (R = 10)
                lambda: RP(z(2, 110, 32), z(2, 32), z(2, 32, 16), z(2, 16), 8),                  # D < 8 + 6 MB + K
                lambda: RP(z(2, 115, 32), z(2, 32), z(2, 32, 16), z(2, 16), 8),                  # 3 rays and no table
                lambda: RP(z(2, 112, 32), z(2, 32), z(2, 32, 16), z(2, 16), 8, rays=np.zeros((4, 2))),   # rays nobody reads
                lambda: RP(z(2, 122, 32), z(2, 31), z(2, 32, 16), z(2, 16), 8),                  # MLPPolicy's own checks still hold
                lambda: RP(z(2, 122, 32), z(2, 32), z(2, 32, 16), z(2, 16), 8, activation="tanh")):
        with pytest.raises(ValueError):
            bad()
    # the kernel alone refuses host weights before anything is launched
    with pytest.raises(ValueError, match="GPU"):
        p.forward(z(5, 104), z(5, 10), p.new_memory(5))
    # MLPPolicy is what it was
    m = policy.MLPPolicy.random(2, 16, 32)
    assert type(m.take([0])) is policy.MLPPolicy and not hasattr(m, "context") and m.n_rays == 10


def test_set_policy_checks_streaming():
    """the errors need no GPU: they come before anything is allocated or launched"""
    from gym_rem2d_amd import policy
    from gym_rem2d_amd.env import BatchedModular2D, Modular2D
    env = BatchedModular2D()
    assert env.policy_memory is None
    with pytest.raises(ValueError, match="reset first"):
        env.set_policy(policy.RecurrentPolicy.random(3, 16, 32, 4))
    env.worlds, env.n_envs = [(None, None)], 4          # a population of four, as far as the checks look
    env._stream_rec = object()                          # ... that streams
    with pytest.raises(ValueError, match="streamed evaluation"):
        env.set_policy(policy.RecurrentPolicy.random(4, 16, 32, 4))
    env._stream_rec = None
    with pytest.raises(ValueError, match="3 weight sets for 4"):
        env.set_policy(policy.RecurrentPolicy.random(3, 16, 32, 4))
    env._stream_rec, env._policy = object(), dict(memory=object())
    with pytest.raises(ValueError, match="RecurrentPolicy is attached"):
        env.refill()
    env.worlds, env._policy, env._stream_rec = [], None, None
    one = policy.RecurrentPolicy.random(1, 16, 32, 4)
    assert Modular2D(closed_loop=True, max_bodies=16, policy=one)._policy is one


def test_reset_beats_nan_memory():
    """In the model a reset byte over NaN memory gives the bits of zero memory; without it the NaN poisons the row; a skipped row
    keeps its memory's very bits."""
    rng = np.random.default_rng(11)
    MB, Rr, K, H, N = 4, 3, 2, 5, 6
    D = M.width(MB) + Rr + K
    x = rng.standard_normal((N, D - K)).astype(f32)
    W = ((rng.standard_normal((N, D, H)) * 0.3).astype(f32), (rng.standard_normal((N, H)) * 0.3).astype(f32),
         (rng.standard_normal((N, H, MB)) * 0.5).astype(f32), (rng.standard_normal((N, MB)) * 0.3).astype(f32))
    nan = np.full((N, K), np.nan, f32)
    zero = np.zeros((N, K), f32)
    t0, v0, m0 = RM.forward_model(x, zero, *W)
    t1, v1, m1 = RM.forward_model(x, nan, *W, reset=np.ones(N, np.uint8))
    assert np.array_equal(RM.bits(t0), RM.bits(t1)) and np.array_equal(v0, v1) and np.array_equal(m0.view(np.uint32), m1.view(np.uint32))
    assert v0.all() and np.isfinite(m0).all() and m0.any()
    some = np.array([1, 0, 1, 1, 0, 1], np.uint8)
    t2, v2, m2 = RM.forward_model(x, nan, *W, reset=some)
    assert np.array_equal(v2, np.repeat(some[:, None], MB, 1)) and np.array_equal(RM.bits(t2)[some != 0], RM.bits(t0)[some != 0])
    assert np.isnan(m2[some == 0]).all() and np.array_equal(m2[some != 0].view(np.uint32), m0[some != 0].view(np.uint32))
    # skipped rows: the memory's bits, a signalling NaN's included
    odd = zero.copy()
    odd.view(np.uint32)[:] = 0x7f800001
    _, _, m3 = RM.forward_model(x, odd, *W, row_mask=some)
    assert (m3.view(np.uint32)[some == 0] == 0x7f800001).all() and np.isnan(m3[some != 0]).all()
    # the law: the targets are the feed-forward model's on [x | c]
    c = rng.standard_normal((N, K)).astype(f32)
    t4, v4, _ = RM.forward_model(x, c, *W, act=PM.RELU)
    t5, v5 = PM.forward_model(np.concatenate([x, c], 1), *W, act=PM.RELU)
    assert np.array_equal(RM.bits(t4), RM.bits(t5)) and np.array_equal(v4, v5)


def test_memory_matters():
    """A hand-made set on a CONSTANT input row (recurrent_model.oscillator): after a 200-step run-in the target's sign changes at
    least 90 times in the next 199 transitions -- numpy binary32 gives 99, a period-4 cycle.  The feed-forward model on the same
    input is constant: trivially true, asserted for the record."""
    targets, mems = RM.oscillator_run(400)
    tail = targets[200:]
    assert len(tail) == 200 and np.isfinite(targets).all() and (tail != 0).all()
    changes = int((np.sign(tail[1:]) != np.sign(tail[:-1])).sum())
    print("sign changes in 199 transitions:", changes, "tail", tail[:8])
    assert changes >= 90
    assert np.array_equal(np.sign(tail[:-4]), np.sign(tail[4:]))        # period 4
    x, W = RM.oscillator()
    still = [PM.forward_model(np.concatenate([x, np.zeros((1, 2), f32)], 1), *W)[0][0, 0] for _ in range(3)]
    assert len(set(still)) == 1
    # from_numpy round trip: the set is a valid RecurrentPolicy of MB = 1, R = 0, H = K = 2
    import torch
    from gym_rem2d_amd import policy
    pol = policy.RecurrentPolicy(*(torch.from_numpy(a) for a in W), 2)
    assert (pol.max_bodies, pol.n_rays, pol.hidden, pol.context, pol.d) == (1, 0, 2, 2, 16)


def test_the_recurrent_loop_is_alive(oracle):
    """recurrent_loop_run on the lsystem loop population, 120 steps: all state finite (the run asserts it), every target valid, and
    the memory finite, not all zero and moving."""
    runs = RM.recurrent_loop_run(oracle, "lsystem", CONT)
    assert len(runs) >= 2
    for run in runs:
        mem = np.stack(run["memory"])
        assert mem.shape == (PM.N_POLICY_LOOP + 1, run["ctx"].N, RM.LOOP_CONTEXT) and mem.dtype == f32
        assert np.isfinite(mem).all() and not mem[0].any() and mem[-1].any()
        assert (np.abs(mem[-1]) > 1e-3).mean() > 0.5 and (mem[-1] != mem[-2]).mean() > 0.5
        assert all(v.all() for v in run["valid"])
