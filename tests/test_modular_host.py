"""Modular device policies without a GPU (include/rem2d_modular.h): the host model against the recurrent model (law (a)), the
header against the binding and the three libraries, the refusals of the three calls on descriptors that are never dereferenced,
and what ``policy.ModularPolicy`` checks and draws.  tests/test_modular_gpu.py holds the kernels to the same model."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import caller_stream
import modular_model as MM
import policy_model as PM
import recurrent_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
EXPORTS = ["rem2d_modular_abi_version", "rem2d_worlds_topology", "rem2d_modular_forward", "rem2d_worlds_act_modular"]


# --------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("MB,H,K,R,act", [(1, 1, 1, 0, PM.SOFTSIGN), (3, 5, 2, 0, PM.RELU), (12, 32, 8, 10, PM.SOFTSIGN),
                                            (64, 8, 8, 10, PM.RELU)])
def test_one_round_is_the_recurrent_pass_on_flattened_rows(MB, H, K, R, act):
    """law (a): one round on (row, body) writes the bits of rem2d_recurrent_forward's model for max_bodies = 1,
    obs' = [head | body], frac' = [frac | shape | children | cm], context = K and memory' = pm"""
    N = 9
    f = MM.forge(3, N, MB, H, K, R)
    W = f["weights"]
    reset = (np.arange(N) % 4 == 1).astype(np.uint8)
    tg, valid, new = MM.forward_model(f["obs"], f["frac"], f["topo"], f["memory"], *W, rounds=1, act=act, reset=reset)
    live, par = MM.tree(f["topo"])
    m0 = f["memory"].copy()
    m0[reset != 0] = 0
    m0[~live] = 0
    nch, cm, pm = MM.gather(m0, live, par)
    x = MM.body_rows(f["obs"], f["frac"], f["topo"], nch, cm, pm)
    seen = 0
    for b in range(MB):
        rows = np.nonzero(live[:, b])[0]
        if not len(rows):
            continue
        flat = x[rows, b, :MM.width(R, K) - K]                    # [head | body b | frac | shape | children | cm]
        t1, v1, m1 = RM.forward_model(flat, pm[rows, b], *W, act=act, index=rows)
        assert t1.shape == (len(rows), 1)
        assert np.array_equal(PM.bits(t1[:, 0]), PM.bits(tg[rows, b])) and np.array_equal(v1[:, 0], valid[rows, b])
        assert np.array_equal(RM.mem_bits(m1), MM.mem_bits(new[rows, b]))
        seen += len(rows)
    assert seen == int(live.sum()) >= N
    # the slots that are not live: nothing
    assert not tg[~live].any() and not valid[~live].any() and not new[~live].view(np.uint32).any()


def test_model_tree_rules_and_sum_order():
    # parents out of range, the body itself, a non-live parent and a 2-cycle
    topo = np.array([[[-1, 1], [0, 1], [7, 1], [3, 1], [5, 1], [1, 0], [5, 2], [8, 1], [7, 1]]], np.int32)
    live, par = MM.tree(topo)
    assert live[0].tolist() == [True] * 5 + [False] + [True] * 3
    assert par[0].tolist() == [-1, 0, 7, -1, -1, -1, -1, 8, 7]     # 2: its parent 7 is live; 7 and 8 are each other's parent
    m = np.zeros((1, 9, 1), f32)
    m[0, :, 0] = [1, 2, 3, 4, 5, 6, 7, 8, 9]
    nch, cm, pm = MM.gather(m, live, par)
    assert nch[0].tolist() == [1, 0, 0, 0, 0, 0, 0, 2, 1] and cm[0, 7, 0] == 12 and cm[0, 8, 0] == 8 and pm[0, 8, 0] == 8
    # the sum runs in ascending child order, one rounded add each: a star whose exact sum differs from the ordered one
    vals = np.array([1e8, 1.0, -1e8, 1.0] * 15 + [1.0] * 3, f32)
    star = np.zeros((1, 64, 2), np.int32)
    star[0, :, 1] = 1
    star[0, 0, 0] = -1
    mem = np.zeros((1, 64, 1), f32)
    mem[0, 1:, 0] = vals
    live, par = MM.tree(star)
    acc = f32(0.0)
    for v in vals:
        acc = f32(acc + v)
    assert MM.gather(mem, live, par)[1][0, 0, 0] == acc != f32(vals.astype(np.float64).sum())


def test_messages_reach_the_root_one_edge_per_round():
    """a 3-chain under a hand-made set (K = 1).  A round makes a body's message from its own words and from the messages of the
    round before, so a word travels one edge per round AFTER the round that put it into its own body's message: the middle body's
    touching word is in the root's message after exactly two rounds, the leaf's after exactly three."""
    W = relay_weights()
    obs = np.zeros((1, 8 + 6 * 3), f32)
    obs[0, 8 + 6 * 1 + 3] = 1.0                                    # body 1, the root's child, touches
    topo = MM.topology_model([MM.chain(3)], [[1, 1, 1]], 3)
    mem = np.zeros((1, 3, 1), f32)
    _, _, a1 = MM.forward_model(obs, None, topo, mem, *W, rounds=1, act=PM.RELU)
    _, _, a2 = MM.forward_model(obs, None, topo, a1, *W, rounds=1, act=PM.RELU)
    assert a1[0, :, 0].tolist() == [0.0, 1.0, 0.0] and a2[0, :, 0].tolist() == [1.0, 1.0, 0.0]      # two acts, not one
    _, _, b1 = MM.forward_model(obs, None, topo, mem, *W, rounds=2, act=PM.RELU)
    assert b1[0, :, 0].tolist() == [1.0, 1.0, 0.0]                                                 # P = 2: one act
    obs = np.zeros((1, 8 + 6 * 3), f32)
    obs[0, 8 + 6 * 2 + 3] = 1.0                                    # body 2 touches
    topo = MM.topology_model([MM.chain(3)], [[1, 1, 1]], 3)
    mem = np.zeros((1, 3, 1), f32)
    _, _, m1 = MM.forward_model(obs, None, topo, mem, *W, rounds=1, act=PM.RELU)
    assert m1[0, :, 0].tolist() == [0.0, 0.0, 1.0]
    t2, _, m2 = MM.forward_model(obs, None, topo, m1, *W, rounds=1, act=PM.RELU)
    assert m2[0, :, 0].tolist() == [0.0, 1.0, 1.0] and t2[0, 0] == 0.0
    t3, _, m3 = MM.forward_model(obs, None, topo, m2, *W, rounds=1, act=PM.RELU)
    assert m3[0, :, 0].tolist() == [1.0, 1.0, 1.0] and t3[0, 0] > 0.0       # the root's target moves with its message
    _, _, p2 = MM.forward_model(obs, None, topo, mem, *W, rounds=2, act=PM.RELU)
    assert p2[0, :, 0].tolist() == [0.0, 1.0, 1.0]
    _, _, p3 = MM.forward_model(obs, None, topo, mem, *W, rounds=3, act=PM.RELU)
    assert p3[0, :, 0].tolist() == [1.0, 1.0, 1.0]


def relay_weights():
    """K = 1, H = 1, R = 0, relu: h = touching + (the children's messages); the target is positive iff h is"""
    Dm = MM.width(0, 1)
    w1 = np.zeros((1, Dm, 1), f32)
    w1[0, 8 + 3, 0] = 1.0                                          # the body's touching word
    w1[0, 8 + 6 + 2, 0] = 1.0                                      # cm_0
    return w1, np.zeros((1, 1), f32), np.ones((1, 1, 1), f32), np.zeros((1, 1), f32)


# ---------------------------------------------------------------------------------------- header, binding and the libraries
def test_header_binding_and_libraries_agree():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib, policy
    with open(os.path.join(ROOT, "include", "rem2d_modular.h")) as f:
        text = f.read()
    declared = re.findall(r"^\s*int\s+(rem2d_\w+)\s*\(", text, flags=re.M)
    assert declared == EXPORTS
    assert int(re.search(r"#define REM2D_MODULAR_ABI_VERSION (\d+)", text).group(1)) == _lib.MODULAR_ABI_VERSION == 1
    assert int(re.search(r"#define REM2D_MODULAR_MAX_ROUNDS (\d+)", text).group(1)) == _lib.MODULAR_MAX_ROUNDS == MM.MAX_ROUNDS == 8
    assert int(re.search(r"#define REM2D_MODULAR_MAX_INPUTS (\d+)", text).group(1)) == _lib.MODULAR_MAX_INPUTS == MM.MAX_INPUTS
    assert _lib.MODULAR_MAX_INPUTS == _lib.SENSE_MAX_RAYS == 64
    # no declaration takes a `void *stream` parameter: the stream is a member of both descriptors
    takers = caller_stream.stream_takers()
    assert not set(EXPORTS) & set(takers)
    assert set(EXPORTS) <= set(caller_stream.declared())
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    for struct, cls in (("rem2d_topology", _lib.Topology), ("rem2d_modular", _lib.Modular)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        members = re.findall(r"^\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+);", body, flags=re.M)
        assert [m[2] for m in members] == [n for n, _ in cls._fields_], members
        for (tname, star, name), (_, ct) in zip(members, cls._fields_):
            assert ct is (C.c_void_p if star else _lib.Policy if tname == "rem2d_policy" else ctype[tname]), name
        assert cls._fields_[-1][0] == "stream" and getattr(cls, "stream").offset == C.sizeof(cls) - 8
    P = C.sizeof(_lib.Policy)
    assert C.sizeof(_lib.Modular) == P + 2 * 4 + 4 * 8 and C.sizeof(_lib.Topology) == 2 * 4 + 3 * 8
    assert [getattr(_lib.Modular, n).offset for n, _ in _lib.Modular._fields_] == [0, P, P + 4, P + 8, P + 16, P + 24, P + 32]
    for path in (_lib.LIB_PATH, _lib.WIDE_LIB_PATH, _lib.FMA_LIB_PATH):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert sorted(re.findall(r" T (rem2d_\w*(?:modular|topology)\w*)", syms)) == sorted(EXPORTS), path
    for wide in (False, True, "fma"):
        L = _lib.lib(wide)
        assert L.rem2d_modular_abi_version() == _lib.MODULAR_ABI_VERSION
        # nothing else changes version
        assert L.rem2d_abi_version() == 11 and L.rem2d_policy_abi_version() == 1 and L.rem2d_recurrent_abi_version() == 1
        assert L.rem2d_control_abi_version() == 1 and L.rem2d_evolve_abi_version() == 1 and L.rem2d_obsnorm_abi_version() == 1
        assert L.rem2d_modular_forward.argtypes == [C.POINTER(_lib.Modular)]
        assert L.rem2d_worlds_topology.argtypes == [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(_lib.Topology)]
        assert L.rem2d_worlds_act_modular.argtypes == [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(_lib.Modular), C.c_void_p]
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):          # the older headers know nothing of it
        if header == "rem2d_modular.h":
            continue
        with open(os.path.join(ROOT, "include", header)) as f:
            other = f.read()
        for name in declared + ["REM2D_MODULAR_", "rem2d_modular", "rem2d_topology"]:
            assert name not in other, (header, name)
    for name in os.listdir(os.path.join(ROOT, "oracle")):                      # no CPU twin
        if name.endswith((".c", ".h", ".py")):
            with open(os.path.join(ROOT, "oracle", name)) as f:
                assert "rem2d_modular" not in f.read(), name
    with open(os.path.join(ROOT, "__graft_entry__.py")) as f:
        entry = f.read()
    assert all('"%s"' % name in entry for name in declared)
    assert issubclass(policy.ModularPolicy, policy.MLPPolicy) and not issubclass(policy.ModularPolicy, policy.RecurrentPolicy)


# ----------------------------------------------------------------------------------------------------------- the refusals
MOD_FIELDS = ("messages", "rounds", "topo", "memory", "reset", "stream")


def _desc(**kw):
    """a good descriptor: MB 16, R 10, K 8, H 32 (Dm = 42), three rows with a set each; the "device pointers" are never dereferenced"""
    from gym_rem2d_amd import _lib
    q = _lib.Modular()
    p = q.p
    p.d, p.max_bodies, p.n_rays, p.hidden, p.activation, p.scale, p.n_sets, p.reserved = 42, 16, 10, 32, 0, 1.5, 3, 0
    for k in ("w1", "b1", "w2", "b2", "obs", "frac", "targets", "valid"):
        setattr(p, k, 256)
    p.index, p.row_mask, p.n_rows = None, None, 3
    q.messages, q.rounds, q.topo, q.memory, q.reset, q.stream = 8, 1, 256, 256, None, None
    for k, v in kw.items():
        setattr(q if k in MOD_FIELDS else p, k, v)
    return q


# (what is wrong, the field the message must name): every REM2D_E_INVALID case the header lists
BAD = [(dict(messages=0, d=26), b"messages must be"), (dict(messages=-2, d=22), b"messages must be"),          # K < 1
       (dict(messages=33, hidden=32, n_rays=0, d=82), b"messages must be"),                                     # K > H
       (dict(messages=27, n_rays=9, d=79), b"n_rays + 2 + 2 messages"),                                          # 9 + 2 + 54 = 65
       (dict(messages=1, n_rays=61, d=79), b"n_rays + 2 + 2 messages"),
       (dict(rounds=0), b"rounds must be"), (dict(rounds=9), b"rounds must be"), (dict(rounds=-1), b"rounds must be"),
       (dict(d=41), b"d must be"), (dict(d=43), b"d must be"), (dict(d=114), b"d must be"), (dict(d=122), b"d must be"),   # (the other rules)
       (dict(topo=None), b"topo"), (dict(memory=None), b"memory"),
       # ... and what rem2d_policy_forward refuses
       (dict(max_bodies=0), b"max_bodies"), (dict(max_bodies=65), b"max_bodies"), (dict(n_rays=-1, d=31), b"n_rays"),
       (dict(n_rays=65, d=107), b"n_rays"), (dict(hidden=0), b"hidden"), (dict(hidden=129), b"hidden"), (dict(activation=2), b"activation"),
       (dict(n_sets=0), b"n_sets"), (dict(n_rows=-1), b"row count"), (dict(w1=None), b"NULL device pointer"),
       (dict(obs=None), b"NULL device pointer"), (dict(frac=None), b"NULL device pointer"), (dict(targets=None), b"NULL device pointer"),
       (dict(valid=None), b"NULL device pointer"), (dict(n_sets=2), b"without an index")]


def test_bad_descriptors_are_refused_by_name():
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
        assert L.rem2d_modular_forward(None) == -1 and b"NULL modular policy" in err()
        assert L.rem2d_worlds_act_modular(fake, 1, None, buf) == -1 and b"NULL modular policy" in err()
        for kw, msg in BAD:
            q = _desc(**kw)
            assert L.rem2d_modular_forward(C.byref(q)) == -1 and msg in err() and err().startswith(b"modular: "), (kw, err())
            assert L.rem2d_worlds_act_modular(fake, 1, C.byref(q), buf) == -1 and msg in err() and err().startswith(b"act_modular: "), (kw, err())
        good = _desc()
        assert L.rem2d_worlds_act_modular(None, 1, C.byref(good), buf) == -1 and b"no worlds" in err()
        assert L.rem2d_worlds_act_modular(fake, 0, C.byref(good), buf) == -1 and b"no worlds" in err()
        assert L.rem2d_worlds_act_modular(fake, 1, C.byref(good), None) == -1 and b"ray offsets" in err()
        assert L.rem2d_worlds_act_modular(null, 1, C.byref(good), buf) == -1 and b"world 0 is NULL" in err()
        # the edges that are allowed: K = H, R + 2 + 2 K = 64, P = 8, MB = 1 and 64, a reset mask, no rays -- on an empty population,
        # which launches nothing
        for kw in (dict(messages=26, n_rays=10, d=78), dict(messages=31, n_rays=0, frac=None, d=78), dict(messages=8, hidden=8),
                   dict(rounds=8), dict(max_bodies=1), dict(max_bodies=64), dict(reset=256)):
            q = _desc(n_rows=0, n_sets=1, index=256, **kw)
            assert L.rem2d_modular_forward(C.byref(q)) == 0, (kw, err())
        # the topology call: rem2d_worlds_observe's refusals, in its order
        t = _lib.Topology()
        t.max_bodies, t.reserved, t.out, t.out_rows, t.stream = 4, 0, 256, 1, None

        def topo(worlds, n, **kw):
            d = _lib.Topology()
            C.memmove(C.byref(d), C.byref(t), C.sizeof(t))
            for k, v in kw.items():
                setattr(d, k, v)
            return L.rem2d_worlds_topology(worlds, n, C.byref(d))
        assert topo(None, 1) == -1 and b"no worlds" in err()
        assert topo(fake, 0) == -1 and b"no worlds" in err()
        assert L.rem2d_worlds_topology(fake, 1, None) == -1 and b"NULL descriptor" in err()
        assert topo(fake, 1, reserved=3) == -1 and b"reserved" in err()
        assert topo(fake, 1, out=None) == -1 and b"NULL device pointer" in err()
        assert topo(fake, 1, max_bodies=0) == -1 and b"max_bodies" in err()
        assert topo(fake, 1, max_bodies=65) == -1 and b"max_bodies" in err()
        assert topo(fake, 1, out_rows=-1) == -1 and b"row count" in err()
        assert topo(null, 1) == -1 and b"world 0 is NULL" in err() and err().startswith(b"topology: ")
        assert topo(two, 2, max_bodies=99) == -1 and b"max_bodies" in err()       # the arguments before any world is looked at


# ----------------------------------------------------------------------------------------------------------- the class
def _arrays(H=32, K=8, R=10, G=2, last=1):
    rng = np.random.default_rng(5)
    Dm = MM.width(R, K)
    return [rng.standard_normal(s).astype(f32) for s in ((G, Dm, H), (G, H), (G, H, last), (G, last))]


def test_modular_policy_validation():
    import torch
    from gym_rem2d_amd import policy
    MP = policy.ModularPolicy
    p = MP(*_arrays(), messages=8, rounds=3, max_bodies=12)
    assert (p.messages, p.rounds, p.max_bodies, p.weight_bodies, p.n_rays, p.hidden, p.d, p.n_sets) == (8, 3, 12, 1, 10, 32, 42, 2)
    assert p.weight_bytes() == 4 * (42 * 32 + 32 + 32 + 1)
    assert tuple(p.new_memory(5).shape) == (5, 12, 8) and p.new_memory(5).dtype == torch.float32 and not p.new_memory(5).any()
    for K in (0, -1, True, 1.5, None):
        with pytest.raises(ValueError, match="messages"):
            MP(*_arrays(), messages=K)
    with pytest.raises(ValueError, match="messages = 9 is more than the 8 hidden"):
        MP(*_arrays(H=8, K=9, R=0), messages=9)
    MP(*_arrays(H=8, K=8, R=0), messages=8)                                         # K = H
    ok = MP(*_arrays(H=32, K=26, R=10), messages=26)                                # R + 2 + 2 K = 64
    assert ok.n_rays == 10 and ok.d == 78
    with pytest.raises(ValueError, match="input rows"):
        MP(*_arrays(H=32, K=26, R=11), messages=26, rays=np.zeros((11, 2)))        # 65
    with pytest.raises(ValueError, match="input rows"):
        MP(*_arrays(H=32, K=8, R=10), messages=14)                                  # R would be negative
    for P in (0, 9, -1, True, 2.0):
        with pytest.raises(ValueError, match="rounds"):
            MP(*_arrays(), messages=8, rounds=P)
    MP(*_arrays(), messages=8, rounds=8)
    for MB in (0, 65, None):
        with pytest.raises(ValueError, match="max_bodies"):
            MP(*_arrays(), messages=8, max_bodies=MB)
    with pytest.raises(ValueError, match="w2's last axis must be 1, not 2"):
        MP(*_arrays(last=2), messages=8)
    # what moves weights about keeps the class, K, P and the row side
    t = p.take([1, 1, 0])
    assert type(t) is MP and (t.messages, t.rounds, t.max_bodies, t.n_sets) == (8, 3, 12, 3) and torch.equal(t.w1[0], p.w1[1])
    s = p._sets(4, zeroed=True)
    assert type(s) is MP and (s.messages, s.rounds, s.max_bodies) == (8, 3, 12) and tuple(s.w2.shape) == (4, 32, 1)
    assert type(p.to("cpu")) is MP
    # a CPU policy has no descriptor
    with pytest.raises(ValueError, match="move the policy to the GPU"):
        p.forward(torch.zeros((2, 8 + 6 * 12)), torch.zeros((2, 10)), torch.zeros((2, 12, 2), dtype=torch.int32), p.new_memory(2))


def test_random_draws_what_an_ordinary_set_of_one_body_draws():
    import torch
    from gym_rem2d_amd import policy
    for R, K in ((10, 8), (0, 1), (10, 26), (3, 5)):
        m = policy.ModularPolicy.random(3, 32, K, rounds=2, max_bodies=12, n_rays=R, seed=11)
        f = policy.MLPPolicy.random(3, 1, 32, n_rays=R + 2 + 2 * K, seed=11, rays=np.zeros((R + 2 + 2 * K, 2)))
        assert all(torch.equal(a, b) for a, b in zip(m.weights, f.weights))
        assert (m.messages, m.rounds, m.max_bodies, m.n_rays, m.d) == (K, 2, 12, R, MM.width(R, K)) and f.d == m.d and f.max_bodies == 1
        assert (m.rays is None) == (R == 0) and (R == 0 or m.rays.shape == (R, 2))


def test_set_policy_refuses_what_is_not_built():
    """normalizer= and a streamed evaluation, on an env that never reaches a library call"""
    from gym_rem2d_amd import policy
    from gym_rem2d_amd.env import BatchedModular2D
    env = BatchedModular2D.__new__(BatchedModular2D)
    env._policy = env._act_args = None
    env._context_reset = False
    env.worlds = [(None, None)]
    env.n_envs = 2
    env._stream_rec = None
    p = policy.ModularPolicy(*_arrays(), messages=8, max_bodies=12)
    with pytest.raises(ValueError, match="a ModularPolicy takes no normalizer"):
        env.set_policy(p, normalizer=object())
    env._stream_rec = object()
    with pytest.raises(ValueError, match="cannot be attached to a streamed evaluation"):
        env.set_policy(p)
    env._policy = dict(topo=object(), memory=object())
    with pytest.raises(ValueError, match="refill: a ModularPolicy is attached"):
        env.refill()
