"""Observation normalisation on a real MI355X (pytest -m gpu; include/rem2d_obsnorm.h) against tests/obsnorm_model.py, bit for bit,
in the three builds: the exact sums at every launch shape, the tables on forged states, the law of the normalised forward passes,
act() under a normaliser on a 64-creature population, and the five calls under a capture and behind a gate on a caller's stream."""
import ctypes as C

import numpy as np
import pytest

import obsnorm_model as OM
import policy_model as PM
import recurrent_model as RM
import test_caller_stream_gpu as TCS
import test_policy_gpu as TP
import test_recurrent_gpu as TR
from test_caller_stream_gpu import gate  # noqa: F401  (the fixture: the gate's cycle count, proved by its control)

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
nan, inf = float("nan"), float("inf")
BUILDS = (False, True, "fma")
SHAPES = [(1, 0), (3, 10), (16, 10)]                          # (MB, R): Dn = 14, 36, 114 -- one and two words per lane
GROUPS = (1, 3, 16, 64, 65, 200)                              # blocks inside a chunk, across wavefronts, across workgroups
CHUNKS = (0, 1, 7, 64, 65536)
H = 2.0 ** -12
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gpu():
    import replay
    return replay.need_gpu()


def bits64(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------------ accumulate
def forge_rows(rng, n, Dn):
    """rows of every kind the header names: a bulk of several sizes; values at +-2048 and beyond; rint ties at odd multiples of
    2^-13; denormals; +-0; rows with one NaN / +inf / -inf word; and a mask that clears some rows, good and bad ones"""
    x = (rng.standard_normal((n, Dn)) * rng.choice([0.01, 1.0, 40.0, 1500.0], (1, Dn))).astype(f32)
    edge = np.array([2048.0, -2048.0, 2048.00025, -2048.00025, 1e30, -3e38, 2047.9999, 1e-40, -1e-45, 0.0, -0.0], f32)
    hit = rng.random((n, Dn)) < 0.08
    x[hit] = rng.choice(edge, int(hit.sum()))
    ties = rng.random((n, Dn)) < 0.08                              # (2 k + 1) 2^-13: exactly between two steps
    x[ties] = ((2 * rng.integers(-4000, 4000, int(ties.sum())) + 1) * 2.0 ** -13).astype(f32)
    for r in range(1, n, 6):
        x[r, rng.integers(Dn)] = (nan, inf, -inf)[(r // 6) % 3]
    mask = (rng.random(n) < 0.8).astype(np.uint8)
    mask[:2] = 0                                                    # one good row and one bad one at least
    mask[2:4] = 1
    return x, mask


def split(torch, x, MB):
    wd = 8 + 6 * MB
    xd = torch.from_numpy(x).to(DEV)
    return xd[:, :wd].contiguous(), (xd[:, wd:].contiguous() if x.shape[1] > wd else None)


def put_state(torch, norm, st):
    for name, a in zip(("count", "s1", "s2hi", "s2lo"), st.words()):
        getattr(norm, name).copy_(torch.from_numpy(a).reshape(getattr(norm, name).shape))


def get_state(norm):
    return [getattr(norm, k).cpu().numpy() for k in ("count", "s1", "s2hi", "s2lo")]


@pytest.mark.parametrize("S", GROUPS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "MB%d-R%d" % s)
def test_accumulate(gpu, shape, S):
    """every state word == the model: from a state that already holds sums, a partial last block and one block without rows, under
    a mask, then a second call on other rows (two calls equal one: the model adds both); at every chunking, in every build"""
    torch = gpu
    from gym_rem2d_amd import policy
    MB, R = shape
    Dn, M = OM.width(MB, R), (4 if S > 1 else 8)
    n = 2 * S + (S + 1) // 2 + (4 if S == 1 else 0)                # not a multiple of S; the last block gets nothing
    rng = np.random.default_rng([MB, R, S])
    x1, m1 = forge_rows(rng, n, Dn)
    x2, m2 = forge_rows(rng, n - 1, Dn)
    start = OM.State(M, Dn)
    start.count[:] = rng.integers(0, 1000, M)
    start.s1[:], start.s2hi[:], start.s2lo[:] = rng.integers(-2 ** 40, 2 ** 40, (M, Dn)), rng.integers(0, 2 ** 40, (M, Dn)), rng.integers(0, 2 ** 40, (M, Dn))
    want1 = OM.accumulate(start.copy(), x1, S, m1)
    want2 = OM.accumulate(want1.copy(), x2, S, None)
    assert 0 < int(OM.contributes(x1, m1).sum()) < int(OM.contributes(x1).sum()) < n
    assert np.array_equal(want2.words()[1][M - 1], start.words()[1][M - 1]) and n <= (M - 1) * S
    norm = policy.ObsNormalizer(M, S, MB, R, device=DEV)
    o1, f1 = split(torch, x1, MB)
    o2, f2 = split(torch, x2, MB)
    md = torch.from_numpy(m1).to(DEV)
    for wide in BUILDS:
        for chunk in CHUNKS:
            put_state(torch, norm, start)
            norm.accumulate(o1, f1, row_mask=md, row_chunk=chunk, wide=wide)
            what = "MB %d R %d S %d chunk %d build %s" % (MB, R, S, chunk, wide)
            for name, g, w in zip(("count", "s1", "s2hi", "s2lo"), get_state(norm), want1.words()):
                assert np.array_equal(g, w), "%s: `%s` differs from the model in %d words" % (what, name, int((g != w).sum()))
            norm.accumulate(o2, f2, row_chunk=chunk, wide=wide)
            for name, g, w in zip(("count", "s1", "s2hi", "s2lo"), get_state(norm), want2.words()):
                assert np.array_equal(g, w), "%s, second call: `%s` differs from the model" % (what, name)
    assert torch.equal(o1.view(torch.int32), split(torch, x1, MB)[0].view(torch.int32))      # the rows are read, never written


def test_no_rows(gpu):
    """n_rows = 0: nothing is launched, nothing moves -- accumulate, and the forward pass of a descriptor cut to no rows"""
    torch = gpu
    from gym_rem2d_amd import _lib, policy
    norm = policy.ObsNormalizer(2, 3, 2, 1, device=DEV)
    norm.s1.fill_(7)
    pol = policy.MLPPolicy.random(1, 2, 4, n_rays=1, rays=np.zeros((1, 2)) + 1.0, index=np.zeros(1, np.int64)).to(DEV)
    obs, frac = torch.zeros((1, 20), device=DEV), torch.zeros((1, 1), device=DEV)
    out = (torch.full((1, 2), 9.0, dtype=torch.float64, device=DEV), torch.full((1, 2), 9, dtype=torch.uint8, device=DEV))
    for wide in BUILDS:
        norm.accumulate(obs[:0], frac[:0], wide=wide)
        p = pol.descriptor(obs, frac, *out)
        p.n_rows = 0
        n = norm.descriptor()
        n.stream = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib(wide).rem2d_obsnorm_forward(C.byref(n), C.byref(p)), wide)
    torch.cuda.synchronize()
    assert bool((norm.s1 == 7).all()) and not norm.count.any() and norm.offered == 0 and bool((out[0] == 9).all()) and bool((out[1] == 9).all())


# ---------------------------------------------------------------------------------------------------------------------- freeze
def forged_states(min_count, min_var):
    """-> (count [M], s1, s2hi, s2lo [M][Dn = 14]) and the blocks' names: one block per kind of state"""
    Dn = 14
    rng = np.random.default_rng(5)
    blocks, names = [], []

    def add(name, n, s1, s2):
        """a block of n rows whose word i has sum s1[i] and sum of squares s2[i] (Python ints), the squares split at 2^23 -- some
        canonically, some with a low part far beyond 2^23, as many rows leave it"""
        hi, lo = [], []
        for i, t in enumerate(s2):
            carry = min((0, 1, (t >> 23) // 3, t >> 23)[i % 4], 1 << 38)            # (the low part stays below 2^62)
            hi.append((t >> 23) - carry)
            lo.append((t & OM.LOW) + (carry << 23))
        blocks.append((n, list(s1), hi, lo))
        names.append(name)
    for n in (min_count - 1, min_count, min_count + 1):                        # n around min_count, on ordinary words
        q = rng.integers(-5000, 5000, (max(n, 1), Dn))
        add("n = %d" % n, n, [int(v) for v in q[:n].sum(axis=0)], [int(v) for v in (q[:n] ** 2).sum(axis=0)])
    mv = f32(min_var)
    n = 1 << 30                                                                 # vx a step either side of min_var: m = 0, s2 = n vx 2^24
    steps = [np.nextafter(mv, f32(0)), mv, np.nextafter(mv, f32(inf))]
    vq = [int(round(float(v) * 2 ** 24 * n)) for v in steps]
    add("vx around min_var", n, [0] * Dn, [vq[i % 3] for i in range(Dn)])
    n, q = (1 << 39) - 7, (1 << 23) - 1                                          # s1 near +-2^62, constant words: v rounds to <= 0
    add("s1 near 2^62", n, [n * q if i % 2 else -n * q for i in range(Dn)], [n * q * q] * Dn)
    add("negative v", 10, [50 + i for i in range(Dn)], [24 + i for i in range(Dn)])        # s2 / n below m m outright
    n = 1 << 20                                                                 # a ladder of variances over 40 binades, around a mean
    for part in range(3):
        ks = [part * 14 + i - 10 for i in range(Dn)]                            # v = 2^k, k = -10 .. 31
        mq = 12345 * (part - 1)
        add("ladder %d" % part, n, [n * mq] * Dn, [(n << (k + 10) >> 10 if k >= 0 else n >> -k) + n * mq * mq for k in ks])
    count = np.array([b[0] for b in blocks], np.int64)
    s1, s2hi, s2lo = (np.array([b[j] for b in blocks], np.int64) for j in (1, 2, 3))
    return (count, s1, s2hi, s2lo), names


@pytest.mark.parametrize("min_var", [2.0 ** -20, 1e-6, 3.0])
def test_freeze(gpu, min_var):
    torch = gpu
    from gym_rem2d_amd import policy
    min_count = 5
    words, names = forged_states(min_count, min_var)
    M = len(names)
    mu, inv = OM.freeze(*words, min_count, min_var)
    # the forged states are what they claim
    b = names.index("vx around min_var")
    assert (inv[b, 0::3] == 0).all() and (inv[b, 1::3] > 0).all() and (inv[b, 2::3] > 0).all() and (inv[b, 1:12:3] >= inv[b, 2::3]).all()
    assert (inv[names.index("n = 4")] == 1).all() and (mu[names.index("n = 4")] == 0).all() and (inv[names.index("n = 5")] != 1).all()
    assert (inv[names.index("s1 near 2^62")] == 0).all() and (inv[names.index("negative v")] == 0).all()
    assert (np.abs(mu[names.index("s1 near 2^62")]) == f32(2048.0 - H)).all()
    ladder = np.concatenate([inv[names.index("ladder %d" % p)] for p in range(3)])
    assert len(set(ladder[ladder > 0].tolist())) >= 20 or min_var > 1
    norm = policy.ObsNormalizer(M, 1, 1, 0, min_count=min_count, min_var=min_var, device=DEV)
    for name, a in zip(("count", "s1", "s2hi", "s2lo"), words):
        getattr(norm, name).copy_(torch.from_numpy(a))
    for wide in BUILDS:
        norm.mu.fill_(-7.0)
        norm.inv.fill_(-7.0)
        got_mu, got_inv = (t.cpu().numpy() for t in norm.freeze(wide=wide))
        for what, g, w in (("mu", got_mu, mu), ("inv", got_inv, inv)):
            ne = OM.tbits(g) != OM.tbits(w)
            where = tuple(np.argwhere(ne)[0]) if ne.any() else None
            assert not ne.any(), "build %s min_var %g: %d words of `%s` differ, first in block `%s` word %d: gpu %r model %r" % (
                wide, min_var, int(ne.sum()), what, names[where[0]], where[1], g[where], w[where])


# --------------------------------------------------------------------------------------------------------------------- forward
T_SENT, V_SENT = TP.T_SENTINEL, TP.V_SENTINEL


def forge_tables(rng, M, Dn, x, S):
    """tables of every kind: ordinary, mu = the word itself, inv = 0 on a third of the words (a NaN / inf of x among them)"""
    mu = (rng.standard_normal((M, Dn)) * 0.5).astype(f32)
    inv = np.exp(rng.standard_normal((M, Dn))).astype(f32)
    inv[:, ::3] = 0.0
    inv[:, 1::7] = 300.0                                                        # these words clip
    blk = np.arange(x.shape[0]) // S
    for k, (r, i) in enumerate(np.argwhere(~np.isfinite(x[:, :Dn]))):           # inf * 0 and inf * something both occur
        inv[blk[r], i] = 0.0 if k % 2 == 0 else 2.0
    return mu, inv


def normed_forward(torch, policy_mod, norm, MB, R, K, act, x, W, index, mask, reset, wide, off):
    """-> (targets bits, valid, memory bits or None) of one normalised pass over guarded, prefilled outputs"""
    N, Dn = x.shape[0], OM.width(MB, R)
    w = [TP._offset_copy(torch, a, off, DEV) for a in W]
    rays = None if R in (0, 10) else np.zeros((R, 2)) + 1.0
    idx = None if index is None else torch.from_numpy(index).to(DEV)
    if K:
        pol = policy_mod.RecurrentPolicy(*w, K, activation=act, index=idx, rays=rays)
    else:
        pol = policy_mod.MLPPolicy(*w, activation=act, index=idx, rays=rays)
    obs, frac = split(torch, np.ascontiguousarray(x[:, :Dn]), MB)
    md = None if mask is None else torch.from_numpy(mask).to(DEV)
    tbuf, t = TP._guarded(torch, N * MB, torch.float64, T_SENT, DEV)
    vbuf, v = TP._guarded(torch, N * MB, torch.uint8, V_SENT, DEV)
    kw = {}
    if K:
        kw = dict(memory=torch.from_numpy(np.ascontiguousarray(x[:, Dn:])).to(DEV), reset=None if reset is None else torch.from_numpy(reset).to(DEV))
    norm.forward(pol, obs, frac, out=(t.view(N, MB), v.view(N, MB)), row_mask=md, wide=wide, **kw)
    tb, vb = tbuf.cpu().numpy(), vbuf.cpu().numpy()
    G = TP.GUARD
    assert (tb[:G] == T_SENT).all() and (tb[-G:] == T_SENT).all() and (vb[:G] == V_SENT).all() and (vb[-G:] == V_SENT).all(), "guards overwritten"
    assert torch.equal(obs.view(torch.int32), split(torch, np.ascontiguousarray(x[:, :Dn]), MB)[0].view(torch.int32))   # obs keeps its raw values
    return PM.bits(tb[G:-G].reshape(N, MB)), vb[G:-G].reshape(N, MB).copy(), (RM.mem_bits(kw["memory"].cpu().numpy()) if K else None)


@pytest.mark.parametrize("act", [PM.SOFTSIGN, PM.RELU])
@pytest.mark.parametrize("shape", [(1, 0, 0, 1), (3, 10, 0, 5), (16, 10, 0, 32), (4, 3, 2, 5), (16, 10, 7, 32)], ids=lambda s: "MB%d-R%d-K%d-H%d" % s)
def test_the_law(gpu, shape, act):
    """targets, valid and memory == the plain passes' models fed x^, bit for bit: per-row sets and 7 sets through an index with a
    row mask (a row's block is r // S, its set whatever the index says), NaN / +-inf words under inv = 0 and under inv != 0, words
    that clip, a partial last block; weights 16-byte aligned and 4 bytes off; the three builds.  Skipped rows keep the sentinels
    and their memory.  Under identity tables and clip = inf the bytes are the plain kernel's own."""
    torch = gpu
    from gym_rem2d_amd import policy
    MB, R, K, Hd = shape
    Dn = OM.width(MB, R)
    off_nan = on_nan = invalid = valid = 0
    for N, S in ((9, 4), (65, 16), (130, 200)):
        M = (N + S - 1) // S
        for mode in ("per_row", "indexed"):
            x, W, index, mask = TP.forge(MB, R + K, Hd, N, mode, 3)
            rng = np.random.default_rng([MB, R, K, Hd, N])
            mu, inv = forge_tables(rng, M, Dn, x, S)
            reset = (rng.random(N) < 0.3).astype(np.uint8) if K else None
            if K:
                want_t, want_v, want_m = OM.forward_memory(x[:, :Dn], x[:, Dn:], mu, inv, 5.0, S, *W, act=act, index=index, reset=reset, row_mask=mask)
                want_m = RM.mem_bits(want_m)
            else:
                want_t, want_v = OM.forward(x, mu, inv, 5.0, S, *W, act=act, index=index)
            run = PM.rows_run(N, W[0].shape[0], index, mask)
            want_t, want_v = PM.bits(want_t), want_v.copy()
            want_t[~run], want_v[~run] = np.array([T_SENT]).view(np.uint64)[0], V_SENT
            bad = ~np.isfinite(x[:, :Dn]) & run[:, None]
            off_nan, on_nan = off_nan + int((bad & (inv[np.arange(N) // S] == 0)).sum()), on_nan + int((bad & (inv[np.arange(N) // S] != 0)).sum())
            invalid, valid = invalid + int((want_v[run] == 0).sum()), valid + int((want_v[run] == 1).sum())
            norm = policy.ObsNormalizer(M, S, MB, R, clip=5.0, device=DEV)
            norm.mu.copy_(torch.from_numpy(mu))
            norm.inv.copy_(torch.from_numpy(inv))
            free = policy.ObsNormalizer(M, S, MB, R, clip=inf, device=DEV)     # identity tables
            for wide in BUILDS:
                for off in (0, 1):
                    what = "%s N %d S %d %s build %s offset %d" % (shape, N, S, mode, wide, off)
                    got_t, got_v, got_m = normed_forward(torch, policy, norm, MB, R, K, act, x, W, index, mask, reset, wide, off)
                    ne = got_t != want_t
                    assert not ne.any(), "%s: %d targets differ from the law, first at %s" % (what, int(ne.sum()), tuple(np.argwhere(ne)[0]))
                    assert np.array_equal(got_v, want_v), what + ": validity bytes differ"
                    if K:
                        assert np.array_equal(got_m, want_m), what + ": memory differs"
                # identity: the plain kernel's bytes
                idt = normed_forward(torch, policy, free, MB, R, K, act, x, W, index, mask, reset, wide, 0)
                if K:
                    pt, pv, pm = TR_plain(torch, policy, MB, R, K, act, x, W, index, mask, reset, wide)
                    assert np.array_equal(idt[2], pm), "identity tables: memory differs from the plain pass"
                else:
                    pt, pv = TP.run_forward(torch, policy, MB, R, act, x, W, index, mask, wide, 0)
                assert np.array_equal(idt[0], pt) and np.array_equal(idt[1], pv), "identity tables differ from the plain pass (build %s)" % (wide,)
    assert off_nan > 0 and on_nan > 0 and invalid > 0 and valid > 0            # the forge is no vacuous one


def TR_plain(torch, policy_mod, MB, R, K, act, x, W, index, mask, reset, wide):
    """the plain pass with memory over sentinel-filled outputs, as normed_forward reads its own"""
    N, Dn = x.shape[0], OM.width(MB, R)
    rays = None if R in (0, 10) else np.zeros((R, 2)) + 1.0
    pol = policy_mod.RecurrentPolicy(*[torch.from_numpy(a).to(DEV) for a in W], K, activation=act,
                                     index=None if index is None else torch.from_numpy(index).to(DEV), rays=rays)
    obs, frac = split(torch, np.ascontiguousarray(x[:, :Dn]), MB)
    mem = torch.from_numpy(np.ascontiguousarray(x[:, Dn:])).to(DEV)
    out = (torch.full((N, MB), T_SENT, dtype=torch.float64, device=DEV), torch.full((N, MB), V_SENT, dtype=torch.uint8, device=DEV))
    pol.forward(obs, frac, mem, reset=None if reset is None else torch.from_numpy(reset).to(DEV), out=out,
                row_mask=None if mask is None else torch.from_numpy(mask).to(DEV), wide=wide)
    return PM.bits(out[0].cpu().numpy()), out[1].cpu().numpy(), RM.mem_bits(mem.cpu().numpy())


# ----------------------------------------------------------------------------------------------------------------------- act()
ACT_S, ACT_MB, ACT_H, ACT_K = 24, 16, 32, 8


def _act_env(torch, pol, specs, accumulate=True, warm=6):
    """a 64-creature env under `pol` and a normaliser of 3 blocks of 24 (the last one partial) whose tables have seen `warm` steps"""
    from gym_rem2d_amd import policy
    from gym_rem2d_amd.env import BatchedModular2D
    env = BatchedModular2D(seed=4, flags=TR.CONT)
    env.reset_specs(specs)
    norm = policy.ObsNormalizer(3, ACT_S, ACT_MB, 10, min_count=2, device=DEV)
    env.set_policy(pol, normalizer=norm)
    env.step_policy(warm)
    norm.freeze()
    env.set_policy(env.policy, normalizer=norm, accumulate=accumulate)
    return env, norm


def _rows_left(env):
    P = env._policy
    return PM.input_rows(P["obs"].cpu().numpy(), P["frac"].cpu().numpy())


def _model_state(norm):
    st = OM.State(norm.n_blocks, norm.width)
    st.count, st.s1, st.s2hi, st.s2lo = get_state(norm)
    return st


@pytest.mark.parametrize("how", ["accumulate", "apply", "compact"])
def test_act_feed_forward(gpu, how):
    """act() under a normaliser: targets and valid == the law on the obs / frac the call left behind under the tables as they stood;
    the sums moved by exactly those rows (or, without accumulation, not at all); the tables did not move; and every byte of every
    world == a second env brought to the same state that was told the model's targets through set_joint_targets(mask = valid).
    compact: after a compact() that retires every third creature, the rows no live world holds neither contribute nor are written."""
    torch = gpu
    from gym_rem2d_amd import policy
    specs = TR._specs64()
    n = len(specs)
    pol = policy.MLPPolicy.random(n, ACT_MB, ACT_H, seed=41)
    W = tuple(t.numpy() for t in pol.weights)
    (a, na), (b, nb) = (_act_env(torch, pol, specs, accumulate=how != "apply") for _ in range(2))
    try:
        assert int(na.count.min()) >= 6 * (n - 2 * ACT_S) and bool((na.inv != 1).any()) and bool((na.inv == 0).any())
        live = np.ones(n, np.uint8)
        if how == "compact":
            for env in (a, b):
                for w, idx in env.worlds:
                    w.view("frozen")[idx % 3 == 0] = 1
                env.compact(min_envs=1, max_alive=1.0)
            live[:] = 0
            for wi, (w, idx) in enumerate(a.worlds):
                if wi not in a._inactive:
                    live[idx.cpu().numpy()] = 1
            assert 0 < int(live.sum()) <= n - n // 3
            a._policy["targets"][torch.from_numpy(live == 0).to(DEV)] = 77.0
        before, offered = _model_state(na), na.offered
        mu, inv = (t.cpu().numpy().copy() for t in na.tables)
        got_t, got_v = (t.cpu().numpy() for t in a.act())
        x = _rows_left(a)
        want_t, want_v = OM.forward(x, mu, inv, na.clip, ACT_S, *W)
        on = live == 1
        assert np.array_equal(PM.bits(got_t[on]), PM.bits(want_t[on])) and np.array_equal(got_v[on], want_v[on])
        assert (got_t[~on] == 77.0).all()
        want_state = OM.accumulate(before.copy(), x, ACT_S, live) if how != "apply" else before
        for name, g, w in zip(("count", "s1", "s2hi", "s2lo"), get_state(na), want_state.words()):
            assert np.array_equal(g, w), "`%s` after act() (%s)" % (name, how)
        assert na.offered == offered + (ACT_S if how != "apply" else 0)
        assert np.array_equal(OM.tbits(na.mu.cpu().numpy()), OM.tbits(mu)) and np.array_equal(OM.tbits(na.inv.cpu().numpy()), OM.tbits(inv))
        # the joints: b is told the model's targets by hand
        hand_t = torch.from_numpy(np.where(on[:, None], want_t, 0.0)).to(DEV)
        hand_v = torch.from_numpy(np.where(on[:, None], want_v, 0).astype(np.uint8)).to(DEV)
        b.set_joint_targets(hand_t, mask=hand_v)
        TP._same_worlds(TP._world_bytes(a), TP._world_bytes(b), "act() under a normaliser (%s) against set_joint_targets" % how)
        # and the closed loop goes on from there, the same in both
        a.step_policy(2)
        b.step(1)
        b.step_policy(1)
        TP._same_worlds(TP._world_bytes(a), TP._world_bytes(b), "the steps after (%s)" % how)
    finally:
        a.close()
        b.close()


def test_act_recurrent_under_autoreset(gpu):
    """a RecurrentPolicy under a normaliser and set_autoreset: after every act() targets, valid and memory == the law from the memory
    before, zero for who has just restarted; the context words are not normalised; the sums move by the rows observed"""
    torch = gpu
    from gym_rem2d_amd import policy
    specs = TR._specs64()
    n = len(specs)
    pol = policy.RecurrentPolicy.random(n, ACT_MB, ACT_H, ACT_K, seed=43)
    W = tuple(t.numpy() for t in pol.weights)
    env, norm = _act_env(torch, pol, specs)
    try:
        assert not bool(env.policy_memory.any())                   # attaching again zeroed the context
        env.set_autoreset(("steps",), 5)
        fresh = 0
        for i in range(12):
            if i == 6:
                norm.freeze()                                       # new tables mid-way: the next act() stages through them
            prev_mem, ended = env.policy_memory.cpu().numpy().copy(), env.episodes.ended.cpu().numpy().astype(np.uint8)
            before = _model_state(norm)
            mu, inv = (t.cpu().numpy().copy() for t in norm.tables)
            env.step_policy(1)
            x = _rows_left(env)
            wt, wv, wm = OM.forward_memory(x, prev_mem, mu, inv, norm.clip, ACT_S, *W, reset=ended)
            assert np.array_equal(RM.mem_bits(env.policy_memory.cpu().numpy()), RM.mem_bits(wm)), "memory after act() %d" % i
            assert np.array_equal(PM.bits(env._policy["targets"].cpu().numpy()), PM.bits(wt)) and np.array_equal(env._policy["valid"].cpu().numpy(), wv)
            for name, g, w in zip(("count", "s1", "s2hi", "s2lo"), get_state(norm), OM.accumulate(before, x, ACT_S).words()):
                assert np.array_equal(g, w), "`%s` after act() %d" % (name, i)
            fresh += int(ended.sum())
        assert fresh >= 2 * n and int(env.episodes.count.min()) >= 2
    finally:
        env.close()


def test_a_loop_with_a_normaliser(gpu):
    """run_policy_es(normalizer=): every generation freezes once, its episode accumulates; the same call twice gives the same bits;
    run_policy_episode(normalizer=) only applies"""
    torch = gpu
    from gym_rem2d_amd import evaluate, policy
    from gym_rem2d_amd.env import BatchedModular2D
    specs = TR._specs64()
    n = len(specs)
    out = []
    for _ in range(2):
        env = BatchedModular2D(seed=4, flags=TR.CONT)
        env.reset_specs(specs)
        norm = policy.ObsNormalizer(4, 16, ACT_MB, 10, device=DEV)
        mean = policy.MLPPolicy.random(4, ACT_MB, ACT_H, seed=5)
        try:
            seen = []
            new, fit, hist = evaluate.run_policy_es(env, mean, 2, seed=3, group_size=16, max_steps=12, chunk=6, normalizer=norm,
                                                   on_generation=lambda g, c, f, m: seen.append((int(norm.count.min()), norm.mu.clone())))
            assert seen[0][0] == 12 * 16 and seen[1][0] == 24 * 16 and not bool(seen[0][1].any()) and bool(seen[1][1].any())
            assert env._policy["normalizer"] is norm and env._policy["accumulate"]
            count = norm.count.clone()
            evaluate.run_policy_episode(env, max_steps=3, chunk=3, compact=False, normalizer=norm)
            assert torch.equal(norm.count, count) and not env._policy["accumulate"]
            out.append([t.cpu().numpy().copy() for t in new.weights] + [fit.cpu().numpy().copy()] + get_state(norm))
        finally:
            env.close()
    for x, y in zip(*out):
        assert x.tobytes() == y.tobytes()


# ------------------------------------------------------------------------------------------------------ the caller's stream
ST_MB, ST_R, ST_H, ST_K, ST_S, ST_N = 4, 3, 5, 2, 13, 65       # five blocks of 13 rows: 65 rows, two wavefronts' worth for forward
ST_DN = OM.width(ST_MB, ST_R)
STATE = ("count", "s1", "s2hi", "s2lo")


def _st_rows(seed, finite, cols):
    rng = np.random.default_rng([seed, 55])
    x = (rng.standard_normal((ST_N, cols)) * 3.0).astype(f32)
    if not finite:
        x[2, 1] = nan
    return x


def _st_state(seed):
    rng = np.random.default_rng([seed, 56])
    st = OM.accumulate(OM.State(5, ST_DN), (rng.standard_normal((ST_N, ST_DN)) * (seed + 1.0)).astype(f32) + f32(seed), ST_S)
    return st.words()


def _st_tables(seed):
    rng = np.random.default_rng([seed, 57])
    return (rng.standard_normal((5, ST_DN)) * 0.5).astype(f32), np.exp(rng.standard_normal((5, ST_DN))).astype(f32)


def _bind_state(c, norm, inout=True):
    sets = [_st_state(s) for s in (1, 2, 3)]
    for j, name in enumerate(STATE):
        c.bind(name, getattr(norm, name), *(s[j] for s in sets))
        if inout:
            c.inout(name)


def stream_case(torch, wide, which):
    """one of the four array calls through the Python layer, as test_caller_stream_gpu's cases are built: three data sets (A, B and
    a finite decoy), outputs under sentinels, the numpy model as the reference"""
    from gym_rem2d_amd import policy
    c = TCS.Case(torch)
    norm = policy.ObsNormalizer(5, ST_S, ST_MB, ST_R, min_count=3, device=c.dev)
    wd = 8 + 6 * ST_MB
    if which == "accumulate":
        sets = [_st_rows(s, s == 3, ST_DN) for s in (1, 2, 3)]
        obs, frac = c.inp("obs", *(s[:, :wd] for s in sets)), c.inp("frac", *(s[:, wd:] for s in sets))
        _bind_state(c, norm)
        c.call = lambda: norm.accumulate(obs, frac, row_chunk=4, wide=wide)

        def want(key):
            d = c.data[key]
            st = OM.State(5, ST_DN)
            st.count, st.s1, st.s2hi, st.s2lo = (d[k].copy() for k in STATE)
            return OM.accumulate(st, np.concatenate([d["obs"], d["frac"]], axis=1), ST_S).words()
        c.want, c.norm = want, lambda key, got: got
        return c
    if which == "freeze":
        _bind_state(c, norm, inout=False)
        c.out_existing("mu", norm.mu, TCS.F_SENT)
        c.out_existing("inv", norm.inv, TCS.F_SENT)
        c.call = lambda: norm.freeze(wide=wide)
        c.want = lambda key: [OM.tbits(t) for t in OM.freeze(*(c.data[key][k] for k in STATE), 3, norm.min_var)]
        c.norm = lambda key, got: [OM.tbits(t) for t in got]
        return c
    K = ST_K if which == "forward_memory" else 0
    sets = [TCS._forward_inputs(ST_R + K, s, s == 3) for s in (1, 2, 3)]        # (x and the four weight arrays at TCS.SHAPE = (4, 3, 5))
    assert TCS.SHAPE == (ST_MB, ST_R, ST_H) and TCS.N_ROWS == ST_N
    obs, frac = c.inp("obs", *(s[0][:, :wd] for s in sets)), c.inp("frac", *(s[0][:, wd:ST_DN] for s in sets))
    mem = c.inp("memory", *(s[0][:, ST_DN:] for s in sets)) if K else None
    w = [c.inp(n, *(s[1 + i] for s in sets)) for i, n in enumerate(TCS.NAMES4)]
    tabs = [_st_tables(s) for s in (1, 2, 3)]
    c.bind("mu", norm.mu, *(t[0] for t in tabs))
    c.bind("inv", norm.inv, *(t[1] for t in tabs))
    rays = np.zeros((ST_R, 2)) + 1.0
    pol = policy.RecurrentPolicy(*w, K, rays=rays) if K else policy.MLPPolicy(*w, rays=rays)
    out = (c.out("targets", (ST_N, ST_MB), torch.float64, TCS.F_SENT), c.out("valid", (ST_N, ST_MB), torch.uint8, 0xA5))
    if K:
        c.inout("memory")
    c.call = lambda: norm.forward(pol, obs, frac, memory=mem, out=out, wide=wide)

    def want_forward(key):
        d = c.data[key]
        x = np.concatenate([d["obs"], d["frac"]], axis=1)
        Wk = [d[k] for k in TCS.NAMES4]
        if K:
            t, v, m = OM.forward_memory(x, d["memory"], d["mu"], d["inv"], norm.clip, ST_S, *Wk)
            return [PM.bits(t), v.astype(np.uint8), RM.mem_bits(m)]
        t, v = OM.forward(x, d["mu"], d["inv"], norm.clip, ST_S, *Wk)
        return [PM.bits(t), v.astype(np.uint8)]
    c.want = want_forward
    c.norm = lambda key, got: [PM.bits(got[0]), got[1]] + ([RM.mem_bits(got[2])] if K else [])
    return c


def prep_act_normed(env):
    from gym_rem2d_amd import policy
    env.set_policy(policy.RecurrentPolicy.random(TCS.N_POP, TCS.ACT_BODIES, TCS.ACT_HIDDEN, TCS.CONTEXT, seed=3),
                   normalizer=policy.ObsNormalizer(5, 13, TCS.ACT_BODIES, 10, min_count=3, device=TCS.DEVICE))


def mk_act_normed(c, env, rig):
    """rem2d_worlds_act_normed through act(): TCS.mk_act's traces -- obs, frac, targets, valid, memory, the joints' words in the
    arenas -- and the normaliser's: the tables it reads (three data sets) and the sums the extra launch adds to"""
    norm = env._policy["normalizer"]
    Dn = norm.width
    for j, name in enumerate(("mu", "inv")):
        rngs = [np.random.default_rng([s, 58 + j]) for s in (1, 2, 3)]
        c.bind(name, getattr(norm, name), *((r.standard_normal((5, Dn)) * 0.5).astype(f32) if j == 0 else np.exp(r.standard_normal((5, Dn))).astype(f32) for r in rngs))
    for j, name in enumerate(STATE):
        c.bind(name, getattr(norm, name), *(np.random.default_rng([s, 60 + j]).integers(0, 1000, tuple(getattr(norm, name).shape)) for s in (1, 2, 3)))
    TCS.mk_act(c, env, rig)
    for name in STATE:
        c.inout(name)


_CASES = {}


def _stream_case(torch, which, build):
    if (which, build) not in _CASES:
        if which == "act_normed":
            c = TCS._world_case(torch, build, mk_act_normed, True, tag="act_normed", prepare=prep_act_normed)
        else:
            c = stream_case(torch, build, which)
            memo, model = {}, c.want
            c.want = lambda key: memo[key] if key in memo else memo.setdefault(key, model(key))
        _CASES[(which, build)] = c
    return _CASES[(which, build)]


@pytest.fixture(scope="module", autouse=True)
def _cases_released():
    yield
    _CASES.clear()
    for key in [k for k in TCS._RIGS if k[0] == "act_normed"]:
        TCS._RIGS.pop(key).close()


CALLS = ("accumulate", "freeze", "forward", "forward_memory", "act_normed")
STREAM_IDS = [pytest.param(w, b, id="%s-%s" % (w, TCS._bid(b))) for w in CALLS for b in BUILDS]


@pytest.mark.parametrize("which,build", STREAM_IDS)
def test_capture_and_replay(gpu, which, build):
    """The call alone captured on a caller's stream (the stream travels in the descriptor): the capture succeeds -- nothing
    synchronised, allocated through HIP or touched the legacy stream --, nothing ran during it, and each replay computes the
    reference of what the inputs hold then: data set A, then B written in place"""
    torch = gpu
    c = _stream_case(torch, which, build)
    what = "%s (%s build)" % (which, TCS._bid(build))
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
    c.load("B")
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    c.compare("B", what + " second replay")
    del g


@pytest.mark.parametrize("which,build", STREAM_IDS)
def test_behind_a_gate(gpu, gate, which, build):  # noqa: F811
    """test_caller_stream_gpu's gate leg, as it is: the call on a caller's stream behind a spin and the copies that bring its real
    inputs; a launch that went to any other stream reads the decoy"""
    torch = gpu
    c = _stream_case(torch, which, build)
    c.reads_decoy()
    TCS._gated(torch, c, gate)
    what = "%s (%s build) behind the gate" % (which, TCS._bid(build))
    got, decoy = c.norm("decoy", c.read()), c.want("decoy")
    for n, g, d in zip(c.names(), got, decoy):
        assert n in c.insensitive or (np.asarray(g).reshape(-1) != np.asarray(d).reshape(-1)).any(), \
            "%s: `%s` holds the DECOY's result: a launch did not wait for the caller's stream" % (what, n)
    c.compare("A", what)


# ------------------------------------------------------------------------------------------------------------- error paths
def test_refusals_write_nothing(gpu):
    """REM2D_E_INVALID on real device buffers: nothing is written after a refusal -- sums, tables and outputs hold what they held"""
    torch = gpu
    from gym_rem2d_amd import _lib, policy
    norm = policy.ObsNormalizer(2, 4, 2, 1, device=DEV)
    norm.s1.fill_(3)
    norm.mu.fill_(0.5)
    pol = policy.MLPPolicy.random(8, 2, 4, n_rays=1, rays=np.zeros((1, 2)) + 1.0).to(DEV)
    obs, frac = torch.ones((8, 20), device=DEV), torch.ones((8, 1), device=DEV)
    out = (torch.full((8, 2), 9.0, dtype=torch.float64, device=DEV), torch.full((8, 2), 9, dtype=torch.uint8, device=DEV))
    for wide in BUILDS:
        L = _lib.lib(wide)
        n = norm.descriptor()
        n.n_rows, n.obs, n.frac = 9, obs.data_ptr(), frac.data_ptr()
        assert L.rem2d_obsnorm_accumulate(C.byref(n)) == -1 and b"9 rows are more than" in L.rem2d_last_error()
        n.n_rows, n.min_var = 8, 0.0
        assert L.rem2d_obsnorm_freeze(C.byref(n)) == -1 and b"min_var" in L.rem2d_last_error()
        n = norm.descriptor()
        n.clip = nan
        p = pol.descriptor(obs, frac, *out)
        assert L.rem2d_obsnorm_forward(C.byref(n), C.byref(p)) == -1 and b"clip" in L.rem2d_last_error()
    torch.cuda.synchronize()
    assert bool((norm.s1 == 3).all()) and not norm.count.any() and bool((norm.mu == 0.5).all()) and bool((out[0] == 9).all()) and bool((out[1] == 9).all())
