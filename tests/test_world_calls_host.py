"""The refusal chains of the closed-loop host layer (csrc/rem2d.hip, `closed-loop control` .. rem2d_worlds_refill, rem2d_worlds_describe
and the observation-normalisation act block), pinned without a GPU against tests/golden/world_call_refusals.json: which of several
faults a call names first, with which code and in which words.

A chain is made like this: start from a call with every fault present at once; record the return code and the whole
rem2d_last_error text; repair the fault that text names (REPAIRS: the first unused row whose needle the text holds); repeat until the
call is taken or stops at the first check that needs a real world.  One list is then the call's whole precedence order.  A text
that no row repairs ends the chain where it stands, so a changed word shows as a chain that differs from the record.

Host half (here): one argument-level chain for each of the nine rem2d_worlds_* calls, on fake pointers that are never dereferenced
and a world list whose only entry is NULL -- "world 0 is NULL" is the last refusal that needs no world -- and one for each of
rem2d_policy_forward, rem2d_recurrent_forward, rem2d_obsnorm_forward and rem2d_obsnorm_forward_memory, which end at "too many rows
for one launch" or "rows are more than" and then, with no row left, are taken without a launch.  A message does not depend on the
build: the three builds are held to the one record.

GPU half (tests/test_world_tables_gpu.py, test_refusal_chains): the world-level chains of the same nine calls on real handles; its
walker lives there, its record under "gpu" in the same file.

The record was made by this file's `--record` mode on an MI355X (the GPU half needs one) from the library as it was before the nine
calls were put on shared helpers; the test never makes it again."""
import ctypes as C
import json
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "world_call_refusals.json")
BUF = 256                                     # a "device pointer" that is never dereferenced
STOP = "world 0 is NULL"
ROWS_TOO_MANY = 1 << 40


class State:
    """the arguments of one call, all faulty at first"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _set(**kw):
    return lambda s: s.__dict__.update(kw)


def _fix_d(s):
    s.p.d = 8 + 6 * s.p.max_bodies + s.p.n_rays + (s.context if hasattr(s, "context") else s.n.context if hasattr(s, "n") else 0)


def _memory(s):
    s.memory = BUF
    if hasattr(s, "n"):
        s.n.memory = BUF


def _policy_pointers(s):
    for k in ("w1", "b1", "w2", "b2", "obs", "frac", "targets", "valid"):
        setattr(s.p, k, BUF)


def _p(**kw):
    def fix(s):
        for k, v in kw.items():
            setattr(s.p, k, v)
    return fix


def _n(**kw):
    def fix(s):
        for k, v in kw.items():
            setattr(s.n, k, v)
    return fix


def _match_normaliser(s):
    s.n.max_bodies, s.n.n_rays = s.p.max_bodies, s.p.n_rays


def _bad_policy(_lib):
    p = _lib.Policy()
    p.max_bodies, p.n_rays, p.hidden, p.d, p.activation, p.n_sets, p.n_rows = 0, -1, 0, 0, 7, 0, -1
    return p


def _bad_normaliser(_lib):
    n = _lib.Obsnorm()
    n.max_bodies, n.n_rays, n.n_blocks, n.group_size, n.row_chunk, n.context, n.reserved, n.clip = 0, -1, 0, 0, -1, -1, 1, 0.0
    return n


WORLDS = [("no worlds", _set(worlds=True))]
TABLE = [("NULL device pointer", _set(buf=BUF)), ("max_bodies must be", _set(max_bodies=4)), ("negative row count", _set(rows=1))]


def policy_rows(rows_then):
    """the faults of a rem2d_policy in the order policy_ok names them; n_rows: -1, then `rows_then`"""
    return [("NULL policy", _set(have_p=True)), ("max_bodies must be", _p(max_bodies=16)), ("n_rays must be", _p(n_rays=60)),
            ("n_rays + context must be", _p(n_rays=10)), ("hidden must be", _p(hidden=32)), ("d must be", _fix_d),
            ("unknown activation", _p(activation=0)), ("n_sets must be", _p(n_sets=3)), ("negative row count", _p(n_rows=rows_then)),
            ("NULL device pointer (ray offsets)", _set(rays=BUF)), ("NULL device pointer (memory)", _memory),
            ("NULL device pointer (mu)", _n(mu=BUF)), ("NULL device pointer (inv)", _n(inv=BUF)),
            ("NULL device pointer (count)", _n(count=BUF + 4)), ("count must be 8-byte aligned", _n(count=BUF)),
            ("NULL device pointer (s1)", _n(s1=BUF)), ("NULL device pointer (s2hi)", _n(s2hi=BUF)), ("NULL device pointer (s2lo)", _n(s2lo=BUF)),
            ("NULL device pointer", _policy_pointers), ("without an index", _p(index=BUF)),
            ("too many rows for one launch", _p(n_rows=0))]


RECURRENT = [("NULL recurrent policy", _set(have_p=True)), ("context must be 1..hidden", _set(context=8)),
             ("reserved must be 0", _set(reserved=0))]


def normaliser_rows(context_then, rows_then):
    """the faults of a rem2d_obsnorm in the order on_ok names them, before policy_rows: a needle both hold is the normaliser's first"""
    return [("NULL descriptor", _set(have_n=True)), ("max_bodies must be", _n(max_bodies=8)), ("n_rays must be", _n(n_rays=3)),
            ("n_blocks must be", _n(n_blocks=1 << 30)), ("group_size must be", _n(group_size=1 << 20)),
            ("n_blocks * group_size must be", _n(group_size=1)), ("n_blocks times the words", _n(n_blocks=4)),
            ("row_chunk must be", _n(row_chunk=0)), ("reserved must be 0", _n(reserved=0)), ("clip must be", _n(clip=5.0)),
            ("context must be at least 0", _n(context=context_then)), ("context must be 0 for", _n(context=0)),
            ("context must be 1..hidden", _n(context=8)), ("the policy has max_bodies", _match_normaliser),
            ("rows are more than", _p(n_rows=rows_then))]


def _worlds(s):
    return ((C.c_void_p * 1)(None), 1) if s.worlds else (None, 0)


def _recurrent(_lib, s):
    q = _lib.Recurrent()
    q.p, q.context, q.reserved, q.memory = s.p, s.context, s.reserved, s.memory
    return q


def entries(_lib, L):
    """{entry point: (call(state) -> rc, the faulty state, REPAIRS)} -- every state is made afresh"""
    def observe(s):
        return L.rem2d_worlds_observe(*_worlds(s), s.max_bodies, s.buf, s.rows, None)

    def control(s):
        return L.rem2d_worlds_control(*_worlds(s), s.mode, s.buf, s.max_bodies, s.rows, None, None)

    def sense(s):
        return L.rem2d_worlds_sense(*_worlds(s), s.buf, s.n_rays, s.buf, None, s.rows, None)

    def describe(s):
        return L.rem2d_worlds_describe(*_worlds(s), s.period, s.n_samples, s.buf, s.rows, None)

    def act(s):
        return L.rem2d_worlds_act(*_worlds(s), C.byref(s.p) if s.have_p else None, s.rays, None)

    def act_recurrent(s):
        return L.rem2d_worlds_act_recurrent(*_worlds(s), C.byref(_recurrent(_lib, s)) if s.have_p else None, s.rays, None)

    def act_normed(s):
        return L.rem2d_worlds_act_normed(*_worlds(s), C.byref(s.n) if s.have_n else None, C.byref(s.p) if s.have_p else None, s.rays, 1)

    def reset_where(s):
        w, n = _worlds(s)
        return L.rem2d_worlds_reset_where(w, C.byref(s.morphs) if s.have_morphs else None, n, s.mask, s.when, s.max_steps, None, s.rows, None)

    def refill(s):
        w, n = _worlds(s)
        return L.rem2d_worlds_refill(w, C.byref(s.morphs) if s.have_morphs else None, n, C.byref(s.feeds) if s.have_feeds else None,
                                     s.occupant, s.when, s.max_steps, None, s.ids, s.rows, None)

    def policy_forward(s):
        return L.rem2d_policy_forward(C.byref(s.p) if s.have_p else None, None)

    def recurrent_forward(s):
        return L.rem2d_recurrent_forward(C.byref(_recurrent(_lib, s)) if s.have_p else None, None)

    def obsnorm_forward(s):
        return L.rem2d_obsnorm_forward(C.byref(s.n) if s.have_n else None, C.byref(s.p) if s.have_p else None)

    def obsnorm_forward_memory(s):
        return L.rem2d_obsnorm_forward_memory(C.byref(s.n) if s.have_n else None, C.byref(s.p) if s.have_p else None)

    def table_state(**kw):
        return State(worlds=False, buf=None, max_bodies=0, rows=-1, **kw)

    def policy_state(**kw):
        return State(worlds=False, have_p=False, p=_bad_policy(_lib), rays=None, **kw)

    when = [("unknown bits in `when`", _set(when=0)), ("no mask and no condition", _set(when=4)), ("no condition (`when` == 0)", _set(when=4)),
            ("needs max_steps > 0", _set(max_steps=9)), ("negative row count", _set(rows=1))]
    morphs = [("NULL morphologies", _set(have_morphs=True))]
    return {
        "rem2d_worlds_observe": (observe, table_state(), WORLDS + TABLE),
        "rem2d_worlds_control": (control, table_state(mode=2), [("unknown mode", _set(mode=0))] + WORLDS + TABLE),
        "rem2d_worlds_sense": (sense, table_state(n_rays=0), WORLDS + [("n_rays must be", _set(n_rays=10))] + TABLE),
        "rem2d_worlds_describe": (describe, table_state(period=0, n_samples=0),
                                  [("period must be", _set(period=15)), ("n_samples must be", _set(n_samples=4))] + WORLDS + TABLE),
        "rem2d_worlds_act": (act, policy_state(), WORLDS + policy_rows(5)),
        "rem2d_worlds_act_recurrent": (act_recurrent, policy_state(context=0, reserved=1, memory=None), WORLDS + RECURRENT + policy_rows(5)),
        "rem2d_worlds_act_normed": (act_normed, policy_state(have_n=False, n=_bad_normaliser(_lib)),
                                    WORLDS + normaliser_rows(3, 3) + policy_rows(5)),
        # (`when`: 8, an unknown bit; then 0, no condition; then 4, REM2D_WHEN_STEPS, with max_steps 0)
        "rem2d_worlds_reset_where": (reset_where, State(worlds=False, have_morphs=False, morphs=_lib.Morph(), mask=None, when=8, max_steps=0, rows=-1),
                                     WORLDS + morphs + when),
        "rem2d_worlds_refill": (refill, State(worlds=False, have_morphs=False, morphs=_lib.Morph(), have_feeds=False, feeds=_lib.Feed(),
                                              occupant=None, when=8, max_steps=0, rows=-1, ids=-1),
                                WORLDS + morphs + [("NULL feeds", _set(have_feeds=True)), ("NULL occupant array", _set(occupant=BUF)),
                                                   ("negative id count", _set(ids=1))] + when),
        "rem2d_policy_forward": (policy_forward, policy_state(), policy_rows(ROWS_TOO_MANY)),
        "rem2d_recurrent_forward": (recurrent_forward, policy_state(context=0, reserved=1, memory=None), RECURRENT + policy_rows(ROWS_TOO_MANY)),
        "rem2d_obsnorm_forward": (obsnorm_forward, policy_state(have_n=False, n=_bad_normaliser(_lib)),
                                  normaliser_rows(3, 0) + policy_rows(ROWS_TOO_MANY)),
        "rem2d_obsnorm_forward_memory": (obsnorm_forward_memory, policy_state(have_n=False, n=_bad_normaliser(_lib)),
                                         normaliser_rows(0, 0) + policy_rows(ROWS_TOO_MANY)),
    }


def chain(call, error_text, state, repairs, taken=lambda state: False, limit=64):
    """[[return code, text], ...] of `call` from `state` down REPAIRS; ends with a call that is taken (code 0, no text), at STOP, at a
    text no unused row repairs, or -- `taken(state)`: the call would proceed -- without making that call"""
    out, used = [], set()
    while len(out) < limit and not taken(state):
        rc = int(call(state))
        text = error_text() if rc else ""
        out.append([rc, text])
        if rc == 0 or text.endswith(STOP):
            break
        for k, (needle, fix) in enumerate(repairs):
            if k not in used and needle in text:
                used.add(k)
                fix(state)
                break
        else:
            break
    return out


def walk(_lib, L):
    L.rem2d_last_error.restype = C.c_char_p
    return {name: chain(call, lambda: L.rem2d_last_error().decode("ascii"), state, repairs)
            for name, (call, state, repairs) in entries(_lib, L).items()}


def test_every_chain_is_the_recorded_one():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    with open(GOLDEN) as f:
        want = json.load(f)["host"]
    # the record is no vacuous yardstick: 13 calls, every chain ends where it should, the long ones are long
    assert len(want) == 13 and sum(len(v) for v in want.values()) > 150
    for name, rows in want.items():
        last = rows[-1]
        assert last == ([0, ""] if "_worlds_" not in name else [-1, "%s: %s" % (rows[0][1].split(":")[0], STOP)]), name
        # (a normaliser and its policy may be refused in the same words one after the other's repair: never twice in a row)
        assert all(rc == -1 for rc, _ in rows[:-1]) and all(a != b for a, b in zip(rows, rows[1:])), name
    assert len(want["rem2d_worlds_act_normed"]) > 30 and len(want["rem2d_worlds_refill"]) == 10 and len(want["rem2d_worlds_reset_where"]) == 7
    for wide in (False, True, "fma"):
        got = walk(_lib, _lib.lib(wide))
        assert sorted(got) == sorted(want)
        for name in want:
            for i, (a, b) in enumerate(zip(got[name], want[name])):
                assert a == b, "%s (build %r), link %d: %r, the record has %r" % (name, wide, i, a, b)
            assert len(got[name]) == len(want[name]), name


if __name__ == "__main__" and sys.argv[1:2] == ["--record"]:
    # python tests/test_world_calls_host.py --record [FILE]: both halves of the record, so on a machine with an MI355X.  A record that
    # exists is what the calls are held to: a changed refusal is a failure of the tests, not a reason to record again.
    path = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    if os.path.exists(path) or os.path.exists(GOLDEN):
        sys.exit("%s exists; it is not overwritten" % (path if os.path.exists(path) else GOLDEN))
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
    from gym_rem2d_amd import _lib
    record = {"host": walk(_lib, _lib.lib())}
    for name, rows in record["host"].items():
        print(name)
        for rc, text in rows:
            print("   %2d %s" % (rc, text))
    import torch
    if not torch.cuda.is_available():
        sys.exit("no GPU: the record holds the chains on real worlds too, and is written only with them")
    import test_world_tables_gpu as G
    record["gpu"], record["gpu_left_out"] = G.record_chains(torch), G.LEFT_OUT
    with open(path, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d host links, %d links on real worlds" % (sum(len(v) for v in record["host"].values()),
                                                      sum(len(c) for v in record["gpu"].values() for c in v.values())))
