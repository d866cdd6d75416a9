"""The refusals of the seven search tiers (evolve, es, snes, novelty, elites, cvt, pareto), pinned byte for byte without a GPU: the
return code and the whole rem2d_last_error text of every case the tiers' host tests hold, through every entry point of its tier
(the calls a case was not written for included), of every pair of neighbouring cases at once (which of two faults wins), of every
pointer of the descriptor set to NULL, of every *_scratch_bytes and of the NULL descriptor, against tests/golden/refusals.json.

The tables and the `_desc` builders are the host tests' own, imported.  The record was made by this file's `--record` mode from the
libraries as they were before the validators were rewritten on shared helpers; a message does not depend on the build, so the three
builds are held to the one record.

Nothing here reaches a launch: every descriptor walked through a launching entry point also carries a fault of that call's LAST
check -- the last pair its validator tests for overlap, or the scratch one byte short where that check is the last -- so that a
case's own fault shows wherever the call looks at it and every other case runs the whole validator.  A case's members win over that
fault (with two exceptions, `with_last`), and the recorder refuses to write a record in which a call was not REM2D_E_INVALID."""
import ctypes as C
import json
import os
import sys

import test_cvt_host as CV
import test_elites_host as EL
import test_es_host as ES
import test_evolve_host as EV
import test_novelty_host as NV
import test_pareto_host as PA
import test_snes_host as SN

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refusals.json")


def _kws(*tables, **base):
    """the descriptor changes of case tables of (kw, message) rows, each over `base`"""
    return [dict(base, **row[0]) for table in tables for row in table]


def _nulls(pointers):
    return [{k: None} for k in pointers]


def _merge(a, b):
    """two cases at once; elites' per-dimension members ({index: value}) are merged member by member"""
    out = dict(a)
    for k, v in b.items():
        out[k] = {**out[k], **v} if isinstance(v, dict) and isinstance(out.get(k), dict) else v
    return out


# One case of this file's own, which no table of test_snes_host.py holds: an output that meets an input AND an output before it.  snes
# tests an output against every input first: the scratch on new_m2_b2, with util right behind new_m2_b2, "overlaps util".
SN_ORDER = [dict(pair_chunk=2, scratch=SN._at("new_m2_b2"), util=SN._at("new_m2_b2") + SN.SET_BYTES["b2"])]
EV_POINTERS = ("fitness", "w1", "b1", "w2", "b2", "child_w1", "child_b1", "child_w2", "child_b2", "parent")
# tier: (_desc, cases, {entry point: (takes a stream, the fault of its last check)}, scratch_bytes entry point)
TIERS = {
    "evolve": (EV._desc, _kws(EV.SHAPE_CASES, EV.WEIGHT_CASES) + _nulls(EV_POINTERS),
               {"rem2d_policy_select": (True, dict(fitness=None)), "rem2d_policy_vary": (True, dict(child_b2=5 << 26)),
                "rem2d_policy_evolve": (True, dict(child_b2=5 << 26))}, None),
    "es": (ES._desc, _kws(ES.SHAPE_CASES, ES._overlaps("child", ES.CHILD_W1_BYTES), ES._overlaps("new", ES.W1_BYTES))
           + _kws(ES.SCRATCH_CASES, pair_chunk=2) + _nulls(ES.POINTERS),
           {"rem2d_es_sample": (True, dict(child_b2=6 << 26)), "rem2d_es_shape": (True, dict(util=None)),
            "rem2d_es_update": (True, dict(pair_chunk=2, scratch_bytes=ES.NEED - 1)),
            "rem2d_es_step": (True, dict(pair_chunk=2, scratch_bytes=ES.NEED - 1))}, "rem2d_es_scratch_bytes"),
    "snes": (SN._desc, _kws(SN.SHAPE_CASES, SN.SAMPLE_OVERLAPS, SN.UPDATE_OVERLAPS, SN.STEP_OVERLAPS) + _kws(SN.SCRATCH_CASES, pair_chunk=2)
             + [dict(sigma_min=lo, sigma_max=hi) for lo, hi in SN.SIGMA_BOUNDS] + _nulls(SN.POINTERS) + SN_ORDER,
             {"rem2d_snes_sample": (True, dict(child_b2=SN._at("child_w2"))),
              # (the last pair of all: the last output, the scratch, on the output before it -- after every input and every other output)
              "rem2d_snes_update": (True, dict(pair_chunk=2, scratch=SN._at("new_m2_b2"))),
              "rem2d_snes_step": (True, dict(pair_chunk=2, scratch=SN._at("new_m2_b2")))}, "rem2d_snes_scratch_bytes"),
    "novelty": (NV._desc, _kws(NV.SHAPE_CASES, NV.SCORE_CASES) + _nulls(NV.POINTERS),
                {"rem2d_novelty_score": (True, dict(novelty=1 << 26)), "rem2d_novelty_add": (True, dict(archive=(1 << 26) + 8)),
                 "rem2d_novelty_step": (True, dict(novelty=1 << 26))}, None),
    "elites": (EL._desc, _kws(EL.SHAPE_CASES, EL.SCRATCH_CASES, EL.INSERT_CASES, EL.SAMPLE_CASES, EL.EMIT_CASES) + _nulls(EL.POINTERS),
               {"rem2d_elites_insert": (True, dict(scratch_bytes=EL.NEED - 1)), "rem2d_elites_sample": (True, dict(scratch_bytes=EL.NEED - 1)),
                "rem2d_elites_emit": (True, dict(scratch_bytes=EL.NEED - 1))}, "rem2d_elites_scratch_bytes"),
    # (cvt's tables are sums, ASSIGN = ASSIGN_SHAPES + SCRATCH + ROWS + its own and so on: the slices are the rows of their own)
    "cvt": (CV._desc, _kws(CV.SHAPES, CV.SCRATCH, CV.ROWS, CV.ASSIGN[len(CV.ASSIGN_SHAPES + CV.SCRATCH + CV.ROWS):],
                           CV.INSERT[len(CV.SHAPES + CV.SCRATCH + CV.ROWS):], CV.LINE[len(CV.SHAPES + CV.SCRATCH):]) + _nulls(CV.POINTERS),
            {"rem2d_cvt_assign": (False, dict(scratch_bytes=8 * CV.R_ - 1)),
             "rem2d_cvt_insert": (False, dict(scratch_bytes=12 * CV.M_ * CV.C_ + 8 * CV.G_ - 1)),
             "rem2d_cvt_emit_line": (False, dict(scratch_bytes=12 * CV.M_ * CV.C_ - 1))}, "rem2d_cvt_scratch_bytes"),
    "pareto": (PA._desc, _kws(PA.BOTH_CASES, PA.RANK_CASES, PA.LOCAL_CASES) + _nulls(PA.POINTERS),
               {"rem2d_pareto_rank": (True, dict(n_fronts=PA.AT["obj"] + 8)), "rem2d_pareto_local": (True, dict(neighbours=PA.AT["fitness"] + 4))},
               None),
}
OPTIONAL = ("n_fronts", "neighbours")      # pareto's last checks are on outputs that may be NULL: nothing mandatory comes as late


def walk(L):
    """{entry point: [[return code, message], ...]} of library L, in the order of the tables"""
    L.rem2d_last_error.restype = C.c_char_p
    out = {}

    def call(fn, desc, stream):
        args = (None if desc is None else C.byref(desc),) + ((None,) if stream else ())
        rc = int(fn(*args))
        return [rc, L.rem2d_last_error().decode("ascii") if rc < 0 else ""]       # (a call that succeeds leaves the text alone)

    def with_last(last, kw):
        # the case's members win, but never a scratch that is long enough for this call, nor a NULL that takes away a last check's
        # buffer where that buffer is optional (a NULL anywhere else is refused as such)
        both = _merge(last, kw)
        for k, v in last.items():
            if k == "scratch_bytes" and k in kw:
                both[k] = min(v, kw[k])
            elif k in OPTIONAL and kw.get(k, v) is None:
                both[k] = v
        return both

    for tier, (desc, cases, entries, scratch_bytes) in TIERS.items():
        walked = cases + [_merge(a, b) for a, b in zip(cases, cases[1:])]
        for name, (stream, last) in entries.items():
            fn = getattr(L, name)
            out[name] = [call(fn, None, stream)] + [call(fn, desc(**with_last(last, kw)), stream) for kw in walked]
        if scratch_bytes:
            fn = getattr(L, scratch_bytes)
            out[scratch_bytes] = [call(fn, None, False)] + [call(fn, desc(**kw), False) for kw in walked]
    return out


def described(name, i):
    """what entry `i` of an entry point's list was: for a failure's message"""
    for tier, (desc, cases, entries, scratch_bytes) in TIERS.items():
        if name in entries or name == scratch_bytes:
            walked = cases + [_merge(a, b) for a, b in zip(cases, cases[1:])]
            return "the NULL descriptor" if i == 0 else repr(walked[i - 1])


def test_every_refusal_is_the_recorded_one():
    import __graft_entry__ as g
    g.build()
    from gym_rem2d_amd import _lib
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sum(len(v) for v in want.values()) > 3000 and len(want) == 25
    for wide in (False, True, "fma"):
        got = walk(_lib.lib(wide))
        assert sorted(got) == sorted(want)
        for name in want:
            assert len(got[name]) == len(want[name]), name
            for i, (a, b) in enumerate(zip(got[name], want[name])):
                assert a == b, "%s (build %r) on %s: %r, the record has %r" % (name, wide, described(name, i), a, b)


if __name__ == "__main__" and sys.argv[1:2] == ["--record"]:
    # python tests/test_refusal_text_host.py --record [--overwrite]: the record of the package's library (REM2D_LIB_PATH names
    # another).  A record that exists is what the validators are held to: it is replaced only where a change of the walk (new
    # cases, a new tier) asks for it, from a library whose refusals are known to be right, and only with --overwrite.
    if os.path.exists(GOLDEN) and "--overwrite" not in sys.argv[2:]:
        sys.exit("%s exists; a changed refusal is a failure of the test, not a reason to record again (--overwrite to replace it)" % GOLDEN)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from gym_rem2d_amd import _lib
    record = walk(_lib.lib())
    for name, rows in record.items():
        for i, (rc, text) in enumerate(rows):
            launching = not name.endswith("_scratch_bytes")
            assert rc == -1 if launching else (rc == -1 or rc >= 0), "%s on %s was not refused as invalid: %d %r" % (name, described(name, i), rc, text)
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join('"%s":%s' % (k, json.dumps(record[k], separators=(",", ":"))) for k in sorted(record)) + "\n}\n")
    print("%d entries over %d entry points" % (sum(len(v) for v in record.values()), len(record)))
