"""The caller-stream contract of the library, function by function: one row per exported function whose declaration in include/*.h
takes a ``void *stream`` ("What 'queued on the caller's stream' covers").

The headers promise of such a function that its work is queued on the caller's stream, that nothing synchronises and that the
library allocates nothing.  A row puts the function in one of three classes:

  queued   it keeps all three promises; tests/test_caller_stream_gpu.py captures the call alone on a caller's stream and replays it,
           and runs it behind a gate on a stream of the caller's
  blocks   it takes a stream and waits on the host; ``says`` quotes the sentence of its header comment that states it
  step     the step family: it owns its capture (REM2D_STEP_GRAPH), its fork / join over step groups and the step train's hand-over;
           test_env_gpu, test_lifecycle_gpu and test_order_gpu cover it on the package's own side streams, and it is NOT run under
           a caller's capture or behind a gate

A ``queued`` row may carry ``blocks_when``: one form of the call that waits on the host, again as a quoted header sentence; the
other forms are held to the contract.  ``via`` names how the GPU test drives a queued row: the public Python method, or "ctypes"
where there is none or the method does more than the call (the row says so).  tests/test_caller_stream_host.py holds the table to
the headers: the key set is exactly the functions that take a stream, and every quoted sentence stands in that function's comment.
The GPU file takes its ids from the queued rows of this table: a row without a case there fails.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

QUEUED, BLOCKS, STEP = "queued", "blocks", "step"


def _q(via):
    return {"class": QUEUED, "via": via}


TABLE = {
    # ---- world reads and writes
    "rem2d_world_reset": _q("ctypes"),                 # (BatchedWorld.reset plans and uploads its tiles first, which blocks)
    "rem2d_world_set_order": dict(_q("BatchedWorld.set_order"), blocks_when=(
        "order_dev NULL", "NULL: back to the identity, and where an order was installed that form blocks: it waits for the whole "
                          "device, then copies from the host.")),
    "rem2d_world_read_order": _q("ctypes"),            # (BatchedWorld.order allocates what it returns)
    "rem2d_world_make_order": _q("BatchedWorld.make_order"),
    "rem2d_world_gather": _q("BatchedWorld.gather"),
    "rem2d_worlds_observe": _q("BatchedModular2D.observe"),
    "rem2d_worlds_control": _q("BatchedModular2D.set_joint_targets"),
    "rem2d_worlds_sense": _q("BatchedModular2D.sense_terrain"),
    "rem2d_worlds_act": _q("BatchedModular2D.act"),
    "rem2d_worlds_act_recurrent": _q("BatchedModular2D.act"),
    "rem2d_worlds_reset_where": _q("BatchedModular2D.reset_where"),
    "rem2d_worlds_refill": _q("BatchedModular2D.refill"),
    "rem2d_worlds_describe": _q("BatchedModular2D.describe"),
    # ---- policies and their evolution
    "rem2d_policy_forward": _q("MLPPolicy.forward"),
    "rem2d_recurrent_forward": _q("RecurrentPolicy.forward"),
    "rem2d_policy_select": _q("ctypes"),
    "rem2d_policy_vary": _q("MLPPolicy.evolve(parents=)"),
    "rem2d_policy_evolve": _q("MLPPolicy.evolve"),
    # ---- evolution strategies
    "rem2d_es_sample": _q("MLPPolicy.es_sample"),
    "rem2d_es_shape": _q("ctypes"),
    "rem2d_es_update": _q("MLPPolicy.es_update(util=)"),
    "rem2d_es_step": _q("MLPPolicy.es_update"),
    "rem2d_snes_sample": _q("SeparableES.sample"),
    "rem2d_snes_update": _q("SeparableES.update(util=)"),
    "rem2d_snes_step": _q("SeparableES.update"),
    # ---- novelty, elites, Pareto
    "rem2d_novelty_score": _q("NoveltyArchive.score"),
    "rem2d_novelty_add": _q("NoveltyArchive.add"),
    "rem2d_novelty_step": _q("NoveltyArchive.step"),
    "rem2d_elites_insert": _q("EliteGrid.insert"),
    "rem2d_elites_sample": _q("EliteGrid.sample"),
    "rem2d_elites_emit": _q("EliteGrid.emit"),
    "rem2d_pareto_rank": _q("pareto.rank"),
    "rem2d_pareto_local": _q("pareto.local_competition"),
    # ---- others
    "rem2d_tree_diversity": _q("ctypes"),
    "rem2d_selftest_scalar": _q("ctypes"),
    "rem2d_selftest_geometry": _q("ctypes"),
    # ---- takes a stream and waits on the host
    "rem2d_world_render": {"class": BLOCKS, "says": "read back to the host and checked (a synchronising copy on `stream`)"},
    # ---- the step family
    "rem2d_world_step": {"class": STEP},
    "rem2d_world_step_ex": {"class": STEP},
    "rem2d_worlds_step": {"class": STEP},
    "rem2d_worlds_step_ex": {"class": STEP},
    "rem2d_groups_step": {"class": STEP},
    "rem2d_groups_step_ex": {"class": STEP},
}


def rows(cls):
    return sorted(n for n, r in TABLE.items() if r["class"] == cls)


# ----------------------------------------------------------------------------------------------------------- reading the headers
_COMMENT = re.compile(r"/\*.*?\*/", re.S)
_DECL = re.compile(r"\b(rem2d_[a-z_0-9]+)\s*\(([^;{}()]*)\)\s*;")
_STREAM = re.compile(r"\bvoid\s*\*\s*stream\b")


def _plain(comment):
    """a comment's words: the frame of stars gone, white space collapsed"""
    body = re.sub(r"\n\s*\*(?!/)", "\n", comment[2:-2])
    return " ".join(body.split())


def declared(include=None):
    """{function: (header file name, its parameter list, the words of the comment in front of its declaration)} for every function
    declared in include/*.h; the comment of a declaration is the last one that ends in front of it."""
    out = {}
    for path in sorted(glob.glob(os.path.join(include or os.path.join(ROOT, "include"), "*.h"))):
        text = open(path).read()
        comments = [(m.start(), m.end(), m.group(0)) for m in _COMMENT.finditer(text)]
        code = _COMMENT.sub(lambda m: re.sub(r"[^\n]", " ", m.group(0)), text)   # same offsets, comments blanked
        for m in _DECL.finditer(code):
            before = [c for c in comments if c[1] <= m.start()]
            out[m.group(1)] = (os.path.basename(path), m.group(2), _plain(before[-1][2]) if before else "")
    return out


def stream_takers(include=None):
    """the functions whose parameter list has a `void *stream`"""
    return sorted(n for n, (_, params, _) in declared(include).items() if _STREAM.search(params))


def quoted(name):
    """the header sentences a row quotes"""
    r = TABLE[name]
    return ([r["says"]] if r["class"] == BLOCKS else []) + ([r["blocks_when"][1]] if "blocks_when" in r else [])
