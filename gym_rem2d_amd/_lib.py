"""ctypes binding of the C ABI in include/rem2d.h (librem2d.so, HIP/gfx950).

The product path has no CPU fallback: if the library is missing this raises, loudly.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("REM2D_LIB_PATH") or os.path.join(_HERE, "librem2d.so")   # override: A/B builds on the GPU box
# the same source built with -DREM2D_WIDE (32 pair slots / 12 solver slots per body): where the creatures that overflowed the
# default build's slots are re-evaluated (evaluate.run_episode) -- Box2D itself has no cap (Modular2DEnv.py:634)
WIDE_LIB_PATH = os.environ.get("REM2D_WIDE_LIB_PATH") or os.path.join(_HERE, "librem2d_wide.so")
# the same source built with -ffp-contract=fast: the compiler fuses a * b + c into v_fma_f32 wherever it likes.  NOT the bit-exact
# product: a labelled TOLERANCE MODE (north_star: "within a stated fp32 tolerance on positions/velocities") that
# tests/test_parity_gpu.py validates transition by transition against the strict build and bench.py reports as a secondary line
# beside the strict headline.  Selected with wide="fma" wherever a `wide` argument is taken.
FMA_LIB_PATH = os.environ.get("REM2D_FMA_LIB_PATH") or os.path.join(_HERE, "librem2d_fma.so")
SRC_PATH = os.path.join(_HERE, "csrc", "rem2d.hip")

FLAG_CONTINUOUS = 1
FLAG_SLEEP_RESET_ALWAYS = 2
FLAG_NO_SLEEP = 4
FLAG_SKIP_FROZEN = 8
FLAG_RETILE = 16

CONTACT_SLOTS = 24
MAX_WORLDS_PER_STEP = 8
MAX_STEP_GROUPS = 16
STEP_GRAPH = 1
SOLVER_SLOTS = 6
ERR_PAIR_OVERFLOW = 1
ERR_SOLVER_OVERFLOW = 2
ERR_HANDOVER = 4   # (the step train's hand-over check, include/rem2d.h)
ERR_CAPACITY = ERR_PAIR_OVERFLOW | ERR_SOLVER_OVERFLOW


def train_fault(step, every_block=1, drop=False):
    """Value of the `train_fault` test option (REM2D_OPT_TRAIN_FAULT): the workgroups of step `step` (1-based inside a launch) of
    the blocks with block % every_block == 0 are told that their hand-over failed / (drop) never get their flag."""
    return int(step) | (int(every_block) << 16) | ((1 << 30) if drop else 0)

# launch options of a world (include/rem2d.h REM2D_OPT_*, rem2d_world_set_option): no result depends on them
OPTIONS = ("pipeline", "fuse_velpost", "prio", "prio_t1", "prio_t2", "heavy_per_wave", "debug", "rebalance", "train_fault")
OPTION_ID = {n: i for i, n in enumerate(OPTIONS)}
_ENV_OPTIONS = {"REM2D_PIPELINE": "pipeline", "REM2D_FUSE_VELPOST": "fuse_velpost", "REM2D_PRIO": "prio",
                "REM2D_PRIO_T1": "prio_t1", "REM2D_PRIO_T2": "prio_t2", "REM2D_HEAVY_PER_WAVE": "heavy_per_wave",
                "REM2D_V4_DBG": "debug", "REM2D_REBALANCE_DEV": "rebalance", "REM2D_TRAIN_FAULT": "train_fault"}


def env_options():
    """Experiment overrides for bench.py and tools/: REM2D_PIPELINE, REM2D_FUSE_VELPOST, REM2D_PRIO, REM2D_PRIO_T1 / _T2,
    REM2D_HEAVY_PER_WAVE, REM2D_V4_DBG from the environment as {option: value} -- what BatchedWorld hands to
    rem2d_world_set_option for every world it creates.  The LIBRARY reads no environment variable; this is the only place
    where the variables mean anything."""
    return {opt: int(os.environ[var]) for var, opt in _ENV_OPTIONS.items() if os.environ.get(var, "") != ""}


def env_tile_shape():
    """REM2D_TILE_SHAPE (0 .. 4) as an experiment override of the tile shape, or None."""
    v = os.environ.get("REM2D_TILE_SHAPE", "")
    return int(v) if v != "" else None


def env_tile_creatures():
    """REM2D_TILE_CREATURES: cap on the creatures per velocity tile (rem2d_plan_tiles' max_creatures), 0 = the default."""
    v = os.environ.get("REM2D_TILE_CREATURES", "")
    return int(v) if v != "" else 0

# field ids: order of the enum in include/rem2d.h
FIELDS = [
    "px", "py", "ang", "vx", "vy", "w", "sleept", "hx", "hy", "invm", "invi",
    "fatlx", "fatly", "fatux", "fatuy",
    "jax", "jay", "jbx", "jby", "jtorque", "jlower", "jupper",
    "jimpx", "jimpy", "jimpz", "jmotorimp", "jmotorspeed",
    "shape", "parent", "jround", "awake", "jlimit", "ccount",
    "camp", "cphase", "cfreq", "coffset", "cistate",
    "cedge", "cinfo", "ckey0", "ckey1", "cn0", "cn1", "ct0", "ct1",
    "wod", "fitness", "reward", "done", "everdone", "frozen", "steps", "invdt0",
    "newfix", "err", "positers", "toievents",
]
FIELD_ID = {n: i for i, n in enumerate(FIELDS)}

MORPH_FIELDS = ("shape", "hx", "hy", "x", "y", "angle", "parent", "jround", "ax", "ay", "bx", "by", "torque",
                "lower", "upper", "amp", "phase", "freq", "offset", "istate")


RENDER_ABI_VERSION = 1      # include/rem2d_render.h
RENDER_MAX_SIZE = 8192      # REM2D_RENDER_MAX_SIZE
CONTROL_ABI_VERSION = 1     # include/rem2d_control.h
SENSE_ABI_VERSION = 1       # include/rem2d_sense.h
SENSE_MAX_RAYS = 64         # REM2D_SENSE_MAX_RAYS
POLICY_ABI_VERSION = 1      # include/rem2d_policy.h
POLICY_MAX_HIDDEN = 128     # REM2D_POLICY_MAX_HIDDEN
POLICY_ACTIVATIONS = ("softsign", "relu")   # REM2D_POLICY_SOFTSIGN, REM2D_POLICY_RELU
EPISODE_ABI_VERSION = 1     # include/rem2d_episode.h
WHEN = {"done": 1, "frozen": 2, "steps": 4}   # REM2D_WHEN_DONE, REM2D_WHEN_FROZEN, REM2D_WHEN_STEPS
STREAM_ABI_VERSION = 1      # include/rem2d_stream.h
EVOLVE_ABI_VERSION = 1      # include/rem2d_evolve.h
ORDER_ABI_VERSION = 1       # include/rem2d_order.h
EVOLVE_MAX_TOURNSIZE = 4    # REM2D_EVOLVE_MAX_TOURNSIZE
ES_ABI_VERSION = 1          # include/rem2d_es.h
NOVELTY_ABI_VERSION = 1     # include/rem2d_novelty.h
NOVELTY_MAX_WIDTH = 32      # REM2D_NOVELTY_MAX_WIDTH
NOVELTY_MAX_K = 32          # REM2D_NOVELTY_MAX_K
NOVELTY_MAX_SAMPLES = 16    # REM2D_NOVELTY_MAX_SAMPLES
ELITES_ABI_VERSION = 1      # include/rem2d_elites.h
ELITES_MAX_WIDTH = 32       # REM2D_ELITES_MAX_WIDTH
ELITES_MAX_DIMS = 4         # REM2D_ELITES_MAX_DIMS
ELITES_MAX_CELLS = 65536    # REM2D_ELITES_MAX_CELLS
CVT_ABI_VERSION = 1         # include/rem2d_cvt.h
CVT_MAX_WIDTH = 32          # REM2D_CVT_MAX_WIDTH
CVT_MAX_CELLS = 65536       # REM2D_CVT_MAX_CELLS
CVT_MAX_SPLITS = 4096       # REM2D_CVT_MAX_SPLITS
SNES_ABI_VERSION = 1        # include/rem2d_snes.h
SNES_MAX_GROUP = 8192       # REM2D_SNES_MAX_GROUP
SNES_ADAM, SNES_NATURAL = 1, 2   # REM2D_SNES_ADAM, REM2D_SNES_NATURAL
PARETO_ABI_VERSION = 1      # include/rem2d_pareto.h
PARETO_MAX_OBJ = 4          # REM2D_PARETO_MAX_OBJ
PARETO_MAX_GROUP = 1024     # REM2D_PARETO_MAX_GROUP
PARETO_MAX_WIDTH = 32       # REM2D_PARETO_MAX_WIDTH
PARETO_MAX_K = 32           # REM2D_PARETO_MAX_K
RECURRENT_ABI_VERSION = 1   # include/rem2d_recurrent.h
RECURRENT_MAX_INPUTS = SENSE_MAX_RAYS   # n_rays + context: what a feed-forward set may have as ray inputs
MODULAR_ABI_VERSION = 1     # include/rem2d_modular.h
MODULAR_MAX_ROUNDS = 8      # REM2D_MODULAR_MAX_ROUNDS
MODULAR_MAX_INPUTS = SENSE_MAX_RAYS   # REM2D_MODULAR_MAX_INPUTS: n_rays + 2 + 2 messages, a feed-forward set's ray inputs
OBSNORM_ABI_VERSION = 1     # include/rem2d_obsnorm.h
OBSNORM_MAX_CHUNK = 65536   # REM2D_OBSNORM_MAX_CHUNK
OBSNORM_CAPACITY_LOG2 = 39  # REM2D_OBSNORM_CAPACITY_LOG2
SELFTEST_ABI_VERSION = 1    # include/rem2d_selftest.h
SELFTEST_CASE_WORDS = 26    # REM2D_SELFTEST_CASE_WORDS
SELFTEST_OUT_WORDS = 8      # REM2D_SELFTEST_OUT_WORDS
SELFTEST_OPS = ("collide", "distance", "toi", "far_apart")   # REM2D_SELFTEST_COLLIDE .. _FAR_APART


class WorldCfg(C.Structure):
    _fields_ = [("n_envs", C.c_int32), ("lanes", C.c_int32), ("flags", C.c_uint32), ("device", C.c_int32)]


class Morph(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in MORPH_FIELDS]


class LsystemGenomes(C.Structure):
    """rem2d_lsystem_genomes (include/rem2d.h): host pointers, SoA over genomes."""
    _fields_ = [("n", C.c_int32), ("n_types", C.c_int32)] + [(k, C.c_void_p) for k in (
        "mod_shape", "mod_width", "mod_height", "mod_radius", "mod_angle", "mod_torque", "ctl_amp", "ctl_phase",
        "ctl_freq", "ctl_offset", "rule_n", "rule_site", "rule_ref")]


class TreeBatch(C.Structure):
    """rem2d_tree_batch (include/rem2d.h): host pointers, [n][max_nodes]."""
    _fields_ = [("n", C.c_int32), ("max_nodes", C.c_int32)] + [(k, C.c_void_p) for k in (
        "node_count", "index", "parent", "site", "shape", "width", "height", "radius", "angle", "torque", "ctl_amp",
        "ctl_phase", "ctl_freq", "ctl_offset")]


class NetworkGenomes(C.Structure):
    """rem2d_network_genomes (include/rem2d.h)."""
    _fields_ = ([("n", C.c_int32), ("n_types", C.c_int32), ("n_hidden", C.c_int32), ("max_modules", C.c_int32)]
                + [(k, C.c_void_p) for k in ("w1", "a1", "w2", "mod_shape", "mod_width", "mod_height", "mod_radius",
                                             "mod_angle", "mod_torque", "ctl_amp", "ctl_phase", "ctl_freq", "ctl_offset")]
                + [(k, C.c_double) for k in ("box_min_width", "box_max_width", "box_min_height", "box_max_height",
                                             "box_min_angle", "box_max_angle", "circle_min_radius", "circle_max_radius",
                                             "circle_min_angle", "circle_max_angle", "ctl_max_amp", "ctl_max_phase",
                                             "ctl_max_offset", "ctl_max_freq")])


class TreePopulation(C.Structure):
    """rem2d_tree_population (include/rem2d.h): host pointers, [n][max_nodes], mutated in place by rem2d_mutate_trees."""
    _fields_ = ([("n", C.c_int32), ("max_nodes", C.c_int32)]
                + [(k, C.c_void_p) for k in ("node_count", "parent", "site", "shape", "width", "height", "radius", "angle", "torque",
                                             "ctl_amp", "ctl_phase", "ctl_freq", "ctl_offset")]
                + [(k, C.c_int32) for k in ("max_modules", "max_depth", "n_box", "n_circle")]
                + [(k, C.c_double) for k in ("proto_box_width", "proto_box_height", "proto_circle_radius", "proto_angle",
                                             "proto_torque", "box_min_width", "box_max_width", "box_min_height", "box_max_height",
                                             "box_min_angle", "box_max_angle", "circle_min_radius", "circle_max_radius",
                                             "circle_min_angle", "circle_max_angle", "ctl_max_amp", "ctl_max_phase",
                                             "ctl_max_offset", "ctl_max_freq")])


class StepGroup(C.Structure):
    """rem2d_step_group (include/rem2d.h)."""
    _fields_ = [("worlds", C.POINTER(C.c_void_p)), ("n_worlds", C.c_int32), ("stream", C.c_void_p)]


class Policy(C.Structure):
    """rem2d_policy (include/rem2d_policy.h): device pointers the caller owns."""
    _fields_ = ([(k, C.c_int32) for k in ("d", "max_bodies", "n_rays", "hidden", "activation")] + [("scale", C.c_float)]
                + [(k, C.c_int32) for k in ("n_sets", "reserved")]
                + [(k, C.c_void_p) for k in ("w1", "b1", "w2", "b2", "index", "row_mask", "obs", "frac", "targets", "valid")]
                + [("n_rows", C.c_int64)])


class Recurrent(C.Structure):
    """rem2d_recurrent (include/rem2d_recurrent.h): a rem2d_policy, the context width and the device memory the caller owns."""
    _fields_ = [("p", Policy), ("context", C.c_int32), ("reserved", C.c_int32), ("memory", C.c_void_p), ("reset", C.c_void_p)]


class Topology(C.Structure):
    """rem2d_topology (include/rem2d_modular.h): where the topology table goes, and the stream the call queues on."""
    _fields_ = [("max_bodies", C.c_int32), ("reserved", C.c_int32), ("out", C.c_void_p), ("out_rows", C.c_int64), ("stream", C.c_void_p)]


class Modular(C.Structure):
    """rem2d_modular (include/rem2d_modular.h): a rem2d_policy, the message width, the rounds, the topology table, the device memory
    the caller owns, and the stream the calls queue on."""
    _fields_ = [("p", Policy), ("messages", C.c_int32), ("rounds", C.c_int32), ("topo", C.c_void_p), ("memory", C.c_void_p),
                ("reset", C.c_void_p), ("stream", C.c_void_p)]


class Obsnorm(C.Structure):
    """rem2d_obsnorm (include/rem2d_obsnorm.h): device pointers the caller owns, and the stream the calls queue on."""
    _fields_ = ([(k, C.c_int32) for k in ("max_bodies", "n_rays", "n_blocks", "group_size", "row_chunk", "context")]
                + [("clip", C.c_float), ("min_var", C.c_float), ("min_count", C.c_int64), ("n_rows", C.c_int64)]
                + [(k, C.c_void_p) for k in ("obs", "frac", "row_mask", "count", "s1", "s2hi", "s2lo", "mu", "inv", "memory", "reset")]
                + [("reserved", C.c_int64), ("stream", C.c_void_p)])


class Evolve(C.Structure):
    """rem2d_evolve (include/rem2d_evolve.h): device pointers the caller owns."""
    _fields_ = ([(k, C.c_int32) for k in ("d", "hidden", "max_bodies", "n_sets", "group_size", "tournsize", "elite")]
                + [("generation", C.c_uint32), ("rate_threshold", C.c_uint64), ("seed", C.c_uint64), ("sigma", C.c_float),
                   ("reserved", C.c_int32)]
                + [(k, C.c_void_p) for k in ("fitness", "w1", "b1", "w2", "b2", "child_w1", "child_b1", "child_w2", "child_b2",
                                             "parent")])


class Es(C.Structure):
    """rem2d_es (include/rem2d_es.h): device pointers the caller owns."""
    _fields_ = ([(k, C.c_int32) for k in ("d", "hidden", "max_bodies", "n_means", "group_size", "pair_chunk")]
                + [("generation", C.c_uint32), ("reserved", C.c_int32), ("seed", C.c_uint64), ("sigma", C.c_float), ("step", C.c_float)]
                + [(k, C.c_void_p) for k in ("fitness", "util", "w1", "b1", "w2", "b2", "child_w1", "child_b1", "child_w2", "child_b2",
                                             "new_w1", "new_b1", "new_w2", "new_b2", "scratch")]
                + [("scratch_bytes", C.c_uint64)])


class Novelty(C.Structure):
    """rem2d_novelty (include/rem2d_novelty.h): device pointers the caller owns."""
    _fields_ = ([(k, C.c_int32) for k in ("width", "n_rows", "group_size", "k", "capacity")]
                + [("generation", C.c_uint32), ("seed", C.c_uint64), ("add_threshold", C.c_uint64)]
                + [(k, C.c_void_p) for k in ("desc", "archive", "total", "novelty", "add_mask")]
                + [("reserved", C.c_int32)])


class Elites(C.Structure):
    """rem2d_elites (include/rem2d_elites.h): device pointers the caller owns."""
    _fields_ = ([(k, C.c_int32) for k in ("d", "hidden", "max_bodies", "width", "n_blocks", "group_size", "n_children", "n_dims")]
                + [("word", C.c_int32 * 4), ("bins", C.c_int32 * 4), ("lo", C.c_float * 4), ("inv", C.c_float * 4)]
                + [("generation", C.c_uint32), ("sigma", C.c_float), ("rate_threshold", C.c_uint64), ("seed", C.c_uint64)]
                + [(k, C.c_void_p) for k in ("desc", "fitness", "mask", "w1", "b1", "w2", "b2", "elite_fitness", "elite_desc",
                                             "elite_w1", "elite_b1", "elite_w2", "elite_b2", "count", "cell", "winner", "child_w1",
                                             "child_b1", "child_w2", "child_b2", "parent", "n_filled", "scratch")]
                + [("scratch_bytes", C.c_uint64), ("reserved", C.c_int32)])


class Cvt(C.Structure):
    """rem2d_cvt (include/rem2d_cvt.h): device pointers the caller owns, and the stream the calls queue on."""
    _fields_ = ([(k, C.c_int32) for k in ("d", "hidden", "max_bodies", "width", "n_cells", "n_blocks", "group_size", "n_children",
                                          "n_rows", "splits")]
                + [("generation", C.c_uint32), ("sigma_iso", C.c_float), ("sigma_line", C.c_float), ("reserved", C.c_int32),
                   ("seed", C.c_uint64)]
                + [(k, C.c_void_p) for k in ("centroids", "desc", "fitness", "mask", "w1", "b1", "w2", "b2", "elite_fitness",
                                             "elite_desc", "elite_w1", "elite_b1", "elite_w2", "elite_b2", "count", "cell", "dist",
                                             "winner", "child_w1", "child_b1", "child_w2", "child_b2", "parent", "parent2", "n_filled",
                                             "scratch")]
                + [("scratch_bytes", C.c_uint64), ("stream", C.c_void_p)])


SNES_ARRAYS = ("w1", "b1", "w2", "b2")


class Snes(C.Structure):
    """rem2d_snes (include/rem2d_snes.h): device pointers the caller owns."""
    _fields_ = ([(k, C.c_int32) for k in ("d", "hidden", "max_bodies", "n_means", "group_size", "pair_chunk")]
                + [("generation", C.c_uint32), ("flags", C.c_uint32), ("seed", C.c_uint64)]
                + [(k, C.c_float) for k in ("mstep", "sstep", "beta1", "omb1", "beta2", "omb2", "alpha", "eps", "sigma_min", "sigma_max")]
                + [("fitness", C.c_void_p), ("util", C.c_void_p)]
                + [(pre + k, C.c_void_p) for pre in ("", "sigma_", "m1_", "m2_", "child_", "new_", "new_sigma_", "new_m1_", "new_m2_")
                   for k in SNES_ARRAYS]
                + [("scratch", C.c_void_p), ("scratch_bytes", C.c_uint64)])


class Pareto(C.Structure):
    """rem2d_pareto (include/rem2d_pareto.h): device pointers the caller owns."""
    _fields_ = ([(k, C.c_int32) for k in ("n_rows", "group_size", "n_obj", "width", "k", "reserved")]
                + [(k, C.c_void_p) for k in ("obj", "front", "crowd", "util", "n_fronts", "desc", "fitness", "local", "neighbours")])


class EpisodeOut(C.Structure):
    """rem2d_episode_out (include/rem2d_episode.h): device arrays in population order the caller owns; any may be NULL."""
    _fields_ = [(k, C.c_void_p) for k in ("reward", "done", "ended", "fitness", "steps", "episodes")]


class Feed(C.Structure):
    """rem2d_feed (include/rem2d_stream.h): the pending creatures of one lane count, device memory the caller owns."""
    _fields_ = [("M", Morph), ("id", C.c_void_p), ("count", C.c_int32), ("lanes", C.c_int32), ("cursor", C.c_void_p)]


class StreamOut(C.Structure):
    """rem2d_stream_out (include/rem2d_stream.h): device arrays indexed by id the caller owns; any may be NULL."""
    _fields_ = [(k, C.c_void_p) for k in ("fitness", "steps", "err", "finished")]


class Rem2dError(RuntimeError):
    pass


class HandoverError(Rem2dError):
    """A step train launch (REM2D_OPT_FUSE_VELPOST = 2, the default launch form) reported failed hand-overs between the workgroups of
    consecutive steps: a block's previous step was published from another XCD, or a wait for it ran into its 2 s limit (a GPU shared
    with another job, a partition mode that changes the workgroup -> XCD mapping).  NOT a contact-capacity problem: the creatures
    that carry REM2D_ERR_HANDOVER hold a state that cannot be trusted; the remedy is the same creatures on per-step launches
    (``options={"fuse_velpost": 1}``), which evaluate.run_episode does by itself.  ``failures``: workgroups that reported it."""

    def __init__(self, failures, where=""):
        self.failures = int(failures)
        super().__init__("%d hand-over(s) between the workgroups of the step train failed%s: the creatures flagged REM2D_ERR_HANDOVER "
                         "(env.errors() & 4) hold a state that is not to be trusted -- step them on per-step launches instead "
                         "(BatchedModular2D(options={'fuse_velpost': 1}) / REM2D_FUSE_VELPOST=1); evaluate.run_episode re-evaluates "
                         "them that way by itself" % (self.failures, where))


# -fno-slp-vectorize: SLP-packing scalar f32 math into v_pk_* costs more register shuffling (v_mov) than it saves here;
# without it the step kernel fits 238 VGPRs with no spills (+11..14 % env-steps/s).  -ffp-contract=off keeps every binary32
# operation separately rounded (what the bit-exact parity rests on).
# (-instcombine-max-copied-from-constant-users: a kernel reads its by-value `Batch` argument straight from the kernarg segment only
# while LLVM's scan of the argument's users stays under this limit -- 300 by default, which rem2d_step_train_kernel's inlined
# phases exceed: the whole 1.5 KB struct was copied to scratch and spilled from there; the other kernels compile the same either way)
# (-Os, round 6: the same arithmetic -- no fast-math, contraction off -- in ~10 % fewer instructions: +1.3 % on configs 3 / 4 and the
# 8-module chains against -O3; -O2 +0.7 %, -O1 -5 %, -Oz -12 %: profiles/r06_experiments.txt 16)
BUILD_FLAGS = ["-Os", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize", "-std=c++17", "-fPIC", "-shared",
               "-mllvm", "-instcombine-max-copied-from-constant-users=4000"]
WIDE_FLAGS = ["-DREM2D_WIDE=1"]
FMA_FLAGS = ["-ffp-contract=fast"]   # (the later -ffp-contract wins over BUILD_FLAGS')


def _variant(wide):
    """(path, extra flags, name of the overriding environment variable) of a build: False the default, True the wide-slot
    build, "fma" the tolerance-mode build."""
    if wide == "fma":
        return FMA_LIB_PATH, FMA_FLAGS, "REM2D_FMA_LIB_PATH"
    return (WIDE_LIB_PATH, WIDE_FLAGS, "REM2D_WIDE_LIB_PATH") if wide else (LIB_PATH, [], "REM2D_LIB_PATH")
INCLUDE_DIR = os.path.join(_ROOT, "include")
_ID_MARKER = b"REM2D_BUILD_ID="


def source_id(extra=()):
    """Identity of a build of the library as the sources stand NOW: sha256 over every file under csrc/ (name and bytes, in
    name order), the headers under include/ and the compile flags, 16 hex digits.  build() compiles it in (-DREM2D_BUILD_ID), lib()
    compares it with rem2d_build_id() and refuses a library built from anything else."""
    import hashlib
    csrc = os.path.dirname(SRC_PATH)
    h = hashlib.sha256()
    headers = sorted(os.path.join(INCLUDE_DIR, f) for f in os.listdir(INCLUDE_DIR) if f.endswith(".h"))
    for path in sorted(os.path.join(csrc, f) for f in os.listdir(csrc)) + headers:
        h.update(os.path.basename(path).encode() + b"\0")
        with open(path, "rb") as f:
            h.update(f.read())
        h.update(b"\0")
    h.update(" ".join(BUILD_FLAGS + list(extra)).encode())
    return h.hexdigest()[:16]


def file_build_id(path):
    """The build id compiled into a library file, read from its bytes (no dlopen: that would pin /opt/rocm's HIP runtime
    before torch has loaded its own); None for a missing file or one without the marker."""
    try:
        with open(path, "rb") as f:
            blob = f.read()
    except OSError:
        return None
    i = blob.find(_ID_MARKER)
    if i < 0:
        return None
    j = blob.find(b"\0", i)
    return blob[i + len(_ID_MARKER):j].decode("ascii", "replace")


def build(force=False, verbose=False):
    """Compile csrc/rem2d.hip for gfx950 into gym_rem2d_amd/librem2d.so, (-DREM2D_WIDE) librem2d_wide.so and (-ffp-contract=fast,
    the labelled tolerance mode) librem2d_fma.so -- hipcc cross-compiles without a GPU; the three compile side by side.  A
    library is rebuilt when the id compiled into it differs from source_id(): the hash of the sources and flags, not a file time."""
    procs = []
    for path, extra in ((LIB_PATH, []), (WIDE_LIB_PATH, WIDE_FLAGS), (FMA_LIB_PATH, FMA_FLAGS)):
        want = source_id(extra)
        if not force and file_build_id(path) == want:
            continue
        cmd = ["hipcc"] + BUILD_FLAGS + extra + ['-DREM2D_BUILD_ID="%s"' % want, "-I" + INCLUDE_DIR, SRC_PATH, "-o", path]
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd)))
    failed = None
    for cmd, pr in procs:   # (wait for every child before raising: no compile is left running behind an exception)
        if pr.wait() != 0 and failed is None:
            failed = (pr.returncode, cmd)
    if failed is not None:
        raise subprocess.CalledProcessError(*failed)
    return LIB_PATH


_lib = None
_libs = {}


def build_id(wide=False):
    """rem2d_build_id() of the loaded library (bench.py prints it)."""
    return lib(wide).rem2d_build_id().decode()


def capacity(wide=False):
    """(REM2D_CONTACT_SLOTS, REM2D_SOLVER_SLOTS) of the default / the wide build."""
    a, b = C.c_int32(), C.c_int32()
    check(lib(wide).rem2d_capacity(C.byref(a), C.byref(b)))
    return a.value, b.value


def lib(wide=False):
    global _lib
    if not wide and _lib is not None:
        return _lib
    if wide and wide in _libs:
        return _libs[wide]
    path, flags, override_var = _variant(wide)
    # PyTorch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so, same SONAME as /opt/rocm's).
    # Import torch first so that librem2d.so binds to the runtime torch initialises -- two runtimes
    # in one process fail with "no ROCm-capable device is detected".
    import torch  # noqa: F401
    if not os.path.exists(path):
        raise Rem2dError(
            "gym_rem2d_amd: %s is missing -- the HIP extension is required (there is no CPU fallback). "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'`." % path)
    L = C.CDLL(path)
    L.rem2d_abi_version.restype = C.c_int
    L.rem2d_last_error.restype = C.c_char_p
    L.rem2d_capacity.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.rem2d_worlds_launch_info.restype = C.c_int
    L.rem2d_worlds_launch_info.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.rem2d_state_bytes.restype = C.c_size_t
    L.rem2d_state_bytes.argtypes = [C.POINTER(WorldCfg)]
    L.rem2d_padded_envs.restype = C.c_int32
    L.rem2d_padded_envs.argtypes = [C.POINTER(WorldCfg)]
    L.rem2d_world_create.argtypes = [C.POINTER(WorldCfg), C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
    L.rem2d_world_destroy.argtypes = [C.c_void_p]
    L.rem2d_world_set_terrain.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                          C.c_float]
    L.rem2d_world_reset.argtypes = [C.c_void_p, C.POINTER(Morph), C.c_void_p]
    L.rem2d_world_set_tiles.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    L.rem2d_world_set_outputs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rem2d_world_gather.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    L.rem2d_plan_tiles.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.rem2d_plan_tiles_shape.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_void_p, C.c_void_p]
    L.rem2d_world_set_tile_shape.argtypes = [C.c_void_p, C.c_int32]
    L.rem2d_world_set_order.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.rem2d_world_set_option.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    L.rem2d_world_get_option.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    L.rem2d_world_adopt.argtypes = [C.c_void_p]
    L.rem2d_world_step.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.rem2d_world_step_ex.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_void_p]
    L.rem2d_worlds_step.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_void_p]
    L.rem2d_worlds_step_ex.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32,
                                       C.c_void_p]
    L.rem2d_groups_step.argtypes = [C.POINTER(StepGroup), C.c_int32, C.c_int32, C.c_void_p, C.c_uint32]
    L.rem2d_groups_step_ex.argtypes = [C.POINTER(StepGroup), C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32,
                                       C.c_void_p, C.c_uint32]
    L.rem2d_compile_lsystem.argtypes = [C.POINTER(LsystemGenomes), C.c_int32, C.c_int32, C.c_double, C.c_int32,
                                        C.POINTER(Morph), C.c_void_p, C.c_int32]
    L.rem2d_compile_trees.argtypes = [C.POINTER(TreeBatch), C.c_double, C.c_int32, C.POINTER(Morph), C.c_void_p, C.c_int32]
    L.rem2d_compile_network.argtypes = [C.POINTER(NetworkGenomes), C.c_int32, C.c_double, C.c_int32, C.POINTER(Morph),
                                        C.c_void_p, C.c_int32]
    L.rem2d_mutate_trees.argtypes = [C.POINTER(TreePopulation), C.c_double, C.c_double, C.c_double, C.c_uint64, C.c_int32]
    L.rem2d_tree_diversity.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    L.rem2d_selftest_scalar.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    L.rem2d_world_field.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                    C.POINTER(C.c_int32)]
    L.rem2d_world_enable_timing.argtypes = [C.c_void_p, C.c_int32]
    L.rem2d_world_kernel_time_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.rem2d_world_step_time_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.rem2d_world_handover_failures.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int32]
    # the renderer (include/rem2d_render.h)
    L.rem2d_render_abi_version.restype = C.c_int
    L.rem2d_world_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                     C.c_void_p, C.c_void_p]
    if L.rem2d_render_abi_version() != RENDER_ABI_VERSION:
        raise Rem2dError("%s: render ABI version mismatch" % os.path.basename(path))
    # closed-loop control (include/rem2d_control.h)
    L.rem2d_control_abi_version.restype = C.c_int
    L.rem2d_worlds_observe.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    L.rem2d_worlds_control.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p,
                                       C.c_void_p]
    if L.rem2d_control_abi_version() != CONTROL_ABI_VERSION:
        raise Rem2dError("%s: control ABI version mismatch" % os.path.basename(path))
    # terrain range sensing (include/rem2d_sense.h)
    L.rem2d_sense_abi_version.restype = C.c_int
    L.rem2d_worlds_sense.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_void_p]
    if L.rem2d_sense_abi_version() != SENSE_ABI_VERSION:
        raise Rem2dError("%s: sense ABI version mismatch" % os.path.basename(path))
    # device policies (include/rem2d_policy.h)
    L.rem2d_policy_abi_version.restype = C.c_int
    L.rem2d_policy_forward.argtypes = [C.POINTER(Policy), C.c_void_p]
    L.rem2d_worlds_act.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(Policy), C.c_void_p, C.c_void_p]
    if L.rem2d_policy_abi_version() != POLICY_ABI_VERSION:
        raise Rem2dError("%s: policy ABI version mismatch" % os.path.basename(path))
    # episode boundaries (include/rem2d_episode.h)
    L.rem2d_episode_abi_version.restype = C.c_int
    L.rem2d_worlds_reset_where.argtypes = [C.POINTER(C.c_void_p), C.POINTER(Morph), C.c_int32, C.c_void_p, C.c_uint32, C.c_int32,
                                           C.POINTER(EpisodeOut), C.c_int64, C.c_void_p]
    if L.rem2d_episode_abi_version() != EPISODE_ABI_VERSION:
        raise Rem2dError("%s: episode ABI version mismatch" % os.path.basename(path))
    # streaming evaluation (include/rem2d_stream.h)
    L.rem2d_stream_abi_version.restype = C.c_int
    L.rem2d_worlds_refill.argtypes = [C.POINTER(C.c_void_p), C.POINTER(Morph), C.c_int32, C.POINTER(Feed), C.c_void_p, C.c_uint32,
                                      C.c_int32, C.POINTER(StreamOut), C.c_int64, C.c_int64, C.c_void_p]
    if L.rem2d_stream_abi_version() != STREAM_ABI_VERSION:
        raise Rem2dError("%s: stream ABI version mismatch" % os.path.basename(path))
    # evolving device policies (include/rem2d_evolve.h)
    L.rem2d_evolve_abi_version.restype = C.c_int
    for fn in (L.rem2d_policy_select, L.rem2d_policy_vary, L.rem2d_policy_evolve):
        fn.argtypes = [C.POINTER(Evolve), C.c_void_p]
    if L.rem2d_evolve_abi_version() != EVOLVE_ABI_VERSION:
        raise Rem2dError("%s: evolve ABI version mismatch" % os.path.basename(path))
    # the creature order, read back and made on demand (include/rem2d_order.h)
    L.rem2d_order_abi_version.restype = C.c_int
    L.rem2d_world_read_order.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.rem2d_world_make_order.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    if L.rem2d_order_abi_version() != ORDER_ABI_VERSION:
        raise Rem2dError("%s: order ABI version mismatch" % os.path.basename(path))
    # an evolution strategy for device policies (include/rem2d_es.h)
    L.rem2d_es_abi_version.restype = C.c_int
    L.rem2d_es_scratch_bytes.restype = C.c_int64
    L.rem2d_es_scratch_bytes.argtypes = [C.POINTER(Es)]
    for fn in (L.rem2d_es_sample, L.rem2d_es_shape, L.rem2d_es_update, L.rem2d_es_step):
        fn.argtypes = [C.POINTER(Es), C.c_void_p]
    if L.rem2d_es_abi_version() != ES_ABI_VERSION:
        raise Rem2dError("%s: es ABI version mismatch" % os.path.basename(path))
    # behavioural novelty (include/rem2d_novelty.h)
    L.rem2d_novelty_abi_version.restype = C.c_int
    L.rem2d_worlds_describe.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    for fn in (L.rem2d_novelty_score, L.rem2d_novelty_add, L.rem2d_novelty_step):
        fn.argtypes = [C.POINTER(Novelty), C.c_void_p]
    if L.rem2d_novelty_abi_version() != NOVELTY_ABI_VERSION:
        raise Rem2dError("%s: novelty ABI version mismatch" % os.path.basename(path))
    # MAP-Elites for device policies (include/rem2d_elites.h)
    L.rem2d_elites_abi_version.restype = C.c_int
    L.rem2d_elites_scratch_bytes.restype = C.c_int64
    L.rem2d_elites_scratch_bytes.argtypes = [C.POINTER(Elites)]
    for fn in (L.rem2d_elites_insert, L.rem2d_elites_sample, L.rem2d_elites_emit):
        fn.argtypes = [C.POINTER(Elites), C.c_void_p]
    if L.rem2d_elites_abi_version() != ELITES_ABI_VERSION:
        raise Rem2dError("%s: elites ABI version mismatch" % os.path.basename(path))
    # centroid archives and the line emitter (include/rem2d_cvt.h): the stream is a member of the descriptor
    L.rem2d_cvt_abi_version.restype = C.c_int
    L.rem2d_cvt_scratch_bytes.restype = C.c_int64
    L.rem2d_cvt_scratch_bytes.argtypes = [C.POINTER(Cvt)]
    for fn in (L.rem2d_cvt_assign, L.rem2d_cvt_insert, L.rem2d_cvt_emit_line):
        fn.argtypes = [C.POINTER(Cvt)]
    if L.rem2d_cvt_abi_version() != CVT_ABI_VERSION:
        raise Rem2dError("%s: cvt ABI version mismatch" % os.path.basename(path))
    # an adaptive evolution strategy for device policies (include/rem2d_snes.h)
    L.rem2d_snes_abi_version.restype = C.c_int
    L.rem2d_snes_scratch_bytes.restype = C.c_int64
    L.rem2d_snes_scratch_bytes.argtypes = [C.POINTER(Snes)]
    for fn in (L.rem2d_snes_sample, L.rem2d_snes_update, L.rem2d_snes_step):
        fn.argtypes = [C.POINTER(Snes), C.c_void_p]
    if L.rem2d_snes_abi_version() != SNES_ABI_VERSION:
        raise Rem2dError("%s: snes ABI version mismatch" % os.path.basename(path))
    # Pareto ranking (include/rem2d_pareto.h)
    L.rem2d_pareto_abi_version.restype = C.c_int
    for fn in (L.rem2d_pareto_rank, L.rem2d_pareto_local):
        fn.argtypes = [C.POINTER(Pareto), C.c_void_p]
    if L.rem2d_pareto_abi_version() != PARETO_ABI_VERSION:
        raise Rem2dError("%s: pareto ABI version mismatch" % os.path.basename(path))
    # recurrent device policies (include/rem2d_recurrent.h)
    L.rem2d_recurrent_abi_version.restype = C.c_int
    L.rem2d_recurrent_forward.argtypes = [C.POINTER(Recurrent), C.c_void_p]
    L.rem2d_worlds_act_recurrent.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(Recurrent), C.c_void_p, C.c_void_p]
    if L.rem2d_recurrent_abi_version() != RECURRENT_ABI_VERSION:
        raise Rem2dError("%s: recurrent ABI version mismatch" % os.path.basename(path))
    # observation normalisation (include/rem2d_obsnorm.h): the stream is a member of the descriptor
    L.rem2d_obsnorm_abi_version.restype = C.c_int
    for fn in (L.rem2d_obsnorm_accumulate, L.rem2d_obsnorm_freeze):
        fn.argtypes = [C.POINTER(Obsnorm)]
    for fn in (L.rem2d_obsnorm_forward, L.rem2d_obsnorm_forward_memory):
        fn.argtypes = [C.POINTER(Obsnorm), C.POINTER(Policy)]
    L.rem2d_worlds_act_normed.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(Obsnorm), C.POINTER(Policy), C.c_void_p, C.c_int32]
    if L.rem2d_obsnorm_abi_version() != OBSNORM_ABI_VERSION:
        raise Rem2dError("%s: obsnorm ABI version mismatch" % os.path.basename(path))
    # modular device policies (include/rem2d_modular.h): the stream is a member of both descriptors
    L.rem2d_modular_abi_version.restype = C.c_int
    L.rem2d_worlds_topology.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(Topology)]
    L.rem2d_modular_forward.argtypes = [C.POINTER(Modular)]
    L.rem2d_worlds_act_modular.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(Modular), C.c_void_p]
    if L.rem2d_modular_abi_version() != MODULAR_ABI_VERSION:
        raise Rem2dError("%s: modular ABI version mismatch" % os.path.basename(path))
    # self-test of the collision geometry (include/rem2d_selftest.h)
    L.rem2d_selftest_abi_version.restype = C.c_int
    L.rem2d_selftest_static_box.argtypes = [C.c_void_p, C.c_void_p]
    L.rem2d_selftest_geometry.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    if L.rem2d_selftest_abi_version() != SELFTEST_ABI_VERSION:
        raise Rem2dError("%s: selftest ABI version mismatch" % os.path.basename(path))
    if L.rem2d_abi_version() != 11:
        raise Rem2dError("%s: ABI version mismatch" % os.path.basename(path))
    L.rem2d_build_id.restype = C.c_char_p
    # the library must have been built from the sources beside it (REM2D_LIB_PATH / REM2D_WIDE_LIB_PATH name an experiment's
    # variant build on purpose: tools/build_variant.sh, exempt)
    overridden = os.environ.get(override_var)
    have, want = L.rem2d_build_id().decode(), source_id(flags)
    if not overridden and have != want:
        raise Rem2dError("%s is stale: built from sources with id %s, the sources here have id %s -- rebuild it with "
                         "`python -c 'import __graft_entry__ as g; g.build()'`" % (os.path.basename(path), have, want))
    if wide:
        _libs[wide] = L
    else:
        _lib = L
    return L


def plan_tiles(parent, jround, n_envs, lanes, n_padded, max_creatures=0, tile_shape=-1, wide=False):
    """Tile plan of the velocity kernel for one morphology batch (rem2d_plan_tiles_shape): int32 tile starts
    [n_tiles + 1].  tile_shape: 0 .. 4, or -1 for the default (3); max_creatures 0: the library's default cap unless
    REM2D_TILE_CREATURES overrides it (experiments)."""
    import numpy as np
    parent = np.ascontiguousarray(parent, dtype=np.int32)
    jround = np.ascontiguousarray(jround, dtype=np.int32)
    out = np.zeros(int(n_padded) + 1, dtype=np.int32)
    n = C.c_int32()
    if max_creatures <= 0:
        max_creatures = env_tile_creatures()
    # (the plan of the build that will run it: the wide build schedules one phase more than the default one, V4_PHASES)
    check(lib(wide).rem2d_plan_tiles_shape(parent.ctypes.data, jround.ctypes.data, int(n_envs), int(lanes), int(n_padded),
                                           int(max_creatures), int(tile_shape), out.ctypes.data, C.byref(n)), wide)
    return out[:n.value + 1].copy()


def world_array(worlds):
    """The `rem2d_world *` array of a list of BatchedWorld, as the rem2d_worlds_* calls and rem2d_step_group take it."""
    handles = [w.h for w in worlds]
    return (C.c_void_p * len(handles))(*handles)


def check(rc, wide=False):
    if rc != 0:
        raise Rem2dError("librem2d: error %d: %s" % (rc, lib(wide).rem2d_last_error().decode()))
