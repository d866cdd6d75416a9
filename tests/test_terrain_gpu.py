"""The step kernels on the ground the parity suite never stood on (tests/terrain_forge.py), on a real MI355X (pytest -m gpu).

The protocol of tests/test_injected_state_gpu.py without the injection, with its comparator (tests/replay.py: read_state / mismatches
over state_forge.masks / state_forge.snapshot): reset on the PLACED morphology, show the reset state equal to the oracle's, then
compare with `==` after each of 60 single-step launches and in a second world after multi-step launches of 1, 9 and 50 steps.
Nobody is left out: the host half holds every input within the build's slots, any error bit on any creature fails the test, and
handover_failures() == 0.

The `rough` parametrisation of the older parity tests stays on the start pad (21 collinear points at y == 5.0); THIS module is
where sloped ground, box obstacles of every kind, other pitches and origins and both ends of the polyline are compared.

Matrix: every terrain x its populations through the step train with continuous physics; the production tracks and the
nine-class sawtooth also through velpost, two_launches and the fused step kernel and once with continuous physics off;
hardcore0 in the wide build; the end terrain through every launch form (the TOI solve calls find_new_pairs from its own site).
Renderer: kernel against tests/render_model.py with np.array_equal on the small-pitch, large-pitch, shifted-xs and negative-x0
terrains, cameras over the steepest edge and over both ends of the polyline (the pitch arithmetic of rem2d_raster.h r_shade).
rem2d_world_set_terrain's refusals (xs not increasing, one x more than 0.1 pitch off) are asserted with their messages.

Measured on an MI355X: 55 ids in 29 s, all passing; nothing differed, so no kernel changed.  Creature-steps compared on the
single-step worlds (ids): rough4 49 320 (7), hardcore4 43 680 (6), hardcore0 22 620 (3), saw 49 320 (7), stairs, vvalley, saw_fine,
saw_coarse, saw_neg, shifted 15 000 (3) each, ends 52 800 (9): 11 terrains, 50 ids, 307 740 creature-steps.
"""
import numpy as np
import pytest

import replay as R
import terrain_forge as G

pytestmark = pytest.mark.gpu

CONT = 1
MULTI = (1, 9, 50)          # the second world's launches: compared after steps 1, 10 and 60
ALL_FORMS = ("velpost", "two_launches", "fused_step_kernel")      # this module's ids are replay.LAUNCH_FORMS' own names


def _cases():
    out = []
    for t, (_, pops, _, _) in G.TERRAINS.items():
        for pop in pops:
            out.append((t, pop, "step_train", CONT, False))
    for t, pop in (("rough4", "lsystem"), ("hardcore4", "cppn"), ("saw", "lsystem")):
        for form in ALL_FORMS:
            out.append((t, pop, form, CONT, False))
        out.append((t, pop, "step_train", 0, False))
    out.append(("hardcore0", "cppn", "step_train", CONT, True))
    for form in ALL_FORMS:
        out.append(("ends", "lsystem", form, CONT, False))
        out.append(("ends", "direct", form, CONT, False))
    return out


def _id(c):
    return "%s-%s-%s-%s%s" % (c[0], c[1], c[2], "continuous" if c[3] else "discrete", "-wide" if c[4] else "")


@pytest.fixture(scope="module")
def gpu():
    return R.need_gpu(world=True)


@pytest.fixture(scope="module")
def tally():
    yield from R.tally("terrain parity (single-step worlds): terrain", G.TERRAINS)


def run_bucket(gpu, run, flags, form, wide):
    """-> creature-steps compared on the single-step world, through replay.replay: both worlds from reset, nobody left out, the
    second one in launches of MULTI steps."""
    from gym_rem2d_amd import _lib
    ctx = run["ctx"]
    marks = list(np.cumsum(MULTI))
    assert marks[-1] == G.N_STEPS
    return R.replay(lambda: R.make_world(gpu, ctx.morph, run["profile"], flags, form, wide), ctx, run["reset"], [1] * G.N_STEPS,
                    run["steps"], _lib.capacity(wide)[0], marks=marks)[0]


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_terrain_bit_exact(gpu, oracle, tally, case):
    terrain, pop, form, flags, wide = case
    from gym_rem2d_amd import _lib
    assert _lib.FLAG_CONTINUOUS == oracle.FLAG_CONTINUOUS == CONT
    runs = G.runs_of(oracle, terrain, pop, flags)       # the oracle first: a non-finite state never reaches the GPU
    cov = G.coverage(runs)
    assert cov["over"] == 0 and (cov["n_edges"] > 0 or cov["n_boxes"] > 0)      # nobody left out, and the ground is met
    compared = sum(run_bucket(gpu, run, flags, form, wide) for run in runs)
    assert compared == G.N_STEPS * cov["creatures"]
    R.count(tally, terrain, _id(case), compared)


def test_set_terrain_refusals(gpu):
    """Non-uniform polylines are refused (the edge window and the renderer compute an edge index from x0 and the pitch)."""
    from gym_rem2d_amd import _lib
    from gym_rem2d_amd.terrain import TerrainProfile
    w = gpu(4, 2, CONT)
    try:
        base = G.profile("saw")
        xs = base.xs.copy()
        xs[:] = xs[::-1]                                  # decreasing
        with pytest.raises(_lib.Rem2dError, match="error -1: terrain xs must be increasing"):
            w.set_terrain(TerrainProfile(xs, base.ys, []))
        xs = base.xs.copy()
        xs[100] += 0.12 * (xs[1] - xs[0])                 # one x more than 0.1 pitch off
        with pytest.raises(_lib.Rem2dError, match="error -1: terrain xs must be uniformly spaced"):
            w.set_terrain(TerrainProfile(xs, base.ys, []))
        xs = base.xs.copy()
        xs[100], xs[101] = xs[101], xs[100]               # locally not increasing: a whole pitch off
        with pytest.raises(_lib.Rem2dError, match="error -1: terrain xs must be uniformly spaced"):
            w.set_terrain(TerrainProfile(xs, base.ys, []))
        xs = base.xs.copy()
        xs[100] += 0.08 * (xs[1] - xs[0])                 # within the tolerance: accepted
        w.set_terrain(TerrainProfile(xs, base.ys, []))
    finally:
        w.close()


@pytest.mark.parametrize("terrain", ["saw_fine", "saw_coarse", "shifted", "saw_neg"])
def test_renderer_on_other_pitches_and_origins(gpu, terrain):
    """rem2d_world_render against the numpy pixel model on polylines whose pitch and x0 are not the reference's: the edge under a
    pixel is found from x0 and 1 / pitch (rem2d_raster.h r_shade)."""
    import env_harness as R
    from gym_rem2d_amd.env import BatchedModular2D
    from oracle import oracle as O
    O.build()
    prof, morphs = G.placed(terrain, "direct")
    env = BatchedModular2D()
    env.terrain = prof                                    # (what _terrain() hands to every world and to the model)
    env.reset_morphology(morphs[1])
    env.step(20)
    n = env.n_envs
    R._compare(env, [0, n // 2, n - 1], 173, 97, O.sincosf)            # follow cameras: the creatures on their ground
    slope, _ = G.edge_geometry(prof)
    k = int(np.argmax(np.abs(slope)))
    xs, ys = prof.xs, prof.ys
    cams = np.array([[xs[k] - 2.0, min(ys[k], ys[k + 1]) - 1.0],       # over the steepest edge
                     [xs[0] - 3.0, ys[0] - 1.5],                       # over the left end: pixels left of xs[0]
                     [xs[-1] - 2.5, ys[-1] - 1.5],                     # over the right end: pixels right of xs[-1]
                     [xs[0] - 40.0, ys[0] - 1.5]], np.float32)         # wholly off the polyline
    R._compare(env, [0, 1, n - 2, n - 1], 173, 97, O.sincosf, cam=cams)
    R._compare(env, [n - 1], 800, 600, O.sincosf, cam=cams[2:3])
    env.close()
