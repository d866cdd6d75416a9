"""What several GPU test modules share beside the replay runner: the closed-loop population harness of tests/test_control_gpu.py
(also tests/test_sense_gpu.py, tests/test_policy_gpu.py) and the renderer-against-model comparison of tests/test_render_gpu.py (also
tests/test_terrain_gpu.py)."""
import numpy as np
import pytest

import control_model as M
import render_model as RM
from replay import read_state, verdict

CONT = 1


def make_env(pop, wide=False, options=None, flags=CONT):
    """BatchedModular2D holding the lane buckets of loop population `pop`, one world per bucket, in an interleaved population
    order: creature e of bucket k is population row rows[k][e].  -> (env, rows, morphs)"""
    from gym_rem2d_amd.env import BatchedModular2D
    terrain, morphs = M.loop_population(pop)
    n = sum(m.n_envs for m in morphs)
    order = np.random.default_rng(5).permutation(n)
    rows, at = [], 0
    for m in morphs:
        rows.append(order[at:at + m.n_envs])
        at += m.n_envs
    env = BatchedModular2D(hardcore=(pop == "cppn"), seed=4, flags=flags, wide=wide, options=options)
    assert np.array_equal(env._terrain().f32()[1], terrain.f32()[1])      # the population's own terrain
    env._upload([(m, r) for m, r in zip(morphs, rows)], n)
    assert len(env.worlds) == len(morphs) and all(w.n_envs == m.n_envs for (w, _), m in zip(env.worlds, morphs))
    return env, rows, morphs


def population_rows(runs, rows, key, t, max_bodies):
    """The runs' per-bucket arrays of step t as one population-order array of `max_bodies` columns of bodies (zero beyond a bucket's)."""
    n = sum(len(r) for r in rows)
    per = M.OBS_BODY if key == "obs" else 1
    head = M.OBS_HEAD if key == "obs" else 0
    out = np.zeros((n, head + per * max_bodies), runs[0][key][t].dtype)
    for run, r in zip(runs, rows):
        v = run[key][t]
        out[r, :v.shape[1]] = v
    return out


def check_final(env, runs, firsts, what):
    from gym_rem2d_amd import _lib
    pair_slots = _lib.capacity(env.wide)[0]
    bad = []
    for (w, _), run, (first, bits) in zip(env.worlds, runs, firsts):
        keep = first >= len(run["obs"])
        bad += verdict(run["ctx"], read_state(w), run["final"], keep, bits, pair_slots, "%s K=%d final" % (what, run["ctx"].K))
        assert w.handover_failures() == 0
    assert not bad, "\n".join(bad)


def _scene(env, c):
    """(bodies, wod) of population creature c, read from its world's state."""
    from gym_rem2d_amd.render import _locate
    _, wis, loc = _locate(env, [c])
    w, e = env.worlds[int(wis[0])][0], int(loc[0])
    cols = [w.view(k)[e].cpu().numpy() for k in ("shape", "px", "py", "ang", "hx", "hy")]
    bodies = list(zip(*cols))
    return bodies, float(w.view("wod")[e].item()), (int(wis[0]), e)


def _model(env, c, cam, width, height, sincosf, fill=None, line=None):
    bodies, wod, (wi, e) = _scene(env, c)
    if fill is None:
        from gym_rem2d_amd.render import _world_colors
        f, l_ = _world_colors(env, wi)
        if f is not None:
            fill, line = f[e].cpu().numpy(), l_[e].cpu().numpy()
    return RM.render(width, height, cam, terrain=RM.Terrain.of(env._terrain()), bodies=bodies, fill=fill, line=line, wod=wod,
                     sincosf=sincosf)


def _compare(env, creatures, width, height, sincosf, cam=None, **kw):
    import torch
    from gym_rem2d_amd import render as R
    got = R.render_frames(env, creatures, width, height, camera=cam, **kw).cpu().numpy()
    camxy = (R.follow_camera(env, creatures) if cam is None else torch.as_tensor(cam, dtype=torch.float32)).cpu().numpy()
    fill, line = kw.get("fill"), kw.get("line")
    for k, c in enumerate(creatures):
        _, _, (wi, e) = _scene(env, c)
        f = None if fill is None else np.asarray(fill.cpu() if hasattr(fill, "cpu") else fill)[e]
        l_ = None if line is None else np.asarray(line.cpu() if hasattr(line, "cpu") else line)[e]
        want = _model(env, c, camxy[k], width, height, sincosf, fill=f, line=l_)
        if not np.array_equal(got[k], want):
            bad = np.argwhere(np.any(got[k] != want, axis=-1))
            pytest.fail("creature %d (%d x %d): %d pixels differ, first %s: kernel %s model %s" % (
                c, width, height, len(bad), bad[0].tolist(), got[k][tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist()))
