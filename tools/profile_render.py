"""Figures of the renderer ("The renderer"): rem2d_world_render for 1, 64 and 1 024 creatures at 800 x 600, the frames/s of
record_frames over one elite episode against Modular2D.render('rgb_array'), and a show_best episode against a config-3 generation.

    python tools/profile_render.py [--out profiles/render_figures.json] [--only-kernel]

--only-kernel renders the three batch sizes and nothing else (the run to wrap in `rocprofv3 --kernel-trace --stats -- ...`).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_ROOF_GBS = 8000.0   # MI355X HBM3E peak


def kernel_figures(reps=20):
    import torch
    from gym_rem2d_amd import render as R, synthetic
    from gym_rem2d_amd.env import BatchedModular2D
    env = BatchedModular2D()
    env.reset_morphology(synthetic.lsystem_population(1024, lanes=16))   # one world: one launch per call
    env.step(37)
    out = {}
    for n in (1, 64, 1024):
        creatures = list(range(n))
        cam = R.follow_camera(env, creatures)
        frames = torch.empty((n, 600, 800, 3), dtype=torch.uint8, device="cuda")
        for _ in range(3):
            R.render_frames(env, creatures, camera=cam, out=frames)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for _ in range(reps):
            R.render_frames(env, creatures, camera=cam, out=frames)
        b.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / reps * 1e3
        ms = a.elapsed_time(b) / reps
        gb = n * 600 * 800 * 3 / 1e9
        out[str(n)] = {"call_ms": round(ms, 4), "host_wall_ms": round(wall, 4), "GB_written": round(gb, 5),
                       "GBps_per_call": round(gb / (ms / 1e3), 1), "frames_per_s": round(n / (ms / 1e3), 1)}
        del frames
    env.close()
    return out


def _elite():
    """A direct-encoding individual that walks a while: the fittest of 16 seeds."""
    import random
    from gym_rem2d_amd import get_module_list
    from gym_rem2d_amd.ea import Individual
    from gym_rem2d_amd.encodings import DirectEncoding
    from gym_rem2d_amd.evaluate import evaluate_population
    inds = []
    for s in range(16):
        random.seed(s)
        ind = Individual()
        ind.genome = DirectEncoding(get_module_list())
        ind.tree_depth = 8
        inds.append(ind)
    fits = evaluate_population(inds, tree_depth=8)
    best = max(range(16), key=lambda k: fits[k])
    return inds[best], fits[best]


def episode_figures():
    import numpy as np
    import torch
    from gym_rem2d_amd import _lib, render as R
    from gym_rem2d_amd.ea import show_best_episode
    from gym_rem2d_amd.env import BatchedModular2D, Modular2D
    from gym_rem2d_amd.evaluate import EPISODE_CAP
    ind, fit = _elite()
    out = {"elite_fitness": fit}
    # record_frames over the whole episode, frames to the host (no file writing)
    env = BatchedModular2D(flags=_lib.FLAG_CONTINUOUS | _lib.FLAG_SKIP_FROZEN)
    env.reset([ind.genome.create(8)], [ind.genome.moduleList])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for _, frames in R.record_frames(env, EPISODE_CAP, [0], every=5):
        n += 1
    dt = time.perf_counter() - t0
    env.close()
    out["record_frames"] = {"frames": n, "seconds": round(dt, 3), "frames_per_s": round(n / dt, 1)}
    # the same episode through show_best_episode with PNGs written (what run_ea(show_best=True, frames_dir=...) costs)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        f2, n2 = show_best_episode(ind, 8, interval=5, frames_dir=d)
        out["show_best_png"] = {"frames": n2, "seconds": round(time.perf_counter() - t0, 3), "fitness": f2}
        t0 = time.perf_counter()
        f3, n3 = show_best_episode(ind, 8, interval=5, frames_dir=None)
        out["show_best_no_files"] = {"frames": n3, "seconds": round(time.perf_counter() - t0, 3), "fitness": f3}
    # Modular2D.render('rgb_array') (matplotlib, one frame per call)
    m = Modular2D()
    m.seed(4)
    m.reset(tree=ind.genome.create(8), module_list=ind.genome.moduleList)
    m.render(mode="rgb_array")
    ts = []
    for _ in range(10):
        for _ in range(5):
            m.step(np.ones(4))
        t0 = time.perf_counter()
        m.render(mode="rgb_array")
        ts.append(time.perf_counter() - t0)
    m.close()
    out["modular2d_render_rgb_array"] = {"ms_per_frame": round(1e3 * float(np.median(ts)), 2),
                                         "frames_per_s": round(1.0 / float(np.median(ts)), 1)}
    return out


def generation_seconds(n=65536):
    """A config-3 generation: 65 536 L-system creatures on the flat terrain, evaluated to the end (run_episode, compact)."""
    import torch
    from gym_rem2d_amd import _lib, synthetic
    from gym_rem2d_amd.env import BatchedModular2D
    from gym_rem2d_amd.evaluate import run_episode
    env = BatchedModular2D(flat=True, flags=_lib.FLAG_CONTINUOUS | _lib.FLAG_SKIP_FROZEN)
    batches = synthetic.lsystem_batches_native(range(n))
    env.reset_batches(batches, n)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_episode(env, on_error="penalty")
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    env.close()
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-kernel", action="store_true")
    a = ap.parse_args()
    res = {"kernel_800x600": kernel_figures(), "hbm_roof_GBps": HBM_ROOF_GBS}
    if not a.only_kernel:
        res["episode"] = episode_figures()
        g = generation_seconds()
        res["config3_generation_seconds"] = round(g, 3)
        res["show_best_share_of_generation"] = round(res["episode"]["show_best_no_files"]["seconds"] / g, 4)
        res["show_best_png_share_of_generation"] = round(res["episode"]["show_best_png"]["seconds"] / g, 4)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
