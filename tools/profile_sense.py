"""Figures of the terrain range sensing: 65 536 config-3 creatures (L-system) on the rough and on the hardcore
track, the device time of rem2d_worlds_sense with the 10 default rays beside rem2d_worlds_observe, and env-steps/s of the loop
observe + sense -> one elementwise torch policy -> set_joint_targets -> step(1) against the bare step(1) loop of the same process.

    python tools/profile_sense.py [--out profiles/sense_figures.json] [--trace] [--n 65536] [--steps 300] [--only-kernels]

--trace adds, per track, the kernels' rows of a `rocprofv3 --kernel-trace --stats -- python tools/profile_sense.py --only-kernels`
run of its own (a child process).  --only-kernels: 20 steps, then 50 observe / sense calls, nothing else.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from profile_control import policy, timed  # noqa: E402


def make_env(n, hardcore):
    import torch
    from gym_rem2d_amd import _lib, synthetic
    from gym_rem2d_amd.env import BatchedModular2D
    env = BatchedModular2D(hardcore=hardcore, flags=_lib.FLAG_CONTINUOUS)
    env.reset_batches(synthetic.lsystem_batches_native(range(n)), n)
    env.step(20)
    torch.cuda.synchronize()
    return env


def figures(n, steps, hardcore, only_kernels=False):
    import torch
    from gym_rem2d_amd import _lib, control
    env = make_env(n, hardcore)
    M = env.max_bodies
    lay = control.layout(M)
    dev = env.worlds[0][0].device
    res = {"creatures": n, "track": "hardcore" if hardcore else "rough", "rays": 10, "worlds": len(env.worlds),
           "static_proxies": len(env._terrain().xs) - 1 + len(env._terrain().polys)}
    env.sense_terrain()
    obs_ms, _ = timed(lambda: env.observe(), 50)
    sense_ms, sense_wall = timed(lambda: env.sense_terrain(), 50)
    hit_ms, _ = timed(lambda: env.sense_terrain(hits=True), 50)
    frac = env.sense_terrain()
    res["observe_call_ms"] = round(obs_ms, 4)
    res["sense"] = {"call_ms": round(sense_ms, 4), "with_hits_call_ms": round(hit_ms, 4), "host_wall_ms": round(sense_wall, 4),
                    "words_written_over_observe": round(10.0 / control.width(M), 4),
                    "time_over_observe": round(sense_ms / obs_ms, 3), "rays_without_a_hit": round(float((frac == 1.0).float().mean()), 4)}
    if only_kernels:
        env.close()
        return res
    ref = torch.linspace(-0.5, 0.5, M, dtype=torch.float32, device=dev)

    def closed():
        env.set_joint_targets(policy(env.observe(), lay, 0.3, ref))
        env.step(1)

    def closed_lidar():
        ahead = env.sense_terrain()[:, 5:].min(dim=1).values
        env.set_joint_targets((policy(env.observe(), lay, 0.3, ref) + 0.5 * (1.0 - ahead)[:, None]).clamp_(-1.5, 1.5))
        env.step(1)
    for name, fn in (("bare_step1_loop", lambda: env.step(1)), ("closed_loop", closed), ("closed_loop_with_sense", closed_lidar),
                     ("bare_step1_loop_again", lambda: env.step(1))):
        ms, wall = timed(fn, steps)
        res[name] = {"ms_per_step": round(ms, 4), "host_wall_ms_per_step": round(wall, 4), "env_steps_per_s": round(n / (ms / 1e3), 1)}
    res["sense_cost_in_the_loop_ms"] = round(res["closed_loop_with_sense"]["ms_per_step"] - res["closed_loop"]["ms_per_step"], 4)
    assert not bool((env.errors() & _lib.ERR_HANDOVER).any())
    env.close()
    return res


def kernel_trace(n, hardcore):
    """rocprofv3 --kernel-trace --stats over a child run of --only-kernels -> the library's kernels' rows of the statistics."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--only-kernels", "--n", str(n)] + (["--hardcore"] if hardcore else [])
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                rows += [r for r in csv.DictReader(f)]
    return [r for r in rows if "rem2d_sense" in r.get("Name", "") or "rem2d_observe" in r.get("Name", "")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--only-kernels", action="store_true")
    ap.add_argument("--hardcore", action="store_true", help="with --only-kernels: the hardcore track instead of the rough one")
    a = ap.parse_args()
    if a.only_kernels:
        print(json.dumps(figures(a.n, a.steps, a.hardcore, True), indent=1))
        return
    res = {"command": "python tools/profile_sense.py" + (" --trace" if a.trace else "") + " --n %d --steps %d" % (a.n, a.steps)}
    for hardcore in (False, True):
        r = figures(a.n, a.steps, hardcore)
        if a.trace:
            r["kernel_trace"] = kernel_trace(a.n, hardcore)
        res[r["track"]] = r
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
