"""Figures of the closed loop: 65 536 config-3 creatures (L-system, flat terrain), the device time of
rem2d_worlds_observe and rem2d_worlds_control, and env-steps/s of the loop observe -> one elementwise torch policy ->
set_joint_targets -> step(1) against the bare step(1) loop of the same process.

    python tools/profile_control.py [--out profiles/control_figures.json] [--trace profiles/control_kernel_trace.json]
                                    [--n 65536] [--steps 300] [--only-kernels]

--trace runs `rocprofv3 --kernel-trace --stats -- python tools/profile_control.py --only-kernels` as a child process of its own
and writes the per-kernel rows of its statistics.  --only-kernels: 20 steps, then 50 observe / control calls, nothing else.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_env(n):
    import torch
    from gym_rem2d_amd import _lib, synthetic
    from gym_rem2d_amd.env import BatchedModular2D
    env = BatchedModular2D(flat=True, flags=_lib.FLAG_CONTINUOUS)
    env.reset_batches(synthetic.lsystem_batches_native(range(n)), n)
    env.step(20)
    torch.cuda.synchronize()
    return env


def timed(fn, reps):
    """(device ms per call, host wall ms per call) of fn() over reps calls on the current stream."""
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, (time.perf_counter() - t0) / reps * 1e3


def policy(obs, lay, gain, ref):
    """The reflex of INTEGRATION.md 6, elementwise on the device: hold a reference pose, give way by the observed joint angle, stop
    pushing with bodies that are off the ground."""
    body = lay.bodies(obs)
    return ((ref - gain * body[..., 0]) * (body[..., 3] > 0)).clamp_(-1.5, 1.5)


def figures(n, steps, only_kernels=False):
    import torch
    from gym_rem2d_amd import _lib, control
    env = make_env(n)
    M = env.max_bodies
    lay = control.layout(M)
    dev = env.worlds[0][0].device
    targets = torch.zeros((n, M), dtype=torch.float64, device=dev)
    res = {"creatures": n, "max_bodies": M, "worlds": len(env.worlds), "lane_buckets": sorted({w.lanes for w, _ in env.worlds}),
           "row_bytes": 4 * control.width(M)}
    obs_ms, obs_wall = timed(lambda: env.observe(), 50)
    ctl_ms, ctl_wall = timed(lambda: env.set_joint_targets(targets), 50)
    # rough lower estimates of the bytes a call moves, not counters: observe loads 10 four-byte words per arena lane (six pose /
    # velocity fields, shape, parent, limit state, pair count) plus one C_INFO word per pair, which is left out, and writes the rows;
    # control (target mode) loads shape and parent per lane and, per jointed lane, one double and stores two
    lanes = sum(w.n_envs_padded * w.lanes for w, _ in env.worlds)
    res["observe"] = {"call_ms": round(obs_ms, 4), "host_wall_ms": round(obs_wall, 4),
                      "GB_moved_estimate": round((lanes * 4 * 10 + n * 4 * control.width(M)) / 1e9, 5)}
    res["control"] = {"call_ms": round(ctl_ms, 4), "host_wall_ms": round(ctl_wall, 4),
                      "GB_moved_estimate": round(lanes * (4 * 2 + 8 * 3) / 1e9, 5)}
    if only_kernels:
        env.close()
        return res
    ref = torch.linspace(-0.5, 0.5, M, dtype=torch.float32, device=dev)

    def closed():
        env.set_joint_targets(policy(env.observe(), lay, 0.3, ref))
        env.step(1)
    for name, fn in (("bare_step1_loop", lambda: env.step(1)), ("closed_loop", closed), ("bare_step1_loop_again", lambda: env.step(1))):
        ms, wall = timed(fn, steps)
        res[name] = {"ms_per_step": round(ms, 4), "host_wall_ms_per_step": round(wall, 4), "env_steps_per_s": round(n / (ms / 1e3), 1)}
    ms, _ = timed(lambda: env.step(100), 3)
    res["step100_calls"] = {"ms_per_step": round(ms / 100, 4), "env_steps_per_s": round(n / (ms / 100 / 1e3), 1)}
    res["closed_loop_cost_over_bare_ms"] = round(res["closed_loop"]["ms_per_step"] - res["bare_step1_loop"]["ms_per_step"], 4)
    assert not bool((env.errors() & _lib.ERR_HANDOVER).any())
    env.close()
    return res


def kernel_trace(n, out):
    """rocprofv3 --kernel-trace --stats over a child run of --only-kernels -> the kernels' rows of the statistics."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--only-kernels", "--n", str(n)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                rows += [r for r in csv.DictReader(f)]
    keep = [r for r in rows if "rem2d_" in r.get("Name", "")]
    text = json.dumps({"command": "rocprofv3 --kernel-trace --stats -- python tools/profile_control.py --only-kernels --n %d" % n,
                       "kernels": keep}, indent=1)
    with open(out, "w") as f:
        f.write(text + "\n")
    return keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--only-kernels", action="store_true")
    a = ap.parse_args()
    res = figures(a.n, a.steps, a.only_kernels)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if a.trace:
        for r in kernel_trace(a.n, a.trace):
            if "observe" in r["Name"] or "control" in r["Name"]:
                print(r)


if __name__ == "__main__":
    main()
