"""Figures of the episode boundaries: the masked reset alone on config 3's population (65 536 L-system creatures, flat
terrain) beside the full reset of the same worlds, and the closed loop with and without auto-reset.

    python tools/profile_episodes.py [--out profiles/episode_figures.json] [--n 65536] [--steps 200] [--reps 30] [--rounds 3]
    python tools/profile_episodes.py --reset-only        # rem2d_world_reset alone: runs on a tree without the episode ABI too

* reset: device events around every single call, median of --reps calls after warm-up.  reset_where with a mask that selects 0 %, 1 %
  and 100 % of the creatures (one library call for all worlds), and rem2d_world_reset on every world of the same env (one call per
  world, all of them inside one event pair).  Bytes are computed from the shapes -- per selected lane the 33 words, 5 doubles and
  8 x REM2D_CONTACT_SLOTS slot words a reset writes and the 15 words and 5 doubles of the morphology it reads, per selected creature
  its 10 words and 2 doubles -- and reported as a share of 6.3 TB/s; they are no counters.
* loop: env-steps/s of step_policy(steps) with set_autoreset(("done", "steps"), 4800) and without, on the same env, alternating,
  --rounds rounds, medians.  The difference is what the extra launch per step costs.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES_PER_S = 6.3e12


def each_call_ms(fn, reps, warm=5):
    """device ms of every one of reps calls of fn() (an event pair each), after warm calls"""
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in pairs]


def summary(ms, moved=None):
    med = statistics.median(ms)
    out = {"calls": len(ms), "median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}
    if moved is not None:
        out.update({"bytes_from_the_shapes": int(moved), "gbytes_per_s": round(moved / (med * 1e-3) / 1e9, 1),
                    "share_of_6.3_TB_per_s": round(moved / (med * 1e-3) / PEAK_BYTES_PER_S, 4)})
    return out


def make_env(n):
    from gym_rem2d_amd import _lib, synthetic
    from gym_rem2d_amd.env import BatchedModular2D
    env = BatchedModular2D(flat=True, flags=_lib.FLAG_CONTINUOUS)
    env.reset_batches(synthetic.lsystem_batches_native(range(n)), n)
    return env


def reset_bytes(env, selected):
    """bytes a reset of the creatures `selected` (bool [N] host array, or None: everyone incl. padding lanes) writes and reads"""
    slots = env.worlds[0][0].contact_slots
    lane_w, lane_r, env_w = 33 * 4 + 5 * 8 + 8 * slots * 4, 15 * 4 + 5 * 8, 10 * 4 + 2 * 8
    total = 0
    for w, idx in env.worlds:
        k = w.n_envs if selected is None else int(selected[idx.cpu().numpy()].sum())
        total += k * (w.lanes * (lane_w + lane_r) + env_w)
    return total


def full_reset_figures(env, reps):
    """rem2d_world_reset on every world of the env, from the device morphology its upload left"""
    from gym_rem2d_amd import _lib
    calls = []
    for w, _ in env.worlds:
        m = _lib.Morph()
        for k in _lib.MORPH_FIELDS:
            setattr(m, k, w._morph_dev[k].data_ptr())
        calls.append((w, m))

    def fn():
        for w, m in calls:
            _lib.check(w.L.rem2d_world_reset(w.h, C.byref(m), w._stream()), w.wide)
    out = summary(each_call_ms(fn, reps), reset_bytes(env, None))
    out["launches_per_call"] = len(calls)
    return out


def reset_figures(n, reps, reset_only):
    import numpy as np
    import torch
    env = make_env(n)
    env.step(20)
    out = {"creatures": n, "population": "config 3: L-system seeds 0..%d, flat terrain" % (n - 1), "worlds": len(env.worlds),
           "lanes": sorted({w.lanes for w, _ in env.worlds}), "contact_slots": env.worlds[0][0].contact_slots,
           "arena_lanes": sum(w.n_envs_padded * w.lanes for w, _ in env.worlds)}
    out["world_reset"] = full_reset_figures(env, reps)
    if not reset_only:
        dev = env.worlds[0][0].device
        rng = np.random.default_rng(1)
        for name, share in (("reset_where_0_percent", 0.0), ("reset_where_1_percent", 0.01), ("reset_where_100_percent", 1.0)):
            sel = np.ones(n, bool) if share == 1.0 else rng.random(n) < share
            mask = torch.from_numpy(sel).to(dev)
            ms = each_call_ms(lambda: env.reset_where(mask), reps)
            out[name] = summary(ms, reset_bytes(env, sel))
            out[name]["selected"] = int(sel.sum())
            assert int(env.episodes.ended.sum()) == int(sel.sum())
    env.close()
    return out


def loop_figures(n, steps, rounds):
    import torch
    from gym_rem2d_amd import _lib
    from profile_policy import device_policy
    env = make_env(n)
    env.set_policy(device_policy(n, env.max_bodies, 32, 10, env.worlds[0][0].device, 2))
    env.step(20)
    torch.cuda.synchronize()

    def rate(auto):
        env.set_autoreset(("done", "steps"), 4800) if auto else env.set_autoreset(None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env.step_policy(steps)
        torch.cuda.synchronize()
        return n * steps / (time.perf_counter() - t0)
    forms = (("step_policy_autoreset", True), ("step_policy", False))
    for _, auto in forms:      # warm-up: both forms once
        rate(auto)
    got = {name: [] for name, _ in forms}
    for _ in range(rounds):
        for name, auto in forms:
            got[name].append(rate(auto))
    res = {"creatures": n, "steps_per_call": steps, "rounds": rounds, "worlds": len(env.worlds), "when": ["done", "steps"], "max_steps": 4800,
           "episodes_ended": int(env.episodes.count.sum())}
    for name, v in got.items():
        res[name] = {"env_steps_per_s": round(statistics.median(v), 1), "all": [round(x, 1) for x in v],
                     "ms_per_step": round(n / statistics.median(v) * 1e3, 4)}
    res["autoreset_cost_ms_per_step"] = round(res["step_policy_autoreset"]["ms_per_step"] - res["step_policy"]["ms_per_step"], 4)
    assert not bool((env.errors() & _lib.ERR_HANDOVER).any())
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reset-only", action="store_true", help="rem2d_world_reset alone (a tree without the episode ABI)")
    a = ap.parse_args()
    from gym_rem2d_amd import _lib
    res = {"command": "python tools/profile_episodes.py --n %d --steps %d --reps %d --rounds %d%s"
                      % (a.n, a.steps, a.reps, a.rounds, " --reset-only" if a.reset_only else ""),
           "build_id": _lib.build_id(), "reset": reset_figures(a.n, a.reps, a.reset_only)}
    if not a.reset_only:
        res["loop"] = loop_figures(a.n, a.steps, a.rounds)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
