"""Figures of the device policies: the forward kernel alone at the workload's own size, and the closed loop against
its parts on config 3's population (65 536 L-system creatures, flat terrain).

    python tools/profile_policy.py [--out profiles/policy_figures.json] [--n 65536] [--steps 200] [--reps 30] [--rounds 3]

* forward: rem2d_policy_forward on n rows, MB 16, R 10, H 32, with one weight set per creature and with one shared set: device
  events around every single call, median of --reps calls after warm-up.  Bytes are computed from the shapes (every weight set, input
  row and output row once) and reported as a share of 6.3 TB/s; they are no counters.
* loop: env-steps/s of step_policy(steps), of steps x step(1) and of step(steps) on the same env, alternating, --rounds rounds,
  medians.  The difference between the first two is what the policy costs; between the last two, what queuing a step at a time costs.
"""
import argparse
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


def device_policy(sets, max_bodies, hidden, n_rays, dev, seed, index=None):
    """MLPPolicy.random's distribution, drawn on the device (65 536 sets are 1.1 GB)"""
    import torch
    from gym_rem2d_amd import policy
    gen = torch.Generator(device=dev).manual_seed(seed)
    D = policy.input_width(max_bodies, n_rays)
    shapes = ((sets, D, hidden), (sets, hidden), (sets, hidden, max_bodies), (sets, max_bodies))
    arrays = [torch.randn(s, generator=gen, device=dev, dtype=torch.float32) * sd for s, sd in zip(shapes, (0.3, 0.3, 0.5, 0.3))]
    return policy.MLPPolicy(*arrays, index=index)


def forward_figures(n, reps, max_bodies=16, n_rays=10, hidden=32):
    import torch
    dev = torch.device("cuda:0")
    out = {"rows": n, "max_bodies": max_bodies, "rays": n_rays, "hidden": hidden}
    gen = torch.Generator(device="cpu").manual_seed(3)
    obs = torch.randn((n, 8 + 6 * max_bodies), generator=gen).to(dev)
    frac = torch.rand((n, n_rays), generator=gen).to(dev)
    for name, sets in (("per_creature", n), ("shared", 1)):
        pol = device_policy(sets, max_bodies, hidden, n_rays, dev, 1, None if sets == n else torch.zeros(n, dtype=torch.int32, device=dev))
        res = (torch.zeros((n, max_bodies), dtype=torch.float64, device=dev), torch.zeros((n, max_bodies), dtype=torch.uint8, device=dev))
        ms = each_call_ms(lambda: pol.forward(obs, frac, out=res), reps)
        moved = sets * pol.weight_bytes() + n * (4 * pol.d + 9 * max_bodies) + (0 if sets == n else 4 * n)
        med = statistics.median(ms)
        out[name] = {"weight_sets": sets, "weight_set_bytes": pol.weight_bytes(), "bytes_from_the_shapes": moved, "calls": reps,
                     "median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                     "gbytes_per_s": round(moved / (med * 1e-3) / 1e9, 1), "share_of_6.3_TB_per_s": round(moved / (med * 1e-3) / PEAK_BYTES_PER_S, 4),
                     "valid_share": round(float(res[1].float().mean()), 4)}
    return out


def loop_figures(n, steps, rounds):
    import torch
    from gym_rem2d_amd import _lib, synthetic
    from gym_rem2d_amd.env import BatchedModular2D
    env = BatchedModular2D(flat=True, flags=_lib.FLAG_CONTINUOUS)
    env.reset_batches(synthetic.lsystem_batches_native(range(n)), n)
    env.set_policy(device_policy(n, env.max_bodies, 32, 10, env.worlds[0][0].device, 2))
    env.step(20)
    torch.cuda.synchronize()

    def rate(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return n * steps / (time.perf_counter() - t0)

    def one_at_a_time():
        for _ in range(steps):
            env.step(1)
    forms = (("step_policy", lambda: env.step_policy(steps)), ("step1_loop", one_at_a_time), ("step_n", lambda: env.step(steps)))
    for _, fn in forms:      # warm-up: every launch form once
        rate(fn)
    got = {name: [] for name, _ in forms}
    for _ in range(rounds):
        for name, fn in forms:
            got[name].append(rate(fn))
    res = {"creatures": n, "population": "config 3: L-system seeds 0..%d, flat terrain" % (n - 1), "steps_per_call": steps, "rounds": rounds,
           "max_bodies": env.max_bodies, "worlds": len(env.worlds)}
    for name, v in got.items():
        res[name] = {"env_steps_per_s": round(statistics.median(v), 1), "all": [round(x, 1) for x in v],
                     "ms_per_step": round(n / statistics.median(v) * 1e3, 4)}
    res["policy_cost_ms_per_step"] = round(res["step_policy"]["ms_per_step"] - res["step1_loop"]["ms_per_step"], 4)
    res["one_step_per_call_cost_ms_per_step"] = round(res["step1_loop"]["ms_per_step"] - res["step_n"]["ms_per_step"], 4)
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
    a = ap.parse_args()
    res = {"command": "python tools/profile_policy.py --n %d --steps %d --reps %d --rounds %d" % (a.n, a.steps, a.reps, a.rounds),
           "forward": forward_figures(a.n, a.reps), "loop": loop_figures(a.n, a.steps, a.rounds)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
