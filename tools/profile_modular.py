"""Figures of the modular device policy at the workload's own shape: 65 536 rows with per-row weight sets,
(MB, R, H, K) = (16, 10, 32, 8), P = 1 and P = 4, bodies per row as in config 3's population (the topology table of --n L-system
creatures), beside rem2d_policy_forward on MLPPolicy(MB 16, R 10, H 32) in the same process.

    python tools/profile_modular.py [--out FILE] [--n 65536] [--reps 30] [--rounds 3]

* the kernels: device events around every single call, median of --reps calls after 5 warm-up calls; the forms alternate --rounds
  times in one visit.  The bytes a call moves, from the shapes: a weight set, the observation row, the ray fractions, the topology
  rows, the messages read and written, the targets and validity bytes.
* the closed loop: act() alone under each policy, timed the same way, and one env step beside it.

The two kernels compute different functions: no ratio here is a pass mark.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    from gym_rem2d_amd import _lib, policy, synthetic
    from gym_rem2d_amd.env import BatchedModular2D
    from profile_policy import device_policy, each_call_ms
    n, MB, R, H, K = a.n, 16, 10, 32, 8
    lines = ["python tools/profile_modular.py --n %d --reps %d --rounds %d" % (n, a.reps, a.rounds), ""]
    env = BatchedModular2D(flat=True, flags=_lib.FLAG_CONTINUOUS)
    env.reset_batches(synthetic.lsystem_batches_native(range(n)), n)
    dev = env.worlds[0][0].device
    topo = env.topology(MB)
    live = int((topo[:, :, 1] != 0).sum())
    ff = device_policy(n, MB, H, R, dev, 2)
    gen = torch.Generator(device=dev).manual_seed(5)
    Dm = 8 + 6 + R + 2 + 2 * K
    sets = [torch.randn(s, generator=gen, device=dev, dtype=torch.float32) * sd
            for s, sd in zip(((n, Dm, H), (n, H), (n, H, 1), (n, 1)), (0.3, 0.3, 0.5, 0.3))]
    mods = {P: policy.ModularPolicy(*sets, messages=K, rounds=P, max_bodies=MB) for P in (1, 4)}
    obs, frac = env.observe(MB).clone(), env.sense_terrain(ff.rays).clone()
    mem = mods[1].new_memory(n)
    res = ff._targets(n)
    forms = [("rem2d_policy_forward (MB 16, R 10, H 32)", lambda: ff.forward(obs, frac, out=res))]
    for P in (1, 4):
        forms.append(("rem2d_modular_forward (K 8, P %d)" % P, lambda P=P: mods[P].forward(obs, frac, topo, mem, out=res)))
    got = {name: [] for name, _ in forms}
    for _ in range(a.rounds):
        for name, fn in forms:
            got[name].append(each_call_ms(fn, a.reps))
    row = 4 * (8 + 6 * MB) + 4 * R + (8 + 1) * MB
    moved = {forms[0][0]: ff.weight_bytes() + row}
    for P in (1, 4):
        moved[forms[1 + (P == 4)][0]] = mods[P].weight_bytes() + row + 8 * MB + 2 * 4 * MB * K
    lines.append("%d rows, %d live bodies (%.2f per row) of %d columns; weight sets: feed-forward %d B, modular %d B; device events, "
                 "median of %d calls after 5 warm-up calls, %d alternating rounds"
                 % (n, live, live / n, MB, ff.weight_bytes(), mods[1].weight_bytes(), a.reps, a.rounds))
    for name, _ in forms:
        every = [v for r in got[name] for v in r]
        med = statistics.median(every)
        lines.append("%-44s median %8.4f ms  (min %8.4f  max %8.4f; round medians: %s)  %6d B a row, %7.1f MB a call, %6.2f TB/s" % (
            name, med, min(every), max(every), ", ".join("%.4f" % statistics.median(r) for r in got[name]), moved[name],
            moved[name] * n / 1e6, moved[name] * n / med / 1e9))
    lines.append("")
    loop = {}
    for _ in range(a.rounds):
        for name, pol in [("feed-forward", ff)] + [("modular P %d" % P, mods[P]) for P in (1, 4)]:
            env.set_policy(pol)
            loop.setdefault("act() " + name, []).append(each_call_ms(lambda: env.act(), a.reps))
        env.set_policy(None)
        loop.setdefault("step(1)", []).append(each_call_ms(lambda: env.step(1), a.reps))
    lines.append("the closed loop on the same %d creatures (%d worlds):" % (n, len(env.worlds)))
    for name, rounds in loop.items():
        every = [v for r in rounds for v in r]
        lines.append("%-44s median %8.4f ms  (min %8.4f  max %8.4f; round medians: %s)" % (
            name, statistics.median(every), min(every), max(every), ", ".join("%.4f" % statistics.median(r) for r in rounds)))
    env.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
