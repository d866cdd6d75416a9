"""Figures of the recurrent device policy at the workload's own shape: 65 536 rows with per-row weights,
(MB, R, K, H) = (16, 10, 32, 32).

    python tools/profile_recurrent.py [--out profiles/policy_recurrent.txt] [--n 65536] [--reps 30] [--rounds 3]

* the kernel: rem2d_recurrent_forward against the yardstick rem2d_policy_forward at (MB, R, H) = (16, 42, 32) -- the same d, the
  same weight bytes, the untouched feed-forward kernel.  Device events around every single call, median of --reps calls after 5
  warm-up calls; the two alternate --rounds times in one visit, and the spread of the feed-forward rounds is what a difference has to
  exceed.  The extra traffic from the shapes: 2 * 4 K bytes per row (the context read, the memory written).
* the closed loop: one step_policy(1) under set_autoreset(("steps",), 7) on --n L-system creatures, with a feed-forward policy
  (R 10, H 32) and with a recurrent one (R 10, K 32, H 32: its reset mask is read every step), timed the same way.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def draw(torch, sets, max_bodies, hidden, inputs, dev, seed):
    """profile_policy.device_policy's draw as four arrays, with `inputs` words after the observation row"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    D = 8 + 6 * max_bodies + inputs
    shapes = ((sets, D, hidden), (sets, hidden), (sets, hidden, max_bodies), (sets, max_bodies))
    return [torch.randn(s, generator=gen, device=dev, dtype=torch.float32) * sd for s, sd in zip(shapes, (0.3, 0.3, 0.5, 0.3))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-loop", action="store_true", help="the kernel figures alone")
    a = ap.parse_args()
    import torch
    from gym_rem2d_amd import _lib, policy, sense, synthetic
    from gym_rem2d_amd.env import BatchedModular2D
    from profile_policy import device_policy, each_call_ms
    dev = torch.device("cuda:0")
    n, MB, R, K, H = a.n, 16, 10, 32, 32
    lines = ["python tools/profile_recurrent.py --n %d --reps %d --rounds %d" % (n, a.reps, a.rounds), ""]

    # ---- the kernel against the feed-forward kernel at the same d
    ff = policy.MLPPolicy(*draw(torch, n, MB, H, R + K, dev, 1), rays=sense.bipedal_rays(R + K))
    rec = policy.RecurrentPolicy(ff.w1, ff.b1, ff.w2, ff.b2, K)
    assert rec.d == ff.d and rec.weight_bytes() == ff.weight_bytes()
    gen = torch.Generator(device="cpu").manual_seed(3)
    obs = torch.randn((n, 8 + 6 * MB), generator=gen).to(dev)
    frac2 = torch.rand((n, R + K), generator=gen).to(dev)
    frac = frac2[:, :R].contiguous()
    mem = frac2[:, R:].contiguous()
    reset = (torch.arange(n, device=dev) % 7 == 0).to(torch.uint8)
    res = (torch.zeros((n, MB), dtype=torch.float64, device=dev), torch.zeros((n, MB), dtype=torch.uint8, device=dev))
    forms = (("rem2d_policy_forward (16, 42, 32)", lambda: ff.forward(obs, frac2, out=res)),
             ("rem2d_recurrent_forward (16, 10, 32, 32)", lambda: rec.forward(obs, frac, mem, out=res)),
             ("... with a reset mask (1 row in 7)", lambda: rec.forward(obs, frac, mem, reset=reset, out=res)))
    got = {name: [] for name, _ in forms}
    for _ in range(a.rounds):
        for name, fn in forms:
            got[name].append(each_call_ms(fn, a.reps))
    set_bytes, extra = ff.weight_bytes(), 2 * 4 * K
    lines.append("%d rows, per-row weight sets of %d B, d = %d; device events, median of %d calls after 5 warm-up calls, %d alternating "
                 "rounds" % (n, set_bytes, ff.d, a.reps, a.rounds))
    lines.append("extra traffic of the recurrent pass from the shapes: %d B per row = %.2f %% of a weight set" % (extra, 100.0 * extra / set_bytes))
    med = {}
    for name, _ in forms:
        rounds = [statistics.median(r) for r in got[name]]
        every = [v for r in got[name] for v in r]
        med[name] = statistics.median(every)
        lines.append("%-42s median %8.4f ms  (calls: min %8.4f  max %8.4f; round medians: %s)" % (
            name, med[name], min(every), max(every), ", ".join("%.4f" % v for v in rounds)))
    base = forms[0][0]
    ff_rounds = [statistics.median(r) for r in got[base]]
    spread = (max(ff_rounds) - min(ff_rounds)) / med[base]
    lines.append("spread of the feed-forward round medians: %.2f %% of their median" % (100.0 * spread))
    for name, _ in forms[1:]:
        lines.append("%-42s %+.2f %% against the feed-forward median (expected from the shapes: %+.2f %%)" % (
            name, 100.0 * (med[name] / med[base] - 1.0), 100.0 * extra / set_bytes))
    lines.append("")
    del ff, rec, obs, frac2, frac, mem, res
    torch.cuda.empty_cache()

    # ---- one step of the closed loop under auto-reset, with and without memory
    if not a.no_loop:
        env = BatchedModular2D(flat=True, flags=_lib.FLAG_CONTINUOUS)
        env.reset_batches(synthetic.lsystem_batches_native(range(n)), n)
        edev = env.worlds[0][0].device
        plain = device_policy(n, env.max_bodies, H, R, edev, 2)
        memory = policy.RecurrentPolicy(*draw(torch, n, env.max_bodies, H, R + K, edev, 2), K)
        env.set_autoreset(("steps",), 7)
        lines.append("one step_policy(1) under set_autoreset(('steps',), 7), %d L-system creatures (max_bodies %d, %d worlds): act, step, "
                     "reset_where" % (n, env.max_bodies, len(env.worlds)))
        loop = {}
        for _ in range(a.rounds):
            for name, pol in (("feed-forward (R 10, H 32, %d B a set)" % plain.weight_bytes(), plain),
                              ("recurrent (R 10, K 32, H 32, %d B a set)" % memory.weight_bytes(), memory)):
                env.set_policy(pol)
                loop.setdefault(name, []).append(each_call_ms(lambda: env.step_policy(1), a.reps))
        for name, rounds in loop.items():
            every = [v for r in rounds for v in r]
            lines.append("%-46s median %8.4f ms  (calls: min %8.4f  max %8.4f; round medians: %s)" % (
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
