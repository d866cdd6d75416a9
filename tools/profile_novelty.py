"""Figures of behavioural novelty on the device at the workload's own shape: 65 536 descriptors.

    python tools/profile_novelty.py [--out profiles/novelty_figures.json] [--n 65536] [--reps 30] [--episode-n 65536]

* score (rem2d_novelty_score) at k = 15, B in {8, 32}, S in {16, 1 024, 65 536}, with an empty archive and with 1 024 live entries
  per block; add (rem2d_novelty_add) at rate 0.02 on the same shapes: device events around every single call, median of --reps
  calls after 5 warm-up calls, into buffers made once (the calls allocate nothing, which is checked).  Distances per second are
  computed from the shapes: rows x (S - 1 + live entries).
* the same score in torch on the same device: cdist of each block against its peers and entries, the diagonal set to inf, topk of
  the k smallest, mean -- timed the same way, with the peak of torch.cuda.max_memory_allocated above what was held before.  Its
  [S + A][S] float temporary is 17 GB for one block of 65 536: tried only where twice that is free, and reported as not fitting
  otherwise.  It fuses products as it likes and is not reproducible.
* describe (rem2d_worlds_describe) at K = 4 and K = 16 on config 3's population (L-system creatures, flat track).
* what descriptors cost a closed-loop episode: evaluate.run_behaviour_episode (4 samples) against run_policy_episode(compact=False)
  on that population, alternating, wall-clock medians of 3 episodes each of --episode-steps steps.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def torch_score(torch, desc, entries, S, k):
    """[G] float32: mean distance to the k nearest among the block's other rows and its entries"""
    M = desc.shape[0] // S
    x = desc.view(M, S, -1)
    d = torch.cdist(x, x)
    d.diagonal(dim1=1, dim2=2).fill_(float("inf"))
    if entries is not None and entries.shape[1]:
        d = torch.cat((d, torch.cdist(x, entries)), dim=2)
    kk = min(k, d.shape[2])
    return d.topk(kk, dim=2, largest=False).values.mean(dim=2).view(-1)


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "calls": len(ms)}


def kernel_figures(n, reps):
    import torch
    from gym_rem2d_amd import novelty
    from profile_policy import each_call_ms
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    out, k = [], 15
    nov = torch.zeros(n, dtype=torch.float64, device=dev)
    for B in (8, 32):
        desc = torch.randn((n, B), generator=gen, device=dev, dtype=torch.float32)
        for S in (16, 1024, 65536):
            if n % S:
                continue
            M = n // S
            for live in (0, 1024):
                a = novelty.NoveltyArchive(M, 1024, B, device=dev)
                a.entries.copy_(torch.randn(a.entries.shape, generator=gen, device=dev, dtype=torch.float32))
                a.total.fill_(live)
                row = {"B": B, "S": S, "blocks": M, "k": k, "live_entries_per_block": live, "rows": n}
                torch.cuda.synchronize()
                held = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                ms = each_call_ms(lambda: a.score(desc, k=k, group_size=S, out=nov), reps)
                assert torch.cuda.max_memory_allocated() == held, "score allocated device memory"
                dists = n * (S - 1 + live)
                row["score"] = dict(summary(ms), distances=dists, g_distances_per_s=round(dists / (statistics.median(ms) * 1e-3) / 1e9, 2))
                if live:
                    g = [0]

                    def add():
                        g[0] += 1
                        a.add(desc, g[0], seed=3, rate=0.02, group_size=S)
                    ms = each_call_ms(add, reps)
                    assert torch.cuda.max_memory_allocated() == held, "add allocated device memory"
                    row["add_rate_0.02"] = dict(summary(ms), rows_read_bytes=n * B * 4)
                # the comparator, where its temporaries fit
                need = 4 * n * (S + live) * 2
                free = torch.cuda.mem_get_info(dev)[0]
                if need * 2 < free:
                    entries = a.entries[:, :live] if live else None
                    torch.cuda.synchronize()
                    held = torch.cuda.memory_allocated()
                    torch.cuda.reset_peak_memory_stats()
                    try:
                        ms = each_call_ms(lambda: torch_score(torch, desc, entries, S, k), min(reps, 10 if S > 1024 else reps), warm=2)
                        row["torch_cdist_topk"] = dict(summary(ms), peak_bytes_above_held=int(torch.cuda.max_memory_allocated() - held))
                    except RuntimeError as err:          # (out of memory: said, not hidden)
                        row["torch_cdist_topk"] = {"does_not_fit": str(err)[:120]}
                else:
                    row["torch_cdist_topk"] = {"does_not_fit": "needs about %.1f GB of temporaries, %.1f GB free" % (need / 1e9, free / 1e9)}
                out.append(row)
                print(json.dumps(row), flush=True)
                del a
                torch.cuda.empty_cache()
    return out


def episode_figures(n, steps, reps):
    import torch
    from gym_rem2d_amd import _lib, evaluate, novelty, synthetic
    from gym_rem2d_amd.env import BatchedModular2D
    from profile_policy import device_policy, each_call_ms
    env = BatchedModular2D(flat=True, flags=_lib.FLAG_CONTINUOUS)
    env.reset_batches(synthetic.lsystem_batches_native(range(n)), n)
    dev = env.worlds[0][0].device
    env.set_policy(device_policy(n, env.max_bodies, 32, 10, dev, 2))
    everyone = torch.ones(n, dtype=torch.uint8, device=dev)
    out = {"creatures": n, "worlds": len(env.worlds), "describe": {}}
    worlds = env._control_worlds()
    for K in (4, 16):
        buf = torch.zeros((n, 2 * K), dtype=torch.float32, device=dev)
        ms = each_call_ms(lambda: novelty.describe(worlds, 1, K, buf), reps)
        out["describe"]["K=%d" % K] = dict(summary(ms), bytes_written=n * 2 * K * 4)
    period = -(-steps // 4)

    def timed(fn):
        env.reset_where(mask=everyone)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    plain, described = [], []
    timed(lambda: evaluate.run_policy_episode(env, max_steps=steps, chunk=period, compact=False, on_error="ignore"))   # (warm-up)
    for _ in range(3):
        plain.append(timed(lambda: evaluate.run_policy_episode(env, max_steps=steps, chunk=period, compact=False, on_error="ignore")))
        described.append(timed(lambda: evaluate.run_behaviour_episode(env, period, 4, max_steps=steps, on_error="ignore")))
    out["episode"] = {"steps": steps, "samples": 4, "period": period, "run_policy_episode_s": [round(t, 4) for t in plain],
                      "run_behaviour_episode_s": [round(t, 4) for t in described],
                      "median_ratio": round(statistics.median(described) / statistics.median(plain), 4)}
    env.close()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--episode-n", type=int, default=65536)
    ap.add_argument("--episode-steps", type=int, default=200)
    a = ap.parse_args()
    res = {"command": "python tools/profile_novelty.py --n %d --reps %d --episode-n %d --episode-steps %d" % (a.n, a.reps, a.episode_n, a.episode_steps),
           "kernels": kernel_figures(a.n, a.reps), "closed_loop": episode_figures(a.episode_n, a.episode_steps, a.reps)}
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
