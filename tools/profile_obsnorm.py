"""Figures of the observation normaliser at the workload's own shape: 65 536 rows, (MB, R, H) = (16, 10, 32), in
blocks of 16 and as one block.

    python tools/profile_obsnorm.py [--out profiles/obsnorm_figures.json] [--n 65536] [--reps 30] [--rounds 3] [--no-loop]

* accumulate: rem2d_obsnorm_accumulate, device events around every call, median of --reps calls after 5 warm-up calls, against the
  time its read (n x 114 x 4 bytes) would take at the 6.3 TB/s this chip's copies reach (profiles/README.md); the fraction, no
  threshold.  At every row_chunk of --chunks too.
* forward: the normalised pass without accumulation against the plain pass (whose code objects are the parent's, byte for byte:
  DESIGN.md 23), alternating, --rounds each; the plain rounds' spread is what a difference has to exceed.
* freeze: the tables of 4 096 blocks and of one.
* act(): one act() on --n L-system creatures without a normaliser, with one that only applies and with one that accumulates.
* the same statistics and apply in torch: a masked mean / variance per block and a normalised copy of the rows; time and the peak
  of the allocator above what was live before.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_TBS = 6.3


def rounds_of(forms, rounds, reps, each_call_ms):
    got = {name: [] for name, _ in forms}
    for _ in range(rounds):
        for name, fn in forms:
            got[name].append(each_call_ms(fn, reps))
    out = {}
    for name, _ in forms:
        every = [v for r in got[name] for v in r]
        out[name] = dict(median_ms=statistics.median(every), min_ms=min(every), max_ms=max(every),
                         round_medians_ms=[statistics.median(r) for r in got[name]])
    return out


def torch_stats(torch, x, S, mask):
    """what a user would write: per-block masked mean / std of the finite rows, then the normalised, clipped copy"""
    n, D = x.shape
    ok = torch.isfinite(x).all(dim=1) & (mask != 0)
    xb = torch.where(ok[:, None], x, torch.zeros((), device=x.device)).view(n // S, S, D)
    cnt = ok.view(n // S, S).sum(dim=1).clamp(min=1).to(torch.float32)[:, None]
    mean = xb.sum(dim=1) / cnt
    var = (xb * xb).sum(dim=1) / cnt - mean * mean
    inv = torch.where(var >= 2.0 ** -20, var.clamp(min=1e-30).rsqrt(), torch.zeros((), device=x.device))
    return ((x.view(n // S, S, D) - mean[:, None]) * inv[:, None]).clamp(-5.0, 5.0).view(n, D)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunks", default="0,8,16,64,256")
    ap.add_argument("--no-loop", action="store_true", help="the array figures alone")
    a = ap.parse_args()
    import torch
    from gym_rem2d_amd import _lib, policy, synthetic
    from gym_rem2d_amd.env import BatchedModular2D
    from profile_policy import device_policy, each_call_ms
    dev = torch.device("cuda:0")
    n, MB, R, H = a.n, 16, 10, 32
    Dn = policy.input_width(MB, R)
    fig = dict(command="python tools/profile_obsnorm.py --n %d --reps %d --rounds %d" % (n, a.reps, a.rounds), rows=n, max_bodies=MB,
               n_rays=R, hidden=H, words=Dn, hbm_tb_per_s=HBM_TBS, build_id=_lib.build_id())
    gen = torch.Generator(device="cpu").manual_seed(3)
    obs = (torch.randn((n, 8 + 6 * MB), generator=gen) * 3.0).to(dev)
    obs[:, 0] += 50.0
    frac = torch.rand((n, R), generator=gen).to(dev)
    mask = (torch.arange(n, device=dev) % 9 != 0).to(torch.uint8)
    read_bytes = n * Dn * 4
    floor_ms = read_bytes / (HBM_TBS * 1e12) * 1e3
    fig["accumulate_read_bytes"], fig["accumulate_read_floor_ms"] = read_bytes, floor_ms
    pol = device_policy(n, MB, H, R, dev, 1)
    res = (torch.zeros((n, MB), dtype=torch.float64, device=dev), torch.zeros((n, MB), dtype=torch.uint8, device=dev))
    for label, S in (("blocks_of_16", 16), ("one_block", n)):
        norm = policy.ObsNormalizer(n // S, S, MB, R, device=dev)
        sec = {}
        forms = [("row_chunk %s" % c, (lambda c=int(c): norm.accumulate(obs, frac, row_mask=mask, row_chunk=c))) for c in a.chunks.split(",")]
        sec["accumulate"] = rounds_of(forms, a.rounds, a.reps, each_call_ms)
        for v in sec["accumulate"].values():
            v["read_floor_over_median"] = floor_ms / v["median_ms"]
        norm.freeze()
        forms = [("rem2d_policy_forward", lambda: pol.forward(obs, frac, out=res)),
                 ("rem2d_obsnorm_forward", lambda: norm.forward(pol, obs, frac, out=res))]
        sec["forward"] = rounds_of(forms, a.rounds, a.reps, each_call_ms)
        plain = sec["forward"]["rem2d_policy_forward"]
        sec["forward"]["plain_round_spread"] = (max(plain["round_medians_ms"]) - min(plain["round_medians_ms"])) / plain["median_ms"]
        sec["forward"]["normed_over_plain"] = sec["forward"]["rem2d_obsnorm_forward"]["median_ms"] / plain["median_ms"]
        sec["freeze"] = rounds_of([("rem2d_obsnorm_freeze", lambda: norm.freeze())], 1, a.reps, each_call_ms)
        # the same in torch
        x = torch.cat([obs, frac], dim=1)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        live = torch.cuda.memory_allocated()
        ms = each_call_ms(lambda: torch_stats(torch, x, S, mask), a.reps)
        sec["torch_stats_and_apply"] = dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms),
                                            peak_temporaries_bytes=torch.cuda.max_memory_allocated() - live)
        del x
        fig[label] = sec
        norm.reset()
    del pol, obs, frac, res
    torch.cuda.empty_cache()
    if not a.no_loop:
        env = BatchedModular2D(flat=True, flags=_lib.FLAG_CONTINUOUS)
        env.reset_batches(synthetic.lsystem_batches_native(range(n)), n)
        edev = env.worlds[0][0].device
        pol = device_policy(n, env.max_bodies, H, R, edev, 2)
        norm = policy.ObsNormalizer(n // 16, 16, env.max_bodies, R, device=edev)
        env.step(5)
        forms = (("act()", {}), ("act(), normaliser applied", dict(normalizer=norm, accumulate=False)),
                 ("act(), normaliser applied and accumulated", dict(normalizer=norm, accumulate=True)))
        got = {name: [] for name, _ in forms}
        for _ in range(a.rounds):
            for name, kw in forms:
                env.set_policy(pol, **kw)
                got[name].append(each_call_ms(env.act, a.reps))
        fig["act"] = dict(creatures=n, max_bodies=env.max_bodies, worlds=len(env.worlds))
        for name, _ in forms:
            every = [v for r in got[name] for v in r]
            fig["act"][name] = dict(median_ms=statistics.median(every), min_ms=min(every), max_ms=max(every),
                                    round_medians_ms=[statistics.median(r) for r in got[name]])
        env.close()
    text = json.dumps(fig, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
