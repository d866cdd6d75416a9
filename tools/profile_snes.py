"""Figures of the adaptive evolution strategy for device policies at the workload's own shape: 65 536 children,
MB 16, R 10, H 32, in blocks of 16 (4 096 means) and in blocks of 8 192 (8 means).

    python tools/profile_snes.py [--out profiles/policy_snes.txt] [--n 65536] [--reps 30] [--groups 16,8192]

* sample and update (util given; plain and with Adam, natural) of policy.SeparableES: device events around every single call, median
  of --reps calls after 5 warm-up calls; the object's own buffers, so the calls allocate nothing, which is checked.
* in the SAME process, rem2d_es_sample / rem2d_es_update (util given) at the same shapes through MLPPolicy.es_sample / es_update
  with out= and scratch=: the cost condition is stated against them -- the new update and the new sample are each to stay within
  1.5 x of the ES's -- and the ratio is printed with a verdict.
* the comparator: the same strategy stated in torch on the same device -- randn noise the size of half the population, children by
  broadcast with a sigma tensor, the update two einsums over the STORED noise (rank differences times noise, rank sums times
  noise squared minus one) -- with the peak of torch.cuda.max_memory_allocated above what was held before the call.  Its float
  sums are not reproducible.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIMIT = 1.5


def torch_sample(torch, mean, sigma, S):
    """-> (children per array, the stored noise per array)"""
    kids, noise = [], []
    for t, sg in zip(mean, sigma):
        M = t.shape[0]
        eps = torch.randn((M, S // 2) + tuple(t.shape[1:]), device=t.device, dtype=torch.float32)
        step = sg[:, None] * eps
        kids.append(torch.stack((t[:, None] + step, t[:, None] - step), dim=2).reshape((M * S,) + tuple(t.shape[1:])))
        noise.append(eps)
    return kids, noise


def torch_update(torch, mean, sigma, noise, util, S, sigma0, lr, lr_sigma):
    M = mean[0].shape[0]
    ranks = util.view(M, S).to(torch.float32) / (2.0 * (S - 1))
    d, p = ranks[:, 0::2] - ranks[:, 1::2], ranks[:, 0::2] + ranks[:, 1::2]
    out = []
    for t, sg, eps in zip(mean, sigma, noise):
        flat = eps.flatten(2)
        g = torch.einsum("bq,bqe->be", d, flat).view_as(t)
        h = torch.einsum("bq,bqe->be", p, flat * flat - 1.0).view_as(t)
        out.append((t + (lr / (S * sigma0)) * g, sg * torch.exp((lr_sigma / (2.0 * S)) * h)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--groups", default="16,8192")
    a = ap.parse_args()
    import torch
    from gym_rem2d_amd import policy
    from profile_policy import device_policy, each_call_ms
    dev = torch.device("cuda:0")
    n = a.n
    kids = device_policy(n, 16, 32, 10, dev, 2)            # the one child policy: every sample writes it
    set_bytes = kids.weight_bytes()
    words = set_bytes // 4
    lines = ["python tools/profile_snes.py --n %d --reps %d --groups %s" % (n, a.reps, a.groups),
             "%d children of %d B (MB 16, R 10, H 32), sigma 0.1, lr 0.05, lr_sigma 4; device events, median of %d calls after 5 warm-up "
             "calls" % (n, set_bytes, a.reps), ""]
    verdicts = []

    def report(name, fn, draws=0):
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ms = each_call_ms(fn, a.reps)
        peak, after = torch.cuda.max_memory_allocated() - held, torch.cuda.memory_allocated() - held
        med = statistics.median(ms)
        line = "%-44s median %8.4f ms  (min %8.4f  max %8.4f)" % (name, med, min(ms), max(ms))
        if draws:
            line += "  %6.1f G Philox blocks/s" % (draws / (med * 1e-3) / 1e9)
        lines.append(line + "  allocated: peak %+.3f GB, kept %+.3f GB" % (peak / 1e9, after / 1e9))
        return med, peak

    for S in (int(s) for s in a.groups.split(",")):
        if S < 2 or S % 2 or n % S:
            raise SystemExit("--groups: %d is not an even divisor of %d" % (S, n))
        M = n // S
        mean = device_policy(M, 16, 32, 10, dev, 1)
        spare = device_policy(M, 16, 32, 10, dev, 3)
        util = (torch.randperm(n, device=dev).view(M, S).argsort(dim=1).to(torch.int32) * 2 - (S - 1)).reshape(n).contiguous()
        gen = [0]

        def bump():
            gen[0] += 1
            return gen[0]
        draws = (n // 2) * words
        lines.append("S = %d: %d mean(s)" % (S, M))
        # the plain strategy, unchanged code: the yardstick of the cost condition
        need = mean.es_scratch_bytes(S)
        scratch = torch.empty(max(need // 8, 1), dtype=torch.int64, device=dev)
        kw = dict(seed=1, sigma=0.1, group_size=S)
        es_s, pk1 = report("rem2d_es_sample", lambda: mean.es_sample(bump(), out=kids, **kw), draws)
        es_u, pk2 = report("rem2d_es_update (util given)", lambda: mean.es_update(None, bump(), lr=0.05, out=spare, scratch=scratch, util=util, **kw), draws)
        peaks = [pk1, pk2]
        for name, extra in (("plain", {}), ("adam, natural", dict(adam=(0.9, 0.999, 1e-8), natural=True))):
            es = policy.SeparableES(mean, S, sigma=0.1, lr=0.05, lr_sigma=4.0, **extra)
            es.sample(1, seed=1, out=kids)
            es.update(None, 1, seed=1, util=util)              # (the object's scratch is made here)
            es.update(None, 1, seed=1, util=util)
            sn_s, pk3 = report("rem2d_snes_sample (%s)" % name, lambda: es.sample(bump(), seed=1, out=kids), draws)
            sn_u, pk4 = report("rem2d_snes_update (%s; util given)" % name, lambda: es.update(None, bump(), seed=1, util=util), draws)
            peaks += [pk3, pk4]
            for what, new, old in (("sample", sn_s, es_s), ("update", sn_u, es_u)):
                ok = new <= LIMIT * old
                verdicts.append(ok)
                lines.append("    %s (%s): %.2f x rem2d_es_%s -- %s the %.1f x condition" % (what, name, new / old, what, "within" if ok else "OUTSIDE", LIMIT))
            lines.append("    scratch %d B (the ES's: %d B); sigma now %.3g .. %.3g" % (
                es.scratch_bytes(), need, min(float(t.min()) for t in es.sigma), max(float(t.max()) for t in es.sigma)))
            del es
        assert all(p == 0 for p in peaks), "a library call allocated device memory"
        # the comparator
        tm = [mean.w1, mean.b1, mean.w2, mean.b2]
        tsg = [torch.full_like(t, 0.1) for t in tm]
        stored = [None]

        def t_sample():
            stored[0] = None                                 # (the previous call's children and noise are released first)
            stored[0] = torch_sample(torch, tm, tsg, S)
        _, tp1 = report("torch: randn + broadcast children", t_sample)
        _, tp2 = report("torch: two einsums on the stored noise", lambda: torch_update(torch, tm, tsg, stored[0][1], util, S, 0.1, 0.05, 4.0))
        lines.append("torch keeps %.3f GB of noise between its two calls and peaks %.3f GB (sample) / %.3f GB (update) above what was "
                     "held before; the library keeps nothing and allocates nothing" % (n * set_bytes / 2 / 1e9, tp1 / 1e9, tp2 / 1e9))
        lines.append("")
        stored[0] = None
        del mean, spare, scratch, util, tm, tsg
        torch.cuda.empty_cache()
    lines.append("cost condition (each new call within %.1f x of its rem2d_es_* counterpart, both shapes): %s"
                 % (LIMIT, "met" if all(verdicts) else "NOT met"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
