"""Figures of evolving device policies at the workload's own shape: 65 536 weight sets, MB 16, R 10, H 32, rate 0.05.

    python tools/profile_evolve.py [--out profiles/policy_evolve.txt] [--n 65536] [--reps 30] [--group 16]

* select, vary (mutating: rate 0.05; copy path: rate 0) and evolve of the library: device events around every single call, median
  of --reps calls after 5 warm-up calls, into buffers made once (out=: the call allocates nothing, which is checked).  Bytes are
  computed from the shapes -- every parent word read once, every child word written once, fitness and parents -- and reported as a
  share of 6.3 TB/s; they are no counters.
* the comparator: the same operator stated in torch on the same device (tournament of 4 by randint / gather / argmax, then per array
  index_select, randn_like, rand_like, where, add), timed the same way, with the peak of torch.cuda.max_memory_allocated above what
  was allocated before the call.  It draws from torch's generator: another stream, the same distributions.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PEAK_BYTES_PER_S = 6.3e12


def torch_evolve(torch, p, fit, rate, sigma, group):
    G = p.n_sets
    base = (torch.arange(G, device=fit.device) // group) * group
    asp = base[:, None] + torch.randint(0, group, (G, 4), device=fit.device)
    win = asp.gather(1, fit[asp].argmax(1, keepdim=True)).squeeze(1)
    kids = []
    for t in (p.w1, p.b1, p.w2, p.b2):
        k = t.index_select(0, win)
        kids.append(torch.where(torch.rand_like(k) < rate, k + sigma * torch.randn_like(k), k))
    return kids, win


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--group", type=int, default=16)
    a = ap.parse_args()
    import torch
    from gym_rem2d_amd import policy
    from profile_policy import device_policy, each_call_ms
    dev = torch.device("cuda:0")
    n, S = a.n, a.group
    p = device_policy(n, 16, 32, 10, dev, 1)
    out = device_policy(n, 16, 32, 10, dev, 2)
    out.parents = torch.zeros(n, dtype=torch.int32, device=dev)
    fit = torch.randn(n, dtype=torch.float64, device=dev)
    set_bytes = p.weight_bytes()
    lines = ["python tools/profile_evolve.py --n %d --reps %d --group %d" % (n, a.reps, S),
             "%d weight sets of %d B (MB 16, R 10, H 32), blocks of %d, tournaments of 4, elite 1, sigma 0.1; device events, median of %d "
             "calls after 5 warm-up calls" % (n, set_bytes, S, a.reps), ""]

    def report(name, fn, moved):
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ms = each_call_ms(fn, a.reps)
        peak, after = torch.cuda.max_memory_allocated() - held, torch.cuda.memory_allocated() - held
        med = statistics.median(ms)
        lines.append("%-34s median %8.4f ms  (min %8.4f  max %8.4f)  %7.3f GB from the shapes  %7.1f GB/s = %5.1f %% of 6.3 TB/s  "
                     "allocated: peak %+.3f GB, kept %+.3f GB" % (name, med, min(ms), max(ms), moved / 1e9, moved / (med * 1e-3) / 1e9,
                                                                 100.0 * moved / (med * 1e-3) / PEAK_BYTES_PER_S, peak / 1e9, after / 1e9))
        return med, peak

    kw = dict(seed=1, sigma=0.1, tournsize=4, group_size=S, elite=1)
    weights = 2 * n * set_bytes                              # parents read, children written
    sel_bytes = n * 4 + n * 4 * 8                            # parents written; up to four fitness values gathered per child
    gen = [0]

    def call(rate, parents=None):
        gen[0] += 1
        return p.evolve(fit, gen[0], rate=rate, parents=parents, out=out, **kw)
    mine = torch.randint(0, n, (n,), dtype=torch.int32, device=dev)
    # selection alone has no Python entry of its own: the library call, through the binding
    import ctypes as C
    from gym_rem2d_amd import _lib
    e = _lib.Evolve()
    e.d, e.hidden, e.max_bodies, e.n_sets, e.group_size, e.tournsize, e.elite = p.d, p.hidden, p.max_bodies, n, S, 4, 1
    e.generation, e.rate_threshold, e.seed, e.sigma = 1, 0, 1, 0.1
    e.fitness, e.parent = fit.data_ptr(), out.parents.data_ptr()
    L = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    report("select", lambda: _lib.check(L.rem2d_policy_select(C.byref(e), stream)), sel_bytes)
    v_mut, pk1 = report("vary, rate 0.05 (mutating)", lambda: call(0.05, mine), weights + 4 * n)
    v_copy, pk2 = report("vary, rate 0 (copy path)", lambda: call(0.0, mine), weights + 4 * n)
    v_all, _ = report("vary, rate 1 (every element hit)", lambda: call(1.0, mine), weights + 4 * n)
    out.parents = torch.zeros(n, dtype=torch.int32, device=dev)     # (not `mine`: evolve writes out's parents)
    ev, pk3 = report("evolve, rate 0.05", lambda: call(0.05), weights + sel_bytes)
    assert pk1 == pk2 == pk3 == 0, "the fused call allocated device memory"
    lines.append("the random stream costs %.4f ms of the mutating pass (%.1f x the copy path)" % (v_mut - v_copy, v_mut / v_copy))
    lines.append("")
    t_ms, t_peak = report("torch: the same operator", lambda: torch_evolve(torch, p, fit, 0.05, 0.1, S), weights + sel_bytes)
    lines.append("evolve is %.2f x the torch statement's speed and allocates nothing; torch's peak above the two weight buffers' worth "
                 "held before the call: %.3f GB" % (t_ms / ev, t_peak / 1e9))
    # a sanity figure: the share of elements the mutating pass changed
    child = call(0.05, torch.arange(n, dtype=torch.int32, device=dev))
    changed = float((child.w1 != p.w1).float().mean())
    lines.append("share of w1 changed at rate 0.05 with every child its own parent's copy: %.5f (one block's first child is an elite copy)" % changed)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
