"""Figures of the evolution strategy for device policies at the workload's own shape: 65 536 children, MB 16, R 10,
H 32, in blocks of 16 (4 096 means) and as one block of 65 536 (one mean).

    python tools/profile_es.py [--out profiles/policy_es.txt] [--n 65536] [--reps 30] [--groups 16,65536]

* sample, shape, update (the library's own pair_chunk) and es_step of the library: device events around every single call, median
  of --reps calls after 5 warm-up calls, into buffers made once (out=, scratch=: the calls allocate nothing, which is checked).
  Bytes are computed from the shapes -- sample: the mean read once, every child word written once; update: the mean read and
  written once, util read, the scratch written and read once -- and, for sample, reported as a share of 6.3 TB/s; they are no
  counters.  The update's work is its draws: pairs x words of a set Philox blocks, reported as blocks per second.
* sample in its other form, a wavefront and a Philox block per CHILD: rem2d_policy_vary with every element hit and
  every child's parent its block's first set moves the same child bytes with twice the integer work.
* the comparator: the same strategy stated in torch on the same device -- randn noise the size of half the population, children
  by broadcast, ranks by a double argsort, the update an einsum over the STORED noise -- timed the same way, with the peak of
  torch.cuda.max_memory_allocated above what was allocated before the call.  It draws from torch's generator (another stream,
  the same distribution up to the tails) and its float sum is not reproducible.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PEAK_BYTES_PER_S = 6.3e12


def torch_sample(torch, mean, S, sigma):
    """-> (children per array, the stored noise per array)"""
    kids, noise = [], []
    for t in (mean.w1, mean.b1, mean.w2, mean.b2):
        M = t.shape[0]
        eps = torch.randn((M, S // 2) + tuple(t.shape[1:]), device=t.device, dtype=torch.float32)
        pair = torch.stack((t[:, None] + sigma * eps, t[:, None] - sigma * eps), dim=2)
        kids.append(pair.reshape((M * S,) + tuple(t.shape[1:])))
        noise.append(eps)
    return kids, noise


def torch_update(torch, mean, noise, fit, S, sigma, lr):
    M = mean.n_sets
    ranks = fit.view(M, S).argsort(dim=1).argsort(dim=1).to(torch.float32) / (S - 1) - 0.5
    d = ranks[:, 0::2] - ranks[:, 1::2]
    out = []
    for t, eps in zip((mean.w1, mean.b1, mean.w2, mean.b2), noise):
        g = torch.einsum("bq,bqe->be", d, eps.flatten(2)).view_as(t)
        out.append(t + (lr / (S * sigma)) * g)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--groups", default="16,65536")
    a = ap.parse_args()
    import torch
    from gym_rem2d_amd import policy
    from profile_policy import device_policy, each_call_ms
    dev = torch.device("cuda:0")
    n = a.n
    kids = device_policy(n, 16, 32, 10, dev, 2)            # the one child policy: every sample writes it
    set_bytes = kids.weight_bytes()
    words = set_bytes // 4
    fit = torch.randn(n, dtype=torch.float64, device=dev)
    lines = ["python tools/profile_es.py --n %d --reps %d --groups %s" % (n, a.reps, a.groups),
             "%d children of %d B (MB 16, R 10, H 32), sigma 0.1, lr 0.05; device events, median of %d calls after 5 warm-up calls"
             % (n, set_bytes, a.reps), ""]

    def report(name, fn, moved, draws=0):
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ms = each_call_ms(fn, a.reps)
        peak, after = torch.cuda.max_memory_allocated() - held, torch.cuda.memory_allocated() - held
        med = statistics.median(ms)
        line = "%-40s median %8.4f ms  (min %8.4f  max %8.4f)  %7.4f GB from the shapes  %7.1f GB/s = %5.1f %% of 6.3 TB/s" % (
            name, med, min(ms), max(ms), moved / 1e9, moved / (med * 1e-3) / 1e9, 100.0 * moved / (med * 1e-3) / PEAK_BYTES_PER_S)
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
        spare.util = torch.zeros(n, dtype=torch.int32, device=dev)
        need = mean.es_scratch_bytes(S)
        scratch = torch.empty(max(need // 8, 1), dtype=torch.int64, device=dev)
        kw = dict(seed=1, sigma=0.1, group_size=S)
        gen = [0]

        def sample():
            gen[0] += 1
            return mean.es_sample(gen[0], out=kids, **kw)

        def update(util=None):
            gen[0] += 1
            return mean.es_update(fit, gen[0], lr=0.05, out=spare, scratch=scratch, util=util, **kw)
        lines.append("S = %d: %d mean(s); the update's scratch: %d B (%d chunks of pairs per block)"
                     % (S, M, need, need // (8 * words * M) if need else 1))
        draws = (n // 2) * words
        _, pk1 = report("sample", sample, n * set_bytes + M * set_bytes, draws)
        # the other form: one wavefront and one Philox block per child (the vary kernel, every element hit)
        parents = device_policy(n, 16, 32, 10, dev, 4) if S == int(a.groups.split(",")[0]) else None
        if parents is not None:
            first = ((torch.arange(n, device=dev) // S) * S).to(torch.int32)
            report("sample's other form: vary, a draw per child", lambda: parents.evolve(fit, 1, rate=1.0, sigma=0.1, group_size=S,
                                                                                          parents=first, out=kids), n * set_bytes + M * set_bytes, n * words)
            del parents
            torch.cuda.empty_cache()
        # shape alone has no Python entry of its own: the library call, through the binding
        import ctypes as C
        from gym_rem2d_amd import _lib
        e = mean._es_descriptor("profile", 1, 1, S)
        e.fitness, e.util = fit.data_ptr(), spare.util.data_ptr()
        L = _lib.lib()
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        report("shape", lambda: _lib.check(L.rem2d_es_shape(C.byref(e), stream)), n * 12)
        util = spare.util.clone()
        upd_bytes = 2 * M * set_bytes + n * 4 + 2 * need
        _, pk2 = report("update (util given)", lambda: update(util), upd_bytes, draws)
        spare.util = torch.zeros(n, dtype=torch.int32, device=dev)
        st, pk3 = report("es_step (shape + update)", update, upd_bytes + n * 12, draws)
        assert pk1 == pk2 == pk3 == 0, "a library call allocated device memory"
        # the comparator
        stored = [None]

        def t_sample():
            stored[0] = None                                 # (the previous call's children and noise are released first)
            stored[0] = torch_sample(torch, mean, S, 0.1)
        ts, tp1 = report("torch: randn + broadcast children", t_sample, n * set_bytes + M * set_bytes)
        tu, tp2 = report("torch: argsort ranks + einsum on noise", lambda: torch_update(torch, mean, stored[0][1], fit, S, 0.1, 0.05),
                         n * set_bytes // 2 + 2 * M * set_bytes)
        lines.append("torch keeps %.3f GB of noise between its two calls and peaks %.3f GB (sample) / %.3f GB (update) above what was "
                     "held before; the library keeps nothing and allocates nothing" % (n * set_bytes / 2 / 1e9, tp1 / 1e9, tp2 / 1e9))
        lines.append("")
        stored[0] = None
        del mean, spare, scratch, util
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
