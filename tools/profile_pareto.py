"""Figures of the Pareto ranking on the device at the workload's own shape: 65 536 rows.

    python tools/profile_pareto.py [--out profiles/pareto_figures.json] [--n 65536] [--reps 30]

* rank (rem2d_pareto_rank) at K in {2, 4}, S in {16, 64, 1 024}, on standard normal objectives and on a chain (S fronts: the
  deepest peel): device events around every single call, median of --reps calls after 5 warm-up calls, into buffers made once (the
  calls allocate nothing, which is checked).
* local competition (rem2d_pareto_local) at B = 8, k = 15 and the same S, timed the same way.
* the same two operators written straightforwardly in torch on the same device -- the domination matrix of every block, the peel
  as a loop of masked reductions, the crowding and the order as [M, S, S] comparisons; cdist, topk and a gather -- timed the same
  way, with the peak of torch.cuda.max_memory_allocated above what was held before.  They are no bit-exact restatement (cdist
  fuses as it likes, topk breaks ties as it likes); they show what the operator costs without the kernels.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def torch_rank(torch, obj, S):
    """(front, crowd, util) of finite objectives [G, K] in blocks of S"""
    G, K = obj.shape
    M = G // S
    x = obj.view(M, S, K)
    ge = (x[:, :, None, :] >= x[:, None, :, :]).all(dim=3)
    gt = (x[:, :, None, :] > x[:, None, :, :]).any(dim=3)
    dom = ge & gt                                           # [b, i, j]: i dominates j
    waiting = dom.sum(dim=1)
    left = torch.ones((M, S), dtype=torch.bool, device=obj.device)
    front = torch.zeros((M, S), dtype=torch.int32, device=obj.device)
    r = 0
    while bool(left.any()):
        free = left & (waiting == 0)
        front[free] = r
        left &= ~free
        waiting = waiting - (dom & free[:, :, None]).sum(dim=1)
        r += 1
    same = front[:, :, None] == front[:, None, :]
    inf = float("inf")
    crowd = torch.zeros((M, S), dtype=torch.float64, device=obj.device)
    open_ = torch.zeros((M, S), dtype=torch.bool, device=obj.device)
    for m in range(K):
        v = x[:, :, m]
        vj = v[:, None, :].expand(M, S, S)
        lt, gtm = same & (vj < v[:, :, None]), same & (vj > v[:, :, None])
        below = torch.where(lt, vj, -inf).amax(dim=2)
        above = torch.where(gtm, vj, inf).amin(dim=2)
        lo = torch.where(same, vj, inf).amin(dim=2)
        hi = torch.where(same, vj, -inf).amax(dim=2)
        open_ |= ~lt.any(dim=2) | ~gtm.any(dim=2)
        crowd = crowd + (above - below) / (hi - lo)
    crowd = torch.where(open_, inf, crowd)
    better = (front[:, :, None] < front[:, None, :]) | (same & (crowd[:, :, None] > crowd[:, None, :]))
    L, W = better.sum(dim=2), better.sum(dim=1)
    util = (2 * L + (S - 1 - L - W) - (S - 1)).to(torch.int32)
    return front.view(-1), crowd.view(-1), util.view(-1)


def torch_local(torch, desc, fitness, S, k):
    """[G] float64: how many of the k nearest other rows of the block have a lower fitness"""
    M = desc.shape[0] // S
    x, f = desc.view(M, S, -1), fitness.view(M, S)
    d = torch.cdist(x, x)
    d.diagonal(dim1=1, dim2=2).fill_(float("inf"))
    kk = min(k, S - 1)
    if kk == 0:
        return torch.zeros_like(fitness)
    idx = d.topk(kk, dim=2, largest=False).indices
    near = torch.gather(f[:, None, :].expand(M, S, S), 2, idx)
    return (near < f[:, :, None]).sum(dim=2).to(torch.float64).view(-1)


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "calls": len(ms)}


def beside(torch, row, name, ours, theirs, reps):
    """time `ours` (which must allocate nothing) and `theirs` (with its peak memory) into row[name]"""
    from profile_policy import each_call_ms
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = each_call_ms(ours, reps)
    assert torch.cuda.max_memory_allocated() == held, "%s allocated device memory" % name
    row[name] = summary(ms)
    torch.cuda.reset_peak_memory_stats()
    try:
        tms = each_call_ms(theirs, reps, warm=2)
        row["torch"] = dict(summary(tms), peak_bytes_above_held=int(torch.cuda.max_memory_allocated() - held))
        row["torch_over_kernel"] = round(row["torch"]["median_ms"] / row[name]["median_ms"], 2)
    except RuntimeError as err:                              # (out of memory: said, not hidden)
        row["torch"] = {"does_not_fit": str(err)[:120]}
    torch.cuda.empty_cache()


def figures(n, reps):
    import torch
    from gym_rem2d_amd import pareto
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    res = {"rank": [], "local": []}
    for K in (2, 4):
        for S in (16, 64, 1024):
            if n % S:
                continue
            M = n // S
            chain = torch.stack([torch.randperm(S, generator=gen, device=dev) for _ in range(min(M, 64))]).repeat(-(-M // 64), 1)[:M]
            for content, obj in (("normal", torch.randn((n, K), generator=gen, device=dev, dtype=torch.float64)),
                                 ("chain", chain.reshape(-1, 1).to(torch.float64).repeat(1, K).contiguous())):
                out = pareto.rank(obj, group_size=S)
                row = {"K": K, "S": S, "blocks": M, "rows": n, "content": content, "fronts_max": int(out.n_fronts.max())}
                beside(torch, row, "rank", lambda: pareto.rank(obj, group_size=S, out=out), lambda: torch_rank(torch, obj, S), reps)
                res["rank"].append(row)
                print(json.dumps(row), flush=True)
    B, k = 8, 15
    desc = torch.randn((n, B), generator=gen, device=dev, dtype=torch.float32)
    fit = torch.randn(n, generator=gen, device=dev, dtype=torch.float64)
    loc = torch.zeros(n, dtype=torch.float64, device=dev)
    for S in (16, 64, 1024):
        if n % S:
            continue
        row = {"B": B, "k": k, "S": S, "blocks": n // S, "rows": n, "distances": n * (S - 1)}
        beside(torch, row, "local", lambda: pareto.local_competition(desc, fit, k=k, group_size=S, out=loc),
               lambda: torch_local(torch, desc, fit, S, k), reps)
        row["g_distances_per_s"] = round(row["distances"] / (row["local"]["median_ms"] * 1e-3) / 1e9, 2)
        res["local"].append(row)
        print(json.dumps(row), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    res = dict({"command": "python tools/profile_pareto.py --n %d --reps %d" % (a.n, a.reps)}, **figures(a.n, a.reps))
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
