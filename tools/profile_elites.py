"""Figures of MAP-Elites on the device at the workload's own shape: 65 536 weight sets of MB 16, R 10, H 32.

    python tools/profile_elites.py [--out profiles/elites_figures.json] [--n 65536] [--reps 30]

* insert (rem2d_elites_insert) into an empty grid and into a full grid whose every incumbent is worse, and emit
  (rem2d_elites_emit, rate 0.05) of n children, for S in {16, 1 024, 65 536} x C in {64, 1 024} (an 8 x 8 / a 32 x 32 grid over two
  of 8 descriptor words) where grid and comparator fit in memory: device events around every single call, median of --reps calls
  after 5 warm-up calls, the grid put back before every call outside the events; the calls allocate nothing, which is checked.
* the same operators in torch on the same device: scatter_reduce amax, the lowest row among those that have it by scatter_reduce
  amin, index_copy of the winners; multinomial over the filled cells, index_select and the mutation of DESIGN.md 15's comparator --
  timed the same way, with the peak of torch.cuda.max_memory_allocated above what was held before.  It is not reproducible.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "calls": len(ms)}


def timed(torch, fn, reps, prepare=None, warm=5):
    """device ms of every one of reps calls of fn(), prepare() before each outside the events"""
    pairs = []
    for i in range(warm + reps):
        if prepare:
            prepare()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        if i >= warm:
            pairs.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in pairs]


def torch_insert(torch, grid, pop, fit, desc, S):
    G, C = fit.shape[0], grid.n_cells
    cell = torch.zeros(G, dtype=torch.long, device=fit.device)
    stride = 1
    for w, b, lo, inv in zip(grid.word, grid.bins, grid.lo, grid.inv):
        cell += ((desc[:, w] - lo) * inv).floor().clamp_(0, b - 1).to(torch.long) * stride
        stride *= b
    rows = torch.arange(G, device=fit.device)
    slot = (rows // S) * C + cell
    slots = grid.n_blocks * C
    best = torch.full((slots,), float("-inf"), dtype=torch.float64, device=fit.device).scatter_reduce(0, slot, fit, "amax")
    cand = torch.where(fit == best[slot], rows, torch.full_like(rows, G))
    win = torch.full((slots,), G, dtype=torch.long, device=fit.device).scatter_reduce(0, slot, cand, "amin")
    take = (win < G) & ((grid.count.view(-1) == 0) | (best > grid.fitness.view(-1)))
    to = torch.nonzero(take).flatten()
    src = win[to]
    grid.fitness.view(-1).index_copy_(0, to, fit[src])
    grid.desc.view(slots, -1).index_copy_(0, to, desc[src])
    grid.count.view(-1).index_add_(0, to, torch.ones_like(to, dtype=torch.int32))
    for mine, theirs in zip((grid.w1, grid.b1, grid.w2, grid.b2), (pop.w1, pop.b1, pop.w2, pop.b2)):
        mine.index_copy_(0, to, theirs.index_select(0, src))
    return win


def torch_emit(torch, grid, per_block, rate, sigma):
    C = grid.n_cells
    pick = torch.multinomial((grid.count != 0).to(torch.float32), per_block, replacement=True)
    parent = (pick + torch.arange(grid.n_blocks, device=pick.device)[:, None] * C).view(-1)
    kids = []
    for t in (grid.w1, grid.b1, grid.w2, grid.b2):
        k = t.index_select(0, parent)
        kids.append(torch.where(torch.rand_like(k) < rate, k + sigma * torch.randn_like(k), k))
    return kids, parent


def figures(n, reps):
    import torch
    from gym_rem2d_amd import elites
    from profile_policy import device_policy
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    pop = device_policy(n, 16, 32, 10, dev, 2)
    kids = device_policy(n, 16, 32, 10, dev, 3)
    desc = torch.randn((n, 8), generator=gen, device=dev, dtype=torch.float32)
    fit = torch.randn(n, generator=gen, device=dev, dtype=torch.float64)
    set_bytes = pop.weight_bytes()
    out = []
    for S in (16, 1024, 65536):
        if n % S:
            continue
        for C in (64, 1024):
            side = int(round(C ** 0.5))
            M = n // S
            row = {"sets": n, "S": S, "blocks": M, "cells": C, "set_bytes": set_bytes, "grid_bytes": M * C * (set_bytes + 8 * 4 + 12)}
            free = torch.cuda.mem_get_info(dev)[0]
            if row["grid_bytes"] * 3 > free:
                row["does_not_fit"] = "the grid is %.1f GB, %.1f GB are free" % (row["grid_bytes"] / 1e9, free / 1e9)
                out.append(row)
                print(json.dumps(row), flush=True)
                continue
            grid = elites.EliteGrid(M, [(6, -2.0, 2.0, side), (7, -2.0, 2.0, side)], 8, like=pop, device=dev)

            def empty():
                grid.count.zero_()

            def full():
                grid.count.fill_(1)
                grid.fitness.fill_(-1e30)
            for name, prepare in (("insert_empty", empty), ("insert_full", full)):
                prepare()
                grid.insert(pop, fit, desc, group_size=S)           # (cell is allocated here, once)
                torch.cuda.synchronize()
                held = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                ms = timed(torch, lambda: grid.insert(pop, fit, desc, group_size=S), reps, prepare)
                assert torch.cuda.max_memory_allocated() == held, "insert allocated device memory"
                replaced = int((grid.winner >= 0).sum())
                row[name] = dict(summary(ms), replaced=replaced, bytes_copied=2 * replaced * set_bytes, bytes_allocated_per_call=0)
            grid.emit(1, n_children=n, out=kids)
            torch.cuda.synchronize()
            held = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            g = [1]

            def emit():
                g[0] += 1
                grid.emit(g[0], seed=3, rate=0.05, sigma=0.1, n_children=n, out=kids)
            ms = timed(torch, emit, reps)
            assert torch.cuda.max_memory_allocated() == held, "emit allocated device memory"
            row["emit"] = dict(summary(ms), filled=int(grid.n_filled.sum()), bytes_moved=2 * n * set_bytes,
                               gbytes_per_s=round(2 * n * set_bytes / (statistics.median(ms) * 1e-3) / 1e9, 1), bytes_allocated_per_call=0)
            for name, prepare in (("torch_insert_empty", empty), ("torch_insert_full", full)):
                torch.cuda.synchronize()
                held = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                try:
                    ms = timed(torch, lambda: torch_insert(torch, grid, pop, fit, desc, S), min(reps, 10), prepare, warm=2)
                    row[name] = dict(summary(ms), peak_bytes_above_held=int(torch.cuda.max_memory_allocated() - held))
                except RuntimeError as err:          # (out of memory: said, not hidden)
                    row[name] = {"does_not_fit": str(err)[:120]}
            torch.cuda.synchronize()
            held = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            try:
                ms = timed(torch, lambda: torch_emit(torch, grid, S, 0.05, 0.1), min(reps, 10), warm=2)
                row["torch_emit"] = dict(summary(ms), peak_bytes_above_held=int(torch.cuda.max_memory_allocated() - held))
            except RuntimeError as err:
                row["torch_emit"] = {"does_not_fit": str(err)[:120]}
            out.append(row)
            print(json.dumps(row), flush=True)
            del grid
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    res = {"command": "python tools/profile_elites.py --n %d --reps %d" % (a.n, a.reps), "shapes": figures(a.n, a.reps)}
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
