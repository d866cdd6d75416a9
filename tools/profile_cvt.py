"""Figures of the centroid archive and the line emitter on the device at the workload's own shape: 65 536 rows of 8
descriptor words, 65 536 weight sets of MB 16, R 10, H 32.

    python tools/profile_cvt.py [--out profiles/cvt_figures.json] [--n 65536] [--reps 30]

* assign (rem2d_cvt_assign) of n rows of 8 words to C in {64, 1 024, 16 384} centroids, and of 64 rows to 65 536 (the split),
  against torch.cdist + argmin on the same device, in row chunks where the [rows, C] matrix would pass 1 GiB, with the peak of
  torch.cuda.max_memory_allocated above what was held before.  torch's result has no defined tie or rounding; the share of rows on
  which it names another centroid is reported.
* insert (rem2d_cvt_insert) against rem2d_elites_insert into a grid of the same C, S in {16, 1 024}, in the same process, into a
  full grid whose every incumbent is worse (every cell with a candidate is copied) and one whose every incumbent is better
  (nothing is copied: the assignment's share shows); the difference is the assignment's launch, reported as a multiple.
* emit_line (rem2d_cvt_emit_line) against rem2d_elites_emit(rate = 1.0) of the same n children, same process: the line kernel
  reads one more gathered set per child, 3 x the set bytes per child in all; its time beside those bytes and the share of the HBM
  rate they are (8.0 TB/s by specification, 6.29 TB/s measured for a float4 copy).  And the same operator in torch: two
  index_select, randn, with its peak of temporaries.

Device events around every single call, the median of --reps calls after 5 warm-up calls, state put back before every call outside
the events; the library's calls allocate nothing, which is checked.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from profile_elites import summary, timed  # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12            # bytes per second: the specification, a measured float4 copy


def torch_assign(torch, desc, cen, chunk):
    out = torch.empty(desc.shape[0], dtype=torch.long, device=desc.device)
    for r0 in range(0, desc.shape[0], chunk):
        out[r0:r0 + chunk] = torch.cdist(desc[r0:r0 + chunk], cen).argmin(dim=1)
    return out


def assign_figures(torch, dev, n, reps, gen):
    from gym_rem2d_amd import elites
    out = []
    desc_all = torch.randn((n, 8), generator=gen, device=dev, dtype=torch.float32)
    for rows, C in ((n, 64), (n, 1024), (n, 16384), (64, 65536)):
        desc = desc_all[:rows].contiguous()
        cen = torch.randn((C, 8), generator=gen, device=dev, dtype=torch.float32)
        cell = torch.empty(rows, dtype=torch.int32, device=dev)
        dist = torch.empty(rows, dtype=torch.float32, device=dev)
        scratch = [None]

        def call():
            scratch[0] = elites._assign("assign", desc, cen, cell, dist, scratch[0])[1]
        call()
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ms = timed(torch, call, reps)
        assert torch.cuda.max_memory_allocated() == held, "assign allocated device memory"
        med = statistics.median(ms) * 1e-3
        row = {"rows": rows, "centroids": C, "width": 8,
               "assign": dict(summary(ms), distances_per_s=round(rows * C / med / 1e9, 2) * 1e9, gflops=round(3 * 8 * rows * C / med / 1e9, 1), bytes_allocated_per_call=0)}
        chunk = max(1, min(rows, (1 << 30) // (4 * C)))
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        got = [None]

        def comparator():
            got[0] = torch_assign(torch, desc, cen, chunk)
        ms = timed(torch, comparator, min(reps, 10), warm=2)
        row["torch_cdist_argmin"] = dict(summary(ms), row_chunk=chunk, peak_bytes_above_held=int(torch.cuda.max_memory_allocated() - held),
                                         share_of_rows_with_another_centroid=float((got[0].to(torch.int32) != cell).float().mean()))
        out.append(row)
        print(json.dumps(row), flush=True)
        del desc, cen, cell, dist, got
        torch.cuda.empty_cache()
    return out


def insert_figures(torch, dev, n, reps, gen, pop):
    from gym_rem2d_amd import elites
    out = []
    desc = torch.randn((n, 8), generator=gen, device=dev, dtype=torch.float32)
    fit = torch.randn(n, generator=gen, device=dev, dtype=torch.float64)
    set_bytes = pop.weight_bytes()
    for S in (16, 1024):
        if n % S:
            continue
        for C in (64, 1024, 16384):
            M, side = n // S, int(round(C ** 0.5))
            row = {"sets": n, "S": S, "blocks": M, "cells": C, "set_bytes": set_bytes, "grid_bytes": M * C * (set_bytes + 8 * 4 + 12)}
            free = torch.cuda.mem_get_info(dev)[0]
            if row["grid_bytes"] * 2.5 > free or M * C > 2 ** 31 - 1:
                row["does_not_fit"] = "two grids of %.1f GB, %.1f GB are free" % (row["grid_bytes"] / 1e9, free / 1e9)
                out.append(row)
                print(json.dumps(row), flush=True)
                continue
            cen = torch.randn((C, 8), generator=gen, device=dev, dtype=torch.float32)
            grids = {"cvt_insert": elites.CentroidArchive(M, cen, like=pop, device=dev),
                     "elites_insert": elites.EliteGrid(M, [(6, -2.0, 2.0, side), (7, -2.0, 2.0, side)], 8, like=pop, device=dev)}
            for name, grid in grids.items():
                for kind, level in (("full_worse", -1e30), ("full_better", 1e30)):
                    def prepare():
                        grid.count.fill_(1)
                        grid.fitness.fill_(level)
                    prepare()
                    grid.insert(pop, fit, desc, group_size=S)
                    torch.cuda.synchronize()
                    held = torch.cuda.memory_allocated()
                    torch.cuda.reset_peak_memory_stats()
                    ms = timed(torch, lambda: grid.insert(pop, fit, desc, group_size=S), reps, prepare)
                    assert torch.cuda.max_memory_allocated() == held, "insert allocated device memory"
                    replaced = int((grid.winner >= 0).sum())
                    row["%s_%s" % (name, kind)] = dict(summary(ms), replaced=replaced, bytes_copied=2 * replaced * set_bytes, bytes_allocated_per_call=0)
            for kind in ("full_worse", "full_better"):
                a, b = row["cvt_insert_" + kind]["median_ms"], row["elites_insert_" + kind]["median_ms"]
                row["cvt_over_elites_" + kind] = round(a / b, 3)
                row["assignment_ms_" + kind] = round(a - b, 4)
            out.append(row)
            print(json.dumps(row), flush=True)
            del grids, grid
            torch.cuda.empty_cache()
    return out


def torch_line(torch, grid, per_block, sigma_iso, sigma_line):
    C = grid.n_cells
    filled = (grid.count != 0).to(torch.float32)
    base = torch.arange(grid.n_blocks, device=filled.device)[:, None] * C
    p1 = (torch.multinomial(filled, per_block, replacement=True) + base).view(-1)
    p2 = (torch.multinomial(filled, per_block, replacement=True) + base).view(-1)
    a = sigma_line * torch.randn(p1.shape[0], device=filled.device)
    kids = []
    for t in (grid.w1, grid.b1, grid.w2, grid.b2):
        x1, x2 = t.index_select(0, p1), t.index_select(0, p2)
        kids.append(x1 + sigma_iso * torch.randn_like(x1) + a.view((-1,) + (1,) * (x1.dim() - 1)) * (x2 - x1))
    return kids


def line_figures(torch, dev, n, reps, pop, kids):
    from gym_rem2d_amd import elites
    out = []
    set_bytes = pop.weight_bytes()
    for S, C in ((1024, 64), (1024, 1024), (16, 64)):
        if n % S:
            continue
        M = n // S
        row = {"children": n, "S": S, "blocks": M, "cells": C, "set_bytes": set_bytes, "grid_bytes": M * C * set_bytes}
        free = torch.cuda.mem_get_info(dev)[0]
        if row["grid_bytes"] * 2 > free:
            row["does_not_fit"] = "the grid is %.1f GB, %.1f GB are free" % (row["grid_bytes"] / 1e9, free / 1e9)
            out.append(row)
            continue
        grid = elites.EliteGrid(M, [(0, 0.0, 1.0, C)], 8, like=pop, device=dev)
        grid.count.fill_(1)
        for t in (grid.w1, grid.b1, grid.w2, grid.b2):
            t.normal_()
        g = [1]

        def line():
            g[0] += 1
            grid.emit_line(g[0], seed=3, sigma_iso=0.01, sigma_line=0.2, n_children=n, out=kids)

        def emit():
            g[0] += 1
            grid.emit(g[0], seed=3, rate=1.0, sigma=0.01, n_children=n, out=kids)
        for name, fn, sets_moved in (("emit_line", line, 3), ("elites_emit_rate_1", emit, 2)):
            fn()
            torch.cuda.synchronize()
            held = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            ms = timed(torch, fn, reps)
            assert torch.cuda.max_memory_allocated() == held, name + " allocated device memory"
            moved = sets_moved * n * set_bytes
            rate = moved / (statistics.median(ms) * 1e-3)
            row[name] = dict(summary(ms), bytes_moved=moved, gbytes_per_s=round(rate / 1e9, 1), share_of_hbm_spec=round(rate / HBM_SPEC, 3),
                             share_of_measured_copy_rate=round(rate / HBM_COPY, 3), bytes_allocated_per_call=0)
        row["emit_line_over_emit"] = round(row["emit_line"]["median_ms"] / row["elites_emit_rate_1"]["median_ms"], 3)
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        try:
            ms = timed(torch, lambda: torch_line(torch, grid, S, 0.01, 0.2), min(reps, 10), warm=2)
            row["torch_line"] = dict(summary(ms), peak_bytes_above_held=int(torch.cuda.max_memory_allocated() - held))
        except RuntimeError as err:                  # (out of memory: said, not hidden)
            row["torch_line"] = {"does_not_fit": str(err)[:120]}
        out.append(row)
        print(json.dumps(row), flush=True)
        del grid
        torch.cuda.empty_cache()
    return out


def figures(n, reps):
    import torch
    from profile_policy import device_policy
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    res = {"assign": assign_figures(torch, dev, n, reps, gen)}
    pop = device_policy(n, 16, 32, 10, dev, 2)
    res["insert"] = insert_figures(torch, dev, n, reps, gen, pop)
    kids = device_policy(n, 16, 32, 10, dev, 3)
    res["emit_line"] = line_figures(torch, dev, n, reps, pop, kids)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    res = {"command": "python tools/profile_cvt.py --n %d --reps %d" % (a.n, a.reps), "hbm_bytes_per_s": {"specification": HBM_SPEC, "measured_float4_copy": HBM_COPY}}
    res.update(figures(a.n, a.reps))
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
