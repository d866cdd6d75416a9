"""The quality figure of DESIGN.md 22, on the host with the numpy models of tests/ alone (no GPU): the line emitter against plain
mutation on a toy whose behaviour is the first two of 16 parameters and whose fitness is minus the squared norm of the other 14.

    python tools/cvt_toy.py [--seeds 10] [--generations 60] [--children 64] [--cells 64]

One block, a centroid archive of --cells centroids over [-1, 1)^2 (elites.cvt_centroids on the CPU), generation 0 = --children
sets drawn from 0.5 N(0, 1); then per generation --children children by cvt_model.line_model (sigma_iso 0.01, sigma_line 0.2, the
defaults of EliteGrid.emit_line) or by elites_model.emit_model (rate 0.05, sigma 0.1, the defaults of EliteGrid.emit), inserted by
cvt_model.insert_model: the same number of evaluations on both sides.  Prints per seed the filled cells and the QD score (the sum
of the fitness over the filled cells; every term is negative, 0 is the best a cell can hold) of both, and the QD score over the
cells both archives fill.  The 16 parameters are the arrays w1 (2 words) and b1 (14 words) of a set; w2 and b2 are one ignored word
each."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ((2,), (14,), (1,), (1,))


def evaluate(kids):
    beh = np.ascontiguousarray(kids[0], np.float32)
    return -(kids[1].astype(np.float64) ** 2).sum(axis=1), beh


def run(seed, generations, children, cen, line):
    import cvt_model as VM
    import elites_model as QM
    rng = np.random.default_rng(seed)
    kids = [(rng.standard_normal((children,) + s) * 0.5).astype(np.float32) for s in SHAPES]
    grid = QM.Grid(1, len(cen), 2, SHAPES)
    for gen in range(generations + 1):
        if gen:
            if line:
                kids = VM.line_model(grid, children, 0.01, 0.2, seed, gen)[0]
            else:
                kids = QM.emit_model(grid, children, QM.rate_threshold(0.05), 0.1, seed, gen)[0]
        fit, beh = evaluate(kids)
        grid = VM.insert_model(cen, grid, kids, fit, beh, children)[0]
    return grid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=10)
    ap.add_argument("--generations", type=int, default=60)
    ap.add_argument("--children", type=int, default=64)
    ap.add_argument("--cells", type=int, default=64)
    a = ap.parse_args()
    from gym_rem2d_amd import elites
    cen = elites.cvt_centroids(a.cells, [-1.0, -1.0], [1.0, 1.0], n_samples=64 * a.cells, iterations=10, seed=0).numpy()
    for seed in range(a.seeds):
        row = {"seed": seed, "evaluations": (a.generations + 1) * a.children}
        grids = {name: run(seed, a.generations, a.children, cen, name == "line") for name in ("line", "mutation")}
        both = (grids["line"].count[0] != 0) & (grids["mutation"].count[0] != 0)
        for name, g in grids.items():
            filled = g.count[0] != 0
            row[name] = {"filled": int(filled.sum()), "qd_score": round(float(g.fitness[0][filled].sum()), 3),
                         "qd_score_on_common_cells": round(float(g.fitness[0][both].sum()), 3)}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
