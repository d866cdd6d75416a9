"""A quality figure for DESIGN.md 23, on the host with the numpy models of tests/ alone (no GPU): the plain evolution strategy of
include/rem2d_es.h on a toy whose target depends on a SMALL-variance input that sits next to an input with a LARGE offset, with and
without the observation normaliser.

    python tools/obsnorm_toy.py [--seeds 10] [--generations 40] [--children 32] [--rows 64]

One mean, the smallest policy there is (max_bodies 1, no rays: 14 input words, --hidden units, one output).  An input row: word 0 =
50 + 0.5 u (a root that has walked 50 m), word 1 = 0.02 s with s uniform in [-1, 1) (a joint angle of a few hundredths of a
radian), the other words 0.  The target of a row is scale * softsign(2 s): what the output should be.  The fitness of a child is
minus its mean squared error over --rows rows that are drawn anew every generation, the same rows for every child.  Per generation:
es_model.sample_model, the fitness, es_model.shape_model and update_model -- sigma 0.1, lr 0.05, the defaults of
run_policy_es -- from w1 of std 0.3 as MLPPolicy.random draws it.  With the normaliser the generation starts with
obsnorm_model.freeze (min_count 2) and the children see obsnorm_model.apply of the rows (clip 5), whose sums then take the
generation's rows, as run_policy_es(normalizer=) does it.  Prints per seed the mean's error on 1 024 fresh rows after the last
generation, raw and normalised; it reports what comes out, no result is promised."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

f32 = np.float32
MB, DN = 1, 14


def rows_of(rng, n):
    x = np.zeros((n, DN), f32)
    s = rng.uniform(-1.0, 1.0, n)
    x[:, 0] = 50.0 + 0.5 * rng.standard_normal(n)
    x[:, 1] = 0.02 * s
    return x, s


def error(PM, W, x, s):
    """mean squared error of every set of W on the rows x: [sets]"""
    want = float(PM.DEFAULT_SCALE) * (2.0 * s) / (1.0 + np.abs(2.0 * s))
    out = []
    for g in range(W[0].shape[0]):
        t, _ = PM.forward_model(x, *(np.repeat(a[g:g + 1], len(x), axis=0) for a in W))
        out.append(float(np.mean((t[:, 0] - want) ** 2)))
    return np.array(out)


def run(seed, generations, children, n_rows, hidden, normalise):
    import es_model as ES
    import obsnorm_model as OM
    import policy_model as PM
    rng = np.random.default_rng(seed)
    mean = [(rng.standard_normal(sh) * sd).astype(f32) for sh, sd in (((1, DN, hidden), 0.3), ((1, hidden), 0.3), ((1, hidden, MB), 0.5), ((1, MB), 0.3))]
    state = OM.State(1, DN)
    see = lambda x: x
    for gen in range(1, generations + 1):
        if normalise:
            mu, inv = OM.freeze(*state.words(), 2, 2.0 ** -20)
            see = lambda x, mu=mu, inv=inv: OM.apply(x, mu, inv, 5.0, len(x))
        x, s = rows_of(rng, n_rows)
        kids = ES.sample_model(mean, children, 0.1, seed, gen)
        fit = -error(PM, kids, see(x), s)
        if normalise:
            OM.accumulate(state, x, len(x))
        util = ES.shape_model(fit, children)
        mean = ES.update_model(mean, util, children, ES.step_for(0.05, children, 0.1), seed, gen)
    x, s = rows_of(np.random.default_rng([seed, 1]), 1024)
    return float(error(PM, mean, see(x), s)[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=10)
    ap.add_argument("--generations", type=int, default=40)
    ap.add_argument("--children", type=int, default=32)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=4)
    a = ap.parse_args()
    out = []
    for seed in range(a.seeds):
        row = {"seed": seed, "evaluations": a.generations * a.children}
        for name in ("raw", "normalised"):
            row[name + "_mse"] = run(seed, a.generations, a.children, a.rows, a.hidden, name == "normalised")
        out.append(row)
        print(json.dumps(row))
    raw, nrm = np.array([r["raw_mse"] for r in out]), np.array([r["normalised_mse"] for r in out])
    print(json.dumps({"seeds": a.seeds, "raw_mse_median": float(np.median(raw)), "normalised_mse_median": float(np.median(nrm)),
                      "normalised_better_in": int((nrm < raw).sum())}))


if __name__ == "__main__":
    main()
