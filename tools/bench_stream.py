#!/usr/bin/env python
"""Streamed against whole-population evaluation on one GPU.

Evaluates N L-system individuals (config 3's generator: synthetic.lsystem_batches_native, seeds 0 .. N-1) two ways, same max_steps,
same chunk, both under evaluate.EVAL_FLAGS and timed from the upload to the fitness on the host's side of a synchronisation:

  (a) whole:    env.reset_batches(everything) + evaluate.run_episode(compact=True) -- what evaluate_population does without `slots`;
  (b) streamed: evaluate.run_stream(slots=S) -- reset_stream + step(chunk) / refill() until everybody has finished.

One warm-up run of each, then --runs alternating runs of each; medians.  Reports individuals per second, the peak of
torch.cuda.max_memory_allocated (the arenas, the device morphologies, the feeds, the population-order buffers: everything the
Python layer allocates; the library's own scratch is hipMalloc'ed per world and not in it), the arena bytes of the two layouts
(sum of rem2d_state_bytes over the worlds) and, from one more streamed run with device events around every refill() call, the call's
own device time.  Asserts that the two fitness arrays are equal under ==.

    python tools/bench_stream.py --n 262144 --slots 65536 --out profiles/stream_figures.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--slots", type=int, default=65536)
    ap.add_argument("--max-steps", type=int, default=2500)
    ap.add_argument("--chunk", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--procs", type=int, default=8, help="host processes that draw the genomes (before the GPU is touched)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from gym_rem2d_amd import synthetic
    t0 = time.perf_counter()
    batches = synthetic.lsystem_batches_native(range(args.n), n_proc=args.procs)       # (forks: before torch initialises the GPU)
    t_pop = time.perf_counter() - t0
    import numpy as np
    import torch
    from gym_rem2d_amd import _lib, evaluate
    from gym_rem2d_amd.env import BatchedModular2D
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)             # (the memory statistics need an initialised device)
    buckets = [(m.lanes, m.n_envs) for m, _ in batches]

    def sync():
        torch.cuda.synchronize(dev)

    def arena_bytes(env):
        return sum(int(w.arena.numel()) for w, _ in env.worlds if w.arena is not None)

    def whole():
        env = BatchedModular2D(seed=4, flags=evaluate.EVAL_FLAGS)
        torch.cuda.reset_peak_memory_stats(dev)
        sync()
        t = time.perf_counter()
        env.reset_batches(batches, args.n)
        arenas = arena_bytes(env)
        fit = evaluate.run_episode(env, args.max_steps, args.chunk, on_error="fallback", compact=True).cpu().numpy()
        sync()
        dt = time.perf_counter() - t
        peak = torch.cuda.max_memory_allocated(dev)
        rep = env.last_episode
        env.close()
        return dict(seconds=dt, peak_bytes=peak, arena_bytes=arenas, fallback=len(rep.overflow) + len(rep.handover)), fit

    def streamed(time_refill=False):
        env = BatchedModular2D(seed=4, flags=evaluate.EVAL_FLAGS)
        events, calls = [], [0]
        if time_refill:
            plain = env.refill

            def refill(*a, **kw):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = plain(*a, **kw)
                e1.record()
                events.append((e0, e1))
                return out
            env.refill = refill
        step = env.step

        def counted(n):
            calls[0] += 1
            return step(n)
        env.step = counted
        torch.cuda.reset_peak_memory_stats(dev)
        sync()
        t = time.perf_counter()
        fit = evaluate.run_stream(env, batches, args.n, args.slots, args.max_steps, args.chunk, on_error="fallback").cpu().numpy()
        sync()
        dt = time.perf_counter() - t
        peak = torch.cuda.max_memory_allocated(dev)
        rep = env.last_episode
        out = dict(seconds=dt, peak_bytes=peak, arena_bytes=arena_bytes(env), chunks=calls[0], slots=[w.n_envs for w, _ in env.worlds],
                   fallback=len(rep.overflow) + len(rep.handover))
        if time_refill:
            ms = sorted(a.elapsed_time(b) for a, b in events)
            out["refill_ms"] = dict(calls=len(ms), median=statistics.median(ms), min=ms[0], max=ms[-1], total=sum(ms))
        env.close()
        return out, fit

    runs_a, runs_b = [], []
    _, fit_a = whole()                     # warm-up (first launches, the allocator's first blocks, code objects)
    _, fit_b = streamed()
    assert fit_a.shape == fit_b.shape == (args.n,)
    assert (fit_a == fit_b).all(), "streamed and whole-population fitness differ at ids %s" % np.flatnonzero(fit_a != fit_b)[:8]
    for _ in range(args.runs):
        ra, fa = whole()
        rb, fb = streamed()
        assert (fa == fit_a).all() and (fb == fit_a).all()
        runs_a.append(ra)
        runs_b.append(rb)
    timed, ft = streamed(time_refill=True)
    assert (ft == fit_a).all()

    def summary(runs):
        sec = [r["seconds"] for r in runs]
        med = statistics.median(sec)
        return dict(seconds_median=med, seconds_all=sec, individuals_per_second=args.n / med,
                    peak_bytes=max(r["peak_bytes"] for r in runs), arena_bytes=runs[0]["arena_bytes"], runs=runs)
    a, b = summary(runs_a), summary(runs_b)
    result = dict(n=args.n, slots=args.slots, max_steps=args.max_steps, chunk=args.chunk, runs=args.runs, buckets=buckets,
                  population_seconds=t_pop, device=torch.cuda.get_device_name(dev), build_id=_lib.build_id(),
                  fitness_equal=True, fitness_nonzero=int((fit_a != 0).sum()),
                  whole=a, streamed=b, refill=timed["refill_ms"], streamed_chunks=timed["chunks"],
                  speed_ratio_streamed_over_whole=b["individuals_per_second"] / a["individuals_per_second"],
                  peak_ratio_whole_over_streamed=a["peak_bytes"] / b["peak_bytes"],
                  arena_ratio_whole_over_streamed=a["arena_bytes"] / b["arena_bytes"])
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
