"""Replay an elite of a reference run as PNG frames -- the reference's ``load_best`` (REM2D_main.py:162-167) on this path.

    python tools/render_elite.py results/s_elite20 --out frames/ [--interval 5] [--index K] [--width 800 --height 600]

Reads an ``s_elite<i>`` (one Individual) or ``s_pop<i>`` (a population: the fittest one, or --index) pickle written by the
reference or by ea.run_ea(save_dir=...) through gym_rem2d_amd.compat, evaluates it again in a 1-creature env on the GPU and writes
``frame<step>.png`` every --interval steps under the reference's scrolling camera.  Prints the fitness.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("pickle", help="s_elite<i> or s_pop<i> of a reference run")
    ap.add_argument("--out", required=True, help="directory for the PNG frames")
    ap.add_argument("--interval", type=int, default=5, help="env-steps between two frames (the reference's INTERVAL)")
    ap.add_argument("--index", type=int, default=None, help="individual of an s_pop file (default: the fittest)")
    ap.add_argument("--depth", type=int, default=None, help="tree depth (default: the individual's own)")
    ap.add_argument("--max-steps", type=int, default=None, help="episode cap (default: evaluate.EPISODE_CAP)")
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=600)
    a = ap.parse_args(argv)
    from gym_rem2d_amd.compat import load_reference_pickle
    from gym_rem2d_amd.ea import show_best_episode
    obj = load_reference_pickle(a.pickle)
    if isinstance(obj, (list, tuple)):
        ind = obj[a.index] if a.index is not None else max(obj, key=lambda i: i.fitness)
    else:
        ind = obj
    fit, n = show_best_episode(ind, a.depth, interval=a.interval, frames_dir=a.out, max_steps=a.max_steps, width=a.width,
                               height=a.height)
    print("fitness %r (stored %r): %d frames in %s" % (fit, getattr(ind, "fitness", None), n, a.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
