"""Streaming evaluation stated on the oracle alone (include/rem2d_stream.h), shared by tests/test_stream_host.py and
tests/test_stream_gpu.py: what episode_model.py is for reset_where.

A streamed evaluation gives every creature of a population one episode: from reset, in chunks of ``chunk`` steps, until a chunk
boundary finds it frozen (evaluate()'s loop has ended) or at ``max_steps`` steps.  Creatures are independent, so WHEN a creature
gets its slot does not matter, and the model needs no slots: one ``oracle.World`` per creature (episode_model.EpisodeModel, which
is control_model.OracleLoop per lane bucket plus the capacity notes), all started together, judged at every chunk boundary.

``run`` -> per lane bucket: ``fitness`` float64 [N], ``steps`` int32 [N] (the step count at the boundary that ended it), ``how``
[N] of "frozen" / "steps", plus ``over`` (episode_model's over_capacity) and the buckets' ``ctxs``."""
import numpy as np

import episode_model as EM

CONT = 1
MAX_STEPS, CHUNK = 125, 25     # the runs of the stream tests: five chunks, half the population frozen before the limit

_RUNS = {}


def run(O, pop, max_steps=MAX_STEPS, chunk=CHUNK, flags=CONT):
    key = (pop, max_steps, chunk, flags)
    if key in _RUNS:
        return _RUNS[key]
    assert max_steps % chunk == 0
    model = EM.EpisodeModel(O, pop, flags)
    n = model.n
    out = dict(ctxs=[loop.ctx for loop in model.loops], fitness=[np.zeros(k, np.float64) for k in n],
               steps=[np.zeros(k, np.int32) for k in n], how=[np.array([""] * k, dtype=object) for k in n])
    open_ = [np.ones(k, bool) for k in n]
    for _ in range(max_steps // chunk):
        model.step(chunk)
        for k, loop in enumerate(model.loops):
            env = loop.env
            frozen, limit = env["frozen"] != 0, env["steps"] >= max_steps
            ends = open_[k] & (frozen | limit)
            out["fitness"][k][ends], out["steps"][k][ends] = env["fitness"][ends], env["steps"][ends]
            out["how"][k][ends & frozen] = "frozen"            # (frozen at the limit's own boundary counts as frozen)
            out["how"][k][ends & ~frozen] = "steps"
            open_[k] &= ~ends
    assert not any(o.any() for o in open_)
    out["over"] = model.over_capacity()
    _RUNS[key] = out
    return out


def by_id(per_bucket, ids, n_total, dtype=None):
    """a per-bucket result in id order: ids[k][e] = the id of creature e of bucket k"""
    out = np.zeros(n_total, per_bucket[0].dtype if dtype is None else dtype)
    for v, i in zip(per_bucket, ids):
        out[np.asarray(i)] = v
    return out
