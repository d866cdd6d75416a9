"""The seven generational loops of evaluate.py (run_policy_generations, _es, _snes, _nses, _pareto_es, _nslc, _map_elites), held
without a GPU to tests/golden/policy_loops.json in two parts:

`traces`: every loop runs against stand-ins that do no device work and note every call made on them, in order, with its salient
arguments: generation, seed and rates, group_size, whether a normaliser was handed on and with which `accumulate`, the sum of a reset
mask, step counts, period / samples, whether the first act() of an episode would read a reset mask.  Every policy and tensor is named
by a label, not by its address: `caller` for the caller's policy or mean, then `buf0`, `buf1`, ... in order of first appearance, so
the trace shows which buffer a generation writes and which one `on_generation` sees.  The `on_generation` arguments, the `log`
strings, the returned history and the label of what is returned are part of it.  The ORDER of the calls is what is pinned; the device
work is not -- the loop replays of the GPU tier hold the bits.

`chains`: the order and wording of what every loop, run_policy_episode and run_behaviour_episode refuse: `peel` of
tests/test_value_error_text_host.py, every argument wrong at once, repaired one at a time until the call reaches the stand-in.

The record was made by this file's `--record` mode before the loops were put on one driver; the test never makes it again."""
import json
import os
import sys

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_rem2d_amd import evaluate, pareto, policy
from gym_rem2d_amd.elites import EliteGrid
from test_value_error_text_host import peel

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "policy_loops.json")
N, S, K = 8, 4, 2          # 8 creatures in blocks of 4; descriptors of 2 samples
CPU = torch.device("cpu")


class Trace:
    """The calls, in order, and the labels of the objects they name"""

    def __init__(self):
        self.calls, self.names, self.kept = [], {}, []

    def name(self, obj, label):
        self.names[id(obj)] = label
        self.kept.append(obj)          # (kept alive: an address is never given out twice)
        return obj

    def label(self, obj):
        if obj is None or isinstance(obj, (bool, int, float, str)):
            return obj
        if isinstance(obj, (tuple, list)):
            return [self.label(o) for o in obj]
        if id(obj) not in self.names:
            self.name(obj, "buf%d" % sum(1 for v in self.names.values() if v.startswith("buf")))
        return self.names[id(obj)]

    def note(self, what, *args, **kw):
        self.calls.append([what] + [self.label(a) for a in args] + [[k, self.label(v)] for k, v in kw.items()])


class World:
    device = CPU


class LoopEnv:
    """What the loops need of a BatchedModular2D, on the CPU: everyone is frozen after the first chunk, the fitness is
    arange(n) + the step calls so far (one per episode), no creature has an error bit."""

    def __init__(self, trace, worlds=True, autoreset=None, stream=None, attached=None):
        self.trace, self.n_envs, self.flags = trace, N, 0
        self.worlds = [(World(), None)] if worlds else []
        self._autoreset, self._stream_rec, self._descriptor, self._policy = autoreset, stream, None, attached
        self._context_reset, self.steps, self.last_episode = False, 0, "an earlier report"

    @property
    def policy(self):
        return self._policy

    def set_policy(self, policy, normalizer=None, accumulate=True):
        self.trace.note("set_policy", policy, normalizer=normalizer is not None, accumulate=accumulate)
        self._policy, self._context_reset = policy, False

    def reset_where(self, mask=None, when=(), max_steps=None):
        self.trace.note("reset_where", None if mask is None else [str(mask.dtype), int(mask.sum())])
        self._context_reset = True

    def _step(self, what, n):
        self.trace.note(what, n, first_act_reads_reset=self._context_reset)
        self._context_reset = False
        self.steps += 1

    def step(self, n):
        self._step("step", n)

    def step_policy(self, n=1):
        self._step("step_policy", n)

    def set_descriptor(self, period, samples=None):
        self.trace.note("set_descriptor", period, samples)
        self._descriptor = (int(period), int(samples), torch.zeros((N, 2 * int(samples)), dtype=torch.float32))

    @property
    def behaviour(self):
        return None if self._descriptor is None else self._descriptor[2]

    def describe(self):
        self.trace.note("describe")

    @property
    def frozen(self):
        return torch.ones(N, dtype=torch.int32)

    @property
    def fitness(self):
        return torch.arange(N, dtype=torch.float64) + self.steps

    def errors(self):
        return torch.zeros(N, dtype=torch.int32)


class LoopPolicy(policy.MLPPolicy):
    """An MLPPolicy on the CPU whose search steps launch nothing: they note the call and return `out`, or a new policy"""
    trace, scratch = None, 0

    @classmethod
    def make(cls, trace, n_sets, scratch=0, label=None, **kw):
        p = cls.random(n_sets, 2, 3, n_rays=0, seed=n_sets, **kw)
        p.trace, p.scratch = trace, scratch
        return trace.name(p, label) if label else p

    def _like(self, w1, b1, w2, b2, index):
        p = LoopPolicy(w1, b1, w2, b2, self.activation, self.scale, index, self.rays)
        p.trace, p.scratch = self.trace, self.scratch
        return p

    def to(self, device):
        self.trace.note("to", self, str(device))
        return self

    def evolve(self, fitness, generation, seed=0, rate=0.05, sigma=0.1, tournsize=4, group_size=None, elite=0, parents=None, out=None,
               wide=False):
        self.trace.note("evolve", self, fitness, generation, seed=seed, rate=rate, sigma=sigma, tournsize=tournsize, group_size=group_size,
                        elite=elite, out=out)
        return self._sets(self.n_sets) if out is None else out

    def es_scratch_bytes(self, group_size, pair_chunk=0, wide=False):
        self.trace.note("es_scratch_bytes", self, group_size)
        return self.scratch

    def es_sample(self, generation, seed=0, sigma=0.1, group_size=None, out=None, wide=False):
        self.trace.note("es_sample", self, generation, seed=seed, sigma=sigma, group_size=group_size, out=out)
        return self._sets(self.n_sets * group_size) if out is None else out

    def es_update(self, fitness, generation, seed=0, sigma=0.1, lr=0.05, group_size=None, out=None, scratch=None, util=None,
                  pair_chunk=0, wide=False):
        self.trace.note("es_update", self, fitness, generation, seed=seed, sigma=sigma, lr=lr, group_size=group_size, out=out,
                        scratch=None if scratch is None else [str(scratch.dtype), scratch.numel()], util=util,
                        util_is=None if util is None else util.tolist())
        return self._sets(self.n_sets) if out is None else out


class LoopES:
    """policy.SeparableES as run_policy_snes uses it: one child policy, two means written in turn"""

    def __init__(self, trace, n_sets=N // S, group_size=S, device=CPU):
        self.trace, self.group_size, self.device = trace, group_size, device
        self.mean, self._spare = LoopPolicy.make(trace, n_sets, label="caller"), LoopPolicy.make(trace, n_sets)
        self._children = LoopPolicy.make(trace, n_sets * group_size)

    def sample(self, generation, seed=0, out=None, wide=False):
        self.trace.note("es.sample", generation, seed=seed)
        return self._children

    def update(self, fitness, generation, seed=0, util=None, scratch=None, pair_chunk=0, wide=False):
        self.trace.note("es.update", fitness, generation, seed=seed)
        self.mean, self._spare = self._spare, self.mean
        return self.mean


class LoopArchive:
    """novelty.NoveltyArchive as the loops use it"""

    def __init__(self, trace, n_blocks=N // S, width=2 * K, device=CPU):
        self.trace, self.n_blocks, self.width, self.device = trace, n_blocks, width, device

    def step(self, desc, generation, k=15, seed=0, rate=0.02, group_size=None, mask=None, out=None):
        self.trace.note("archive.step", desc, generation, k=k, seed=seed, rate=rate, group_size=group_size, out=out)
        out.copy_(torch.arange(N, dtype=torch.float64) * generation)
        return out


class LoopGrid(EliteGrid):
    """elites.EliteGrid (or a CentroidArchive: the loop asks for no more) as run_policy_map_elites uses it"""

    def __init__(self, trace, n_blocks=N // S, width=2 * K, device=CPU):
        self.trace, self.n_blocks, self.width, self._device, self.inserts = trace, n_blocks, width, device, 0

    @property
    def device(self):
        return self._device

    @property
    def n_filled(self):
        return torch.full((self.n_blocks,), self.inserts, dtype=torch.int32)

    def qd_score(self):
        return torch.full((self.n_blocks,), 0.5 * self.inserts, dtype=torch.float64)

    def emit(self, generation, seed=0, rate=0.05, sigma=0.1, n_children=None, out=None, wide=False):
        self.trace.note("grid.emit", generation, seed=seed, rate=rate, sigma=sigma, n_children=n_children, out=out)
        return out

    def emit_line(self, generation, seed=0, sigma_iso=0.01, sigma_line=0.2, n_children=None, out=None, wide=False):
        self.trace.note("grid.emit_line", generation, seed=seed, sigma_iso=sigma_iso, sigma_line=sigma_line, n_children=n_children, out=out)
        return out

    def insert(self, policy, fitness, desc, mask=None, group_size=None, wide=False):
        self.trace.note("grid.insert", policy, fitness, desc, group_size=group_size)
        self.inserts += 1


class LoopNormalizer:
    def __init__(self, trace):
        self.trace = trace

    def freeze(self, wide=False):
        self.trace.note("normalizer.freeze")


def patched(trace, monkeypatch):
    """evaluate._es_ranks, pareto.rank and pareto.local_competition as recorders that write something that tells the calls apart"""
    count = [0]

    def es_ranks(mean, values, group_size, out):
        count[0] += 1
        trace.note("_es_ranks", mean, values, group_size, out)
        return out.copy_(torch.arange(N, dtype=torch.int32) + 10 * count[0])

    def rank(objectives, group_size=None, out=None, wide=False):
        count[0] += 1
        trace.note("pareto.rank", objectives, group_size=group_size, out=out, objectives_are=objectives.tolist())
        out[2].copy_(torch.arange(N, dtype=torch.int32) + 10 * count[0])
        return pareto.ParetoRank(*out)

    def local_competition(desc, fitness, k=15, group_size=None, out=None, wide=False):
        trace.note("pareto.local_competition", desc, fitness, k=k, group_size=group_size, out=out)
        return out.copy_(fitness * 2)
    monkeypatch.setattr(evaluate, "_es_ranks", es_ranks)
    monkeypatch.setattr(pareto, "rank", rank)
    monkeypatch.setattr(pareto, "local_competition", local_competition)


# --------------------------------------------------------------------------------------------------------------- the traces
def trace_cases():
    """{case: (loop, generations, keywords beyond the common ones)}; `normalizer`: True where one is handed on"""
    cases = {}
    for name, kw in (("run_policy_generations", dict(seed=3, rate=0.1, sigma=0.2, tournsize=2, group_size=S, elite=1, chunk=7, max_steps=20)),
                     ("run_policy_es", dict(seed=3, sigma=0.2, lr=0.3, group_size=S, chunk=7, max_steps=20)),
                     ("run_policy_snes", dict(seed=3, chunk=7, max_steps=20)),
                     ("run_policy_nses", dict(k=3, rate=0.3, weights=(1, 1), samples=K, seed=3, sigma=0.2, lr=0.3, group_size=S, max_steps=20)),
                     ("run_policy_pareto_es", dict(k=3, rate=0.3, samples=K, seed=3, sigma=0.2, lr=0.3, group_size=S, max_steps=20)),
                     ("run_policy_nslc", dict(k=3, rate=0.3, samples=K, seed=3, mut_rate=0.1, sigma=0.2, tournsize=2, group_size=S, max_steps=20)),
                     ("run_policy_map_elites", dict(samples=K, seed=3, rate=0.1, sigma=0.2, group_size=S, max_steps=20))):
        cases[name] = (name, 3, kw)
        cases[name + "(n_generations=0)"] = (name, 0, kw)
        if name not in ("run_policy_pareto_es", "run_policy_nslc"):
            cases[name + "(normalizer=)"] = (name, 3, dict(kw, normalizer=True))
    cases["run_policy_es(scratch)"] = ("run_policy_es", 3, dict(cases["run_policy_es"][2], scratch=64))
    cases["run_policy_nses(weights=(1, 0), period=)"] = ("run_policy_nses", 3, dict(cases["run_policy_nses"][2], weights=(1, 0), period=6, scratch=64))
    cases["run_policy_pareto_es(scratch)"] = ("run_policy_pareto_es", 3, dict(cases["run_policy_pareto_es"][2], scratch=64))
    cases["run_policy_nslc(elite=, period=)"] = ("run_policy_nslc", 3, dict(cases["run_policy_nslc"][2], elite=1, period=6))
    cases["run_policy_map_elites(sigma_line=)"] = ("run_policy_map_elites", 3, dict(cases["run_policy_map_elites"][2], sigma_line=0.4))
    cases["run_policy_map_elites(group_size=None, normalizer=)"] = ("run_policy_map_elites", 2, dict(cases["run_policy_map_elites"][2], group_size=None,
                                                                                                    normalizer=True))
    return cases


def run_case(monkeypatch, loop, generations, kw):
    """One loop against the stand-ins -> its trace"""
    t = Trace()
    patched(t, monkeypatch)
    kw = dict(kw)
    scratch = kw.pop("scratch", 0)
    if kw.pop("normalizer", False):
        kw["normalizer"] = LoopNormalizer(t)
    env = LoopEnv(t)
    per_creature = loop in ("run_policy_generations", "run_policy_nslc", "run_policy_map_elites")
    args = [LoopES(t) if loop == "run_policy_snes" else LoopPolicy.make(t, N if per_creature else N // S, scratch, label="caller")]
    if loop == "run_policy_map_elites":
        args.append(t.name(LoopGrid(t), "grid"))
    args.append(generations)
    if loop in ("run_policy_nses", "run_policy_pareto_es", "run_policy_nslc"):
        args.append(t.name(LoopArchive(t), "archive"))
    got = getattr(evaluate, loop)(env, *args, on_generation=lambda *a: t.note("on_generation", *a), log=lambda s: t.note("log", s), **kw)
    assert env.last_episode is None or generations == 0
    return {"calls": t.calls, "returned": [t.label(got[0]), t.label(got[1])], "history": [list(row) for row in got[2]]}


def traces(monkeypatch):
    return {name: run_case(monkeypatch, *case) for name, case in trace_cases().items()}


# --------------------------------------------------------------------------------------------------------------- the refusals
def chains(monkeypatch):
    """{entry point: its chain}.  The env's faults come off one at a time (no population, then auto-reset or streaming: one message
    for both, so each loop that looks is walked once with either); an archive or grid is first of the wrong type or block count, then
    of the wrong width, then on the wrong device."""
    t = Trace()
    patched(t, monkeypatch)
    meta = torch.device("meta")
    out = {}

    def envs(**second):
        return [LoopEnv(t, worlds=False, **second)] + ([LoopEnv(t, **second)] if second else [])

    def archives(make):
        return [make(t, n_blocks=3, width=5, device=meta), make(t, width=5, device=meta), make(t, device=meta)]

    mean, pop = LoopPolicy.make(t, N // S), LoopPolicy.make(t, N)
    out["run_policy_episode"] = peel(evaluate.run_policy_episode, dict(env=LoopEnv(t, attached=pop), max_steps=5, on_error="ignore"),
                                     dict(env=[LoopEnv(t)], on_error=["fallback"]))
    out["run_behaviour_episode"] = peel(evaluate.run_behaviour_episode, dict(env=LoopEnv(t), period=5, samples=K, max_steps=5, on_error="ignore"),
                                        dict(env=[LoopEnv(t, worlds=False)], on_error=["fallback"]))
    good = dict(env=LoopEnv(t), n_generations=1, group_size=S, max_steps=5, on_error="warn")
    out["run_policy_generations"] = peel(evaluate.run_policy_generations, dict(good, policy=pop), dict(on_error=["penalty"]))
    out["run_policy_es"] = peel(evaluate.run_policy_es, dict(good, mean=mean),
                                dict(env=envs(), group_size=[3, 1], mean=[LoopPolicy.make(t, 3)], on_error=["penalty"]))
    out["run_policy_snes"] = peel(evaluate.run_policy_snes, dict(env=LoopEnv(t), es=LoopES(t), n_generations=1, max_steps=5, on_error="warn"),
                                  dict(env=envs(), es=[LoopES(t, group_size=3, device=meta), LoopES(t, n_sets=3, device=meta), LoopES(t, device=meta)],
                                       on_error=["penalty"]))
    searching = dict(good, archive=LoopArchive(t), samples=K)
    for tag, second in (("auto-reset", dict(autoreset=(("done",), 100))), ("streaming", dict(stream=object()))):
        bad = dict(env=envs(**second), group_size=[3, 1], archive=archives(LoopArchive), on_error=["penalty"])
        if tag == "auto-reset":         # (run_policy_nses does not look at either)
            out["run_policy_nses"] = peel(evaluate.run_policy_nses, dict(searching, mean=mean, weights=(2, -3)),
                                          dict(bad, env=envs(), mean=[LoopPolicy.make(t, 3)], weights=[(1.5, 1), (1, 40000), (-32768, 1)]))
        out["run_policy_pareto_es (%s)" % tag] = peel(evaluate.run_policy_pareto_es, dict(searching, mean=mean), dict(bad, mean=[LoopPolicy.make(t, 3)]))
        out["run_policy_nslc (%s)" % tag] = peel(evaluate.run_policy_nslc, dict(searching, policy=pop), dict(bad, policy=[mean]))
        out["run_policy_map_elites (%s)" % tag] = peel(
            evaluate.run_policy_map_elites, dict(good, policy=pop, grid=LoopGrid(t), samples=K),
            dict(grid=[LoopArchive(t)] + archives(LoopGrid), env=envs(**second), group_size=[3],
                 policy=[LoopPolicy.make(t, 3, index=[0] * N)], on_error=["penalty"]))     # (one message for a wrong count and an index)
    return out


def walk(monkeypatch):
    return json.loads(json.dumps({"traces": traces(monkeypatch), "chains": chains(monkeypatch)}))


@pytest.fixture(scope="module")
def record():
    with open(GOLDEN) as f:
        want = json.load(f)
    assert len(want["traces"]) == 25 and sum(len(v["calls"]) for v in want["traces"].values()) >= 608      # (a walk that shrank is no record)
    assert len(want["chains"]) == 12 and sum(len(v) for v in want["chains"].values()) >= 92
    return want


@pytest.mark.parametrize("name", sorted(trace_cases()))
def test_a_loop_makes_the_recorded_calls_in_the_recorded_order(name, record, monkeypatch):
    got = json.loads(json.dumps(run_case(monkeypatch, *trace_cases()[name])))
    want = record["traces"][name]
    for i, (a, b) in enumerate(zip(got["calls"], want["calls"])):
        assert a == b, "call %d of %s: %r, the record has %r" % (i, name, a, b)
    assert len(got["calls"]) == len(want["calls"])
    assert got["returned"] == want["returned"] and got["history"] == want["history"]


def test_every_case_is_recorded(record):
    assert sorted(record["traces"]) == sorted(trace_cases())


def test_every_refusal_is_the_recorded_one_in_the_recorded_order(record, monkeypatch):
    got = json.loads(json.dumps(chains(monkeypatch)))
    assert sorted(got) == sorted(record["chains"])
    for name, want in record["chains"].items():
        for i, (a, b) in enumerate(zip(got[name], want)):
            assert a == b, "refusal %d of %s: %r, the record has %r" % (i, name, a, b)
        assert len(got[name]) == len(want), name
        assert got[name][-1] == ["returned", ""], name          # (repaired, the call reaches the stand-in and comes back)


if __name__ == "__main__" and sys.argv[1:2] == ["--record"]:
    # python tests/test_policy_loops_host.py --record [--overwrite].  A record that exists is what the loops are held to: a changed
    # call, order or text is a failure of the test, not a reason to record again; it is replaced only where the walk itself changes.
    if os.path.exists(GOLDEN) and "--overwrite" not in sys.argv[2:]:
        sys.exit("%s exists; a changed trace is a failure of the test, not a reason to record again (--overwrite to replace it)" % GOLDEN)
    with pytest.MonkeyPatch.context() as mp:
        made = walk(mp)
        assert made == walk(mp), "two walks differ: a trace holds something that changes from run to run"
    with open(GOLDEN, "w") as f:
        json.dump(made, f, indent=0, sort_keys=True)
        f.write("\n")
    print("traces: %d calls over %d cases; chains: %d refusals over %d entries" % (
        sum(len(v["calls"]) for v in made["traces"].values()), len(made["traces"]), sum(len(v) for v in made["chains"].values()), len(made["chains"])))
