"""The refusals of the search tiers' Python layer (policy.py, elites.py, novelty.py, pareto.py), pinned byte for byte without a GPU
against tests/golden/value_errors.json, in two walks:

`cases`: the tiers' own refusal tests, imported and run as they are while `pytest.raises` is a wrapper that hands on to the real one
and notes the type and the whole text of what was raised -- every message the tests provoke, in their order.

`chains`: the ORDER of every public call's checks, which cases of one fault each cannot show.  A call is made with every argument
wrong at once and its message noted; then the one argument whose repair changes the message is repaired, and so on until nothing is
wrong: on the CPU the last refusal is that of a device that is no GPU (`CentroidArchive.assign` has a host route and returns).  An
argument may hold several faults, repaired one after the other (a fitness of the wrong dtype, then of the wrong shape, then on the
wrong device).  Two checks that swap places change a chain.

The record was made by this file's `--record` mode before the four modules were put on gym_rem2d_amd/_tier.py; no text holds an
address, and none depends on the build of the library."""
import importlib
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "value_errors.json")

WALKED = (
    ("test_elites_host", ("test_elites_value_errors",)),
    ("test_es_host", ("test_es_value_errors", "test_run_policy_es_checks_the_env")),
    ("test_snes_host", ("test_separable_es_value_errors", "test_run_policy_snes_checks_the_env")),
    ("test_novelty_host", ("test_novelty_value_errors",)),
    ("test_pareto_host", ("test_pareto_value_errors",)),
    ("test_cvt_host", ("test_python_layer_errors", "test_cvt_centroids_on_the_cpu")),
    ("test_evolve_host", ("test_evolve_value_errors", "test_run_policy_generations_checks_the_env")),
    ("test_policy_host", ("test_mlp_policy_shapes_and_values", "test_set_policy_checks_the_population")),
    ("test_recurrent_host", ("test_recurrent_policy_shapes_and_values", "test_set_policy_checks_streaming")),
)


class _Noting:
    """pytest.raises, handed on to; what was raised is appended to `log` on the way out"""

    def __init__(self, real, log, args, kw):
        self.inner, self.log = real(*args, **kw), log

    def __enter__(self):
        return self.inner.__enter__()

    def __exit__(self, kind, value, tb):
        caught = self.inner.__exit__(kind, value, tb)      # (fails as the real one does where nothing, or something else, was raised)
        if value is not None:
            self.log.append([type(value).__name__, str(value)])
        return caught


def walk_cases():
    """{module.function: [[type name, text], ...]} of the tiers' refusal tests"""
    real, out = pytest.raises, {}
    for module, names in WALKED:
        mod = importlib.import_module(module)
        for name in names:
            log = out[module + "." + name] = []
            pytest.raises = lambda *a, **kw: _Noting(real, log, a, kw)
            try:
                getattr(mod, name)()
            finally:
                pytest.raises = real
    return out


# ---------------------------------------------------------------------------------------------------- the order of the checks
def peel(call, good, bad):
    """[[type name, text], ...]: `call(**arguments)` with every fault of `bad` {argument: [worse, ..., less bad]} in place, then
    with the one fault repaired whose repair changes the message, until `good` is all there is."""
    stage = {k: 0 for k in bad}

    def attempt(stage):
        kw = {k: (bad[k][stage[k]] if k in stage and stage[k] < len(bad[k]) else v) for k, v in good.items()}
        try:
            call(**kw)
        except Exception as e:
            return [type(e).__name__, str(e)]
        return ["returned", ""]

    chain = [attempt(stage)]
    while any(stage[k] < len(bad[k]) for k in bad):
        for k in bad:
            if stage[k] < len(bad[k]):
                after = attempt(dict(stage, **{k: stage[k] + 1}))
                if after != chain[-1]:
                    stage[k] += 1
                    chain.append(after)
                    break
        else:
            raise AssertionError("no repair moves the call past %r: %r" % (chain[-1], stage))
    return chain


def _method(name):
    return lambda self, **kw: getattr(self, name)(**kw)


def chains():
    """{entry point: its chain}.  Faults that an earlier check hides by design, and so make no link:
    - `seed` out of range shares one message with `generation`; `sigma` (evolve, es_sample, emit) and `lr` (es_update) are not checked by
      the wrappers;
    - forward, of both policy classes: on the CPU the first check of `descriptor` is the device's, which hides all the others;
    - `fitness` where `util=` is given (es_update, SeparableES.update): it is not looked at;
    - emit / emit_line with `out=`: n_children that is no multiple of the blocks is refused as "must have n weight sets" first."""
    import torch
    from gym_rem2d_amd import elites, novelty, pareto, policy
    f32, f64, i32, i64 = torch.float32, torch.float64, torch.int32, torch.int64
    out = {}

    def four(p):
        return p.w1, p.b1, p.w2, p.b2

    # ---- policy.py: M = 4 means or sets, S = 4 children each (two pairs, so that pair_chunk = 1 asks for scratch)
    M, S = 4, 4
    p, q = policy.MLPPolicy.random(M, 2, 3, n_rays=0, seed=1), policy.MLPPolicy.random(M, 2, 3, n_rays=0, seed=2)
    kids, wrong = policy.MLPPolicy.random(M * S, 2, 3, n_rays=0, seed=3), policy.MLPPolicy.random(M, 2, 5, n_rays=0, seed=4)
    n1 = p.w1[0].numel()
    base = torch.zeros(M * S * n1 + 8)
    mean = policy.MLPPolicy(base[:M * n1].view_as(p.w1), p.b1, p.w2, p.b2)                 # a mean inside storage that `over` covers
    over = policy.MLPPolicy(base[4:4 + M * S * n1].view(M * S, *p.w1.shape[1:]), kids.b1, kids.w2, kids.b2)
    indexed = policy.MLPPolicy(*four(mean), index=list(range(M)))
    view = policy.MLPPolicy(mean.w1, q.b1, q.w2, q.b2)
    fit = lambda n: [torch.zeros(n, dtype=f32), torch.zeros(n - 1, dtype=f64), torch.zeros(n, dtype=f64, device="meta")]
    rec = policy.RecurrentPolicy.random(M, 2, 3, 2, n_rays=0)
    obs = torch.zeros((M, p.d))
    out["MLPPolicy.forward"] = peel(_method("forward"), dict(self=p, obs=obs.double(), frac=obs, out=(obs, obs), row_mask=obs), {})
    out["RecurrentPolicy.forward"] = peel(_method("forward"), dict(self=rec, obs=obs.double(), frac=obs, memory=obs, reset=obs), {})
    good = dict(self=mean, fitness=torch.zeros(M, dtype=f64), generation=1, seed=0, rate=0.05, tournsize=2, group_size=2, elite=0, out=q)
    bad = dict(self=[indexed], fitness=fit(M), group_size=[3], tournsize=[9], elite=[2], rate=[1.5], generation=[-1], out=[mean, wrong, view])
    out["MLPPolicy.evolve"] = peel(_method("evolve"), good, bad)
    out["MLPPolicy.evolve(parents=)"] = peel(_method("evolve"), dict(good, parents=torch.zeros(M, dtype=i32)),
                                             dict(bad, parents=[torch.zeros(M, dtype=i64)]))
    out["MLPPolicy.es_sample"] = peel(_method("es_sample"), dict(self=mean, generation=1, seed=0, group_size=S, out=kids),
                                      dict(self=[indexed], group_size=[3, 2 ** 30], generation=[2 ** 32], out=[mean, q, over]))
    good = dict(self=mean, fitness=torch.zeros(M * S, dtype=f64), generation=1, seed=0, sigma=0.1, group_size=S, out=q, pair_chunk=1,
                scratch=torch.zeros(1 << 12, dtype=i64))
    bad = dict(self=[indexed], fitness=fit(M * S), group_size=[3, 2 ** 30], generation=[-1], pair_chunk=[-1], sigma=[0.0],
               scratch=[torch.zeros(1, dtype=i64)], out=[mean, kids, view])
    out["MLPPolicy.es_update"] = peel(_method("es_update"), good, bad)
    del bad["fitness"]
    out["MLPPolicy.es_update(util=)"] = peel(_method("es_update"), dict(good, fitness=None, util=torch.zeros(M * S, dtype=i32)),
                                             dict(bad, util=[torch.zeros(M, dtype=i32)]))
    es = policy.SeparableES(p, S)
    es.mean.w1 = base[:M * n1].view_as(p.w1)                                                # (as `mean` above; then the same for sigma)
    base2 = torch.zeros(M * S * n1 + 8)
    es.sigma[0] = base2[:M * n1].view_as(p.w1)
    over2 = policy.MLPPolicy(base2[4:4 + M * S * n1].view(M * S, *p.w1.shape[1:]), kids.b1, kids.w2, kids.b2)
    out["SeparableES.sample"] = peel(_method("sample"), dict(self=es, generation=1, seed=0, out=kids),
                                     dict(generation=[-1], out=[es.mean, q, over, over2]))
    good = dict(self=es, fitness=torch.zeros(M * S, dtype=f64), generation=1, seed=0, pair_chunk=1, scratch=torch.zeros(1 << 12, dtype=i64))
    bad = dict(generation=[-1], pair_chunk=[-1], fitness=fit(M * S), scratch=[torch.zeros(1, dtype=i64)])
    out["SeparableES.update"] = peel(_method("update"), good, bad)
    del bad["fitness"]
    out["SeparableES.update(util=)"] = peel(_method("update"), dict(good, fitness=None, util=torch.zeros(M * S, dtype=i32)),
                                            dict(bad, util=[torch.zeros(M, dtype=i32)]))

    # ---- elites.py: 2 blocks, 8 rows of 2 words
    like = policy.MLPPolicy.random(8, 1, 2, n_rays=0)
    other = policy.MLPPolicy.random(8, 1, 3, n_rays=0)
    indexed = policy.MLPPolicy(*four(like), index=torch.arange(8))
    cen = torch.arange(10, dtype=f32).view(5, 2)
    for name, g in (("EliteGrid", elites.EliteGrid(2, [(0, -1.0, 1.0, 4), (1, 0.0, 2.0, 3)], 2, like)),
                    ("CentroidArchive", elites.CentroidArchive(2, cen, like))):
        inside = torch.zeros(16 + 2 * g.n_cells * 2)
        g.desc = inside[:2 * g.n_cells * 2].view(2, g.n_cells, 2)
        shared = policy.MLPPolicy(g.w1[:8], like.b1, like.w2, like.b2)
        desc = [torch.zeros((8, 2), dtype=f64), torch.zeros((8, 3)), inside[2 * g.n_cells * 2 - 8:][:16].view(8, 2)]
        if name == "CentroidArchive":
            pool = torch.zeros(16 + 10)
            g.centroids = pool[:10].view(5, 2)
            desc.append(pool[6:22].view(8, 2))
        good = dict(self=g, policy=like, fitness=torch.zeros(8, dtype=f64), desc=torch.zeros((8, 2)), mask=torch.ones(8, dtype=torch.bool), group_size=4)
        bad = dict(policy=[indexed, other, like.to("meta"), shared], fitness=[torch.zeros(8), torch.zeros(7, dtype=f64)], desc=desc,
                   group_size=[3], mask=[torch.zeros(8), torch.zeros(7, dtype=torch.bool)])
        out[name + ".insert"] = peel(_method("insert"), good, bad)
        out[name + ".insert(group_size=None)"] = peel(_method("insert"), dict(good, group_size=None, self=elites.EliteGrid(3, [(0, 0.0, 1.0, 2)], 2, like)
                                                                              if name == "EliteGrid" else elites.CentroidArchive(3, cen, like)), {})
        out[name + ".sample"] = peel(_method("sample"), dict(self=g, generation=1, seed=0, n_children=4, out=torch.zeros(4, dtype=i32)),
                                     dict(generation=[-1], n_children=[3], out=[torch.zeros(2, dtype=i32)]))
        good = dict(self=g, generation=1, seed=0, n_children=8, out=policy.MLPPolicy.random(8, 1, 2, n_rays=0, seed=5))
        bad = dict(out=[g, other, like.to("meta"), shared], n_children=[6], generation=[2 ** 32])
        out[name + ".emit"] = peel(_method("emit"), dict(good, rate=0.05), dict(bad, rate=[1.5]))
        out[name + ".emit(out=None)"] = peel(_method("emit"), dict(good, rate=0.05, out=None), dict(generation=[-1], n_children=[3], rate=[-0.1]))
        out[name + ".emit_line"] = peel(_method("emit_line"), dict(good, sigma_iso=0.01, sigma_line=0.2), dict(bad, sigma_iso=[float("nan")]))
        out[name + ".emit_line(out=None)"] = peel(_method("emit_line"), dict(good, sigma_line=0.2, out=None),
                                                  dict(generation=[-1], n_children=[3], sigma_line=[float("inf")]))
    arch = elites.CentroidArchive(2, cen, like)
    rows = torch.zeros((7, 2))
    out["CentroidArchive.assign"] = peel(_method("assign"), dict(self=arch, desc=rows, out=torch.zeros(7, dtype=i32), dist=torch.zeros(7), splits=0),
                                         dict(desc=[rows.double(), torch.zeros((7, 3)), rows[:0], rows.to("meta")], out=[torch.zeros(6, dtype=i32)],
                                              dist=[torch.zeros(7, dtype=f64)], splits=[-1]))

    # ---- novelty.py: 2 blocks, 8 rows of 2 words
    a = novelty.NoveltyArchive(2, 6, 2)
    inside = torch.zeros(16 + 24)
    a.entries = inside[:24].view(2, 6, 2)
    desc = torch.zeros((8, 2))
    bad = dict(desc=[desc.double(), torch.zeros((8, 3)), desc[:0], desc.to("meta"), inside[20:36].view(8, 2)], group_size=[3])
    score = dict(k=[0], out=[torch.zeros(7, dtype=f64), desc.view(f64).view(8)])
    draw = dict(generation=[-1], rate=[1.5], mask=[torch.zeros(8), torch.zeros(7, dtype=torch.bool)])
    good = dict(self=a, desc=desc, group_size=4)
    out["NoveltyArchive.score"] = peel(_method("score"), dict(good, k=3, out=torch.zeros(8, dtype=f64)), dict(bad, **score))
    out["NoveltyArchive.score(group_size=None)"] = peel(_method("score"), dict(self=a, desc=torch.zeros((7, 2)), group_size=None), {})
    out["NoveltyArchive.add"] = peel(_method("add"), dict(good, generation=1, seed=0, rate=0.02, mask=torch.ones(8, dtype=torch.bool)), dict(bad, **draw))
    out["NoveltyArchive.step"] = peel(_method("step"), dict(good, generation=1, seed=0, k=3, rate=0.02, mask=torch.ones(8, dtype=torch.uint8),
                                                            out=torch.zeros(8, dtype=f64)), dict(bad, **score, **draw))

    # ---- pareto.py: 8 rows
    obj = torch.zeros((8, 2), dtype=f64)
    outs = (torch.zeros(8, dtype=i32), torch.zeros(8, dtype=f64), torch.zeros(8, dtype=i32), torch.zeros(2, dtype=i32))
    out["pareto.rank"] = peel(pareto.rank, dict(objectives=obj, group_size=4, out=outs),
                              dict(objectives=[obj.float(), torch.zeros((8, 2, 1), dtype=f64), torch.zeros((8, 5), dtype=f64)], group_size=[3],
                                   out=[outs[:3], (outs[0], outs[1].float(), outs[2], outs[3]), (outs[0], None, outs[2], outs[0]),
                                        (None, obj.view(16)[:8], None, None)]))
    desc, fitness = torch.zeros((8, 2)), torch.zeros(8, dtype=f64)
    out["pareto.local_competition"] = peel(pareto.local_competition, dict(desc=desc, fitness=fitness, k=3, group_size=4, out=torch.zeros(8, dtype=f64)),
                                           dict(desc=[desc.double(), torch.zeros((8, 33))], fitness=[fitness.float()], k=[0], group_size=[3],
                                                out=[torch.zeros(8), desc.view(f64).view(8), fitness]))
    return out


def walk():
    import __graft_entry__ as g
    g.build()              # (es_update and SeparableES.update ask the library for their scratch size)
    return {"cases": walk_cases(), "chains": chains()}


def test_every_value_error_is_the_recorded_one():
    with open(GOLDEN) as f:
        want = json.load(f)
    assert len(want["cases"]) == 15 and sum(len(v) for v in want["cases"].values()) >= 423      # (a walk that shrank is no record)
    assert len(want["chains"]) == 31 and sum(len(v) for v in want["chains"].values()) >= 228
    got = walk()
    for part in ("cases", "chains"):
        assert sorted(got[part]) == sorted(want[part])
        for name in want[part]:
            for i, (a, b) in enumerate(zip(got[part][name], want[part][name])):
                assert a == b, "%s, refusal %d of %s: %r, the record has %r" % (part, i, name, a, b)
            assert len(got[part][name]) == len(want[part][name]), name


if __name__ == "__main__" and sys.argv[1:2] == ["--record"]:
    # python tests/test_value_error_text_host.py --record [--overwrite].  A record that exists is what the Python layer is held to: a
    # changed text or order is a failure of the test, not a reason to record again; it is replaced only where the walk itself changes.
    if os.path.exists(GOLDEN) and "--overwrite" not in sys.argv[2:]:
        sys.exit("%s exists; a changed refusal is a failure of the test, not a reason to record again (--overwrite to replace it)" % GOLDEN)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    record = walk()
    assert record == walk(), "two walks differ: a text holds something that changes from run to run"
    with open(GOLDEN, "w") as f:
        json.dump(record, f, indent=0, sort_keys=True)
        f.write("\n")
    for part, rows in record.items():
        print("%s: %d refusals over %d entries" % (part, sum(len(v) for v in rows.values()), len(rows)))
