"""Population-order reads of a multi-world env (fitness / frozen / steps / errors) on the GPU path (pytest -m gpu).

They are one kernel of librem2d.so per world (rem2d_world_gather, include/rem2d_gather.h), whose code object the steps have
already loaded.  They used to be torch's index_copy_, whose first launch loads a code object of torch's own: 8-45 ms inside
the first timed block of bench.py, which doubled it.  The guard is structural: the reads must not reach a torch
indexing op at all."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_TORCH_INDEXING = ("index_copy_", "index_copy", "index_put_", "index_put", "index_select", "index_add_", "scatter_", "take")


@pytest.fixture(scope="module")
def need_gpu():
    import replay
    replay.need_gpu()


def test_population_reads_use_the_library_gather(need_gpu, monkeypatch):
    import torch
    from gym_rem2d_amd.env import BatchedModular2D
    from gym_rem2d_amd.population import LSystemPopulation
    pop = LSystemPopulation.random(600, np.random.default_rng(5), max_modules=15)
    env = BatchedModular2D()
    env._upload(pop.compile(2), len(pop))
    assert len(env.worlds) > 1
    env.step(40)
    torch.cuda.synchronize()
    want = {}
    for name in ("fitness", "frozen", "steps", "err"):
        parts = [(idx.cpu().numpy(), w.view(name).cpu().numpy()) for w, idx in env.worlds]
        a = np.zeros(len(pop), dtype=parts[0][1].dtype)
        for idx, v in parts:
            a[idx] = v
        want[name] = a

    def refuse(*args, **kwargs):
        raise AssertionError("a population-order read reached a torch indexing op")
    for op in _TORCH_INDEXING:
        monkeypatch.setattr(torch.Tensor, op, refuse)
    got = {"fitness": env.fitness, "frozen": env.frozen, "steps": env.steps, "err": env.errors()}
    monkeypatch.undo()
    for name, v in got.items():
        assert np.array_equal(v.cpu().numpy(), want[name]), name
    assert (want["steps"] == 40).all() and (want["fitness"] != 0).any()
    env.close()


def test_world_gather_checks_its_arguments_and_skips_foreign_indices(need_gpu):
    import torch
    from gym_rem2d_amd import _lib, make_terrain, synthetic
    from gym_rem2d_amd.world import BatchedWorld
    morph = synthetic.chain_population(64, 4, "left")
    w = BatchedWorld(morph.n_envs, morph.lanes, flags=1, device="cuda:0")
    w.set_terrain(make_terrain(4))
    w.reset(morph)
    w.step(3)
    n = morph.n_envs
    out = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    with pytest.raises(_lib.Rem2dError, match="population index"):
        w.gather("steps", out)                        # no rem2d_world_set_outputs yet
    with pytest.raises(ValueError):
        w.gather("fitness", out)                      # f64 field, i32 buffer
    with pytest.raises(_lib.Rem2dError, match="per-creature"):
        _lib.check(w.L.rem2d_world_gather(w.h, _lib.FIELD_ID["px"], out.data_ptr(), n, w._stream()))
    # a reversed order with two indices outside the buffer: those two are skipped, the rest land where the index says
    index = torch.arange(n - 1, -1, -1, dtype=torch.int32, device="cuda:0")
    index[0], index[1] = n + 5, -1
    w.set_outputs(torch.zeros(n, device="cuda:0"), torch.zeros(n, dtype=torch.bool, device="cuda:0"), index)
    w.gather("steps", out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:n - 2] == 3).all() and (got[n - 2:] == -7).all()
    w.close()                                         # (never stepped with that index: the kernels would write through it)
