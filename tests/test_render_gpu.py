"""The renderer on the GPU (pytest -m gpu): rem2d_world_render against the numpy pixel model (tests/render_model.py) with
np.array_equal, on the right creature of a split / compacted population, without touching the state, and run_ea's show_best."""
import random

import numpy as np
import pytest

from env_harness import _compare

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def need_gpu():
    import replay
    replay.need_gpu()


@pytest.fixture(scope="module")
def sincosf(need_gpu):
    from oracle import oracle as O
    O.build()
    return O.sincosf


def _trees(n, seed0=0, depth=4):
    """n direct-encoding trees (boxes and circles) and their module lists."""
    from gym_rem2d_amd import get_module_list
    from gym_rem2d_amd.encodings import DirectEncoding
    trees, lists = [], []
    for k in range(n):
        random.seed(seed0 + k)
        ml = get_module_list()
        trees.append(DirectEncoding(ml).create(depth))
        lists.append(ml)
    return trees, lists


def _env(kind, terrain="default", n=None, **kw):
    from gym_rem2d_amd import synthetic
    from gym_rem2d_amd.env import BatchedModular2D
    env = BatchedModular2D(hardcore=terrain == "hardcore", flat=terrain == "flat", **kw)
    if kind == "lsystem":
        env.reset_specs(synthetic.lsystem_specs(range(n or 256)))
    elif kind == "direct":
        trees, lists = _trees(n or 64)
        env.reset(trees, lists)
    elif kind == "chain8":
        env.reset_morphology(synthetic.chain_population(n or 128, 8, "left"))
    return env


@pytest.mark.parametrize("kind,terrain", [("lsystem", "default"), ("direct", "hardcore"), ("chain8", "flat"),
                                          ("lsystem", "hardcore"), ("direct", "default")])
def test_kernel_equals_model(need_gpu, sincosf, kind, terrain):
    env = _env(kind, terrain)
    n = env.n_envs
    rng = np.random.default_rng(1)
    sample = sorted(set(rng.choice(n, 5, replace=False).tolist()) | {0, n - 1})
    wide = sorted(set(rng.choice(n, min(n, 24), replace=False).tolist()))
    for steps, after in ((0, 0), (37, 37), (463, 500)):
        if steps:
            env.step(steps)
        _compare(env, sample, 800, 600, sincosf)
        _compare(env, list(range(n)) if after == 37 else wide, 173, 97, sincosf)   # (every creature once)
    # a camera of its own: far to the left and below the terrain (negative coordinates), and one over the flag
    cams = np.array([[-30.0, -12.5]] * 2 + [[0.0, 3.0]] * 2, np.float32)
    _compare(env, [0, 1, n - 2, n - 1], 173, 97, sincosf, cam=cams)
    env.close()


def test_explicit_colour_tables(need_gpu, sincosf):
    import torch
    env = _env("chain8", "default", n=64)
    env.step(37)
    w = env.worlds[0][0]
    g = torch.Generator().manual_seed(2)
    fill = torch.randint(0, 256, (w.n_envs, w.lanes, 3), dtype=torch.uint8, generator=g).cuda()
    line = torch.randint(0, 256, (w.n_envs, w.lanes, 3), dtype=torch.uint8, generator=g).cuda()
    _compare(env, [0, 5, 63], 800, 600, sincosf, fill=fill, line=line)
    _compare(env, list(range(64)), 173, 97, sincosf, fill=fill, line=line)
    env.close()


def test_direct_population_has_circles(need_gpu):
    env = _env("direct", "default")
    assert sum(int((w.view("shape") == 2).sum()) for w, _ in env.worlds) > 0
    env.close()


def test_rendering_changes_nothing(need_gpu):
    import torch
    a, b = _env("lsystem", "default", n=128), _env("lsystem", "default", n=128)
    for env in (a, b):
        env.step(13)
    before = [w.arena.clone() for w, _ in a.worlds]
    a.render(width=173, height=97)
    a.render([3, 7], width=800, height=600)
    torch.cuda.synchronize()
    for (w, _), snap in zip(a.worlds, before):
        assert torch.equal(w.arena, snap)
    for _ in range(6):
        a.step(5)
        a.render(list(range(0, 128, 3)), width=64, height=48)
        b.step(5)
    for (wa, _), (wb, _) in zip(a.worlds, b.worlds):
        assert torch.equal(wa.arena, wb.arena)
    assert torch.equal(a.fitness, b.fitness)
    a.close()
    b.close()


def _single(spec_or_tree, ml=None, steps=0, terrain="default"):
    from gym_rem2d_amd.env import BatchedModular2D
    env = BatchedModular2D(hardcore=terrain == "hardcore")
    if ml is None:
        env.reset_specs([spec_or_tree])
    else:
        env.reset([spec_or_tree], [ml])
    if steps:
        env.step(steps)
    return env


def test_right_creature_across_buckets_groups_and_compact(need_gpu):
    """A mixed population split over lane buckets and step groups, then compacted: every image equals the one a 1-creature env of
    the same creature draws at the same step, under the same camera."""
    import torch
    from gym_rem2d_amd import _lib, synthetic
    from gym_rem2d_amd.env import BatchedModular2D
    specs = synthetic.lsystem_specs(range(96))
    env = BatchedModular2D(flags=_lib.FLAG_CONTINUOUS | _lib.FLAG_SKIP_FROZEN)
    env.step_groups = 3
    env.reset_specs(specs)
    assert len({w.lanes for w, _ in env.worlds}) >= 2 and len(env.groups) >= 2
    rng = np.random.default_rng(4)
    pick = sorted(rng.choice(96, 10, replace=False).tolist())
    cam = torch.tensor([[3.0, 1.0]] * len(pick), dtype=torch.float32)
    env.step(40)
    got = env.render(pick, width=173, height=97, camera=cam).cpu().numpy()
    for k, c in enumerate(pick):
        one = _single(specs[c], steps=40)
        want = one.render([0], width=173, height=97, camera=cam[:1]).cpu().numpy()[0]
        one.close()
        assert np.array_equal(got[k], want), c
    # compact() every bucket down to its open creatures (min_envs=0, max_alive=1: whatever is left)
    env.step(110)
    alive = env.compact(min_envs=0, max_alive=1.0)
    assert env._compacted
    frozen = env.frozen.cpu().numpy()
    open_ = [c for c in range(96) if frozen[c] == 0]
    assert alive == len(open_) > 0
    pick = open_[:6] + open_[-3:]
    got = env.render(pick, width=173, height=97, camera=cam[:1].expand(len(pick), 2)).cpu().numpy()
    for k, c in enumerate(pick):
        one = _single(specs[c], steps=150)
        want = one.render([0], width=173, height=97, camera=cam[:1]).cpu().numpy()[0]
        one.close()
        assert np.array_equal(got[k], want), c
    gone = [c for c in range(96) if frozen[c] != 0]
    if gone:
        with pytest.raises(ValueError):
            env.render([gone[0]], width=8, height=8)
    env.close()


def test_refusals(need_gpu):
    import ctypes as C
    import torch
    from gym_rem2d_amd import _lib
    env = _env("chain8", "default", n=16)
    with pytest.raises(IndexError):
        env.render([16])
    with pytest.raises(IndexError):
        env.render([-1])
    for wh in ((0, 10), (10, 0), (_lib.RENDER_MAX_SIZE + 1, 4), (4, _lib.RENDER_MAX_SIZE + 1)):
        with pytest.raises(ValueError):
            env.render([0], width=wh[0], height=wh[1])
    with pytest.raises(NotImplementedError):
        env.render(mode="human")
    # the C entry point checks on its own: a bad index or size is REM2D_E_INVALID with a message, nothing is launched
    w = env.worlds[0][0]
    idx = torch.tensor([0, 16], dtype=torch.int32, device="cuda")
    cam = torch.zeros((2, 2), dtype=torch.float32, device="cuda")
    out = torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device="cuda")
    rc = w.L.rem2d_world_render(w.h, idx.data_ptr(), 2, cam.data_ptr(), None, None, 4, 4, out.data_ptr(), w._stream())
    assert rc == -1 and b"creature index 16" in w.L.rem2d_last_error()
    rc = w.L.rem2d_world_render(w.h, idx.data_ptr(), 1, cam.data_ptr(), None, None, 0, 4, out.data_ptr(), w._stream())
    assert rc == -1 and b"width and height" in w.L.rem2d_last_error()
    torch.cuda.synchronize()
    assert int(out.sum()) == 0
    env.close()


def test_record_frames_follows_the_reference_camera(need_gpu):
    """record_frames: the frames before steps 0, 5, 10, ... under the reference's scroll, which it updates every step."""
    import torch
    from gym_rem2d_amd import render as R
    env = _env("chain8", "default", n=4)
    twin = _env("chain8", "default", n=4)
    cam = R.ReferenceCamera(2, "cuda")
    got = list(R.record_frames(env, 23, [1, 2], every=5, width=96, height=64, chunk=2, stop_when_frozen=False))
    assert [s for s, _ in got] == [0, 5, 10, 15, 20, 23]
    t = 0
    for s, frames in got:
        while t < s:
            twin.step(1)
            p = R.root_poses(twin, [1, 2])
            cam.update(p[:, 0], p[:, 1])
            t += 1
        want = twin.render([1, 2], width=96, height=64, camera=cam).cpu().numpy()
        assert frames.shape == (2, 64, 96, 3) and np.array_equal(frames, want), s
    env.close()
    twin.close()


def test_run_ea_show_best(need_gpu, tmp_path):
    from gym_rem2d_amd import ea
    logged = []
    random.seed(11)
    pop, hist = ea.run_ea(ea.make_config(population_size=16, encoding="direct"), seed=11, n_generations=1, log=logged.append,
                          show_best=True, interval=5, frames_dir=str(tmp_path))
    (gen, fit, n_frames), = ea.run_ea.last_show_best
    assert gen == 0 and n_frames >= 1
    assert fit == hist[0][2] == max(ind.fitness for ind in pop)
    line = [s for s in logged if s.startswith("Fitness of best =")]
    assert len(line) == 1 and float(line[0].split("=")[1]) == hist[0][2]
    files = sorted((tmp_path / "gen0").iterdir())
    assert len(files) == n_frames and files[0].name == "frame00000.png"
    from PIL import Image
    im = np.asarray(Image.open(files[0]))
    assert im.shape == (600, 800, 3) and im.dtype == np.uint8
