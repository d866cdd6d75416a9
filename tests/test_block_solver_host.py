"""The populations of tests/block_solver_forge.py exercise what the wave-uniform skip of the 2-point block solve touches -- shown on
the oracle alone, no GPU: tests/test_block_solver_gpu.py compares the kernels with the oracle on exactly these runs.

Over the compared tile-steps of EACH population that lie on the population's code path (block_solver_forge.NC_RANGE: the count of
touching manifolds that puts the tile in pair mode, in classic mode, past the 64 register-resident manifolds):
  * every one of the four patterns of accumulated normal impulses (case 1 .. 4 of the block solve) occurs;
  * a tile-step where every 2-point manifold ends in case 1 (the kernels skip cases 2 .. 4), one where some manifold does not
    (they run them), and one that mixes 1-point and 2-point manifolds (lanes outside the 2-point branch beside lanes in it);
  * `spilled`: among the manifolds beyond the register set (rank >= 64 of the tile's contact map) both a case 1 and another case;
  * `toi`: TOI events occur (the TOI solve's contact_solve_quad runs);
  * nobody is left out (state_forge.left_out; its cap LEFT_OUT_CAP = 2 % of at most 32 creatures is 0).

Measured (python tests/block_solver_forge.py): pair 50 / 3 / 5 / 2 manifolds in cases 1 / 2 / 3 / 4, 8 tile-steps skipped, 7 not;
classic 130 / 11 / 11 / 14, 3 and 12; spilled 196 / 15 / 7 / 6 (rank >= 64: 30 / 2 / 4 / 2), 2 and 11; toi 13 / 2 / 3 / 3, 3 and 6, with
12 TOI events.
"""
import numpy as np
import pytest

import block_solver_forge as B
import state_forge as F


@pytest.mark.parametrize("name", list(B.POPS))
def test_population_exercises_the_block_solver(oracle, name):
    run = B.oracle_run(oracle, name)
    ctx = run["ctx"]
    cov = B.coverage(run)
    print(name, {k: v for k, v in cov.items() if k != "nc"}, "NC", cov["nc"])
    assert len(B.tiles(ctx.morph)) == 1 and ctx.N * ctx.K <= 64            # one 64-lane tile
    assert cov["on_path"] >= 10, cov["nc"]                                  # (most of the 15 tile-steps are on the path)
    if name in ("pair", "classic", "spilled"):
        assert cov["on_path"] == cov["tile_steps"], cov["nc"]
    if name == "pair":
        assert ctx.N == 4 and ctx.K == 16 and max(cov["nc"]) <= 32
    if name == "classic":
        assert ctx.K == 2 and min(cov["nc"]) > 32 and max(cov["nc"]) <= 64
    if name == "spilled":
        assert ctx.K == 2 and min(cov["nc"]) > 64
        assert cov["spilled_cases"][1] > 0 and sum(cov["spilled_cases"][c] for c in (2, 3, 4)) > 0, cov["spilled_cases"]
    if name == "toi":
        assert int((run["steps"][-1]["toievents"] - run["settled"]["toievents"]).sum()) > 0
    assert all(cov["cases"][c] > 0 for c in (1, 2, 3, 4)), cov["cases"]
    assert cov["skipped"] > 0 and cov["fallback"] > 0 and cov["mixed"] > 0, cov
    assert B.N_STEPS == F.N_STEPS   # (state_forge.left_out's "never" is its own N_STEPS)
    first, _ = F.left_out(run)
    gone = int((first < B.N_STEPS).sum())
    assert gone <= int(F.LEFT_OUT_CAP * ctx.N), gone


def test_patterns_are_told_apart():
    """The reading of the four patterns on a hand-made snapshot (no oracle)."""
    snap = {f: np.zeros((2, 1, 1), np.float32 if f in F.CONTACT_F else np.int32) for f in F.SLOT_FIELDS}
    snap["ccount"] = np.array([[1]], np.int32)
    snap["cedge"][0], snap["cnpt"][0], snap["ckey0"][0], snap["ckey1"][0] = 7, 2, 11, 12
    rec = (0, 0, 0, 7, 11, 12, 0.1)
    for (n0, n1), case in (((1.0, 2.0), 1), ((1.0, 0.0), 2), ((0.0, 2.0), 3), ((0.0, 0.0), 4)):
        snap["cn0"][0], snap["cn1"][0] = n0, n1
        assert B._case_after(snap, rec) == case
    assert B._case_after(snap, (0, 0, 0, 7, 11, 13, 0.1)) is None      # (another feature key: not the same manifold)
    snap["cnpt"][0] = 1
    assert B._case_after(snap, rec) is None
