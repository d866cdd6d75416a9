"""Episode loop and population evaluation.

``evaluate`` has the reference's signature and fitness rule (``REM2D_main.py:350-378`` ==
``Demo1_Random_Individual.py:4-36``).  ``evaluate_population`` replaces
``pool.map(evaluate, population)`` (``REM2D_main.py:256-267,291``) with one batched episode on
the GPU; ``evaluate_population_sharded`` shards the population over the ranks of a
torch.distributed job (one process per GPU, contiguous blocks) and gathers the fitness with a
single all-gather -- RCCL over xGMI on the MI355X node, gloo in the CPU tests.  There is no
per-step collective: creatures are independent.
"""
import collections
import math

import numpy as np
import torch

from . import _lib

EPISODE_CAP = 2500  # wall of death advances 0.04/step and the goal is x > 100
# the flags of an evaluation env: fitness is all that leaves it, and creatures whose fitness is final need no more steps
EVAL_FLAGS = _lib.FLAG_CONTINUOUS | _lib.FLAG_SKIP_FROZEN

# What an episode found (run_episode_masked builds it once, at its end; ``BatchedModular2D.last_episode`` keeps it until the next
# upload).  codes: int32 [N], the creatures' final REM2D_ERR_* bits (of the wide run where there was one: what SolverOverflow
# reports for the creatures still unresolved); handover: sorted population indices re-run on per-step launches; overflow: indices
# that needed the wide build; unresolved: indices without a valid fitness after every fallback.
EpisodeReport = collections.namedtuple("EpisodeReport", "codes handover overflow unresolved")


def _env_singleton():
    global _ENV
    try:
        return _ENV
    except NameError:
        from .env import Modular2D
        _ENV = Modular2D()
        return _ENV


def evaluate(individual, EVALUATION_STEPS=10000, HEADLESS=True, INTERVAL=100, ENV_LENGTH=100, TREE_DEPTH=None,
             CONTROLLER=None):
    """One individual, one episode, reference semantics (action ignored, reward sentinels)."""
    env = _env_singleton()
    if TREE_DEPTH is None:
        try:
            TREE_DEPTH = individual.tree_depth
        except AttributeError:
            raise Exception("Tree depth not defined in evaluation")
    tree = individual.genome.create(TREE_DEPTH)
    env.seed(4)
    env.reset(tree=tree, module_list=individual.genome.moduleList)
    fitness = 0
    for i in range(EVALUATION_STEPS):
        action = np.ones_like(env.action_space.sample())
        _, reward, done, _ = env.step(action)
        if reward < -10:
            break
        elif reward > ENV_LENGTH:
            reward += (EVALUATION_STEPS - i) / EVALUATION_STEPS
            fitness = reward
            break
        if reward > 0:
            fitness = reward
    return fitness


class SolverOverflow(_lib.Rem2dError):
    """A creature ran out of engine capacity during an episode, so its trajectory is NOT what the reference's Box2D
    computes: more than REM2D_SOLVER_SLOTS touching contacts on one body (the extra manifold was left out of the solver)
    or more than REM2D_CONTACT_SLOTS broadphase pairs on one body (the extra pair was never created).
    ``indices`` are the affected population indices, ``codes`` their REM2D_ERR_* bits."""

    def __init__(self, indices, codes):
        self.indices, self.codes = indices, codes
        super().__init__("%d creature(s) overflowed the solver / pair slots (first: %s, REM2D_ERR bits %s); their fitness "
                         "is not the reference's" % (len(indices), indices[:8], sorted(set(codes))))


HandoverError = _lib.HandoverError   # (the step train's hand-over check: a launch-form failure, not a capacity one -- see _lib)

# What a creature gets whose contacts did not fit even the wide build (run_episode's on_error="penalty"): the value
# evaluate() starts from and returns for an individual that never scored (REM2D_main.py:361 ``fitness = 0``).  Box2D has
# no contact cap (Modular2DEnv.py:634), the engine here has two tiers (24 / 6, then 32 / 12 pair / solver slots per body);
# DESIGN.md 8 shows that no module the reference's classes can produce (boxes <= 1 x 1, circles r <= 0.5: limitWH,
# simple_module.py:55-68) reaches the second tier's limits, so this is the verdict on hand-built out-of-domain bodies --
# an EA generation records the mask and goes on instead of raising.
UNRESOLVED_FITNESS = 0.0


def check_errors(env, on_error="raise"):
    """Read the per-creature engine error bits of a BatchedModular2D.  REM2D_ERR_HANDOVER (the step train's hand-over check) is a
    launch-form failure and is judged first and apart: "raise" and "warn" both raise HandoverError for it (no mode scores such a
    creature), "ignore" returns it in the mask.  The capacity bits (REM2D_ERR_PAIR_OVERFLOW / _SOLVER_OVERFLOW) -- on_error:
    "raise" -> SolverOverflow with the creatures' real codes; "warn" -> warnings.warn and return the mask; "ignore" -> return the
    mask (every non-zero code)."""
    return judge_errors(env.errors(), on_error)


def judge_errors(err, on_error="raise"):
    """check_errors' verdict on REM2D_ERR_* codes already read (int32 [N]; run_stream: ``stream.err``, indexed by id)."""
    bad = err != 0
    if on_error != "ignore" and bool(bad.any()):
        hand = (err & _lib.ERR_HANDOVER) != 0
        if bool(hand.any()):
            raise HandoverError(int(hand.sum()), " (creatures, first: %s)" % torch.nonzero(hand).flatten().cpu().tolist()[:8])
        idx = torch.nonzero(bad).flatten().cpu().tolist()
        codes = err[bad].cpu().tolist()
        if on_error == "raise":
            raise SolverOverflow(idx, codes)
        import warnings
        warnings.warn(str(SolverOverflow(idx, codes)))
    return bad


def _episode(env, max_steps, chunk, compact, step=None):
    step = env.step if step is None else step
    done_steps = 0
    compact = compact and bool(env.flags & _lib.FLAG_SKIP_FROZEN)
    while done_steps < max_steps:
        n = min(chunk, max_steps - done_steps)
        step(n)
        done_steps += n
        if compact:
            if env.compact() == 0:
                break
        elif bool((env.frozen != 0).all()):
            break


def _replay_env(env, uploaded, ids, wide, options):
    """A fresh BatchedModular2D that holds, reset, exactly the creatures ``ids`` (a sorted array) of ``uploaded`` ([(Morphology, ids)]
    as reset_batches takes them), creature ``ids[i]`` at index i: ``env``'s terrain, seed, flags and device, the build ``wide``, its
    launch options with ``options`` on top, on_handover="flag".  The caller closes it."""
    from .env import BatchedModular2D
    opts = dict(env.options)
    opts.pop("train_fault", None)   # (a test hook of the first run's launch form; the second run is there to be trusted)
    opts.update(options or {})
    again = BatchedModular2D(hardcore=env.hardcore, flat=env.flat, seed=env._seed, device=env.device, flags=env.flags,
                             wide=wide, options=opts, on_handover="flag")
    again.terrain = env._terrain()
    batches = []
    for morph, idx in uploaded:
        sel = np.nonzero(np.isin(idx, ids))[0]
        if sel.size:
            batches.append((morph.take(sel), np.searchsorted(ids, idx[sel]).tolist()))
    again.reset_batches(batches, int(ids.size))
    return again


def reevaluate(env, mask, fit, wide=None, options=None, max_steps=EPISODE_CAP, chunk=100):
    """Creatures are independent and an episode is a function of the morphology alone (fixed terrain seed, open-loop controller:
    SURVEY facts 5 / 6), so any subset can simply be evaluated AGAIN from reset in worlds of another build or launch form -- same
    kernels, same arithmetic, same bits for everything both forms can hold.  ``mask``: bool [N] in population order; wide / options:
    the build (None: the env's own) and launch options of the second run.  Writes the fitness of those creatures into ``fit`` and
    returns their REM2D_ERR_* codes of the second run as int32 [N] (0 elsewhere).  Two callers:
      * the overflow fallback (``reevaluate_wide``): Box2D has no cap on the contacts of a body (Modular2DEnv.py:634 world.Step
        solves whatever touches); the default build keeps 24 pair / 6 solver slots per body and flags the creature that needs
        more -- re-run in librem2d_wide.so (32 / 12);
      * the hand-over fallback: creatures a step train flagged REM2D_ERR_HANDOVER -- re-run in the SAME build on per-step launches
        (``options={"fuse_velpost": 1}``: no hand-over between workgroups exists there)."""
    idx_bad = torch.nonzero(mask).flatten().cpu().numpy()
    codes = torch.zeros(mask.shape, dtype=torch.int32, device=mask.device)
    if idx_bad.size == 0:
        return codes
    again = _replay_env(env, env._uploaded, idx_bad, env.wide if wide is None else wide, options)
    _episode(again, max_steps, chunk, compact=False)
    where = torch.as_tensor(idx_bad, dtype=torch.long, device=fit.device)
    fit.index_copy_(0, where, again.fitness.to(fit.device))
    codes.index_copy_(0, where.to(codes.device), again.errors().to(codes.device))
    again.close()
    return codes


def reevaluate_wide(env, bad, fit, handover, max_steps=EPISODE_CAP, chunk=100):
    """The overflow fallback (see ``reevaluate``): the creatures of ``bad`` again, from reset, in the wide build.  Writes their
    fitness into ``fit`` and returns the REM2D_ERR_* codes [N] of the wide run (0 elsewhere): non-zero = overflowed even there."""
    return _resolve_handover(env, reevaluate(env, bad, fit, wide=True, max_steps=max_steps, chunk=chunk), fit, True, handover,
                             max_steps, chunk)


def _resolve_handover(env, err, fit, wide, handover, max_steps, chunk):
    """``err``: REM2D_ERR_* codes [N] of a run in the env's own (wide=None) or the wide build.  The creatures that carry
    REM2D_ERR_HANDOVER are evaluated again on per-step launches of that build; returns the codes with theirs replaced by the second
    run's, and adds their population indices to the set ``handover``.  A hand-over bit that survives per-step launches cannot
    exist (they have no hand-over); if it does, HandoverError."""
    hand = (err & _lib.ERR_HANDOVER) != 0
    if not bool(hand.any()):
        return err
    idx = torch.nonzero(hand).flatten().cpu().tolist()
    handover.update(idx)
    import warnings
    warnings.warn("%d creature(s) were flagged REM2D_ERR_HANDOVER by a step train launch (first: %s): evaluating them again on "
                  "per-step launches" % (len(idx), idx[:8]))
    again = reevaluate(env, hand, fit, wide=wide, options={"fuse_velpost": 1}, max_steps=max_steps, chunk=chunk)
    if bool(((again & _lib.ERR_HANDOVER) != 0).any()):
        raise HandoverError(int(((again & _lib.ERR_HANDOVER) != 0).sum()), " even on per-step launches")
    return torch.where(hand, again, err)


def run_episode_masked(env, max_steps=EPISODE_CAP, chunk=100, compact=True, fallback=True):
    """run_episode without the verdict: (fitness [N] float64, unresolved [N] bool).  ``unresolved`` marks the creatures
    whose fitness is NOT what the reference's Box2D computes: they overflowed the default build's contact capacity and
    (with ``fallback``) the wide build's as well.  Never raises on overflow -- what a sharded job calls before its
    collective (a rank that raised here would leave the others waiting in the all-gather).
    Creatures a step train flagged REM2D_ERR_HANDOVER are ALWAYS resolved here (whatever ``fallback`` says): evaluated again on
    per-step launches of the same build, never sent to the wide build for it, never penalised.  What the episode found is left
    in ``env.last_episode`` (EpisodeReport)."""
    policy, env.on_handover = env.on_handover, "flag"   # (the episode goes on for everybody else; the flagged ones are dealt with below)
    try:
        _episode(env, max_steps, chunk, compact)
        fit = env.fitness.clone()
        err = env.errors().to(torch.int32)
    finally:
        env.on_handover = policy
    handover = set()
    # (the counter is read and cleared without a synchronisation before it, and a count above 0 with no flagged creature is
    # dropped here: kept exactly as it was -- ADVICE.md's finding on this line is a change of behaviour and not made here)
    if env.handover_failures(clear=True) or bool(((err & _lib.ERR_HANDOVER) != 0).any()):
        err = _resolve_handover(env, err, fit, None, handover, max_steps, chunk)
    bad = (err & _lib.ERR_CAPACITY) != 0
    overflow = torch.nonzero(bad).flatten().cpu().tolist()   # population indices that needed the fallback
    if fallback and bool(bad.any()):
        err = reevaluate_wide(env, bad, fit, handover, max_steps, chunk)
        bad = err != 0
    env.last_episode = EpisodeReport(err, sorted(handover), overflow, torch.nonzero(bad).flatten().cpu().tolist())
    return fit, bad


def apply_penalty(fit, bad, warn=True):
    """The defined verdict on creatures without a valid fitness (``bad``: bool mask): UNRESOLVED_FITNESS, in place, with a
    warning that names them.  Returns their indices."""
    idx = torch.nonzero(torch.as_tensor(bad)).flatten().cpu().tolist()
    if idx:
        fit[torch.as_tensor(idx, dtype=torch.long, device=fit.device)] = UNRESOLVED_FITNESS
        if warn:
            import warnings
            warnings.warn("%d creature(s) overflowed even the wide build's contact capacity (first: %s): fitness set to "
                          "UNRESOLVED_FITNESS = %s" % (len(idx), idx[:8], UNRESOLVED_FITNESS))
    return idx


def run_episode(env, max_steps=EPISODE_CAP, chunk=100, on_error="fallback", compact=True):
    """Advance a BatchedModular2D until every creature's fitness is final (or max_steps).
    Returns fitness[N] (float64 tensor on the env's device).  Engine overflows (see SolverOverflow) are not silent and,
    by default, not fatal: on_error="fallback" re-evaluates the flagged creatures in the wide build (reevaluate_wide) so
    that every individual gets the fitness Box2D would give, and raises only for creatures that overflow even that;
    on_error="penalty" (what the EA loops use) does the same but never raises: a creature beyond the wide build gets
    UNRESOLVED_FITNESS, a warning names it and ``env.last_episode.unresolved`` lists it;
    "raise" / "warn" / "ignore" judge the default build's flags without a second attempt (and leave no report:
    ``env.last_episode`` is None after them).  compact: in worlds created
    with REM2D_FLAG_SKIP_FROZEN (the bodies of finished creatures are nobody's business any more) the survivors are
    moved into smaller worlds between chunks once most of a world has finished (BatchedModular2D.compact) -- same
    fitness, a shorter episode."""
    if on_error in ("penalty", "fallback"):
        fit, bad = run_episode_masked(env, max_steps, chunk, compact, fallback=True)
        if on_error == "penalty":
            apply_penalty(fit, bad)
        elif bool(bad.any()):
            report = env.last_episode
            raise SolverOverflow(report.unresolved, report.codes[bad].cpu().tolist())   # (the creatures' real REM2D_ERR_* bits of the wide run)
        return fit
    env.last_episode = None
    _episode(env, max_steps, chunk, compact)
    check_errors(env, on_error)   # (REM2D_ERR_HANDOVER raises HandoverError in "raise" and "warn"; so does env.fitness below)
    return env.fitness.clone()


def _strict_on_error(on_error):
    """The episodes of device policies have no second attempt: on_error is one of check_errors' three modes"""
    if on_error not in ("raise", "warn", "ignore"):
        raise ValueError("on_error must be 'raise', 'warn' or 'ignore', not %r" % (on_error,))


def run_policy_episode(env, max_steps=EPISODE_CAP, chunk=100, compact=True, on_error="raise", normalizer=None):
    """run_episode for a BatchedModular2D with a device policy attached (``env.set_policy``): the same episode loop, every step
    preceded by the policy's control step (``env.step_policy``), chunks of ``chunk`` steps queued without a synchronisation in
    between.  Returns fitness[N] (float64 tensor on the env's device).  on_error: "raise" | "warn" | "ignore", judged by
    ``check_errors`` on the default build's flags.  There is no second attempt here: replaying the flagged creatures from reset in
    the wide build, as run_episode's fallback does for open-loop creatures, is not built for policies yet -- construct the env
    with wide=True where creatures may outgrow the default build's contact slots.  ``env.last_episode`` is None afterwards.
    ``normalizer``: a ``policy.ObsNormalizer`` that is only APPLIED: the env's policy is attached again under it with ``accumulate=False`` (its tables as they stand; its sums are
    not touched).  Without it the env runs as ``set_policy`` left it, a normaliser attached there included."""
    _strict_on_error(on_error)
    if env.policy is None:
        raise ValueError("run_policy_episode: the env has no policy (set_policy first)")
    if normalizer is not None:
        env.set_policy(env.policy, normalizer=normalizer, accumulate=False)
    env.last_episode = None
    _episode(env, max_steps, chunk, compact, step=env.step_policy)
    check_errors(env, on_error)
    return env.fitness.clone()


# ---- the generational loops of device policies: one driver; a loop keeps its checks, its buffers and its two steps
def _fitness_row(fit, *more):
    """(min, max, mean) of the fitness and ``more`` float64 scalars on the device: one read, the only numbers that leave it"""
    return tuple(torch.stack((fit.min(), fit.max(), fit.mean()) + more).cpu().tolist())


def _generations(env, first, n_generations, produce, episode, update, on_generation, log, normalizer=None, reset_first=False,
                 rows_from=1, row=_fitness_row, text="Generation %d : Min %s, Max %s, Avg %s"):
    """Generations ``first`` (0 or 1) .. n_generations of a search loop.  Every one is ``produce(gen)`` -> the policy to run;
    ``normalizer.freeze()`` (one set of tables per generation: every child sees the same) and ``env.set_policy``;
    ``env.reset_where`` of everyone, except in generation 0, which runs the population as the caller reset it; ``episode()`` ->
    ``(fitness, ...)``; ``update(gen, that policy, fitness, ...)`` -> what ``on_generation`` is told after ``gen``; from generation
    ``rows_from`` on the history row ``(gen,) + row(fitness)`` and, after ``on_generation``, the ``log`` line ``text % row``.
    ``reset_first``: reset_where comes before freeze / set_policy instead of after.  The order is part of the launch arguments:
    set_policy clears the env's note that a reset happened and reset_where sets it, so it decides whether a RecurrentPolicy's
    first act() is handed a reset mask (the context words are zero either way).  Returns ``(fitness, history)`` of the last
    generation run."""
    everyone = torch.ones(env.n_envs, dtype=torch.uint8, device=env.worlds[0][0].device) if env.worlds else None
    fit, history = None, []
    for gen in range(first, int(n_generations) + 1):
        running = produce(gen)
        if gen and reset_first:
            env.reset_where(mask=everyone)
        if normalizer is not None:
            normalizer.freeze()
        env.set_policy(running, normalizer=normalizer)
        if gen and not reset_first:
            env.reset_where(mask=everyone)
        fit, *seen = episode()
        told = update(gen, running, fit, *seen)
        if gen >= rows_from:
            history.append((gen,) + row(fit))
        if on_generation:
            on_generation(gen, *told)
        if log and gen >= rows_from:
            log(text % history[-1])
    return fit, history


def _policy_episode(env, max_steps, chunk, on_error):
    """A loop's episode without a descriptor.  (compact=False: compaction would drop the device morphology the next reset needs)"""
    return lambda: (run_policy_episode(env, max_steps, chunk, compact=False, on_error=on_error),)


def _behaviour_episode(env, period, samples, max_steps, on_error):
    """A loop's episode with a descriptor -> (fitness, behaviour)"""
    return lambda: run_behaviour_episode(env, period, samples, max_steps=max_steps, on_error=on_error)


def _population(what, env, described=False):
    """The population a loop needs in place -> how many creatures; ``described``: one whose descriptors can be recorded"""
    if not env.worlds:
        raise ValueError("%s: no population in place (reset first)" % what)
    if described and (env._autoreset is not None or env._stream_rec is not None):
        raise ValueError("%s: descriptors are not recorded under auto-reset or streaming" % what)
    return env.n_envs


def _es_groups(what, n, mean, group_size):
    """-> S, the children per mean of run_policy_es and run_policy_nses"""
    S = n if group_size is None else int(group_size)
    if S < 2 or S % 2 or n % S or mean.n_sets * S != n:
        raise ValueError("%s: %d creatures are not %d means times an even group_size (%r)" % (what, n, mean.n_sets, group_size))
    return S


def _period(period, samples, max_steps):
    """The steps between two samples of a loop's descriptor; default: max_steps over samples, rounded up"""
    return -(-int(max_steps) // samples) if period is None else int(period)


def _archive_fits(what, env, archive, n_blocks, samples):
    """The novelty archive of a loop: its shape, then its device -> the env's device"""
    if archive.n_blocks != n_blocks or archive.width != 2 * samples:
        raise ValueError("%s: the archive must have %d blocks of width %d, not %d of %d"
                         % (what, n_blocks, 2 * samples, archive.n_blocks, archive.width))
    dev = env.worlds[0][0].device
    if archive.device != dev:
        raise ValueError("%s: the archive must be on %s, not %s" % (what, dev, archive.device))
    return dev


def _es_scratch(mean, group_size, dev):
    """The scratch tensor es_update asks for, or None where the update is one launch"""
    need = mean.es_scratch_bytes(group_size)
    return torch.empty(need // 8, dtype=torch.int64, device=dev) if need else None


def run_policy_generations(env, policy, n_generations, seed=0, rate=0.05, sigma=0.1, tournsize=4, group_size=None, elite=0,
                           max_steps=EPISODE_CAP, chunk=100, on_error="raise", log=None, on_generation=None,
                           normalizer=None):
    """population.run_generations for device policies: the generational loop of run2D.run_deap (REM2D_main.py:280-298) with the
    population -- the weight sets of ``policy``, one per creature of ``env`` (reset first) -- on the device throughout.  Generation
    0's episode runs first; every generation is then ``policy.evolve`` (generation g = 1 .., this ``seed``), ``env.set_policy``,
    ``env.reset_where`` of everyone and ``run_policy_episode(compact=False)`` -- compaction would drop the device morphology the
    reset needs.  The generations from 1 on use two sets of weight buffers in turn; ``policy`` itself is never written.  Returns ``(policy, fitness, history)``: the last generation, its
    fitness (float64 [N] on the device) and rows ``(gen, min, max, mean)``, the only numbers that leave the device.
    ``on_generation(gen, policy, fitness)``, if given, is called after every episode, generation 0's included, with the tensors
    themselves (a checkpoint hook: clone what must last, the weight buffers are overwritten two generations later).  The creatures
    do not change: group_size names the blocks of consecutive creatures whose policies compete (those of one morphology).
    ``normalizer``: a ``policy.ObsNormalizer`` whose blocks cover the creatures: every generation starts with its ``freeze()`` -- within
    a generation every child sees the same tables -- and the generation's episodes add what they observe to its sums."""
    spare = last = None

    def child(gen):
        nonlocal policy, spare
        if gen:
            new = policy.evolve(last, gen, seed=seed, rate=rate, sigma=sigma, tournsize=tournsize, group_size=group_size, elite=elite,
                                out=spare)
            spare, policy = (policy if gen > 1 else None), new    # (generation 0's buffers are the caller's: never written)
        return policy

    def scored(gen, attached, fit):
        nonlocal policy, last
        if not gen:
            policy = env.policy      # (the caller's, on the env's device)
        last = fit
        return policy, fit
    fit, history = _generations(env, 0, n_generations, child, _policy_episode(env, max_steps, chunk, on_error), scored, on_generation, log,
                                normalizer=normalizer)
    return policy, fit, history


def run_policy_es(env, mean, n_generations, seed=0, sigma=0.1, lr=0.05, group_size=None, max_steps=EPISODE_CAP, chunk=100,
                  on_error="raise", log=None, on_generation=None,
                  normalizer=None):
    """An evolution strategy for device policies: ``mean`` holds one controller per block of ``group_size`` = S consecutive
    creatures of ``env`` (reset first; the creatures of a block share a morphology, or are whatever the caller wants ranked
    together; default: one block of everyone), M = n_envs / S sets in all.  Every generation g = 1 .. is ``mean.es_sample`` (the
    S children of every mean, antithetic pairs, this ``seed``), ``env.set_policy``, ``env.reset_where`` of everyone,
    ``run_policy_episode(compact=False)`` -- compaction would drop the device morphology the reset needs -- and ``es_update``:
    centred ranks of the fitness within each block, the mean moved by ``lr / (S sigma)`` times the rank-weighted noise
    (include/rem2d_es.h).  One child policy, two sets of mean buffers, one util and one scratch tensor are reused throughout;
    ``mean`` itself is never written.  Returns ``(mean, fitness, history)``: the mean after the last update, the last generation's
    fitness (float64 [N] on the device) and rows ``(gen, min, max, mean)``, the only numbers that leave the device.
    ``on_generation(gen, children, fitness, mean)``, if given, is called after every update with the tensors themselves and the
    NEW mean (a checkpoint hook: clone what must last, every buffer is overwritten one or two generations later).
    ``normalizer``: a ``policy.ObsNormalizer`` whose blocks cover the creatures: every generation starts with its ``freeze()`` -- within
    a generation every child sees the same tables -- and the generation's episodes add what they observe to its sums."""
    n = _population("run_policy_es", env)
    S = _es_groups("run_policy_es", n, mean, group_size)
    dev = env.worlds[0][0].device
    mean = mean.to(dev)
    children = spare = None
    scratch = _es_scratch(mean, S, dev)

    def sample(gen):
        nonlocal children
        children = mean.es_sample(gen, seed=seed, sigma=sigma, group_size=S, out=children)
        return children

    def update(gen, children, fit):
        nonlocal mean, spare
        new = mean.es_update(fit, gen, seed=seed, sigma=sigma, lr=lr, group_size=S, out=spare, scratch=scratch)
        spare, mean = (mean if gen > 1 else None), new      # (the first mean's buffers are the caller's: never written)
        return children, fit, mean
    fit, history = _generations(env, 1, n_generations, sample, _policy_episode(env, max_steps, chunk, on_error), update, on_generation, log,
                                normalizer=normalizer)
    return mean, fit, history


def run_policy_snes(env, es, n_generations, seed=0, max_steps=EPISODE_CAP, chunk=100, on_error="raise", log=None, on_generation=None,
                    normalizer=None):
    """``run_policy_es`` around a ``policy.SeparableES`` (per-parameter sigma, Adam on request; include/rem2d_snes.h): ``es`` holds one
    mean per block of ``es.group_size`` consecutive creatures of ``env`` (reset first).  Every generation g = 1 .. is ``es.sample``,
    ``env.set_policy``, ``env.reset_where`` of everyone, ``run_policy_episode(compact=False)`` and ``es.update``.  The strategy's own
    buffers are reused throughout: after the first generation nothing is allocated.  Returns ``(mean, fitness, history)`` as
    ``run_policy_es`` does; ``on_generation(gen, children, fitness, mean)`` likewise (``es.sigma``, ``es.t`` and ``es.state()`` are
    there for a checkpoint hook).
    ``normalizer``: a ``policy.ObsNormalizer`` whose blocks cover the creatures: every generation starts with its ``freeze()`` -- within
    a generation every child sees the same tables -- and the generation's episodes add what they observe to its sums."""
    n = _population("run_policy_snes", env)
    S = es.group_size
    if n % S or es.mean.n_sets * S != n:
        raise ValueError("run_policy_snes: %d creatures are not %d means times the strategy's group_size %d" % (n, es.mean.n_sets, S))
    dev = env.worlds[0][0].device
    if es.device != dev:
        raise ValueError("run_policy_snes: the strategy is on %s, the population on %s" % (es.device, dev))
    fit, history = _generations(env, 1, n_generations, lambda gen: es.sample(gen, seed=seed), _policy_episode(env, max_steps, chunk, on_error),
                                lambda gen, children, fit: (children, fit, es.update(fit, gen, seed=seed)), on_generation, log,
                                normalizer=normalizer)
    return es.mean, fit, history


def run_behaviour_episode(env, period, samples, max_steps=EPISODE_CAP, on_error="raise"):
    """An episode that records where every creature went: ``env.set_descriptor(period, samples)`` (kept where the env already has
    that descriptor), ``describe()`` once at step 0, then ``period`` steps and ``describe()`` in turn -- ``env.step_policy`` if a
    policy is attached, else ``env.step``, so the reference's oscillator-driven creatures are described as well -- until ``samples``
    periods have run, or ``max_steps`` steps, or everyone is frozen (one small read per period).  Never compacts: compaction would
    retire rows.  Returns ``(fitness, behaviour)``: float64 ``[N]`` (a clone) and the env's float32 ``[N, 2 * samples]`` descriptor
    buffer itself (clone what must last), slot k the root position at step ``(k + 1) * period`` or the last one recorded before the
    creature's episode ended (include/rem2d_novelty.h).  on_error: "raise" | "warn" | "ignore", as run_policy_episode."""
    _strict_on_error(on_error)
    _population("run_behaviour_episode", env)
    have = env._descriptor
    if have is None or have[0] != int(period) or have[1] != (None if samples is None else int(samples)):
        env.set_descriptor(period, samples)
    period, samples = env._descriptor[:2]
    step = env.step if env.policy is None else env.step_policy
    env.last_episode = None
    env.describe()
    done_steps = 0
    for _ in range(samples):
        n = min(period, int(max_steps) - done_steps)
        if n <= 0:
            break
        step(n)
        done_steps += n
        env.describe()
        if bool((env.frozen != 0).all()):
            break
    check_errors(env, on_error)
    return env.fitness.clone(), env.behaviour


def _es_ranks(mean, values, group_size, out):
    """Centred ranks of float64 ``values`` within blocks of group_size into int32 ``out`` (rem2d_es_shape: ties averaged, NaN lowest)."""
    import ctypes as C
    e = mean._es_descriptor("run_policy_nses", 0, 0, group_size)
    e.fitness, e.util = values.data_ptr(), out.data_ptr()
    dev = values.device
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().rem2d_es_shape(C.byref(e), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return out


def run_policy_nses(env, mean, n_generations, archive, k=15, rate=0.02, weights=(1, 1), period=None, samples=4, seed=0, sigma=0.1,
                    lr=0.05, group_size=None, max_steps=EPISODE_CAP, on_error="raise", log=None, on_generation=None,
                    normalizer=None):
    """run_policy_es with behavioural novelty beside the fitness (NS-ES / NSR-ES): every generation is ``mean.es_sample``,
    ``env.set_policy``, ``env.reset_where`` of everyone, ``run_behaviour_episode`` (``samples`` root positions, one every ``period``
    steps; default period: ``max_steps`` over ``samples``, rounded up, so that the samples span the episode -- the episode ends after
    ``min(samples * period, max_steps)`` steps), ``archive.step`` (a ``novelty.NoveltyArchive`` of M blocks of width ``2 * samples``
    on the env's device: the k-nearest-neighbour novelty of every child among its block's peers and archive, then a share ``rate``
    of the children joins the archive), the centred ranks of the fitness and of the novelty within each block, and
    ``es_update(util = w_f * ranks(fitness) + w_n * ranks(novelty))`` with the integer ``weights`` (w_f, w_n): (1, 0) is
    run_policy_es bit for bit, (0, 1) is NS-ES, (1, 1) NSR-ES.  The combination is int32 arithmetic on the device.  One child policy,
    two sets of mean buffers and one each of novelty, rank and scratch tensors are reused throughout; ``mean`` itself is never
    written.  Returns ``(mean, fitness, history)`` as run_policy_es, the history rows being ``(gen, min, max, mean)`` of the fitness.
    ``on_generation(gen, children, fitness, mean, behaviour, novelty, util)``, if given, is called after every update with the
    tensors themselves and the NEW mean (clone what must last).
    ``normalizer``: a ``policy.ObsNormalizer`` whose blocks cover the creatures: every generation starts with its ``freeze()`` -- within
    a generation every child sees the same tables -- and the generation's episodes add what they observe to its sums."""
    n = _population("run_policy_nses", env)
    S = _es_groups("run_policy_nses", n, mean, group_size)
    wf, wn = (int(w) for w in weights)
    if (wf, wn) != tuple(weights) or abs(wf) > 32767 or abs(wn) > 32767:
        raise ValueError("run_policy_nses: weights must be two integers of at most 15 bits, not %r" % (weights,))
    samples = int(samples)
    period = _period(period, samples, max_steps)
    dev = _archive_fits("run_policy_nses", env, archive, mean.n_sets, samples)
    mean = mean.to(dev)
    children = spare = None
    scratch = _es_scratch(mean, S, dev)
    nov = torch.empty(n, dtype=torch.float64, device=dev)
    util_f, util_n, util = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))

    def sample(gen):
        nonlocal children
        children = mean.es_sample(gen, seed=seed, sigma=sigma, group_size=S, out=children)
        return children

    def update(gen, children, fit, behaviour):
        nonlocal mean, spare
        archive.step(behaviour, gen, k=k, seed=seed, rate=rate, group_size=S, out=nov)
        _es_ranks(mean, fit, S, util_f)
        _es_ranks(mean, nov, S, util_n)
        torch.add(util_f.mul_(wf), util_n, alpha=wn, out=util)
        new = mean.es_update(None, gen, seed=seed, sigma=sigma, lr=lr, group_size=S, out=spare, scratch=scratch, util=util)
        spare, mean = (mean if gen > 1 else None), new      # (the first mean's buffers are the caller's: never written)
        return children, fit, mean, behaviour, nov, util
    fit, history = _generations(env, 1, n_generations, sample, _behaviour_episode(env, period, samples, max_steps, on_error), update,
                                on_generation, log, normalizer=normalizer)
    return mean, fit, history


def _pareto_loop_checks(what, env, n_sets, group_size, even, archive, samples, max_steps, period, on_error):
    """What run_policy_pareto_es and run_policy_nslc refuse, before anything is allocated -> (n, S, samples, period, device)"""
    _strict_on_error(on_error)
    n = _population(what, env, described=True)
    S = n if group_size is None else int(group_size)
    if S < 1 or n % S or S > _lib.PARETO_MAX_GROUP or (even and (S < 2 or S % 2)) or n_sets * (S if even else 1) != n:
        raise ValueError("%s: %d creatures and %d weight sets are not blocks of %s group_size of at most %d (%r)"
                         % (what, n, n_sets, "an even" if even else "one", _lib.PARETO_MAX_GROUP, group_size))
    samples = int(samples)
    period = _period(period, samples, max_steps)
    return n, S, samples, period, _archive_fits(what, env, archive, n // S, samples)


def run_policy_pareto_es(env, mean, n_generations, archive, k=15, rate=0.02, period=None, samples=4, seed=0, sigma=0.1, lr=0.05,
                         group_size=None, max_steps=EPISODE_CAP, on_error="raise", log=None, on_generation=None):
    """run_policy_nses with a Pareto ranking in place of the weighted sum of ranks: every generation is ``mean.es_sample``,
    ``env.set_policy``, ``env.reset_where`` of everyone, ``run_behaviour_episode``, ``archive.step`` (the novelty of every child,
    then a share ``rate`` of them joins the archive) and ``es_update(util = pareto.rank(stack(fitness, novelty)).util)``: within
    each block the children are ordered by non-dominated front, then by crowding (include/rem2d_pareto.h), so a child that is the
    most novel of its block counts as much as the fittest one, whatever the other objective says -- which no weights of
    run_policy_nses give.  group_size is at most 1024.  One child policy, two sets of mean buffers and one each of novelty,
    objective, rank and scratch tensors are reused throughout: nothing is allocated after the first generation; ``mean`` itself is
    never written.  Returns ``(mean, fitness, history)`` as run_policy_es.  ``on_generation(gen, children, fitness, mean,
    behaviour, novelty, util)``, if given, is called after every update with the tensors themselves and the NEW mean (clone what
    must last).  Like ``describe`` it raises under auto-reset or streaming."""
    from . import pareto
    n, S, samples, period, dev = _pareto_loop_checks("run_policy_pareto_es", env, mean.n_sets, group_size, True, archive, samples,
                                                     max_steps, period, on_error)
    mean = mean.to(dev)
    children = None
    scratch = _es_scratch(mean, S, dev)
    # (the two sets of mean buffers, written in turn: the first mean's buffers are the caller's and never written)
    turn = [mean._like(*(torch.empty_like(t) for t in (mean.w1, mean.b1, mean.w2, mean.b2)), None) for _ in range(2)]
    nov = torch.empty(n, dtype=torch.float64, device=dev)
    obj = torch.empty((n, 2), dtype=torch.float64, device=dev)
    ranks = (None, None, torch.empty(n, dtype=torch.int32, device=dev), None)

    def sample(gen):
        nonlocal children
        children = mean.es_sample(gen, seed=seed, sigma=sigma, group_size=S, out=children)
        return children

    def update(gen, children, fit, behaviour):
        nonlocal mean
        archive.step(behaviour, gen, k=k, seed=seed, rate=rate, group_size=S, out=nov)
        obj[:, 0].copy_(fit)
        obj[:, 1].copy_(nov)
        util = pareto.rank(obj, group_size=S, out=ranks).util
        mean = mean.es_update(None, gen, seed=seed, sigma=sigma, lr=lr, group_size=S, out=turn[gen & 1], scratch=scratch, util=util)
        return children, fit, mean, behaviour, nov, util
    fit, history = _generations(env, 1, n_generations, sample, _behaviour_episode(env, period, samples, max_steps, on_error), update,
                                on_generation, log)
    return mean, fit, history


def run_policy_nslc(env, policy, n_generations, archive, k=15, rate=0.02, period=None, samples=4, seed=0, mut_rate=0.05, sigma=0.1,
                    tournsize=4, group_size=None, elite=0, max_steps=EPISODE_CAP, on_error="raise", log=None, on_generation=None):
    """Novelty search with local competition (Lehman and Stanley) for device policies: run_policy_generations' loop on
    ``run_behaviour_episode``, selecting by a Pareto ranking of two objectives -- the novelty of a creature's behaviour
    (``archive.step``: k nearest neighbours among its block's peers and archive; a share ``rate`` then joins the archive) and its
    local competition (``pareto.local_competition``: how many of its k nearest peers it out-walks).  Generation 0's episode runs
    first; every generation g = 1 .. is ``policy.evolve(fitness = util as float64, g, rate=mut_rate, ...)`` with ``util`` the rank
    utility of the generation before (include/rem2d_pareto.h), ``env.set_policy``, ``env.reset_where`` of everyone and the
    episode.  group_size (default: everyone) is at most 1024.  Two sets of weight buffers and one each of novelty, local, objective
    and rank tensors are reused; ``policy`` itself is never written.  Returns ``(policy, fitness, history)`` as
    run_policy_generations.  ``on_generation(gen, policy, fitness, behaviour, novelty, local, util)``, if given, is called after
    every episode, generation 0's included, with the tensors themselves (clone what must last).  Like ``describe`` it raises under
    auto-reset or streaming."""
    from . import pareto
    n, S, samples, period, dev = _pareto_loop_checks("run_policy_nslc", env, policy.n_sets, group_size, False, archive, samples,
                                                     max_steps, period, on_error)
    nov, loc = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2))
    obj = torch.empty((n, 2), dtype=torch.float64, device=dev)
    sel = torch.empty(n, dtype=torch.float64, device=dev)
    ranks = (None, None, torch.empty(n, dtype=torch.int32, device=dev), None)
    spare = None

    def child(gen):
        nonlocal policy, spare
        if gen:
            new = policy.evolve(sel, gen, seed=seed, rate=mut_rate, sigma=sigma, tournsize=tournsize, group_size=S, elite=elite, out=spare)
            spare, policy = (policy if gen > 1 else None), new    # (generation 0's buffers are the caller's: never written)
        return policy

    def scored(gen, attached, fit, behaviour):
        nonlocal policy
        if not gen:
            policy = env.policy      # (the caller's, on the env's device)
        archive.step(behaviour, gen, k=k, seed=seed, rate=rate, group_size=S, out=nov)
        pareto.local_competition(behaviour, fit, k=k, group_size=S, out=loc)
        obj[:, 0].copy_(nov)
        obj[:, 1].copy_(loc)
        util = pareto.rank(obj, group_size=S, out=ranks).util
        sel.copy_(util)
        return policy, fit, behaviour, nov, loc, util
    fit, history = _generations(env, 0, n_generations, child, _behaviour_episode(env, period, samples, max_steps, on_error), scored,
                                on_generation, log)
    return policy, fit, history


def run_policy_map_elites(env, policy, grid, n_generations, period=None, samples=4, seed=0, rate=0.05, sigma=0.1, group_size=None,
                          max_steps=EPISODE_CAP, on_error="raise", log=None, on_generation=None, sigma_line=None,
                          normalizer=None):
    """MAP-Elites for device policies: ``grid`` (an ``elites.EliteGrid`` of M = n_envs / ``group_size`` blocks over descriptor rows
    of ``2 * samples`` words on the env's device) keeps, per block of consecutive creatures -- a morphology -- and per cell of
    behaviour space, the best controller seen so far.  Generation 0 evaluates ``policy`` (one weight set per creature of ``env``,
    reset first) with ``run_behaviour_episode`` (``samples`` root positions, one every ``period`` steps; default period:
    ``max_steps`` over ``samples``, rounded up) and inserts it; every generation g = 1 .. is ``grid.emit`` (generation g, this
    ``seed``, ``rate`` and ``sigma`` as ``MLPPolicy.evolve`` takes them) into ONE reused child policy, ``env.set_policy``,
    ``env.reset_where`` of everyone, ``run_behaviour_episode`` and ``grid.insert``.  Emit reads the grid, not the previous children,
    so there is no double buffer; a block whose grid is still empty (nobody admissible so far) runs its children again as they are;
    ``policy`` itself is never written.  Returns ``(grid, fitness, history)``: the last generation's fitness (float64 [N] on the
    device) and rows ``(gen, min, max, mean, filled cells, qd_score)``, generation 0's included, the only numbers that leave the
    device.  ``on_generation(gen, children, fitness, behaviour, grid)``, if given, is called after every insert with the tensors
    themselves (clone what must last).  Like ``describe`` it raises under auto-reset or streaming.

    ``grid`` may be an ``elites.CentroidArchive`` over rows of ``2 * samples`` words: insertion is then by nearest centroid.
    ``sigma_line``: None is the emission above; a float switches it to ``grid.emit_line(sigma_iso=sigma, sigma_line=sigma_line)``,
    the iso+line variation between two elites, which moves every element: ``rate`` is then unused.
    ``normalizer``: a ``policy.ObsNormalizer`` whose blocks cover the creatures: every generation starts with its ``freeze()`` -- within
    a generation every child sees the same tables -- and the generation's episodes add what they observe to its sums."""
    from .elites import EliteGrid
    if not isinstance(grid, EliteGrid):
        raise ValueError("run_policy_map_elites: grid must be an elites.EliteGrid")
    n = _population("run_policy_map_elites", env, described=True)
    S = n // grid.n_blocks if group_size is None else int(group_size)
    if S < 1 or S * grid.n_blocks != n:
        raise ValueError("run_policy_map_elites: %d creatures in groups of %r are not the grid's %d blocks" % (n, group_size, grid.n_blocks))
    if policy.index is not None or policy.n_sets != n:
        raise ValueError("run_policy_map_elites: the policy must hold one weight set per creature (%d), without an index" % n)
    samples = int(samples)
    if grid.width != 2 * samples:
        raise ValueError("run_policy_map_elites: the grid must be over rows of %d words (2 * samples), not %d" % (2 * samples, grid.width))
    period = _period(period, samples, max_steps)
    dev = env.worlds[0][0].device
    if grid.device != dev:
        raise ValueError("run_policy_map_elites: the grid must be on %s, not %s" % (dev, grid.device))
    children = policy = policy.to(dev)

    def emit(gen):
        nonlocal children
        if gen:
            if children is policy:      # the one child buffer, made of the caller's sets: what a still empty block runs again
                children = policy._like(policy.w1.clone(), policy.b1.clone(), policy.w2.clone(), policy.b2.clone(), None)
            if sigma_line is None:
                grid.emit(gen, seed=seed, rate=rate, sigma=sigma, n_children=n, out=children)
            else:
                grid.emit_line(gen, seed=seed, sigma_iso=sigma, sigma_line=float(sigma_line), n_children=n, out=children)
        return children

    def insert(gen, children, fit, behaviour):
        grid.insert(children, fit, behaviour, group_size=S)
        return children, fit, behaviour, grid

    def row(fit):
        stats = _fitness_row(fit, grid.n_filled.sum().to(torch.float64), grid.qd_score().sum())
        return stats[:3] + (int(stats[3]), stats[4])
    fit, history = _generations(env, 0, n_generations, emit, _behaviour_episode(env, period, samples, max_steps, on_error), insert,
                                on_generation, log, normalizer=normalizer, reset_first=True, rows_from=0, row=row,
                                text="Generation %d : Min %s, Max %s, Avg %s, Cells %d, QD %s")
    return grid, fit, history


def run_stream(env, batches, n_total, slots, max_steps=EPISODE_CAP, chunk=100, on_error="fallback"):
    """run_episode for a population that does not get an arena per creature: ``batches`` ([(Morphology, ids)] per lane bucket, as
    reset_batches takes them) are streamed through ``slots`` slots of ``env`` (BatchedModular2D.reset_stream) -- ``step(chunk)``,
    ``refill()``, until every creature has finished; one small read per chunk.  A creature's episode ends when its fitness is final
    (REM2D_F_FROZEN) or after ``max_steps`` steps, whichever a refill() finds first; its slot goes to the next pending creature of its
    lane count.  Returns fitness[n_total] (float64 tensor on the env's device), the same values run_episode gives the same
    population uploaded as a whole: creatures are independent.

    The env needs REM2D_FLAG_SKIP_FROZEN (EVAL_FLAGS): a retired slot must stop costing steps.  ``max_steps`` must be a multiple of
    ``chunk``: the step limit is judged between two step calls, and a creature loaded at a call boundary has to meet it exactly.
    on_error: "raise" / "warn" / "ignore" judge ``stream.err`` as check_errors judges errors() (``env.last_episode`` is None after
    them); "fallback" / "penalty" evaluate the creatures with any error bit -- a failed hand-over of the step train, a capacity
    overflow -- again from reset in a fresh env on per-step launches through run_episode(on_error=...), which resolves overflow in
    the wide build and applies the penalty, and leave the EpisodeReport (by id) in ``env.last_episode``."""
    if on_error not in ("fallback", "penalty", "raise", "warn", "ignore"):
        raise ValueError("on_error must be 'fallback', 'penalty', 'raise', 'warn' or 'ignore', not %r" % (on_error,))
    if not env.flags & _lib.FLAG_SKIP_FROZEN:
        raise ValueError("run_stream: the env needs REM2D_FLAG_SKIP_FROZEN (flags=evaluate.EVAL_FLAGS): retired slots must stop being stepped")
    max_steps, chunk = int(max_steps), int(chunk)
    if chunk <= 0 or max_steps <= 0 or max_steps % chunk != 0:
        raise ValueError("run_stream: max_steps (%d) must be a positive multiple of chunk (%d): the step limit is judged between step "
                         "calls, and a creature loaded at a call boundary must meet it exactly" % (max_steps, chunk))
    batches = [(m, np.asarray(idx, dtype=np.int64)) for m, idx in batches]
    env.reset_stream(batches, n_total, slots)
    st = env.stream
    # every slot hands on at least one creature per max_steps steps: more chunks than this and something is wrong
    limit = (max_steps // chunk) * (int(n_total) + 1)
    policy, env.on_handover = env.on_handover, "flag"   # (flagged creatures are dealt with below, like run_episode_masked's)
    try:
        for _ in range(limit):
            env.step(chunk)
            env.refill(when=("frozen", "steps"), max_steps=max_steps)
            if bool(st.finished.all()):
                break
        else:
            raise _lib.Rem2dError("run_stream: %d creature(s) unfinished after %d chunks" % (int((~st.finished).sum()), limit))
    finally:
        env.on_handover = policy
    env.handover_failures(clear=True)
    fit, err = st.fitness.clone(), st.err.clone()
    if on_error in ("raise", "warn", "ignore"):
        env.last_episode = None
        judge_errors(err, on_error)
        return fit
    bad = torch.nonzero(err != 0).flatten().cpu().numpy()
    handover, overflow, unresolved = [], [], []
    if bad.size:
        again = _replay_env(env, batches, bad, env.wide, {"fuse_velpost": 1})   # per-step launches: no hand-over between workgroups exists there
        try:
            fit2 = run_episode(again, max_steps, chunk, on_error=on_error, compact=False)
        except SolverOverflow as e:
            raise SolverOverflow([int(bad[i]) for i in e.indices], e.codes)
        finally:
            report = again.last_episode
            again.close()
        where = torch.as_tensor(bad, dtype=torch.long, device=fit.device)
        fit.index_copy_(0, where, fit2.to(fit.device))
        handover = sorted(int(i) for i in bad[(err[where] & _lib.ERR_HANDOVER).cpu().numpy() != 0])
        err.index_copy_(0, where, report.codes.to(err.device))
        handover = sorted(set(handover) | {int(bad[i]) for i in report.handover})
        overflow, unresolved = [int(bad[i]) for i in report.overflow], [int(bad[i]) for i in report.unresolved]
    env.last_episode = EpisodeReport(err, handover, overflow, unresolved)
    return fit


def evaluate_population(individuals, tree_depth=None, env=None, max_steps=EPISODE_CAP, workers=None, on_error="fallback",
                        slots=None, **env_kw):
    """Batched stand-in for ``toolbox.map(toolbox.evaluate, population)``: list of floats.
    The genotype -> phenotype step runs natively on ``workers`` host threads (encode.encode_native).
    on_error: what to do when a creature overflowed the engine's contact capacity ("fallback": re-evaluate it in the
    wide build and raise only if even that overflows, the default | "penalty": the same without ever raising, see
    run_episode | "raise" | "warn" | "ignore").
    slots: None (the default) uploads every individual; a number below ``len(individuals)`` streams the population through that
    many arena slots instead (run_stream: the same fitness from a fraction of the device memory; the env needs EVAL_FLAGS and
    max_steps a multiple of 100)."""
    from .encode import encode_native
    from .env import BatchedModular2D
    own = env is None
    if own:
        env_kw.setdefault("flags", EVAL_FLAGS)
        env = BatchedModular2D(**env_kw)
    batches = encode_native(individuals, tree_depth, n_threads=workers or 0)
    if slots is not None and len(individuals) > slots:
        fit = run_stream(env, batches, len(individuals), slots, max_steps, on_error=on_error).cpu().tolist()
    else:
        env.reset_batches(batches, len(individuals))
        fit = run_episode(env, max_steps, on_error=on_error).cpu().tolist()
    if own:
        env.close()
    return fit


def shard_range(n, rank, world_size):
    """Contiguous block [lo, hi) of rank `rank` (rank r owns [r*ceil(n/W), (r+1)*ceil(n/W)))."""
    per = math.ceil(n / world_size)
    lo = min(n, rank * per)
    return lo, min(n, lo + per)


def shard_balanced(cost, world_size):
    """Cost-balanced shards (what replaces the dynamic balancing of REM2D_main.py:256-262's pool.map): the individuals in
    descending order of a static cost key (ties: population order -- every rank computes the same deal) are dealt snake-wise
    over the ranks, 0 .. W-1, W-1 .. 0, 0 ..  Returns int64 [W][ceil(n / W)]: row r = the population indices of rank r in the order
    it evaluates them, padded with -1.  Episodes end early for creatures that fall or get caught (Modular2DEnv.py:642-649), which
    no static key sees; what the key evens out is the per-step cost (lanes, joint rounds, solver work: all grow with the bodies)."""
    cost = np.asarray(cost)
    n, W = len(cost), int(world_size)
    per = math.ceil(n / W) if n else 0
    order = np.argsort(-cost.astype(np.int64), kind="stable")
    out = np.full((W, per), -1, dtype=np.int64)
    k = np.arange(n)
    rnd, pos = k // W, k % W
    rank = np.where(rnd % 2 == 0, pos, W - 1 - pos)
    out[rank, rnd] = order
    return out


def shard_costs(cost, index):
    """Predicted cost of every rank under the deal `index` (shard_balanced): float64 [W]."""
    cost = np.asarray(cost, dtype=np.float64)
    return np.array([cost[row[row >= 0]].sum() for row in np.asarray(index)])


def all_gather_fitness(local, n_total, group=None, flags=None, index=None):
    """One all_gather of float64 fitness scalars: [per] -> [n_total] on every rank.  `local` is padded to ceil(n/W) so
    that the collective is a single equal-sized all_gather_into_tensor.  float64 like the reference's python floats
    (REM2D_main.py:372-375 compares ``reward + (10000 - i) / 10000`` in doubles): a sharded and a single-GPU run return
    the same values, so tournament winners cannot depend on the world size.  8 MiB at 1 M individuals.
    flags: optional bool / int [per] mask of the rank's creatures without a valid fitness (run_episode_masked); it rides
    in the same collective as a second column and the call returns (fitness [n_total], flags [n_total] bool) -- every
    rank learns about every rank's failures AFTER the collective and can raise in step.
    index: the deal of shard_balanced (int64 [W][per], -1 padding) when the ranks hold dealt instead of contiguous shards:
    rank r's j-th value belongs to individual index[r][j]; the result is in population order either way."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    per = math.ceil(n_total / world)
    cols = 1 if flags is None else 2
    buf = torch.zeros(cols, per, dtype=torch.float64, device=local.device)
    buf[0, :local.numel()] = local.to(torch.float64)
    if flags is not None:
        buf[1, :local.numel()] = torch.as_tensor(flags, device=local.device).to(torch.float64)
    out = torch.empty(world * cols * per, dtype=torch.float64, device=local.device)
    dist.all_gather_into_tensor(out, buf.reshape(-1), group=group)
    out = out.view(world, cols, per)
    if index is None:
        fit = out[:, 0].reshape(-1)[:n_total]
        bad = out[:, 1].reshape(-1)[:n_total] != 0 if flags is not None else None
    else:   # dealt shards: scatter back to population order
        idx = torch.as_tensor(np.asarray(index), dtype=torch.long, device=out.device).reshape(-1)
        keep = idx >= 0
        fit = torch.zeros(n_total, dtype=torch.float64, device=out.device)
        fit[idx[keep]] = out[:, 0].reshape(-1)[keep]
        bad = None
        if flags is not None:
            bad = torch.zeros(n_total, dtype=torch.bool, device=out.device)
            bad[idx[keep]] = out[:, 1].reshape(-1)[keep] != 0
    if flags is None:
        return fit
    return fit, bad


def _evaluate_sharded(n_total, run_local, cost, group, device, on_error):
    """The protocol of a sharded evaluation, once: deal (``cost``: a static key per individual, shard_balanced) or cut (None:
    contiguous blocks, shard_range) the shards, evaluate this rank's with ``run_local(population indices, int64 array) -> fitness``
    (or ``-> (fitness, unresolved mask)``: run_episode_masked), one all-gather, the verdict after it.
    Returns (fitness [n_total] float64 tensor in population order, unresolved indices, predicted cost per rank | None).
    The mask rides in the fitness all-gather: a rank with a creature that has no valid fitness does not raise before the
    collective (the others would wait in it for ever).  After it every rank holds the same mask: every rank raises SolverOverflow
    in step, or (on_error="penalty") the creatures get UNRESOLVED_FITNESS on every rank alike and every rank warns."""
    import torch.distributed as dist
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    index = shard_cost = None
    if cost is not None:
        index = shard_balanced(cost, world)
        shard_cost = shard_costs(cost, index)
        mine = index[rank][index[rank] >= 0]
    else:
        mine = np.arange(*shard_range(n_total, rank, world))
    local, mask = run_local(mine), None
    if isinstance(local, tuple):
        local, mask = local
    local = torch.as_tensor(local, dtype=torch.float64, device=device)
    if mask is None:
        mask = torch.zeros(local.numel(), dtype=torch.bool)
    fit, bad = all_gather_fitness(local, n_total, group, flags=mask, index=index)
    unresolved = []
    if bool(bad.any()):
        if on_error != "penalty":
            idx = torch.nonzero(bad).flatten().cpu().tolist()
            raise SolverOverflow(idx, [_lib.ERR_SOLVER_OVERFLOW] * len(idx))
        unresolved = apply_penalty(fit, bad, warn=True)
    return fit, unresolved, shard_cost


def evaluate_population_sharded(n_total, local_eval, group=None, device=None, on_error="raise", cost=None):
    """Shard [0, n_total) over the job's ranks, evaluate the local block with
    ``local_eval(lo, hi) -> tensor[hi-lo]`` (or ``-> (tensor, unresolved mask)``, run_episode_masked) and all-gather.
    cost (optional, [n_total], the same on every rank): a static cost key per individual -- the shards are then dealt by
    shard_balanced instead of cut contiguously, ``local_eval(indices)`` gets the rank's population indices (int64 array) and
    ``evaluate_population_sharded.last_shard_cost`` holds the predicted cost per rank (None after a call without ``cost``); the
    result is in population order.
    Returns fitness[n_total] (float64).  The mask rides in the same collective, so every rank learns about every rank's
    unresolved creatures AFTER it: with on_error="raise" (the library default -- the reference has no contact cap and would
    have produced a fitness) every rank raises SolverOverflow in step; with "penalty" (an EA loop's opt-in) they get
    UNRESOLVED_FITNESS on every rank alike, every rank warns, ``evaluate_population_sharded.last_unresolved`` lists them and
    the job goes on."""
    run_local = local_eval
    if cost is None:   # (a contiguous block as its two ends; an empty one lies at the population's end: shard_range)
        def run_local(idx):
            return local_eval(int(idx[0]), int(idx[-1]) + 1) if len(idx) else local_eval(n_total, n_total)
    fit, evaluate_population_sharded.last_unresolved, evaluate_population_sharded.last_shard_cost = _evaluate_sharded(
        n_total, run_local, cost, group, device, on_error)
    return fit


class sharded_evaluator:
    """evaluate(population) for a torch.distributed job (one process per GPU): every rank holds the whole
    population as arrays (selection and mutation are replicated from a shared seed, so no genome ever crosses a
    rank boundary), expresses and evaluates only its share with ``local_eval(population of that share) -> fitness``
    (or ``-> (fitness, unresolved mask)``: gpu_evaluator(masked=True)) and the ranks exchange one all-gather of float64
    fitness (REM2D_main.py:256-267 pool.map).  Returns the fitness in population order as float64 numpy.

    balance (default): the reference's pool balances dynamically (pool.map hands out chunks as workers finish); a static
    contiguous cut does not, and a generation ends with its slowest rank.  Every rank therefore computes the same deal from the
    arrays it holds anyway -- the individuals in descending order of body count (a native expression pass, population.body_counts)
    dealt snake-wise over the ranks, shard_balanced -- and the fitness comes back in population order through the same
    single all-gather.  ``last_shard_cost`` = the predicted cost (bodies) per rank.  balance=False: contiguous blocks.

    on_error: what to do about creatures without a valid fitness (beyond even the wide build's contact slots -- Box2D has
    no such cap, so the reference would have produced a number).  "raise" (the library default): every rank raises
    SolverOverflow AFTER the collective, in step.  "penalty" (what an EA loop opts into so that one out-of-domain creature
    does not abort a run): UNRESOLVED_FITNESS on every rank alike, a warning on EVERY rank, the indices in ``last_unresolved``
    and kept per call in ``unresolved_log`` (a list that grows by one entry per call: a long run cannot lose them)."""

    def __init__(self, local_eval, group=None, device=None, on_error="raise", balance=True, n_threads=0):
        self.local_eval, self.group, self.device, self.on_error = local_eval, group, device, on_error
        self.balance, self.n_threads = balance, n_threads
        self.last_unresolved, self.unresolved_log, self.last_shard_cost = [], [], None

    def __call__(self, pop):
        def run_local(idx):
            return self.local_eval(pop.select(idx)) if len(idx) else np.zeros(0, dtype=np.float64)
        fit, self.last_unresolved, self.last_shard_cost = _evaluate_sharded(
            len(pop), run_local, pop.body_counts(self.n_threads) if self.balance else None, self.group, self.device, self.on_error)
        self.unresolved_log.append(list(self.last_unresolved))
        return fit.cpu().numpy().astype(np.float64)


class gpu_evaluator:
    """local_eval for sharded_evaluator / evaluate for run_generations on one GPU: native expression, upload,
    whole episodes (evaluate()'s rule), fitness as float64 numpy.  Creatures that overflow the default build's contact
    slots are re-evaluated in the wide build (reevaluate_wide); one that overflows even that
    raises SolverOverflow (on_error="fallback", the library default: Box2D has no contact cap, so there is no fitness the
    reference would have given) or, if the caller opts in with on_error="penalty" (the EA loops do: one out-of-domain
    creature does not abort a generation), gets UNRESOLVED_FITNESS, a warning, and an entry in
    ``last_unresolved`` / ``unresolved_log`` (one list per call) -- or, with masked=True
    (what a sharded job wants), comes back in a second array ``(fitness, unresolved)`` so that the verdict is taken after
    the job's collective."""

    def __init__(self, env=None, max_steps=None, n_threads=0, masked=False, on_error="fallback"):
        self.env, self.n_threads, self.masked, self.on_error = env, n_threads, masked, on_error
        self.max_steps = max_steps if max_steps is not None else EPISODE_CAP
        self.last_unresolved, self.unresolved_log = [], []

    def __call__(self, pop):
        if self.env is None:
            from .env import BatchedModular2D
            self.env = BatchedModular2D(flags=EVAL_FLAGS)
        self.env.reset_batches(pop.compile(self.n_threads), len(pop))
        if self.masked:
            fit, bad = run_episode_masked(self.env, self.max_steps)
            return fit.cpu().numpy(), bad.cpu().numpy()
        fit = run_episode(self.env, self.max_steps, on_error=self.on_error).cpu().numpy()
        report = self.env.last_episode   # (None after the modes that judge without a second attempt)
        self.last_unresolved = list(report.unresolved) if report is not None else []
        self.unresolved_log.append(list(self.last_unresolved))
        return fit
