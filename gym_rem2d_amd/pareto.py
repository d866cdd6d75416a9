"""Pareto ranking on the device (include/rem2d_pareto.h): the non-dominated fronts, the crowding distance and a rank utility of rows
of up to four objectives -- the order NSGA-II keeps a population in -- and the local-competition score of novelty search with local
competition: among a row's nearest behavioural neighbours, how many it out-performs.

``rank(...).util`` is int32 ``[G]`` in the range and with the zero block sums of the evolution strategy's rank shaping, so
``MLPPolicy.es_update(util=...)`` takes it as it is and ``MLPPolicy.evolve(fitness=util.double())`` selects by it;
``evaluate.run_policy_pareto_es`` and ``evaluate.run_policy_nslc`` are those two loops.

Every ValueError comes before anything is allocated; every call is one library call queued on the current stream; nothing
synchronises.  tests/pareto_model.py restates every output bit in numpy."""
import collections

import torch

from . import _lib
from ._tier import is_tensor, launch, overlaps

ParetoRank = collections.namedtuple("ParetoRank", "front crowd util n_fronts")
RANK_OUT = (("front", torch.int32), ("crowd", torch.float64), ("util", torch.int32), ("n_fronts", torch.int32))


def _disjoint(what, out_name, out, in_name, inp):
    if overlaps(out, inp):
        raise ValueError("%s: %s shares memory with %s" % (what, out_name, in_name))


def _groups(what, G, group_size, limit=None):
    S = G if group_size is None else int(group_size)
    if S < 1 or G % S or (limit is not None and S > limit):
        raise ValueError("%s: group_size must be 1 .. %s and divide the %d rows, not %r" % (what, "any" if limit is None else limit, G, group_size))
    return S


def rank(objectives, group_size=None, out=None, wide=False):
    """``ParetoRank(front, crowd, util, n_fronts)`` of ``objectives``, float64 ``[G, K]`` on the GPU (a ``[G]`` tensor is one
    objective), K up to 4, every objective maximised, within blocks of ``group_size`` consecutive rows (default: one block; at most
    1024 rows): ``front`` int32 ``[G]``, 0 for the rows nobody dominates, then the peel; ``crowd`` float64 ``[G]``, NSGA-II's
    crowding distance on values (+inf where a row has no strictly smaller or no strictly greater peer in its front); ``util`` int32
    ``[G]``, ``2 L + E - (S - 1)`` on the order (front ascending, crowd descending); ``n_fronts`` int32 ``[G / S]``.  A row with a
    non-finite word is not admitted: it dominates nobody and shares the last front (rem2d_pareto_rank; the header defines every
    bit).  ``out``: a ParetoRank (or any sequence of four) of contiguous tensors to write into, any of which may be None -- that
    output is left out and comes back as None; without ``out`` all four are allocated."""
    what = "rank"
    if not isinstance(objectives, torch.Tensor) or objectives.dtype != torch.float64:
        raise ValueError("%s: objectives must be a torch.float64 tensor" % what)
    if objectives.dim() not in (1, 2) or objectives.shape[0] < 1 or not objectives.is_contiguous():
        raise ValueError("%s: objectives must be a contiguous tensor [G, K] or [G] of at least one row, not %s" % (what, list(objectives.shape)))
    G = int(objectives.shape[0])
    K = 1 if objectives.dim() == 1 else int(objectives.shape[1])
    if not 1 <= K <= _lib.PARETO_MAX_OBJ:
        raise ValueError("%s: 1 .. %d objectives, not %d" % (what, _lib.PARETO_MAX_OBJ, K))
    if G > 2 ** 31 - 1:
        raise ValueError("%s: more than 2^31 - 1 rows" % what)
    S = _groups(what, G, group_size, _lib.PARETO_MAX_GROUP)
    dev = objectives.device
    if out is not None:
        out = tuple(out)
        if len(out) != 4:
            raise ValueError("%s: out must hold four tensors (front, crowd, util, n_fronts), each of which may be None" % what)
        for (name, dtype), o in zip(RANK_OUT, out):
            if o is None:
                continue
            n = G // S if name == "n_fronts" else G
            if not is_tensor(o, dtype, (n,), dev):
                raise ValueError("%s: out.%s must be a contiguous %s [%d] tensor on %s" % (what, name, dtype, n, dev))
            _disjoint(what, "out." + name, o, "objectives", objectives)
    if dev.type != "cuda":
        raise ValueError("%s: objectives are on %s; the ranking runs on the GPU" % (what, dev))
    if out is None:
        out = tuple(torch.empty(G // S if name == "n_fronts" else G, dtype=dtype, device=dev) for name, dtype in RANK_OUT)
    p = _lib.Pareto()
    p.n_rows, p.group_size, p.n_obj, p.reserved = G, S, K, 0
    p.obj = objectives.data_ptr()
    p.front, p.crowd, p.util, p.n_fronts = (None if o is None else o.data_ptr() for o in out)
    launch(_lib.lib(wide).rem2d_pareto_rank, p, dev, wide)
    return ParetoRank(*out)


def local_competition(desc, fitness, k=15, group_size=None, out=None, wide=False):
    """float64 ``[G]``: for every row, the number of its ``k`` nearest behavioural neighbours -- the other rows of its block of
    ``group_size`` consecutive rows (default: one block), by squared Euclidean distance of ``desc`` (float32 ``[G, B]`` on the GPU,
    B up to 32), ties to the lower row -- whose ``fitness`` (float64 ``[G]``) is below its own, a NaN being below every number
    (rem2d_pareto_local; the header defines every bit).  Fewer than k candidates at a finite distance: those there are.  A row with
    a non-finite descriptor word scores NaN.  ``out``: a contiguous float64 ``[G]`` tensor to write into."""
    what = "local_competition"
    if not isinstance(desc, torch.Tensor) or desc.dtype != torch.float32:
        raise ValueError("%s: desc must be a torch.float32 tensor" % what)
    if desc.dim() != 2 or desc.shape[0] < 1 or not 1 <= desc.shape[1] <= _lib.PARETO_MAX_WIDTH or not desc.is_contiguous():
        raise ValueError("%s: desc must be a contiguous tensor [G, B] of at least one row and 1 .. %d words, not %s"
                         % (what, _lib.PARETO_MAX_WIDTH, list(desc.shape)))
    G, B = int(desc.shape[0]), int(desc.shape[1])
    dev = desc.device
    if G > 2 ** 31 - 1:
        raise ValueError("%s: more than 2^31 - 1 rows" % what)
    if not is_tensor(fitness, torch.float64, (G,), dev):
        raise ValueError("%s: fitness must be a contiguous torch.float64 [%d] tensor on %s" % (what, G, dev))
    if not 1 <= int(k) <= _lib.PARETO_MAX_K:
        raise ValueError("%s: k must be 1 .. %d, not %r" % (what, _lib.PARETO_MAX_K, k))
    S = _groups(what, G, group_size)
    if out is not None:
        if not is_tensor(out, torch.float64, (G,), dev):
            raise ValueError("%s: out must be a contiguous torch.float64 [%d] tensor on %s" % (what, G, dev))
        _disjoint(what, "out", out, "desc", desc)
        _disjoint(what, "out", out, "fitness", fitness)
    if dev.type != "cuda":
        raise ValueError("%s: desc is on %s; the score runs on the GPU" % (what, dev))
    if out is None:
        out = torch.empty(G, dtype=torch.float64, device=dev)
    p = _lib.Pareto()
    p.n_rows, p.group_size, p.width, p.k, p.reserved = G, S, B, int(k), 0
    p.desc, p.fitness, p.local, p.neighbours = desc.data_ptr(), fitness.data_ptr(), out.data_ptr(), None
    launch(_lib.lib(wide).rem2d_pareto_local, p, dev, wide)
    return out
