"""Behavioural novelty on the device (include/rem2d_novelty.h): the k-nearest-neighbour novelty of behaviour descriptors against
their block's peers and an archive of what was seen before, and the archive's upkeep -- what novelty search, NS-ES / NSR-ES and
the distance half of quality-diversity methods rank by instead of, or beside, the fitness.

A descriptor is any float32 ``[G, B]`` on the device, B up to 32; ``BatchedModular2D.set_descriptor`` / ``describe`` record one --
the root position sampled K times over the episode -- and ``evaluate.run_behaviour_episode`` returns it.  The scores are float64
``[G]`` as ``MLPPolicy.evolve(fitness=...)`` takes them; ``evaluate.run_policy_nses`` ranks them for ``es_update(util=...)``.

Nothing here allocates after ``NoveltyArchive`` was made and ``out=`` is given; every call is one library call queued on the current
stream; nothing synchronises.  tests/novelty_model.py restates every output bit in numpy."""
import torch

from . import _lib
from ._tier import draw_ok, is_tensor, launch, overlaps, rate_threshold      # (rate_threshold, here the ``add_threshold``, is a public name of this module too)


class NoveltyArchive:
    """One ring of ``capacity`` descriptors of ``width`` words per block: ``entries`` float32 ``[n_blocks, capacity, width]`` and
    ``total`` int64 ``[n_blocks]``, the entries ever added -- entry e of block b is live while ``e < min(total[b], capacity)``, and
    the (total[b] + j)-th addition lands on entry ``(total[b] + j) % capacity``.  A block is ``group_size`` consecutive rows of the
    descriptors handed to ``score`` / ``add`` / ``step`` (the creatures of one morphology, or whatever the caller wants compared);
    the default group size is all rows over ``n_blocks``."""

    def __init__(self, n_blocks, capacity, width, device=None):
        n_blocks, capacity, width = int(n_blocks), int(capacity), int(width)
        if n_blocks < 1:
            raise ValueError("NoveltyArchive: n_blocks must be at least 1, not %r" % (n_blocks,))
        if capacity < 0 or capacity > 2 ** 31 - 1:
            raise ValueError("NoveltyArchive: capacity must be 0 .. 2^31 - 1, not %r" % (capacity,))
        if not 1 <= width <= _lib.NOVELTY_MAX_WIDTH:
            raise ValueError("NoveltyArchive: width must be 1 .. %d, not %r" % (_lib.NOVELTY_MAX_WIDTH, width))
        self.n_blocks, self.capacity, self.width = n_blocks, capacity, width
        self.entries = torch.zeros((n_blocks, capacity, width), dtype=torch.float32, device="cpu" if device is None else device)
        self.device = self.entries.device                   # (with its index: "cuda" became "cuda:0")
        self.total = torch.zeros(n_blocks, dtype=torch.int64, device=self.device)

    # ---- checkpoints ----
    def state_dict(self):
        return {"entries": self.entries.clone(), "total": self.total.clone()}

    def load_state_dict(self, state):
        entries, total = state["entries"], state["total"]
        if tuple(entries.shape) != tuple(self.entries.shape) or entries.dtype != torch.float32:
            raise ValueError("load_state_dict: entries must be float32 %s, not %s %s"
                             % (list(self.entries.shape), entries.dtype, list(entries.shape)))
        if tuple(total.shape) != tuple(self.total.shape) or total.dtype != torch.int64:
            raise ValueError("load_state_dict: total must be int64 %s, not %s %s" % (list(self.total.shape), total.dtype, list(total.shape)))
        self.entries.copy_(entries)
        self.total.copy_(total)

    # ---- the descriptor of a call, checked; nothing is allocated before the last check ----
    def _descriptor(self, what, desc, group_size, k=1, out=None, want_out=False, generation=0, seed=0, rate=0.0, mask=None):
        dev = self.device
        if not isinstance(desc, torch.Tensor) or desc.dtype != torch.float32:
            raise ValueError("%s: desc must be a torch.float32 tensor" % what)
        if desc.dim() != 2 or desc.shape[1] != self.width or desc.shape[0] < 1 or not desc.is_contiguous():
            raise ValueError("%s: desc must be a contiguous tensor [G, %d] of at least one row, not %s" % (what, self.width, list(desc.shape)))
        if desc.device != dev:
            raise ValueError("%s: desc must be on %s, not %s" % (what, dev, desc.device))
        G = int(desc.shape[0])
        if G > 2 ** 31 - 1:
            raise ValueError("%s: more than 2^31 - 1 rows" % what)
        if group_size is None:
            if G % self.n_blocks:
                raise ValueError("%s: %d rows are not %d blocks of one group_size" % (what, G, self.n_blocks))
            group_size = G // self.n_blocks
        S = int(group_size)
        if S < 1 or G % S or G // S != self.n_blocks:
            raise ValueError("%s: %d rows in groups of %r are not the archive's %d blocks" % (what, G, group_size, self.n_blocks))
        if not 1 <= int(k) <= _lib.NOVELTY_MAX_K:
            raise ValueError("%s: k must be 1 .. %d, not %r" % (what, _lib.NOVELTY_MAX_K, k))
        draw_ok(what, generation, seed)
        if not 0.0 <= float(rate) <= 1.0:
            raise ValueError("%s: rate must be in [0, 1], not %r" % (what, rate))
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8):
                raise ValueError("%s: mask must be a torch.bool or torch.uint8 tensor" % what)
            if not is_tensor(mask, (torch.bool, torch.uint8), (G,), dev):
                raise ValueError("%s: mask must be a contiguous tensor of one entry per row [%d] on %s, not %s" % (what, G, dev, list(mask.shape)))
        if out is not None and not is_tensor(out, torch.float64, (G,), dev):
            raise ValueError("%s: out must be a contiguous torch.float64 [%d] tensor on %s" % (what, G, dev))
        for name, other in (("the archive's entries", self.entries), ("out", out)):
            if other is not None and overlaps(other, desc):
                raise ValueError("%s: desc shares memory with %s" % (what, name))
        if dev.type != "cuda":
            raise ValueError("%s: the archive is on %s; make it on the GPU (device=...)" % (what, dev))
        if want_out and out is None:
            out = torch.empty(G, dtype=torch.float64, device=dev)
        n = _lib.Novelty()
        n.width, n.n_rows, n.group_size, n.k, n.capacity = self.width, G, S, int(k), self.capacity
        n.generation, n.seed, n.add_threshold, n.reserved = int(generation), int(seed), rate_threshold(rate), 0
        n.desc = desc.data_ptr()
        n.archive = self.entries.data_ptr() if self.capacity else None
        n.total = self.total.data_ptr()
        n.novelty = None if out is None else out.data_ptr()
        n.add_mask = None if mask is None else mask.data_ptr()
        return n, out

    def score(self, desc, k=15, group_size=None, out=None, wide=False):
        """novelty float64 ``[G]``: for every row of ``desc`` (float32 ``[G, width]`` on the archive's device) the mean Euclidean
        distance to its ``k`` nearest neighbours among the other rows of its block and the block's live archive entries
        (rem2d_novelty_score; the header states the arithmetic, of which every bit is defined).  Fewer than k candidates: the mean
        over those there are, 0.0 for none; candidates at a non-finite distance are ignored; a row with a non-finite word scores
        NaN, which ``evolve`` and the rank shaping put lowest.  ``out``: a contiguous float64 ``[G]`` tensor to write into."""
        n, out = self._descriptor("score", desc, group_size, k=k, out=out, want_out=True)
        launch(_lib.lib(wide).rem2d_novelty_score, n, self.device, wide)
        return out

    def add(self, desc, generation, seed=0, rate=0.02, mask=None, group_size=None, wide=False):
        """Add a random share ``rate`` of the rows to their block's ring (rem2d_novelty_add): row c is taken iff all its words are
        finite, ``mask`` (bool / uint8 ``[G]``, None = everyone) admits it and the counter-based draw of ``(seed, generation, c)``
        falls below ``rate`` -- a function of those alone, so a replay adds the same rows.  Returns ``total``."""
        n, _ = self._descriptor("add", desc, group_size, generation=generation, seed=seed, rate=rate, mask=mask)
        self._mask = mask   # (the tensor the queued kernel reads)
        launch(_lib.lib(wide).rem2d_novelty_add, n, self.device, wide)
        return self.total

    def step(self, desc, generation, k=15, seed=0, rate=0.02, mask=None, group_size=None, out=None, wide=False):
        """``score`` then ``add``, queued by one library call (rem2d_novelty_step): the scores are blind to the rows this call
        adds.  Returns the novelty, float64 ``[G]``."""
        n, out = self._descriptor("step", desc, group_size, k=k, out=out, want_out=True, generation=generation, seed=seed, rate=rate,
                                  mask=mask)
        self._mask = mask
        launch(_lib.lib(wide).rem2d_novelty_step, n, self.device, wide)
        return out


def describe(worlds, period, samples, out):
    """rem2d_worlds_describe for a list of BatchedWorld on one device: ``out`` float32 ``[rows, 2 * samples]``, written in place."""
    w0 = worlds[0]
    _lib.check(w0.L.rem2d_worlds_describe(_lib.world_array(worlds), len(worlds), int(period), int(samples), out.data_ptr(),
                                          int(out.shape[0]), w0._stream()), w0.wide)
    return out
