"""MAP-Elites for device policies (include/rem2d_elites.h): per block of creatures -- a morphology -- a grid over behaviour space
whose every cell keeps the best controller ever seen there, with its fitness and its descriptor row, on the device.

``EliteGrid.insert`` files a whole evaluated population (an ``MLPPolicy``, its float64 fitness and its float32 descriptors, as
``evaluate.run_behaviour_episode`` returns them) into the grids; ``EliteGrid.emit`` makes the next children, mutated copies of
uniformly drawn elites, with the mutation of ``MLPPolicy.evolve``; ``evaluate.run_policy_map_elites`` is the loop.

``CentroidArchive`` (include/rem2d_cvt.h) is the same state over C centroids instead of a regular cell map -- CVT-MAP-Elites: a row
belongs to its nearest centroid, over the whole descriptor row --, ``cvt_centroids`` makes the centroids, and ``EliteGrid.emit_line``
is the directional iso+line variation between two elites, on grids and centroid archives alike.  tests/cvt_model.py restates those.

Nothing here allocates after the grid was made and ``out=`` is given; every call is one library call queued on the current stream;
nothing synchronises.  tests/elites_model.py restates every output bit in numpy."""
import math

import numpy as np
import torch

from . import _lib
from ._tier import draw_ok, is_tensor, launch, overlaps, point, rate_threshold      # (rate_threshold is a public name of this module too)
from .policy import MLPPolicy


def _check_dims(dims, width):
    """dims [(word, lo, hi, bins), ...] -> (word, bins, lo float32, inv float32) lists, checked"""
    try:
        dims = [tuple(d) for d in dims]
    except TypeError:
        raise ValueError("EliteGrid: dims must be a list of (word, lo, hi, bins)")
    if not 1 <= len(dims) <= _lib.ELITES_MAX_DIMS or any(len(d) != 4 for d in dims):
        raise ValueError("EliteGrid: dims must be 1 .. %d tuples (word, lo, hi, bins), not %r" % (_lib.ELITES_MAX_DIMS, dims))
    word, bins, lo, inv, cells = [], [], [], [], 1
    for i, (w, l, h, n) in enumerate(dims):
        if int(w) != w or not 0 <= int(w) < width:
            raise ValueError("EliteGrid: dims[%d]: word must be 0 .. %d, not %r" % (i, width - 1, w))
        if int(n) != n or int(n) < 1:
            raise ValueError("EliteGrid: dims[%d]: bins must be at least 1, not %r" % (i, n))
        with np.errstate(all="ignore"):
            l32, h32 = np.float32(l), np.float32(h)
            v = np.float32(int(n)) / (h32 - l32)
        if not np.isfinite(l32) or not np.isfinite(h32) or not h32 > l32:
            raise ValueError("EliteGrid: dims[%d]: lo and hi must be finite binary32 values with lo < hi, not %r, %r" % (i, l, h))
        if not np.isfinite(v) or not v > 0:
            raise ValueError("EliteGrid: dims[%d]: bins / (hi - lo) is not a finite positive binary32 value" % i)
        cells *= int(n)
        if cells > _lib.ELITES_MAX_CELLS:
            raise ValueError("EliteGrid: the product of bins must be at most %d cells" % _lib.ELITES_MAX_CELLS)
        word.append(int(w)); bins.append(int(n)); lo.append(float(l32)); inv.append(float(v))
    return word, bins, lo, inv, cells


class EliteGrid:
    """``n_blocks`` grids of C = the product of the ``bins`` cells over descriptor rows of ``width`` words; ``dims``: one
    ``(word, lo, hi, bins)`` per dimension (1 .. 4), the cell of a row along it being ``int((row[word] - lo) * (bins / (hi - lo)))``
    in binary32, clamped to ``[0, bins - 1]`` (the header states every rounding).  ``like``: an ``MLPPolicy`` whose per-set shapes,
    activation, scale and rays the elites have.  The tensors, zeroed to begin with, all on ``device``:

    ``fitness`` float64 ``[M, C]``, ``desc`` float32 ``[M, C, width]``, ``count`` int32 ``[M, C]`` (a cell is empty iff its count is
    0), ``w1 [M C, D, H]``, ``b1``, ``w2``, ``b2`` (slot ``b C + q`` is one weight set), ``winner`` int32 ``[M, C]`` and, after an
    ``insert`` of G rows, ``cell`` int32 ``[G]``."""

    def __init__(self, n_blocks, dims, width, like, device=None):
        n_blocks, width = int(n_blocks), int(width)
        if n_blocks < 1:
            raise ValueError("EliteGrid: n_blocks must be at least 1, not %r" % (n_blocks,))
        if not 1 <= width <= _lib.ELITES_MAX_WIDTH:
            raise ValueError("EliteGrid: width must be 1 .. %d, not %r" % (_lib.ELITES_MAX_WIDTH, width))
        if not isinstance(like, MLPPolicy):
            raise ValueError("EliteGrid: like must be an MLPPolicy (the shapes of the weight sets the grid keeps)")
        self.word, self.bins, self.lo, self.inv, C_ = _check_dims(dims, width)
        if n_blocks * C_ > 2 ** 31 - 1:
            raise ValueError("EliteGrid: %d blocks of %d cells are more than 2^31 - 1 slots" % (n_blocks, C_))
        self.n_blocks, self.width, self.n_cells, self.dims = n_blocks, width, C_, [tuple(d) for d in dims]
        self.d, self.hidden, self.max_bodies = like.d, like.hidden, like.weight_bodies
        self.like = like
        dev = "cpu" if device is None else device
        slots = n_blocks * C_
        self.fitness = torch.zeros((n_blocks, C_), dtype=torch.float64, device=dev)
        self.device = self.fitness.device                   # (with its index: "cuda" became "cuda:0")
        dev = self.device
        self.desc = torch.zeros((n_blocks, C_, width), dtype=torch.float32, device=dev)
        self.count = torch.zeros((n_blocks, C_), dtype=torch.int32, device=dev)
        self.winner = torch.full((n_blocks, C_), -1, dtype=torch.int32, device=dev)
        self.w1 = torch.zeros((slots, like.d, like.hidden), dtype=torch.float32, device=dev)
        self.b1 = torch.zeros((slots, like.hidden), dtype=torch.float32, device=dev)
        self.w2 = torch.zeros((slots, like.hidden, like.weight_bodies), dtype=torch.float32, device=dev)
        self.b2 = torch.zeros((slots, like.weight_bodies), dtype=torch.float32, device=dev)
        self.filled = torch.zeros(n_blocks, dtype=torch.int32, device=dev)     # n_filled as the last sample / emit wrote it
        self.scratch = torch.zeros((slots * 12 + 7) // 8, dtype=torch.int64, device=dev)
        self.cell = None
        self._keep = None

    # ---- what the grid holds (torch on its own tensors) ----
    @property
    def n_filled(self):
        """int64 ``[M]``: the filled cells of every block"""
        return (self.count != 0).sum(dim=1)

    def coverage(self):
        """float64 ``[M]``: the filled share of every block's cells"""
        return self.n_filled.to(torch.float64) / float(self.n_cells)

    def qd_score(self):
        """float64 ``[M]``: the sum of the fitness over every block's filled cells"""
        return torch.where(self.count != 0, self.fitness, torch.zeros_like(self.fitness)).sum(dim=1)

    def elites(self, block):
        """The ``MLPPolicy`` of the filled cells of ``block``, in ascending cell order (a copy)."""
        b = int(block)
        if not 0 <= b < self.n_blocks:
            raise ValueError("elites: block must be 0 .. %d, not %r" % (self.n_blocks - 1, block))
        q = torch.nonzero(self.count[b] != 0).flatten()
        if q.numel() == 0:
            raise ValueError("elites: block %d has no filled cell" % b)
        sel = q + b * self.n_cells
        return self.like._like(self.w1[sel], self.b1[sel], self.w2[sel], self.b2[sel], None)

    # ---- checkpoints ----
    _STATE = ("fitness", "desc", "count", "w1", "b1", "w2", "b2")

    def state_dict(self):
        return {k: getattr(self, k).clone() for k in self._STATE}

    def load_state_dict(self, state):
        for k in self._STATE:
            have, t = getattr(self, k), state[k]
            if tuple(t.shape) != tuple(have.shape) or t.dtype != have.dtype:
                raise ValueError("load_state_dict: %s must be %s %s, not %s %s" % (k, have.dtype, list(have.shape), t.dtype, list(t.shape)))
        for k in self._STATE:
            getattr(self, k).copy_(state[k])

    # ---- the library's descriptors ----
    @property
    def weights(self):
        """(w1, b1, w2, b2): slot ``b C + q`` of each is cell q of block b"""
        return self.w1, self.b1, self.w2, self.b2

    def _elite_fields(self, e):
        """the grids' state, written into a rem2d_elites or a rem2d_cvt: both name it alike"""
        e.d, e.hidden, e.max_bodies, e.width, e.n_blocks = self.d, self.hidden, self.max_bodies, self.width, self.n_blocks
        e.elite_fitness, e.elite_desc, e.count = self.fitness.data_ptr(), self.desc.data_ptr(), self.count.data_ptr()
        point(e, "elite_", self.weights)
        e.winner, e.n_filled = self.winner.data_ptr(), self.filled.data_ptr()
        e.scratch, e.scratch_bytes = self.scratch.data_ptr(), self.scratch.numel() * 8
        return e

    def _descriptor(self, generation=0, seed=0, rate=0.0, sigma=0.0):
        e = self._elite_fields(_lib.Elites())
        e.n_dims = len(self.word)
        for i in range(len(self.word)):
            e.word[i], e.bins[i], e.lo[i], e.inv[i] = self.word[i], self.bins[i], self.lo[i], self.inv[i]
        e.generation, e.sigma, e.rate_threshold, e.seed, e.reserved = int(generation), float(sigma), rate_threshold(rate), int(seed), 0
        return e

    def _line_descriptor(self, generation, seed, sigma_iso, sigma_line):
        v = self._elite_fields(_lib.Cvt())
        v.n_cells = self.n_cells
        v.generation, v.seed, v.sigma_iso, v.sigma_line, v.splits, v.reserved = int(generation), int(seed), float(sigma_iso), float(sigma_line), 0, 0
        return v

    def _launch(self, name, e, wide):
        """(a call of include/rem2d_cvt.h takes its stream as a member of the descriptor, not as a parameter)"""
        launch(getattr(_lib.lib(wide), name), e, self.device, wide, stream_member=isinstance(e, _lib.Cvt))

    def _fits(self, what, policy, n_sets=None):
        if not isinstance(policy, MLPPolicy) or policy.index is not None:
            raise ValueError("%s: the policy must be an MLPPolicy without an index" % what)
        if (policy.d, policy.hidden, policy.weight_bodies) != (self.d, self.hidden, self.max_bodies):
            raise ValueError("%s: the policy's sets are [%d, %d] -> [%d], the grid's [%d, %d] -> [%d]"
                             % (what, policy.d, policy.hidden, policy.weight_bodies, self.d, self.hidden, self.max_bodies))
        if policy.device != self.device:
            raise ValueError("%s: the policy must be on %s, not %s" % (what, self.device, policy.device))
        if n_sets is not None and policy.n_sets != n_sets:
            raise ValueError("%s: the policy must have %d weight sets, not %d" % (what, n_sets, policy.n_sets))
        if overlaps(policy.weights, self.weights):
            raise ValueError("%s: the policy shares memory with the grid" % what)

    _NOUN, _INSERT = "grid", "rem2d_elites_insert"       # what ``insert`` calls the object, and the library call it queues

    def _insert_descriptor(self, G):
        """the descriptor of an ``insert`` of G rows, with whatever outputs beyond ``cell`` the call has (made here if need be)"""
        return self._descriptor()

    def insert(self, policy, fitness, desc, mask=None, group_size=None, wide=False):
        """File the G evaluated sets of ``policy`` into the grids (rem2d_elites_insert): ``fitness`` float64 ``[G]``, ``desc``
        float32 ``[G, width]``, ``mask`` bool / uint8 ``[G]`` (None: everyone), all on the grid's device; blocks of ``group_size``
        consecutive rows (default G over n_blocks).  Per block and cell the row of greatest fitness (ties: the lowest row; NaN
        fitness and rows with a non-finite selected word are not admitted) replaces the incumbent iff the cell is empty or it is
        strictly better.  Returns ``winner`` int32 ``[M, C]``: the row that took the cell, or -1; ``self.cell`` int32 ``[G]`` is
        every row's cell, -1 for a row that was not admitted."""
        dev = self.device
        self._fits("insert", policy)
        G = policy.n_sets
        if not isinstance(fitness, torch.Tensor) or fitness.dtype != torch.float64:
            raise ValueError("insert: fitness must be a torch.float64 tensor")
        if not is_tensor(fitness, torch.float64, (G,), dev):
            raise ValueError("insert: fitness must be a contiguous tensor of one entry per weight set [%d] on %s, not %s" % (G, dev, list(fitness.shape)))
        if not isinstance(desc, torch.Tensor) or desc.dtype != torch.float32:
            raise ValueError("insert: desc must be a torch.float32 tensor")
        if not is_tensor(desc, torch.float32, (G, self.width), dev):
            raise ValueError("insert: desc must be a contiguous tensor [%d, %d] on %s, not %s" % (G, self.width, dev, list(desc.shape)))
        if group_size is None:
            if G % self.n_blocks:
                raise ValueError("insert: %d rows are not %d blocks of one group_size" % (G, self.n_blocks))
            group_size = G // self.n_blocks
        S = int(group_size)
        if S < 1 or S * self.n_blocks != G:
            raise ValueError("insert: %d rows in groups of %r are not the %s's %d blocks" % (G, group_size, self._NOUN, self.n_blocks))
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8):
                raise ValueError("insert: mask must be a torch.bool or torch.uint8 tensor")
            if not is_tensor(mask, (torch.bool, torch.uint8), (G,), dev):
                raise ValueError("insert: mask must be a contiguous tensor of one entry per row [%d] on %s, not %s" % (G, dev, list(mask.shape)))
        for name in self._STATE:                            # (what a checkpoint holds is what the call reads beside its arguments)
            if overlaps(getattr(self, name), desc):
                raise ValueError("insert: desc shares memory with the %s's %s" % (self._NOUN, name))
        if dev.type != "cuda":
            raise ValueError("insert: the %s is on %s; make it on the GPU (device=...)" % (self._NOUN, dev))
        if self.cell is None or tuple(self.cell.shape) != (G,):
            self.cell = torch.empty(G, dtype=torch.int32, device=dev)
        e = self._insert_descriptor(G)
        e.group_size = S
        e.desc, e.fitness, e.mask = desc.data_ptr(), fitness.data_ptr(), None if mask is None else mask.data_ptr()
        point(e, "", policy.weights)
        e.cell = self.cell.data_ptr()
        self._keep = (policy, fitness, desc, mask)          # (the tensors the queued kernels read)
        self._launch(self._INSERT, e, wide)
        return self.winner

    def _draw(self, what, generation, seed, n_children, parents):
        draw_ok(what, generation, seed)
        n = self.n_blocks if n_children is None else int(n_children)
        if n < 1 or n % self.n_blocks or n > 2 ** 31 - 1:
            raise ValueError("%s: n_children must be a positive multiple of the grid's %d blocks, not %r" % (what, self.n_blocks, n_children))
        if parents is not None and not is_tensor(parents, torch.int32, (n,), self.device):
            raise ValueError("%s: parents must be a contiguous torch.int32 [%d] tensor on %s" % (what, n, self.device))
        return n

    def _emit_checks(self, what, generation, seed, n_children, out):
        """the first checks of ``emit`` and ``emit_line`` -> the number of children (default: those of ``out``, else one per block)"""
        if out is not None:
            self._fits(what, out, None if n_children is None else int(n_children))
            if n_children is None:
                n_children = out.n_sets
        return self._draw(what, generation, seed, n_children, None)

    def _emit_out(self, out, n, indices):
        """``out``, or a new zeroed policy of n sets, with every int32 ``[n]`` attribute named in ``indices``: one it has is reused
        where it is the tensor a kernel can write, else made"""
        dev = self.device
        out = self.like._sets(n, zeroed=True, device=dev) if out is None else self.like._adopt(out)
        for attr in indices:
            if not is_tensor(getattr(out, attr, None), torch.int32, (n,), dev):
                setattr(out, attr, torch.empty(n, dtype=torch.int32, device=dev))
        return out

    def sample(self, generation, seed=0, n_children=None, out=None, wide=False):
        """The draw alone (rem2d_elites_sample): ``parents`` int32 ``[n_children]``, for each child the slot ``b C + q`` of a
        uniformly drawn filled cell of its block -- a function of ``(seed, generation, child)`` and the set of filled cells -- or -1
        where the block's grid is empty; ``n_children`` consecutive children per block, a multiple of n_blocks.  ``self.filled``
        int32 ``[M]`` holds the filled cells it counted.  ``out``: the int32 tensor to write."""
        n = self._draw("sample", generation, seed, n_children, out)
        if self.device.type != "cuda":
            raise ValueError("sample: the grid is on %s; make it on the GPU (device=...)" % self.device)
        if out is None:
            out = torch.empty(n, dtype=torch.int32, device=self.device)
        e = self._descriptor(generation, seed)
        e.n_children, e.parent = n, out.data_ptr()
        self._launch("rem2d_elites_sample", e, wide)
        return out

    def emit(self, generation, seed=0, rate=0.05, sigma=0.1, n_children=None, out=None, wide=False):
        """The next children (rem2d_elites_emit): ``n_children`` sets (a multiple of n_blocks; default: those of ``out``, else one
        per block), child c a copy of the elite ``sample`` draws for it, mutated as ``MLPPolicy.evolve`` mutates -- ``rate`` the
        probability that an element is hit, ``sigma`` the step, the same ``(seed, generation)`` the same bits in every build.  A
        child of a block whose grid is empty keeps the words its buffer holds (zeros in a new one).  ``out``: an ``MLPPolicy`` of
        n_children sets of the grid's shapes whose weights and ``.parents`` are overwritten and which is returned.

        Returns the child ``MLPPolicy`` with ``.parents`` int32 ``[n_children]`` (slots of the grid, or -1)."""
        n = self._emit_checks("emit", generation, seed, n_children, out)
        if not 0.0 <= float(rate) <= 1.0:
            raise ValueError("emit: rate must be in [0, 1], not %r" % (rate,))
        if self.device.type != "cuda":
            raise ValueError("emit: the grid is on %s; make it on the GPU (device=...)" % self.device)
        out = self._emit_out(out, n, ("parents",))
        e = self._descriptor(generation, seed, rate, sigma)
        e.n_children, e.parent = n, out.parents.data_ptr()
        point(e, "child_", out.weights)
        self._launch("rem2d_elites_emit", e, wide)
        return out

    def emit_line(self, generation, seed=0, sigma_iso=0.01, sigma_line=0.2, n_children=None, out=None, wide=False):
        """The next children by the iso+line variation (rem2d_cvt_emit_line; Vassiliades & Mouret 2018): child c descends from TWO
        uniformly drawn elites of its block, ``x1`` (the draw of ``sample`` / ``emit``) and ``x2`` (a draw of its own), as
        ``(x1 + sigma_iso * z) + a * (x2 - x1)``: ``z`` a unit-variance draw per element, ``a = sigma_line * zl`` one draw per child.
        Every element moves; there is no rate.  ``sigma_line = 0`` is ``emit(rate=1.0, sigma=sigma_iso)`` bit for bit.  A child of a
        block whose grid is empty keeps the words its buffer holds.  ``n_children``, ``out``: as ``emit``.

        Returns the child ``MLPPolicy`` with ``.parents`` and ``.parents2`` int32 ``[n_children]`` (slots of the grid, or -1)."""
        n = self._emit_checks("emit_line", generation, seed, n_children, out)
        if not math.isfinite(float(sigma_iso)) or not math.isfinite(float(sigma_line)):
            raise ValueError("emit_line: sigma_iso and sigma_line must be finite, not %r, %r" % (sigma_iso, sigma_line))
        if self.device.type != "cuda":
            raise ValueError("emit_line: the grid is on %s; make it on the GPU (device=...)" % self.device)
        out = self._emit_out(out, n, ("parents", "parents2"))
        v = self._line_descriptor(generation, seed, sigma_iso, sigma_line)
        v.n_children, v.parent, v.parent2 = n, out.parents.data_ptr(), out.parents2.data_ptr()
        point(v, "child_", out.weights)
        self._launch("rem2d_cvt_emit_line", v, wide)
        return out


def assign_host(desc, centroids, chunk=None):
    """The nearest centroid of every row as include/rem2d_cvt.h defines it, in numpy on the host: ``d2 = d2 + (t * t)`` with
    ``t = x_i - y_i`` for ascending i, every operation a binary32 one; the lowest centroid of the least finite d2
    -> (cell int32 [n], dist float32 [n]); cell -1 and dist +inf for a row with no finite candidate."""
    x, y = np.ascontiguousarray(desc, np.float32), np.ascontiguousarray(centroids, np.float32)
    n, B = x.shape
    C_ = y.shape[0]
    cell, dist = np.full(n, -1, np.int32), np.full(n, np.inf, np.float32)
    step = max(1, (1 << 22) // max(C_, 1)) if chunk is None else int(chunk)
    with np.errstate(all="ignore"):
        for r0 in range(0, n, step):
            xs = x[r0:r0 + step]
            d2 = np.zeros((xs.shape[0], C_), np.float32)
            for i in range(B):
                t = xs[:, i, None] - y[None, :, i]
                d2 = d2 + t * t
            assert d2.dtype == np.float32
            d2 = np.where(np.isfinite(d2), d2, np.float32(np.inf))
            q = np.argmin(d2, axis=1)                          # (the first of equal minima: the lowest centroid)
            best = d2[np.arange(xs.shape[0]), q]
            cell[r0:r0 + step] = np.where(best < np.inf, q, -1)
            dist[r0:r0 + step] = best
    return cell, dist


def _check_rows(what, desc, width, dev):
    if not isinstance(desc, torch.Tensor) or desc.dtype != torch.float32:
        raise ValueError("%s: desc must be a torch.float32 tensor" % what)
    if desc.dim() != 2 or desc.shape[1] != width or desc.shape[0] < 1 or not desc.is_contiguous() or desc.device != dev:
        raise ValueError("%s: desc must be a contiguous tensor [n, %d] on %s, not %s on %s" % (what, width, dev, list(desc.shape), desc.device))
    if desc.shape[0] > 2 ** 31 - 1:
        raise ValueError("%s: at most 2^31 - 1 rows" % what)


def _assign(what, desc, centroids, out, dist, scratch, wide=False, splits=0):
    """rem2d_cvt_assign (a GPU device) or assign_host (the CPU) -> (cell, the scratch tensor to keep)"""
    dev = centroids.device
    _check_rows(what, desc, centroids.shape[1], dev)
    n = desc.shape[0]
    for name, t, dt in (("out", out, torch.int32), ("dist", dist, torch.float32)):
        if t is not None and not is_tensor(t, dt, (n,), dev):
            raise ValueError("%s: %s must be a contiguous %s [%d] tensor on %s" % (what, name, dt, n, dev))
    if not 0 <= int(splits) <= _lib.CVT_MAX_SPLITS:
        raise ValueError("%s: splits must be 0 .. %d, not %r" % (what, _lib.CVT_MAX_SPLITS, splits))
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=dev)
    if dev.type != "cuda":
        cell, d = assign_host(desc.numpy(), centroids.numpy())
        out.copy_(torch.from_numpy(cell))
        if dist is not None:
            dist.copy_(torch.from_numpy(d))
        return out, scratch
    if scratch is None or scratch.numel() < n:
        scratch = torch.empty(n, dtype=torch.int64, device=dev)
    v = _lib.Cvt()
    v.width, v.n_cells, v.n_rows, v.splits, v.reserved = centroids.shape[1], centroids.shape[0], n, int(splits), 0
    v.centroids, v.desc, v.cell, v.dist = centroids.data_ptr(), desc.data_ptr(), out.data_ptr(), None if dist is None else dist.data_ptr()
    v.scratch, v.scratch_bytes = scratch.data_ptr(), scratch.numel() * 8
    launch(_lib.lib(wide).rem2d_cvt_assign, v, dev, wide, stream_member=True)
    return out, scratch


def _check_centroids(what, centroids, dev):
    if isinstance(centroids, np.ndarray):
        if centroids.dtype != np.float32:
            raise ValueError("%s: centroids must be float32, not %s" % (what, centroids.dtype))
        centroids = torch.from_numpy(np.ascontiguousarray(centroids))
    if not isinstance(centroids, torch.Tensor) or centroids.dtype != torch.float32 or centroids.dim() != 2:
        raise ValueError("%s: centroids must be a float32 [C, width] array or tensor" % what)
    C_, width = int(centroids.shape[0]), int(centroids.shape[1])
    if not 1 <= C_ <= _lib.CVT_MAX_CELLS:
        raise ValueError("%s: 1 .. %d centroids, not %d" % (what, _lib.CVT_MAX_CELLS, C_))
    if not 1 <= width <= _lib.CVT_MAX_WIDTH:
        raise ValueError("%s: width must be 1 .. %d, not %d" % (what, _lib.CVT_MAX_WIDTH, width))
    return centroids.detach().to(dev).contiguous().clone()


class CentroidArchive(EliteGrid):
    """``n_blocks`` archives of C cells over descriptor rows of ``width`` words, CVT-MAP-Elites (include/rem2d_cvt.h):
    ``centroids`` float32 ``[C, width]`` (1 <= C <= 65536, width <= 32; ``cvt_centroids`` makes them), shared by all blocks; the
    cell of a row is its NEAREST centroid -- squared distance summed word by word in binary32, ties to the lowest centroid, a
    non-finite distance never chosen, no finite one: not admitted.  The tensors are ``EliteGrid``'s, plus ``centroids`` (a copy on
    ``device``) and, after an ``insert``, ``dist`` float32 ``[G]``: every row's squared distance to its centroid.  ``sample``,
    ``emit``, ``emit_line`` and the readings are inherited: to them the archive is a grid of one dimension of C bins."""

    def __init__(self, n_blocks, centroids, like, device=None):
        dev = torch.zeros(0, device="cpu" if device is None else device).device
        cen = _check_centroids("CentroidArchive", centroids, dev)
        C_, width = int(cen.shape[0]), int(cen.shape[1])
        super().__init__(n_blocks, [(0, 0.0, float(C_), C_)], width, like, device=dev)
        self.centroids = cen
        self.dist = None
        self._vscratch = None

    _STATE = EliteGrid._STATE + ("centroids",)

    def assign(self, desc, out=None, dist=None, wide=False, splits=0):
        """The nearest centroid of every row of ``desc`` float32 ``[n, width]`` (rem2d_cvt_assign; on a CPU archive ``assign_host``,
        the same definition in numpy): returns ``out`` int32 ``[n]`` (made if None), -1 for a row with no finite distance;
        ``dist`` float32 ``[n]``, if given, receives the squared distances (+inf beside -1).  ``splits``: the launch shape (0: the
        library's choice); no result depends on it."""
        out, self._vscratch = _assign("assign", desc, self.centroids, out, dist, self._vscratch, wide, splits)
        return out

    _NOUN, _INSERT = "archive", "rem2d_cvt_insert"

    def _insert_descriptor(self, G):
        dev = self.device
        if self.dist is None or tuple(self.dist.shape) != (G,):
            self.dist = torch.empty(G, dtype=torch.float32, device=dev)
        need = (12 * self.n_blocks * self.n_cells + 8 * G + 7) // 8
        if self._vscratch is None or self._vscratch.numel() < need:
            self._vscratch = torch.empty(need, dtype=torch.int64, device=dev)
        v = self._line_descriptor(0, 0, 0.0, 0.0)
        v.centroids, v.dist = self.centroids.data_ptr(), self.dist.data_ptr()
        v.scratch, v.scratch_bytes = self._vscratch.data_ptr(), self._vscratch.numel() * 8
        return v

    def insert(self, policy, fitness, desc, mask=None, group_size=None, wide=False):
        """``EliteGrid.insert`` with the nearest centroid as the cell (rem2d_cvt_insert): the same arguments, checks and return.
        A row is admitted iff it has a finite distance to some centroid, its fitness is not a NaN and the mask admits it;
        ``self.cell`` int32 ``[G]`` holds the cells (-1: not admitted), ``self.dist`` float32 ``[G]`` every row's squared distance."""
        return super().insert(policy, fitness, desc, mask, group_size, wide)


def cvt_centroids(n_cells, lo, hi, n_samples=None, iterations=10, seed=0, device=None, wide=False):
    """Centroids of a centroidal Voronoi tessellation of the box ``[lo, hi)`` (one pair per descriptor word), by Lloyd's algorithm
    (Vassiliades et al. 2018): ``n_samples`` points (default 64 per cell) drawn uniformly in the box from
    ``numpy.random.Generator(PCG64(seed))`` as binary32; the start is the first ``n_cells`` points; each of ``iterations`` rounds
    assigns every point to its nearest centroid -- ``rem2d_cvt_assign`` where ``device`` is a GPU, ``assign_host`` otherwise: one
    definition, the same bits -- and moves every centroid to the mean of its points, accumulated on the host in binary64 in
    ascending point order and rounded to binary32; a centroid without points stays.  Returns float32 ``[n_cells, width]`` on
    ``device`` (default: the CPU), a function of the arguments alone, the same on both routes."""
    C_ = int(n_cells)
    lo32, hi32 = np.atleast_1d(np.asarray(lo, np.float32)), np.atleast_1d(np.asarray(hi, np.float32))
    if lo32.ndim != 1 or lo32.shape != hi32.shape or not 1 <= lo32.shape[0] <= _lib.CVT_MAX_WIDTH:
        raise ValueError("cvt_centroids: lo and hi must be two sequences of 1 .. %d words" % _lib.CVT_MAX_WIDTH)
    if not np.isfinite(lo32).all() or not np.isfinite(hi32).all() or not (hi32 > lo32).all() or not np.isfinite(hi32 - lo32).all():
        raise ValueError("cvt_centroids: lo and hi must be finite binary32 values with lo < hi")
    if not 1 <= C_ <= _lib.CVT_MAX_CELLS:
        raise ValueError("cvt_centroids: n_cells must be 1 .. %d, not %r" % (_lib.CVT_MAX_CELLS, n_cells))
    n = 64 * C_ if n_samples is None else int(n_samples)
    if n < C_ or n > 2 ** 31 - 1:
        raise ValueError("cvt_centroids: n_samples must be n_cells .. 2^31 - 1, not %r" % (n_samples,))
    if int(iterations) < 0:
        raise ValueError("cvt_centroids: iterations must not be negative")
    B = lo32.shape[0]
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    pts = (lo32 + rng.random((n, B), dtype=np.float32) * (hi32 - lo32)).astype(np.float32)
    pts = np.where(pts >= hi32, np.nextafter(hi32, lo32), pts).astype(np.float32)      # (a product rounded up to hi: still inside)
    cen = pts[:C_].copy()
    dev = torch.zeros(0, device="cpu" if device is None else device).device
    on_gpu = dev.type == "cuda"
    if on_gpu:
        pts_d, cen_d = torch.from_numpy(pts).to(dev), torch.empty((C_, B), dtype=torch.float32, device=dev)
        cell_d, scratch = torch.empty(n, dtype=torch.int32, device=dev), None
    pts64 = pts.astype(np.float64)
    for _ in range(int(iterations)):
        if on_gpu:
            cen_d.copy_(torch.from_numpy(cen))
            cell_d, scratch = _assign("cvt_centroids", pts_d, cen_d, cell_d, None, scratch, wide)
            cell = cell_d.cpu().numpy()
        else:
            cell = assign_host(pts, cen)[0]
        ok = cell >= 0
        members = np.bincount(cell[ok], minlength=C_)
        for i in range(B):                                     # (bincount adds in ascending point order, in binary64)
            total = np.bincount(cell[ok], weights=pts64[ok, i], minlength=C_)
            with np.errstate(all="ignore"):
                cen[:, i] = np.where(members > 0, (total / members).astype(np.float32), cen[:, i])
    return torch.from_numpy(cen).to(dev)
