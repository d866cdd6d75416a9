"""Device policies: per-creature MLP controllers evaluated by the library between what the creatures sense and what their joints
are told (include/rem2d_policy.h).

``MLPPolicy`` holds the weights of G controllers -- one per creature, or fewer that creatures share through an ``index`` -- as
float32 tensors.  Its input row is ``BatchedModular2D.observe(max_bodies)`` followed by ``sense_terrain(rays)``, its output one joint
target per body column, ``scale * softsign(.)``, and a validity byte per target (false: not finite, the joint is left alone).
``BatchedModular2D.set_policy`` / ``act`` / ``step_policy`` run it for a population; ``MLPPolicy.forward`` is the kernel alone.

The arithmetic is binary32, one separately rounded operation after the other in a fixed order (the header states it), the same in
every build of the library: what a policy computes is as reproducible as a step.

``RecurrentPolicy`` is the same controller with memory (include/rem2d_recurrent.h): K of its hidden activations are
input words of the next step, carried per creature in device memory that its own kernel reads and rewrites in place.

``ModularPolicy`` is one controller per BODY (include/rem2d_modular.h): the same small network runs for every module
of a creature and exchanges K message words with the module's parent and children, so that one weight set drives any tree.
"""
import math

import numpy as np
import torch

from . import _lib, _tier, control, sense

ABI_VERSION = _lib.POLICY_ABI_VERSION
MAX_HIDDEN = _lib.POLICY_MAX_HIDDEN
ACTIVATIONS = _lib.POLICY_ACTIVATIONS     # index = REM2D_POLICY_SOFTSIGN / REM2D_POLICY_RELU
DEFAULT_SCALE = float(np.float32(math.pi / 2))   # the reference's joint limit, as binary32


def input_width(max_bodies, n_rays):
    """D: words of a policy's input row."""
    return control.width(max_bodies) + int(n_rays)


def _f32(t, what, dims):
    t = torch.as_tensor(t)
    if t.dtype != torch.float32:
        if t.dtype not in (torch.float64, torch.float16, torch.bfloat16):
            raise ValueError("%s must be a float tensor" % what)
        t = t.to(torch.float32)
    if t.dim() == dims - 1:
        t = t.unsqueeze(0)      # one weight set given without its leading axis
    if t.dim() != dims:
        raise ValueError("%s must have %d axes ([G, ...]), not shape %r" % (what, dims, tuple(t.shape)))
    return t.contiguous()


def _check_fitness(what, fitness, n, per, dev):
    """``fitness`` as a kernel reads it: float64 ``[n]`` (one entry per ``per``), contiguous, on ``dev``"""
    if not isinstance(fitness, torch.Tensor) or fitness.dtype != torch.float64:
        raise ValueError("%s: fitness must be a torch.float64 tensor" % what)
    if tuple(fitness.shape) != (n,) or not fitness.is_contiguous():
        raise ValueError("%s: fitness must be a contiguous tensor of one entry per %s [%d], not %s" % (what, per, n, list(fitness.shape)))
    if fitness.device != dev:
        raise ValueError("%s: fitness must be on %s, not %s" % (what, dev, fitness.device))


def _check_ranked(what, fitness, util, n, dev):
    """What an update is ranked by: the children's ``fitness``, or the caller's ``util`` int32 ``[n]``, beside which fitness is not
    looked at"""
    if util is None:
        _check_fitness(what, fitness, n, "child", dev)
    elif not _tier.is_tensor(util, torch.int32, (n,), dev):
        raise ValueError("%s: util must be a contiguous torch.int32 [%d] tensor on %s" % (what, n, dev))


def _check_scratch(what, scratch, need, dev):
    """The caller's ``scratch``, if any: int64, contiguous, on ``dev``, of at least ``need`` bytes"""
    if scratch is not None and (not _tier.is_tensor(scratch, torch.int64, None, dev) or scratch.numel() * 8 < need):
        raise ValueError("%s: scratch must be a contiguous torch.int64 tensor of at least %d entries on %s" % (what, need // 8, dev))


class MLPPolicy:
    """G feed-forward controllers ``x [D] -> softsign / relu -> [H] -> scale * softsign -> [max_bodies]``.

    w1 ``[G, D, H]``, b1 ``[G, H]``, w2 ``[G, H, max_bodies]``, b2 ``[G, max_bodies]`` (a single set may come without the G axis);
    ``max_bodies``, ``H``, ``G`` and the number of rays ``R = D - 8 - 6 * max_bodies`` follow from the shapes.  ``index``: int
    ``[N]``, the weight set of population row r (a value outside ``[0, G)`` leaves that creature to its oscillators); without it
    row r uses set r.  ``rays``: float64 ``[R, 2]`` offsets of the rays whose fractions follow the observation words; default
    ``sense.bipedal_rays()`` when R is 10, none when R is 0."""

    def __init__(self, w1, b1, w2, b2, activation="softsign", scale=None, index=None, rays=None):
        w1, b1, w2, b2 = _f32(w1, "w1", 3), _f32(b1, "b1", 2), _f32(w2, "w2", 3), _f32(b2, "b2", 2)
        G, D, H = (int(v) for v in w1.shape)
        MB = int(w2.shape[2])
        if tuple(b1.shape) != (G, H) or tuple(w2.shape) != (G, H, MB) or tuple(b2.shape) != (G, MB):
            raise ValueError("shapes do not fit: w1 %r b1 %r w2 %r b2 %r (want [G, D, H], [G, H], [G, H, M], [G, M])"
                             % (tuple(w1.shape), tuple(b1.shape), tuple(w2.shape), tuple(b2.shape)))
        if G < 1:
            raise ValueError("a policy needs at least one weight set")
        if not 1 <= MB <= control.MAX_BODIES:
            raise ValueError("max_bodies (w2's last axis) must be 1..%d, not %d" % (control.MAX_BODIES, MB))
        if not 1 <= H <= MAX_HIDDEN:
            raise ValueError("the hidden width must be 1..%d, not %d" % (MAX_HIDDEN, H))
        R = self._ray_inputs(D, MB)
        if activation not in ACTIVATIONS:
            raise ValueError("activation must be one of %r, not %r" % (ACTIVATIONS, activation))
        if len({t.device for t in (w1, b1, w2, b2)}) != 1:
            raise ValueError("the four weight tensors must share a device")
        if rays is None:
            if R == len(sense.bipedal_rays()):
                rays = sense.bipedal_rays()
            elif R != 0:
                raise ValueError("w1 asks for %d rays: pass their offsets as rays=[%d, 2]" % (R, R))
        elif R == 0:
            raise ValueError("rays given, but w1 has no input rows for ray fractions")
        if rays is not None:
            rays = sense.check_rays(rays.detach().cpu().numpy() if isinstance(rays, torch.Tensor) else rays)
            if rays.shape[0] != R:
                raise ValueError("w1 asks for %d rays, rays has %d" % (R, rays.shape[0]))
        if index is not None:
            index = torch.as_tensor(index)
            if index.dim() != 1 or index.dtype in (torch.float16, torch.float32, torch.float64, torch.bool):
                raise ValueError("index must be a 1-d integer tensor")
            index = index.to(device=w1.device, dtype=torch.int32).contiguous()
        self.w1, self.b1, self.w2, self.b2 = w1, b1, w2, b2
        self.activation = activation
        self.scale = DEFAULT_SCALE if scale is None else float(np.float32(scale))
        self.index, self.rays = index, rays
        self.n_sets, self.d, self.hidden, self.max_bodies, self.n_rays = G, D, H, MB, R
        self.weight_bodies = MB  # w2's last axis: what the search operators call max_bodies (a ModularPolicy's is 1, whatever its rows)
        self.parents = None     # int32 [G] on a policy that evolve() made: the set each of its sets came from
        self.util = None        # int32 [M S] on a mean that es_update() made: the utilities of the children it was moved by

    # ---- construction ----
    def _ray_inputs(self, D, MB):
        """R: how many of w1's D input rows are ray fractions (checked)."""
        R = D - control.width(MB)
        if not 0 <= R <= sense.MAX_RAYS:
            raise ValueError("w1 has %d input rows: with max_bodies = %d that must be %d + R, R in 0..%d"
                             % (D, MB, control.width(MB), sense.MAX_RAYS))
        return R

    @classmethod
    def random(cls, n_sets, max_bodies, hidden, n_rays=10, seed=0, std=(0.3, 0.3, 0.5, 0.3), **kw):
        """n_sets controllers with normal weights: w1, b1, w2, b2 drawn in that order from ``numpy.random.default_rng(seed)``, scaled
        by ``std`` (one number, or one per array).  Keyword arguments go to the constructor."""
        return cls._random(n_sets, max_bodies, hidden, n_rays, seed, std, kw)

    @classmethod
    def _random(cls, n_sets, max_bodies, hidden, n_rays, seed, std, kw, more_rows=0, more_args=()):
        """``random`` of this class and of its subclasses: w1 has ``more_rows`` input rows beyond those of ``n_rays`` rays, and the
        constructor takes ``more_args`` after the four arrays."""
        std = (float(std),) * 4 if np.isscalar(std) else tuple(float(s) for s in std)
        rng = np.random.default_rng(seed)
        D = input_width(max_bodies, n_rays) + more_rows
        shapes = ((n_sets, D, hidden), (n_sets, hidden), (n_sets, hidden, max_bodies), (n_sets, max_bodies))
        arrays = [torch.from_numpy((rng.standard_normal(s) * sd).astype(np.float32)) for s, sd in zip(shapes, std)]
        if n_rays not in (0, 10) and "rays" not in kw:
            kw["rays"] = sense.bipedal_rays(n_rays)
        return cls(*arrays, *more_args, **kw)

    def _like(self, w1, b1, w2, b2, index):
        return MLPPolicy(w1, b1, w2, b2, self.activation, self.scale, index, self.rays)

    @property
    def weights(self):
        """(w1, b1, w2, b2)"""
        return self.w1, self.b1, self.w2, self.b2

    def _shapes(self, n):
        """the shapes of w1, b1, w2, b2 of ``n`` sets of this policy's per-set shapes"""
        D, H, MB = self.d, self.hidden, self.weight_bodies
        return (n, D, H), (n, H), (n, H, MB), (n, MB)

    def _sets(self, n, zeroed=False, device=None):
        """A policy like this one of ``n`` new weight sets of its per-set shapes, uninitialised or ``zeroed``, on its device or on
        ``device``"""
        make = torch.zeros if zeroed else torch.empty
        dev = self.device if device is None else device
        return self._like(*(make(shape, dtype=torch.float32, device=dev) for shape in self._shapes(n)), None)

    def _adopt(self, out):
        """``out``, a policy the caller gave to be overwritten, with this policy's activation, scale and rays"""
        out.activation, out.scale, out.rays = self.activation, self.scale, self.rays
        return out

    def _out_ok(self, what, out, n_sets, than, shapes, shares):
        """``out`` checked as the destination of n_sets sets of this policy's per-set shapes that shares no memory with it; the
        caller's wording: out must be another MLPPolicy than ``than``, must have ``shapes``, shares memory with ``shares``."""
        if out is self or not isinstance(out, MLPPolicy):
            raise ValueError("%s: out must be another MLPPolicy than %s" % (what, than))
        dev = self.device
        if out.index is not None or any(a.shape != shape or a.device != dev for a, shape in zip(out.weights, self._shapes(n_sets))):
            raise ValueError("%s: out must have %s, and no index" % (what, shapes))
        if _tier.overlaps(out.weights, self.weights):    # (the library checks it too; here the message can name the argument)
            raise ValueError("%s: out shares memory with %s" % (what, shares))

    def _targets(self, n_rows):
        """New zeroed ``(targets float64 [n_rows, max_bodies], valid uint8 [n_rows, max_bodies])`` for ``forward`` to write"""
        return (torch.zeros((n_rows, self.max_bodies), dtype=torch.float64, device=self.device),
                torch.zeros((n_rows, self.max_bodies), dtype=torch.uint8, device=self.device))

    def take(self, indices):
        """The policy of a selection: weight sets ``indices`` (repeats allowed), in that order, one per creature -- what an EA's
        selection step needs.  With an ``index`` the creatures' sets are resolved through it first."""
        sel = torch.as_tensor(indices, dtype=torch.long, device=self.device)
        if self.index is not None:
            sel = self.index.to(torch.long)[sel]
            if bool(((sel < 0) | (sel >= self.n_sets)).any()):
                raise ValueError("take: a selected creature's index names no weight set")
        return self._like(self.w1[sel], self.b1[sel], self.w2[sel], self.b2[sel], None)

    @property
    def device(self):
        return self.w1.device

    def to(self, device):
        device = torch.device(device)
        if device == self.device:
            return self
        return self._like(self.w1.to(device), self.b1.to(device), self.w2.to(device), self.b2.to(device),
                          None if self.index is None else self.index.to(device))

    def weight_bytes(self):
        """Bytes of one weight set."""
        return 4 * (self.d * self.hidden + self.hidden + self.hidden * self.weight_bodies + self.weight_bodies)

    # ---- the library's descriptor ----
    def descriptor(self, obs, frac, targets, valid, row_mask=None):
        """rem2d_policy over these buffers (checked: contiguous, right dtype and shape, this policy's device)."""
        dev, N = self.device, int(obs.shape[0])

        def ok(t, dtype, shape, what):
            if not _tier.is_tensor(t, dtype, shape, dev):
                raise ValueError("policy: %s must be a contiguous %s %r tensor on %s" % (what, dtype, shape, dev))
        if dev.type != "cuda":
            raise ValueError("policy: the weights are on %s; move the policy to the GPU with .to(device)" % dev)
        ok(obs, torch.float32, (N, control.width(self.max_bodies)), "obs")
        if self.n_rays:
            ok(frac, torch.float32, (N, self.n_rays), "frac")
        ok(targets, torch.float64, (N, self.max_bodies), "targets")
        ok(valid, torch.uint8, (N, self.max_bodies), "valid")
        if row_mask is not None:
            ok(row_mask, torch.uint8, (N,), "row_mask")
        if self.index is not None and int(self.index.shape[0]) != N:
            raise ValueError("policy: index has %d entries for %d rows" % (self.index.shape[0], N))
        if self.index is None and self.n_sets != N:
            raise ValueError("policy: %d weight sets for %d rows (share sets through index=)" % (self.n_sets, N))
        p = _lib.Policy()
        p.d, p.max_bodies, p.n_rays, p.hidden = self.d, self.max_bodies, self.n_rays, self.hidden
        p.activation, p.scale, p.n_sets, p.reserved = ACTIVATIONS.index(self.activation), self.scale, self.n_sets, 0
        _tier.point(p, "", self.weights)
        p.index = None if self.index is None else self.index.data_ptr()
        p.row_mask = None if row_mask is None else row_mask.data_ptr()
        p.obs, p.frac = obs.data_ptr(), (frac.data_ptr() if self.n_rays else None)
        p.targets, p.valid, p.n_rows = targets.data_ptr(), valid.data_ptr(), N
        return p

    def forward(self, obs, frac=None, out=None, row_mask=None, wide=False):
        """The forward pass alone (rem2d_policy_forward) on the current stream: ``obs`` float32 ``[N, 8 + 6 * max_bodies]``, ``frac``
        float32 ``[N, R]`` (None when R is 0) -> ``(targets float64 [N, max_bodies], valid uint8 [N, max_bodies])``.  ``out``: that
        pair to write into (rows a ``row_mask`` uint8 ``[N]`` clears, or whose index names no weight set, keep what they hold);
        without it new zeroed tensors.  ``wide``: the build whose kernel runs (all three write the same bits)."""
        if out is None:
            out = self._targets(int(obs.shape[0]))
        p = self.descriptor(obs, frac, out[0], out[1], row_mask)
        _tier.launch(_lib.lib(wide).rem2d_policy_forward, p, self.device, wide)
        return out

    # ---- the next generation (include/rem2d_evolve.h) ----
    def evolve(self, fitness, generation, seed=0, rate=0.05, sigma=0.1, tournsize=4, group_size=None, elite=0, parents=None, out=None,
               wide=False):
        """The child policy of one generation, made on the device by one library call (rem2d_policy_evolve: tournament selection,
        then per-element mutation; include/rem2d_evolve.h states both) on the current stream; nothing synchronises and the library
        allocates nothing.  ``fitness``: float64 ``[G]`` on the policy's device, one per weight set (NaN loses to everything).
        ``generation``, ``seed``: the random stream -- the same (seed, generation) gives the same children, bit for bit, in every
        build.  ``rate``: the probability that an element is mutated (``floor(rate * 2**32)`` is what the library compares with);
        ``sigma``: the step, the noise has unit variance.  ``tournsize`` 1..4; ``group_size``: sets compete within blocks of that many
        consecutive sets (default: all of them; it must divide G); ``elite=1``: the first child of every block is the block's best
        set, unmutated.  ``parents``: int32 ``[G]`` on the device, the parent of every child -- selection is skipped
        (rem2d_policy_vary) and a value outside ``[0, G)`` leaves that child's words as they are.  ``out``: a policy of the same
        shapes whose buffers -- the weights and, where it has one, ``.parents`` -- are overwritten and which is returned (the
        grandparent, for double buffering); without it new tensors.

        Returns the child ``MLPPolicy`` -- same activation, scale and rays -- with ``.parents``, int32 ``[G]``."""
        dev, G = self.device, self.n_sets
        if self.index is not None:
            raise ValueError("evolve: a policy with an index shares weight sets among creatures; evolve the sets of take() instead")
        _check_fitness("evolve", fitness, G, "weight set", dev)
        S = G if group_size is None else int(group_size)
        if S < 1 or G % S:
            raise ValueError("evolve: group_size must divide the %d weight sets, not %d" % (G, S))
        if not 1 <= int(tournsize) <= _lib.EVOLVE_MAX_TOURNSIZE:
            raise ValueError("evolve: tournsize must be 1..%d, not %r" % (_lib.EVOLVE_MAX_TOURNSIZE, tournsize))
        if elite not in (0, 1):
            raise ValueError("evolve: elite must be 0 or 1, not %r" % (elite,))
        if not 0.0 <= float(rate) <= 1.0:
            raise ValueError("evolve: rate must be in [0, 1], not %r" % (rate,))
        _tier.draw_ok("evolve", generation, seed)
        if parents is not None and not _tier.is_tensor(parents, torch.int32, (G,), dev):
            raise ValueError("evolve: parents must be a contiguous torch.int32 [%d] tensor on %s" % (G, dev))
        if out is not None:
            self._out_ok("evolve", out, G, "the one that is evolved", "this policy's shapes and device", "the policy that is evolved")
        if dev.type != "cuda":
            raise ValueError("evolve: the weights are on %s; move the policy to the GPU with .to(device)" % dev)
        # (with parents= a skipped child keeps what its buffer held: zeros)
        child = self._sets(G, zeroed=parents is not None) if out is None else self._adopt(out)
        if parents is not None:
            child.parents = parents
        elif child.parents is None or child.parents is self.parents:
            child.parents = torch.empty(G, dtype=torch.int32, device=dev)
        e = _lib.Evolve()
        e.d, e.hidden, e.max_bodies, e.n_sets, e.group_size = self.d, self.hidden, self.weight_bodies, G, S
        e.tournsize, e.elite, e.generation = int(tournsize), int(elite), int(generation)
        e.rate_threshold, e.seed, e.sigma, e.reserved = _tier.rate_threshold(rate), int(seed), float(sigma), 0
        e.fitness = fitness.data_ptr()
        _tier.point(e, "", self.weights)
        _tier.point(e, "child_", child.weights)
        e.parent = child.parents.data_ptr()
        L = _lib.lib(wide)
        _tier.launch(L.rem2d_policy_evolve if parents is None else L.rem2d_policy_vary, e, dev, wide)
        return child

    # ---- an evolution strategy around this policy as the mean (include/rem2d_es.h) ----
    def _es_descriptor(self, what, generation, seed, group_size, pair_chunk=0):
        """rem2d_es with this policy's shapes as the mean's, checked; no pointer is set."""
        if self.index is not None:
            raise ValueError("%s: a policy with an index shares weight sets among creatures; the mean is the sets of take() instead" % what)
        if group_size is None or int(group_size) < 2 or int(group_size) % 2:
            raise ValueError("%s: group_size (children per mean) must be even and at least 2, not %r" % (what, group_size))
        if self.n_sets * int(group_size) > 2 ** 31 - 1:
            raise ValueError("%s: %d means of group_size %d are more than 2^31 - 1 children" % (what, self.n_sets, int(group_size)))
        _tier.draw_ok(what, generation, seed)
        if int(pair_chunk) < 0:
            raise ValueError("%s: pair_chunk must be at least 0, not %r" % (what, pair_chunk))
        e = _lib.Es()
        e.d, e.hidden, e.max_bodies, e.n_means, e.group_size = self.d, self.hidden, self.weight_bodies, self.n_sets, int(group_size)
        e.pair_chunk, e.generation, e.reserved, e.seed = int(pair_chunk), int(generation), 0, int(seed)
        return e

    def _es_out(self, what, out, n_sets):
        """``_out_ok`` in the words of a strategy, whose mean this policy is"""
        self._out_ok(what, out, n_sets, "the mean", "%d sets of this policy's shapes on its device" % n_sets, "the mean")

    def es_scratch_bytes(self, group_size, pair_chunk=0, wide=False):
        """Bytes of scratch that ``es_update`` needs for this mean (rem2d_es_scratch_bytes); 0 where the update is one launch."""
        e = self._es_descriptor("es_scratch_bytes", 0, 0, group_size, pair_chunk)
        return _tier.scratch_bytes(_lib.lib(wide).rem2d_es_scratch_bytes, e, wide)

    def es_sample(self, generation, seed=0, sigma=0.1, group_size=None, out=None, wide=False):
        """The children of one generation of an evolution strategy whose mean this policy is: ``group_size`` = S sets around each
        of its M sets, in antithetic pairs -- set ``b S + 2 q`` is ``mean[b] + sigma z`` and set ``b S + 2 q + 1`` is
        ``mean[b] - sigma z`` -- made on the device by one library call (rem2d_es_sample; include/rem2d_es.h states the draw) on the
        current stream; nothing synchronises and the library allocates nothing.  ``generation``, ``seed``: the random stream -- the
        same pair gives the same children, bit for bit, in every build, and ``es_update`` regenerates the same noise from it.
        ``out``: a policy of M S sets of the same per-set shapes whose weights are overwritten and which is returned; without it
        new tensors.

        Returns the child ``MLPPolicy`` of M S sets -- same activation, scale and rays."""
        e = self._es_descriptor("es_sample", generation, seed, group_size)
        G = self.n_sets * e.group_size
        if out is not None:
            self._es_out("es_sample", out, G)
        if self.device.type != "cuda":
            raise ValueError("es_sample: the weights are on %s; move the policy to the GPU with .to(device)" % self.device)
        child = self._sets(G) if out is None else self._adopt(out)
        e.sigma = float(sigma)
        _tier.point(e, "", self.weights)
        _tier.point(e, "child_", child.weights)
        _tier.launch(_lib.lib(wide).rem2d_es_sample, e, self.device, wide)
        return child

    def es_update(self, fitness, generation, seed=0, sigma=0.1, lr=0.05, group_size=None, out=None, scratch=None, util=None,
                  pair_chunk=0, wide=False):
        """The new mean after one generation: the children's ``fitness`` -- float64 ``[M S]`` on the policy's device, in the order of
        ``es_sample`` -- is turned into centred ranks within each block of S (ties averaged, NaN lowest) and the mean moves by
        ``lr / (S sigma)`` times the rank-weighted sum of the noise, which the library regenerates from ``(seed, generation)``: the
        children are not read, no noise was stored, and the sum is exact in 64-bit integers, so the result is the same bits whatever
        the launch shape (rem2d_es_step; include/rem2d_es.h).  On the current stream; nothing synchronises and the library allocates
        nothing.  ``sigma``, ``seed``, ``generation``, ``group_size``: what ``es_sample`` was given.  ``util``: int32 ``[M S]`` on the
        device, the caller's own utilities instead of ranks -- ``fitness`` is not looked at (rem2d_es_update).  ``out``: a policy of
        this policy's shapes whose weights -- and, where it has one, ``.util`` -- are overwritten and which is returned; without it
        new tensors.  ``scratch``: a contiguous int64 tensor of at least ``es_scratch_bytes(group_size, pair_chunk) / 8`` entries
        on the device; without it one is allocated where the update needs it (few means of many children).  ``pair_chunk``: pairs
        per wavefront, 0 for the library's choice; no result depends on it.

        Returns the new mean ``MLPPolicy`` -- same activation, scale and rays -- with ``.util``, int32 ``[M S]``."""
        dev = self.device
        e = self._es_descriptor("es_update", generation, seed, group_size, pair_chunk)
        S = e.group_size
        G = self.n_sets * S
        _check_ranked("es_update", fitness, util, G, dev)
        if not float(sigma) > 0.0 or not math.isfinite(float(sigma)):
            raise ValueError("es_update: sigma must be positive and finite, not %r" % (sigma,))
        need = self.es_scratch_bytes(S, pair_chunk, wide)
        _check_scratch("es_update", scratch, need, dev)
        if out is not None:
            self._es_out("es_update", out, self.n_sets)
        if dev.type != "cuda":
            raise ValueError("es_update: the weights are on %s; move the policy to the GPU with .to(device)" % dev)
        new = self._sets(self.n_sets) if out is None else self._adopt(out)
        if util is not None:
            new.util = util
        elif new.util is None or tuple(new.util.shape) != (G,) or new.util.device != dev or new.util is self.util:
            new.util = torch.empty(G, dtype=torch.int32, device=dev)
        if scratch is None and need:
            scratch = torch.empty(need // 8, dtype=torch.int64, device=dev)
        e.sigma = float(sigma)
        e.step = float(np.float32(float(lr) / (2.0 * (S - 1) * S * float(sigma))))
        e.fitness = None if util is not None else fitness.data_ptr()
        e.util = new.util.data_ptr()
        _tier.point(e, "", self.weights)
        _tier.point(e, "new_", new.weights)
        e.scratch, e.scratch_bytes = (None, 0) if scratch is None else (scratch.data_ptr(), scratch.numel() * 8)
        L = _lib.lib(wide)
        _tier.launch(L.rem2d_es_step if util is None else L.rem2d_es_update, e, dev, wide)
        return new


class RecurrentPolicy(MLPPolicy):
    """G Elman-style partially recurrent controllers (include/rem2d_recurrent.h): an ``MLPPolicy`` whose first
    ``context`` = K hidden activations of one control step are K extra input words of the next.  The weights have the shapes of an
    ``MLPPolicy`` with ``D = 8 + 6 * max_bodies + R + K`` input rows -- the K last rows of w1 are the recurrent weights -- so
    ``R = D - 8 - 6 * max_bodies - K`` and ``1 <= K <= min(H, 64 - R)``.  The context words are not part of the policy: they are a
    float32 ``[N, K]`` tensor per population (``new_memory``; ``BatchedModular2D.set_policy`` keeps one as ``env.policy_memory``),
    which ``forward`` reads and rewrites in place.  To everything that only moves weights about -- ``take``, ``to``, ``evolve``,
    ``es_sample`` / ``es_update``, ``SeparableES``, ``EliteGrid`` -- it is an ordinary weight set of R + K ray inputs, and what those
    return stays a ``RecurrentPolicy`` of the same K."""

    def __init__(self, w1, b1, w2, b2, context, activation="softsign", scale=None, index=None, rays=None):
        if isinstance(context, bool) or not isinstance(context, (int, np.integer)) or int(context) < 1:
            raise ValueError("context (K, the hidden units fed back) must be an integer of at least 1, not %r" % (context,))
        self.context = int(context)
        super().__init__(w1, b1, w2, b2, activation, scale, index, rays)
        if self.context > self.hidden:
            raise ValueError("context = %d is more than the %d hidden units there are to feed back" % (self.context, self.hidden))

    def _ray_inputs(self, D, MB):
        K = self.context
        R = D - control.width(MB) - K
        if R < 0 or R + K > _lib.RECURRENT_MAX_INPUTS:
            raise ValueError("w1 has %d input rows: with max_bodies = %d and context = %d that must be %d + R + %d, R in 0..%d"
                             % (D, MB, K, control.width(MB), K, _lib.RECURRENT_MAX_INPUTS - K))
        return R

    @classmethod
    def random(cls, n_sets, max_bodies, hidden, context, n_rays=10, seed=0, std=(0.3, 0.3, 0.5, 0.3), **kw):
        """As ``MLPPolicy.random``, with ``context`` more input rows in w1: the same draw as an ``MLPPolicy`` of
        ``n_rays + context`` rays."""
        return cls._random(n_sets, max_bodies, hidden, n_rays, seed, std, kw, int(context), (context,))

    def _like(self, w1, b1, w2, b2, index):
        return RecurrentPolicy(w1, b1, w2, b2, self.context, self.activation, self.scale, index, self.rays)

    def new_memory(self, n_rows):
        """Zeroed context words for ``n_rows`` population rows: float32 ``[n_rows, context]`` on the policy's device."""
        return torch.zeros((int(n_rows), self.context), dtype=torch.float32, device=self.device)

    # ---- the library's descriptor ----
    def descriptor(self, obs, frac, targets, valid, memory, reset=None, row_mask=None):
        """rem2d_recurrent over these buffers (checked as ``MLPPolicy.descriptor`` checks its own; ``memory`` float32 ``[N, K]``,
        ``reset`` uint8 or bool ``[N]`` or None)."""
        p = super().descriptor(obs, frac, targets, valid, row_mask)
        dev, N = self.device, int(obs.shape[0])
        if not _tier.is_tensor(memory, torch.float32, (N, self.context), dev):
            raise ValueError("policy: memory must be a contiguous torch.float32 %r tensor on %s" % ((N, self.context), dev))
        if reset is not None and not _tier.is_tensor(reset, (torch.uint8, torch.bool), (N,), dev):
            raise ValueError("policy: reset must be a contiguous torch.uint8 or torch.bool %r tensor on %s" % ((N,), dev))
        q = _lib.Recurrent()
        q.p, q.context, q.reserved = p, self.context, 0
        q.memory, q.reset = memory.data_ptr(), (None if reset is None else reset.data_ptr())
        return q

    def forward(self, obs, frac, memory, reset=None, out=None, row_mask=None, wide=False):
        """The recurrent forward pass alone (rem2d_recurrent_forward) on the current stream: ``obs``, ``frac``, ``out``, ``row_mask``
        and ``wide`` as ``MLPPolicy.forward`` takes them; ``memory`` float32 ``[N, context]`` is the rows' context, read and then
        overwritten IN PLACE with this step's first ``context`` hidden activations; ``reset`` uint8 / bool ``[N]``: a row whose
        entry is set reads +0 for its context whatever memory holds (a new episode).  A row that is skipped keeps its memory too.
        Returns ``(targets, valid)``."""
        if out is None:
            out = self._targets(int(obs.shape[0]))
        q = self.descriptor(obs, frac, out[0], out[1], memory, reset, row_mask)
        _tier.launch(_lib.lib(wide).rem2d_recurrent_forward, q, self.device, wide)
        return out


class ModularPolicy(MLPPolicy):
    """G shared modular controllers (include/rem2d_modular.h): ONE small network that runs once per body of a creature
    instead of once per creature.  It reads the 8 head words of the observation row, the 6 words of its own body, the R ray
    fractions, the body's shape word, its number of children, the sum of its children's ``messages`` = K message words and its
    parent's K message words, and writes that body's joint target and its own next message (its first K hidden activations);
    ``rounds`` = P such exchanges happen per control step.  A weight set is tied to no body column: one set drives creatures of
    any tree.

    The weights have the shapes of an ``MLPPolicy`` of ``max_bodies = 1`` with ``D = 8 + 6 + R + 2 + 2 K`` input rows: w1 ``[G, D, H]``,
    b1 ``[G, H]``, w2 ``[G, H, 1]``, b2 ``[G, 1]``; ``1 <= K <= H``, ``R + 2 + 2 K <= 64``, ``1 <= P <= 8``.  ``max_bodies`` is the ROW
    side's: the body columns of the observation rows, the targets and the topology table (default 16); ``weight_bodies`` is 1.  The
    messages are not part of the policy: they are a float32 ``[N, max_bodies, K]`` tensor per population (``new_memory``;
    ``BatchedModular2D.set_policy`` keeps one as ``env.policy_memory``), which ``forward`` reads and rewrites in place.  To everything
    that only moves weights about -- ``take``, ``to``, ``evolve``, ``es_sample`` / ``es_update``, ``SeparableES``, ``EliteGrid`` /
    ``CentroidArchive`` -- it is an ordinary weight set of one body and R + 2 + 2 K ray inputs, and what those return stays a
    ``ModularPolicy`` of the same K, P and ``max_bodies``.  GRU cells, observation normalisation, streaming and a CPU twin are not
    built."""

    def __init__(self, w1, b1, w2, b2, messages, rounds=1, max_bodies=16, activation="softsign", scale=None, index=None, rays=None):
        if isinstance(messages, bool) or not isinstance(messages, (int, np.integer)) or int(messages) < 1:
            raise ValueError("messages (K, the hidden units handed to the neighbours) must be an integer of at least 1, not %r" % (messages,))
        if isinstance(rounds, bool) or not isinstance(rounds, (int, np.integer)) or not 1 <= int(rounds) <= _lib.MODULAR_MAX_ROUNDS:
            raise ValueError("rounds (P, message exchanges per control step) must be an integer in 1..%d, not %r"
                             % (_lib.MODULAR_MAX_ROUNDS, rounds))
        if isinstance(max_bodies, bool) or not isinstance(max_bodies, (int, np.integer)) or not 1 <= int(max_bodies) <= control.MAX_BODIES:
            raise ValueError("max_bodies (the body columns of a row) must be an integer in 1..%d, not %r" % (control.MAX_BODIES, max_bodies))
        self.messages, self.rounds = int(messages), int(rounds)
        super().__init__(w1, b1, w2, b2, activation, scale, index, rays)
        if self.weight_bodies != 1:
            raise ValueError("a modular weight set drives one body: w2's last axis must be 1, not %d" % self.weight_bodies)
        if self.messages > self.hidden:
            raise ValueError("messages = %d is more than the %d hidden units there are to hand on" % (self.messages, self.hidden))
        self.max_bodies = int(max_bodies)

    def _ray_inputs(self, D, MB):
        K = self.messages
        R = D - control.width(1) - 2 - 2 * K
        if R < 0 or R + 2 + 2 * K > _lib.MODULAR_MAX_INPUTS:
            raise ValueError("w1 has %d input rows: with messages = %d that must be %d + R + 2 + %d, R in 0..%d"
                             % (D, K, control.width(1), 2 * K, _lib.MODULAR_MAX_INPUTS - 2 - 2 * K))
        return R

    @classmethod
    def random(cls, n_sets, hidden, messages, rounds=1, max_bodies=16, n_rays=10, seed=0, std=(0.3, 0.3, 0.5, 0.3), **kw):
        """As ``MLPPolicy.random``, with ``2 + 2 * messages`` more input rows in w1 and one body on the weight side: the same draw
        as ``MLPPolicy.random(n_sets, 1, hidden, n_rays + 2 + 2 * messages)``."""
        return cls._random(n_sets, 1, hidden, n_rays, seed, std, kw, 2 + 2 * int(messages), (messages, rounds, max_bodies))

    def _like(self, w1, b1, w2, b2, index):
        return ModularPolicy(w1, b1, w2, b2, self.messages, self.rounds, self.max_bodies, self.activation, self.scale, index, self.rays)

    def new_memory(self, n_rows):
        """Zeroed messages for ``n_rows`` population rows: float32 ``[n_rows, max_bodies, messages]`` on the policy's device."""
        return torch.zeros((int(n_rows), self.max_bodies, self.messages), dtype=torch.float32, device=self.device)

    # ---- the library's descriptor ----
    def descriptor(self, obs, frac, targets, valid, topo, memory, reset=None, row_mask=None):
        """rem2d_modular over these buffers (checked as ``MLPPolicy.descriptor`` checks its own; ``topo`` int32 ``[N, max_bodies, 2]``,
        ``memory`` float32 ``[N, max_bodies, K]``, ``reset`` uint8 or bool ``[N]`` or None).  The stream is not set."""
        p = super().descriptor(obs, frac, targets, valid, row_mask)
        dev, N = self.device, int(obs.shape[0])
        if not _tier.is_tensor(topo, torch.int32, (N, self.max_bodies, 2), dev):
            raise ValueError("policy: topo must be a contiguous torch.int32 %r tensor on %s" % ((N, self.max_bodies, 2), dev))
        if not _tier.is_tensor(memory, torch.float32, (N, self.max_bodies, self.messages), dev):
            raise ValueError("policy: memory must be a contiguous torch.float32 %r tensor on %s" % ((N, self.max_bodies, self.messages), dev))
        if reset is not None and not _tier.is_tensor(reset, (torch.uint8, torch.bool), (N,), dev):
            raise ValueError("policy: reset must be a contiguous torch.uint8 or torch.bool %r tensor on %s" % ((N,), dev))
        q = _lib.Modular()
        q.p, q.messages, q.rounds = p, self.messages, self.rounds
        q.topo, q.memory, q.reset = topo.data_ptr(), memory.data_ptr(), (None if reset is None else reset.data_ptr())
        return q

    def forward(self, obs, frac, topo, memory, reset=None, out=None, row_mask=None, wide=False):
        """The modular forward pass alone (rem2d_modular_forward) on the current stream: ``obs``, ``frac``, ``out``, ``row_mask`` and
        ``wide`` as ``MLPPolicy.forward`` takes them; ``topo`` int32 ``[N, max_bodies, 2]`` is the creatures' tree in body order
        (``BatchedModular2D.topology``: the parent's body index or -1, and the shape word whose being non-zero makes a slot live;
        any values are safe); ``memory`` float32 ``[N, max_bodies, messages]`` is the bodies' messages, read and then overwritten IN
        PLACE; ``reset`` uint8 / bool ``[N]``: a row whose entry is set reads +0 for its messages whatever memory holds (a new
        episode).  A row that is skipped keeps its memory too; the slots of a row that are not live get target 0, valid 0 and zero
        messages.  Returns ``(targets, valid)``."""
        if out is None:
            out = self._targets(int(obs.shape[0]))
        q = self.descriptor(obs, frac, out[0], out[1], topo, memory, reset, row_mask)
        if int(obs.shape[0]):       # (no row: nothing to do, and an empty tensor has no address to hand over)
            _tier.launch(_lib.lib(wide).rem2d_modular_forward, q, self.device, wide, stream_member=True)
        return out


class SeparableES:
    """An adaptive evolution strategy around an ``MLPPolicy`` as the mean (include/rem2d_snes.h): the antithetic sampling of
    ``MLPPolicy.es_sample`` with a step size PER PARAMETER -- a sigma tensor of the mean's shapes, adapted every update from the
    same utilities (a separable NES) -- and, with ``adam=(beta1, beta2, eps)``, Adam on the mean.  ``mean``: M sets without an
    ``index`` (copied: the caller's tensors are never written); ``group_size`` = S children per set, even, 2 .. 8192.  ``sigma``:
    what every sigma word starts from; ``lr``: the mean's rate (``mean += lr / (S sigma) * sum rank z`` without Adam, Adam's step size
    with it); ``lr_sigma``: sigma's rate (``log sigma += lr_sigma / (2 S) * sum rank (z^2 - 1)``, the exponential in its (1,1) Pade
    form; 0 keeps sigma fixed); ``natural``: the mean's step is scaled by each element's sigma; ``sigma_bounds``: sigma is clamped to
    them.  The object owns two sets of the mean, sigma and (with Adam) the moments m1, m2, which ``update`` writes in turn, the
    update count ``t``, one child policy, one util and one scratch tensor: after the first generation nothing is allocated.
    Everything runs on the device by library calls whose results are the same bits whatever the launch shape; tests/snes_model.py
    restates them."""

    def __init__(self, mean, group_size, sigma=0.1, lr=0.05, lr_sigma=4.0, adam=None, natural=False, sigma_bounds=(1e-6, 10.0)):
        if not isinstance(mean, MLPPolicy):
            raise ValueError("SeparableES: mean must be an MLPPolicy")
        if mean.index is not None:
            raise ValueError("SeparableES: a policy with an index shares weight sets among creatures; the mean is the sets of take() instead")
        S = None if group_size is None else int(group_size)
        if S is None or S < 2 or S % 2 or S > _lib.SNES_MAX_GROUP:
            raise ValueError("SeparableES: group_size (children per mean) must be even and 2..%d, not %r" % (_lib.SNES_MAX_GROUP, group_size))
        if mean.n_sets * S > 2 ** 31 - 1:
            raise ValueError("SeparableES: %d means of group_size %d are more than 2^31 - 1 children" % (mean.n_sets, S))
        if not float(sigma) > 0.0 or not math.isfinite(float(sigma)):
            raise ValueError("SeparableES: sigma must be positive and finite, not %r" % (sigma,))
        if not math.isfinite(float(lr)):
            raise ValueError("SeparableES: lr must be finite, not %r" % (lr,))
        if not float(lr_sigma) >= 0.0 or not math.isfinite(float(lr_sigma)):
            raise ValueError("SeparableES: lr_sigma must be finite and at least 0, not %r" % (lr_sigma,))
        if adam is not None:
            try:
                adam = tuple(float(v) for v in adam)
            except TypeError:
                adam = ()
            if len(adam) != 3 or not 0.0 <= adam[0] < 1.0 or not 0.0 <= adam[1] < 1.0 or not adam[2] > 0.0 or not math.isfinite(adam[2]):
                raise ValueError("SeparableES: adam must be None or (beta1, beta2, eps) with the betas in [0, 1) and eps positive")
        try:
            lo, hi = (float(np.float32(v)) for v in sigma_bounds)
        except (TypeError, ValueError):
            lo, hi = math.nan, math.nan
        if not (0.0 < lo <= hi) or not math.isfinite(hi):
            raise ValueError("SeparableES: sigma_bounds must be finite (min, max) with 0 < min <= max, not %r" % (sigma_bounds,))
        if not lo <= float(sigma) <= hi:
            raise ValueError("SeparableES: sigma %r lies outside sigma_bounds %r" % (sigma, sigma_bounds))
        self.group_size, self.sigma0, self.lr, self.lr_sigma = S, float(sigma), float(lr), float(lr_sigma)
        self.adam, self.natural, self.sigma_bounds = adam, bool(natural), (lo, hi)
        self.t = 0
        own = [t.clone() for t in mean.weights]
        self.mean = mean._like(*own, None)
        self._spare_mean = mean._sets(mean.n_sets)
        self.sigma = [torch.full_like(t, float(sigma)) for t in own]
        self._spare_sigma = [torch.empty_like(t) for t in own]
        self.m1 = self.m2 = self._spare_m1 = self._spare_m2 = None
        if adam is not None:
            self.m1, self.m2 = [torch.zeros_like(t) for t in own], [torch.zeros_like(t) for t in own]
            self._spare_m1, self._spare_m2 = [torch.empty_like(t) for t in own], [torch.empty_like(t) for t in own]
        self._children = self._scratch = self._util = None

    @property
    def device(self):
        return self.mean.device

    @property
    def flags(self):
        return (_lib.SNES_ADAM if self.adam is not None else 0) | (_lib.SNES_NATURAL if self.natural else 0)

    def scalars(self, t):
        """The ten binary32 scalars of update number t = 1, 2, ..., each computed in Python floats and rounded once."""
        S = self.group_size
        f = lambda v: float(np.float32(v))
        c = dict(mstep=f(self.lr / (2.0 * (S - 1) * S * self.sigma0)), sstep=f(self.lr_sigma / (4.0 * (S - 1) * S)), beta1=0.0, omb1=0.0,
                 beta2=0.0, omb2=0.0, alpha=0.0, eps=0.0, sigma_min=self.sigma_bounds[0], sigma_max=self.sigma_bounds[1])
        if self.adam is not None:
            b1, b2, eps = self.adam
            c.update(mstep=f(1.0 / (2.0 * (S - 1) * S)), beta1=f(b1), omb1=f(1.0 - b1), beta2=f(b2), omb2=f(1.0 - b2), eps=f(eps),
                     alpha=f(self.lr * math.sqrt(1.0 - b2 ** int(t)) / (1.0 - b1 ** int(t))))
        return c

    def _descriptor(self, what, generation, seed, pair_chunk=0):
        _tier.draw_ok(what, generation, seed)
        if int(pair_chunk) < 0:
            raise ValueError("%s: pair_chunk must be at least 0, not %r" % (what, pair_chunk))
        m = self.mean
        e = _lib.Snes()
        e.d, e.hidden, e.max_bodies, e.n_means, e.group_size = m.d, m.hidden, m.weight_bodies, m.n_sets, self.group_size
        e.pair_chunk, e.generation, e.flags, e.seed = int(pair_chunk), int(generation), self.flags, int(seed)
        return e

    def scratch_bytes(self, pair_chunk=0, wide=False):
        """Bytes of scratch that ``update`` needs (rem2d_snes_scratch_bytes); 0 where the update is one launch."""
        e = self._descriptor("SeparableES.scratch_bytes", 0, 0, pair_chunk)
        return _tier.scratch_bytes(_lib.lib(wide).rem2d_snes_scratch_bytes, e, wide)

    def sample(self, generation, seed=0, out=None, wide=False):
        """The children of one generation: set ``b S + 2 q`` is ``mean[b] + sigma[b] z`` and set ``b S + 2 q + 1`` is
        ``mean[b] - sigma[b] z``, element by element (rem2d_snes_sample), on the current stream.  ``out``: a policy of M S sets of the
        mean's per-set shapes whose weights are overwritten and which is returned; without it the object's own child policy,
        allocated by the first call and overwritten by every later one."""
        e = self._descriptor("SeparableES.sample", generation, seed)
        G = self.mean.n_sets * self.group_size
        if out is not None:
            self.mean._es_out("SeparableES.sample", out, G)
            if _tier.overlaps(out.weights, self.sigma):
                raise ValueError("SeparableES.sample: out shares memory with sigma")
        if self.device.type != "cuda":
            raise ValueError("SeparableES.sample: the weights are on %s; build the strategy around a mean on the GPU" % self.device)
        if out is None:
            if self._children is None:
                self._children = self.mean._sets(G)
            child = self._children
        else:
            child = self.mean._adopt(out)
        _tier.point(e, "", self.mean.weights)
        _tier.point(e, "sigma_", self.sigma)
        _tier.point(e, "child_", child.weights)
        _tier.launch(_lib.lib(wide).rem2d_snes_sample, e, self.device, wide)
        return child

    def update(self, fitness, generation, seed=0, util=None, scratch=None, pair_chunk=0, wide=False):
        """One update from the children's ``fitness`` -- float64 ``[M S]`` on the device, in the order of ``sample`` -- ranked within
        each block (rem2d_snes_step), or from the caller's ``util`` (int32 ``[M S]`` on the device; ``fitness`` is not looked at:
        rem2d_snes_update).  ``generation``, ``seed``: what ``sample`` was given -- the draws are regenerated, not read.  The new mean,
        sigma and moments go to the object's spare buffers, which then become the current ones; ``t`` counts the update.
        ``scratch``: a contiguous int64 tensor of at least ``scratch_bytes(pair_chunk) / 8`` entries; without it the object's own.
        ``pair_chunk``: pairs per wavefront, 0 for the library's choice; no result depends on it.

        Returns the new mean ``MLPPolicy`` (``self.mean``) with ``.util``, int32 ``[M S]``."""
        dev = self.device
        e = self._descriptor("SeparableES.update", generation, seed, pair_chunk)
        G = self.mean.n_sets * self.group_size
        _check_ranked("SeparableES.update", fitness, util, G, dev)
        need = self.scratch_bytes(pair_chunk, wide)
        _check_scratch("SeparableES.update", scratch, need, dev)
        if dev.type != "cuda":
            raise ValueError("SeparableES.update: the weights are on %s; build the strategy around a mean on the GPU" % dev)
        new = self._spare_mean
        if util is not None:
            new.util = util
        else:                       # (one util per set of buffers, both made by the first call)
            if self._util is None:
                self._util = [torch.empty(G, dtype=torch.int32, device=dev) for _ in range(2)]
            new.util = self._util[self.t % 2]
        if scratch is None and need:
            if self._scratch is None or self._scratch.numel() * 8 < need:
                self._scratch = torch.empty(need // 8, dtype=torch.int64, device=dev)
            scratch = self._scratch
        for k, v in self.scalars(self.t + 1).items():
            setattr(e, k, v)
        e.fitness = None if util is not None else fitness.data_ptr()
        e.util = new.util.data_ptr()
        _tier.point(e, "", self.mean.weights)
        _tier.point(e, "sigma_", self.sigma)
        _tier.point(e, "new_", new.weights)
        _tier.point(e, "new_sigma_", self._spare_sigma)
        if self.adam is not None:
            _tier.point(e, "m1_", self.m1)
            _tier.point(e, "m2_", self.m2)
            _tier.point(e, "new_m1_", self._spare_m1)
            _tier.point(e, "new_m2_", self._spare_m2)
        e.scratch, e.scratch_bytes = (None, 0) if scratch is None else (scratch.data_ptr(), scratch.numel() * 8)
        L = _lib.lib(wide)
        _tier.launch(L.rem2d_snes_step if util is None else L.rem2d_snes_update, e, dev, wide)
        self.mean, self._spare_mean = new, self.mean
        self.sigma, self._spare_sigma = self._spare_sigma, self.sigma
        self.m1, self._spare_m1 = self._spare_m1, self.m1
        self.m2, self._spare_m2 = self._spare_m2, self.m2
        self.t += 1
        return self.mean

    # ---- checkpoints ----
    def state(self):
        """A plain dict for a checkpoint: ``mean``, ``sigma`` and, with Adam, ``m1`` and ``m2`` -- lists of four CPU tensors (w1, b1, w2,
        b2) -- and the update count ``t``."""
        cpu = lambda ts: [t.detach().cpu().clone() for t in ts]
        s = {"mean": cpu(self.mean.weights), "sigma": cpu(self.sigma), "t": int(self.t)}
        if self.adam is not None:
            s["m1"], s["m2"] = cpu(self.m1), cpu(self.m2)
        return s

    def load_state(self, state):
        """Continue from ``state()``'s dict: the tensors are copied into the object's current buffers (same shapes), ``t`` is set."""
        names = ("mean", "sigma") + (("m1", "m2") if self.adam is not None else ())
        mine = {"mean": self.mean.weights, "sigma": self.sigma, "m1": self.m1, "m2": self.m2}
        if not isinstance(state, dict) or any(k not in state for k in names + ("t",)):
            raise ValueError("SeparableES.load_state: state must be a dict with %s and t" % ", ".join(names))
        if isinstance(state["t"], bool) or not isinstance(state["t"], int) or state["t"] < 0:
            raise ValueError("SeparableES.load_state: t must be an integer of at least 0, not %r" % (state["t"],))
        for k in names:
            got = state[k]
            if (not isinstance(got, (list, tuple)) or len(got) != 4 or any(not isinstance(a, torch.Tensor) or a.dtype != torch.float32
                                                                          or a.shape != b.shape for a, b in zip(got, mine[k]))):
                raise ValueError("SeparableES.load_state: %s must be four float32 tensors of the mean's shapes" % k)
        for k in names:
            for a, b in zip(state[k], mine[k]):
                b.copy_(a)
        self.t = state["t"]


class ObsNormalizer:
    """Running mean / standard deviation of the policies' input words, kept on the device in exact integer sums and applied inside
    the forward pass (include/rem2d_obsnorm.h): ARS's "V2", OpenAI-ES's virtual batch normalisation.  A block is
    ``group_size`` consecutive population rows -- row r belongs to block ``r // group_size`` -- and every block has its own
    statistics of the ``Dn = 8 + 6 * max_bodies + n_rays`` words of a row (a ``RecurrentPolicy``'s context words are not normalised).
    ``accumulate`` adds rows to the sums; ``freeze`` turns the sums into the two float32 tables ``mu`` and ``inv`` (``tables``) that
    a normalised forward pass stages a row through: ``clamp((x - mu) * inv, -clip, clip)``.  Until a block holds ``min_count`` rows
    (default: ``max(2, group_size)``) its tables are the identity; a word whose variance stays below ``min_var`` gets ``inv = 0``
    (switched off).  ``clip`` may be ``inf``.  A row with a NaN or an infinite word contributes nothing; words are clamped to
    +-2048 and quantised to 2**-12 on their way into the sums, which makes them exact: the same bits whatever the launch shape, and
    two calls equal one call on the concatenation.

    A block may take ``2**39`` rows in its lifetime.  The object keeps a host-side upper bound (``offered``: the most rows any one
    block can have been given, call by call) and raises ``OverflowError`` before a call that could pass it; ``reset()`` starts
    over.  ``BatchedModular2D.set_policy(policy, normalizer=...)`` attaches one to a population; ``forward`` is the kernel alone."""

    CAPACITY = 2 ** _lib.OBSNORM_CAPACITY_LOG2

    def __init__(self, n_blocks, group_size, max_bodies, n_rays, clip=5.0, min_count=None, min_var=2.0 ** -20, device="cuda"):
        M, S, MB, R = (int(v) for v in (n_blocks, group_size, max_bodies, n_rays))
        if M < 1 or S < 1 or M * S > 2 ** 31 - 1:
            raise ValueError("ObsNormalizer: n_blocks and group_size must be at least 1 and their product at most 2^31 - 1, not %r and %r"
                             % (n_blocks, group_size))
        if not 1 <= MB <= control.MAX_BODIES or not 0 <= R <= sense.MAX_RAYS:
            raise ValueError("ObsNormalizer: max_bodies must be 1..%d and n_rays 0..%d, not %r and %r"
                             % (control.MAX_BODIES, sense.MAX_RAYS, max_bodies, n_rays))
        if not float(clip) > 0.0:
            raise ValueError("ObsNormalizer: clip must be greater than 0 (it may be inf), not %r" % (clip,))
        min_count = max(2, S) if min_count is None else min_count
        if isinstance(min_count, bool) or not isinstance(min_count, (int, np.integer)) or not 1 <= int(min_count) < 2 ** 63:
            raise ValueError("ObsNormalizer: min_count must be an integer of at least 1, not %r" % (min_count,))
        mv = float(np.float32(min_var))
        if not mv > 0.0 or not math.isfinite(mv):
            raise ValueError("ObsNormalizer: min_var must be positive and finite as binary32, not %r" % (min_var,))
        self.n_blocks, self.group_size, self.max_bodies, self.n_rays = M, S, MB, R
        self.width = input_width(MB, R)
        self.clip, self.min_count, self.min_var = float(np.float32(clip)), int(min_count), mv
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.count = torch.zeros(M, dtype=torch.int64, device=dev)
        self.s1, self.s2hi, self.s2lo = (torch.zeros((M, self.width), dtype=torch.int64, device=dev) for _ in range(3))
        self.mu = torch.zeros((M, self.width), dtype=torch.float32, device=dev)
        self.inv = torch.ones((M, self.width), dtype=torch.float32, device=dev)
        self.offered = 0

    @property
    def device(self):
        return self.count.device

    @property
    def tables(self):
        """``(mu, inv)``: float32 ``[n_blocks, Dn]`` each, as the last ``freeze()`` left them (the identity before the first)"""
        return self.mu, self.inv

    def reset(self):
        """Empty sums, identity tables, a fresh capacity."""
        for t in (self.count, self.s1, self.s2hi, self.s2lo, self.mu):
            t.zero_()
        self.inv.fill_(1.0)
        self.offered = 0

    def _offer(self, what, n_rows):
        """Count a call that offers ``n_rows`` rows against the capacity: no block can get more than group_size of them"""
        most = min(int(n_rows), self.group_size)
        if self.offered + most > self.CAPACITY:
            raise OverflowError("%s: a block may have been given %d rows already; %d more could pass the capacity of 2^%d rows per block "
                                "(reset() starts over)" % (what, self.offered, most, _lib.OBSNORM_CAPACITY_LOG2))
        return most

    def descriptor(self, row_chunk=0):
        """rem2d_obsnorm over this object's state and tables; no row, policy or stream is set."""
        n = _lib.Obsnorm()
        n.max_bodies, n.n_rays, n.n_blocks, n.group_size = self.max_bodies, self.n_rays, self.n_blocks, self.group_size
        n.row_chunk, n.context, n.clip, n.min_var, n.min_count, n.n_rows, n.reserved = int(row_chunk), 0, self.clip, self.min_var, self.min_count, 0, 0
        n.count, n.s1, n.s2hi, n.s2lo = (t.data_ptr() for t in (self.count, self.s1, self.s2hi, self.s2lo))
        n.mu, n.inv = self.mu.data_ptr(), self.inv.data_ptr()
        return n

    def _on_gpu(self, what):
        if self.device.type != "cuda":
            raise ValueError("%s: the normaliser is on %s; build it with device='cuda'" % (what, self.device))

    def accumulate(self, obs, frac=None, row_mask=None, row_chunk=0, wide=False):
        """Add rows to the sums (rem2d_obsnorm_accumulate) on the current stream: ``obs`` float32 ``[N, 8 + 6 * max_bodies]``,
        ``frac`` float32 ``[N, n_rays]`` (None when n_rays is 0), ``N <= n_blocks * group_size``; ``row_mask`` uint8 ``[N]``: 0 keeps
        a row out.  ``row_chunk``: rows of a block per wavefront, 0 for the library's choice; no result depends on it."""
        dev = self.device
        if not isinstance(obs, torch.Tensor) or obs.dim() != 2:
            raise ValueError("ObsNormalizer.accumulate: obs must be a 2-d tensor")
        N = int(obs.shape[0])

        def ok(t, dtype, shape, what):
            if not _tier.is_tensor(t, dtype, shape, dev):
                raise ValueError("ObsNormalizer.accumulate: %s must be a contiguous %s %r tensor on %s" % (what, dtype, shape, dev))
        ok(obs, torch.float32, (N, control.width(self.max_bodies)), "obs")
        if self.n_rays:
            ok(frac, torch.float32, (N, self.n_rays), "frac")
        if row_mask is not None:
            ok(row_mask, torch.uint8, (N,), "row_mask")
        if N > self.n_blocks * self.group_size:
            raise ValueError("ObsNormalizer.accumulate: %d rows are more than n_blocks * group_size = %d" % (N, self.n_blocks * self.group_size))
        if not 0 <= int(row_chunk) <= _lib.OBSNORM_MAX_CHUNK:
            raise ValueError("ObsNormalizer.accumulate: row_chunk must be 0..%d, not %r" % (_lib.OBSNORM_MAX_CHUNK, row_chunk))
        most = self._offer("ObsNormalizer.accumulate", N)
        self._on_gpu("ObsNormalizer.accumulate")
        if N == 0:                  # (nothing to add, and an empty tensor has no address to hand over)
            return
        n = self.descriptor(row_chunk)
        n.n_rows, n.obs, n.frac = N, obs.data_ptr(), (frac.data_ptr() if self.n_rays else None)
        n.row_mask = None if row_mask is None else row_mask.data_ptr()
        _tier.launch(_lib.lib(wide).rem2d_obsnorm_accumulate, n, dev, wide, stream_member=True)
        self.offered += most

    def freeze(self, wide=False):
        """The tables of the sums as they stand (rem2d_obsnorm_freeze), on the current stream; returns ``tables``."""
        self._on_gpu("ObsNormalizer.freeze")
        _tier.launch(_lib.lib(wide).rem2d_obsnorm_freeze, self.descriptor(), self.device, wide, stream_member=True)
        return self.tables

    def _fits(self, what, policy, n_rows):
        if not isinstance(policy, MLPPolicy):
            raise ValueError("%s: policy must be an MLPPolicy" % what)
        if policy.max_bodies != self.max_bodies or policy.n_rays != self.n_rays:
            raise ValueError("%s: the policy has max_bodies %d and %d rays, the normaliser %d and %d"
                             % (what, policy.max_bodies, policy.n_rays, self.max_bodies, self.n_rays))
        if policy.device != self.device:
            raise ValueError("%s: the policy is on %s, the normaliser on %s" % (what, policy.device, self.device))
        if int(n_rows) > self.n_blocks * self.group_size:
            raise ValueError("%s: %d rows are more than n_blocks * group_size = %d" % (what, n_rows, self.n_blocks * self.group_size))

    def forward(self, policy, obs, frac=None, memory=None, reset=None, out=None, row_mask=None, wide=False):
        """The normalised forward pass alone (rem2d_obsnorm_forward; with a ``RecurrentPolicy`` rem2d_obsnorm_forward_memory, which
        reads and rewrites ``memory`` in place) on the current stream, under the tables as they stand.  Arguments and return value
        as ``MLPPolicy.forward`` / ``RecurrentPolicy.forward`` take and give them; ``obs`` and ``frac`` are not written."""
        self._fits("ObsNormalizer.forward", policy, obs.shape[0])
        self._on_gpu("ObsNormalizer.forward")
        if out is None:
            out = policy._targets(int(obs.shape[0]))
        n = self.descriptor()
        if isinstance(policy, RecurrentPolicy):
            q = policy.descriptor(obs, frac, out[0], out[1], memory, reset, row_mask)
            n.context, n.memory, n.reset = q.context, q.memory, q.reset
            self._call(_lib.lib(wide).rem2d_obsnorm_forward_memory, n, q.p, wide)
        else:
            self._call(_lib.lib(wide).rem2d_obsnorm_forward, n, policy.descriptor(obs, frac, out[0], out[1], row_mask), wide)
        return out

    def _call(self, fn, n, p, wide):
        """``fn(&n, &p)`` queued on the current stream of the normaliser's device, checked"""
        import ctypes as C
        with torch.cuda.device(self.device):
            n.stream = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(fn(C.byref(n), C.byref(p)), wide)

    # ---- checkpoints ----
    def state(self):
        """A plain dict for a checkpoint: the sums ``count``, ``s1``, ``s2hi``, ``s2lo`` (int64 CPU tensors), the tables ``mu`` and
        ``inv`` (float32 CPU tensors) and ``offered``."""
        s = {k: getattr(self, k).detach().cpu().clone() for k in ("count", "s1", "s2hi", "s2lo", "mu", "inv")}
        s["offered"] = int(self.offered)
        return s

    def load_state(self, state):
        """Continue from ``state()``'s dict: the tensors are copied into the object's buffers (same shapes), ``offered`` is set."""
        names = ("count", "s1", "s2hi", "s2lo", "mu", "inv")
        if not isinstance(state, dict) or any(k not in state for k in names + ("offered",)):
            raise ValueError("ObsNormalizer.load_state: state must be a dict with %s and offered" % ", ".join(names))
        off = state["offered"]
        if isinstance(off, bool) or not isinstance(off, int) or not 0 <= off <= self.CAPACITY:
            raise ValueError("ObsNormalizer.load_state: offered must be an integer in 0..2^%d, not %r" % (_lib.OBSNORM_CAPACITY_LOG2, off))
        for k in names:
            a, b = state[k], getattr(self, k)
            if not isinstance(a, torch.Tensor) or a.dtype != b.dtype or a.shape != b.shape:
                raise ValueError("ObsNormalizer.load_state: %s must be a %s tensor of shape %r" % (k, b.dtype, tuple(b.shape)))
        for k in names:
            getattr(self, k).copy_(state[k])
        self.offered = off
