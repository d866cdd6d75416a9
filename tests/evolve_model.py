"""Evolving device policies stated on the host (include/rem2d_evolve.h), shared by tests/test_evolve_host.py (numpy alone) and
tests/test_evolve_gpu.py: what policy_model.py is for the forward pass.  Written from the header, not from the kernel.

* ``philox``: Philox4x32-10 on uint32 arrays (the 32 x 32 -> 64 bit products in uint64).
* ``select_model``: parent int32 [G] -- the elite rule and the tournament, on the header's order on fitness.
* ``vary_model``: the four child arrays from the four parent arrays and ``parent``, plus the hit masks.  The noise is integer
  arithmetic up to the exact conversion ``(float)s``; then `w + (sigma * (s * C))` on float32 arrays, which numpy evaluates as
  separately rounded products and one rounded sum.

NaNs: a hit whose result is a NaN (a NaN parent word, inf * 0, inf - inf) has no defined sign or payload and the host's and the
device's arithmetic choose differently, so ``bits`` maps the NaNs AT HIT ELEMENTS to one pattern before a comparison.  A missed
element and an elite child's are bit copies and are compared as they are, NaN payloads included.
"""
import numpy as np

f32 = np.float32
u32, u64 = np.uint32, np.uint64
M0, M1 = u64(0xD2511F53), u64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
NOISE_SCALE = np.array([0x37B504F3], u32).view(f32)[0]     # fl32(sqrt 2) * 2^-16
NOISE_BIAS = 196605
MASK32 = u64(0xffffffff)
SELECT, W1_DOMAIN = 0, 1                                   # domains: selection, then w1, b1, w2, b2 = 1 .. 4


def philox(counter, key):
    """counter: four uint32 arrays (or scalars) that broadcast together, key: two -> x0 .. x3 uint32 arrays"""
    c = [np.asarray(v, u64) & MASK32 for v in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                      # < 2^64: no wrap
        c = [(p1 >> u64(32)) ^ c[1] ^ u64(k0), p1 & MASK32, (p0 >> u64(32)) ^ c[3] ^ u64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return [v.astype(u32) for v in c]


def seed_key(seed):
    seed = int(seed)
    return seed & 0xffffffff, (seed >> 32) & 0xffffffff


def rate_threshold(rate):
    """floor(rate * 2^32) as the caller computes it (rate a binary64 in [0, 1]: the product is exact)"""
    return int(np.floor(float(rate) * 4294967296.0))


def greater(a, b):
    """a above b in the order on fitness: NaN below everything and equal to itself, -0 == +0"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore"):
        return ~np.isnan(a) & (np.isnan(b) | (a > b))


def select_model(fitness, group_size, tournsize, elite, seed, generation, late_ties=False):
    """parent int32 [G].  late_ties: the WRONG tournament whose ties go to the later aspirant (for the teeth test)"""
    fit = np.asarray(fitness, np.float64)
    G, S = fit.shape[0], int(group_size)
    assert S >= 1 and G % S == 0 and 1 <= tournsize <= 4
    c = np.arange(G, dtype=np.int64)
    base = (c // S) * S
    x = philox((0, c, generation, SELECT), seed_key(seed))
    asp = [base + ((xk.astype(u64) * u64(S)) >> u64(32)).astype(np.int64) for xk in x]
    win = asp[0].copy()
    for k in range(1, tournsize):
        better = greater(fit[asp[k]], fit[win])
        if late_ties:
            better = ~greater(fit[win], fit[asp[k]])
        win = np.where(better, asp[k], win)
    if elite:
        for b in range(0, G, S):
            best = b
            for i in range(b + 1, b + S):
                if greater(fit[i], fit[best]):
                    best = i
            win[b] = best
    return win.astype(np.int32)


def noise(x1, x2, x3):
    """z float32 of the draws: (float)s * C, s the sum of the six 16-bit halves minus 196605"""
    s = np.zeros(np.shape(x1), np.int64)
    for x in (x1, x2, x3):
        s += (x & u32(0xffff)).astype(np.int64) + (x >> u32(16)).astype(np.int64)
    s -= NOISE_BIAS
    sf = s.astype(f32)
    assert np.array_equal(sf.astype(np.int64), s)          # exact in binary32
    return sf * NOISE_SCALE


def draws(n, child, domain, seed, generation):
    """the Philox words of elements 0 .. n-1 of array `domain` of child set `child`"""
    return philox((np.arange(n, dtype=np.int64), child, generation, domain), seed_key(seed))


def mutate_set(w, child, domain, threshold, sigma, seed, generation):
    """one array of one set (any shape, C order) -> (child words float32, hit mask)"""
    flat = np.ascontiguousarray(w, f32).reshape(-1)
    x0, x1, x2, x3 = draws(flat.size, child, domain, seed, generation)
    hit = x0.astype(u64) < u64(threshold)
    with np.errstate(all="ignore"):
        z = noise(x1, x2, x3)
        moved = flat + (f32(sigma) * z)
    assert moved.dtype == f32 and z.dtype == f32
    out = flat.copy()
    out[hit] = moved[hit]
    return out.reshape(np.shape(w)), hit.reshape(np.shape(w))


def vary_model(weights, parent, group_size, elite, threshold, sigma, seed, generation, before=None):
    """weights: (w1 [G, D, H], b1 [G, H], w2 [G, H, MB], b2 [G, MB]); parent int [G]
    -> (children: four arrays, hits: four bool arrays, written: bool [G]).  A child whose parent lies outside [0, G) keeps what
    ``before`` (four arrays, default zeros) holds and is not `written`."""
    weights = [np.asarray(a, f32) for a in weights]
    G, S = weights[0].shape[0], int(group_size)
    parent = np.asarray(parent, np.int64)
    written = (parent >= 0) & (parent < G)
    kids = [np.zeros_like(a) if before is None else np.array(before[k], f32) for k, a in enumerate(weights)]
    hits = [np.zeros(a.shape, bool) for a in weights]
    for c in range(G):
        if not written[c]:
            continue
        for k, a in enumerate(weights):
            src = a[parent[c]]
            if elite and c % S == 0:
                kids[k][c] = src
            else:
                kids[k][c], hits[k][c] = mutate_set(src, c, W1_DOMAIN + k, threshold, sigma, seed, generation)
    return kids, hits, written


def evolve_model(weights, fitness, group_size, tournsize, elite, threshold, sigma, seed, generation):
    """select, then vary -> (children, hits, parent)"""
    parent = select_model(fitness, group_size, tournsize, elite, seed, generation)
    kids, hits, _ = vary_model(weights, parent, group_size, elite, threshold, sigma, seed, generation)
    return kids, hits, parent


def bits(a, hits=None):
    """float32 array -> uint32 words; with ``hits``, the NaNs at hit elements mapped to one pattern"""
    a = np.array(a, f32)
    if hits is not None:
        a[np.isnan(a) & hits] = f32("nan")
    return a.view(u32)


# --------------------------------------------------------------------------------------------- an episode under given weights
def episode_replay(O, terrain, morphs, rows, weights, flags, n_steps, max_bodies):
    """The oracle's closed loop of policy_model.policy_loop_run, under the weight sets ``weights`` (four arrays in POPULATION order;
    ``rows[k]``: the population indices of lane bucket ``morphs[k]``), from reset, n_steps steps
    -> (fitness float64 [n], gone bool [n]: the creature outgrew the default build's contact slots on the way)."""
    import control_model as M
    import policy_model as PM
    import range_model as R
    T = R.Terrain.of(terrain)
    rays = R.bipedal_rays()
    n = sum(len(r) for r in rows)
    fitness, gone = np.zeros(n, np.float64), np.zeros(n, bool)
    for morph, r in zip(morphs, rows):
        loop = M.OracleLoop(O, terrain, morph, flags, "replay")
        ctx = loop.ctx
        W = [a[np.asarray(r)] for a in weights]
        run = dict(ctx=ctx, caps=[], obs=[])
        for t in range(n_steps + 1):
            snap = loop.snapshot()
            run["obs"].append(None)
            run["caps"].append(np.stack([snap["ccount"].max(axis=1),
                                         ((snap["ctouch"] != 0) & M.F.masks(ctx, snap)["cedge"]).sum(axis=0).max(axis=1)], 1))
            if t == n_steps:
                break
            obs = M.observe_model(ctx, snap, max_bodies)
            frac = R.cast(T, snap["px"][:, 0], snap["py"][:, 0], rays)[0]
            tg, valid = PM.forward_model(PM.input_rows(obs, frac), *W)
            loop.set_targets(tg, mask=valid)
            loop.step()
        fitness[r] = loop.env["fitness"]
        gone[r] = M.left_out_first(run)[0] < len(run["obs"])
    return fitness, gone
