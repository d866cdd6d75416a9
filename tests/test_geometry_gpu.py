"""The device's narrowphase, GJK, TOI and TOI skip against the oracle on a real MI355X (pytest -m gpu), on the cases of
tests/geometry_forge.py: inputs a test chose, not the pairs of shapes the dynamics produce.

rem2d_selftest_geometry (include/rem2d_selftest.h) runs collide_edge_circle / collide_edge_box / collide_polygons /
collide_polygon_circle, gjk_distance and time_of_impact -- the functions the step kernels call, one lane per case -- and every
output word of every case must equal rem2d_oracle_kat_geometry_batch's: integers exactly, floats with == (so -0 == +0 as
everywhere in this suite, and a NaN fails).  One exception, stated in `same`: a manifold without points is compared by its count
alone, since Box2D leaves its other words undefined.  The default and the wide build are held to this.  librem2d_fma.so is the labelled
tolerance build for engine arithmetic (-ffp-contract=fast): it is NOT held to bits here and not run by this module.

toi_far_apart has no oracle counterpart; what the kernels rely on is the implication
    far_apart == 1  =>  not (oracle state == touching and t < 1)
(solve_toi_lane turns every other answer into alpha = 1).  It is run on every TOI case and on the dense near-miss family, whose
sub-families each hold >= 25 % cases that must NOT be skipped (tests/test_geometry_forge_host.py, CPU) and must each show at least
one skip here, so the implication is not empty.  The shares the skip catches are printed (-s) and recorded in DESIGN.md.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import geometry_forge as G

pytestmark = pytest.mark.gpu

CANARY_F, CANARY_I, PAD = 1234.5, -77, 64
OPS = {"collide": 0, "distance": 1, "toi": 2, "far_apart": 3}


@pytest.fixture(scope="module")
def gpu():
    import replay
    return replay.need_gpu()


@functools.lru_cache(maxsize=None)
def cases(name):
    """(spec, family, oracle fout, oracle iout) of one table; made once, shared by every test, never written to."""
    from oracle import oracle as O
    O.build()
    if name == "collide":
        a, b = G.collide_cases(), G.collide_bulk()
        spec, fam = np.concatenate((a[0], b[0])), np.concatenate((a[1], b[1]))
    else:
        spec, fam = {"distance": G.distance_cases, "toi": G.toi_cases, "near": G.near_miss_cases}[name]()
    fo, io, _ = O.geometry_batch("toi" if name == "near" else name, spec)
    assert np.isfinite(fo).all(), "a case whose oracle output is not finite is a forge error"
    for a in (spec, fam, fo, io):
        a.setflags(write=False)
    return spec, fam, fo, io


def device(torch, op, spec, wide=False, n=None, words=G.DEVICE_WORDS, edit=None):
    """rem2d_selftest_geometry on the table; the outputs sit between canaries, which are checked."""
    from gym_rem2d_amd import _lib
    L = _lib.lib(wide)
    dev = G.device_table(spec, G.library_static_box(L))
    if edit is not None:
        edit(dev)
    if words > G.DEVICE_WORDS:
        dev = np.concatenate((dev, np.full((len(dev), words - G.DEVICE_WORDS), np.nan, np.float32)), axis=1)
    n = len(dev) if n is None else n
    tc = torch.from_numpy(np.ascontiguousarray(dev)).cuda()
    fbuf = torch.full((2 * PAD + len(dev) * G.OUT_WORDS,), CANARY_F, dtype=torch.float32, device="cuda")
    ibuf = torch.full((2 * PAD + len(dev) * G.OUT_WORDS,), CANARY_I, dtype=torch.int32, device="cuda")
    _lib.check(L.rem2d_selftest_geometry(OPS[op], n, tc.data_ptr(), words, fbuf.data_ptr() + 4 * PAD, ibuf.data_ptr() + 4 * PAD, 0,
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)), wide)
    torch.cuda.synchronize()
    f, i = fbuf.cpu().numpy(), ibuf.cpu().numpy()
    used = PAD + n * G.OUT_WORDS
    assert (f[:PAD] == CANARY_F).all() and (f[used:] == CANARY_F).all(), "fout written outside its n rows"
    assert (i[:PAD] == CANARY_I).all() and (i[used:] == CANARY_I).all(), "iout written outside its n rows"
    return f[PAD:used].reshape(n, G.OUT_WORDS), i[PAD:used].reshape(n, G.OUT_WORDS)


def same(got, want, spec, fam, what, manifold=False):
    """manifold: a manifold WITHOUT points carries nothing but its count -- Box2D's routines return early and leave type, normal and
    points as the caller's b2Manifold held them (the oracle's entry point hands in zeros, the device's routines start from
    e_faceA) -- so for count 0 the count alone is compared; with points, every word."""
    (gf, gi), (wf, wi) = got, want
    if manifold:
        empty = (wi[:, 1] == 0) & (gi[:, 1] == 0)
        bad = ~empty & ((gf != wf).any(axis=1) | (gi != wi).any(axis=1))
    else:
        bad = (gf != wf).any(axis=1) | (gi != wi).any(axis=1)
    if bad.any():
        k = int(np.argmax(bad))
        pytest.fail("%s: %d of %d cases differ; first: case %d (%s)\n inputs %r\n device f %r i %r\n oracle f %r i %r" % (
            what, int(bad.sum()), len(bad), k, fam[k], spec[k].tolist(), gf[k].tolist(), gi[k].tolist(), wf[k].tolist(), wi[k].tolist()))


@pytest.mark.parametrize("wide", [False, True], ids=["default", "wide"])
@pytest.mark.parametrize("op", ["collide", "distance", "toi"])
def test_every_word_equals_the_oracle(gpu, op, wide):
    spec, fam, fo, io = cases(op)
    same(device(gpu, op, spec, wide), (fo, io), spec, fam, "%s, %s build" % (op, "wide" if wide else "default"), manifold=op == "collide")


def _bbox_bound(spec):
    """toi_far_apart's first bound, restated in numpy for the REPORT only (which of the two bounds a skip is owed to): the gap
    between the bounding boxes of the static shape and of the swept core disk.  NOT the device's word: the device reports 0 / 1
    only, and an exact "which bound" output would change a function that every step kernel inlines.  Nothing is asserted on it."""
    f = np.float32
    edge = spec[:, 0] == 0
    ax, ay = spec[:, 1:9:2].copy(), spec[:, 2:9:2].copy()
    ax[edge, 2:], ay[edge, 2:] = ax[edge, :1], ay[edge, :1]
    box = spec[:, 9] == 1
    coreR = np.where(box, np.sqrt((spec[:, 10] * spec[:, 10] + spec[:, 11] * spec[:, 11]).astype(f)), f(0)).astype(f)
    blx, bhx = np.minimum(spec[:, 12], spec[:, 15]) - coreR, np.maximum(spec[:, 12], spec[:, 15]) + coreR
    bly, bhy = np.minimum(spec[:, 13], spec[:, 16]) - coreR, np.maximum(spec[:, 13], spec[:, 16]) + coreR
    gap = np.maximum(np.maximum(blx - ax.max(1), ax.min(1) - bhx), np.maximum(bly - ay.max(1), ay.min(1) - bhy))
    total = f(0.01) + np.where(box, f(0.01), spec[:, 10]).astype(f)
    need = np.maximum(f(0.005), total - f(3) * f(0.005)) + f(0.25) * f(0.005)
    return gap > need + f(0.005)


@pytest.mark.parametrize("wide", [False, True], ids=["default", "wide"])
def test_far_apart_skips_no_toi_event(gpu, wide):
    """far_apart == 1 => not (oracle touching and t < 1), on every TOI case and the near-miss family; every near-miss sub-family
    shows at least one skip."""
    report = []
    for name in ("toi", "near"):
        spec, fam, fo, io = cases(name)
        _, gi = device(gpu, "far_apart", spec, wide)
        skip = gi[:, 0]
        assert set(np.unique(skip).tolist()) <= {0, 1}
        event = (io[:, 0] == 3) & (fo[:, 0] < 1.0)
        wrong = (skip == 1) & event
        if wrong.any():
            k = int(np.argmax(wrong))
            pytest.fail("%s: toi_far_apart skips %d pair(s) whose b2TimeOfImpact is an event; first: case %d (%s), oracle touching at "
                        "t = %r\n inputs %r" % (name, int(wrong.sum()), k, fam[k], float(fo[k, 0]), spec[k].tolist()))
        bbox = _bbox_bound(spec)
        for f in sorted(set(fam.tolist())) if name == "near" else ["toi (all)"]:
            m = (fam == f) if name == "near" else np.ones(len(fam), bool)
            alpha1 = m & ~event
            report.append((f, int(m.sum()), int(event[m].sum()), int(alpha1.sum()), int((skip == 1)[alpha1].sum()),
                           int(((skip == 1) & bbox)[alpha1].sum())))
            if name == "near":
                assert (skip == 1)[m].sum() > 0, "%s: the skip never fires" % f
    print("\nfar_apart, %s build: family | cases | events | alpha = 1 | skipped | of those by the bounding-box bound (numpy restatement)" % ("wide" if wide else "default"))
    for r in report:
        print("| %s | %d | %d | %d | %d | %d |" % r)


def test_launch_edges(gpu):
    """n = 0 writes nothing; an n that is no multiple of 64 writes its n rows and no more (the canaries in `device`); a wider
    row stride reads the same 26 words; a case with an unknown kind or shape answers -1."""
    spec, fam, fo, io = cases("toi")
    sub = np.ascontiguousarray(spec[:1000])
    f0, i0 = device(gpu, "toi", sub, n=0)
    assert f0.shape == (0, G.OUT_WORDS) and i0.shape == (0, G.OUT_WORDS)
    for n in (1, 63, 65, 131):
        gf, gi = device(gpu, "toi", sub, n=n)
        assert (gf == fo[:n]).all() and (gi == io[:n]).all(), n
    gf, gi = device(gpu, "toi", sub, n=131, words=G.DEVICE_WORDS + 5)
    assert (gf == fo[:131]).all() and (gi == io[:131]).all()
    def odd(dev):
        dev[0, 0], dev[1, 17] = 7, 0
    gf, gi = device(gpu, "collide", sub[:4], edit=odd)
    assert gi[0, 0] == -1 and gi[1, 0] == -1 and (gi[:2, 1:] == 0).all() and (gf[:2] == 0).all() and (gi[2:, 0] >= 0).all()
