// rem2d_sense.h -- terrain range sensing (include/rem2d_sense.h): batched ray casts from every creature's root against the track.
// Part of the single translation unit rem2d.hip (see its header comment); not a stand-alone header.
//
// What BipedalWalker calls lidar: for creature e and ray r of a table of binary64 offsets, the fraction of the segment
//     p1 = root (px, py)                       p2 = ((float)((double)px + off[r].x), (float)((double)py + off[r].y))
// at which it first meets a static proxy of the terrain (1.0 = nothing within reach), and optionally which proxy.  The position is
// widened, the offset added in binary64 and the sum narrowed once, as pybox2d does when Python adds to a body.position and hands
// the point back through SWIG (row[6] of observe follows the same convention).  d = p2 - p1 in binary32, maxFraction = 1.
//
// The two ray casts are Box2D 2.3.x's b2EdgeShape::RayCast (two-sided, isolated edges: no ghost vertices) and
// b2PolygonShape::RayCast (the lower / upper clipping loop over the stored normals; the polygon radius plays no part; a ray that
// starts inside has index < 0 and does not hit).  Both are [B2D-recalled] like the rest of the engine:
// restated from memory of the published source, not copied from a checkout.  Statics sit at the origin with the identity rotation,
// so the b2MulT of the input into the shape's frame is dropped.
//
// Closest hit: proxies are scanned in ascending index (creation order: boxes 0 .. nPoly-1, edge i = nPoly + i) and a hit replaces
// the best one only on a strictly smaller fraction, so the lowest index wins a tie (a vertex shared by two edges) and a NaN
// fraction (a non-finite root) never wins: such a creature reads 1.0 / -1.
//
// Arithmetic: every rounded operation is one separately rounded binary32 operation in all three builds.  Spelling them
// __fmul_rn / __fadd_rn is not enough for that: this toolchain defines those as the plain operators, and under -ffp-contract=fast
// the backend fuses a product into the sum that consumes it wherever it finds one (librem2d_fma.so would compute the dots with
// v_fmac_f32).  So a product that can reach a sum goes through sn_keep(), a register move the instruction selector cannot see
// through (an identity DPP move, folded into the consuming v_add_f32 where possible): the same instructions in the three builds.
// sqrtf and `/` are the correctly rounded forms the engine uses (__fsqrt_rn is the hardware's approximate v_sqrt_f32 here).
// Plain C++ loads and stores, no atomics, no LDS, no scratch.
//
// Launch shape: that of observe (rem2d_control.h): CtlTable / ctl_locate, a wavefront = one 64-lane block of one world, the root
// position by __shfl from lane `base`; the R rays of a creature are dealt over the K lanes of its group (lane `sub` takes rays
// sub, sub + K, ...), dead lanes included.
//
// Candidates: the terrain's edges have a (nearly) uniform pitch (rem2d_world_set_terrain verifies |xs[i] - (x0 + i pitch)| <=
// 0.1 pitch), so edge i lies inside index range [i - 0.1, i + 1.1] of fi(x) = (x - x0) / pitch, and a ray whose x-extent is
// [xlo, xhi] can only meet edges floor(fi(xlo) - 0.25) - 1 .. floor(fi(xhi) + 0.25) + 1: the 0.1 the xs may deviate by plus 0.15
// for the rounding of fi and of the hit point, and one more edge on either side.  The bounds are clamped in floating point before
// they become integers (and as integers once more), so a NaN or infinite root yields an empty window, never an index outside the tables.  The boxes (29 on the hardcore
// track) are all tested after a reject of their stored fat AABB (0.11 m beyond the box) against the ray's bounding box.
// The tables (under 10 KB, the same lines for every wavefront) are read through the caches, as `pre` reads them.
#ifndef REM2D_SENSE_KERNELS_H
#define REM2D_SENSE_KERNELS_H

struct SenseTerrain { // a world's Terrain, as the 20 planes of [nStatic] floats rem2d_world_set_terrain uploads behind `base`
    const float *base; // flx fly fux fuy | vx[4] | vy[4] | nx[4] | ny[4]
    int nEdge, nPoly;
    float x0, invPitch;
};
struct SenseTable {
    SenseTerrain t[CTL_TABLE]; // world i of the launch's CtlTable
};

// (sn_keep: rem2d_math.h -- the renderer needs the same move)
DEV float sn_mul(float a, float b) { return sn_keep(__fmul_rn(a, b)); }
DEV float sn_dot(float ax, float ay, float bx, float by) { return __fadd_rn(sn_mul(ax, bx), sn_mul(ay, by)); }

// b2EdgeShape::RayCast [B2D-recalled]: v1 -> v2, ray p1 + t d, maxFraction 1
DEV bool sn_edge(float p1x, float p1y, float dx, float dy, float v1x, float v1y, float v2x, float v2y, float &frac) {
    const float ex = __fsub_rn(v2x, v1x), ey = __fsub_rn(v2y, v1y);
    float nx = ey, ny = -ex;
    const float len = sqrtf(__fadd_rn(sn_mul(nx, nx), sn_mul(ny, ny))); // b2Vec2::Normalize
    if (!(len < B2_EPSILON)) {
        const float inv = 1.0f / len;
        nx = sn_mul(nx, inv);
        ny = sn_mul(ny, inv);
    }
    const float numerator = sn_dot(nx, ny, __fsub_rn(v1x, p1x), __fsub_rn(v1y, p1y));
    const float denominator = sn_dot(nx, ny, dx, dy);
    if (denominator == 0.0f) return false;
    const float t = numerator / denominator;
    if (t < 0.0f || 1.0f < t) return false;
    const float qx = __fadd_rn(p1x, sn_mul(t, dx)), qy = __fadd_rn(p1y, sn_mul(t, dy));
    const float rr = sn_dot(ex, ey, ex, ey);
    if (rr == 0.0f) return false;
    const float s = sn_dot(__fsub_rn(qx, v1x), __fsub_rn(qy, v1y), ex, ey) / rr;
    if (s < 0.0f || 1.0f < s) return false;
    frac = t;
    return true;
}

// b2PolygonShape::RayCast [B2D-recalled] on static proxy s (a quad: vertices and normals at plane stride nS)
DEV bool sn_poly(float p1x, float p1y, float dx, float dy, const float *vx, const float *vy, const float *nx, const float *ny, int s,
                 int nS, float &frac) {
    float lower = 0.0f, upper = 1.0f;
    int index = -1;
    for (int i = 0; i < 4; ++i) {
        const int at = i * nS + s;
        const float nix = nx[at], niy = ny[at];
        const float numerator = sn_dot(nix, niy, __fsub_rn(vx[at], p1x), __fsub_rn(vy[at], p1y));
        const float denominator = sn_dot(nix, niy, dx, dy);
        if (denominator == 0.0f) {
            if (numerator < 0.0f) return false;
        } else {
            if (denominator < 0.0f && numerator < __fmul_rn(lower, denominator)) { // the segment enters this half-space
                lower = numerator / denominator;
                index = i;
            } else if (denominator > 0.0f && numerator < __fmul_rn(upper, denominator)) { // ... leaves it
                upper = numerator / denominator;
            }
        }
        if (upper < lower) return false;
    }
    if (index < 0) return false;
    frac = lower;
    return true;
}

// rays [nRays][2] binary64 offsets; frac [rows][nRays]; hit [rows][nRays] or nullptr
__global__ __launch_bounds__(CTL_THREADS) void rem2d_sense_kernel(CtlTable Tb, SenseTable Ts, const double *rays, int nRays, float *frac,
                                                                   int *hit, long long rows) {
    CtlLane c;
    if (!ctl_locate(Tb, c)) return;
    CTL_SCOPE(c);
    // (every lane of the block loads: the arena is padded to whole blocks, and the shuffles want all lanes)
    const float px = LF(L_PX), py = LF(L_PY);
    const float p1x = __shfl(px, c.base), p1y = __shfl(py, c.base);
    if (!c.inWorld) return;
    const long long r = S.index ? (long long)S.index[env] : (long long)env;
    if (r < 0 || r >= rows) return;
    const SenseTerrain T = Ts.t[c.world];
    const int nS = T.nEdge + T.nPoly;
    const float *flx = T.base, *fly = flx + nS, *fux = fly + nS, *fuy = fux + nS;
    const float *vx = fuy + nS, *vy = vx + 4 * nS, *nx = vy + 4 * nS, *ny = nx + 4 * nS;
    const size_t out = (size_t)r * (size_t)nRays;
    for (int k = c.sub; k < nRays; k += c.K) {
        const float p2x = (float)((double)p1x + rays[2 * k]), p2y = (float)((double)p1y + rays[2 * k + 1]);
        const float dx = __fsub_rn(p2x, p1x), dy = __fsub_rn(p2y, p1y);
        const float xlo = fminf(p1x, p2x), xhi = fmaxf(p1x, p2x), ylo = fminf(p1y, p2y), yhi = fmaxf(p1y, p2y);
        float best = 1.0f;
        int bestAt = -1;
        for (int s = 0; s < T.nPoly; ++s) {
            if (fux[s] < xlo || flx[s] > xhi || fuy[s] < ylo || fly[s] > yhi) continue; // (a NaN rejects nothing)
            float t;
            if (sn_poly(p1x, p1y, dx, dy, vx, vy, nx, ny, s, nS, t) && t < best) {
                best = t;
                bestAt = s;
            }
        }
        // the window of edges the ray's x-extent covers, clamped as floats: NaN -> [0, -1], +inf -> [nEdge, nEdge - 1], -inf -> [0, -1]
        const float filo = sn_mul(__fsub_rn(xlo, T.x0), T.invPitch), fihi = sn_mul(__fsub_rn(xhi, T.x0), T.invPitch);
        const float wlo = fminf(fmaxf(floorf(filo - 0.25f) - 1.0f, 0.0f), (float)T.nEdge);
        const float whi = fminf(fmaxf(floorf(fihi + 0.25f) + 1.0f, -1.0f), (float)(T.nEdge - 1));
        const int i0 = max((int)wlo, 0), i1 = min((int)whi, T.nEdge - 1);
        for (int i = i0; i <= i1; ++i) {
            const int s = T.nPoly + i;
            float t;
            if (sn_edge(p1x, p1y, dx, dy, vx[s], vy[s], vx[nS + s], vy[nS + s], t) && t < best) {
                best = t;
                bestAt = s;
            }
        }
        frac[out + (size_t)k] = best;
        if (hit) hit[out + (size_t)k] = bestAt;
    }
}

#endif
