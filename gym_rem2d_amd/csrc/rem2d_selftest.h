// rem2d_selftest.h -- the collision geometry on a table of cases a test chose (include/rem2d_selftest.h).
// Part of the single translation unit rem2d.hip, included LAST: its kernel comes after every other one in the code object, and
// its host code uses what rem2d.hip defines above it (fail, HIP_TRY, host_poly_set).  Not a stand-alone header.
#ifndef REM2D_SELFTEST_KERNEL_H
#define REM2D_SELFTEST_KERNEL_H

#include <rem2d_selftest.h> // the public header (include/)

// One lane per case.  The lane builds the arguments as contact_update_slot and solve_toi_lane do and calls the device functions
// THEY call: collide_* (rem2d_narrowphase.h), gjk_distance, time_of_impact, toi_far_apart (rem2d_toi.h).  No function body is
// restated here.  Plain loads and stores, no LDS, no atomics; speed does not matter.
// (A template for its place alone: the compiler emits the kernels that are template instantiations after the plain ones, in the
// order the source first names them -- rem2d_gather_kernel came last so far -- and as a plain kernel this one would sit in front
// of those and move them.  LANES is the block size.)
template <int LANES> __global__ __launch_bounds__(LANES) void rem2d_selftest_geometry_kernel(int op, int n, const float *cases, int caseWords,
                                                                        float *fout, int *iout) {
    const unsigned i = blockIdx.x * LANES + threadIdx.x;
    if (i >= (unsigned)n) return;
    const float *c = cases + (size_t)i * (size_t)caseWords;
    float *fo = fout + (size_t)i * REM2D_SELFTEST_OUT_WORDS;
    int *io = iout + (size_t)i * REM2D_SELFTEST_OUT_WORDS;
    float f0 = 0.0f, f1 = 0.0f, f2 = 0.0f, f3 = 0.0f, f4 = 0.0f, f5 = 0.0f, f6 = 0.0f, f7 = 0.0f;
    int i0 = 0, i1 = 0, i2 = 0, i3 = 0, i4 = 0, i5 = 0, i6 = 0;
    const int kindA = (int)c[0], shape = (int)c[17];
    if ((kindA != 0 && kindA != 1) || (shape != SHAPE_BOX && shape != SHAPE_CIRCLE)) {
        i0 = -1;
    } else {
        const float hx = c[18], hy = c[19];
        // the static side at the identity: an isolated edge, or a hardcore box as the terrain upload stores it
        Poly4 PA;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            PA.v[k] = mk(c[1 + 2 * k], c[2 + 2 * k]);
            PA.n[k] = mk(c[9 + 2 * k], c[10 + 2 * k]);
        }
        Proxy pA = proxy_edge(PA.v[0], PA.v[1]);
        if (kindA == 1) { pA.v[2] = PA.v[2]; pA.v[3] = PA.v[3]; pA.count = 4; }
        const Proxy pB = proxy_body(shape, hx, hy);
        const float coreR = shape == SHAPE_BOX ? sqrtf(hx * hx + hy * hy) : 0.0f;
        Sweep sw;
        sw.c0 = mk(c[20], c[21]); sw.a0 = c[22]; sw.c = mk(c[23], c[24]); sw.a = c[25];
        const Rot q = rot_set(sw.a0);
        const V2 p = vsub(sw.c0, rmul(q, mk(0.0f, 0.0f)));
        if (op == REM2D_SELFTEST_COLLIDE) {
            Manifold m;
            if (kindA == 1) {
                if (shape == SHAPE_BOX) collide_polygons(m, PA, box_poly(hx, hy), p, q);
                else collide_polygon_circle(m, PA, hx, p);
            } else {
                if (shape == SHAPE_BOX) collide_edge_box(m, PA.v[0], PA.v[1], hx, hy, p, q);
                else collide_edge_circle(m, PA.v[0], PA.v[1], hx, p);
            }
            i0 = m.type; i1 = m.count; i2 = (int)m.k0; i3 = (int)m.k1;
            f0 = m.ln.x; f1 = m.ln.y; f2 = m.lp.x; f3 = m.lp.y; f4 = m.p0.x; f5 = m.p0.y; f6 = m.p1.x; f7 = m.p1.y;
        } else if (op == REM2D_SELFTEST_DISTANCE) {
            SCache cache;
            cache.metric = 0.0f; cache.count = 0; cache.iA0 = cache.iA1 = cache.iA2 = cache.iB0 = cache.iB1 = cache.iB2 = 0;
            XF xfB; xfB.p = p; xfB.q = q;
            f0 = gjk_distance(cache, pA, xf_identity(), pB, xfB);
            f1 = cache.metric;
            i0 = cache.count;
            i1 = cache.count > 0 ? cache.iA0 : -1; i2 = cache.count > 1 ? cache.iA1 : -1; i3 = cache.count > 2 ? cache.iA2 : -1;
            i4 = cache.count > 0 ? cache.iB0 : -1; i5 = cache.count > 1 ? cache.iB1 : -1; i6 = cache.count > 2 ? cache.iB2 : -1;
        } else if (op == REM2D_SELFTEST_TOI) {
            int state;
            float t;
            time_of_impact(state, t, pA, pB, sw);
            i0 = state;
            f0 = t;
        } else {
            i0 = toi_far_apart(pA, pB, sw, shape, hx, hy, coreR) ? 1 : 0;
        }
    }
    fo[0] = f0; fo[1] = f1; fo[2] = f2; fo[3] = f3; fo[4] = f4; fo[5] = f5; fo[6] = f6; fo[7] = f7;
    io[0] = i0; io[1] = i1; io[2] = i2; io[3] = i3; io[4] = i4; io[5] = i5; io[6] = i6; io[7] = 0;
}

extern "C" int rem2d_selftest_abi_version(void) { return REM2D_SELFTEST_ABI_VERSION; }
extern "C" int rem2d_selftest_static_box(const float *xy, float *out16) {
    if (!xy || !out16) return fail(REM2D_E_INVALID, "selftest: NULL argument");
    float vx[4], vy[4], nx[4], ny[4];
    if (!host_poly_set(xy, vx, vy, nx, ny)) return fail(REM2D_E_INVALID, "selftest: the static box must be a convex quad");
    for (int k = 0; k < 4; ++k) {
        out16[2 * k] = vx[k]; out16[2 * k + 1] = vy[k];
        out16[8 + 2 * k] = nx[k]; out16[9 + 2 * k] = ny[k];
    }
    return REM2D_OK;
}
extern "C" int rem2d_selftest_geometry(int32_t op, int32_t n, const float *cases_dev, int32_t case_words, float *fout_dev,
                                       int32_t *iout_dev, int32_t device, void *stream) {
    // (arguments first: nothing is dereferenced or launched before it has been checked)
    if (op < 0 || op >= REM2D_SELFTEST_OP_COUNT) return fail(REM2D_E_INVALID, "selftest: unknown op " + std::to_string(op));
    if (n < 0) return fail(REM2D_E_INVALID, "selftest: n < 0");
    if (case_words < REM2D_SELFTEST_CASE_WORDS)
        return fail(REM2D_E_INVALID, "selftest: case_words must be at least " + std::to_string(REM2D_SELFTEST_CASE_WORDS) + ", not " +
                                         std::to_string(case_words));
    if (n == 0) return REM2D_OK;
    if (!cases_dev || !fout_dev || !iout_dev) return fail(REM2D_E_INVALID, "selftest: NULL device pointer");
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(rem2d_selftest_geometry_kernel<WAVE>, dim3(((unsigned)n + WAVE - 1u) / WAVE), dim3(WAVE), 0, (hipStream_t)stream,
                       (int)op, (int)n, cases_dev, (int)case_words, fout_dev, (int *)iout_dev);
    HIP_TRY(hipGetLastError());
    return REM2D_OK;
}

#endif
