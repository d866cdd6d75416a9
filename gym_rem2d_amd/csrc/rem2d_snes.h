// rem2d_snes.h -- an adaptive evolution strategy for device policies (include/rem2d_snes.h): the ES's antithetic sampling with one
// sigma word per word of the mean, the update of sigma from the second moment of the regenerated draws and, on request, Adam on
// the mean.  Part of the single translation unit rem2d.hip (see its header comment); not a stand-alone header.
//
// Everything of rem2d_es.h that fits is reused by call: ev_philox, es_sum, es_item, es_key and rem2d_es_shape_kernel; SnArgs
// carries an EsArgs for them.  The draws are the ES's, and like the ES's update this one REGENERATES them: g = sum d s and
// h = sum p (s^2 - 2^31) are exact int64 sums whose value does not depend on how the pairs are dealt over lanes and launches.
//
// rem2d_snes_sample_kernel: rem2d_es_sample_kernel with a second load, the sigma word: a workgroup is ONE wavefront that owns one
// pair of children, V = 4 (dwordx4) where the per-set length is a multiple of 4 and the three bases are 16-byte aligned, V = 1
// otherwise.  No LDS, no atomics.
//
// rem2d_snes_update_kernel: a workgroup is ONE wavefront whose lanes take 64 consecutive elements of one array of one block, for
// one chunk of the block's pairs.  util[a] and util[a + 1] are the same in every lane -- scalar loads -- and a pair whose d AND p
// are 0 is skipped as a whole, Philox block included.  One Philox block per live pair serves both sums:
//   g += d * s            one 32 x 32 + 64 multiply-add (v_mad_i64_i32)
//   hs += p * (s * s)     s * s < 2^36 is one 32 x 32 -> 64 multiply; the product with the sign-extended p is a 64-bit
//                         multiply-add modulo 2^64 (one 32 x 32 + 64 multiply-add and the high word's 32-bit products, whose p
//                         halves are scalars)
// and the - 2^31 is taken out of the loop: h = hs - (sum of the live p) * 2^31 modulo 2^64, the sum of p being the same in every
// lane (scalar adds).  In the ring of integers modulo 2^64 that is the header's sum, whatever util holds.  In the compiled loop
// the second sum is four vector multiplies (one v_mad_i64_i32, one v_mad_u64_u32, two v_mul_lo_u32) beside the seventeen of the
// Philox block and the first sum.  Without a split (one chunk) the wavefront applies the update itself;
// otherwise its two partials go to the caller's scratch, [block][chunk][2][element], and rem2d_snes_finish_kernel sums a block's
// chunks and applies them.  Plain vector stores, no atomics, no LDS.
//
// Arithmetic: every product goes through sn_mul (rem2d_sense.h), so that -ffp-contract=fast finds nothing to fuse; sqrtf and `/`
// are the correctly rounded forms, as rem2d_sense.h notes.
#ifndef REM2D_SNES_KERNELS_H
#define REM2D_SNES_KERNELS_H

struct SnArgs {
    EsArgs es;            // fitness, util, mean, child, next (the new mean), scratch, the shapes and the split; es.sigma, es.step unused
    const float *sigma[4];
    const float *m1[4], *m2[4];
    float *nextSigma[4];
    float *nextM1[4], *nextM2[4];
    unsigned flags;
    float mstep, sstep, beta1, omb1, beta2, omb2, alpha, eps, sigmaMin, sigmaMax;
};

// ------------------------------------------------------------------------------------------------------------------- sample
template <int V> DEV void sn_sample_array(const float *mean, const float *sigma, float *even, float *odd, int n, unsigned anchor, unsigned domain,
                                          const EsArgs &A, int lane) {
    for (int i = lane * V; i < n; i += WAVE * V) { // (n is a multiple of V where V is 4: the host's choice)
        EvVec<V> m, sg, e, o;
        m.load(mean + i);
        sg.load(sigma + i);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int s = es_sum(ev_philox((unsigned)(i + v), anchor, A.generation, domain, A.key0, A.key1));
            const float t = sn_mul(sg.v[v], sn_mul((float)s, __uint_as_float(EV_NOISE_SCALE)));
            e.v[v] = __fadd_rn(m.v[v], t);
            o.v[v] = __fadd_rn(m.v[v], -t);
        }
        e.store(even + i);
        o.store(odd + i);
    }
}

__global__ __launch_bounds__(WAVE) void rem2d_snes_sample_kernel(SnArgs B) {
    const EsArgs &A = B.es;
    const int lane = (int)threadIdx.x;
    const long long a = 2ll * (A.itemBase + (long long)blockIdx.x); // the anchor; < M S: the grid is pairs
    const int b = (int)(a / (long long)A.S);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float *mean = A.mean[k] + (size_t)b * (size_t)A.len[k];
        const float *sigma = B.sigma[k] + (size_t)b * (size_t)A.len[k];
        float *even = A.child[k] + (size_t)a * (size_t)A.len[k];
        if (A.vec[k]) sn_sample_array<4>(mean, sigma, even, even + A.len[k], A.len[k], (unsigned)a, ES_DOMAIN0 + 1u + (unsigned)k, A, lane);
        else sn_sample_array<1>(mean, sigma, even, even + A.len[k], A.len[k], (unsigned)a, ES_DOMAIN0 + 1u + (unsigned)k, A, lane);
    }
}

// ------------------------------------------------------------------------------------------------------------------- update
// the new words of element `at` of array k from the old ones and the two exact sums: the header's operations in the header's order
DEV void sn_apply(const SnArgs &B, int k, size_t at, long long g, long long h) {
    const float m = B.es.mean[k][at], sg = B.sigma[k][at];
    const float G = sn_mul(__double2float_rn(__ll2double_rn(g)), __uint_as_float(EV_NOISE_SCALE));
    const float Hh = sn_mul(__double2float_rn(__ll2double_rn(h)), 4.656612873077392578125e-10f); // 2^-31
    float x = sn_mul(B.sstep, Hh);
    if (x != x) x = 0.0f;
    else x = x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x);
    const float f = __fadd_rn(2.0f, x) / __fsub_rn(2.0f, x);
    float sn = sn_mul(sg, f);
    sn = sn < B.sigmaMin ? B.sigmaMin : (sn > B.sigmaMax ? B.sigmaMax : sn); // (a NaN fails both tests: it passes through)
    B.nextSigma[k][at] = sn;
    const float t = (B.flags & REM2D_SNES_NATURAL) ? sn_mul(sg, G) : G; // the OLD sigma
    const float gh = sn_mul(B.mstep, t);
    if (B.flags & REM2D_SNES_ADAM) {
        const float a1 = __fadd_rn(sn_mul(B.beta1, B.m1[k][at]), sn_mul(B.omb1, gh));
        const float a2 = __fadd_rn(sn_mul(B.beta2, B.m2[k][at]), sn_mul(B.omb2, sn_mul(gh, gh)));
        B.nextM1[k][at] = a1;
        B.nextM2[k][at] = a2;
        B.es.next[k][at] = __fadd_rn(m, sn_mul(B.alpha, a1 / __fadd_rn(sqrtf(a2), B.eps)));
    } else {
        B.es.next[k][at] = __fadd_rn(m, gh);
    }
}

__global__ __launch_bounds__(WAVE) void rem2d_snes_update_kernel(SnArgs B) {
    const EsArgs &A = B.es;
    const int lane = (int)threadIdx.x;
    const EsItem it = es_item(A, A.itemBase + (long long)blockIdx.x, A.nChunks, lane);
    const int P = A.S >> 1;
    const int q0 = (int)((long long)it.ch * (long long)A.pairChunk);
    const int q1 = (long long)q0 + (long long)A.pairChunk < (long long)P ? q0 + A.pairChunk : P;
    const int *__restrict__ u = A.util + (size_t)it.b * (size_t)A.S;
    const unsigned base = (unsigned)((long long)it.b * (long long)A.S), domain = ES_DOMAIN0 + 1u + (unsigned)it.k;
    long long g = 0;
    unsigned long long hs = 0, psum = 0; // hs: sum of p s^2; psum: sum of p (sign-extended), the same in every lane
    for (int q = q0; q < q1; ++q) {
        const unsigned ua = (unsigned)u[2 * q], ub = (unsigned)u[2 * q + 1]; // the same in every lane
        const int d = (int)(ua - ub), p = (int)(ua + ub);                    // modulo 2^32, as the header says
        if ((d | p) == 0) continue;
        const int s = es_sum(ev_philox((unsigned)it.i, base + 2u * (unsigned)q, A.generation, domain, A.key0, A.key1));
        g += (long long)d * (long long)s;
        hs += (unsigned long long)(long long)p * (unsigned long long)((long long)s * (long long)s);
        psum += (unsigned long long)(long long)p;
    }
    const long long h = (long long)(hs - (psum << 31));
    const int n = A.len[it.k];
    if (it.i >= n) return;
    if (A.nChunks == 1) {
        sn_apply(B, it.k, (size_t)it.b * (size_t)n + (size_t)it.i, g, h);
    } else {
        long long *out = A.scratch + ((size_t)it.b * (size_t)A.nChunks + (size_t)it.ch) * 2 * (size_t)A.E + (size_t)(A.off[it.k] + it.i);
        out[0] = g;
        out[A.E] = h;
    }
}

// the chunks' partial sums of one element, summed and applied; items are ordered [block][slot]
__global__ __launch_bounds__(WAVE) void rem2d_snes_finish_kernel(SnArgs B) {
    const EsArgs &A = B.es;
    const int lane = (int)threadIdx.x;
    const EsItem it = es_item(A, A.itemBase + (long long)blockIdx.x, 1, lane);
    const int n = A.len[it.k];
    if (it.i >= n) return;
    const long long *p = A.scratch + (size_t)it.b * (size_t)A.nChunks * 2 * (size_t)A.E + (size_t)(A.off[it.k] + it.i);
    unsigned long long g = 0, h = 0; // (wrapping sums)
    for (int ch = 0; ch < A.nChunks; ++ch) {
        g += (unsigned long long)p[(size_t)ch * 2 * (size_t)A.E];
        h += (unsigned long long)p[((size_t)ch * 2 + 1) * (size_t)A.E];
    }
    sn_apply(B, it.k, (size_t)it.b * (size_t)n + (size_t)it.i, (long long)g, (long long)h);
}

#endif
