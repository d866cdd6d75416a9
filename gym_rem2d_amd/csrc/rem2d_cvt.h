// rem2d_cvt.h -- centroid archives and the iso+line emitter (include/rem2d_cvt.h): the nearest centroid of every descriptor row, the
// insertion's key pass over assigned cells, the draw of two parents among the filled cells and the line variation.
// Part of the single translation unit rem2d.hip (see its header comment); not a stand-alone header.
//
// rem2d_cvt_assign_kernel<BP>: lane = row, CV_TILE rows per workgroup, as rem2d_novelty_score_kernel.  The row's words live in
// registers; BP >= B is a compile-time bound (4, 8, 16, 32), so nothing is indexed dynamically.  Padding is exact: a padded word is 0
// on both sides, t = 0 - 0 = +0, d2 + (0 * 0) = d2 for every d2 the sum can hold (never -0).  Centroids are staged through LDS in
// tiles of CV_TILE centroids of BP words and read as broadcasts (every lane the same word).  A lane walks its centroids in ascending
// order and keeps (bestd, best) under `d2 < bestd`: a NaN and +inf never pass, ties stay with the lower centroid.
// blockIdx.y deals the centroids over `splits` workgroups per row tile, chunk y = [y per, (y + 1) per).  With one split the lane
// writes cell and dist itself.  With more, every lane that found a candidate does ONE atomicMin on the row's 64-bit word of
// caller-owned scratch with (d2 bits << 32) | q: a finite d2 is >= +0, so the integer order is the order of (d2, q) and the minimum
// over the chunks is the sequential rule's answer.  Integer minima commute: the order of the atomics does not matter.
// rem2d_cvt_clear_kernel sets the words to all ones ("no candidate") ahead of it, rem2d_cvt_finish_kernel reads them out.
// The atomics are HIP's ordinary device atomics on global memory (vector instructions), relaxed, device scope; a kernel boundary
// orders one pass after the other.  No float atomics, no scratch memory.
//
// rem2d_cvt_key_kernel: rem2d_elites_key_kernel with the cell read from cell[] (the assignment's) instead of computed; a row that is
// not admissible gets cell -1.  The insertion's other three launches are rem2d_elites_clear / _row / _commit_kernel, unchanged.
//
// rem2d_cvt_draw_kernel: rem2d_elites_sample_kernel's compaction of the filled cells of a block, then two draws per child: domain
// 10 (the elites header's, bit for bit) and domain 11.
//
// rem2d_cvt_line_kernel: the bandwidth pass, child-major, as rem2d_evolve_vary_kernel: a workgroup is ONE wavefront that owns child
// c; parent[c] and parent2[c] are read once and made wave-uniform, so both gathers are scalar base addresses; per array the
// EvVec<4> / EvVec<1> walk, V chosen per array on the host.  The line coefficient a = sigma_line * zl is one Philox block per child,
// computed by every lane alike.  (x1 + (sigma_iso * z)) + (a * (x2 - x1)): both products go through sn_mul, so that
// -ffp-contract=fast finds nothing to fuse.  sigma_line == +-0 (wave-uniform) never reads the second parent.
#ifndef REM2D_CVT_KERNELS_H
#define REM2D_CVT_KERNELS_H

#define CV_TILE 256
#define CV_DOMAIN2 11u // counter word 3 of the second parent's draw
#define CV_DOMAINA 12u // ... of the line coefficient
#define CV_NONE 0xffffffffffffffffull

struct CvArgs {
    const float *desc, *centroids;
    const double *fitness;
    const unsigned char *mask;
    int *count, *cell, *parent, *parent2, *nFilled;
    float *dist;
    unsigned long long *best; // scratch: [rows], the split assign's (d2 bits, q) minima
    unsigned long long *key;  // scratch: [M C], the insertion's fitness keys
    int *list;                // scratch: [M C], the draw's filled cells
    long long rows;           // of the assignment
    unsigned key0, key1, generation;
    int B, M, S, C, perBlock, splits, per; // per: centroids per split
};

struct CvLine {
    const float *src[4]; // the elite arrays
    float *dst[4];       // the children
    const int *parent, *parent2;
    unsigned key0, key1, generation;
    int len[4], vec[4], slots;
    float sigmaIso, sigmaLine;
};

__global__ __launch_bounds__(CV_TILE) void rem2d_cvt_clear_kernel(CvArgs A) {
    const long long r = (long long)blockIdx.x * CV_TILE + (long long)threadIdx.x;
    if (r < A.rows) A.best[r] = CV_NONE;
}

template <int BP> __global__ __launch_bounds__(CV_TILE) void rem2d_cvt_assign_kernel(CvArgs A) {
    __shared__ float tile[CV_TILE * BP];
    const int t = (int)threadIdx.x;
    const long long r = (long long)blockIdx.x * CV_TILE + (long long)t;
    const bool on = r < A.rows;
    float x[BP];
#pragma unroll
    for (int i = 0; i < BP; ++i) x[i] = (on && i < A.B) ? A.desc[(size_t)r * (size_t)A.B + (size_t)i] : 0.0f;
    const int q0 = (int)blockIdx.y * A.per; // (splits * per < 2^31: both are bounded by the host)
    const int q1 = q0 + A.per < A.C ? q0 + A.per : A.C;
    float bestd = __uint_as_float(0x7f800000u);
    int best = -1;
    for (int c0 = q0; c0 < q1; c0 += CV_TILE) {
        const int n = q1 - c0 < CV_TILE ? q1 - c0 : CV_TILE;
        __syncthreads(); // everyone is done with the tile before
        for (int w = t; w < n * BP; w += CV_TILE) {
            const int j = w / BP, i = w % BP;
            tile[w] = i < A.B ? A.centroids[(size_t)(c0 + j) * (size_t)A.B + (size_t)i] : 0.0f;
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const float *y = tile + j * BP;
            float d2 = 0.0f;
#pragma unroll
            for (int i = 0; i < BP; ++i) {
                const float u = __fsub_rn(x[i], y[i]);
                d2 = __fadd_rn(d2, sn_mul(u, u));
            }
            if (d2 < bestd) { // (a NaN and +inf never pass; an equal d2 of a later centroid does not either)
                bestd = d2;
                best = c0 + j;
            }
        }
    }
    if (!on) return;
    if (A.splits == 1) {
        A.cell[r] = best;
        if (A.dist) A.dist[r] = bestd;
    } else if (best >= 0) {
        atomicMin(A.best + r, ((unsigned long long)__float_as_uint(bestd) << 32) | (unsigned long long)(unsigned)best);
    }
}

__global__ __launch_bounds__(CV_TILE) void rem2d_cvt_finish_kernel(CvArgs A) {
    const long long r = (long long)blockIdx.x * CV_TILE + (long long)threadIdx.x;
    if (r >= A.rows) return;
    const unsigned long long k = A.best[r];
    const bool none = k == CV_NONE;
    A.cell[r] = none ? -1 : (int)(unsigned)(k & 0xffffffffull);
    if (A.dist) A.dist[r] = __uint_as_float(none ? 0x7f800000u : (unsigned)(k >> 32));
}

__global__ __launch_bounds__(CV_TILE) void rem2d_cvt_key_kernel(CvArgs A) {
    const long long c = (long long)blockIdx.x * CV_TILE + (long long)threadIdx.x;
    if (c >= (long long)A.M * (long long)A.S) return;
    const int q = A.cell[c];
    if (q < 0) return;
    const double f = A.fitness[c];
    if ((A.mask && A.mask[c] == 0) || f != f) {
        A.cell[c] = -1;
        return;
    }
    const long long slot = (c / (long long)A.S) * (long long)A.C + (long long)q;
    atomicMax(A.key + slot, el_key(f));
}

__global__ __launch_bounds__(CV_TILE) void rem2d_cvt_draw_kernel(CvArgs A) {
    __shared__ int waveCount[CV_TILE / WAVE];
    __shared__ int base;
    const int t = (int)threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
    const long long b = (long long)blockIdx.x, s0 = b * (long long)A.C;
    int *list = A.list + s0;
    if (t == 0) base = 0;
    __syncthreads();
    for (int q0 = 0; q0 < A.C; q0 += CV_TILE) {
        const int q = q0 + t;
        const bool in = q < A.C && A.count[s0 + q] != 0;
        const unsigned long long m = __ballot(in);
        if (lane == 0) waveCount[wv] = __popcll(m);
        __syncthreads();
        int j = base + __popcll(m & ((1ull << lane) - 1ull));
        int all = 0;
#pragma unroll
        for (int w = 0; w < CV_TILE / WAVE; ++w) {
            if (w < wv) j += waveCount[w];
            all += waveCount[w];
        }
        if (in) list[j] = q; // j < C: at most one entry per cell
        __syncthreads();     // everyone has read base and the counts
        if (t == 0) base += all;
    }
    __threadfence_block();
    __syncthreads(); // the list is written, base is final
    const int n = base;
    if (t == 0) A.nFilled[b] = n;
    for (int i = t; i < A.perBlock; i += CV_TILE) {
        const long long c = b * (long long)A.perBlock + (long long)i;
        int p = -1, p2 = -1;
        if (n > 0) {
            const unsigned u = ev_philox(0u, (unsigned)c, A.generation, EL_DOMAIN, A.key0, A.key1).x0;
            const unsigned u2 = ev_philox(0u, (unsigned)c, A.generation, CV_DOMAIN2, A.key0, A.key1).x0;
            p = (int)(s0 + (long long)list[(int)(((unsigned long long)u * (unsigned long long)(unsigned)n) >> 32)]);
            p2 = (int)(s0 + (long long)list[(int)(((unsigned long long)u2 * (unsigned long long)(unsigned)n) >> 32)]);
        }
        A.parent[c] = p;
        A.parent2[c] = p2;
    }
}

// the evolve header's z of one Philox block
DEV float cv_noise(const EvWords &x) {
    const int s = (int)((x.x1 & 0xffffu) + (x.x1 >> 16) + (x.x2 & 0xffffu) + (x.x2 >> 16) + (x.x3 & 0xffffu) + (x.x3 >> 16)) - EV_NOISE_BIAS;
    return sn_mul((float)s, __uint_as_float(EV_NOISE_SCALE));
}

// one array of one child: n words; x1 and x2 the two parents' sets, `line`: the second one is read
template <int V> DEV void cv_array(const float *x1, const float *x2, float *dst, int n, bool line, float a, unsigned c, unsigned domain, const CvLine &A, int lane) {
    for (int i = lane * V; i < n; i += WAVE * V) { // (n is a multiple of V where V is 4: the host's choice)
        EvVec<V> w, o;
        w.load(x1 + i);
        if (line) o.load(x2 + i);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float z = cv_noise(ev_philox((unsigned)(i + v), c, A.generation, domain, A.key0, A.key1));
            float y = __fadd_rn(w.v[v], sn_mul(A.sigmaIso, z));
            if (line) y = __fadd_rn(y, sn_mul(a, __fsub_rn(o.v[v], w.v[v])));
            w.v[v] = y;
        }
        w.store(dst + i);
    }
}

__global__ __launch_bounds__(WAVE) void rem2d_cvt_line_kernel(CvLine A) {
    const int lane = (int)threadIdx.x;
    const int c = (int)blockIdx.x; // < n_children: the grid is n_children workgroups
    const int p1 = __builtin_amdgcn_readfirstlane(A.parent[c]);
    const int p2 = __builtin_amdgcn_readfirstlane(A.parent2[c]);
    if (p1 < 0 || p1 >= A.slots || p2 < 0 || p2 >= A.slots) return;
    const bool line = A.sigmaLine != 0.0f; // (false for both zeros)
    const float a = sn_mul(A.sigmaLine, cv_noise(ev_philox(0u, (unsigned)c, A.generation, CV_DOMAINA, A.key0, A.key1)));
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float *x1 = A.src[k] + (size_t)p1 * (size_t)A.len[k];
        const float *x2 = A.src[k] + (size_t)p2 * (size_t)A.len[k];
        float *dst = A.dst[k] + (size_t)c * (size_t)A.len[k];
        if (A.vec[k]) cv_array<4>(x1, x2, dst, A.len[k], line, a, (unsigned)c, (unsigned)(k + 1), A, lane);
        else cv_array<1>(x1, x2, dst, A.len[k], line, a, (unsigned)c, (unsigned)(k + 1), A, lane);
    }
}

#endif
