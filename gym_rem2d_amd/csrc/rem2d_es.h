// rem2d_es.h -- an evolution strategy for device policies (include/rem2d_es.h): antithetic sampling around one mean per block of S
// child sets, rank shaping of the fitness, and the rank-weighted update of the mean.
// Part of the single translation unit rem2d.hip (see its header comment); not a stand-alone header.
//
// Random stream: ev_philox and the constants of rem2d_evolve.h, counter (i, anchor, generation, 4 + k).  The update REGENERATES
// every draw from its counter: it reads neither the children nor stored noise, and because the draw is an integer s times one
// constant, the weighted sum is an exact int64 whose value does not depend on how it is dealt over lanes, wavefronts or launches.
//
// rem2d_es_sample_kernel: the bandwidth pass.  A workgroup is ONE wavefront that owns one PAIR of children (anchor a, a + 1): one
// Philox block per element serves both, the mean's word is loaded once and two words are stored.  The block index is the
// workgroup's, so the mean's base is scalar.  Per array, consecutive lanes take consecutive V-word groups, V = 4 (dwordx4) where
// the per-set length is a multiple of 4 and both bases are 16-byte aligned (the host's choice, as rem2d_evolve_vary_kernel's),
// V = 1 otherwise.  No LDS, no atomics.
//
// rem2d_es_shape_kernel: lane = child, ES_TILE children per workgroup.  The fitness of every block that the workgroup's children
// belong to is staged through LDS in tiles of ES_TILE values, as int64 keys whose signed order is the order on fitness (es_key:
// one integer compare instead of three binary64 ones); every lane then walks the tile, all lanes reading the same word (an LDS
// broadcast), and counts the sets of its own block below it (L) and level with it (E).  Blocks smaller than the tile share one,
// larger ones loop, and a tile that lies inside the block of every lane of a wavefront is walked without the range test.  No
// atomics: every count is a lane's own.
//
// rem2d_es_update_kernel: a workgroup is ONE wavefront whose lanes take 64 consecutive elements of one array of one block, for one
// chunk of the block's pairs.  d_q = util[a] - util[a + 1] is the same in every lane -- a scalar load -- and a pair with d_q == 0
// is skipped as a whole, Philox block included.  The accumulate is one 64-bit multiply-add per draw.  Without a split (one chunk)
// the wavefront applies the update itself; otherwise its int64 partial goes to the caller's scratch, [block][chunk][element], and
// rem2d_es_finish_kernel sums a block's chunks and applies them.  Plain stores, no atomics, no LDS.
//
// Arithmetic: every product goes through sn_mul (rem2d_sense.h), so that -ffp-contract=fast finds nothing to fuse.
#ifndef REM2D_ES_KERNELS_H
#define REM2D_ES_KERNELS_H

#define ES_TILE 256       // children per workgroup of the shape kernel == fitness values per LDS tile
#define ES_DOMAIN0 4u     // counter word 3 is ES_DOMAIN0 + k, k = 1 .. 4

struct EsArgs {
    const double *fitness;
    int *util;
    const float *mean[4]; // w1, b1, w2, b2 of the mean
    float *child[4];      // ... of the children
    float *next[4];       // ... of the new mean
    long long *scratch;   // [M][nChunks][E] partial sums
    long long itemBase;   // first work item of this launch
    unsigned key0, key1, generation;
    int len[4];   // words of one set, per array
    int vec[4];   // 1: 16-byte accesses on that array (sample)
    int slots[4]; // wavefronts that cover one array of one set: ceil(len / 64)
    int off[4];   // first element of the array inside a set's E words
    int W, E;     // sums of slots and of len
    int M, S;
    int pairChunk, nChunks; // pairs per wavefront of the update; chunks per block (1: no split)
    float sigma, step;
};

// s: the six 16-bit halves of x1, x2, x3, centred
DEV int es_sum(const EvWords &x) {
    return (int)((x.x1 & 0xffffu) + (x.x1 >> 16) + (x.x2 & 0xffffu) + (x.x2 >> 16) + (x.x3 & 0xffffu) + (x.x3 >> 16)) - EV_NOISE_BIAS;
}

// ------------------------------------------------------------------------------------------------------------------- sample
// one array of one pair: n words of the mean, the even child's and the odd child's (each the set's own base)
template <int V> DEV void es_sample_array(const float *mean, float *even, float *odd, int n, unsigned anchor, unsigned domain, const EsArgs &A, int lane) {
    for (int i = lane * V; i < n; i += WAVE * V) { // (n is a multiple of V where V is 4: the host's choice)
        EvVec<V> m, e, o;
        m.load(mean + i);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int s = es_sum(ev_philox((unsigned)(i + v), anchor, A.generation, domain, A.key0, A.key1));
            const float t = sn_mul(A.sigma, sn_mul((float)s, __uint_as_float(EV_NOISE_SCALE)));
            e.v[v] = __fadd_rn(m.v[v], t);
            o.v[v] = __fadd_rn(m.v[v], -t);
        }
        e.store(even + i);
        o.store(odd + i);
    }
}

__global__ __launch_bounds__(WAVE) void rem2d_es_sample_kernel(EsArgs A) {
    const int lane = (int)threadIdx.x;
    const long long a = 2ll * (A.itemBase + (long long)blockIdx.x); // the anchor; < M S: the grid is pairs
    const int b = (int)(a / (long long)A.S);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float *mean = A.mean[k] + (size_t)b * (size_t)A.len[k];
        float *even = A.child[k] + (size_t)a * (size_t)A.len[k];
        if (A.vec[k]) es_sample_array<4>(mean, even, even + A.len[k], A.len[k], (unsigned)a, ES_DOMAIN0 + 1u + (unsigned)k, A, lane);
        else es_sample_array<1>(mean, even, even + A.len[k], A.len[k], (unsigned)a, ES_DOMAIN0 + 1u + (unsigned)k, A, lane);
    }
}

// -------------------------------------------------------------------------------------------------------------------- shape
// fitness -> an int64 whose signed order is the order on fitness: every NaN the minimum, -0 and +0 one key
DEV long long es_key(double f) {
    if (f != f) return (long long)0x8000000000000000ull;
    if (f == 0.0) f = 0.0; // -0 -> +0
    const long long b = __double_as_longlong(f);
    return b ^ ((b >> 63) & 0x7fffffffffffffffll); // a negative value: the lower 63 bits flipped (-inf stays above the NaN key)
}

__global__ __launch_bounds__(ES_TILE) void rem2d_es_shape_kernel(EsArgs A) {
    __shared__ long long tile[ES_TILE];
    const int t = (int)threadIdx.x;
    const long long G = (long long)A.M * (long long)A.S, S = (long long)A.S;
    const long long c0 = (long long)blockIdx.x * ES_TILE; // < G: the grid is ceil(G / ES_TILE)
    const long long c = c0 + t;
    const bool on = c < G;
    // the sets this lane counts: its own block; the sets the workgroup stages: every block one of its children belongs to
    const long long lo = on ? (c / S) * S : 0, hi = on ? lo + S : 0;
    const long long last = (c0 + ES_TILE < G ? c0 + ES_TILE : G) - 1;
    const long long first = (c0 / S) * S, end = (last / S + 1) * S; // end <= G
    const long long mine = on ? es_key(A.fitness[c]) : 0;
    int below = 0, level = 0; // level counts the lane's own set too
    for (long long t0 = first; t0 < end; t0 += ES_TILE) {
        __syncthreads();
        if (t0 + t < end) tile[t] = es_key(A.fitness[t0 + t]);
        __syncthreads();
        const int n = (int)(end - t0 < ES_TILE ? end - t0 : ES_TILE);
        // the part of the tile that belongs to the lane's block
        const long long a0 = lo - t0, a1 = hi - t0;
        const int jlo = a0 < 0 ? 0 : (a0 > n ? n : (int)a0), jhi = a1 < 0 ? 0 : (a1 > n ? n : (int)a1);
        if (__all(jlo == 0 && jhi == n)) { // a tile inside the block of every lane of the wavefront: what a long block mostly sees
#pragma unroll 16 // (sixteen LDS reads in flight: a long block leaves one wavefront per SIMD, nothing else hides their latency)
            for (int j = 0; j < n; ++j) {
                const long long k = tile[j]; // the same word in every lane
                below += k < mine ? 1 : 0;
                level += k == mine ? 1 : 0;
            }
        } else {
            for (int j = 0; j < n; ++j) {
                const long long k = tile[j];
                const bool in = j >= jlo && j < jhi;
                below += (in && k < mine) ? 1 : 0;
                level += (in && k == mine) ? 1 : 0;
            }
        }
    }
    if (on) A.util[c] = 2 * below + (level - 1) - (A.S - 1);
}

// ------------------------------------------------------------------------------------------------------------------- update
struct EsItem {
    int b, ch, k, i; // block, chunk of pairs, array, element of the array (may be >= len[k]: a lane past the end)
};

// work item -> (block, chunk, array, first element + lane); items are ordered [block][chunk][slot]
DEV EsItem es_item(const EsArgs &A, long long item, int chunks, int lane) {
    EsItem it;
    int w = (int)(item % (long long)A.W);
    const long long bc = item / (long long)A.W;
    it.ch = (int)(bc % (long long)chunks);
    it.b = (int)(bc / (long long)chunks);
    it.k = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (it.k == k && w >= A.slots[k]) {
            w -= A.slots[k];
            it.k = k + 1;
        }
    it.i = w * WAVE + lane;
    return it;
}

// new mean word from the mean's and the exact sum
DEV float es_apply(float m, long long g, float step) {
    const float gf = __double2float_rn(__ll2double_rn(g));
    return __fadd_rn(m, sn_mul(step, sn_mul(gf, __uint_as_float(EV_NOISE_SCALE))));
}

__global__ __launch_bounds__(WAVE) void rem2d_es_update_kernel(EsArgs A) {
    const int lane = (int)threadIdx.x;
    const EsItem it = es_item(A, A.itemBase + (long long)blockIdx.x, A.nChunks, lane);
    const int P = A.S >> 1;
    const int q0 = (int)((long long)it.ch * (long long)A.pairChunk);
    const int q1 = (long long)q0 + (long long)A.pairChunk < (long long)P ? q0 + A.pairChunk : P;
    const int *__restrict__ u = A.util + (size_t)it.b * (size_t)A.S;
    const unsigned base = (unsigned)((long long)it.b * (long long)A.S), domain = ES_DOMAIN0 + 1u + (unsigned)it.k;
    long long g = 0;
    for (int q = q0; q < q1; ++q) {
        const int d = (int)((unsigned)u[2 * q] - (unsigned)u[2 * q + 1]); // the same in every lane; modulo 2^32, as the header says
        if (d == 0) continue;
        const int s = es_sum(ev_philox((unsigned)it.i, base + 2u * (unsigned)q, A.generation, domain, A.key0, A.key1));
        g += (long long)d * (long long)s;
    }
    const int n = A.len[it.k];
    if (it.i >= n) return;
    if (A.nChunks == 1) {
        const size_t at = (size_t)it.b * (size_t)n + (size_t)it.i;
        A.next[it.k][at] = es_apply(A.mean[it.k][at], g, A.step);
    } else {
        A.scratch[((size_t)it.b * (size_t)A.nChunks + (size_t)it.ch) * (size_t)A.E + (size_t)(A.off[it.k] + it.i)] = g;
    }
}

// the chunks' partial sums of one element, summed and applied; items are ordered [block][slot]
__global__ __launch_bounds__(WAVE) void rem2d_es_finish_kernel(EsArgs A) {
    const int lane = (int)threadIdx.x;
    const EsItem it = es_item(A, A.itemBase + (long long)blockIdx.x, 1, lane);
    const int n = A.len[it.k];
    if (it.i >= n) return;
    const long long *p = A.scratch + (size_t)it.b * (size_t)A.nChunks * (size_t)A.E + (size_t)(A.off[it.k] + it.i);
    long long g = 0;
    for (int ch = 0; ch < A.nChunks; ++ch) g += p[(size_t)ch * (size_t)A.E];
    const size_t at = (size_t)it.b * (size_t)n + (size_t)it.i;
    A.next[it.k][at] = es_apply(A.mean[it.k][at], g, A.step);
}

#endif
