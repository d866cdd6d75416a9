// rem2d_evolve.h -- evolving device policies (include/rem2d_evolve.h): tournament selection and mutation of the weight sets of
// rem2d_policy.h for a whole population.
// Part of the single translation unit rem2d.hip (see its header comment); not a stand-alone header.
//
// Random stream: Philox4x32-10 (Random123), key (seed lo, seed hi), counter (i, c, generation, domain); the public header states
// which draw decides what.  A draw is a function of its counter alone, so neither kernel keeps generator state and no result
// depends on how the work is dealt over lanes.
//
// rem2d_evolve_select_kernel: a workgroup is ONE wavefront, lane = child c.  A tournament is the lane's own: one Philox block gives
// the (at most four) aspirants, whose fitness the lane gathers.  An elite child (c the first of its block of S sets) needs the
// block's arg max: the wavefront takes its elite lanes one after the other (ballot loop), all 64 lanes walk that block S / 64 sets
// apiece keeping (best fitness, lowest index), and a butterfly of __shfl_xor folds the 64 candidates.  The order on fitness is a
// total preorder and ties go to the lower index, so the fold's order does not matter.
//
// rem2d_evolve_vary_kernel: the bandwidth pass, child-major.  A workgroup is ONE wavefront that owns child c; p = parent[c] is
// read once and made wave-uniform (readfirstlane), so the gather is a scalar base address.  Per array, consecutive lanes take
// consecutive V-word groups: V = 4 (dwordx4 loads and stores) where the array's per-set length is a multiple of 4 and both bases
// are 16-byte aligned -- decided per array on the host, as the forward kernel's V is -- V = 1 otherwise.  An elite child and
// rate_threshold == 0 take the copy path: the same walk without a Philox block.  A p outside [0, G) is a branch around everything.
// Plain vector loads and stores, no atomics, no LDS, no scratch.
//
// Arithmetic of a hit: w + (sigma * ((float)s * C)), every operation rounded separately in all three builds: both products go
// through sn_mul (rem2d_sense.h), so that -ffp-contract=fast finds nothing to fuse.
#ifndef REM2D_EVOLVE_KERNELS_H
#define REM2D_EVOLVE_KERNELS_H

#define EV_M0 0xD2511F53u
#define EV_M1 0xCD9E8D57u
#define EV_W0 0x9E3779B9u
#define EV_W1 0xBB67AE85u
#define EV_NOISE_SCALE 0x37B504F3u // fl32(sqrt 2) * 2^-16
#define EV_NOISE_BIAS 196605       // 3 * 65535: the mean of six 16-bit halves, times six

struct EvolveArgs {
    const double *fitness;
    const float *src[4]; // w1, b1, w2, b2 of the parents
    float *dst[4];       // ... of the children
    int *parent;
    unsigned long long rateThreshold;
    unsigned key0, key1, generation;
    int len[4]; // words of one set, per array
    int vec[4]; // 1: 16-byte accesses on that array
    int G, S, T, elite;
    float sigma;
};

struct EvWords {
    unsigned x0, x1, x2, x3;
};

DEV EvWords ev_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)EV_M0 * (unsigned long long)c0;
        const unsigned long long p1 = (unsigned long long)EV_M1 * (unsigned long long)c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1;
        c3 = (unsigned)p0;
        c0 = n0;
        c2 = n2;
        k0 += EV_W0;
        k1 += EV_W1;
    }
    EvWords w;
    w.x0 = c0; w.x1 = c1; w.x2 = c2; w.x3 = c3;
    return w;
}

// a above b in the order on fitness: NaN below everything and equal to itself, -0 == +0
DEV bool ev_greater(double a, double b) { return a == a && (b != b || a > b); }

// candidate (a, ia) is to be kept over (b, ib): the greater fitness, on a tie the lower index; an index < 0 is no candidate
DEV bool ev_keeps(double a, int ia, double b, int ib) {
    if (ib < 0) return true;
    if (ia < 0) return false;
    return ev_greater(a, b) || (!ev_greater(b, a) && ia < ib);
}

__global__ __launch_bounds__(WAVE) void rem2d_evolve_select_kernel(EvolveArgs A) {
    const int lane = (int)threadIdx.x;
    const long long cl = (long long)blockIdx.x * WAVE + lane;
    const bool on = cl < (long long)A.G;
    const int c = on ? (int)cl : 0;
    const int base = (c / A.S) * A.S;
    const bool elite = on && A.elite != 0 && c == base;
    int winner = -1;
    if (on && !elite) {
        const EvWords w = ev_philox(0u, (unsigned)c, A.generation, 0u, A.key0, A.key1);
        const unsigned x[4] = {w.x0, w.x1, w.x2, w.x3};
        winner = base + (int)(((unsigned long long)x[0] * (unsigned long long)(unsigned)A.S) >> 32);
        double best = A.fitness[winner];
#pragma unroll
        for (int k = 1; k < REM2D_EVOLVE_MAX_TOURNSIZE; ++k) {
            if (k < A.T) {
                const int a = base + (int)(((unsigned long long)x[k] * (unsigned long long)(unsigned)A.S) >> 32);
                const double f = A.fitness[a];
                if (ev_greater(f, best)) {
                    best = f;
                    winner = a;
                }
            }
        }
    }
    // the elite lanes of the wavefront, one block scan after the other, all lanes helping
    unsigned long long todo = __ballot(elite);
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const int b0 = __builtin_amdgcn_readfirstlane(__shfl(base, src));
        double best = 0.0;
        int at = -1;
        for (int i = lane; i < A.S; i += WAVE) { // ascending indices per lane: a tie keeps the earlier one
            const double f = A.fitness[b0 + i];
            if (at < 0 || ev_greater(f, best)) {
                best = f;
                at = b0 + i;
            }
        }
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const double ob = __shfl_xor(best, o);
            const int oa = __shfl_xor(at, o);
            if (!ev_keeps(best, at, ob, oa)) {
                best = ob;
                at = oa;
            }
        }
        if (lane == src) winner = at;
    }
    if (on) A.parent[c] = winner;
}

typedef float ev_f4 __attribute__((ext_vector_type(4)));
template <int V> struct EvVec;
template <> struct EvVec<1> {
    float v[1];
    DEV void load(const float *p) { v[0] = *p; }
    DEV void store(float *p) const { *p = v[0]; }
};
template <> struct EvVec<4> {
    float v[4];
    DEV void load(const float *p) {
        const ev_f4 q = *(const ev_f4 *)p;
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
    DEV void store(float *p) const {
        ev_f4 q;
        q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
        *(ev_f4 *)p = q;
    }
};

// one element: the parent's word w, the draw of its counter
DEV float ev_mutate(float w, const EvWords &x, unsigned long long rateThreshold, float sigma) {
    if ((unsigned long long)x.x0 >= rateThreshold) return w;
    const int s = (int)((x.x1 & 0xffffu) + (x.x1 >> 16) + (x.x2 & 0xffffu) + (x.x2 >> 16) + (x.x3 & 0xffffu) + (x.x3 >> 16)) - EV_NOISE_BIAS;
    const float z = sn_mul((float)s, __uint_as_float(EV_NOISE_SCALE));
    return __fadd_rn(w, sn_mul(sigma, z));
}

// one array of one child: n words from src to dst (both the set's own base), mutated unless `copy`
template <int V> DEV void ev_array(const float *src, float *dst, int n, bool copy, unsigned c, unsigned domain, const EvolveArgs &A, int lane) {
    for (int i = lane * V; i < n; i += WAVE * V) { // (n is a multiple of V where V is 4: the host's choice)
        EvVec<V> w;
        w.load(src + i);
        if (!copy) {
#pragma unroll
            for (int v = 0; v < V; ++v) w.v[v] = ev_mutate(w.v[v], ev_philox((unsigned)(i + v), c, A.generation, domain, A.key0, A.key1), A.rateThreshold, A.sigma);
        }
        w.store(dst + i);
    }
}

__global__ __launch_bounds__(WAVE) void rem2d_evolve_vary_kernel(EvolveArgs A) {
    const int lane = (int)threadIdx.x;
    const int c = (int)blockIdx.x; // < G: the grid is G workgroups
    const int p = __builtin_amdgcn_readfirstlane(A.parent[c]);
    if (p < 0 || p >= A.G) return;
    const bool copy = A.rateThreshold == 0ull || (A.elite != 0 && c % A.S == 0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float *src = A.src[k] + (size_t)p * (size_t)A.len[k];
        float *dst = A.dst[k] + (size_t)c * (size_t)A.len[k];
        if (A.vec[k]) ev_array<4>(src, dst, A.len[k], copy, (unsigned)c, (unsigned)(k + 1), A, lane);
        else ev_array<1>(src, dst, A.len[k], copy, (unsigned)c, (unsigned)(k + 1), A, lane);
    }
}

#endif
