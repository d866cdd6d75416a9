// rem2d_novelty.h -- behavioural novelty (include/rem2d_novelty.h): descriptor rows recorded between two steps, the k-nearest-
// neighbour score of every row against its block's peers and archive, and the archive's upkeep.
// Part of the single translation unit rem2d.hip (see its header comment); not a stand-alone header.
//
// rem2d_describe_kernel: the launch shape of rem2d_observe_kernel (ctl_locate / CtlTable, one launch per 16 worlds); only a creature's
// root lane works: two loads, up to 2 K stores.  The env4 plane (FROZEN, STEPS) is not in CtlWorld, so it comes in a table beside it.
// Plain loads and stores, no LDS, no atomics.
//
// rem2d_novelty_score_kernel<BP, KP>: lane = query row, NV_TILE rows per workgroup, as rem2d_es_shape_kernel.  The query's words and
// its KP best squared distances live in registers; BP >= B and KP >= k are compile-time bounds (powers of two), so nothing is
// indexed dynamically.  Padding is exact: a padded word is 0 on both sides, t = 0 - 0, d2 + (0 * 0) = d2 for every d2 the sum can
// hold (never -0), and the k smallest of a multiset are the first k of its KP smallest.  Candidates are staged through LDS in tiles
// of NV_TILE rows of BP words and read as broadcasts (every lane the same word).  First the rows of every block the workgroup's
// queries belong to, then those blocks' live archive entries -- through LDS too where blocks are at least a tile long, read by
// every lane from its own block's ring where they are shorter (the lanes of a block share the words in the cache; no barrier).
// A wavefront walks only the part of a tile that
// belongs to a block of one of its lanes, and a tile that lies inside the block of every lane runs without the range test.  A
// candidate that is out of range, the query itself or not finite becomes +inf, which never beats the current worst; the sorted
// insertion is guarded by a wave-level ballot, so a tile that improves nobody costs distances only.  No atomics, no scratch, no
// communication between workgroups.
//
// rem2d_novelty_add_kernel: a workgroup per block walks the block's rows in order, twice -- once to count the rows the call adds (n,
// which decides who is written where more than cap are added), once to write.  Offsets are ballot / popcount prefixes inside a
// wavefront plus the wavefronts' counts and a running base in LDS.  Plain stores, no atomics.
//
// Arithmetic: every product goes through sn_mul (rem2d_sense.h), so that -ffp-contract=fast finds nothing to fuse.
#ifndef REM2D_NOVELTY_KERNELS_H
#define REM2D_NOVELTY_KERNELS_H

#define NV_TILE 256   // query rows per workgroup of the score kernel == candidate rows per LDS tile
#define NV_DOMAIN 9u  // counter word 3 of the add
#define NV_INF __uint_as_float(0x7f800000u)

struct NvTable { // the env4 plane of the worlds of a describe launch, beside their CtlWorld
    char *env4[CTL_TABLE];
};

struct NvArgs {
    const float *desc;
    float *archive;
    long long *total;
    double *novelty;
    const unsigned char *mask;
    unsigned long long threshold;
    unsigned key0, key1, generation;
    int B, G, S, k, cap;
};

// ----------------------------------------------------------------------------------------------------------------- describe
__global__ __launch_bounds__(CTL_THREADS) void rem2d_describe_kernel(CtlTable Tb, NvTable Te, int period, int K, float *out, long long outRows) {
    CtlLane c;
    if (!ctl_locate(Tb, c)) return;
    if (!c.inWorld || c.sub != 0) return; // (no wavefront-wide operation follows ctl_locate)
    struct { char *lane4, *env4; unsigned Lp, Np; } S;
    S.lane4 = c.S.lane4; S.env4 = Te.env4[c.world]; S.Lp = c.S.Lp; S.Np = c.S.Np;
    const unsigned gl = c.gl, env = c.env;
    const long long r = c.S.index ? (long long)c.S.index[env] : (long long)env;
    if (r < 0 || r >= outRows) return;
    if (EI(E_FROZEN) != 0) return; // the episode is over: the row stays as it is
    const long long s = (long long)EI(E_STEPS);
    const float px = LF(L_PX), py = LF(L_PY);
    float *row = out + (size_t)r * (size_t)(2 * K);
    for (int k = 0; k < K; ++k)
        if ((long long)(k + 1) * (long long)period >= s) {
            row[2 * k] = px;
            row[2 * k + 1] = py;
        }
}

// -------------------------------------------------------------------------------------------------------------------- score
DEV bool nv_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// one candidate (BP words at y, the same address in every lane) against the lane's query; `ok`: it counts for this lane
template <int BP, int KP> DEV void nv_visit(const float *y, bool ok, const float (&x)[BP], float (&best)[KP]) {
    float d2 = 0.0f;
#pragma unroll
    for (int i = 0; i < BP; ++i) {
        const float t = __fsub_rn(x[i], y[i]);
        d2 = __fadd_rn(d2, sn_mul(t, t));
    }
    d2 = ok ? d2 : NV_INF;
    if (__ballot(d2 < best[KP - 1]) != 0ull) { // somebody's list changes (a NaN and +inf never pass)
#pragma unroll
        for (int q = KP - 1; q > 0; --q) best[q] = d2 < best[q - 1] ? best[q - 1] : (d2 < best[q] ? d2 : best[q]);
        best[0] = d2 < best[0] ? d2 : best[0];
    }
}

// rows [r0, r0 + n) of `src` (B words each) -> tile rows 0 .. n-1 of BP words, zero padded
template <int BP> DEV void nv_stage(float *tile, const float *src, long long r0, int n, int B, int t) {
    for (int w = t; w < n * BP; w += NV_TILE) {
        const int j = w / BP, i = w % BP;
        tile[w] = i < B ? src[(size_t)(r0 + j) * (size_t)B + (size_t)i] : 0.0f;
    }
}

template <int BP, int KP> __global__ __launch_bounds__(NV_TILE) void rem2d_novelty_score_kernel(NvArgs A) {
    __shared__ float tile[NV_TILE * BP];
    const int t = (int)threadIdx.x;
    const long long G = (long long)A.G, S = (long long)A.S;
    const long long c0 = (long long)blockIdx.x * NV_TILE; // < G: the grid is ceil(G / NV_TILE)
    const long long c = c0 + t;
    const bool on = c < G;
    const long long myb = on ? c / S : -1;
    const long long lo = on ? myb * S : 0, hi = on ? lo + S : 0;
    const long long last = (c0 + NV_TILE < G ? c0 + NV_TILE : G) - 1;
    const long long first = (c0 / S) * S, end = (last / S + 1) * S; // end <= G
    // the rows that belong to a block of one of this wavefront's lanes (wave-uniform: its lanes are consecutive rows)
    const long long cw0 = c0 + (long long)(t & ~(WAVE - 1));
    const long long cwl = cw0 + WAVE - 1 < G ? cw0 + WAVE - 1 : G - 1;
    const bool waveOn = cw0 < G;
    const long long wlo = waveOn ? (cw0 / S) * S : 0, whi = waveOn ? (cwl / S + 1) * S : 0;
    float x[BP], best[KP];
    bool xfinite = true;
#pragma unroll
    for (int i = 0; i < BP; ++i) {
        x[i] = (on && i < A.B) ? A.desc[(size_t)c * (size_t)A.B + (size_t)i] : 0.0f;
        xfinite = xfinite && nv_finite(x[i]);
    }
#pragma unroll
    for (int q = 0; q < KP; ++q) best[q] = NV_INF;
    // ---- the rows of the blocks
    for (long long t0 = first; t0 < end; t0 += NV_TILE) {
        const int n = (int)(end - t0 < NV_TILE ? end - t0 : NV_TILE);
        __syncthreads();
        nv_stage<BP>(tile, A.desc, t0, n, A.B, t);
        __syncthreads();
        const long long a0 = lo - t0, a1 = hi - t0, w0 = wlo - t0, w1 = whi - t0;
        const int jlo = a0 < 0 ? 0 : (a0 > n ? n : (int)a0), jhi = a1 < 0 ? 0 : (a1 > n ? n : (int)a1);
        const int j0 = __builtin_amdgcn_readfirstlane(w0 < 0 ? 0 : (w0 > n ? n : (int)w0));
        const int j1 = __builtin_amdgcn_readfirstlane(w1 < 0 ? 0 : (w1 > n ? n : (int)w1));
        const int self = (int)(c - t0 < 0 || c - t0 >= n ? -1 : c - t0);
        if (__all(jlo == 0 && jhi == n)) { // a tile inside the block of every lane of the wavefront: what a long block mostly sees
            for (int j = j0; j < j1; ++j) nv_visit<BP, KP>(tile + j * BP, j != self, x, best);
        } else {
            for (int j = j0; j < j1; ++j) nv_visit<BP, KP>(tile + j * BP, j >= jlo && j < jhi && j != self, x, best);
        }
    }
    // ---- the live archive entries of the same blocks
    if (S >= NV_TILE) { // (workgroup-uniform) long blocks: a workgroup's rows belong to one or two blocks, whose entries go through LDS
        const long long bFirst = first / S, bEnd = end / S;
        const long long wbFirst = waveOn ? cw0 / S : 0, wbEnd = waveOn ? cwl / S + 1 : 0;
        for (long long b = bFirst; b < bEnd; ++b) {
            const long long tot = A.total[b];
            const int live = (int)(tot < 0 ? 0 : (tot < (long long)A.cap ? tot : (long long)A.cap));
            const bool waveIn = b >= wbFirst && b < wbEnd; // wave-uniform
            for (int e0 = 0; e0 < live; e0 += NV_TILE) {
                const int n = live - e0 < NV_TILE ? live - e0 : NV_TILE;
                __syncthreads();
                nv_stage<BP>(tile, A.archive, b * (long long)A.cap + e0, n, A.B, t);
                __syncthreads();
                if (!waveIn) continue;
                if (__all(myb == b)) {
                    for (int j = 0; j < n; ++j) nv_visit<BP, KP>(tile + j * BP, true, x, best);
                } else {
                    for (int j = 0; j < n; ++j) nv_visit<BP, KP>(tile + j * BP, myb == b, x, best);
                }
            }
        }
    } else {
        // short blocks: the workgroup's rows belong to 256 / S blocks and more, each with entries of its own; staging them one
        // block after the other would leave most wavefronts waiting at the barriers.  Every lane reads its OWN block's entries
        // straight from memory -- the lanes of a block read the same words, a broadcast in the cache -- with no barrier at all
        int myLive = 0;
        if (on) {
            const long long tot = A.total[myb];
            myLive = (int)(tot < 0 ? 0 : (tot < (long long)A.cap ? tot : (long long)A.cap));
        }
        int maxLive = myLive; // the most of any lane of the wavefront: everyone walks that far, for the ballot's sake
#pragma unroll
        for (int m = WAVE / 2; m > 0; m >>= 1) maxLive = max(maxLive, __shfl_xor(maxLive, m));
        const float *mine = A.archive + (size_t)(on ? myb : 0) * (size_t)A.cap * (size_t)A.B;
        for (int e = 0; e < maxLive; ++e) {
            const bool ok = e < myLive;
            float y[BP];
#pragma unroll
            for (int i = 0; i < BP; ++i) y[i] = (ok && i < A.B) ? mine[(size_t)e * (size_t)A.B + (size_t)i] : 0.0f;
            nv_visit<BP, KP>(y, ok, x, best);
        }
    }
    if (!on) return;
    double sum = 0.0;
    int kk = 0;
#pragma unroll
    for (int q = 0; q < KP; ++q)
        if (q < A.k && best[q] < NV_INF) { // ascending: best is sorted
            sum = __dadd_rn(sum, (double)sqrtf(best[q]));
            ++kk;
        }
    double nov = kk ? sum / (double)kk : 0.0;
    if (!xfinite) nov = __longlong_as_double(0x7ff8000000000000ll);
    A.novelty[c] = nov;
}

// ---------------------------------------------------------------------------------------------------------------------- add
// is row c added?  (every lane may ask: c < G is the caller's business)
DEV bool nv_admit(const NvArgs &A, long long c) {
    if (A.mask && A.mask[c] == 0) return false;
    const float *x = A.desc + (size_t)c * (size_t)A.B;
    bool fin = true;
    for (int i = 0; i < A.B; ++i) fin = fin && nv_finite(x[i]);
    if (!fin) return false;
    return (unsigned long long)ev_philox(0u, (unsigned)c, A.generation, NV_DOMAIN, A.key0, A.key1).x0 < A.threshold;
}

__global__ __launch_bounds__(NV_TILE) void rem2d_novelty_add_kernel(NvArgs A) {
    __shared__ int waveCount[NV_TILE / WAVE];
    __shared__ long long base;
    const int t = (int)threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
    const long long b = (long long)blockIdx.x, S = (long long)A.S, r0 = b * S;
    const long long tot = A.total[b]; // read by everyone before the one store at the end
    long long added = 0;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && (A.cap == 0 || added == 0)) break; // (uniform)
        __syncthreads();
        if (t == 0) base = 0;
        __syncthreads();
        for (long long j0 = 0; j0 < S; j0 += NV_TILE) {
            const long long c = r0 + j0 + t;
            const bool in = j0 + t < S && nv_admit(A, c);
            const unsigned long long m = __ballot(in);
            if (lane == 0) waveCount[wv] = __popcll(m);
            __syncthreads();
            long long j = base + (long long)__popcll(m & ((1ull << lane) - 1ull));
            int all = 0;
#pragma unroll
            for (int w = 0; w < NV_TILE / WAVE; ++w) {
                if (w < wv) j += waveCount[w];
                all += waveCount[w];
            }
            if (pass == 1 && in && j >= added - (long long)A.cap) {
                const unsigned long long e = ((unsigned long long)tot % (unsigned long long)A.cap + (unsigned long long)j) % (unsigned long long)A.cap;
                float *dst = A.archive + ((size_t)b * (size_t)A.cap + (size_t)e) * (size_t)A.B;
                const float *src = A.desc + (size_t)c * (size_t)A.B;
                for (int i = 0; i < A.B; ++i) dst[i] = src[i];
            }
            __syncthreads(); // everyone has read base and the counts
            if (t == 0) base += all;
        }
        __syncthreads();
        added = base;
    }
    if (t == 0) A.total[b] = tot + added;
}

#endif
