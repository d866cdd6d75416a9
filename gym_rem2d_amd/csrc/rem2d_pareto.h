// rem2d_pareto.h -- Pareto ranking (include/rem2d_pareto.h): the fronts, the crowding and the rank utility of rows of up to four
// objectives, and the local-competition score among a row's nearest behavioural neighbours.
// Part of the single translation unit rem2d.hip (see its header comment); not a stand-alone header.
//
// rem2d_pareto_rank_kernel<K, T>: lane = row, T threads per workgroup, which serves P = T / S whole blocks (T = 256 for S <= 256, so
// that short blocks do not cost a workgroup each, T = 1024 above).  K is a compile-time bound: nothing is indexed dynamically.  The
// rows of the workgroup's blocks sit in LDS ([row][K] binary64, 32 KB at T = 1024 and K = 4) and are read as broadcasts; the lane's
// own row stays in registers.  Three scans over the lane's block:
//   1. the peel: round r gives front r to every row left that no row left dominates.  A row counts as left in round r while its
//      LDS word is PA_LEFT or r (given out in this very round), so one barrier a round is enough; that barrier is the workgroup-wide
//      "anyone left" vote.  A lane remembers the dominator it found last and scans again only once that one is gone.  The round
//      loop is a counted `for` of at most S rounds -- a block has at most S fronts -- and every scan a counted `for` of S rows.
//   2. the crowding: below / above / lo / hi per objective over the rows of the lane's own front, and F on the way.
//   3. the utility: (front, crowd) of every other row against the lane's own.
// Lanes beyond the workgroup's last block walk through every barrier and write nothing.
//
// rem2d_pareto_local_kernel<BP, KP>: the launch shape of the novelty score (rem2d_novelty.h): lane = query row, NV_TILE rows per
// workgroup, candidates staged through LDS in tiles of NV_TILE rows of BP words with their fitness beside them, wave-uniform
// block bounds, zero padding that is exact.  Candidates are visited in ascending row order, so the strict d2 < worst insertion is
// the (d2, index) tie-break.  Next to each kept distance the lane keeps one "beaten" bit, in a 32-bit register mask that is
// shifted where the distances are.
//
// Plain loads and stores, no atomics, no scratch, no communication between workgroups.  Every product goes through sn_mul
// (rem2d_sense.h), so that -ffp-contract=fast finds nothing to fuse; the crowding has no product at all.
#ifndef REM2D_PARETO_KERNELS_H
#define REM2D_PARETO_KERNELS_H

#define PA_LEFT (-2)  // an admitted row that has no front yet
#define PA_OUT (-1)   // an unadmitted row
#ifndef PA_SHORT
#define PA_SHORT 256 // threads of a workgroup for blocks up to this long (a build-time experiment may choose another: DESIGN.md 20)
#endif
#define PA_LONG 1024  // ... and for longer ones: REM2D_PARETO_MAX_GROUP
#define PA_DINF __longlong_as_double(0x7ff0000000000000ll)
#define PA_DNAN __longlong_as_double(0x7ff8000000000000ll)

struct PaArgs {
    const double *obj;
    int *front;
    double *crowd;
    int *util;
    int *nfronts;
    const float *desc;
    const double *fitness;
    double *local;
    int *neigh;
    int G, S, B, k;
};

DEV bool pa_finite(double v) { return (((unsigned long long)__double_as_longlong(v) >> 52) & 0x7ffull) != 0x7ffull; }
// a above b in the order on crowding: a NaN is below every number and level with a NaN
DEV bool pa_above(double a, double b) { return a > b || (a == a && b != b); }

// --------------------------------------------------------------------------------------------------------------------- rank
template <int K, int T> __global__ __launch_bounds__(T) void rem2d_pareto_rank_kernel(PaArgs A) {
    __shared__ double sobj[T * K];
    __shared__ double scrowd[T];
    __shared__ int sfront[T];
    const int t = (int)threadIdx.x;
    const int S = A.S, P = T / S; // P >= 1: the host picks T >= S
    const long long M = (long long)A.G / S;
    const int p = t / S, own = t - p * S;
    const long long blk = (long long)blockIdx.x * P + p;
    const bool on = p < P && blk < M;
    const int base = on ? p * S : 0; // (an idle lane scans block 0 of the workgroup, to stay in step, and writes nothing)
    const long long c = blk * S + own;
    double mine[K];
    bool adm = on;
#pragma unroll
    for (int m = 0; m < K; ++m) {
        mine[m] = on ? A.obj[(size_t)c * K + m] : 0.0;
        adm = adm && pa_finite(mine[m]);
        sobj[t * K + m] = mine[m];
    }
    int myf = adm ? PA_LEFT : PA_OUT;
    sfront[t] = myf;
    scrowd[t] = 0.0;
    // ---- 1. the peel
    int last = -1; // the dominator found last
    for (int r = 0; r < S; ++r) {
        if (!__syncthreads_or(myf == PA_LEFT)) break; // (uniform) nobody of the workgroup is left
        bool seek = myf == PA_LEFT;
        if (seek && last >= 0) {
            const int f = sfront[base + last];
            seek = !(f == PA_LEFT || f == r);
        }
        bool free = seek; // no row left dominates this one
        if (__ballot(seek) != 0ull) {
            for (int j = 0; j < S; ++j) {
                const int f = sfront[base + j];
                bool ge = f == PA_LEFT || f == r, gt = false;
#pragma unroll
                for (int m = 0; m < K; ++m) {
                    const double v = sobj[(base + j) * K + m];
                    ge = ge && v >= mine[m];
                    gt = gt || v > mine[m];
                }
                if (free && ge && gt) {
                    free = false;
                    last = j;
                }
                if (__ballot(free) == 0ull) break; // everyone of the wavefront has a dominator
            }
        }
        if (free) {
            myf = r;
            sfront[t] = r;
        }
    }
    __syncthreads();
    // ---- 2. the crowding, and F
    int F = 0;
    double below[K], above[K], lo[K], hi[K];
#pragma unroll
    for (int m = 0; m < K; ++m) {
        below[m] = -PA_DINF;
        above[m] = PA_DINF;
        lo[m] = PA_DINF;
        hi[m] = -PA_DINF;
    }
    for (int j = 0; j < S; ++j) {
        const int f = sfront[base + j];
        F = f + 1 > F ? f + 1 : F;
        const bool peer = adm && f == myf;
#pragma unroll
        for (int m = 0; m < K; ++m) {
            const double v = sobj[(base + j) * K + m];
            lo[m] = peer && v < lo[m] ? v : lo[m];
            hi[m] = peer && v > hi[m] ? v : hi[m];
            below[m] = peer && v < mine[m] && v > below[m] ? v : below[m];
            above[m] = peer && v > mine[m] && v < above[m] ? v : above[m];
        }
    }
    double cr = 0.0;
    bool open = false; // a side without a neighbour
#pragma unroll
    for (int m = 0; m < K; ++m) {
        open = open || below[m] == -PA_DINF || above[m] == PA_DINF;
        cr = __dadd_rn(cr, __ddiv_rn(__dsub_rn(above[m], below[m]), __dsub_rn(hi[m], lo[m])));
    }
    if (open) cr = PA_DINF;
    if (!adm) {
        cr = 0.0;
        myf = F;
    }
    __syncthreads(); // everyone has read the fronts of the peel
    sfront[t] = myf;
    scrowd[t] = cr;
    __syncthreads();
    // ---- 3. the utility
    int L = 0, E = 0;
    for (int j = 0; j < S; ++j) {
        const int f = sfront[base + j];
        const double cj = scrowd[base + j];
        const bool better = myf < f || (myf == f && pa_above(cr, cj));
        const bool worse = f < myf || (f == myf && pa_above(cj, cr));
        const bool other = j != own;
        L += (other && better) ? 1 : 0;
        E += (other && !better && !worse) ? 1 : 0;
    }
    if (!on) return;
    if (A.front) A.front[c] = myf;
    if (A.crowd) A.crowd[c] = cr;
    if (A.util) A.util[c] = 2 * L + E - (S - 1);
    if (A.nfronts && own == 0) A.nfronts[blk] = F;
}

// -------------------------------------------------------------------------------------------------------------------- local
// fitness a below fitness b in the evolve header's order: a NaN is below every number and not below a NaN
DEV bool pa_below(double a, double b) { return a < b || (a != a && b == b); }

// one candidate (BP words at y, the same address in every lane) against the lane's query; `ok`: it counts for this lane,
// `beaten`: its fitness is below the lane's
template <int BP, int KP> DEV void pa_visit(const float *y, bool ok, bool beaten, const float (&x)[BP], float (&best)[KP], unsigned &mask) {
    float d2 = 0.0f;
#pragma unroll
    for (int i = 0; i < BP; ++i) {
        const float t = __fsub_rn(x[i], y[i]);
        d2 = __fadd_rn(d2, sn_mul(t, t));
    }
    d2 = ok ? d2 : NV_INF;
    const bool ins = d2 < best[KP - 1]; // (a NaN and +inf never pass)
    if (__ballot(ins) != 0ull) {
        int at = 0; // the slot it lands on: behind everything that is not farther
#pragma unroll
        for (int q = 0; q < KP; ++q) at += d2 < best[q] ? 0 : 1;
#pragma unroll
        for (int q = KP - 1; q > 0; --q) best[q] = d2 < best[q - 1] ? best[q - 1] : (d2 < best[q] ? d2 : best[q]);
        best[0] = d2 < best[0] ? d2 : best[0];
        if (ins) { // at <= KP - 1 <= 31
            const unsigned low = (1u << at) - 1u;
            mask = (mask & low) | ((mask & ~low) << 1) | (beaten ? 1u << at : 0u);
        }
    }
}

template <int BP, int KP> __global__ __launch_bounds__(NV_TILE) void rem2d_pareto_local_kernel(PaArgs A) {
    __shared__ float tile[NV_TILE * BP];
    __shared__ double tfit[NV_TILE];
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
    unsigned mask = 0u;
    bool xfinite = true;
#pragma unroll
    for (int i = 0; i < BP; ++i) {
        x[i] = (on && i < A.B) ? A.desc[(size_t)c * (size_t)A.B + (size_t)i] : 0.0f;
        xfinite = xfinite && nv_finite(x[i]);
    }
    const double fc = on ? A.fitness[c] : 0.0;
#pragma unroll
    for (int q = 0; q < KP; ++q) best[q] = NV_INF;
    for (long long t0 = first; t0 < end; t0 += NV_TILE) {
        const int n = (int)(end - t0 < NV_TILE ? end - t0 : NV_TILE);
        __syncthreads();
        nv_stage<BP>(tile, A.desc, t0, n, A.B, t);
        if (t < n) tfit[t] = A.fitness[t0 + t];
        __syncthreads();
        const long long a0 = lo - t0, a1 = hi - t0, w0 = wlo - t0, w1 = whi - t0;
        const int jlo = a0 < 0 ? 0 : (a0 > n ? n : (int)a0), jhi = a1 < 0 ? 0 : (a1 > n ? n : (int)a1);
        const int j0 = __builtin_amdgcn_readfirstlane(w0 < 0 ? 0 : (w0 > n ? n : (int)w0));
        const int j1 = __builtin_amdgcn_readfirstlane(w1 < 0 ? 0 : (w1 > n ? n : (int)w1));
        const int self = (int)(c - t0 < 0 || c - t0 >= n ? -1 : c - t0);
        for (int j = j0; j < j1; ++j)
            pa_visit<BP, KP>(tile + j * BP, j >= jlo && j < jhi && j != self, pa_below(tfit[j], fc), x, best, mask);
    }
    if (!on) return;
    int kk = 0;
#pragma unroll
    for (int q = 0; q < KP; ++q) kk += (q < A.k && best[q] < NV_INF) ? 1 : 0;
    const unsigned lowk = A.k >= 32 ? 0xffffffffu : (1u << A.k) - 1u; // (the bit of a slot that holds no candidate is 0)
    A.local[c] = xfinite ? (double)__popc(mask & lowk) : PA_DNAN;
    if (A.neigh) A.neigh[c] = kk;
}

#endif
