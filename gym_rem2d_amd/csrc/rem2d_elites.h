// rem2d_elites.h -- MAP-Elites for device policies (include/rem2d_elites.h): the insertion of an evaluated population into the elite
// grids of its blocks and the draw of parents among the filled cells.
// Part of the single translation unit rem2d.hip (see its header comment); not a stand-alone header.
//
// The insertion is four launches over caller-owned scratch (key[M C] 64-bit, row[M C] 32-bit):
//   rem2d_elites_clear_kernel   a thread per (block, cell): key = 0, row = INT_MAX, winner = -1.
//   rem2d_elites_key_kernel     a thread per row: the row's cell (written to cell[]), and for an admissible row atomicMax(key[slot],
//                               the order-preserving integer key of its fitness).  -0 maps to +0 first; a NaN is never admitted, so
//                               every key is above 0 and 0 means "no candidate".
//   rem2d_elites_row_kernel     a thread per row: where the row's key IS the cell's maximum, atomicMin(row[slot], c): the lowest
//                               such row.  Integer maxima and minima commute: the order of the atomics does not matter.
//   rem2d_elites_commit_kernel  ONE wavefront per (block, cell): the challenger against the incumbent, decided wave-uniformly, then
//                               the bit copy of the descriptor row and of the set with the EvVec<4> / EvVec<1> walk of ev_array
//                               (rem2d_evolve.h's kernels file) in copy mode, V chosen per array on the host as vary chooses it.
// The atomics are HIP's ordinary device atomics on global memory (vector instructions), relaxed, device scope; a kernel boundary
// orders one pass after the other.  No LDS but the sample kernel's scan, no scratch memory.
//
// rem2d_elites_sample_kernel: one workgroup of EL_TILE threads per block.  It walks the block's count[] a tile at a time, compacts
// the filled cells in ascending order into the scratch's row region (ballot + popcount within a wavefront, the wavefronts' counts
// through LDS, as the novelty add kernel does), then deals the children of the block over its threads: one Philox block each, one
// load from the list.  The emission's second launch is rem2d_evolve_vary_kernel itself, unchanged, on the elite arrays.
#ifndef REM2D_ELITES_KERNELS_H
#define REM2D_ELITES_KERNELS_H

#define EL_TILE 256
#define EL_DOMAIN 10u // counter word 3 of the draw

struct ElArgs {
    const float *desc;
    const double *fitness;
    const unsigned char *mask;
    double *eliteFitness;
    float *eliteDesc;
    int *count, *cell, *winner, *parent, *nFilled;
    unsigned long long *key; // scratch: [M C]
    int *row;                // scratch: [M C], behind the keys; the sample kernel's list of filled cells
    float lo[4], inv[4];
    int word[4], bins[4];
    unsigned key0, key1, generation;
    int nDims, B, M, S, C, perBlock; // perBlock: S', children per block
};

// the order-preserving key of a fitness that is not a NaN: a > b in the order of rem2d_evolve.h iff key(a) > key(b)
DEV unsigned long long el_key(double f) {
    if (f == 0.0) f = 0.0; // -0 == +0
    const unsigned long long u = (unsigned long long)__double_as_longlong(f);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// the cell of row c, or -1 where the row is not admissible
DEV int el_cell(const ElArgs &A, long long c) {
    if (A.mask && A.mask[c] == 0) return -1;
    const double f = A.fitness[c];
    if (f != f) return -1;
    const float *x = A.desc + (size_t)c * (size_t)A.B;
    int q = 0, stride = 1;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < REM2D_ELITES_MAX_DIMS; ++i) {
        if (i < A.nDims) {
            const float v = x[A.word[i]];
            ok = ok && nv_finite(v);
            const float u = sn_mul(__fsub_rn(v, A.lo[i]), A.inv[i]);
            const int qi = u < 0.0f ? 0 : (u >= (float)A.bins[i] ? A.bins[i] - 1 : (int)u);
            q += qi * stride;
            stride *= A.bins[i];
        }
    }
    return ok ? q : -1;
}

__global__ __launch_bounds__(EL_TILE) void rem2d_elites_clear_kernel(ElArgs A) {
    const long long s = (long long)blockIdx.x * EL_TILE + (long long)threadIdx.x;
    if (s >= (long long)A.M * (long long)A.C) return;
    A.key[s] = 0ull;
    A.row[s] = 0x7fffffff;
    A.winner[s] = -1;
}

__global__ __launch_bounds__(EL_TILE) void rem2d_elites_key_kernel(ElArgs A) {
    const long long c = (long long)blockIdx.x * EL_TILE + (long long)threadIdx.x;
    if (c >= (long long)A.M * (long long)A.S) return;
    const int q = el_cell(A, c);
    A.cell[c] = q;
    if (q < 0) return;
    const long long slot = (c / (long long)A.S) * (long long)A.C + (long long)q;
    atomicMax(A.key + slot, el_key(A.fitness[c]));
}

__global__ __launch_bounds__(EL_TILE) void rem2d_elites_row_kernel(ElArgs A) {
    const long long c = (long long)blockIdx.x * EL_TILE + (long long)threadIdx.x;
    if (c >= (long long)A.M * (long long)A.S) return;
    const int q = A.cell[c];
    if (q < 0) return;
    const long long slot = (c / (long long)A.S) * (long long)A.C + (long long)q;
    if (A.key[slot] == el_key(A.fitness[c])) atomicMin(A.row + slot, (int)c);
}

// E: src = the evaluated sets, dst = the elite arrays, len and vec per array (evolve_args' fields; the rest is not looked at)
__global__ __launch_bounds__(WAVE) void rem2d_elites_commit_kernel(ElArgs A, EvolveArgs E) {
    const int lane = (int)threadIdx.x;
    const long long slot = (long long)blockIdx.x; // < M C: the grid is M C workgroups
    if (A.key[slot] == 0ull) return;              // no candidate: winner stays -1
    const int w = __builtin_amdgcn_readfirstlane(A.row[slot]);
    const double f = A.fitness[w];
    const int seen = A.count[slot];
    if (seen != 0 && !ev_greater(f, A.eliteFitness[slot])) return; // the incumbent holds (everyone has read the same words)
    const float *x = A.desc + (size_t)w * (size_t)A.B;
    float *y = A.eliteDesc + (size_t)slot * (size_t)A.B;
    if (lane < A.B) y[lane] = x[lane];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float *src = E.src[k] + (size_t)w * (size_t)E.len[k];
        float *dst = E.dst[k] + (size_t)slot * (size_t)E.len[k];
        if (E.vec[k]) ev_array<4>(src, dst, E.len[k], true, 0u, 0u, E, lane);
        else ev_array<1>(src, dst, E.len[k], true, 0u, 0u, E, lane);
    }
    if (lane == 0) {
        A.eliteFitness[slot] = f;
        A.count[slot] = seen + 1;
        A.winner[slot] = w;
    }
}

__global__ __launch_bounds__(EL_TILE) void rem2d_elites_sample_kernel(ElArgs A) {
    __shared__ int waveCount[EL_TILE / WAVE];
    __shared__ int base;
    const int t = (int)threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
    const long long b = (long long)blockIdx.x, s0 = b * (long long)A.C;
    int *list = A.row + s0;
    if (t == 0) base = 0;
    __syncthreads();
    for (int q0 = 0; q0 < A.C; q0 += EL_TILE) {
        const int q = q0 + t;
        const bool in = q < A.C && A.count[s0 + q] != 0;
        const unsigned long long m = __ballot(in);
        if (lane == 0) waveCount[wv] = __popcll(m);
        __syncthreads();
        int j = base + __popcll(m & ((1ull << lane) - 1ull));
        int all = 0;
#pragma unroll
        for (int w = 0; w < EL_TILE / WAVE; ++w) {
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
    for (int i = t; i < A.perBlock; i += EL_TILE) {
        const long long c = b * (long long)A.perBlock + (long long)i;
        int p = -1;
        if (n > 0) {
            const unsigned x0 = ev_philox(0u, (unsigned)c, A.generation, EL_DOMAIN, A.key0, A.key1).x0;
            const int j = (int)(((unsigned long long)x0 * (unsigned long long)(unsigned)n) >> 32);
            p = (int)(s0 + (long long)list[j]);
        }
        A.parent[c] = p;
    }
}

#endif
