// rem2d_obsnorm.h -- observation normalisation for device policies (include/rem2d_obsnorm.h): exact running sums of the policies'
// input words, the tables made of them, and the application that the forward kernels of rem2d_policy.h / rem2d_recurrent.h stage
// their rows through (their NORM instantiations; this file comes before them).
// Part of the single translation unit rem2d.hip (see its header comment); not a stand-alone header.
//
// State per block b of S consecutive rows: count[b], and per word i < Dn = 8 + 6 MB + R: s1, s2hi, s2lo, all int64.  A row
// contributes iff its mask byte is set (or there is no mask) and ALL its Dn words are finite; then per word
//     c = clamp(x, -2048, 2048);  q = (int64)rintf(c * 4096.0f);  s1 += q;  p = q q;  s2hi += p >> 23;  s2lo += p & (2^23 - 1)
// Integer sums: the same bits in any order.
//
// Launch shape of the accumulation: a workgroup is ON_WAVES = 4 wavefronts; wavefront w of workgroup g takes item 4 g + w, item
// (b, c) being rows [b S + c rowChunk, b S + min(S, (c + 1) rowChunk)) of block b, cut at nRows.  Lane l owns words l, l + 64, ...
// (WPL = 1, 2, 4 or 8 of them: Dn <= 456), so a row is WPL coalesced dword reads of the wavefront; ON_UNROLL = 4 rows are loaded
// before the first is summed.  The finiteness of a row is one __ballot over the wavefront, whose 64 lanes are all in the loop (its
// bounds are wave-uniform).  The sums of a wavefront's rows stay in registers (3 WPL int64 per lane).  Where a block has more than
// one item (nChunks > 1), the wavefronts of a workgroup that follow one of the same block hand their sums over through LDS
// (__syncthreads; 3 slots of 3 WPL 64 + 1 int64: 36.9 KB at WPL = 8, 9.2 KB at the workload's WPL = 2) and the first of the run adds
// them up; then one 64-bit integer atomicAdd per non-zero (word, sum) of the run and one for the count.  Blocks of 16 rows: one
// wavefront per block, no LDS, no barrier.  One block of 65 536 rows at rowChunk 32: 2048 wavefronts, 512 atomics per address.
// Plain vector loads; the only stores are the atomics.
//
// The tables: one thread per (block, word), binary64 operations kept apart by on_keep so that -ffp-contract=fast finds nothing to
// fuse (include/rem2d_obsnorm.h section 3 states them one by one).
#ifndef REM2D_OBSNORM_KERNELS_H
#define REM2D_OBSNORM_KERNELS_H

#define ON_THREADS 256
#define ON_WAVES (ON_THREADS / WAVE)
#define ON_UNROLL 4
#define ON_MAX_WPL 8 // words per lane: Dn <= 8 + 6 * 64 + 64 = 456 <= 8 * 64

// ---- the application: what a forward kernel stages for word x of a row whose block has (mu, inv) for it ----
struct PolNorm {
    const float *mu, *inv; // [M][Dn]
    float clip;
    int S, Dn;
};
DEV float on_apply(float x, float mu, float inv, float clip) {
    const float t = sn_mul(__fsub_rn(x, mu), inv);
    return t > clip ? clip : (t < -clip ? -clip : t);
}

// ---- the accumulation ----
struct OnArgs {
    const float *obs, *frac;
    const unsigned char *rowMask;
    long long *count, *s1, *s2hi, *s2lo;
    long long nRows, items;
    int nObs, R, Dn, S, rowChunk, nChunks; // nChunks: items per block
};

template <int WPL> __global__ __launch_bounds__(ON_THREADS) void rem2d_obsnorm_accumulate_kernel(OnArgs A) {
    extern __shared__ long long on_lds[];
    constexpr int SLOT = 3 * WPL * WAVE + 1;
    const int lane = (int)threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / WAVE);
    const long long item = (long long)blockIdx.x * ON_WAVES + wave;
    const bool have = item < A.items;
    long long b = 0, r0 = 0, r1 = 0;
    if (have) {
        b = item / A.nChunks;
        const long long c = item - b * A.nChunks, first = b * (long long)A.S;
        r0 = first + c * (long long)A.rowChunk;
        r1 = first + std::min((long long)A.S, (c + 1) * (long long)A.rowChunk);
        r1 = std::min(r1, A.nRows);
    }
    long long a1[WPL], ah[WPL], al[WPL], cnt = 0;
#pragma unroll
    for (int k = 0; k < WPL; ++k) a1[k] = ah[k] = al[k] = 0;
    for (long long r = r0; r < r1; r += ON_UNROLL) {
        float x[ON_UNROLL][WPL];
        bool live[ON_UNROLL];
#pragma unroll
        for (int j = 0; j < ON_UNROLL; ++j) {
            const long long row = r + j;
            live[j] = row < r1 && (!A.rowMask || A.rowMask[row] != 0);
#pragma unroll
            for (int k = 0; k < WPL; ++k) {
                const int w = lane + k * WAVE;
                float v = 0.0f; // (a lane without a word of this row: finite, and q = 0)
                if (live[j] && w < A.Dn)
                    v = w < A.nObs ? A.obs[(size_t)row * (size_t)A.nObs + (size_t)w] : A.frac[(size_t)row * (size_t)A.R + (size_t)(w - A.nObs)];
                x[j][k] = v;
            }
        }
#pragma unroll
        for (int j = 0; j < ON_UNROLL; ++j) {
            bool fin = true;
#pragma unroll
            for (int k = 0; k < WPL; ++k) fin = fin && (__float_as_uint(x[j][k]) & 0x7f800000u) != 0x7f800000u;
            if (live[j] && __ballot(!fin) == 0ull) { // the row-wide vote: every lane of the wavefront is here
                cnt += 1;
#pragma unroll
                for (int k = 0; k < WPL; ++k) {
                    const float v = x[j][k];
                    const float c = v < -2048.0f ? -2048.0f : (v > 2048.0f ? 2048.0f : v);
                    const long long q = (long long)(int)rintf(__fmul_rn(c, 4096.0f));
                    const long long p = q * q;
                    a1[k] += q;
                    ah[k] += p >> 23;
                    al[k] += p & 0x7fffffLL;
                }
            }
        }
    }
    bool head = true;
    if (A.nChunks > 1) { // (uniform over the launch) the wavefronts of a workgroup that hold the same block: add up in LDS
        head = wave == 0 || !have || (item - 1) / A.nChunks != b;
        if (!head) {
            long long *slot = on_lds + (size_t)(wave - 1) * SLOT;
#pragma unroll
            for (int k = 0; k < WPL; ++k) {
                slot[(0 * WPL + k) * WAVE + lane] = a1[k];
                slot[(1 * WPL + k) * WAVE + lane] = ah[k];
                slot[(2 * WPL + k) * WAVE + lane] = al[k];
            }
            if (lane == 0) slot[3 * WPL * WAVE] = cnt;
        }
        __syncthreads();
        if (have && head)
            for (int w2 = wave + 1; w2 < ON_WAVES && item + (w2 - wave) < A.items && (item + (w2 - wave)) / A.nChunks == b; ++w2) {
                const long long *slot = on_lds + (size_t)(w2 - 1) * SLOT;
#pragma unroll
                for (int k = 0; k < WPL; ++k) {
                    a1[k] += slot[(0 * WPL + k) * WAVE + lane];
                    ah[k] += slot[(1 * WPL + k) * WAVE + lane];
                    al[k] += slot[(2 * WPL + k) * WAVE + lane];
                }
                cnt += slot[3 * WPL * WAVE];
            }
    }
    if (!have || !head || cnt == 0) return;
    const size_t at = (size_t)b * (size_t)A.Dn;
#pragma unroll
    for (int k = 0; k < WPL; ++k) {
        const int w = lane + k * WAVE;
        if (w < A.Dn) {
            if (a1[k]) atomicAdd((unsigned long long *)(A.s1 + at + w), (unsigned long long)a1[k]);
            if (ah[k]) atomicAdd((unsigned long long *)(A.s2hi + at + w), (unsigned long long)ah[k]);
            if (al[k]) atomicAdd((unsigned long long *)(A.s2lo + at + w), (unsigned long long)al[k]);
        }
    }
    if (lane == 0) atomicAdd((unsigned long long *)(A.count + b), (unsigned long long)cnt);
}

// ---- the tables ----
struct OnFreezeArgs {
    const long long *count, *s1, *s2hi, *s2lo;
    float *mu, *inv;
    long long total, minCount; // total = M Dn
    int Dn;
    float minVar;
};
// a binary64 value the compiler must take as it is: keeps a product from being fused into the difference that consumes it
DEV double on_keep(double x) {
    asm volatile("" : "+v"(x));
    return x;
}
__global__ __launch_bounds__(ON_THREADS) void rem2d_obsnorm_freeze_kernel(OnFreezeArgs A) {
    const long long i = (long long)blockIdx.x * ON_THREADS + (long long)threadIdx.x;
    if (i >= A.total) return;
    const long long n = A.count[i / A.Dn];
    float mu = 0.0f, inv = 1.0f;
    if (n >= A.minCount) {
        const double nd = (double)n;
        const double m = on_keep((double)A.s1[i] / nd);
        const double hi = on_keep((double)A.s2hi[i] * 8388608.0);
        const double s2 = on_keep(on_keep(hi + (double)A.s2lo[i]) / nd);
        const double mm = on_keep(m * m);
        double v = on_keep(s2 - mm);
        if (!(v > 0.0)) v = 0.0;
        mu = (float)on_keep(m / 4096.0);
        const float vx = (float)on_keep(v / 16777216.0);
        inv = vx >= A.minVar ? 1.0f / sqrtf(vx) : 0.0f;
    }
    A.mu[i] = mu;
    A.inv[i] = inv;
}

#endif
