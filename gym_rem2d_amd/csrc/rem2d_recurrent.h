// rem2d_recurrent.h -- recurrent device policies (include/rem2d_recurrent.h): the controller of rem2d_policy.h with K context units
// per creature, carried in device memory and rewritten in place by the kernel that evaluates the population.
// Part of the single translation unit rem2d.hip (see its header comment); not a stand-alone header.  Included after rem2d_policy.h,
// whose PolicyArgs, PolVec, pol_accumulate and pol_softsign it shares; rem2d_policy_forward_kernel itself is not touched.
//
// For population row r with weight set g: x = the observation row, the R ray fractions, then c_0 .. c_{K-1} with
// c_k = (reset && reset[r]) ? +0.0f : memory[r][k]; D = 8 + 6 MB + R + K words.  a_j, h_j, y_m, t_m, targets and valid as in
// rem2d_policy.h over these D words; then memory[r][k] = h_k for k < K, as computed.
//
// Launch shape: rem2d_policy_forward_kernel's -- one wavefront per workgroup, RPW = 64 / LPR consecutive rows, x and h staged in LDS
// (RPW (D + H) words; R + K <= 64, so the feed-forward kernel's bound of 2368 words holds), 16-byte weight loads where a layer allows.
// The context words are read into xs in the staging phase, before the first lds_sync; memory is written from the row's own lanes
// after the hidden layer, from hs, consecutive lanes consecutive words.
//
// In place: a row belongs to exactly one wavefront, and no row reads another row's memory.  Inside the wavefront every h_k is a
// function of ALL D staged words -- the add chain of pol_accumulate runs over the whole of xs -- and xs is read only after the
// lds_sync that follows the staging stores, each of which needed its global load's data.  So the loads of memory[r][..] have
// completed before the first store to memory[r][..] can issue: the dependence is through data, not through timing.  A skipped row
// (row mask, index outside [0, G)) is a branch around all of it: its memory is neither read nor written.
// Plain vector loads and stores, no atomics, no scratch.
#ifndef REM2D_RECURRENT_KERNELS_H
#define REM2D_RECURRENT_KERNELS_H

struct RecurrentArgs {
    PolicyArgs P; // P.D counts the context words, P.R the rays alone
    float *memory;
    const unsigned char *reset;
    int K;
};

// V1 / V2: output units a lane owns per pass of the hidden / the output layer; NORM (as in rem2d_policy.h): the observation words
// and the ray fractions are staged through on_apply, the context words as they are
template <int V1, int V2, bool NORM = false>
__global__ __launch_bounds__(WAVE) void rem2d_recurrent_forward_kernel(RecurrentArgs Q, typename PolNormArg<NORM>::type Nm) {
    extern __shared__ float rec_lds[];
    const PolicyArgs &P = Q.P;
    const int lane = (int)threadIdx.x, lpr = P.lpr;
    const int sub = lane / lpr, u = lane & (lpr - 1); // row of the wavefront, lane inside the row
    const long long r = (long long)blockIdx.x * (long long)(WAVE / lpr) + (long long)sub;
    bool on = r < P.nRows;
    if (on && P.rowMask) on = P.rowMask[r] != 0;
    long long g = r;
    if (on && P.index) g = (long long)P.index[r];
    on = on && g >= 0 && g < (long long)P.G;
    float *xs = rec_lds + (size_t)sub * (size_t)(P.D + P.H), *hs = xs + P.D;
    float *mem = Q.memory + (size_t)(on ? r : 0) * (size_t)Q.K;
    if (on) { // the row's input: observation words, ray fractions, context words
        const int nObs = P.D - P.R - Q.K;
        const float *obs = P.obs + (size_t)r * (size_t)nObs;
        if constexpr (NORM) {
            const size_t tb = (size_t)(r / (long long)Nm.S) * (size_t)Nm.Dn;
            const float *mu = Nm.mu + tb, *inv = Nm.inv + tb;
            for (int i = u; i < nObs; i += lpr) xs[i] = on_apply(obs[i], mu[i], inv[i], Nm.clip);
            if (P.R > 0) {
                const float *frac = P.frac + (size_t)r * (size_t)P.R;
                for (int i = u; i < P.R; i += lpr) xs[nObs + i] = on_apply(frac[i], mu[nObs + i], inv[nObs + i], Nm.clip);
            }
        } else {
            for (int i = u; i < nObs; i += lpr) xs[i] = obs[i];
            if (P.R > 0) {
                const float *frac = P.frac + (size_t)r * (size_t)P.R;
                for (int i = u; i < P.R; i += lpr) xs[nObs + i] = frac[i];
            }
        }
        const bool fresh = Q.reset && Q.reset[r] != 0; // substituted, not multiplied: memory is not read at all
        for (int k = u; k < Q.K; k += lpr) xs[nObs + P.R + k] = fresh ? 0.0f : mem[k];
    }
    lds_sync();
    if (on) {
        const float *w1 = P.w1 + (size_t)g * (size_t)P.D * (size_t)P.H, *b1 = P.b1 + (size_t)g * (size_t)P.H;
        for (int j = u * V1; j < P.H; j += lpr * V1) {
            float a[V1];
#pragma unroll
            for (int v = 0; v < V1; ++v) a[v] = b1[j + v];
            pol_accumulate<V1>(xs, P.D, w1, P.H, j, a);
#pragma unroll
            for (int v = 0; v < V1; ++v) hs[j + v] = P.act == REM2D_POLICY_RELU ? (a[v] > 0.0f ? a[v] : 0.0f) : pol_softsign(a[v]);
        }
    }
    lds_sync();
    if (on) {
        for (int k = u; k < Q.K; k += lpr) mem[k] = hs[k]; // the next step's context (K <= H)
        const float *w2 = P.w2 + (size_t)g * (size_t)P.H * (size_t)P.MB, *b2 = P.b2 + (size_t)g * (size_t)P.MB;
        const size_t out = (size_t)r * (size_t)P.MB;
        for (int m = u * V2; m < P.MB; m += lpr * V2) {
            float y[V2];
#pragma unroll
            for (int v = 0; v < V2; ++v) y[v] = b2[m + v];
            pol_accumulate<V2>(hs, P.H, w2, P.MB, m, y);
#pragma unroll
            for (int v = 0; v < V2; ++v) {
                const float t = __fmul_rn(P.scale, pol_softsign(y[v]));
                P.targets[out + (size_t)(m + v)] = (double)t;
                P.valid[out + (size_t)(m + v)] = (__float_as_uint(t) & 0x7f800000u) != 0x7f800000u ? 1 : 0;
            }
        }
    }
}

#endif
