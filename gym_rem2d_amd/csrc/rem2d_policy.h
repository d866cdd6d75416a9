// rem2d_policy.h -- device policies (include/rem2d_policy.h): a small feed-forward controller per creature, evaluated for a whole
// population between observe / sense and control.
// Part of the single translation unit rem2d.hip (see its header comment); not a stand-alone header.
//
// For population row r with weight set g (index[r], or r): x = the row of rem2d_worlds_observe followed by the R ray fractions of
// rem2d_worlds_sense, D = 8 + 6 MB + R words.
//     a_j = b1[j];  for i = 0 .. D-1:  a_j = a_j + (x_i * w1[i][j])        h_j = act(a_j)
//     y_m = b2[m];  for j = 0 .. H-1:  y_m = y_m + (h_j * w2[j][m])        t_m = scale * (y_m / (1 + |y_m|))
// targets[r][m] = (double)t_m, valid[r][m] = isfinite(t_m).  act: SOFTSIGN a / (1 + |a|), or RELU a > 0 ? a : +0.
//
// Arithmetic: every product and every sum is one separately rounded binary32 operation, in ascending order of i / j, in all three
// builds: the products go through sn_mul (rem2d_sense.h), i.e. sn_keep of rem2d_math.h, so that -ffp-contract=fast finds nothing to
// fuse.  `/` is the correctly rounded division the engine uses.  No transcendental function.
//
// Launch shape: a workgroup is ONE wavefront that owns RPW = 64 / LPR consecutive rows; the LPR lanes of a row (a power of two, 8 ..
// 64) each own V consecutive output units of a layer, consecutive lanes consecutive units, so a weight row [n_out] is one contiguous
// read of a wave-instruction.  V = 4 (16-byte loads) where the layer's width is a multiple of 4 and its weight base is 16-byte
// aligned, V = 1 (dword loads) otherwise; a layer wider than V LPR units is walked in passes.  x and h of the wavefront's rows are
// staged in LDS (RPW (D + H) words, dynamic) and read back as broadcasts: every lane of a row reads the same word.  The i loop is
// unrolled by POL_UNROLL = 8: the 8 weight loads are issued before the add chain that depends on them.  The hand-over through LDS
// stays inside the wavefront (lds_sync).  A row that the row mask clears or whose index lies outside [0, G) is a branch around all of
// it: nothing of it is read and its outputs stay as they are.  Plain vector loads and stores, no atomics, no scratch.
#ifndef REM2D_POLICY_KERNELS_H
#define REM2D_POLICY_KERNELS_H

#define POL_UNROLL 8
#define POL_MIN_LPR 8 // at most 8 rows per wavefront: bounds the LDS of a wavefront (2368 words at the worst shape)

struct PolicyArgs {
    const float *w1, *b1, *w2, *b2;
    const int *index;
    const unsigned char *rowMask;
    const float *obs, *frac;
    double *targets;
    unsigned char *valid;
    long long nRows;
    int D, MB, R, H, G, act, lpr;
    float scale;
};

typedef float pol_f4 __attribute__((ext_vector_type(4)));
template <int V> struct PolVec;
template <> struct PolVec<1> {
    float v[1];
    DEV void load(const float *p) { v[0] = *p; }
};
template <> struct PolVec<4> {
    float v[4];
    DEV void load(const float *p) {
        const pol_f4 q = *(const pol_f4 *)p;
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
};

// a[v] = a[v] + (xs[i] * w[i][unit + v]) for i = 0 .. nIn-1, in that order; xs in LDS, w [nIn][nOut] in global memory
template <int V> DEV void pol_accumulate(const float *xs, int nIn, const float *w, int nOut, int unit, float (&a)[V]) {
    const float *p = w + unit;
    int i = 0;
    for (; i + POL_UNROLL <= nIn; i += POL_UNROLL) {
        PolVec<V> wv[POL_UNROLL];
#pragma unroll
        for (int k = 0; k < POL_UNROLL; ++k) wv[k].load(p + (size_t)(i + k) * (size_t)nOut);
#pragma unroll
        for (int k = 0; k < POL_UNROLL; ++k) {
            const float x = xs[i + k];
#pragma unroll
            for (int v = 0; v < V; ++v) a[v] = __fadd_rn(a[v], sn_mul(x, wv[k].v[v]));
        }
    }
    for (; i < nIn; ++i) {
        PolVec<V> wv;
        wv.load(p + (size_t)i * (size_t)nOut);
        const float x = xs[i];
#pragma unroll
        for (int v = 0; v < V; ++v) a[v] = __fadd_rn(a[v], sn_mul(x, wv.v[v]));
    }
}

DEV float pol_softsign(float a) { return a / __fadd_rn(1.0f, __builtin_fabsf(a)); }

// The second kernel argument of a forward kernel: nothing, or with NORM the normaliser's tables (rem2d_obsnorm.h: PolNorm,
// on_apply).  The NORM = false instantiations hold the code they held before NORM existed.
struct PolNoNorm {};
template <bool NORM> struct PolNormArg { typedef PolNoNorm type; };
template <> struct PolNormArg<true> { typedef PolNorm type; };

// V1 / V2: output units a lane owns per pass of the hidden / the output layer; NORM: the row is staged through on_apply
template <int V1, int V2, bool NORM = false>
__global__ __launch_bounds__(WAVE) void rem2d_policy_forward_kernel(PolicyArgs P, typename PolNormArg<NORM>::type Nm) {
    extern __shared__ float pol_lds[];
    const int lane = (int)threadIdx.x, lpr = P.lpr;
    const int sub = lane / lpr, u = lane & (lpr - 1); // row of the wavefront, lane inside the row
    const long long r = (long long)blockIdx.x * (long long)(WAVE / lpr) + (long long)sub;
    bool on = r < P.nRows;
    if (on && P.rowMask) on = P.rowMask[r] != 0;
    long long g = r;
    if (on && P.index) g = (long long)P.index[r];
    on = on && g >= 0 && g < (long long)P.G;
    float *xs = pol_lds + (size_t)sub * (size_t)(P.D + P.H), *hs = xs + P.D;
    if (on) { // the row's input: observation words, then ray fractions
        const int nObs = P.D - P.R;
        const float *obs = P.obs + (size_t)r * (size_t)nObs;
        if constexpr (NORM) { // the row's block of S consecutive rows names its tables
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
