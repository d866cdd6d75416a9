// rem2d_modular.h -- modular device policies (include/rem2d_modular.h): ONE controller of rem2d_policy.h's kind that runs once per
// body of a creature and exchanges K message words with the body's parent and children along the creature's tree, and the table
// of that tree in body order.
// Part of the single translation unit rem2d.hip (see its header comment); not a stand-alone header.  Included after rem2d_control.h
// (CtlTable, ctl_locate) and rem2d_policy.h, whose PolicyArgs, PolVec, pol_accumulate and pol_softsign it shares as they are; no
// other kernel is touched.
//
// rem2d_topology_kernel: rem2d_observe_kernel's launch shape (one lane per arena lane, a wavefront = one 64-lane block of one world,
// the worlds in a table in the kernel arguments).  The parent's BODY index is the rank of lane `parent` among the creature's live
// lanes: a ballot of the live lanes, shifted to the creature's group, and a population count below the parent's bit.  No LDS.
//
// rem2d_modular_forward_kernel: for population row r with weight set g, P rounds of
//     x_b = [head | body b | frac | shape_b | #children_b | sum of the children's messages | the parent's message]     (Dm words)
//     h_b = act(b1 + x_b w1)      m'_b = h_b[0 .. K)      and after the last round  t_b = scale * softsign(b2 + h_b w2)
// with the arithmetic of rem2d_policy.h (pol_accumulate: one rounded product, one rounded add, ascending input index).
//
// Launch shape: a workgroup is ONE wavefront that owns ONE row.  The row's weight set (Dm H + 2 H + 1 <= 78 * 128 + 257 words) is
// staged in LDS once and reused by every body and every round (16-byte loads where w1's rows are whole float4s and the set's base is
// aligned); so are the observation row, the ray fractions and the tree.  The two message buffers m^p / m^{p+1} [MB][K] alternate in
// LDS.  The 64 lanes are split over (body, hidden unit): LPB lanes (a power of two, 2 .. 64) serve one live body and own V
// consecutive hidden units each (V = 4 where H is a multiple of 4: ds_read_b128 of a weight row; else 1), so 64 / LPB bodies are
// evaluated side by side; the live bodies are walked in passes of that many, in ascending body order (a compacted list: empty
// slots cost nothing).  A round that is not the last needs only the K units that become messages -- the bits of h_k do not
// depend on the other units -- so it runs at the finer split LPB(K) and computes min(H, K rounded up to V) units; the last round
// computes all H and, by the first lane of each body, the output unit.  The children of a body are a linked list in ascending body
// order (first / next), built once per row by one lane per body from a single descending sweep over the parents: the 63-add chain
// of a star is walked in that order, one rounded add per child.
// LDS: at most 10241 (weights) + 2 * 64 K (messages) + 32 Dm (x, 64 / LPB <= 32 bodies) + 256 (h) + 392 + 64 (row) + 384 (tree) words;
// K <= 31 and Dm <= 78 (R + 2 + 2 K <= 64) keep the sum under 14 976 words = 58.5 KB, inside the 64 KB a workgroup may ask for
// (modular_lds below computes the exact figure, which the launcher checks).
//
// topo may hold anything: a parent is accepted only if it lies in [0, MB), is not the body itself and is live; a child must be
// live; `next` only ever grows, so every list ends; nothing follows more than one edge.  All indices into LDS and into the row's
// arrays are body indices < MB or list entries made from them.
//
// In place: a row belongs to exactly one wavefront, and no row reads another row's memory.  The row's messages are loaded from
// memory[r][..] in the staging phase and stored into LDS (m^0) there; every such LDS store consumes its global load's data, so the
// wavefront -- which issues its instructions in program order -- has received ALL of the row's memory words before it passes the
// first lds_sync.  The stores to memory[r][..] are issued after the last round, which lies behind that lds_sync in program order,
// and they take their values from the LDS buffer m^P, itself written by instructions behind it: the order is through data and
// program order of one wavefront, not through timing.  A skipped row (row mask, index outside [0, G)) leaves before anything of it
// is read: its targets, valid bytes and memory are neither read nor written.
// Plain vector loads and stores, no atomics, no scratch.
#ifndef REM2D_MODULAR_KERNELS_H
#define REM2D_MODULAR_KERNELS_H

__global__ __launch_bounds__(CTL_THREADS) void rem2d_topology_kernel(CtlTable Tb, int maxBodies, int *out, long long outRows) {
    CtlLane c;
    if (!ctl_locate(Tb, c)) return;
    CTL_SCOPE(c);
    const int K = c.K, base = c.base, sub = c.sub, body = c.body, nBodies = c.nBodies;
    // (every lane of the block loads: the arena is padded to whole blocks, and the ballot wants all lanes)
    const int shape = LI(L_SHAPE), parent = LI(L_PARENT);
    const unsigned long long grp = (__ballot(c.live) >> base) & (K == WAVE ? ~0ull : ((1ull << K) - 1ull));
    if (!c.inWorld) return;
    const long long r = S.index ? (long long)S.index[env] : (long long)env;
    if (r < 0 || r >= outRows) return;
    int *row = out + (size_t)r * (size_t)maxBodies * 2;
    if (c.live) {
        if (body < maxBodies) {
            int pb = -1;
            if (parent >= 0 && parent < K && ((grp >> parent) & 1ull)) pb = __popcll(grp & ((1ull << parent) - 1ull));
            row[2 * body] = pb < maxBodies ? pb : -1;
            row[2 * body + 1] = shape;
        }
    } else { // the d-th empty lane of the creature clears body slot nBodies + d
        const int slot = nBodies + (sub - body);
        if (slot < maxBodies) { row[2 * slot] = -1; row[2 * slot + 1] = 0; }
    }
    if (sub == 0)
        for (int slot = K; slot < maxBodies; ++slot) { row[2 * slot] = -1; row[2 * slot + 1] = 0; } // slots no lane of this bucket stands for
}

struct ModularArgs {
    PolicyArgs P; // P.D = Dm, P.MB the row side's body columns, P.lpr the lanes per body of the LAST round (LPB(H))
    const int *topo;
    float *memory;
    const unsigned char *reset;
    int K, rounds;
    int lpbK; // lanes per body of the rounds before the last (LPB(K))
};

#define MOD_MIN_LPB 2 // at most 32 bodies side by side: bounds xs
static __host__ __device__ __forceinline__ int mod_align4(int n) { return (n + 3) & ~3; }
// The LDS of a workgroup, in words, and where its parts begin (the kernel and the launcher share it).
struct ModularLds {
    int w1, b1, w2, b2, m0, m1, obs, frac, xs, hs, par, first, next, nch, shape, list, words;
};
static __host__ __device__ __forceinline__ ModularLds modular_lds(int Dm, int H, int MB, int R, int K, int lpbH, int lpbK) {
    ModularLds L;
    int at = 0;
    L.w1 = at; at += Dm * H;
    L.b1 = at; at += H;
    L.w2 = at; at += H;
    L.b2 = at; at = mod_align4(at + 1);
    L.m0 = at; at += MB * K;
    L.m1 = at; at += MB * K;
    L.obs = at; at += REM2D_OBS_HEAD + REM2D_OBS_BODY * MB;
    L.frac = at; at += R;
    const int bppH = WAVE / lpbH, bppK = WAVE / lpbK;
    L.xs = at; at += (bppH > bppK ? bppH : bppK) * Dm;
    L.hs = at; at += bppH * H;
    L.par = at; at += MB;
    L.first = at; at += MB;
    L.next = at; at += MB;
    L.nch = at; at += MB;
    L.shape = at; at += MB;
    L.list = at; at += MB;
    L.words = at;
    return L;
}

// n words from global memory into LDS by the whole wavefront; 16-byte loads where both sides allow
DEV void mod_stage(float *dst, const float *src, int n, int lane) {
    if ((n & 3) == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0) {
        for (int i = lane * 4; i < n; i += WAVE * 4) *(pol_f4 *)(dst + i) = *(const pol_f4 *)(src + i);
    } else {
        for (int i = lane; i < n; i += WAVE) dst[i] = src[i];
    }
}

// One round for the live bodies list[0 .. nLive): LPB lanes per body, V units per lane.  LAST: all H units, h kept, the output unit.
template <int V, bool LAST>
DEV void mod_round(const ModularArgs &Q, float *lds, const ModularLds &L, int lane, long long r, int nLive, const float *cur, float *nxt) {
    const PolicyArgs &P = Q.P;
    const int Dm = P.D, H = P.H, R = P.R, K = Q.K;
    const int lpb = LAST ? P.lpr : Q.lpbK, bpp = WAVE / lpb;
    const int s = lane / lpb, u = lane & (lpb - 1); // body of the pass, lane inside the body
    const int nUnits = LAST ? H : min(H, (K + V - 1) / V * V);
    const int *par = (const int *)(lds + L.par), *first = (const int *)(lds + L.first), *next = (const int *)(lds + L.next);
    const int *nch = (const int *)(lds + L.nch), *shape = (const int *)(lds + L.shape), *list = (const int *)(lds + L.list);
    float *x = lds + L.xs + s * Dm, *h = lds + L.hs + s * H;
    const int oShape = REM2D_OBS_HEAD + REM2D_OBS_BODY + R, oCm = oShape + 2, oPm = oCm + K;
    for (int i0 = 0; i0 < nLive; i0 += bpp) {
        const bool on = i0 + s < nLive;
        const int b = on ? list[i0 + s] : 0;
        if (on) { // the body's input row
            const int pb = par[b];
            for (int w = u; w < Dm; w += lpb) {
                float v;
                if (w < REM2D_OBS_HEAD) v = lds[L.obs + w];
                else if (w < REM2D_OBS_HEAD + REM2D_OBS_BODY) v = lds[L.obs + REM2D_OBS_BODY * b + w];
                else if (w < oShape) v = lds[L.frac + (w - REM2D_OBS_HEAD - REM2D_OBS_BODY)];
                else if (w == oShape) v = (float)shape[b];
                else if (w == oShape + 1) v = (float)nch[b];
                else if (w < oPm) { // the children's messages, summed in ascending body order
                    const int k = w - oCm;
                    v = 0.0f;
                    for (int c = first[b]; c >= 0; c = next[c]) v = __fadd_rn(v, cur[c * K + k]);
                } else v = pb >= 0 ? cur[pb * K + (w - oPm)] : 0.0f;
                x[w] = v;
            }
        }
        lds_sync();
        if (on) {
            for (int j = u * V; j < nUnits; j += lpb * V) {
                float a[V];
#pragma unroll
                for (int v = 0; v < V; ++v) a[v] = lds[L.b1 + j + v];
                pol_accumulate<V>(x, Dm, lds + L.w1, H, j, a);
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const float hv = P.act == REM2D_POLICY_RELU ? (a[v] > 0.0f ? a[v] : 0.0f) : pol_softsign(a[v]);
                    if (LAST) h[j + v] = hv;
                    if (j + v < K) nxt[b * K + j + v] = hv; // the body's next message
                }
            }
        }
        lds_sync();
        if (LAST && on && u == 0) {
            float y[1] = {lds[L.b2]};
            pol_accumulate<1>(h, H, lds + L.w2, 1, 0, y);
            const float t = __fmul_rn(P.scale, pol_softsign(y[0]));
            const size_t at = (size_t)r * (size_t)P.MB + (size_t)b;
            P.targets[at] = (double)t;
            P.valid[at] = (__float_as_uint(t) & 0x7f800000u) != 0x7f800000u ? 1 : 0;
        }
        lds_sync(); // (x and h are the next pass's)
    }
}

template <int V> __global__ __launch_bounds__(WAVE) void rem2d_modular_forward_kernel(ModularArgs Q) {
    extern __shared__ __attribute__((aligned(16))) float mod_lds[];
    const PolicyArgs &P = Q.P;
    const int lane = (int)threadIdx.x;
    const long long r = (long long)blockIdx.x; // < P.nRows: the grid is the rows
    // (wave-uniform: the wavefront is the row)
    if (P.rowMask && P.rowMask[r] == 0) return;
    const long long g = P.index ? (long long)P.index[r] : r;
    if (g < 0 || g >= (long long)P.G) return;
    const int Dm = P.D, H = P.H, MB = P.MB, R = P.R, K = Q.K;
    const ModularLds L = modular_lds(Dm, H, MB, R, K, P.lpr, Q.lpbK);
    float *lds = mod_lds;
    // ---- the weight set, the row and its messages
    mod_stage(lds + L.w1, P.w1 + (size_t)g * (size_t)Dm * (size_t)H, Dm * H, lane);
    mod_stage(lds + L.b1, P.b1 + (size_t)g * (size_t)H, H, lane);
    mod_stage(lds + L.w2, P.w2 + (size_t)g * (size_t)H, H, lane);
    if (lane == 0) lds[L.b2] = P.b2[g];
    const int nObs = REM2D_OBS_HEAD + REM2D_OBS_BODY * MB;
    mod_stage(lds + L.obs, P.obs + (size_t)r * (size_t)nObs, nObs, lane);
    if (R > 0) mod_stage(lds + L.frac, P.frac + (size_t)r * (size_t)R, R, lane);
    // ---- the tree: lane b is body b
    int pr = -1, shp = 0;
    if (lane < MB) {
        const int *t = Q.topo + ((size_t)r * (size_t)MB + (size_t)lane) * 2;
        pr = t[0];
        shp = t[1];
    }
    const bool live = shp != 0;
    const unsigned long long liveMask = __ballot(live);
    if (!(live && pr >= 0 && pr < MB && pr != lane && ((liveMask >> pr) & 1ull))) pr = -1;
    int *par = (int *)(lds + L.par), *list = (int *)(lds + L.list);
    if (lane < MB) {
        par[lane] = pr;
        ((int *)(lds + L.shape))[lane] = shp;
    }
    if (live) list[__popcll(liveMask & ((1ull << lane) - 1ull))] = lane;
    const int nLive = __popcll(liveMask);
    float *mem = Q.memory + (size_t)r * (size_t)MB * (size_t)K;
    const bool fresh = Q.reset && Q.reset[r] != 0; // substituted, not multiplied: memory is not read at all
    for (int i = lane; i < MB * K; i += WAVE) lds[L.m0 + i] = !fresh && ((liveMask >> (i / K)) & 1ull) ? mem[i] : 0.0f;
    lds_sync();
    {   // first child, next sibling and the number of children, from one descending sweep: the smallest index is written last
        int first = -1, next = -1, n = 0;
        for (int c = MB - 1; c >= 0; --c) {
            const int p = par[c];
            if (p == lane) { first = c; ++n; }
            if (c > lane && pr >= 0 && p == pr) next = c;
        }
        if (lane < MB) {
            ((int *)(lds + L.first))[lane] = first;
            ((int *)(lds + L.next))[lane] = next;
            ((int *)(lds + L.nch))[lane] = n;
        }
    }
    lds_sync();
    // ---- the rounds
    float *cur = lds + L.m0, *nxt = lds + L.m1;
    for (int p = 0; p + 1 < Q.rounds; ++p) {
        mod_round<V, false>(Q, lds, L, lane, r, nLive, cur, nxt);
        float *t = cur; cur = nxt; nxt = t;
    }
    mod_round<V, true>(Q, lds, L, lane, r, nLive, cur, nxt);
    // ---- what the row keeps: the live bodies' messages; the empty slots read zero everywhere
    for (int i = lane; i < MB * K; i += WAVE) mem[i] = ((liveMask >> (i / K)) & 1ull) ? nxt[i] : 0.0f;
    if (lane < MB && !live) {
        const size_t at = (size_t)r * (size_t)MB + (size_t)lane;
        P.targets[at] = 0.0;
        P.valid[at] = 0;
    }
}

#endif
