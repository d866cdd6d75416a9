// rem2d_control.h -- closed-loop control (include/rem2d_control.h): observation rows and controller writes of a whole population.
// Part of the single translation unit rem2d.hip (see its header comment); not a stand-alone header.
//
// No step kernel knows about any of this.  Both kernels run between two steps on the state arena alone, one lane per (creature,
// lane of the arena) exactly as the step kernels lay the bodies out, so every field access is a coalesced load / store (lane
// fastest) and the parent's angle / velocity come by __shfl from lane `parent` of the creature's K-lane group, as in `pre`
// (rem2d_pipeline.h).  A wavefront = one 64-lane block of ONE world; the worlds of a launch (all lane buckets and step groups of a
// population) sit in a table in the kernel arguments, like the Batch of rem2d_worlds_step: 16 small launches twice per env-step
// would be a measurable share of a 1 ms step.
//
// Body index of a lane = its rank among the creature's live lanes (ballot + prefix count inside the group): the order of
// robot.components and of the oracle's bodies.
//
// Arithmetic: each observed difference is one __fsub_rn (never contracted), everything else a copy or an exact conversion -- the
// -ffp-contract=fast build writes the same bits.  Plain C++ loads and stores only.
#ifndef REM2D_CONTROL_KERNELS_H
#define REM2D_CONTROL_KERNELS_H

#define CTL_TABLE 16    // worlds per launch (a population of 4 lane buckets x 4 step groups); more are split into chunks
#define CTL_THREADS 256 // four wavefronts = four 64-lane blocks per workgroup
static_assert(REM2D_CONTROL_MAX_BODIES == WAVE, "a creature's bodies are the lanes of one wavefront");

struct CtlWorld { // the members the accessors of rem2d_state.h go through (as `S`), the population index and the world's blocks
    char *lane4, *lane8, *slot4, *env8;
    const int *index;  // creature -> population row (rem2d_world_set_outputs), nullptr: the identity
    unsigned Lp, Np, nEnvs, lanes;
    unsigned blockEnd; // 64-lane blocks of this launch up to and including this world's
    unsigned pad;
};
struct CtlTable {
    CtlWorld w[CTL_TABLE];
    int n;
};

// Which world and which of its lanes a thread serves.
struct CtlLane {
    CtlWorld S;        // the world of this wavefront
    int world;         // ... and its index in the launch's table
    unsigned gl, env;  // arena lane (< Lp) and creature of this thread
    int K, base, sub;  // lanes per creature; first lane of the creature's group inside the wavefront; lane inside the group
    bool inWorld, live; // a creature of the world (not padding); ... and a body (shape != 0)
    int body, nBodies; // rank of this lane among the creature's live lanes; their number
};
// false for the wavefronts past the last block of the launch (wave-uniform: the whole wavefront leaves)
__device__ __forceinline__ bool ctl_locate(const CtlTable &Tb, CtlLane &c) {
    const unsigned wv = blockIdx.x * (CTL_THREADS / WAVE) + (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    int wi = 0;
    unsigned firstBlock = 0;
    while (wi < Tb.n && wv >= Tb.w[wi].blockEnd) firstBlock = Tb.w[wi++].blockEnd;
    if (wi >= Tb.n) return false;
    c.S = Tb.w[wi];
    c.world = wi;
    const CtlWorld &S = c.S;
    c.K = (int)S.lanes;
    const int lane = (int)(threadIdx.x & (WAVE - 1));
    c.base = lane & ~(c.K - 1);
    c.sub = lane & (c.K - 1);
    const unsigned gl = (wv - firstBlock) * WAVE + (unsigned)lane; // < Lp: blockEnd - firstBlock = Lp / 64
    c.gl = gl;
    c.env = gl / (unsigned)c.K;
    c.inWorld = c.env < S.nEnvs;
    c.live = c.inWorld && LI(L_SHAPE) != SHAPE_NONE;
    const unsigned long long grp = (__ballot(c.live) >> c.base) & (c.K == WAVE ? ~0ull : ((1ull << c.K) - 1ull));
    c.body = __popcll(grp & ((1ull << c.sub) - 1ull));
    c.nBodies = __popcll(grp);
    return true;
}
// (the accessors of rem2d_state.h want S, gl and env in scope)
#define CTL_SCOPE(c) const CtlWorld &S = (c).S; const unsigned gl = (c).gl, env = (c).env; (void)env

__device__ __forceinline__ void obs_body(float *p, float a, float b, float c, float d, float e, float f) {
    p[0] = a; p[1] = b; p[2] = c; p[3] = d; p[4] = e; p[5] = f;
}

__global__ __launch_bounds__(CTL_THREADS) void rem2d_observe_kernel(CtlTable Tb, int maxBodies, float *out, long long outRows) {
    CtlLane c;
    if (!ctl_locate(Tb, c)) return;
    CTL_SCOPE(c);
    const int K = c.K, base = c.base, sub = c.sub, body = c.body, nBodies = c.nBodies;
    const bool inWorld = c.inWorld, live = c.live;
    // (every lane of the block loads: the arena is padded to whole blocks, and the shuffles want all lanes)
    const float px = LF(L_PX), py = LF(L_PY), ang = LF(L_ANG), vx = LF(L_VX), vy = LF(L_VY), w = LF(L_W);
    const int parent = LI(L_PARENT);
    const int pl = base + (parent >= 0 ? parent : 0);
    const float angParent = __shfl(ang, pl), wParent = __shfl(w, pl);
    const float pxRoot = __shfl(px, base), pyRoot = __shfl(py, base);
    if (!inWorld) return;
    const long long r = S.index ? (long long)S.index[env] : (long long)env;
    if (r < 0 || r >= outRows) return;
    float *row = out + (size_t)r * (size_t)(REM2D_OBS_HEAD + maxBodies * REM2D_OBS_BODY);
    if (live) {
        if (body < maxBodies) {
            int touching = 0;
            const int cCount = min(LI(L_CCOUNT), KC);
            for (int s = 0; s < cCount; ++s) touching += (CI(C_INFO, (unsigned)s * S.Lp + gl) & 0xff) > 0 ? 1 : 0;
            float *p = row + REM2D_OBS_HEAD + body * REM2D_OBS_BODY;
            if (body == 0) obs_body(p, 0.0f, 0.0f, 0.0f, (float)touching, 0.0f, 0.0f);
            else
                obs_body(p, __fsub_rn(__fsub_rn(ang, angParent), 0.0f), __fsub_rn(w, wParent), (float)LI(L_JLIMIT), (float)touching,
                         __fsub_rn(px, pxRoot), __fsub_rn(py, pyRoot));
        }
    } else { // the d-th empty lane of the creature clears body slot nBodies + d
        const int slot = nBodies + (sub - body);
        if (slot < maxBodies) obs_body(row + REM2D_OBS_HEAD + slot * REM2D_OBS_BODY, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
    }
    if (sub == 0) {
        row[0] = px; row[1] = py; row[2] = ang; row[3] = vx; row[4] = vy; row[5] = w;
        row[6] = (float)((double)px - ED(E_WOD));
        row[7] = (float)nBodies;
        for (int slot = K; slot < maxBodies; ++slot) // body slots no lane of this bucket stands for
            obs_body(row + REM2D_OBS_HEAD + slot * REM2D_OBS_BODY, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// values [nRows][maxBodies] (REM2D_CTRL_TARGET) or [nRows][maxBodies][4] (REM2D_CTRL_PARAMS); mask [nRows][maxBodies] or nullptr
__global__ __launch_bounds__(CTL_THREADS) void rem2d_control_kernel(CtlTable Tb, int mode, const double *values, int maxBodies,
                                                                     long long nRows, const unsigned char *mask) {
    CtlLane c;
    if (!ctl_locate(Tb, c)) return;
    CTL_SCOPE(c);
    const int body = c.body;
    if (!c.live || LI(L_PARENT) < 0 || body < 1 || body >= maxBodies) return; // a jointed live body that has a column
    const long long r = S.index ? (long long)S.index[env] : (long long)env;
    if (r < 0 || r >= nRows) return;
    const size_t at = (size_t)r * (size_t)maxBodies + (size_t)body;
    if (mask && mask[at] == 0) return;
    if (mode == REM2D_CTRL_TARGET) {
        LD(D_CAMP) = 0.0; // target = (0 * sin(..)) + offset = offset, exactly
        LD(D_COFFSET) = values[at];
    } else {
        const double *v = values + 4 * at;
        LD(D_CAMP) = v[0]; LD(D_CPHASE) = v[1]; LD(D_CFREQ) = v[2]; LD(D_COFFSET) = v[3];
    }
}

#endif
