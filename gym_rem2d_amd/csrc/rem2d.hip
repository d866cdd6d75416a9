// rem2d.hip -- MI355X (gfx950) batched 2D rigid-body stepper + its C ABI (include/rem2d.h).
//
// Replaces the world.Step() hot loop of gym_rem2D's Modular2D.step()/reset()
// (gym_rem2D/envs/Modular2DEnv.py:565-653; engine semantics: Box2D 2.3.x, SURVEY.md
// Appendix A) for N independent creatures at once.
//
// Execution model (wave64, no MFMA -- this is VALU/latency bound, not a contraction):
//   * one lane = one rigid body, its revolute joint to the parent body and its contact
//     list; K = 2..32 consecutive lanes = one creature = one Box2D island; a 64-lane
//     wavefront (= one workgroup) steps 64/K creatures in lockstep;
//   * a body's pose/velocity, its joint's effective-mass terms and accumulated impulses and
//     up to REM2D_SOLVER_SLOTS contact constraints live in VGPRs for a whole launch
//     (n_steps steps), so HBM is touched once per launch for them;
//   * contacts only couple a body to static terrain, so all bodies solve their contacts in
//     parallel; joints couple two lanes and are solved in precomputed rounds that keep
//     Box2D's island order among joints sharing a body, exchanging body velocities /
//     positions through a 1.5 KB LDS mailbox -- the result is bit-identical to the sequential
//     Gauss-Seidel sweep of the CPU restatement;
//   * the per-body broadphase pair list (edge index, feature keys, warm-start impulses) is
//     SoA in HBM ([slot][lane], coalesced) and walked with rolled loops.
//
// Build: hipcc with the flags of gym_rem2d_amd/_lib.py BUILD_FLAGS (-Os --offload-arch=gfx950 -ffp-contract=off
// -fno-slp-vectorize ...: every binary32 operation rounded separately, like an x86-64 Box2D build; this is what makes bit-exact
// parity possible).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "rem2d.h"
#include "rem2d_gather.h"
#include "rem2d_render.h"
#include <rem2d_control.h> // the public header (include/); the quoted name below is the kernels' file beside this one
#include <rem2d_sense.h>   // (likewise)
#include <rem2d_policy.h>  // (likewise)
#include <rem2d_episode.h> // (likewise)
#include <rem2d_stream.h>  // (likewise)
#include <rem2d_evolve.h>  // (likewise)
#include <rem2d_order.h>   // (the public header; it has no kernels of its own)
#include <rem2d_es.h>      // (as rem2d_evolve.h: the quoted name below is the kernels' file)
#include <rem2d_novelty.h> // (likewise)
#include <rem2d_elites.h>  // (likewise)
#include <rem2d_cvt.h>     // (likewise)
#include <rem2d_snes.h>    // (likewise)
#include <rem2d_pareto.h>  // (likewise)
#include <rem2d_recurrent.h> // (likewise)
#include <rem2d_obsnorm.h> // (likewise)
#include <rem2d_modular.h> // (likewise)

#define KC REM2D_CONTACT_SLOTS
#define KT REM2D_SOLVER_SLOTS   // touching contacts per body that can enter the solver
#define KR 3                    // ... of which this many are register resident in the velocity loop
#define WAVE 64
#define SCR_WORDS 9 // manifold scratch words per solver slot
// pair-slot map of a body's touching contacts: 5 bits per solver slot (REM2D_CONTACT_SLOTS <= 32), one or two words
static_assert(KC <= 32, "pair-slot indices are packed in 5 bits");
#if REM2D_SOLVER_SLOTS * 5 <= 32
typedef unsigned slotpack_t;
#define SP_WORDS 1
#else
typedef unsigned long long slotpack_t;
#define SP_WORDS 2
static_assert(KT * 5 <= 64, "pair-slot map: at most 12 solver slots");
#endif
#define SP_PUT(s, t) ((slotpack_t)(unsigned)(s) << (5 * (t)))
#define SP_GET(p, t) ((unsigned)((p) >> (5 * (t))) & 0x1fu)

// ---- b2Settings.h constants (same expressions as Box2D so that they fold identically) ----
#define B2_PI 3.14159265359f
#define B2_EPSILON FLT_EPSILON
#define B2_LINEAR_SLOP 0.005f
#define B2_ANGULAR_SLOP (2.0f / 180.0f * B2_PI)
#define B2_POLYGON_RADIUS (2.0f * B2_LINEAR_SLOP)
#define B2_AABB_EXTENSION 0.1f
#define B2_AABB_MULTIPLIER 2.0f
#define B2_MAX_LINEAR_CORRECTION 0.2f
#define B2_MAX_ANGULAR_CORRECTION (8.0f / 180.0f * B2_PI)
#define B2_MAX_TRANSLATION 2.0f
#define B2_MAX_TRANSLATION_SQ (B2_MAX_TRANSLATION * B2_MAX_TRANSLATION)
#define B2_MAX_ROTATION (0.5f * B2_PI)
#define B2_MAX_ROTATION_SQ (B2_MAX_ROTATION * B2_MAX_ROTATION)
#define B2_BAUMGARTE 0.2f
#define B2_TIME_TO_SLEEP 0.5f
#define B2_LINEAR_SLEEP_TOL 0.01f
#define B2_ANGULAR_SLEEP_TOL (2.0f / 180.0f * B2_PI)

enum { SHAPE_NONE = 0, SHAPE_BOX = 1, SHAPE_CIRCLE = 2 };
enum { MF_CIRCLES = 0, MF_FACE_A = 1, MF_FACE_B = 2 };
enum { LIM_INACTIVE = 0, LIM_AT_LOWER = 1, LIM_AT_UPPER = 2, LIM_EQUAL = 3 };
enum { CF_VERTEX = 0, CF_FACE = 1 };

#include "rem2d_state.h"
#include "rem2d_math.h"
#include "rem2d_narrowphase.h"
#include "rem2d_solver.h"
#include "rem2d_toi.h"
#include "rem2d_position.h"
#include "rem2d_kernels.h"
#include "rem2d_pipeline.h"
#include "rem2d_vel4.h"
#include "rem2d_diversity.h"
#include "rem2d_raster.h"
#include "rem2d_control.h"
#include "rem2d_sense.h"
#include "rem2d_obsnorm.h" // (before the two forward kernels, whose NORM instantiations stage their rows through it)
#include "rem2d_policy.h"
#include "rem2d_recurrent.h"
#include "rem2d_modular.h"
#include "rem2d_episode.h"
#include "rem2d_stream.h"
#include "rem2d_evolve.h"
#include "rem2d_es.h"
#include "rem2d_novelty.h"
#include "rem2d_elites.h"
#include "rem2d_cvt.h"
#include "rem2d_snes.h"
#include "rem2d_pareto.h"

// =====================================================================================
// host side: handle + C ABI
// =====================================================================================
static thread_local std::string g_err;
static int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(REM2D_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define OK_TRY(expr) \
    do { const int rc_ = (expr); if (rc_ != REM2D_OK) return rc_; } while (0)

// Pairs of timing events: made by rem2d_world_enable_timing (outside any timed region), recorded by the step calls, read back by
// rem2d_world_kernel_time_ms / rem2d_world_step_time_ms.  Launches beyond the pool go untimed.
typedef std::pair<hipEvent_t, hipEvent_t> EventPair;
struct EventPool {
    std::vector<EventPair> pairs;
    std::vector<int> weight; // what pair i adds to `count` once read (a step train's step bracket holds a whole launch of env-steps)
    int used = 0;
    double ms = 0.0; // read back and not yet reported
    int64_t count = 0;
    int fill(size_t want) {
        while (pairs.size() < want) {
            hipEvent_t a = nullptr, b = nullptr;
            HIP_TRY(hipEventCreate(&a));
            hipError_t e = hipEventCreate(&b);
            if (e != hipSuccess) {
                (void)hipEventDestroy(a);
                return fail(REM2D_E_HIP, std::string("hipEventCreate: ") + hipGetErrorString(e));
            }
            pairs.emplace_back(a, b);
        }
        weight.resize(pairs.size(), 1);
        return REM2D_OK;
    }
    // the next free pair (counted as used, weight 1) for a launch that records it itself, or nullptr
    const EventPair *take(bool on) {
        if (!on || used >= (int)pairs.size()) return nullptr;
        weight[(size_t)used] = 1;
        return &pairs[(size_t)used++];
    }
    // a bracket of stream events around what is queued between open and close; false: nothing opened, do not close
    bool open(bool on, hipStream_t st) { return on && used < (int)pairs.size() && hipEventRecord(pairs[(size_t)used].first, st) == hipSuccess; }
    void close(hipStream_t st, int w) {
        (void)hipEventRecord(pairs[(size_t)used].second, st);
        weight[(size_t)used] = w;
        used += 1;
    }
    void drain() { // (the device has been drained: every recorded pair is complete)
        for (int i = 0; i < used; ++i) {
            float t = 0.0f;
            if (hipEventElapsedTime(&t, pairs[(size_t)i].first, pairs[(size_t)i].second) == hipSuccess) {
                ms += t;
                count += weight[(size_t)i];
            }
        }
        used = 0;
    }
    void report(double *total_ms, int64_t *n) {
        if (total_ms) *total_ms = ms;
        if (n) *n = count;
        ms = 0.0;
        count = 0;
    }
    void free() {
        for (auto &p : pairs) {
            (void)hipEventDestroy(p.first);
            (void)hipEventDestroy(p.second);
        }
        pairs.clear();
        used = 0;
    }
};

struct rem2d_world {
    rem2d_world_cfg cfg;
    Layout L;
    char *state;
    State S;
    Terrain T;
    float *terrainBuf;
    int *tilesDev; // [nTiles + 1] creature index where each tile of rem2d_vel4_kernel starts
    int nTiles;
    int tileShape; // REM2D_TILE_SHAPE id of rem2d_vel4_kernel for this world's tiles
    bool haveTerrain, haveReset;
    bool timing;
    EventPool evKernel; // around the dominant kernel of each launch; count = launches
    EventPool evStep;   // around all kernels of an env-step (re-ordering .. toi_heavy) of the tile pipeline, or of a train launch; count = env-steps
    hipEvent_t evFork, evJoin; // fork / join edges of rem2d_groups_step (created on first use)
    uint64_t epoch;            // bumped whenever something the kernel arguments embed changes (graph replay key)
    int32_t opt[REM2D_OPT_COUNT]; // launch options (rem2d_world_set_option); results never depend on them
    int64_t stepsQueued;          // env-steps queued so far (the cadence of REM2D_OPT_REBALANCE)
    int64_t stepsAtOrder;         // ... at the step train's last re-ordering launch
    unsigned *trainFlags; size_t trainCap; // the step train's hand-over flags (device; grown on demand, as the first world of a launch)
    unsigned *trainFailures;      // pinned host word: hand-overs of this world's trains that failed (rem2d_world_handover_failures)
    bool hostOrder;               // rem2d_world_set_order installed an order (REM2D_STATE_ORDERED = hostOrder || REBALANCE > 0)
};
// the kernels go through State::order while the host has installed an order OR the library re-makes one every N steps
static void order_flag_update(rem2d_world *w) {
    if (w->hostOrder || w->opt[REM2D_OPT_REBALANCE] > 0) w->S.flags |= REM2D_STATE_ORDERED;
    else w->S.flags &= ~REM2D_STATE_ORDERED;
}

// Tile shape of rem2d_vel4_kernel (rem2d_world_set_tile_shape; rem2d_vel4.h explains the trade-off):
//   0: 256 bodies, 4 joint sets, 2 contact sets, 2 waves/SIMD   1: 128 bodies, 2 + 1 sets, 4 waves/SIMD (round 4)
//   2: 192 bodies, 3 + 1 sets, 3 waves/SIMD (round 4)
//   3: 64 bodies, 1 + 1 sets, 4 waves/SIMD (default: measured fastest on config 3; the same at 5 waves/SIMD spills: 24.7 M)
//   4: 128 bodies, 2 + 1 sets, 3 waves/SIMD with the static phase -> set map of rounds 2-3: what fixed-morphology populations
//      want (every creature the same schedule: nothing to rotate, and the 8-module chains are 5 % faster with it, 186 vs 176 M)
// Shapes 1-3 place joints flexibly (rem2d_vel4.h FLEX): any tile within 64 joints per set IN ALL fits.
#ifndef REM2D_SHAPE1_WPS
#define REM2D_SHAPE1_WPS 4 // wavefronts per SIMD the 128-body tile shape is compiled for
#endif
#ifndef REM2D_SHAPE4_WPS
#define REM2D_SHAPE4_WPS 3 // the same for the static 128-body shape of the fixed-morphology populations (4: 128 VGPRs, 3 spilled; 65 536 8-module chains 164 instead of 185 M)
#endif
#ifndef REM2D_SHAPE1_PAIR
#define REM2D_SHAPE1_PAIR false // (lane-pair contact solves: a 128-body tile's manifolds rarely fit 32 lanes; without them 3 VGPR spills instead of 7, +2.7 % at 393 216 creatures)
#endif
typedef void (*PreKernel)(Batch, StepArgs);
typedef void (*Vel4Kernel)(Vel4Batch, Vel4Args);
typedef void (*TrainKernel)(Batch, StepArgs, Vel4Args, unsigned *, unsigned, int, unsigned *);
// The instantiations, named once -- in the order the launch code has always first named them, which is their order inside the code
// object (pre 4 3, velocity tiles 0 1 2 4 3, trains 4 1): the table below may list them by shape id without moving a kernel.
static constexpr PreKernel kPre4 = rem2d_pre_multi_kernel<4>, kPre3 = rem2d_pre_multi_kernel<3>;
static constexpr Vel4Kernel kVel0 = rem2d_vel4_kernel<4, 4, 2, 2, false>, kVel1 = rem2d_vel4_kernel<2, 2, 1, REM2D_SHAPE1_WPS, REM2D_SHAPE1_PAIR>,
                            kVel2 = rem2d_vel4_kernel<3, 3, 1, 3, true>, kVel4 = rem2d_vel4_kernel<2, 2, 1, REM2D_SHAPE4_WPS, false, false>,
                            kVel3 = rem2d_vel4_kernel<1, 1, 1, 4, true>;
static constexpr TrainKernel kTrain4 = rem2d_step_train128_kernel<false, REM2D_SHAPE4_WPS>, kTrain1 = rem2d_step_train128_kernel<true, REM2D_SHAPE1_WPS>;
// One row per shape: all that planning and launching know about it.  A new shape is a row here (and its instantiations above).
struct TileShape {
    int sets, passes, csets, flex;
    // which kernel runs a merged launch of worlds planned for different shapes: the highest rank, whose kernel takes every world's
    // tiles (a tile planned under the static phase -> set map fits a flexible kernel of the same size, not the other way round)
    int rank;
    Vel4Kernel vel4;   // the velocity tiles
    PreKernel pre;     // pre beside them, compiled for the same wavefronts per SIMD (4, or 3: rem2d_pipeline.h)
    TrainKernel train; // all steps of a call in one launch for tiles of this shape (REM2D_OPT_FUSE_VELPOST = 2), or nullptr
};
#define REM2D_TILE_SHAPES 5
#define DEFAULT_TILE_SHAPE 3
static const TileShape kTileShapes[REM2D_TILE_SHAPES] = {
    {4, 4, 2, 0, 4, kVel0, kPre3, nullptr},
    {2, 2, 1, 1, 2, kVel1, REM2D_SHAPE1_WPS >= 4 ? kPre4 : kPre3, kTrain1},
    {3, 3, 1, 1, 3, kVel2, kPre3, nullptr},
    {1, 1, 1, 1, 0, kVel3, kPre4, rem2d_step_train_kernel},
    {2, 2, 1, 0, 1, kVel4, kPre3, kTrain4},
};
static bool tile_shape_ok(int id) { return id >= 0 && id < REM2D_TILE_SHAPES; }
static const TileShape &tile_shape(int id) { return kTileShapes[tile_shape_ok(id) ? id : DEFAULT_TILE_SHAPE]; }
// the default plan as a tile table: valid for every morphology of the world's lanes per creature
static std::vector<int32_t> default_tiles(const rem2d_world *w) {
    const TileShape &shp = tile_shape(w->tileShape);
    const int lanes = w->cfg.lanes;
    // flexible shapes: a creature has fewer joints than lanes, so passes * 64 lanes never exceed sets * 64 joints (passes <= sets);
    // four sets = one phase per set: 128 / lanes creatures never have more than 64 joints in a phase
    int per = (shp.flex ? shp.passes * WAVE : (shp.sets >= 4 ? 128 : 64)) / lanes;
    if (per * lanes > shp.passes * WAVE) per = shp.passes * WAVE / lanes;
    if (per < 1) per = 1;
    std::vector<int32_t> ts;
    for (int c = 0; c < w->L.Np; c += per) ts.push_back(c);
    ts.push_back(w->L.Np);
    return ts;
}
// Launch options of a world (include/rem2d.h REM2D_OPT_*): defaults and valid ranges.  None of them changes a result; the
// library reads no environment variable -- hosts that want overrides for experiments pass them here (gym_rem2d_amd._lib
// maps REM2D_* variables onto these calls for bench.py and the tools).
//   PIPELINE       3 = tile pipeline pre -> velocity tiles -> post (default), 0 = the fused body-per-lane step kernel of round 1,
//                  kept as an independently written second formulation that the parity suite runs against the same oracle
//   FUSE_VELPOST   velocity tiles and position iterations of a 64-lane block in one launch (rem2d_velpost_kernel) where the
//                  tile tables allow it.  The slowest velocity tile is usually the slowest position block as well, so
//                  max(v + p) is only a little less than max v + max p: +1.0 % on config 3 in 100-step blocks, +1.7 % on the
//                  driver's command (one launch per step and group less to wait for at the join of every call)
//   PRIO           issue priority (s_setprio) for the wavefronts expected to be the long ones of their launch -- bit 1: the
//                  velocity tiles with the most slots per iteration (cost 7 ticks + 10 sub-slots >= PRIO_T1: priority 1,
//                  >= PRIO_T2: priority 3), bit 4: the wavefronts of the TOI solve.  profiles/archive/r03_prio.txt: config 3 +4.6 %
//   HEAVY_PER_WAVE bodies of the TOI work list per wavefront of rem2d_toi_heavy_multi_kernel, 1..64 (one: a wavefront that
//                  holds two runs the union of their code paths)
//   DEBUG          diagnostic builds (-DREM2D_V4_PROBES) only: Vel4Args::dbg
//   REBALANCE      N > 0: every N env-steps the world's creature order is re-made on the device (rem2d_rebalance_kernel: the
//                  creatures that used every position iteration first, a stable partition), 0 = off
//   TRAIN_FAULT    test hook of the step train's hand-over check: s | m << 16 [| 1 << 30] -- the items (step s of a launch, s >= 1,
//                  blocks with block % m == 0; m <= 1: every block) are told that their hand-over failed, or (bit 30) never get
//                  their flag and wait into the limit.  What the kernels COMPUTE does not change; the creatures carry
//                  REM2D_ERR_HANDOVER and the world's failure counter moves (tests/test_handover_gpu.py)
static const int32_t kOptDefault[REM2D_OPT_COUNT] = {3, 2, 5, 60, 75, 1, 0, 0, 0};
static const int32_t kOptMin[REM2D_OPT_COUNT] = {0, 0, 0, 0, 0, 1, 0, 0, 0};
static const int32_t kOptMax[REM2D_OPT_COUNT] = {3, 2, 7, 1 << 20, 1 << 20, WAVE, 1 << 30, 1 << 20, 0x7fffffff};

static uint32_t __float_as_uint_host(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

extern "C" int rem2d_abi_version(void) { return REM2D_ABI_VERSION; }
// Build identity: the builder (gym_rem2d_amd/_lib.py build(), tools/build_variant.sh) hashes every file under csrc/, include/rem2d.h
// and the compile flags into -DREM2D_BUILD_ID; the loader recomputes the hash from the sources beside it and refuses a library
// built from anything else (the .so files are git-ignored yet travel to the GPU box: a stale one must not be benched silently).
// The marker in front lets a tool read the id from the file without dlopen.
#ifndef REM2D_BUILD_ID
#define REM2D_BUILD_ID "unidentified"
#endif
static const char kBuildId[] = "REM2D_BUILD_ID=" REM2D_BUILD_ID;
extern "C" const char *rem2d_build_id(void) { return kBuildId + 15; }
extern "C" const char *rem2d_last_error(void) { return g_err.c_str(); }
extern "C" int rem2d_capacity(int32_t *contact_slots, int32_t *solver_slots) {
    if (contact_slots) *contact_slots = REM2D_CONTACT_SLOTS;
    if (solver_slots) *solver_slots = REM2D_SOLVER_SLOTS;
    return REM2D_OK;
}

static bool cfg_ok(const rem2d_world_cfg *cfg) {
    if (!cfg || cfg->n_envs <= 0) return false;
    int k = cfg->lanes;
    return k == 2 || k == 4 || k == 8 || k == 16 || k == 32 || k == 64;
}
extern "C" size_t rem2d_state_bytes(const rem2d_world_cfg *cfg) {
    if (!cfg_ok(cfg)) return 0;
    return make_layout(cfg).total;
}
extern "C" int32_t rem2d_padded_envs(const rem2d_world_cfg *cfg) {
    if (!cfg_ok(cfg)) return 0;
    return make_layout(cfg).Np;
}

static uint64_t next_epoch() { // (worlds of different host threads draw from it)
    static std::atomic<uint64_t> e{0};
    return ++e;
}
static void bind_state(rem2d_world *w) {
    State &S = w->S;
    const Layout &L = w->L;
    S.lane4 = w->state + L.groupOff[G_LANE4];
    S.lane8 = w->state + L.groupOff[G_LANE8];
    S.slot4 = w->state + L.groupOff[G_SLOT4];
    S.env4 = w->state + L.groupOff[G_ENV4];
    S.env8 = w->state + L.groupOff[G_ENV8];
    S.Lp = (unsigned)L.Lp;
    S.Np = (unsigned)L.Np;
    S.nEnvs = (unsigned)w->cfg.n_envs;
    S.flags = w->cfg.flags;
    S.outReward = nullptr;
    S.outDone = nullptr;
    S.outIndex = nullptr;
}

extern "C" int rem2d_world_create(const rem2d_world_cfg *cfg, void *state_dev, size_t state_bytes, rem2d_world **out) {
    if (!out) return fail(REM2D_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!cfg_ok(cfg)) return fail(REM2D_E_INVALID, "cfg: n_envs must be > 0 and lanes one of 2,4,8,16,32,64");
    Layout L = make_layout(cfg);
    if (!state_dev || state_bytes < L.total) return fail(REM2D_E_INVALID, "state buffer missing or too small");
    // 32-bit per-lane byte offsets: (slots * Lp + lane) * 4 and (scratch words * Lp + lane) * 4 must fit
    if ((size_t)L.Lp * (SCR_TOTAL_WORDS + 1) * 4 >= ((size_t)1 << 32))
        return fail(REM2D_E_INVALID, "too many lanes for one world (n_envs * lanes must stay below ~5 million)");
    if (((uintptr_t)state_dev & 255) != 0) return fail(REM2D_E_INVALID, "state buffer must be 256-byte aligned");
    HIP_TRY(hipSetDevice(cfg->device));
    rem2d_world *w = new (std::nothrow) rem2d_world();
    if (!w) return fail(REM2D_E_NOMEM, "host allocation failed");
    w->cfg = *cfg;
    w->L = L;
    w->state = (char *)state_dev;
    w->terrainBuf = nullptr;
    w->haveTerrain = w->haveReset = false;
    w->timing = false;
    w->evFork = w->evJoin = nullptr;
    w->epoch = next_epoch();
    for (int k = 0; k < REM2D_OPT_COUNT; ++k) w->opt[k] = kOptDefault[k];
    w->stepsQueued = 0;
    w->stepsAtOrder = 0;
    w->hostOrder = false;
    w->trainFlags = nullptr;
    w->trainCap = 0;
    w->trainFailures = nullptr;
    bind_state(w);
    w->S.scr = nullptr;
    hipError_t e = hipMalloc((void **)&w->S.scr, ((size_t)SCR_TOTAL_WORDS * L.Lp + L.Lp + 64) * sizeof(float));
    if (e != hipSuccess) {
        delete w;
        return fail(REM2D_E_HIP, std::string("hipMalloc(scratch): ") + hipGetErrorString(e));
    }
    w->S.toiWork = (int *)(w->S.scr + (size_t)SCR_TOTAL_WORDS * L.Lp);
    e = hipMemset(w->S.toiWork, 0, 64 * sizeof(int));
    if (e != hipSuccess) {
        (void)hipFree(w->S.scr);
        delete w;
        return fail(REM2D_E_HIP, std::string("hipMemset(scratch): ") + hipGetErrorString(e));
    }
    // creature order of the post kernel (rem2d_pipeline.h, "Dynamic re-tiling"): both halves start as the identity
    {
        std::vector<int> ord((size_t)2 * L.Np + 4, 0);
        for (int i = 0; i < L.Np; ++i) ord[i] = ord[(size_t)L.Np + i] = i;
        w->S.order = nullptr;
        e = hipMalloc((void **)&w->S.order, ord.size() * sizeof(int));
        if (e == hipSuccess) e = hipMemcpy(w->S.order, ord.data(), ord.size() * sizeof(int), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (w->S.order) (void)hipFree(w->S.order);
            (void)hipFree(w->S.scr);
            delete w;
            return fail(REM2D_E_HIP, std::string("hipMalloc(order): ") + hipGetErrorString(e));
        }
    }
    // default tiles of the velocity kernel.  The joints of one schedule phase of a creature are a matching of its tree
    // (<= lanes / 2 of them), so 128 / lanes creatures never have more than 64 joints in a phase;
    // rem2d_world_set_tiles lets the host pack tiles tighter from the actual morphologies.
    {
        w->tileShape = DEFAULT_TILE_SHAPE;
        const std::vector<int32_t> ts = default_tiles(w);
        w->tilesDev = nullptr;
        w->nTiles = 0;
        int rc = rem2d_world_set_tiles(w, ts.data(), (int32_t)ts.size() - 1);
        if (rc != REM2D_OK) {
            (void)hipFree(w->S.scr);
            (void)hipFree(w->S.order);
            delete w;
            return rc;
        }
    }
    *out = w;
    return REM2D_OK;
}

extern "C" int rem2d_world_adopt(rem2d_world *w) {
    if (!w) return fail(REM2D_E_INVALID, "world is NULL");
    if (!w->haveTerrain) return fail(REM2D_E_STATE, "rem2d_world_set_terrain must be called before adopt");
    w->haveReset = true; // the arena is the whole state between two steps: the scratch is rewritten by every step
    return REM2D_OK;
}

extern "C" int rem2d_world_set_outputs(rem2d_world *w, float *reward_dev, uint8_t *done_dev, const int32_t *index_dev) {
    if (!w) return fail(REM2D_E_INVALID, "world is NULL");
    if ((reward_dev == nullptr) != (done_dev == nullptr) || (reward_dev == nullptr) != (index_dev == nullptr))
        return fail(REM2D_E_INVALID, "set_outputs: pass all three pointers, or three NULLs to switch it off");
    w->S.outReward = reward_dev;
    w->S.outDone = done_dev;
    w->S.outIndex = index_dev;
    w->epoch = next_epoch();
    return REM2D_OK;
}

extern "C" int rem2d_world_set_tile_shape(rem2d_world *w, int32_t tile_shape_sel) {
    if (!w) return fail(REM2D_E_INVALID, "world is NULL");
    if (!tile_shape_ok(tile_shape_sel)) return fail(REM2D_E_INVALID, "tile shape must be 0 .. 4");
    if (w->tileShape == tile_shape_sel) return REM2D_OK;
    w->tileShape = tile_shape_sel;
    // the tile table in place may not fit the new shape: back to the default plan, valid for every morphology
    const std::vector<int32_t> ts = default_tiles(w);
    return rem2d_world_set_tiles(w, ts.data(), (int32_t)ts.size() - 1);
}

extern "C" int rem2d_world_set_order(rem2d_world *w, const int32_t *order_dev, void *stream) {
    if (!w) return fail(REM2D_E_INVALID, "world is NULL");
    if (w->cfg.flags & REM2D_FLAG_RETILE) return fail(REM2D_E_INVALID, "set_order: the world deals its creatures itself (REM2D_FLAG_RETILE)");
    HIP_TRY(hipSetDevice(w->cfg.device));
    if (order_dev) {
        // both halves (the REM2D_FLAG_RETILE machinery reads the first, swaps in the second): what the kernels read stays put
        HIP_TRY(hipMemcpyAsync(w->S.order, order_dev, (size_t)w->L.Np * sizeof(int), hipMemcpyDeviceToDevice, (hipStream_t)stream));
        HIP_TRY(hipMemcpyAsync(w->S.order + w->L.Np, order_dev, (size_t)w->L.Np * sizeof(int), hipMemcpyDeviceToDevice, (hipStream_t)stream));
        w->hostOrder = true;
    } else {
        // back to the arena order.  With REM2D_OPT_REBALANCE on the kernels keep going through State::order (the library
        // re-makes it every N steps), so the identity is written there instead of dropping the indirection -- and with it off as
        // well: rem2d_world_read_order shows the array, and switching REM2D_OPT_REBALANCE on later starts from what it holds
        if (w->hostOrder) {
            std::vector<int> ident((size_t)w->L.Np);
            for (int i = 0; i < w->L.Np; ++i) ident[(size_t)i] = i;
            HIP_TRY(hipDeviceSynchronize()); // (rare call: no kernel of any step group may still read the old order)
            HIP_TRY(hipMemcpy(w->S.order, ident.data(), ident.size() * sizeof(int), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(w->S.order + w->L.Np, ident.data(), ident.size() * sizeof(int), hipMemcpyHostToDevice));
        }
        w->hostOrder = false;
    }
    order_flag_update(w);
    w->epoch = next_epoch();
    return REM2D_OK;
}

extern "C" int rem2d_world_set_option(rem2d_world *w, int32_t key, int32_t value) {
    if (!w) return fail(REM2D_E_INVALID, "world is NULL");
    if (key < 0 || key >= REM2D_OPT_COUNT) return fail(REM2D_E_INVALID, "set_option: unknown option");
    if (value < kOptMin[key] || value > kOptMax[key] || (key == REM2D_OPT_PIPELINE && value != 0 && value != 3))
        return fail(REM2D_E_INVALID, "set_option: value out of range for this option");
    if (key == REM2D_OPT_REBALANCE) {
        if (value > 0 && (w->cfg.flags & REM2D_FLAG_RETILE))
            return fail(REM2D_E_INVALID, "set_option: the world deals its creatures itself (REM2D_FLAG_RETILE)");
    }
    if (w->opt[key] != value) {
        w->opt[key] = value;
        w->epoch = next_epoch(); // (a captured replay of the old launch sequence is stale)
    }
    // REBALANCE: the kernels go through State::order from now on (the identity, or the host's order, until the first
    // rebalance) / directly again unless the host has an order installed (rem2d_world_set_order)
    if (key == REM2D_OPT_REBALANCE) order_flag_update(w);
    return REM2D_OK;
}
extern "C" int rem2d_world_get_option(const rem2d_world *w, int32_t key, int32_t *value) {
    if (!w || !value) return fail(REM2D_E_INVALID, "get_option: NULL argument");
    if (key < 0 || key >= REM2D_OPT_COUNT) return fail(REM2D_E_INVALID, "get_option: unknown option");
    *value = w->opt[key];
    return REM2D_OK;
}

extern "C" int rem2d_world_set_tiles(rem2d_world *w, const int32_t *tile_start, int32_t n_tiles) {
    if (!w || !tile_start || n_tiles <= 0) return fail(REM2D_E_INVALID, "tiles: NULL table or no tiles");
    if (tile_start[0] != 0 || tile_start[n_tiles] < w->cfg.n_envs || tile_start[n_tiles] > w->L.Np)
        return fail(REM2D_E_INVALID, "tiles must cover creatures [0, n_envs) (at most the padded count)");
    for (int t = 0; t < n_tiles; ++t) {
        const long long c = (long long)tile_start[t + 1] - tile_start[t];
        if (c <= 0) return fail(REM2D_E_INVALID, "tile starts must be strictly increasing");
        if (c * w->cfg.lanes > tile_shape(w->tileShape).passes * WAVE) return fail(REM2D_E_INVALID, "a tile holds too many lanes for the tile shape in use");
    }
    HIP_TRY(hipSetDevice(w->cfg.device));
    int *dev = nullptr;
    HIP_TRY(hipMalloc((void **)&dev, ((size_t)n_tiles + 1) * sizeof(int)));
    hipError_t e = hipMemcpy(dev, tile_start, ((size_t)n_tiles + 1) * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(dev);
        return fail(REM2D_E_HIP, std::string("hipMemcpy(tiles): ") + hipGetErrorString(e));
    }
    if (w->tilesDev) (void)hipFree(w->tilesDev); // hipFree waits for kernels that may still read the old table
    w->tilesDev = dev;
    w->nTiles = n_tiles;
    w->S.tiles = dev;
    // a regular table (tile t = creatures [t cap, (t + 1) cap), cap dividing the creatures of a 64-lane block -- or a multiple of
    // them: a tile of whole blocks): the velocity + position launch and the step trains can find the tiles of a block
    {
        const int cap = tile_start[1] - tile_start[0], cpb = WAVE / w->cfg.lanes;
        bool regular = w->cfg.lanes <= WAVE && cap > 0 && (cpb % cap == 0 || cap % cpb == 0) && tile_start[n_tiles] <= n_tiles * cap;
        for (int t = 0; t < n_tiles && regular; ++t) regular = tile_start[t] == t * cap;
        w->S.nTiles = n_tiles;
        w->S.tileCap = regular ? cap : 0;
    }
    w->epoch = next_epoch();
    return REM2D_OK;
}

extern "C" int rem2d_plan_tiles(const int32_t *parent, const int32_t *jround, int32_t n_envs, int32_t lanes, int32_t n_padded,
                                int32_t max_creatures, int32_t *tile_start_out, int32_t *n_tiles_out) {
    return rem2d_plan_tiles_shape(parent, jround, n_envs, lanes, n_padded, max_creatures, -1, tile_start_out, n_tiles_out);
}
extern "C" int rem2d_plan_tiles_shape(const int32_t *parent, const int32_t *jround, int32_t n_envs, int32_t lanes,
                                      int32_t n_padded, int32_t max_creatures, int32_t tile_shape_sel, int32_t *tile_start_out,
                                      int32_t *n_tiles_out) {
    if (!parent || !jround || !tile_start_out || !n_tiles_out) return fail(REM2D_E_INVALID, "plan_tiles: NULL argument");
    if (tile_shape_sel != -1 && !tile_shape_ok(tile_shape_sel))
        return fail(REM2D_E_INVALID, "plan_tiles: tile shape must be 0 .. 4 or -1 (the default, 3)");
    const TileShape &sh = tile_shape(tile_shape_sel < 0 ? DEFAULT_TILE_SHAPE : tile_shape_sel);
    const int maxLanes = sh.passes * WAVE;
    if (n_envs <= 0 || n_padded < n_envs || lanes <= 0 || lanes > maxLanes) return fail(REM2D_E_INVALID, "plan_tiles: bad shape");
    if (max_creatures <= 0) {
        // (fewer, fuller tiles are fewer wave-instructions: with the step train, which issues at 0.9 of the chip's peak, two-lane
        // creatures 32 to a 64-lane tile are +1.0 % on config 3 over 16 to a tile, 8 to a tile -28 %; under the per-step launches
        // of rounds 2-4, bound by their chain, 16 was the better cap: 46.8 vs 46.4 M then)
        max_creatures = 32;
    }
    const int capBodies = maxLanes / lanes; // creatures per tile by lanes
    const int cap = max_creatures < capBodies ? max_creatures : capBodies;
    int nt = 0;
    tile_start_out[0] = 0;
    int first = 0;          // first creature of the open tile
    int P = 1;              // its period
    int cnt[V4_PHASES];     // its joints per register set (phases ph = s mod sets share set s)
    for (int s = 0; s < V4_PHASES; ++s) cnt[s] = 0;
    auto creature_period = [&](int e) {
        int p = 1;
        if (e < n_envs)
            for (int k = 0; k < lanes; ++k) {
                const int q = (jround[(size_t)e * lanes + k] >> 16) & 0xff;
                p = q > p ? q : p;
            }
        return p;
    };
    auto add_counts = [&](int e, int period, int *c) { // joints of creature e per register set under `period`
        if (e >= n_envs) return;
        for (int k = 0; k < lanes; ++k) {
            const size_t i = (size_t)e * lanes + k;
            if (parent[i] < 0) continue;
            const int ph = (jround[i] & 0xff) % period;
            if (ph < V4_PHASES) c[ph % sh.sets] += 1; // periods beyond V4_PHASES are refused by the kernel (REM2D_ERR_SOLVER_OVERFLOW)
        }
    };
    for (int e = 0; e < n_padded; ++e) {
        const int pe = creature_period(e);
        bool fits = (e - first) < cap;
        int c2[V4_PHASES], P2 = P;
        for (int s = 0; s < V4_PHASES; ++s) c2[s] = 0;
        if (fits) {
            P2 = pe > P ? pe : P;
            if (P2 != P) {
                for (int x = first; x < e; ++x) add_counts(x, P2, c2);
            } else {
                for (int s = 0; s < V4_PHASES; ++s) c2[s] = cnt[s];
            }
            add_counts(e, P2, c2);
            if (sh.flex) { // flexible placement (rem2d_vel4.h FLEX): 64 joints per register set in all
                int all = 0;
                for (int s = 0; s < V4_PHASES; ++s) all += c2[s];
                fits = fits && all <= sh.sets * WAVE;
            } else {
                for (int s = 0; s < V4_PHASES; ++s) fits = fits && c2[s] <= WAVE;
            }
        }
        if (!fits && e > first) { // close the tile before e, start a new one with e
            tile_start_out[++nt] = e;
            first = e;
            P2 = pe;
            for (int s = 0; s < V4_PHASES; ++s) c2[s] = 0;
            add_counts(e, P2, c2);
        }
        P = P2;
        for (int s = 0; s < V4_PHASES; ++s) cnt[s] = c2[s];
    }
    tile_start_out[++nt] = n_padded;
    *n_tiles_out = nt;
    return REM2D_OK;
}

static void drain_timing(rem2d_world *w) {
    // the device is drained once; after that every recorded pair is complete.  (No hipEventSynchronize per event: the
    // start / stop events of hipExtLaunchKernelGGL are not stream records, and waiting on one can block for ever.)
    if (w->evKernel.used > 0 || w->evStep.used > 0) (void)hipDeviceSynchronize();
    w->evKernel.drain();
    w->evStep.drain();
    (void)hipGetLastError(); // an event pair that was never reached leaves hipErrorInvalidHandle / NotReady behind
}

static void graphs_forget(const rem2d_world *w); // (the hipGraph replays of rem2d_groups_step, below)
extern "C" int rem2d_world_destroy(rem2d_world *w) {
    if (!w) return REM2D_OK;
    (void)hipSetDevice(w->cfg.device);
    graphs_forget(w);
    w->evKernel.free();
    w->evStep.free();
    if (w->evFork) (void)hipEventDestroy(w->evFork);
    if (w->evJoin) (void)hipEventDestroy(w->evJoin);
    if (w->S.scr) (void)hipFree(w->S.scr);
    if (w->S.order) (void)hipFree(w->S.order);
    if (w->tilesDev) (void)hipFree(w->tilesDev);
    if (w->terrainBuf) (void)hipFree(w->terrainBuf);
    if (w->trainFlags) (void)hipFree(w->trainFlags);
    if (w->trainFailures) (void)hipHostFree(w->trainFailures);
    delete w;
    return REM2D_OK;
}

// b2PolygonShape::Set for one hardcore box (2.3.1): weld, gift-wrap hull from the right-most (lowest)
// point, counter-clockwise, edge normals.  Host arithmetic in binary32, no FMA (-ffp-contract=off).
static bool host_poly_set(const float *xy /*[4][2]*/, float vx[4], float vy[4], float nx[4], float ny[4]) {
    float px[4], py[4];
    int n = 0;
    for (int i = 0; i < 4; ++i) {
        float x = xy[2 * i], y = xy[2 * i + 1];
        bool unique = true;
        for (int j = 0; j < n; ++j) {
            float dx = x - px[j], dy = y - py[j];
            if (dx * dx + dy * dy < 0.5f * B2_LINEAR_SLOP) { unique = false; break; }
        }
        if (unique) { px[n] = x; py[n] = y; ++n; }
    }
    if (n != 4) return false;
    int i0 = 0;
    float x0 = px[0];
    for (int i = 1; i < n; ++i) {
        float x = px[i];
        if (x > x0 || (x == x0 && py[i] < py[i0])) { i0 = i; x0 = x; }
    }
    int hull[4], m = 0, ih = i0;
    for (;;) {
        if (m >= 4) return false;
        hull[m] = ih;
        int ie = 0;
        for (int j = 1; j < n; ++j) {
            if (ie == ih) { ie = j; continue; }
            float rx = px[ie] - px[hull[m]], ry = py[ie] - py[hull[m]];
            float wx = px[j] - px[hull[m]], wy = py[j] - py[hull[m]];
            float c = rx * wy - ry * wx;
            if (c < 0.0f) ie = j;
            if (c == 0.0f && wx * wx + wy * wy > rx * rx + ry * ry) ie = j;
        }
        ++m;
        ih = ie;
        if (ie == i0) break;
    }
    if (m != 4) return false;
    for (int i = 0; i < 4; ++i) { vx[i] = px[hull[i]]; vy[i] = py[hull[i]]; }
    for (int i = 0; i < 4; ++i) {
        int i2 = i + 1 < 4 ? i + 1 : 0;
        float ex = vx[i2] - vx[i], ey = vy[i2] - vy[i];
        float tx = 1.0f * ey, ty = -1.0f * ex; // b2Cross(edge, 1.0f)
        float len = sqrtf(tx * tx + ty * ty);
        if (!(len < B2_EPSILON)) {
            float inv = 1.0f / len;
            tx *= inv;
            ty *= inv;
        }
        nx[i] = tx;
        ny[i] = ty;
    }
    return true;
}

extern "C" int rem2d_world_set_terrain(rem2d_world *w, const float *xs, const float *ys, int32_t npts, const float *polys,
                                       int32_t npolys, float friction) {
    if (!w || !xs || !ys || npts < 2) return fail(REM2D_E_INVALID, "terrain needs at least two polyline points");
    if (npolys < 0 || (npolys > 0 && !polys)) return fail(REM2D_E_INVALID, "bad hardcore polygon list");
    HIP_TRY(hipSetDevice(w->cfg.device));
    const int nEdge = npts - 1, nPoly = npolys, nS = nEdge + nPoly;
    std::vector<float> h((size_t)20 * nS, 0.0f);
    float *flx = h.data(), *fly = flx + nS, *fux = fly + nS, *fuy = fux + nS;
    float *vx = fuy + nS, *vy = vx + 4 * nS, *nx = vy + 4 * nS, *ny = nx + 4 * nS;
    const float r = B2_POLYGON_RADIUS;
    for (int i = 0; i < nPoly; ++i) {
        float pvx[4], pvy[4], pnx[4], pny[4];
        if (!host_poly_set(polys + (size_t)i * 8, pvx, pvy, pnx, pny))
            return fail(REM2D_E_INVALID, "hardcore polygons must be convex quads");
        float lx = 0, ly = 0, ux = 0, uy = 0;
        for (int k = 0; k < 4; ++k) {
            vx[k * nS + i] = pvx[k]; vy[k * nS + i] = pvy[k]; nx[k * nS + i] = pnx[k]; ny[k * nS + i] = pny[k];
            // b2PolygonShape::ComputeAABB with the identity transform
            float tx = (1.0f * pvx[k] - 0.0f * pvy[k]) + 0.0f, ty = (0.0f * pvx[k] + 1.0f * pvy[k]) + 0.0f;
            if (k == 0) { lx = ux = tx; ly = uy = ty; }
            else { lx = lx < tx ? lx : tx; ly = ly < ty ? ly : ty; ux = ux > tx ? ux : tx; uy = uy > ty ? uy : ty; }
        }
        flx[i] = (lx - r) - B2_AABB_EXTENSION; fly[i] = (ly - r) - B2_AABB_EXTENSION;
        fux[i] = (ux + r) + B2_AABB_EXTENSION; fuy[i] = (uy + r) + B2_AABB_EXTENSION;
    }
    for (int i = 0; i < nEdge; ++i) {
        const int s = nPoly + i;
        // b2EdgeShape::ComputeAABB with the identity transform, then the broadphase fattening
        float ax = (1.0f * xs[i] - 0.0f * ys[i]) + 0.0f, ay = (0.0f * xs[i] + 1.0f * ys[i]) + 0.0f;
        float bx = (1.0f * xs[i + 1] - 0.0f * ys[i + 1]) + 0.0f, by = (0.0f * xs[i + 1] + 1.0f * ys[i + 1]) + 0.0f;
        vx[0 * nS + s] = xs[i]; vy[0 * nS + s] = ys[i]; vx[1 * nS + s] = xs[i + 1]; vy[1 * nS + s] = ys[i + 1];
        float lx = ax < bx ? ax : bx, ly = ay < by ? ay : by;
        float ux = ax > bx ? ax : bx, uy = ay > by ? ay : by;
        lx = lx - r; ly = ly - r; ux = ux + r; uy = uy + r;
        flx[s] = lx - B2_AABB_EXTENSION; fly[s] = ly - B2_AABB_EXTENSION;
        fux[s] = ux + B2_AABB_EXTENSION; fuy[s] = uy + B2_AABB_EXTENSION;
    }
    float pitch = (xs[npts - 1] - xs[0]) / (float)nEdge;
    if (!(pitch > 0.0f)) return fail(REM2D_E_INVALID, "terrain xs must be increasing");
    // the edge scan assumes a (nearly) uniform pitch; verify so that the candidate range is conservative
    for (int i = 0; i < npts; ++i) {
        float expect = xs[0] + pitch * (float)i;
        if (fabsf(xs[i] - expect) > 0.1f * pitch) return fail(REM2D_E_INVALID, "terrain xs must be uniformly spaced");
    }
    if (w->terrainBuf) { (void)hipFree(w->terrainBuf); w->terrainBuf = nullptr; }
    HIP_TRY(hipMalloc((void **)&w->terrainBuf, h.size() * sizeof(float)));
    HIP_TRY(hipMemcpy(w->terrainBuf, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    Terrain &T = w->T;
    T.nEdge = nEdge;
    T.nPoly = nPoly;
    T.nStatic = nS;
    T.flx = w->terrainBuf; T.fly = T.flx + nS; T.fux = T.fly + nS; T.fuy = T.fux + nS;
    T.vx = T.fuy + nS; T.vy = T.vx + 4 * nS; T.nx = T.vy + 4 * nS; T.ny = T.nx + 4 * nS;
    T.x0 = xs[0];
    T.invPitch = 1.0f / pitch;
    T.friction = sqrtf(friction * 0.1f); // b2MixFriction(terrain fixture, module fixture friction 0.1)
    w->haveTerrain = true;
    w->epoch = next_epoch();
    return REM2D_OK;
}

extern "C" int rem2d_world_reset(rem2d_world *w, const rem2d_morph *m, void *stream) {
    if (!w || !m) return fail(REM2D_E_INVALID, "world or morphology is NULL");
    if (!m->shape || !m->hx || !m->hy || !m->x || !m->y || !m->angle || !m->parent || !m->jround || !m->ax || !m->ay ||
        !m->bx || !m->by || !m->torque || !m->lower || !m->upper || !m->amp || !m->phase || !m->freq || !m->offset ||
        !m->istate)
        return fail(REM2D_E_INVALID, "morphology has NULL arrays");
    HIP_TRY(hipSetDevice(w->cfg.device));
    int threads = 256, blocks = (w->L.Lp + threads - 1) / threads;
    hipLaunchKernelGGL(rem2d_reset_kernel, dim3(blocks), dim3(threads), 0, (hipStream_t)stream, w->S, *m, w->cfg.lanes);
    HIP_TRY(hipGetLastError());
    w->haveReset = true;
    return REM2D_OK;
}

static int pipeline_mode(const rem2d_world *w) { return w->opt[REM2D_OPT_PIPELINE] == 0 ? 0 : 3; }
// Worlds of one merged launch run in ONE kernel shape: the highest TileShape::rank among theirs.
static int launch_shape(rem2d_world *const *ws, int n_worlds) {
    int id = DEFAULT_TILE_SHAPE;
    for (int i = 0; i < n_worlds; ++i)
        if (tile_shape(ws[i]->tileShape).rank > tile_shape(id).rank) id = ws[i]->tileShape;
    return id;
}
// Every mix is sound but one kind: a flexibly placed tile of more than two passes (shape 2: 192 bodies, <= 192 joints IN ALL) may hold
// more than 64 joints in one schedule phase -- a phase is a matching, up to 32 joints per pass --, which a static kernel (shape 0: one
// phase per register set) cannot take: that launch would drop joints.
static bool shapes_mix_ok(rem2d_world *const *ws, int n_worlds) {
    const TileShape &run = tile_shape(launch_shape(ws, n_worlds));
    for (int i = 0; i < n_worlds; ++i) {
        const TileShape &planned = tile_shape(ws[i]->tileShape);
        if (!run.flex && planned.flex && planned.passes > 2) return false;
    }
    return true;
}
#define SHAPES_TRY(ws, n) \
    do { if (!shapes_mix_ok((ws), (n))) return fail(REM2D_E_INVALID, "worlds of tile shapes 0 and 2 cannot share a launch (step them in separate calls / groups)"); } while (0)

// The worlds of one launch (a step call, one step group): a list of 1 .. REM2D_MAX_BATCH worlds on the device of `same_device`
// (nullptr: of the first) that agree on REM2D_FLAG_CONTINUOUS and have their terrain and their creatures; !to_step: a list of worlds.
static int worlds_ok(rem2d_world *const *ws, int n_worlds, const rem2d_world *same_device, bool to_step) {
    if (!ws || n_worlds <= 0) return fail(REM2D_E_INVALID, "no worlds");
    static_assert(REM2D_MAX_WORLDS_PER_STEP == REM2D_MAX_BATCH, "batch size");
    if (n_worlds > REM2D_MAX_BATCH) return fail(REM2D_E_INVALID, "too many worlds for one launch");
    for (int i = 0; i < n_worlds; ++i) {
        const rem2d_world *w = ws[i];
        if (!w) return fail(REM2D_E_INVALID, "world is NULL");
        if (!to_step) continue; // (rem2d_worlds_launch_info answers for any list of worlds)
        if (!w->haveTerrain) return fail(REM2D_E_STATE, "rem2d_world_set_terrain must be called before step");
        if (!w->haveReset) return fail(REM2D_E_STATE, "rem2d_world_reset must be called before step");
        if (w->cfg.device != (same_device ? same_device : ws[0])->cfg.device) return fail(REM2D_E_INVALID, "worlds of one call must share the device");
        if ((w->cfg.flags & REM2D_FLAG_CONTINUOUS) != (ws[0]->cfg.flags & REM2D_FLAG_CONTINUOUS))
            return fail(REM2D_E_INVALID, "worlds of one launch must agree on REM2D_FLAG_CONTINUOUS");
    }
    return REM2D_OK;
}

// Kernel, grid, block, stream, arguments: the one way a step kernel is launched.  With an event pair the kernel gets its own begin /
// end timestamps (hipExtLaunchKernelGGL's start / stop events bracket exactly the kernel, which is what rocprofv3 --kernel-trace
// reports; events recorded on the stream around the launch also count the dispatch gaps).
template <typename... Params, typename... Args>
static void launch(void (*kernel)(Params...), dim3 grid, dim3 block, hipStream_t st, const EventPair *timed, const Args &...args) {
    if (timed) hipExtLaunchKernelGGL(kernel, grid, block, 0, st, timed->first, timed->second, 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, 0, st, args...);
}
// the worlds' Batch in the order given; returns the 64-lane blocks
static unsigned batch_fill(Batch &B, rem2d_world *const *ws, const int *order, int n_worlds) {
    memset(&B, 0, sizeof(B));
    unsigned blocks = 0;
    for (int i = 0; i < n_worlds; ++i) {
        const rem2d_world *w = ws[order ? order[i] : i];
        B.S[i] = w->S;
        B.T[i] = w->T;
        B.lanes[i] = w->cfg.lanes;
        blocks += (unsigned)w->L.Lp / WAVE;
        B.blockEnd[i] = blocks;
    }
    B.n = n_worlds;
    return blocks;
}
// REM2D_OPT_REBALANCE: a new creature order, made from the last step's state (the callers know when one is due)
static void launch_rebalance(rem2d_world *w, hipStream_t st, int pos_iters) {
    int threads = WAVE;
    while (threads < REBALANCE_MAX_THREADS && threads * 256 < w->cfg.n_envs) threads *= 2;
    hipLaunchKernelGGL(rem2d_rebalance_kernel, dim3(1), dim3(threads), 0, st, w->S, pos_iters);
}

// The tile pipeline for one or several worlds (lane buckets) in one grid per kernel: pre and post run one body per
// lane; the velocity iterations run one tile per wavefront (rem2d_vel4.h).  TilePlan = the launch arguments of one env-step of
// one step group (they do not change from step to step); tiles_launch_step enqueues that step's kernels.
struct TilePlan {
    Batch B;
    Vel4Batch VB;
    StepArgs A;
    Vel4Args V;
    unsigned blocks, tiles;
    int launchShape;
    bool continuous;
    bool velpost; // one launch for the velocity iterations and post (rem2d_velpost_kernel)
    bool train;   // ... and ONE launch for all steps of a call, pre and the TOI solve included (TileShape::train; REM2D_OPT_FUSE_VELPOST = 2)
    bool train128; // ... of the 128-lane tile shapes 1 / 4 (rem2d_step_train128_kernel: an item = a tile's one or two blocks)
    unsigned items; // items per step of that launch: blocks (64-lane train) / tile-sized groups of blocks summed over the worlds (128-lane)
    size_t flagWords; // ... and the hand-over flag words it needs
    rem2d_world *w0;
    rem2d_world *ws[REM2D_MAX_BATCH]; // the group's worlds (REM2D_OPT_REBALANCE runs per world)
    int nw;
};
static void tiles_plan(TilePlan &P, rem2d_world *const *ws, int n_worlds, float dt, int vel_iters, int pos_iters) {
    Vel4Batch &VB = P.VB;
    memset(&VB, 0, sizeof(VB));
    // tiles of the widest creatures first: their chains are the longest (period 3-4, more joint rounds), so they must
    // not start last
    int order[REM2D_MAX_BATCH];
    for (int i = 0; i < n_worlds; ++i) order[i] = i;
    for (int i = 1; i < n_worlds; ++i)
        for (int j = i; j > 0 && ws[order[j]]->cfg.lanes > ws[order[j - 1]]->cfg.lanes; --j) {
            const int t = order[j]; order[j] = order[j - 1]; order[j - 1] = t;
        }
    const unsigned blocks = batch_fill(P.B, ws, order, n_worlds);
    unsigned tiles = 0;
    for (int i = 0; i < n_worlds; ++i) {
        const rem2d_world *w = ws[order[i]];
        VB.S[i] = w->S;
        VB.friction[i] = w->T.friction;
        VB.lanes[i] = w->cfg.lanes;
        tiles += (unsigned)w->nTiles;
        VB.tileEnd[i] = tiles;
    }
    VB.n = n_worlds;
    P.blocks = blocks;
    P.tiles = tiles;
    P.w0 = ws[0];
    P.nw = n_worlds;
    for (int i = 0; i < n_worlds; ++i) P.ws[i] = ws[i];
    // worlds planned for different tile shapes in one grid: the largest shape runs the smaller ones' tiles as well
    // (a tile within 64 joints fits any shape; one within 64 joints per phase pair fits the four-set shape)
    P.launchShape = launch_shape(ws, n_worlds);
    P.velpost = ws[0]->opt[REM2D_OPT_FUSE_VELPOST] != 0 && P.launchShape == 3;
    for (int i = 0; i < n_worlds; ++i) // (a tile within a block: cap <= the creatures of a block)
        P.velpost = P.velpost && ws[i]->S.tileCap > 0 && ws[i]->S.tileCap * ws[i]->cfg.lanes <= WAVE && ws[i]->tileShape == 3; // (REM2D_FLAG_RETILE: tile slots and block slots go through the same creature order)
    // the step train: where the one-launch form is possible, for worlds whose creature order does not change inside a launch
    // (REM2D_FLAG_RETILE re-deals it in every step, grid-wide) and outside the fused kernel's diagnostics (REM2D_OPT_DEBUG)
    const bool wantTrain = ws[0]->opt[REM2D_OPT_FUSE_VELPOST] == 2 && ws[0]->opt[REM2D_OPT_DEBUG] == 0;
    P.train = P.velpost && wantTrain;
    for (int i = 0; i < n_worlds; ++i) P.train = P.train && !(ws[i]->cfg.flags & REM2D_FLAG_RETILE);
    P.items = blocks;
    // ... and its form for the 128-lane tile shapes (1 flexible, 4 static): regular tables of tiles of at most two blocks
    P.train128 = !P.train && wantTrain && (P.launchShape == 1 || P.launchShape == 4);
    if (P.train128) {
        unsigned items = 0;
        for (int i = 0; i < n_worlds; ++i) {
            const rem2d_world *w = ws[i];
            P.train128 = P.train128 && !(w->cfg.flags & REM2D_FLAG_RETILE) && w->S.tileCap > 0 && w->S.tileCap * w->cfg.lanes <= 2 * WAVE &&
                         (w->tileShape == 3 || w->tileShape == 1 || w->tileShape == 4);
            // the static kernel keeps the ARENA order in its velocity tiles (the host planned them for the creatures they hold) while
            // pre and post follow the creature order: under an order a tile's creatures are not the ones this workgroup's pre / post
            // handle -- legal between launches, not inside one workgroup.  Such worlds keep their per-step launches.
            if (P.launchShape == 4 && (w->S.flags & REM2D_STATE_ORDERED)) P.train128 = false;
            const unsigned lanesPerTile = (unsigned)w->S.tileCap * (unsigned)w->cfg.lanes, bpt = lanesPerTile > WAVE ? lanesPerTile / WAVE : 1u;
            items += ((unsigned)w->L.Lp / WAVE + bpt - 1) / bpt; // (the kernel's item -> world walk does the same sum)
        }
        if (P.train128) P.items = items;
    }
    P.train = P.train || P.train128;
    P.flagWords = TRAIN_FLAG_WORDS + (size_t)P.items;
    P.continuous = (ws[0]->cfg.flags & REM2D_FLAG_CONTINUOUS) != 0;
    P.A.nSteps = 1;
    P.A.dt = dt;
    P.A.velIters = vel_iters;
    P.A.posIters = pos_iters;
    // (the options of the group's first world steer the launch: a group is one launch sequence)
    P.A.heavyPerWave = ws[0]->opt[REM2D_OPT_HEAVY_PER_WAVE];
    P.A.prio = P.V.prio = ws[0]->opt[REM2D_OPT_PRIO];
    P.V.prioT1 = ws[0]->opt[REM2D_OPT_PRIO_T1];
    P.V.prioT2 = ws[0]->opt[REM2D_OPT_PRIO_T2];
    P.A.defer = P.continuous ? 2 : 0; // 2: post runs the TOI scan itself (the fused kernel's path keeps 1 = separate scan kernel)
    P.V.velIters = vel_iters;
    P.V.dt = dt;
    P.V.dbg = ws[0]->opt[REM2D_OPT_DEBUG];
}
// one env-step of one step group.  With timing on (rem2d_world_enable_timing; never inside a region whose wall time is
// being measured -- bench.py times kernels in a pass of its own) the dominant kernel gets its own begin / end timestamps
// (launch) and the whole sequence a pair of stream events.
static void tiles_launch_step(const TilePlan &P, hipStream_t st) {
    rem2d_world *w0 = P.w0;
    const TileShape &shape = tile_shape(P.launchShape); // (a merged launch of shapes 1 and 4: rank picks 1, whose flexible kernel takes the statically planned tiles too)
    const dim3 grid(P.blocks), block(WAVE);
    // (the step's time bracket opens in front of the re-ordering launches: they belong to the step that needs them)
    const bool timedStep = w0->evStep.open(w0->timing, st);
    for (int i = 0; i < P.nw; ++i) { // REM2D_OPT_REBALANCE: a new creature order every N env-steps
        rem2d_world *w = P.ws[i];
        const int every = w->opt[REM2D_OPT_REBALANCE];
        if (every > 0 && w->stepsQueued > 0 && w->stepsQueued % every == 0 && (w->S.flags & REM2D_STATE_ORDERED)) launch_rebalance(w, st, P.A.posIters);
        w->stepsQueued += 1;
    }
    launch(shape.pre, grid, block, st, nullptr, P.B, P.A);
    const EventPair *timed = w0->evKernel.take(w0->timing);
    if (P.velpost) {
        launch(rem2d_velpost_kernel, grid, dim3(WAVE * REM2D_VELPOST_WAVES), st, timed, P.B, P.A, P.V);
    } else {
        launch(shape.vel4, dim3(P.tiles), block, st, timed, P.VB, P.V);
        launch(rem2d_post_multi_kernel, grid, block, st, nullptr, P.B, P.A);
    }
    if (P.continuous) launch(rem2d_toi_heavy_multi_kernel, grid, block, st, nullptr, P.B, P.A);
    if (timedStep) w0->evStep.close(st, 1);
}
// The step train (TileShape::train): the steps of a call in one launch -- or in one launch per stretch between two
// re-orderings of the creature order (REM2D_OPT_REBALANCE), which run in front of the stretch they are due for.
// (the flag buffer and the failure counter of a train's first world: sized before anything of the launch is queued -- growing frees
// the old buffer, which waits for the launches that use it)
static int train_reserve(const TilePlan &P) {
    rem2d_world *w0 = P.w0;
    const size_t need = P.flagWords;
    if (w0->trainCap < need) {
        if (w0->trainFlags) HIP_TRY(hipFree(w0->trainFlags));
        w0->trainFlags = nullptr; w0->trainCap = 0;
        HIP_TRY(hipMalloc(&w0->trainFlags, need * sizeof(unsigned)));
        w0->trainCap = need;
    }
    if (!w0->trainFailures) {
        HIP_TRY(hipHostMalloc((void **)&w0->trainFailures, sizeof(unsigned), hipHostMallocDefault));
        *w0->trainFailures = 0u;
    }
    return REM2D_OK;
}
static int tiles_launch_train(TilePlan &P, hipStream_t st, int n_steps) {
    rem2d_world *w0 = P.w0;
    { int rc = train_reserve(P); if (rc != REM2D_OK) return rc; }
    const unsigned nPad = (P.items + 7u) & ~7u;
    const int fault = w0->opt[REM2D_OPT_TRAIN_FAULT];
    // The creature order is re-made in front of a launch once N (REM2D_OPT_REBALANCE) or more steps have run since the last time --
    // a cadence in launches, not in steps: a call is cut only where it is itself longer than N steps, never because a multiple
    // of N falls inside it (two short trains drain twice).  Any cadence gives the same bits.
    int l = 0;
    while (l < n_steps) {
        int seg = n_steps - l;
        if ((unsigned long long)nPad * (unsigned)seg > 0x7fffffffull) seg = (int)(0x7fffffffull / nPad);
        if (seg > (int)TRAIN_STEP_MASK) seg = (int)TRAIN_STEP_MASK; // (the flag's step field; nPad >= 8 keeps seg below it anyway)
        for (int i = 0; i < P.nw; ++i) {
            const int every = P.ws[i]->opt[REM2D_OPT_REBALANCE];
            if (every > 0 && seg > every) seg = every;
        }
        const bool timedStep = w0->evStep.open(w0->timing, st);
        for (int i = 0; i < P.nw; ++i) {
            rem2d_world *w = P.ws[i];
            const int every = w->opt[REM2D_OPT_REBALANCE];
            if (every > 0 && w->stepsQueued > 0 && w->stepsQueued - w->stepsAtOrder >= every && (w->S.flags & REM2D_STATE_ORDERED)) {
                launch_rebalance(w, st, P.A.posIters);
                w->stepsAtOrder = w->stepsQueued;
            }
            w->stepsQueued += seg;
        }
        HIP_TRY(hipMemsetAsync(w0->trainFlags, 0, P.flagWords * sizeof(unsigned), st));
        P.A.nSteps = seg;
        launch(tile_shape(P.launchShape).train, dim3(nPad * (unsigned)seg), dim3(WAVE), st, w0->evKernel.take(w0->timing), P.B, P.A, P.V,
               w0->trainFlags, P.items, fault, w0->trainFailures);
        if (timedStep) w0->evStep.close(st, seg); // (this bracket holds `seg` env-steps)
        l += seg;
    }
    P.A.nSteps = 1;
    HIP_TRY(hipGetLastError());
    return REM2D_OK;
}
static int step_tiles(rem2d_world *const *ws, int n_worlds, int n_steps, float dt, int vel_iters, int pos_iters, hipStream_t st) {
    TilePlan P;
    tiles_plan(P, ws, n_worlds, dt, vel_iters, pos_iters);
    if (P.train) return tiles_launch_train(P, st, n_steps);
    for (int l = 0; l < n_steps; ++l) tiles_launch_step(P, st);
    HIP_TRY(hipGetLastError());
    return REM2D_OK;
}

// The fused formulation (REM2D_PIPELINE=0; round 1's body-per-lane step kernel + the TOI kernels) for one or several
// worlds in one grid per kernel: n_steps env-steps per launch in discrete mode, one per launch when the TOI kernels follow.
static int step_fused(rem2d_world *const *ws, int n_worlds, int n_steps, float dt, int vel_iters, int pos_iters, hipStream_t st) {
    Batch B;
    const dim3 grid(batch_fill(B, ws, nullptr, n_worlds)), block(WAVE);
    rem2d_world *w0 = ws[0];
    const bool continuous = (w0->cfg.flags & REM2D_FLAG_CONTINUOUS) != 0;
    StepArgs A;
    A.nSteps = continuous ? 1 : n_steps;
    A.dt = dt;
    A.velIters = vel_iters;
    A.posIters = pos_iters;
    A.heavyPerWave = w0->opt[REM2D_OPT_HEAVY_PER_WAVE];
    A.prio = w0->opt[REM2D_OPT_PRIO];
    A.defer = continuous ? 1 : 0;
    const int launches = continuous ? n_steps : 1;
    for (int l = 0; l < launches; ++l) {
        const bool timed = w0->evKernel.open(w0->timing, st); // (stream events around the kernel: the form this path has always reported)
        launch(rem2d_step_multi_kernel, grid, block, st, nullptr, B, A);
        if (timed) w0->evKernel.close(st, 1);
        if (continuous) {
            launch(rem2d_toi_scan_multi_kernel, grid, block, st, nullptr, B, A);
            launch(rem2d_toi_heavy_multi_kernel, grid, block, st, nullptr, B, A);
        }
    }
    HIP_TRY(hipGetLastError());
    return REM2D_OK;
}

extern "C" int rem2d_worlds_launch_info(rem2d_world *const *ws, int32_t n_worlds, int32_t *tile_shape_out, int32_t *fused_velpost) {
    { int rc = worlds_ok(ws, n_worlds, nullptr, false); if (rc != REM2D_OK) return rc; }
    if (pipeline_mode(ws[0]) != 3) { // the fused step kernel: no tiles
        if (tile_shape_out) *tile_shape_out = -1;
        if (fused_velpost) *fused_velpost = 0;
        return REM2D_OK;
    }
    SHAPES_TRY(ws, n_worlds);
    TilePlan P;
    tiles_plan(P, ws, n_worlds, 1.0f / 50.0f, 180, 60);
    if (tile_shape_out) *tile_shape_out = P.launchShape;
    if (fused_velpost) *fused_velpost = P.train ? 2 : (P.velpost ? 1 : 0); // (2 with tile shape 1 / 4: rem2d_step_train128_kernel)
    return REM2D_OK;
}

// The solver loops count ticks (iteration x schedule period + joint round) in 16 bits (wave_max_active): refuse iteration
// counts that would not fit instead of silently running fewer sweeps.  (Box2D's own arguments are 8 / 3; the reference
// passes 180 / 60, Modular2DEnv.py:634.)
#define REM2D_MAX_ITERS 8192
static bool iters_ok(int vel_iters, int pos_iters) {
    return vel_iters >= 0 && pos_iters >= 0 && vel_iters <= REM2D_MAX_ITERS && pos_iters <= REM2D_MAX_ITERS;
}
#define ITERS_TRY(v, p) \
    do { if (!iters_ok((v), (p))) return fail(REM2D_E_INVALID, "velocity / position iterations must be in 0..8192"); } while (0)
// b2World::Step skips Solve and SolveTOI at dt == 0 and keeps the old inv_dt0; the kernels have no such path (only invDt0 and the
// TOI scan look at h > 0), and a negative or non-finite dt is a caller's error in Box2D too: refuse all of them here, before a launch.
static bool dt_ok(float dt) { return dt > 0.0f && dt <= 3.402823466e+38f; } // (false for NaN: both comparisons are)
#define DT_TRY(dt) \
    do { if (!dt_ok(dt)) return fail(REM2D_E_INVALID, "dt must be finite and > 0"); } while (0)

extern "C" int rem2d_world_step_ex(rem2d_world *w, int32_t n_steps, float dt, int32_t vel_iters, int32_t pos_iters,
                                   void *stream) {
    return rem2d_worlds_step_ex(&w, 1, n_steps, dt, vel_iters, pos_iters, stream);
}
extern "C" int rem2d_worlds_step_ex(rem2d_world *const *ws, int32_t n_worlds, int32_t n_steps, float dt, int32_t vel_iters,
                                    int32_t pos_iters, void *stream) {
    ITERS_TRY(vel_iters, pos_iters); // (first: what a caller passes for the worlds is not looked at behind bad counts)
    DT_TRY(dt);
    { int rc = worlds_ok(ws, n_worlds, nullptr, true); if (rc != REM2D_OK) return rc; }
    if (n_steps <= 0) return REM2D_OK;
    HIP_TRY(hipSetDevice(ws[0]->cfg.device));
    if (pipeline_mode(ws[0]) != 3) return step_fused(ws, n_worlds, n_steps, dt, vel_iters, pos_iters, (hipStream_t)stream);
    SHAPES_TRY(ws, n_worlds);
    return step_tiles(ws, n_worlds, n_steps, dt, vel_iters, pos_iters, (hipStream_t)stream);
}
extern "C" int rem2d_worlds_step(rem2d_world *const *ws, int32_t n_worlds, int32_t n_steps, void *stream) {
    return rem2d_worlds_step_ex(ws, n_worlds, n_steps, (float)(1.0 / 50), 6 * 30, 2 * 30, stream);
}
extern "C" int rem2d_world_step(rem2d_world *w, int32_t n_steps, void *stream) {
    // Modular2DEnv.py:634  self.world.Step(1.0/FPS, 6*30, 2*30)
    return rem2d_world_step_ex(w, n_steps, (float)(1.0 / 50), 6 * 30, 2 * 30, stream);
}

// ---- all step groups of a population in one call (include/rem2d.h) ----
// Graph replay: the launches of one call (n_steps x groups x 3-4 kernels, fork / join edges between the streams) are
// captured once and replayed with one hipGraphLaunch per call; the kernel arguments are by-value structs that only
// change when a world's tile table / outputs / terrain change (epoch).
struct GraphEntry {
    uint64_t key;
    hipGraphExec_t exec;
    hipGraph_t graph;
    std::vector<const rem2d_world *> worlds; // whose kernel arguments and fork / join events the replay holds
};
static std::vector<GraphEntry> g_graphs;
// one lock for the replay cache and the capture stream: ctypes releases the GIL around the ABI calls, so two host threads
// may step / destroy different envs at once.  Held across capture, instantiate and launch (a capture in Relaxed mode on
// the one shared capture stream must not interleave with another) and while a destroy drops the replays of its world.
static std::mutex g_graphMu;
static void graph_entry_free(GraphEntry &e) {
    (void)hipDeviceSynchronize(); // (a replay may still be in flight)
    (void)hipGraphExecDestroy(e.exec);
    (void)hipGraphDestroy(e.graph);
}
// a world is going away: so must every replay that was captured with it (its events and scratch pointers)
static void graphs_forget(const rem2d_world *w) {
    std::lock_guard<std::mutex> lk(g_graphMu);
    for (size_t i = 0; i < g_graphs.size();) {
        bool uses = false;
        for (const rem2d_world *x : g_graphs[i].worlds) uses = uses || x == w;
        if (uses) {
            graph_entry_free(g_graphs[i]);
            g_graphs.erase(g_graphs.begin() + (long)i);
        } else {
            ++i;
        }
    }
}
static hipStream_t g_captureStream = nullptr;
static uint64_t mix64(uint64_t h, uint64_t v) {
    h ^= v + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
    return h;
}

static hipStream_t group_stream(const rem2d_step_group &g, hipStream_t origin) { return g.stream ? (hipStream_t)g.stream : origin; }
// `plans`: the groups' TilePlans (tiles_plan), or nullptr for the fused kernel
static int groups_enqueue(const rem2d_step_group *groups, int n_groups, TilePlan *plans, int n_steps, float dt, int vel_iters,
                          int pos_iters, hipStream_t origin) {
    // (a step train's flag buffer is sized BEFORE the fork: growing it frees the old one, a device-wide wait that does not belong
    // between a fork and its join, and an error here must not leave forked streams behind)
    for (int g = 0; plans && g < n_groups; ++g)
        if (plans[g].train) { int rc = train_reserve(plans[g]); if (rc != REM2D_OK) return rc; }
    // fork: every group stream waits for what the origin stream has queued so far
    rem2d_world *w00 = groups[0].worlds[0];
    bool forked = false;
    int rcAll = REM2D_OK; // (an error after the fork still runs the join: no group stream is left un-joined behind an error return)
    for (int g = 0; g < n_groups; ++g) {
        hipStream_t sg = group_stream(groups[g], origin);
        if (sg == origin) continue;
        if (!forked) {
            HIP_TRY(hipEventRecord(w00->evFork, origin));
            forked = true;
        }
        HIP_TRY(hipStreamWaitEvent(sg, w00->evFork, 0));
    }
    if (plans) {
        // round-robin: step l of every group is queued before step l + 1 of any, so that no group's stream runs dry while
        // the host is still busy queueing another group's whole train (and the groups start together)
        for (int g = 0; g < n_groups && rcAll == REM2D_OK; ++g) // (a group whose steps go in one launch: queued whole)
            if (plans[g].train) rcAll = tiles_launch_train(plans[g], group_stream(groups[g], origin), n_steps);
        for (int l = 0; l < n_steps && rcAll == REM2D_OK; ++l)
            for (int g = 0; g < n_groups; ++g)
                if (!plans[g].train) tiles_launch_step(plans[g], group_stream(groups[g], origin));
        if (rcAll == REM2D_OK) {
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) rcAll = fail(REM2D_E_HIP, std::string("groups_enqueue: ") + hipGetErrorString(e));
        }
    } else {
        for (int g = 0; g < n_groups && rcAll == REM2D_OK; ++g)
            rcAll = step_fused(groups[g].worlds, groups[g].n_worlds, n_steps, dt, vel_iters, pos_iters, group_stream(groups[g], origin));
    }
    // join: the origin stream waits for every group
    for (int g = 0; g < n_groups; ++g) {
        hipStream_t sg = group_stream(groups[g], origin);
        if (sg == origin) continue;
        rem2d_world *wg = groups[g].worlds[0];
        hipError_t e = hipEventRecord(wg->evJoin, sg);
        if (e == hipSuccess) e = hipStreamWaitEvent(origin, wg->evJoin, 0);
        if (e != hipSuccess && rcAll == REM2D_OK) rcAll = fail(REM2D_E_HIP, std::string("groups_enqueue (join): ") + hipGetErrorString(e));
    }
    return rcAll;
}

extern "C" int rem2d_groups_step_ex(const rem2d_step_group *groups, int32_t n_groups, int32_t n_steps, float dt,
                                    int32_t vel_iters, int32_t pos_iters, void *stream, uint32_t flags) {
    if (!groups || n_groups <= 0) return fail(REM2D_E_INVALID, "no step groups");
    if (n_groups > REM2D_MAX_STEP_GROUPS) return fail(REM2D_E_INVALID, "too many step groups");
    ITERS_TRY(vel_iters, pos_iters);
    DT_TRY(dt);
    bool timing = false;
    for (int g = 0; g < n_groups; ++g) {
        int rc = worlds_ok(groups[g].worlds, groups[g].n_worlds, g > 0 ? groups[0].worlds[0] : nullptr, true);
        if (rc != REM2D_OK) return rc;
        for (int i = 0; i < groups[g].n_worlds; ++i) timing = timing || groups[g].worlds[i]->timing;
    }
    if (n_steps <= 0) return REM2D_OK;
    rem2d_world *w00 = groups[0].worlds[0];
    HIP_TRY(hipSetDevice(w00->cfg.device));
    for (int g = 0; g < n_groups; ++g) {
        rem2d_world *wg = groups[g].worlds[0];
        if (!wg->evFork) HIP_TRY(hipEventCreateWithFlags(&wg->evFork, hipEventDisableTiming));
        if (!wg->evJoin) HIP_TRY(hipEventCreateWithFlags(&wg->evJoin, hipEventDisableTiming));
    }
    hipStream_t origin = (hipStream_t)stream;
    if (pipeline_mode(w00) != 3) return groups_enqueue(groups, n_groups, nullptr, n_steps, dt, vel_iters, pos_iters, origin);
    // the groups' plans, made once: the plain enqueue, the capture and the choice between them read the same ones
    TilePlan plans[REM2D_MAX_STEP_GROUPS];
    bool train = false; // (a step train is one launch per call already, and sizes its flag buffer while it is queued: never captured)
    for (int g = 0; g < n_groups; ++g) {
        SHAPES_TRY(groups[g].worlds, groups[g].n_worlds);
        tiles_plan(plans[g], groups[g].worlds, groups[g].n_worlds, dt, vel_iters, pos_iters);
        train = train || plans[g].train;
    }
    if (!(flags & REM2D_STEP_GRAPH) || timing || train)
        return groups_enqueue(groups, n_groups, plans, n_steps, dt, vel_iters, pos_iters, origin);

    // ---- graph replay ----
    std::lock_guard<std::mutex> graphLock(g_graphMu);
    uint64_t key = mix64(0x5bd1e995u, (uint64_t)n_steps);
    key = mix64(key, (uint64_t)__float_as_uint_host(dt));
    key = mix64(key, ((uint64_t)(uint32_t)vel_iters << 32) | (uint32_t)pos_iters);
    for (int g = 0; g < n_groups; ++g) {
        key = mix64(key, (uint64_t)(uintptr_t)groups[g].stream);
        for (int i = 0; i < groups[g].n_worlds; ++i) {
            const rem2d_world *w = groups[g].worlds[i];
            key = mix64(key, (uint64_t)(uintptr_t)w);
            key = mix64(key, w->epoch);
            // REM2D_OPT_REBALANCE: which steps of the call carry a re-ordering launch depends on where the call starts in the
            // cadence -- part of the key, so that a replay re-orders every N env-steps exactly like the plain enqueue does.  A world's
            // very first step is a phase of its own (`every`): nothing is re-ordered in front of it, so a call captured there holds
            // one launch less than the same call N steps later, which must not replay it
            const int every = w->opt[REM2D_OPT_REBALANCE];
            if (every > 0) key = mix64(key, 0xabcd0000ull + (uint64_t)(w->stepsQueued == 0 ? every : w->stepsQueued % every));
        }
        key = mix64(key, 0xfeedull + (uint64_t)groups[g].n_worlds);
    }
    GraphEntry *hit = nullptr;
    for (auto &e : g_graphs)
        if (e.key == key) hit = &e;
    if (!hit) {
        if (!g_captureStream) HIP_TRY(hipStreamCreateWithFlags(&g_captureStream, hipStreamNonBlocking));
        // the capture starts on a stream of the library's own (the caller's may be the NULL stream, which cannot capture);
        // group streams are pulled into the capture by the fork events
        HIP_TRY(hipStreamBeginCapture(g_captureStream, hipStreamCaptureModeRelaxed));
        int rc = groups_enqueue(groups, n_groups, plans, n_steps, dt, vel_iters, pos_iters, g_captureStream);
        hipGraph_t graph = nullptr;
        hipError_t e = hipStreamEndCapture(g_captureStream, &graph);
        if (rc != REM2D_OK) {
            if (graph) (void)hipGraphDestroy(graph);
            return rc;
        }
        if (e != hipSuccess) return fail(REM2D_E_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
        hipGraphExec_t exec = nullptr;
        e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        if (e != hipSuccess) {
            (void)hipGraphDestroy(graph);
            return fail(REM2D_E_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
        }
        if (g_graphs.size() >= 16) { // call lengths come and go: drop the oldest replay
            graph_entry_free(g_graphs.front());
            g_graphs.erase(g_graphs.begin());
        }
        GraphEntry ge;
        ge.key = key; ge.exec = exec; ge.graph = graph;
        for (int g = 0; g < n_groups; ++g)
            for (int i = 0; i < groups[g].n_worlds; ++i) ge.worlds.push_back(groups[g].worlds[i]);
        g_graphs.push_back(ge);
        hit = &g_graphs.back();
    } else { // (a capture advances the worlds' step counters itself, tiles_launch_step; a replay does it here)
        for (int g = 0; g < n_groups; ++g)
            for (int i = 0; i < groups[g].n_worlds; ++i) groups[g].worlds[i]->stepsQueued += n_steps;
    }
    HIP_TRY(hipGraphLaunch(hit->exec, origin));
    return REM2D_OK;
}
extern "C" int rem2d_groups_step(const rem2d_step_group *groups, int32_t n_groups, int32_t n_steps, void *stream, uint32_t flags) {
    return rem2d_groups_step_ex(groups, n_groups, n_steps, (float)(1.0 / 50), 6 * 30, 2 * 30, stream, flags);
}

// ---- the creature order, read back and made on demand (include/rem2d_order.h): host code around what is there ----
extern "C" int rem2d_order_abi_version(void) { return REM2D_ORDER_ABI_VERSION; }
extern "C" int rem2d_world_read_order(const rem2d_world *w, int32_t *out_dev, void *stream) {
    if (!w) return fail(REM2D_E_INVALID, "read_order: world is NULL");
    if (!out_dev) return fail(REM2D_E_INVALID, "read_order: NULL output array");
    HIP_TRY(hipSetDevice(w->cfg.device));
    HIP_TRY(hipMemcpyAsync(out_dev, w->S.order, (size_t)2 * w->L.Np * sizeof(int), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return REM2D_OK;
}
extern "C" int rem2d_world_make_order(rem2d_world *w, int32_t pos_iters, void *stream) {
    if (!w) return fail(REM2D_E_INVALID, "make_order: world is NULL");
    if (w->cfg.flags & REM2D_FLAG_RETILE) return fail(REM2D_E_INVALID, "make_order: the world deals its creatures itself (REM2D_FLAG_RETILE)");
    if (pos_iters < 1) return fail(REM2D_E_INVALID, "make_order: pos_iters must be >= 1");
    HIP_TRY(hipSetDevice(w->cfg.device));
    launch_rebalance(w, (hipStream_t)stream, pos_iters); // (the step paths' own launch: stepsQueued, stepsAtOrder, flags and options stay)
    HIP_TRY(hipGetLastError());
    return REM2D_OK;
}

extern "C" int rem2d_tree_diversity(const double *pos_dev, const int32_t *count_dev, int32_t n_trees, int32_t max_nodes,
                                    int64_t *out_dev, int32_t device, void *stream) {
    if (!pos_dev || !count_dev || !out_dev) return fail(REM2D_E_INVALID, "NULL device pointer");
    if (n_trees < 0 || max_nodes <= 0 || max_nodes > DIV_MAX_NODES)
        return fail(REM2D_E_INVALID, "max_nodes must be 1..64");
    if (n_trees == 0) return REM2D_OK;
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(rem2d_tree_diversity_kernel, dim3((unsigned)n_trees), dim3(DIV_THREADS), 0, (hipStream_t)stream, pos_dev,
                       count_dev, n_trees, max_nodes, (long long *)out_dev);
    HIP_TRY(hipGetLastError());
    return REM2D_OK;
}

#include "rem2d_compile.h"

// ---- self-test of the scalar helpers the solvers are built from (include/rem2d.h rem2d_selftest_scalar) ----
__global__ void rem2d_selftest_scalar_kernel(const float *a, const float *b, const float *c, int n, float *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = fmin32(a[i], b[i]);
    out[(size_t)n + i] = fmax32(a[i], b[i]);
    out[2 * (size_t)n + i] = fclamp(a[i], b[i], c[i]);
    const Rot q = rot_set(a[i]);
    out[3 * (size_t)n + i] = q.s;
    out[4 * (size_t)n + i] = q.c;
}
extern "C" int rem2d_selftest_scalar(const float *a_dev, const float *b_dev, const float *c_dev, int32_t n, float *out_dev,
                                     int32_t device, void *stream) {
    if (!a_dev || !b_dev || !c_dev || !out_dev) return fail(REM2D_E_INVALID, "NULL device pointer");
    if (n <= 0) return REM2D_OK;
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(rem2d_selftest_scalar_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a_dev,
                       b_dev, c_dev, n, out_dev);
    HIP_TRY(hipGetLastError());
    return REM2D_OK;
}

extern "C" int rem2d_world_field(const rem2d_world *w, int32_t field, size_t *offset_bytes, size_t *count, int32_t *dtype) {
    if (!w || field < 0 || field >= REM2D_F_COUNT) return fail(REM2D_E_INVALID, "bad field id");
    int dt = 0;
    field_place(w->L, field, offset_bytes, count, &dt);
    if (dtype) *dtype = dt;
    return REM2D_OK;
}

// ---- population-order read-back of a per-creature field (include/rem2d_gather.h) ----
// Part of this library's code object, which the first step has loaded: a caller's first read after the steps loads nothing.  (A torch
// indexing kernel in its place loads its own code object at its first launch: 8-45 ms inside the first timed block of bench.py.)
template <typename T>
__global__ void rem2d_gather_kernel(const T *src, const int32_t *index, unsigned n, T *out, unsigned long long outCount) {
    const unsigned e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int32_t i = index[e];
    if (i >= 0 && (unsigned long long)i < outCount) out[i] = src[e];
}
extern "C" int rem2d_world_gather(const rem2d_world *w, int32_t field, void *out_dev, int64_t out_count, void *stream) {
    if (!w) return fail(REM2D_E_INVALID, "world is NULL");
    if (field < REM2D_F_WOD || field >= REM2D_F_COUNT) return fail(REM2D_E_INVALID, "gather: not a per-creature field");
    if (!out_dev || out_count < 0) return fail(REM2D_E_INVALID, "gather: no output buffer");
    if (!w->S.outIndex) return fail(REM2D_E_STATE, "gather: rem2d_world_set_outputs has installed no population index");
    size_t off = 0;
    int dt = 0;
    field_place(w->L, field, &off, nullptr, &dt);
    const unsigned n = (unsigned)w->cfg.n_envs;
    HIP_TRY(hipSetDevice(w->cfg.device));
    const dim3 grid((n + 255u) / 256u), block(256);
    if (dt == REM2D_DT_F64)
        hipLaunchKernelGGL(rem2d_gather_kernel<uint64_t>, grid, block, 0, (hipStream_t)stream, (const uint64_t *)(w->state + off),
                           w->S.outIndex, n, (uint64_t *)out_dev, (unsigned long long)out_count);
    else
        hipLaunchKernelGGL(rem2d_gather_kernel<uint32_t>, grid, block, 0, (hipStream_t)stream, (const uint32_t *)(w->state + off),
                           w->S.outIndex, n, (uint32_t *)out_dev, (unsigned long long)out_count);
    HIP_TRY(hipGetLastError());
    return REM2D_OK;
}

// ---- the creature renderer (include/rem2d_render.h, rem2d_raster.h) ----
extern "C" int rem2d_render_abi_version(void) { return REM2D_RENDER_ABI_VERSION; }
extern "C" int rem2d_world_render(const rem2d_world *w, const int32_t *creatures_dev, int32_t n, const float *cam_xy_dev,
                                  const uint8_t *fill_rgb_dev, const uint8_t *line_rgb_dev, int32_t width, int32_t height,
                                  uint8_t *out_dev, void *stream) {
    if (!w) return fail(REM2D_E_INVALID, "render: world is NULL");
    if (n < 0) return fail(REM2D_E_INVALID, "render: n < 0");
    if (width < 1 || height < 1 || width > REM2D_RENDER_MAX_SIZE || height > REM2D_RENDER_MAX_SIZE)
        return fail(REM2D_E_INVALID, "render: width and height must be 1.." + std::to_string(REM2D_RENDER_MAX_SIZE) + ", not " +
                                         std::to_string(width) + " x " + std::to_string(height));
    if (!w->haveTerrain) return fail(REM2D_E_STATE, "render: rem2d_world_set_terrain must be called before render");
    if (n == 0) return REM2D_OK;
    if (!creatures_dev || !cam_xy_dev || !out_dev) return fail(REM2D_E_INVALID, "render: NULL device pointer");
    if (w->cfg.lanes > 64) return fail(REM2D_E_INVALID, "render: more than 64 lanes per creature");
    static_assert(R_MAX_SIZE == REM2D_RENDER_MAX_SIZE, "one size limit");
    HIP_TRY(hipSetDevice(w->cfg.device));
    std::vector<int32_t> idx((size_t)n);
    HIP_TRY(hipMemcpyAsync(idx.data(), creatures_dev, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    for (int32_t k = 0; k < n; ++k)
        if (idx[k] < 0 || idx[k] >= w->cfg.n_envs)
            return fail(REM2D_E_INVALID, "render: creature index " + std::to_string(idx[k]) + " (image " + std::to_string(k) +
                                             ") outside the world's 0.." + std::to_string(w->cfg.n_envs - 1));
    const int tilesX = (width + R_TILE_W - 1) / R_TILE_W, tilesY = (height + R_TILE_H - 1) / R_TILE_H;
    const long long blocks = (long long)tilesX * tilesY * n;
    if (blocks > 0x7fffffffLL) return fail(REM2D_E_INVALID, "render: too many images for one launch");
    hipLaunchKernelGGL(rem2d_render_kernel, dim3((unsigned)blocks), dim3(R_THREADS), 0, (hipStream_t)stream, w->S, w->T, w->cfg.lanes,
                       w->cfg.n_envs, creatures_dev, cam_xy_dev, fill_rgb_dev, line_rgb_dev, (int)width, (int)height, tilesX,
                       tilesX * tilesY, out_dev);
    HIP_TRY(hipGetLastError());
    return REM2D_OK;
}

// ---- closed-loop control (include/rem2d_control.h, csrc/rem2d_control.h) ----
extern "C" int rem2d_control_abi_version(void) { return REM2D_CONTROL_ABI_VERSION; }
// The refusals that the calls on a list of worlds share, one fault each; `p` is the caller's prefix ("observe: ").  Every call
// composes them in an order of its own, which tests/golden/world_call_refusals.json holds: no function here knows its caller.
static int worlds_given(const std::string &p, rem2d_world *const *worlds, int32_t n_worlds) {
    return worlds && n_worlds > 0 ? REM2D_OK : fail(REM2D_E_INVALID, p + "no worlds");
}
static int rows_ok(const std::string &p, int64_t rows) { return rows >= 0 ? REM2D_OK : fail(REM2D_E_INVALID, p + "negative row count"); }
static int max_bodies_ok(const std::string &p, int32_t max_bodies) {
    if (max_bodies >= 1 && max_bodies <= REM2D_CONTROL_MAX_BODIES) return REM2D_OK;
    return fail(REM2D_E_INVALID, p + "max_bodies must be 1.." + std::to_string(REM2D_CONTROL_MAX_BODIES) + ", not " + std::to_string(max_bodies));
}
static int world_present(const std::string &p, rem2d_world *const *worlds, int32_t i) {
    return worlds[i] ? REM2D_OK : fail(REM2D_E_INVALID, p + "world " + std::to_string(i) + " is NULL");
}
static int worlds_present(const std::string &p, rem2d_world *const *worlds, int32_t n_worlds) {
    for (int32_t i = 0; i < n_worlds; ++i) OK_TRY(world_present(p, worlds, i));
    return REM2D_OK;
}
// (lanes, then device: no call has anything between the two)
static int world_fits(const std::string &p, const rem2d_world *w, const rem2d_world *first) {
    if (w->cfg.lanes > 64) return fail(REM2D_E_INVALID, p + "more than 64 lanes per creature");
    return w->cfg.device == first->cfg.device ? REM2D_OK : fail(REM2D_E_INVALID, p + "the worlds must share a device");
}
static int world_terrain(const std::string &p, const rem2d_world *w) {
    return w->haveTerrain ? REM2D_OK : fail(REM2D_E_STATE, p + "rem2d_world_set_terrain must be called first");
}
static int world_reset(const std::string &p, const rem2d_world *w) {
    return w->haveReset ? REM2D_OK : fail(REM2D_E_STATE, p + "rem2d_world_reset (or adopt) must be called first");
}
// The order of observe, control, describe and the act calls: world by world, a NULL among them.
static int worlds_ready(const std::string &p, rem2d_world *const *worlds, int32_t n_worlds) {
    for (int32_t i = 0; i < n_worlds; ++i) {
        OK_TRY(world_present(p, worlds, i));
        OK_TRY(world_fits(p, worlds[i], worlds[0]));
        OK_TRY(world_reset(p, worlds[i]));
    }
    return REM2D_OK;
}
// The table of worlds [first, first + n) of a call (n <= CTL_TABLE) -> the 64-lane blocks of the launch.
static unsigned control_table(CtlTable &Tb, rem2d_world *const *worlds, int first, int n) {
    memset(&Tb, 0, sizeof(Tb));
    unsigned blocks = 0;
    for (int i = 0; i < n; ++i) {
        const rem2d_world *w = worlds[first + i];
        CtlWorld &c = Tb.w[i];
        c.lane4 = w->S.lane4; c.lane8 = w->S.lane8; c.slot4 = w->S.slot4; c.env8 = w->S.env8;
        c.index = w->S.outIndex;
        c.Lp = w->S.Lp; c.Np = w->S.Np; c.nEnvs = w->S.nEnvs; c.lanes = (unsigned)w->cfg.lanes;
        blocks += (unsigned)w->L.Lp / WAVE;
        c.blockEnd = blocks;
    }
    Tb.n = n;
    return blocks;
}
// The launches of a call on checked worlds, one per `table` worlds (CTL_TABLE; STREAM_TABLE where the call's second table is the
// longer one): launch(first, n, Tb, grid) fills the call's own table for worlds [first, first + n), if it has one, and launches.
template <typename Launch> static int table_launches(int table, rem2d_world *const *worlds, int n_worlds, Launch launch) {
    HIP_TRY(hipSetDevice(worlds[0]->cfg.device));
    for (int first = 0; first < n_worlds; first += table) {
        CtlTable Tb;
        const int n = std::min(table, n_worlds - first);
        const unsigned blocks = control_table(Tb, worlds, first, n), per = CTL_THREADS / WAVE;
        launch(first, n, Tb, dim3((blocks + per - 1) / per));
        HIP_TRY(hipGetLastError());
    }
    return REM2D_OK;
}
// The launches of a kernel that writes rows of max_bodies columns in population order: observe, and the topology table of
// include/rem2d_modular.h, whose kernels take the same arguments.
template <typename Kernel, typename T>
static int rows_launch(Kernel kernel, rem2d_world *const *worlds, int n_worlds, int max_bodies, T *out_dev, long long out_rows, hipStream_t st) {
    return table_launches(CTL_TABLE, worlds, n_worlds, [&](int, int, const CtlTable &Tb, dim3 grid) {
        hipLaunchKernelGGL(kernel, grid, dim3(CTL_THREADS), 0, st, Tb, max_bodies, out_dev, out_rows);
    });
}
static int observe_launch(rem2d_world *const *worlds, int n_worlds, int max_bodies, float *out_dev, long long out_rows, hipStream_t st) {
    return rows_launch(rem2d_observe_kernel, worlds, n_worlds, max_bodies, out_dev, out_rows, st);
}
static int control_launch(rem2d_world *const *worlds, int n_worlds, int mode, const double *values_dev, int max_bodies, long long n_rows,
                          const unsigned char *mask_dev, hipStream_t st) {
    return table_launches(CTL_TABLE, worlds, n_worlds, [&](int, int, const CtlTable &Tb, dim3 grid) {
        hipLaunchKernelGGL(rem2d_control_kernel, grid, dim3(CTL_THREADS), 0, st, Tb, mode, values_dev, max_bodies, n_rows, mask_dev);
    });
}
static int buffer_given(const std::string &p, const void *buffer_dev) {
    return buffer_dev ? REM2D_OK : fail(REM2D_E_INVALID, p + "NULL device pointer");
}
// What observe and control refuse, in their order.
static int table_call_ok(const std::string &p, rem2d_world *const *worlds, int32_t n_worlds, const void *buffer_dev, int32_t max_bodies,
                         int64_t rows) {
    OK_TRY(worlds_given(p, worlds, n_worlds));
    OK_TRY(buffer_given(p, buffer_dev));
    OK_TRY(max_bodies_ok(p, max_bodies));
    OK_TRY(rows_ok(p, rows));
    return worlds_ready(p, worlds, n_worlds);
}
extern "C" int rem2d_worlds_observe(rem2d_world *const *worlds, int32_t n_worlds, int32_t max_bodies, float *out_dev, int64_t out_rows,
                                    void *stream) {
    OK_TRY(table_call_ok("observe: ", worlds, n_worlds, out_dev, max_bodies, out_rows));
    return observe_launch(worlds, n_worlds, max_bodies, out_dev, out_rows, (hipStream_t)stream);
}
extern "C" int rem2d_worlds_control(rem2d_world *const *worlds, int32_t n_worlds, int32_t mode, const double *values_dev,
                                    int32_t max_bodies, int64_t n_rows, const uint8_t *mask_dev, void *stream) {
    if (mode != REM2D_CTRL_TARGET && mode != REM2D_CTRL_PARAMS) return fail(REM2D_E_INVALID, "control: unknown mode " + std::to_string(mode));
    OK_TRY(table_call_ok("control: ", worlds, n_worlds, values_dev, max_bodies, n_rows));
    return control_launch(worlds, n_worlds, mode, values_dev, max_bodies, n_rows, mask_dev, (hipStream_t)stream);
}

// ---- terrain range sensing (include/rem2d_sense.h, csrc/rem2d_sense.h) ----
extern "C" int rem2d_sense_abi_version(void) { return REM2D_SENSE_ABI_VERSION; }
static int sense_launch(rem2d_world *const *worlds, int n_worlds, const double *ray_offsets_dev, int n_rays, float *frac_dev, int *hit_dev,
                        long long rows, hipStream_t st) {
    return table_launches(CTL_TABLE, worlds, n_worlds, [&](int first, int n, const CtlTable &Tb, dim3 grid) {
        SenseTable Ts;
        memset(&Ts, 0, sizeof(Ts));
        for (int i = 0; i < n; ++i) {
            const Terrain &T = worlds[first + i]->T; // (flx is the start of the 20 planes rem2d_world_set_terrain uploads)
            Ts.t[i].base = T.flx;
            Ts.t[i].nEdge = T.nEdge; Ts.t[i].nPoly = T.nPoly;
            Ts.t[i].x0 = T.x0; Ts.t[i].invPitch = T.invPitch;
        }
        hipLaunchKernelGGL(rem2d_sense_kernel, grid, dim3(CTL_THREADS), 0, st, Tb, Ts, ray_offsets_dev, n_rays, frac_dev, hit_dev, rows);
    });
}
extern "C" int rem2d_worlds_sense(rem2d_world *const *worlds, int32_t n_worlds, const double *ray_offsets_dev, int32_t n_rays,
                                  float *frac_dev, int32_t *hit_dev, int64_t rows, void *stream) {
    // (arguments first, worlds after: nothing is dereferenced before it has been checked)
    const std::string p = "sense: ";
    OK_TRY(worlds_given(p, worlds, n_worlds));
    OK_TRY(buffer_given(p, ray_offsets_dev));
    OK_TRY(buffer_given(p, frac_dev));
    if (n_rays < 1 || n_rays > REM2D_SENSE_MAX_RAYS)
        return fail(REM2D_E_INVALID, p + "n_rays must be 1.." + std::to_string(REM2D_SENSE_MAX_RAYS) + ", not " + std::to_string(n_rays));
    OK_TRY(rows_ok(p, rows));
    OK_TRY(worlds_present(p, worlds, n_worlds));
    for (int32_t i = 0; i < n_worlds; ++i) {
        OK_TRY(world_fits(p, worlds[i], worlds[0]));
        OK_TRY(world_terrain(p, worlds[i]));
        OK_TRY(world_reset(p, worlds[i]));
    }
    return sense_launch(worlds, n_worlds, ray_offsets_dev, n_rays, frac_dev, (int *)hit_dev, rows, (hipStream_t)stream);
}

// ---- device policies (include/rem2d_policy.h, csrc/rem2d_policy.h) ----
extern "C" int rem2d_policy_abi_version(void) { return REM2D_POLICY_ABI_VERSION; }
// Checks a policy descriptor; `what` prefixes the message.  Nothing it points to is read.
static int policy_ok(const char *what, const rem2d_policy *p) {
    const std::string s = std::string(what) + ": ";
    if (!p) return fail(REM2D_E_INVALID, s + "NULL policy");
    if (p->max_bodies < 1 || p->max_bodies > REM2D_CONTROL_MAX_BODIES)
        return fail(REM2D_E_INVALID, s + "max_bodies must be 1.." + std::to_string(REM2D_CONTROL_MAX_BODIES) + ", not " + std::to_string(p->max_bodies));
    if (p->n_rays < 0 || p->n_rays > REM2D_SENSE_MAX_RAYS)
        return fail(REM2D_E_INVALID, s + "n_rays must be 0.." + std::to_string(REM2D_SENSE_MAX_RAYS) + ", not " + std::to_string(p->n_rays));
    if (p->hidden < 1 || p->hidden > REM2D_POLICY_MAX_HIDDEN)
        return fail(REM2D_E_INVALID, s + "hidden must be 1.." + std::to_string(REM2D_POLICY_MAX_HIDDEN) + ", not " + std::to_string(p->hidden));
    if (p->d != REM2D_OBS_HEAD + REM2D_OBS_BODY * p->max_bodies + p->n_rays)
        return fail(REM2D_E_INVALID, s + "d must be 8 + 6 max_bodies + n_rays = " +
                                         std::to_string(REM2D_OBS_HEAD + REM2D_OBS_BODY * p->max_bodies + p->n_rays) + ", not " + std::to_string(p->d));
    if (p->activation != REM2D_POLICY_SOFTSIGN && p->activation != REM2D_POLICY_RELU)
        return fail(REM2D_E_INVALID, s + "unknown activation " + std::to_string(p->activation));
    if (p->n_sets < 1) return fail(REM2D_E_INVALID, s + "n_sets must be at least 1");
    if (p->n_rows < 0) return fail(REM2D_E_INVALID, s + "negative row count");
    if (!p->w1 || !p->b1 || !p->w2 || !p->b2 || !p->obs || !p->targets || !p->valid || (p->n_rays > 0 && !p->frac))
        return fail(REM2D_E_INVALID, s + "NULL device pointer");
    if (!p->index && (int64_t)p->n_sets != p->n_rows)
        return fail(REM2D_E_INVALID, s + "without an index n_sets must be n_rows (" + std::to_string(p->n_sets) + " sets, " +
                                         std::to_string(p->n_rows) + " rows)");
    return REM2D_OK;
}
static unsigned pow2_at_least(unsigned v) {
    unsigned p = 1;
    while (p < v) p <<= 1;
    return p;
}
// The two families of forward kernels as types, for the one launcher below: Args is the first kernel argument, kernel<V1, V2, NORM>()
// the instantiation.  rem2d_recurrent.h comes after rem2d_policy.h, so both are known here.
struct PolicyKernels {
    typedef PolicyArgs Args;
    template <int V1, int V2, bool NORM> static auto kernel() { return rem2d_policy_forward_kernel<V1, V2, NORM>; }
};
struct RecurrentKernels {
    typedef RecurrentArgs Args;
    template <int V1, int V2, bool NORM> static auto kernel() { return rem2d_recurrent_forward_kernel<V1, V2, NORM>; }
};
// The forward pass of a checked descriptor on `st`, feed-forward or recurrent, plain (Nm = PolNoNorm) or normalised (PolNorm,
// include/rem2d_obsnorm.h): one launch shape.  A is the family's zeroed argument struct, P the PolicyArgs in it; `what` names the
// family in the one refusal that is left to the launch.
template <typename Kernels, bool NORM>
static int forward_launch(const char *what, const rem2d_policy *p, typename Kernels::Args &A, PolicyArgs &P,
                          const typename PolNormArg<NORM>::type &nm, hipStream_t st) {
    if (p->n_rows == 0) return REM2D_OK;
    P.w1 = p->w1; P.b1 = p->b1; P.w2 = p->w2; P.b2 = p->b2;
    P.index = p->index; P.rowMask = p->row_mask;
    P.obs = p->obs; P.frac = p->frac; P.targets = p->targets; P.valid = p->valid;
    P.nRows = p->n_rows;
    P.D = p->d; P.MB = p->max_bodies; P.R = p->n_rays; P.H = p->hidden; P.G = p->n_sets; P.act = p->activation;
    P.scale = p->scale;
    // 16-byte loads where a weight row is whole float4s and its base is aligned (the sets' strides D H and H MB then are too)
    const bool v1 = p->hidden % 4 == 0 && (uintptr_t)p->w1 % 16 == 0;
    const bool v2 = p->max_bodies % 4 == 0 && (uintptr_t)p->w2 % 16 == 0;
    const unsigned need = std::max((unsigned)(p->hidden + (v1 ? 3 : 0)) / (v1 ? 4u : 1u), (unsigned)(p->max_bodies + (v2 ? 3 : 0)) / (v2 ? 4u : 1u));
    const unsigned lpr = std::min((unsigned)WAVE, std::max((unsigned)POL_MIN_LPR, pow2_at_least(need)));
    P.lpr = (int)lpr;
    const unsigned rpw = WAVE / lpr;
    const long long blocks = (p->n_rows + rpw - 1) / rpw;
    if (blocks > 0x7fffffffLL) return fail(REM2D_E_INVALID, std::string(what) + ": too many rows for one launch");
    const size_t lds = (size_t)rpw * (size_t)(p->d + p->hidden) * sizeof(float);
    const auto kernel = v1 ? (v2 ? Kernels::template kernel<4, 4, NORM>() : Kernels::template kernel<4, 1, NORM>())
                           : (v2 ? Kernels::template kernel<1, 4, NORM>() : Kernels::template kernel<1, 1, NORM>());
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(WAVE), lds, st, A, nm);
    HIP_TRY(hipGetLastError());
    return REM2D_OK;
}
template <typename Kernels>
static int forward_launch(const char *what, const rem2d_policy *p, typename Kernels::Args &A, PolicyArgs &P, const PolNorm *nm, hipStream_t st) {
    return nm ? forward_launch<Kernels, true>(what, p, A, P, *nm, st) : forward_launch<Kernels, false>(what, p, A, P, PolNoNorm(), st);
}
static int policy_launch(const rem2d_policy *p, hipStream_t st, const PolNorm *nm = nullptr) {
    PolicyArgs A;
    memset(&A, 0, sizeof(A));
    return forward_launch<PolicyKernels>("policy", p, A, A, nm, st);
}
extern "C" int rem2d_policy_forward(const rem2d_policy *p, void *stream) {
    OK_TRY(policy_ok("policy", p));
    return policy_launch(p, (hipStream_t)stream);
}
// What rem2d_worlds_act, _act_recurrent, _act_normed and _act_modular do once their descriptors are checked: the ray offsets and the worlds
// (everything before the first launch), then observe, sense, `forward()` and control on `st`, launches only.
template <typename Forward>
static int act(const std::string &s, rem2d_world *const *worlds, int32_t n_worlds, const rem2d_policy *p, const double *ray_offsets_dev,
               hipStream_t st, Forward forward) {
    if (p->n_rays > 0 && !ray_offsets_dev) return fail(REM2D_E_INVALID, s + "NULL device pointer (ray offsets)");
    OK_TRY(worlds_present(s, worlds, n_worlds));
    OK_TRY(worlds_ready(s, worlds, n_worlds));
    if (p->n_rays > 0)
        for (int32_t i = 0; i < n_worlds; ++i) OK_TRY(world_terrain(s, worlds[i]));
    OK_TRY(observe_launch(worlds, n_worlds, p->max_bodies, const_cast<float *>(p->obs), p->n_rows, st));
    if (p->n_rays > 0) OK_TRY(sense_launch(worlds, n_worlds, ray_offsets_dev, p->n_rays, const_cast<float *>(p->frac), nullptr, p->n_rows, st));
    OK_TRY(forward());
    return control_launch(worlds, n_worlds, REM2D_CTRL_TARGET, p->targets, p->max_bodies, p->n_rows, p->valid, st);
}
extern "C" int rem2d_worlds_act(rem2d_world *const *worlds, int32_t n_worlds, const rem2d_policy *p, const double *ray_offsets_dev,
                                void *stream) {
    OK_TRY(worlds_given("act: ", worlds, n_worlds));
    OK_TRY(policy_ok("act", p));
    return act("act: ", worlds, n_worlds, p, ray_offsets_dev, (hipStream_t)stream, [&] { return policy_launch(p, (hipStream_t)stream); });
}

// ---- recurrent device policies (include/rem2d_recurrent.h, csrc/rem2d_recurrent.h) ----
extern "C" int rem2d_recurrent_abi_version(void) { return REM2D_RECURRENT_ABI_VERSION; }
// Checks a recurrent descriptor; `what` prefixes the message.  Nothing it points to is read.  policy_ok checks everything of q->p
// but d, whose rule here counts the context words.
static int recurrent_ok(const char *what, const rem2d_recurrent *q) {
    const std::string s = std::string(what) + ": ";
    if (!q) return fail(REM2D_E_INVALID, s + "NULL recurrent policy");
    rem2d_policy c = q->p;
    c.d = REM2D_OBS_HEAD + REM2D_OBS_BODY * c.max_bodies + c.n_rays; // (what policy_ok wants of a feed-forward set: checked below instead)
    const int rc = policy_ok(what, &c);
    if (rc != REM2D_OK) return rc;
    if (q->context < 1 || q->context > q->p.hidden)
        return fail(REM2D_E_INVALID, s + "context must be 1..hidden (" + std::to_string(q->p.hidden) + "), not " + std::to_string(q->context));
    if (q->p.n_rays + q->context > REM2D_SENSE_MAX_RAYS)
        return fail(REM2D_E_INVALID, s + "n_rays + context must be at most " + std::to_string(REM2D_SENSE_MAX_RAYS) + ", not " +
                                         std::to_string(q->p.n_rays) + " + " + std::to_string(q->context));
    if (q->p.d != c.d + q->context)
        return fail(REM2D_E_INVALID, s + "d must be 8 + 6 max_bodies + n_rays + context = " + std::to_string(c.d + q->context) + ", not " +
                                         std::to_string(q->p.d));
    if (q->reserved != 0) return fail(REM2D_E_INVALID, s + "reserved must be 0, not " + std::to_string(q->reserved));
    if (!q->memory) return fail(REM2D_E_INVALID, s + "NULL device pointer (memory)");
    return REM2D_OK;
}
static int recurrent_launch(const rem2d_recurrent *q, hipStream_t st, const PolNorm *nm = nullptr) {
    RecurrentArgs Q;
    memset(&Q, 0, sizeof(Q));
    Q.memory = q->memory; Q.reset = q->reset; Q.K = q->context;
    return forward_launch<RecurrentKernels>("recurrent", &q->p, Q, Q.P, nm, st);
}
extern "C" int rem2d_recurrent_forward(const rem2d_recurrent *q, void *stream) {
    OK_TRY(recurrent_ok("recurrent", q));
    return recurrent_launch(q, (hipStream_t)stream);
}
extern "C" int rem2d_worlds_act_recurrent(rem2d_world *const *worlds, int32_t n_worlds, const rem2d_recurrent *q,
                                          const double *ray_offsets_dev, void *stream) {
    OK_TRY(worlds_given("act_recurrent: ", worlds, n_worlds));
    OK_TRY(recurrent_ok("act_recurrent", q));
    return act("act_recurrent: ", worlds, n_worlds, &q->p, ray_offsets_dev, (hipStream_t)stream,
               [&] { return recurrent_launch(q, (hipStream_t)stream); });
}

// ---- modular device policies (include/rem2d_modular.h, csrc/rem2d_modular.h) ----
extern "C" int rem2d_modular_abi_version(void) { return REM2D_MODULAR_ABI_VERSION; }
static_assert(REM2D_MODULAR_MAX_INPUTS == REM2D_SENSE_MAX_RAYS, "a modular set is an ordinary set of R + 2 + 2 K ray inputs");
extern "C" int rem2d_worlds_topology(rem2d_world *const *worlds, int32_t n_worlds, const rem2d_topology *t) {
    const std::string p = "topology: ";
    OK_TRY(worlds_given(p, worlds, n_worlds));
    if (!t) return fail(REM2D_E_INVALID, p + "NULL descriptor");
    if (t->reserved != 0) return fail(REM2D_E_INVALID, p + "reserved must be 0, not " + std::to_string(t->reserved));
    OK_TRY(table_call_ok(p, worlds, n_worlds, t->out, t->max_bodies, t->out_rows));
    return rows_launch(rem2d_topology_kernel, worlds, n_worlds, (int)t->max_bodies, (int *)t->out, (long long)t->out_rows, (hipStream_t)t->stream);
}
// Checks a modular descriptor; `what` prefixes the message.  Nothing it points to is read.  policy_ok checks everything of q->p but
// d, whose rule here is the per-body one.
static int modular_ok(const char *what, const rem2d_modular *q) {
    const std::string s = std::string(what) + ": ";
    if (!q) return fail(REM2D_E_INVALID, s + "NULL modular policy");
    rem2d_policy c = q->p;
    c.d = REM2D_OBS_HEAD + REM2D_OBS_BODY * c.max_bodies + c.n_rays; // (what policy_ok wants of a feed-forward set: checked below instead)
    const int rc = policy_ok(what, &c);
    if (rc != REM2D_OK) return rc;
    if (q->messages < 1 || q->messages > q->p.hidden)
        return fail(REM2D_E_INVALID, s + "messages must be 1..hidden (" + std::to_string(q->p.hidden) + "), not " + std::to_string(q->messages));
    if (q->p.n_rays + 2 + 2 * (int64_t)q->messages > REM2D_MODULAR_MAX_INPUTS)
        return fail(REM2D_E_INVALID, s + "n_rays + 2 + 2 messages must be at most " + std::to_string(REM2D_MODULAR_MAX_INPUTS) + ", not " +
                                         std::to_string(q->p.n_rays) + " + 2 + 2 * " + std::to_string(q->messages));
    if (q->rounds < 1 || q->rounds > REM2D_MODULAR_MAX_ROUNDS)
        return fail(REM2D_E_INVALID, s + "rounds must be 1.." + std::to_string(REM2D_MODULAR_MAX_ROUNDS) + ", not " + std::to_string(q->rounds));
    const int dm = REM2D_OBS_HEAD + REM2D_OBS_BODY + q->p.n_rays + 2 + 2 * q->messages;
    if (q->p.d != dm)
        return fail(REM2D_E_INVALID, s + "d must be 8 + 6 + n_rays + 2 + 2 messages = " + std::to_string(dm) + ", not " + std::to_string(q->p.d));
    if (!q->topo) return fail(REM2D_E_INVALID, s + "NULL device pointer (topo)");
    if (!q->memory) return fail(REM2D_E_INVALID, s + "NULL device pointer (memory)");
    return REM2D_OK;
}
// lanes per body for n units of which a lane owns v: a power of two, MOD_MIN_LPB .. 64
static int modular_lpb(int n, int v) { return (int)std::min((unsigned)WAVE, std::max((unsigned)MOD_MIN_LPB, pow2_at_least((unsigned)((n + v - 1) / v)))); }
static int modular_launch(const rem2d_modular *q) {
    const rem2d_policy *p = &q->p;
    if (p->n_rows == 0) return REM2D_OK;
    if (p->n_rows > 0x7fffffffLL) return fail(REM2D_E_INVALID, "modular: too many rows for one launch");
    ModularArgs Q;
    memset(&Q, 0, sizeof(Q));
    PolicyArgs &P = Q.P;
    P.w1 = p->w1; P.b1 = p->b1; P.w2 = p->w2; P.b2 = p->b2;
    P.index = p->index; P.rowMask = p->row_mask;
    P.obs = p->obs; P.frac = p->frac; P.targets = p->targets; P.valid = p->valid;
    P.nRows = p->n_rows;
    P.D = p->d; P.MB = p->max_bodies; P.R = p->n_rays; P.H = p->hidden; P.G = p->n_sets; P.act = p->activation;
    P.scale = p->scale;
    Q.topo = q->topo; Q.memory = q->memory; Q.reset = q->reset; Q.K = q->messages; Q.rounds = q->rounds;
    const bool v4 = p->hidden % 4 == 0; // (the weights are read from LDS, whose base is aligned)
    const int V = v4 ? 4 : 1;
    P.lpr = modular_lpb(p->hidden, V);
    Q.lpbK = modular_lpb(std::min(p->hidden, (q->messages + V - 1) / V * V), V);
    const size_t lds = (size_t)modular_lds(P.D, P.H, P.MB, P.R, Q.K, P.lpr, Q.lpbK).words * sizeof(float);
    if (lds > 65536) return fail(REM2D_E_INVALID, "modular: the row does not fit the LDS of a workgroup"); // (no shape within the limits gets here)
    if (v4) hipLaunchKernelGGL(rem2d_modular_forward_kernel<4>, dim3((unsigned)p->n_rows), dim3(WAVE), lds, (hipStream_t)q->stream, Q);
    else hipLaunchKernelGGL(rem2d_modular_forward_kernel<1>, dim3((unsigned)p->n_rows), dim3(WAVE), lds, (hipStream_t)q->stream, Q);
    HIP_TRY(hipGetLastError());
    return REM2D_OK;
}
extern "C" int rem2d_modular_forward(const rem2d_modular *q) {
    OK_TRY(modular_ok("modular", q));
    return modular_launch(q);
}
extern "C" int rem2d_worlds_act_modular(rem2d_world *const *worlds, int32_t n_worlds, const rem2d_modular *q, const double *ray_offsets_dev) {
    OK_TRY(worlds_given("act_modular: ", worlds, n_worlds));
    OK_TRY(modular_ok("act_modular", q));
    return act("act_modular: ", worlds, n_worlds, &q->p, ray_offsets_dev, (hipStream_t)q->stream, [&] { return modular_launch(q); });
}

// ---- episode boundaries (include/rem2d_episode.h, csrc/rem2d_episode.h) ----
extern "C" int rem2d_episode_abi_version(void) { return REM2D_EPISODE_ABI_VERSION; }
static_assert(sizeof(CtlTable) + sizeof(EpTable) + sizeof(EpArgs) + 16 <= 4096, "rem2d_reset_where_kernel: kernel arguments within the 4 KB kernarg limit");
static bool morph_complete(const rem2d_morph *m) {
    return m->shape && m->hx && m->hy && m->x && m->y && m->angle && m->parent && m->jround && m->ax && m->ay && m->bx && m->by &&
           m->torque && m->lower && m->upper && m->amp && m->phase && m->freq && m->offset && m->istate;
}
// What reset_where and refill refuse of their morphologies and of `when`, each in the call's own place.
static int morphs_complete(const std::string &p, const rem2d_morph *morphs, int32_t n_worlds) {
    for (int32_t i = 0; i < n_worlds; ++i)
        if (!morph_complete(morphs + i)) return fail(REM2D_E_INVALID, p + "morphology " + std::to_string(i) + " has NULL arrays");
    return REM2D_OK;
}
static int when_bits_ok(const std::string &p, uint32_t when) {
    if (when & ~(uint32_t)(REM2D_WHEN_DONE | REM2D_WHEN_FROZEN | REM2D_WHEN_STEPS))
        return fail(REM2D_E_INVALID, p + "unknown bits in `when` (" + std::to_string(when) + ")");
    return REM2D_OK;
}
static int when_steps_ok(const std::string &p, uint32_t when, int32_t max_steps) {
    if ((when & REM2D_WHEN_STEPS) && max_steps <= 0)
        return fail(REM2D_E_INVALID, p + "REM2D_WHEN_STEPS needs max_steps > 0, not " + std::to_string(max_steps));
    return REM2D_OK;
}
extern "C" int rem2d_worlds_reset_where(rem2d_world *const *worlds, const rem2d_morph *morphs, int32_t n_worlds, const uint8_t *mask_dev,
                                        uint32_t when, int32_t max_steps, const rem2d_episode_out *out, int64_t n_rows, void *stream) {
    // (arguments first, worlds after, everything before the first launch)
    const std::string p = "reset_where: ";
    OK_TRY(worlds_given(p, worlds, n_worlds));
    if (!morphs) return fail(REM2D_E_INVALID, p + "NULL morphologies");
    OK_TRY(when_bits_ok(p, when));
    OK_TRY(when_steps_ok(p, when, max_steps));
    if (!mask_dev && when == 0)
        return fail(REM2D_E_INVALID, p + "no mask and no condition would reset every creature (that is rem2d_world_reset)");
    OK_TRY(rows_ok(p, n_rows));
    OK_TRY(worlds_present(p, worlds, n_worlds));
    OK_TRY(morphs_complete(p, morphs, n_worlds));
    for (int32_t i = 0; i < n_worlds; ++i) {
        OK_TRY(world_fits(p, worlds[i], worlds[0]));
        OK_TRY(world_reset(p, worlds[i]));
    }
    EpArgs A;
    memset(&A, 0, sizeof(A));
    A.mask = mask_dev;
    if (out) A.out = *out;
    A.nRows = n_rows;
    A.when = when;
    A.maxSteps = max_steps;
    return table_launches(CTL_TABLE, worlds, n_worlds, [&](int first, int n, const CtlTable &Tb, dim3 grid) {
        EpTable Te;
        memset(&Te, 0, sizeof(Te));
        for (int i = 0; i < n; ++i) {
            Te.w[i].M = morphs[first + i];
            Te.w[i].env4 = worlds[first + i]->S.env4;
        }
        hipLaunchKernelGGL(rem2d_reset_where_kernel, grid, dim3(CTL_THREADS), 0, (hipStream_t)stream, Tb, Te, A);
    });
}

// ---- streaming evaluation (include/rem2d_stream.h, csrc/rem2d_stream.h) ----
extern "C" int rem2d_stream_abi_version(void) { return REM2D_STREAM_ABI_VERSION; }
static_assert(sizeof(CtlTable) + sizeof(StTable) + sizeof(StArgs) + 16 <= 4096, "rem2d_refill_kernel: kernel arguments within the 4 KB kernarg limit");
extern "C" int rem2d_worlds_refill(rem2d_world *const *worlds, const rem2d_morph *morphs, int32_t n_worlds, const rem2d_feed *feeds,
                                   int32_t *occupant_dev, uint32_t when, int32_t max_steps, const rem2d_stream_out *out, int64_t n_ids,
                                   int64_t n_rows, void *stream) {
    // (arguments first, worlds after, everything before the first launch)
    const std::string p = "refill: ";
    OK_TRY(worlds_given(p, worlds, n_worlds));
    if (!morphs) return fail(REM2D_E_INVALID, p + "NULL morphologies");
    if (!feeds) return fail(REM2D_E_INVALID, p + "NULL feeds");
    if (!occupant_dev) return fail(REM2D_E_INVALID, p + "NULL occupant array");
    OK_TRY(when_bits_ok(p, when));
    if (when == 0) return fail(REM2D_E_INVALID, p + "no condition (`when` == 0): nobody's episode could end");
    OK_TRY(when_steps_ok(p, when, max_steps));
    OK_TRY(rows_ok(p, n_rows));
    if (n_ids < 0) return fail(REM2D_E_INVALID, p + "negative id count");
    OK_TRY(worlds_present(p, worlds, n_worlds));
    OK_TRY(morphs_complete(p, morphs, n_worlds));
    for (int32_t i = 0; i < n_worlds; ++i) {
        const rem2d_feed *f = feeds + i;
        if (f->count < 0) return fail(REM2D_E_INVALID, p + "feed " + std::to_string(i) + " has a negative count");
        if (!f->cursor) return fail(REM2D_E_INVALID, p + "feed " + std::to_string(i) + " has no cursor");
        if (f->count > 0 && (!morph_complete(&f->M) || !f->id))
            return fail(REM2D_E_INVALID, p + "feed " + std::to_string(i) + " has pending creatures and NULL arrays");
    }
    for (int32_t i = 0; i < n_worlds; ++i) {
        const rem2d_world *w = worlds[i];
        OK_TRY(world_fits(p, w, worlds[0]));
        if (feeds[i].lanes != w->cfg.lanes)
            return fail(REM2D_E_INVALID, p + "feed " + std::to_string(i) + " holds creatures of " + std::to_string(feeds[i].lanes) +
                                             " lanes, its world creatures of " + std::to_string(w->cfg.lanes));
    }
    for (int32_t i = 0; i < n_worlds; ++i) { // (the tile shape and the reset after every world's lanes: a loop of their own)
        const rem2d_world *w = worlds[i];
        if (!tile_shape(w->tileShape).flex)
            return fail(REM2D_E_STATE, p + "world " + std::to_string(i) + " is on the static tile shape " + std::to_string(w->tileShape) +
                                           ": the tile table of shapes 0 and 4 is planned from the joints of the creatures in it, "
                                           "so its slots cannot take other creatures (use a flexible shape: 1, 2 or 3)");
        OK_TRY(world_reset(p, w));
    }
    StArgs A;
    memset(&A, 0, sizeof(A));
    A.occupant = occupant_dev;
    if (out) A.out = *out;
    A.nIds = n_ids;
    A.nRows = n_rows;
    A.when = when;
    A.maxSteps = max_steps;
    return table_launches(STREAM_TABLE, worlds, n_worlds, [&](int first, int n, const CtlTable &Tb, dim3 grid) {
        StTable Ts;
        memset(&Ts, 0, sizeof(Ts));
        for (int i = 0; i < n; ++i) {
            const rem2d_feed &f = feeds[first + i];
            Ts.w[i].M = morphs[first + i];
            Ts.w[i].env4 = worlds[first + i]->S.env4;
            Ts.w[i].F = f.M;
            Ts.w[i].id = f.id;
            Ts.w[i].cursor = f.cursor;
            Ts.w[i].count = f.count;
        }
        hipLaunchKernelGGL(rem2d_refill_kernel, grid, dim3(CTL_THREADS), 0, (hipStream_t)stream, Tb, Ts, A);
    });
}

// ---- what the search tiers below share on the host: net shapes, buffer spans, scratch, launches ----
// The w1 / b1 / w2 / b2 members of a descriptor whose names begin with `pre` (which may be empty): the initialiser of an array of four.
#define QUAD(e, pre) {(e)->pre##w1, (e)->pre##b1, (e)->pre##w2, (e)->pre##b2}
static const char *const kNet[4] = {"w1", "b1", "w2", "b2"};
// The three refusals of a net's shape; `s` prefixes the message.
static int net_ok(const std::string &s, int d, int hidden, int max_bodies) {
    if (max_bodies < 1 || max_bodies > REM2D_CONTROL_MAX_BODIES)
        return fail(REM2D_E_INVALID, s + "max_bodies must be 1.." + std::to_string(REM2D_CONTROL_MAX_BODIES) + ", not " + std::to_string(max_bodies));
    if (hidden < 1 || hidden > REM2D_POLICY_MAX_HIDDEN)
        return fail(REM2D_E_INVALID, s + "hidden must be 1.." + std::to_string(REM2D_POLICY_MAX_HIDDEN) + ", not " + std::to_string(hidden));
    const int d0 = REM2D_OBS_HEAD + REM2D_OBS_BODY * max_bodies;
    if (d < d0 || d > d0 + REM2D_SENSE_MAX_RAYS)
        return fail(REM2D_E_INVALID, s + "d must be 8 + 6 max_bodies + R with R in 0.." + std::to_string(REM2D_SENSE_MAX_RAYS) + " (" +
                                         std::to_string(d0) + ".." + std::to_string(d0 + REM2D_SENSE_MAX_RAYS) + "), not " + std::to_string(d));
    return REM2D_OK;
}
// Words of one set of w1, b1, w2, b2 of a net whose shape is good.
struct Net {
    size_t len[4];
    Net(int d, int hidden, int max_bodies) : len{(size_t)d * (size_t)hidden, (size_t)hidden, (size_t)hidden * (size_t)max_bodies, (size_t)max_bodies} {}
};
// A buffer as a validator sees it; a message names it `pre` `name`.
struct Span {
    uintptr_t at;
    size_t bytes;
    const char *pre, *name;
};
static Span span(const void *p, size_t bytes, const char *name) { return {(uintptr_t)p, bytes, "", name}; }
// The four arrays of a family, `sets` sets each, into to[0 .. 3]; false where one of them is NULL.
static bool add4(Span *to, const float *const (&p)[4], const char *pre, size_t sets, const Net &N) {
    for (int k = 0; k < 4; ++k) {
        if (!p[k]) return false;
        to[k] = {(uintptr_t)p[k], sets * N.len[k] * sizeof(float), pre, kNet[k]};
    }
    return true;
}
static bool meet(const Span &a, const Span &b) { return a.at < b.at + b.bytes && b.at < a.at + a.bytes; }
// Refuses the first of a[0] with b[0], a[0] with b[1], ..., a[1] with b[0], ... that meet.  Which pairs a tier hands in is the tier's rule.
static int apart(const std::string &s, const Span *a, int na, const Span *b, int nb) {
    for (int i = 0; i < na; ++i)
        for (int j = 0; j < nb; ++j)
            if (meet(a[i], b[j])) {
                std::string m;
                m.reserve(s.size() + 64); // the whole message in one allocation
                m.append(s);
                if (*a[i].pre) m.append(a[i].pre);
                m.append(a[i].name).append(" overlaps ");
                if (*b[j].pre) m.append(b[j].pre);
                return fail(REM2D_E_INVALID, m.append(b[j].name));
            }
    return REM2D_OK;
}
static int scratch_ok(const std::string &s, const void *scratch, uint64_t have, size_t need) {
    if (!scratch) return fail(REM2D_E_INVALID, s + "NULL device pointer (scratch): " + std::to_string(need) + " bytes are needed");
    if ((uintptr_t)scratch % 8 != 0) return fail(REM2D_E_INVALID, s + "scratch must be 8-byte aligned");
    if (have < (uint64_t)need) return fail(REM2D_E_INVALID, s + "scratch holds " + std::to_string(have) + " bytes, " + std::to_string(need) + " are needed");
    return REM2D_OK;
}
// 16-byte accesses where a set of the array is whole float4s and both bases are aligned (every set's base then is too)
static int vec_ok(size_t len, const void *a, const void *b) { return len % 4 == 0 && (uintptr_t)a % 16 == 0 && (uintptr_t)b % 16 == 0; }
static void seed_keys(uint64_t seed, unsigned &key0, unsigned &key1) {
    key0 = (unsigned)(seed & 0xffffffffull);
    key1 = (unsigned)(seed >> 32);
}
template <typename T, typename U> static void set4(T (&to)[4], U *const (&from)[4]) {
    for (int k = 0; k < 4; ++k) to[k] = from[k];
}
// len, src, dst and vec of a kernel that copies or varies sets of `src` into `dst` (EvolveArgs, CvLine).
template <typename A> static void quads(A &X, const Net &N, const float *const (&src)[4], float *const (&dst)[4]) {
    for (int k = 0; k < 4; ++k) {
        X.len[k] = (int)N.len[k];
        X.src[k] = src[k];
        X.dst[k] = dst[k];
        X.vec[k] = vec_ok(N.len[k], src[k], dst[k]);
    }
}
enum { ES_MAX_GRID = 1 << 24 }; // workgroups of one launch; what lies beyond goes into further launches
// `items` workgroups of one wavefront of one kernel, ES_MAX_GRID of them per launch, each launch told its first item in `itemBase`
// (a member of `args`).
template <typename K, typename A> static int launch_items(K kernel, long long items, A &args, long long &itemBase, hipStream_t st) {
    for (long long base = 0; base < items; base += ES_MAX_GRID) {
        const long long n = items - base < (long long)ES_MAX_GRID ? items - base : (long long)ES_MAX_GRID;
        itemBase = base;
        hipLaunchKernelGGL(kernel, dim3((unsigned)n), dim3(WAVE), 0, st, args);
        HIP_TRY(hipGetLastError());
    }
    return REM2D_OK;
}
// An insertion into an elite grid on `st`: clear, the tier's key kernel on its own arguments, row, commit.  L holds the rows, the grid
// and the scratch's key | row; the sets of `src` go to `elite`.  (The key kernel's grid is sized by EL_TILE whichever tier's it
// is: the cvt section's static_assert(CV_TILE == EL_TILE) is what allows that.)
template <typename K, typename KA>
static int insert_launch(K key_kernel, const KA &key_args, const ElArgs &L, const Net &N, const float *const (&src)[4], float *const (&elite)[4], hipStream_t st) {
    const long long G = (long long)L.M * (long long)L.S, slots = (long long)L.M * (long long)L.C;
    EvolveArgs E;
    memset(&E, 0, sizeof(E));
    quads(E, N, src, elite);
    hipLaunchKernelGGL(rem2d_elites_clear_kernel, dim3((unsigned)((slots + EL_TILE - 1) / EL_TILE)), dim3(EL_TILE), 0, st, L);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(key_kernel, dim3((unsigned)((G + EL_TILE - 1) / EL_TILE)), dim3(EL_TILE), 0, st, key_args);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(rem2d_elites_row_kernel, dim3((unsigned)((G + EL_TILE - 1) / EL_TILE)), dim3(EL_TILE), 0, st, L);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(rem2d_elites_commit_kernel, dim3((unsigned)slots), dim3(WAVE), 0, st, L, E);
    HIP_TRY(hipGetLastError());
    return REM2D_OK;
}
// An entry point: the tier's check of the descriptor for `stages`, then its launch of them.
template <typename D>
static int run(int (*ok)(const char *, const D *, int), int (*launch)(const D *, int, hipStream_t), const char *what, const D *e, int stages, void *stream) {
    OK_TRY(ok(what, e, stages));
    return launch(e, stages, (hipStream_t)stream);
}

// ---- evolving device policies (include/rem2d_evolve.h, csrc/rem2d_evolve.h) ----
extern "C" int rem2d_evolve_abi_version(void) { return REM2D_EVOLVE_ABI_VERSION; }
enum { EVOLVE_SELECT = 1, EVOLVE_VARY = 2 };
// Checks an evolve descriptor for the calls in `stages`; `what` prefixes the message.  Nothing it points to is read.
static int evolve_ok(const char *what, const rem2d_evolve *e, int stages) {
    const std::string s = std::string(what) + ": ";
    if (!e) return fail(REM2D_E_INVALID, s + "NULL descriptor");
    OK_TRY(net_ok(s, e->d, e->hidden, e->max_bodies));
    if (e->n_sets < 1) return fail(REM2D_E_INVALID, s + "n_sets must be at least 1");
    if (e->group_size < 1 || e->n_sets % e->group_size != 0)
        return fail(REM2D_E_INVALID, s + "group_size must be a divisor of n_sets (" + std::to_string(e->n_sets) + "), not " + std::to_string(e->group_size));
    if (e->tournsize < 1 || e->tournsize > REM2D_EVOLVE_MAX_TOURNSIZE)
        return fail(REM2D_E_INVALID, s + "tournsize must be 1.." + std::to_string(REM2D_EVOLVE_MAX_TOURNSIZE) + ", not " + std::to_string(e->tournsize));
    if (e->elite != 0 && e->elite != 1) return fail(REM2D_E_INVALID, s + "elite must be 0 or 1, not " + std::to_string(e->elite));
    if (e->rate_threshold > (1ull << 32)) return fail(REM2D_E_INVALID, s + "rate_threshold must be at most 2^32");
    if (!e->parent) return fail(REM2D_E_INVALID, s + "NULL device pointer (parent)");
    if ((stages & EVOLVE_SELECT) && !e->fitness) return fail(REM2D_E_INVALID, s + "NULL device pointer (fitness)");
    if (stages & EVOLVE_VARY) {
        const Net N(e->d, e->hidden, e->max_bodies);
        Span src[4], dst[4];
        if (!add4(src, QUAD(e, ), "the parents' ", (size_t)e->n_sets, N) || !add4(dst, QUAD(e, child_), "child_", (size_t)e->n_sets, N))
            return fail(REM2D_E_INVALID, s + "NULL device pointer (weights)");
        OK_TRY(apart(s, dst, 4, src, 4));
    }
    return REM2D_OK;
}
static void evolve_args(EvolveArgs &A, const rem2d_evolve *e) {
    memset(&A, 0, sizeof(A));
    A.fitness = e->fitness;
    quads(A, Net(e->d, e->hidden, e->max_bodies), QUAD(e, ), QUAD(e, child_));
    A.parent = e->parent;
    A.rateThreshold = e->rate_threshold;
    seed_keys(e->seed, A.key0, A.key1); A.generation = e->generation;
    A.G = e->n_sets; A.S = e->group_size; A.T = e->tournsize; A.elite = e->elite;
    A.sigma = e->sigma;
}
// The stages of a checked descriptor on `st`.
static int evolve_launch(const rem2d_evolve *e, int stages, hipStream_t st) {
    EvolveArgs A;
    evolve_args(A, e);
    if (stages & EVOLVE_SELECT) {
        hipLaunchKernelGGL(rem2d_evolve_select_kernel, dim3(((unsigned)e->n_sets + WAVE - 1) / WAVE), dim3(WAVE), 0, st, A);
        HIP_TRY(hipGetLastError());
    }
    if (stages & EVOLVE_VARY) {
        hipLaunchKernelGGL(rem2d_evolve_vary_kernel, dim3((unsigned)e->n_sets), dim3(WAVE), 0, st, A);
        HIP_TRY(hipGetLastError());
    }
    return REM2D_OK;
}
extern "C" int rem2d_policy_select(const rem2d_evolve *e, void *stream) { return run(evolve_ok, evolve_launch, "select", e, EVOLVE_SELECT, stream); }
extern "C" int rem2d_policy_vary(const rem2d_evolve *e, void *stream) { return run(evolve_ok, evolve_launch, "vary", e, EVOLVE_VARY, stream); }
extern "C" int rem2d_policy_evolve(const rem2d_evolve *e, void *stream) { return run(evolve_ok, evolve_launch, "evolve", e, EVOLVE_SELECT | EVOLVE_VARY, stream); }

// ---- an evolution strategy for device policies (include/rem2d_es.h, csrc/rem2d_es.h) ----
extern "C" int rem2d_es_abi_version(void) { return REM2D_ES_ABI_VERSION; }
enum { ES_SAMPLE = 1, ES_SHAPE = 2, ES_UPDATE = 4 };
// The shapes of an es or an snes descriptor: what their checks, the split and the scratch's size read.
struct EsShape {
    int d, hidden, max_bodies, n_means, group_size, pair_chunk;
};
template <typename D> static EsShape es_shape(const D *e) { return {e->d, e->hidden, e->max_bodies, e->n_means, e->group_size, e->pair_chunk}; }
// The split of a block's pairs for shapes that are good: pairs per wavefront and chunks per block.
static void es_split(const EsShape &X, int &pairChunk, int &nChunks) {
    const long long P = X.group_size / 2;
    long long chunk = X.pair_chunk;
    if (chunk == 0) {
        // the library's choice: no split while the blocks alone fill the machine or a block is short; otherwise chunks of at
        // least 64 pairs, as many as bring the launch to about 4096 wavefronts
        const Net N(X.d, X.hidden, X.max_bodies);
        long long W = 0;
        for (int k = 0; k < 4; ++k) W += ((long long)N.len[k] + WAVE - 1) / WAVE;
        const long long waves = W * (long long)X.n_means;
        chunk = P;
        if (waves < 1024 && P > 64) {
            const long long want = (4096 + waves - 1) / waves;
            chunk = (P + want - 1) / want;
            if (chunk < 64) chunk = 64;
        }
    }
    if (chunk > P) chunk = P;
    pairChunk = (int)chunk;
    nChunks = (int)((P + chunk - 1) / chunk);
}
// Checks the shapes es and snes share; `s` prefixes the message.
static int es_shape_ok(const std::string &s, const EsShape &X) {
    OK_TRY(net_ok(s, X.d, X.hidden, X.max_bodies));
    if (X.n_means < 1) return fail(REM2D_E_INVALID, s + "n_means must be at least 1");
    if (X.group_size < 2 || X.group_size % 2 != 0)
        return fail(REM2D_E_INVALID, s + "group_size must be even and at least 2, not " + std::to_string(X.group_size));
    if ((long long)X.n_means * (long long)X.group_size > 2147483647ll)
        return fail(REM2D_E_INVALID, s + "n_means * group_size must be at most 2^31 - 1");
    if (X.pair_chunk < 0) return fail(REM2D_E_INVALID, s + "pair_chunk must be at least 0, not " + std::to_string(X.pair_chunk));
    return REM2D_OK;
}
// Checks the shapes and parameters of an es descriptor; `s` prefixes the message.  No pointer is looked at.
static int es_shapes_ok(const std::string &s, const rem2d_es *e) {
    if (!e) return fail(REM2D_E_INVALID, s + "NULL descriptor");
    OK_TRY(es_shape_ok(s, es_shape(e)));
    if (e->reserved != 0) return fail(REM2D_E_INVALID, s + "reserved must be 0");
    return REM2D_OK;
}
static size_t es_scratch_need(const EsShape &X) {
    int pairChunk, nChunks;
    es_split(X, pairChunk, nChunks);
    if (nChunks == 1) return 0;
    const Net N(X.d, X.hidden, X.max_bodies);
    return (size_t)X.n_means * (size_t)nChunks * (N.len[0] + N.len[1] + N.len[2] + N.len[3]) * sizeof(long long);
}
// Checks an es descriptor for the calls in `stages`.  Nothing it points to is read.
static int es_ok(const char *what, const rem2d_es *e, int stages) {
    const std::string s = std::string(what) + ": ";
    OK_TRY(es_shapes_ok(s, e));
    if ((stages & ES_SHAPE) && !e->fitness) return fail(REM2D_E_INVALID, s + "NULL device pointer (fitness)");
    if ((stages & (ES_SHAPE | ES_UPDATE)) && !e->util) return fail(REM2D_E_INVALID, s + "NULL device pointer (util)");
    const Net N(e->d, e->hidden, e->max_bodies);
    const size_t M = (size_t)e->n_means, G = M * (size_t)e->group_size;
    // each destination against the mean, and against nothing else
    const struct { int stage; const float *p[4]; const char *pre; size_t sets; } outs[2] = {
        {ES_SAMPLE, QUAD(e, child_), "child_", G}, {ES_UPDATE, QUAD(e, new_), "new_", M}};
    Span mean[4], dst[4];
    const bool have = add4(mean, QUAD(e, ), "the mean's ", M, N);
    for (const auto &o : outs) {
        if (!(stages & o.stage)) continue;
        if (!have || !add4(dst, o.p, o.pre, o.sets, N)) return fail(REM2D_E_INVALID, s + "NULL device pointer (weights)");
        OK_TRY(apart(s, dst, 4, mean, 4));
    }
    if (stages & ES_UPDATE) {
        const size_t need = es_scratch_need(es_shape(e));
        if (need != 0) OK_TRY(scratch_ok(s, e->scratch, e->scratch_bytes, need));
    }
    return REM2D_OK;
}
// What es and snes hand their kernels alike, from either descriptor: all of EsArgs but sigma and step.
template <typename D> static void es_args(EsArgs &A, const D *e) {
    memset(&A, 0, sizeof(A));
    A.fitness = e->fitness;
    A.util = e->util;
    set4(A.mean, QUAD(e, )); set4(A.child, QUAD(e, child_)); set4(A.next, QUAD(e, new_));
    A.scratch = (long long *)e->scratch;
    seed_keys(e->seed, A.key0, A.key1); A.generation = e->generation;
    const Net N(e->d, e->hidden, e->max_bodies);
    for (int k = 0; k < 4; ++k) {
        A.len[k] = (int)N.len[k];
        A.vec[k] = vec_ok(N.len[k], A.mean[k], A.child[k]);
        A.slots[k] = (A.len[k] + WAVE - 1) / WAVE;
        A.off[k] = A.E;
        A.W += A.slots[k];
        A.E += A.len[k];
    }
    A.M = e->n_means; A.S = e->group_size;
    es_split(es_shape(e), A.pairChunk, A.nChunks);
}
// The stages of a checked descriptor on `st`.
static int es_launch(const rem2d_es *e, int stages, hipStream_t st) {
    EsArgs A;
    es_args(A, e);
    A.sigma = e->sigma; A.step = e->step;
    const long long G = (long long)A.M * (long long)A.S;
    if (stages & ES_SAMPLE) OK_TRY(launch_items(rem2d_es_sample_kernel, G / 2, A, A.itemBase, st));
    if (stages & ES_SHAPE) {
        A.itemBase = 0; // (ceil(G / ES_TILE) < 2^23 workgroups: one launch)
        hipLaunchKernelGGL(rem2d_es_shape_kernel, dim3((unsigned)((G + ES_TILE - 1) / ES_TILE)), dim3(ES_TILE), 0, st, A);
        HIP_TRY(hipGetLastError());
    }
    if (stages & ES_UPDATE) {
        OK_TRY(launch_items(rem2d_es_update_kernel, (long long)A.M * (long long)A.nChunks * (long long)A.W, A, A.itemBase, st));
        if (A.nChunks > 1) OK_TRY(launch_items(rem2d_es_finish_kernel, (long long)A.M * (long long)A.W, A, A.itemBase, st));
    }
    return REM2D_OK;
}
extern "C" int64_t rem2d_es_scratch_bytes(const rem2d_es *e) {
    OK_TRY(es_shapes_ok("es_scratch_bytes: ", e));
    return (int64_t)es_scratch_need(es_shape(e));
}
extern "C" int rem2d_es_sample(const rem2d_es *e, void *stream) { return run(es_ok, es_launch, "es_sample", e, ES_SAMPLE, stream); }
extern "C" int rem2d_es_shape(const rem2d_es *e, void *stream) { return run(es_ok, es_launch, "es_shape", e, ES_SHAPE, stream); }
extern "C" int rem2d_es_update(const rem2d_es *e, void *stream) { return run(es_ok, es_launch, "es_update", e, ES_UPDATE, stream); }
extern "C" int rem2d_es_step(const rem2d_es *e, void *stream) { return run(es_ok, es_launch, "es_step", e, ES_SHAPE | ES_UPDATE, stream); }

// ---- an adaptive evolution strategy for device policies (include/rem2d_snes.h, csrc/rem2d_snes.h) ----
extern "C" int rem2d_snes_abi_version(void) { return REM2D_SNES_ABI_VERSION; }
enum { SN_SAMPLE = 1, SN_SHAPE = 2, SN_UPDATE = 4 };
// Checks the shapes and parameters of an snes descriptor; `s` prefixes the message.  No pointer is looked at.
static int sn_shapes_ok(const std::string &s, const rem2d_snes *e) {
    if (!e) return fail(REM2D_E_INVALID, s + "NULL descriptor");
    OK_TRY(es_shape_ok(s, es_shape(e)));
    if (e->group_size > REM2D_SNES_MAX_GROUP)
        return fail(REM2D_E_INVALID, s + "group_size must be at most " + std::to_string(REM2D_SNES_MAX_GROUP) + ", not " + std::to_string(e->group_size));
    if (e->flags & ~(REM2D_SNES_ADAM | REM2D_SNES_NATURAL)) return fail(REM2D_E_INVALID, s + "unknown bits in flags: " + std::to_string(e->flags));
    return REM2D_OK;
}
static size_t sn_scratch_need(const rem2d_snes *e) { return 2 * es_scratch_need(es_shape(e)); } // two int64 per element per chunk
// Checks an snes descriptor for the calls in `stages`.  Nothing it points to is read.
static int sn_ok(const char *what, const rem2d_snes *e, int stages) {
    const std::string s = std::string(what) + ": ";
    OK_TRY(sn_shapes_ok(s, e));
    const bool adam = (e->flags & REM2D_SNES_ADAM) != 0;
    if ((stages & SN_SHAPE) && !e->fitness) return fail(REM2D_E_INVALID, s + "NULL device pointer (fitness)");
    if ((stages & (SN_SHAPE | SN_UPDATE)) && !e->util) return fail(REM2D_E_INVALID, s + "NULL device pointer (util)");
    const Net N(e->d, e->hidden, e->max_bodies);
    const size_t M = (size_t)e->n_means, G = M * (size_t)e->group_size;
    // what the calls read and what they write, in the order the overlaps are looked for
    Span in[4 * 4 + 2], out[5 * 4 + 1];
    int ni = 8, no = 0;
    bool all = add4(in, QUAD(e, ), "the mean's ", M, N) && add4(in + 4, QUAD(e, sigma_), "sigma_", M, N);
    if (stages & SN_SAMPLE) {
        all = all && add4(out, QUAD(e, child_), "child_", G, N);
        no = 4;
    }
    if (stages & SN_UPDATE) {
        all = all && add4(out + no, QUAD(e, new_), "new_", M, N) && add4(out + no + 4, QUAD(e, new_sigma_), "new_sigma_", M, N);
        no += 8;
        if (adam) {
            all = all && add4(in + 8, QUAD(e, m1_), "m1_", M, N) && add4(in + 12, QUAD(e, m2_), "m2_", M, N) &&
                  add4(out + no, QUAD(e, new_m1_), "new_m1_", M, N) && add4(out + no + 4, QUAD(e, new_m2_), "new_m2_", M, N);
            ni = 16;
            no += 8;
        }
    }
    if (!all) return fail(REM2D_E_INVALID, s + "NULL device pointer (weights or state)");
    if (stages & SN_UPDATE) {
        if (!(e->sigma_min > 0.0f) || !(e->sigma_min <= e->sigma_max) || !std::isfinite(e->sigma_min) || !std::isfinite(e->sigma_max))
            return fail(REM2D_E_INVALID, s + "sigma_min and sigma_max must be finite with 0 < sigma_min <= sigma_max");
        in[ni++] = span(e->util, G * sizeof(int32_t), "util");
        const size_t need = sn_scratch_need(e);
        if (need != 0) {
            OK_TRY(scratch_ok(s, e->scratch, e->scratch_bytes, need));
            out[no++] = span(e->scratch, need, "scratch");
        }
    }
    if (stages & SN_SHAPE) in[ni++] = span(e->fitness, G * sizeof(double), "fitness");
    // each output against every input, then against the outputs before it
    for (int i = 0; i < no; ++i) {
        OK_TRY(apart(s, out + i, 1, in, ni));
        OK_TRY(apart(s, out + i, 1, out, i));
    }
    return REM2D_OK;
}
// The stages of a checked descriptor on `st`.
static int sn_launch(const rem2d_snes *e, int stages, hipStream_t st) {
    SnArgs B;
    memset(&B, 0, sizeof(B));
    es_args(B.es, e);
    set4(B.sigma, QUAD(e, sigma_)); set4(B.m1, QUAD(e, m1_)); set4(B.m2, QUAD(e, m2_));
    set4(B.nextSigma, QUAD(e, new_sigma_)); set4(B.nextM1, QUAD(e, new_m1_)); set4(B.nextM2, QUAD(e, new_m2_));
    for (int k = 0; k < 4; ++k) B.es.vec[k] = B.es.vec[k] && (uintptr_t)B.sigma[k] % 16 == 0; // the third base of the sample
    B.flags = e->flags;
    B.mstep = e->mstep; B.sstep = e->sstep; B.beta1 = e->beta1; B.omb1 = e->omb1; B.beta2 = e->beta2; B.omb2 = e->omb2;
    B.alpha = e->alpha; B.eps = e->eps; B.sigmaMin = e->sigma_min; B.sigmaMax = e->sigma_max;
    const EsArgs &A = B.es;
    const long long G = (long long)A.M * (long long)A.S;
    if (stages & SN_SAMPLE) OK_TRY(launch_items(rem2d_snes_sample_kernel, G / 2, B, B.es.itemBase, st));
    if (stages & SN_SHAPE) {
        B.es.itemBase = 0;
        hipLaunchKernelGGL(rem2d_es_shape_kernel, dim3((unsigned)((G + ES_TILE - 1) / ES_TILE)), dim3(ES_TILE), 0, st, B.es);
        HIP_TRY(hipGetLastError());
    }
    if (stages & SN_UPDATE) {
        OK_TRY(launch_items(rem2d_snes_update_kernel, (long long)A.M * (long long)A.nChunks * (long long)A.W, B, B.es.itemBase, st));
        if (A.nChunks > 1) OK_TRY(launch_items(rem2d_snes_finish_kernel, (long long)A.M * (long long)A.W, B, B.es.itemBase, st));
    }
    return REM2D_OK;
}
extern "C" int64_t rem2d_snes_scratch_bytes(const rem2d_snes *e) {
    OK_TRY(sn_shapes_ok("snes_scratch_bytes: ", e));
    return (int64_t)sn_scratch_need(e);
}
extern "C" int rem2d_snes_sample(const rem2d_snes *e, void *stream) { return run(sn_ok, sn_launch, "snes_sample", e, SN_SAMPLE, stream); }
extern "C" int rem2d_snes_update(const rem2d_snes *e, void *stream) { return run(sn_ok, sn_launch, "snes_update", e, SN_UPDATE, stream); }
extern "C" int rem2d_snes_step(const rem2d_snes *e, void *stream) { return run(sn_ok, sn_launch, "snes_step", e, SN_SHAPE | SN_UPDATE, stream); }

// ---- behavioural novelty (include/rem2d_novelty.h, csrc/rem2d_novelty.h) ----
extern "C" int rem2d_novelty_abi_version(void) { return REM2D_NOVELTY_ABI_VERSION; }
static_assert(sizeof(CtlTable) + sizeof(NvTable) + 32 <= 4096, "rem2d_describe_kernel: kernel arguments within the 4 KB kernarg limit");
static_assert(2 * REM2D_NOVELTY_MAX_SAMPLES <= REM2D_NOVELTY_MAX_WIDTH, "a descriptor row is a score row");
extern "C" int rem2d_worlds_describe(rem2d_world *const *worlds, int32_t n_worlds, int32_t period, int32_t n_samples, float *out_dev,
                                     int64_t out_rows, void *stream) {
    if (period < 1) return fail(REM2D_E_INVALID, "describe: period must be at least 1, not " + std::to_string(period));
    if (n_samples < 1 || n_samples > REM2D_NOVELTY_MAX_SAMPLES)
        return fail(REM2D_E_INVALID, "describe: n_samples must be 1.." + std::to_string(REM2D_NOVELTY_MAX_SAMPLES) + ", not " + std::to_string(n_samples));
    const std::string p = "describe: "; // (observe's refusals without a max_bodies)
    OK_TRY(worlds_given(p, worlds, n_worlds));
    OK_TRY(buffer_given(p, out_dev));
    OK_TRY(rows_ok(p, out_rows));
    OK_TRY(worlds_ready(p, worlds, n_worlds));
    return table_launches(CTL_TABLE, worlds, n_worlds, [&](int first, int n, const CtlTable &Tb, dim3 grid) {
        NvTable Te;
        memset(&Te, 0, sizeof(Te));
        for (int i = 0; i < n; ++i) Te.env4[i] = worlds[first + i]->S.env4;
        hipLaunchKernelGGL(rem2d_describe_kernel, grid, dim3(CTL_THREADS), 0, (hipStream_t)stream, Tb, Te, (int)period, (int)n_samples, out_dev,
                           (long long)out_rows);
    });
}
enum { NV_SCORE = 1, NV_ADD = 2 };
// Checks a novelty descriptor for the calls in `stages`.  Nothing it points to is read.
static int nv_ok(const char *what, const rem2d_novelty *n, int stages) {
    const std::string s = std::string(what) + ": ";
    if (!n) return fail(REM2D_E_INVALID, s + "NULL descriptor");
    if (n->width < 1 || n->width > REM2D_NOVELTY_MAX_WIDTH)
        return fail(REM2D_E_INVALID, s + "width must be 1.." + std::to_string(REM2D_NOVELTY_MAX_WIDTH) + ", not " + std::to_string(n->width));
    if (n->n_rows < 1) return fail(REM2D_E_INVALID, s + "n_rows must be at least 1, not " + std::to_string(n->n_rows));
    if (n->group_size < 1 || n->n_rows % n->group_size != 0)
        return fail(REM2D_E_INVALID, s + "group_size must be at least 1 and divide n_rows (" + std::to_string(n->n_rows) + "), not " + std::to_string(n->group_size));
    if (n->k < 1 || n->k > REM2D_NOVELTY_MAX_K)
        return fail(REM2D_E_INVALID, s + "k must be 1.." + std::to_string(REM2D_NOVELTY_MAX_K) + ", not " + std::to_string(n->k));
    if (n->capacity < 0) return fail(REM2D_E_INVALID, s + "capacity must be at least 0, not " + std::to_string(n->capacity));
    if (n->add_threshold > (1ull << 32)) return fail(REM2D_E_INVALID, s + "add_threshold must be at most 2^32");
    if (n->reserved != 0) return fail(REM2D_E_INVALID, s + "reserved must be 0");
    if (!n->desc) return fail(REM2D_E_INVALID, s + "NULL device pointer (desc)");
    if (!n->total) return fail(REM2D_E_INVALID, s + "NULL device pointer (total)");
    if (n->capacity > 0 && !n->archive) return fail(REM2D_E_INVALID, s + "NULL device pointer (archive)");
    if ((stages & NV_SCORE) && !n->novelty) return fail(REM2D_E_INVALID, s + "NULL device pointer (novelty)");
    const size_t G = (size_t)n->n_rows, M = (size_t)(n->n_rows / n->group_size);
    const Span desc = span(n->desc, G * (size_t)n->width * sizeof(float), "desc");
    Span out[2];
    int no = 0;
    if (n->capacity > 0) out[no++] = span(n->archive, M * (size_t)n->capacity * (size_t)n->width * sizeof(float), "archive");
    if (stages & NV_SCORE) out[no++] = span(n->novelty, G * sizeof(double), "novelty");
    return apart(s, out, no, &desc, 1);
}
template <int BP> static void nv_launch_score(const NvArgs &A, int kp, dim3 grid, hipStream_t st) {
    if (kp <= 2) hipLaunchKernelGGL((rem2d_novelty_score_kernel<BP, 2>), grid, dim3(NV_TILE), 0, st, A);
    else if (kp <= 8) hipLaunchKernelGGL((rem2d_novelty_score_kernel<BP, 8>), grid, dim3(NV_TILE), 0, st, A);
    else if (kp <= 16) hipLaunchKernelGGL((rem2d_novelty_score_kernel<BP, 16>), grid, dim3(NV_TILE), 0, st, A);
    else hipLaunchKernelGGL((rem2d_novelty_score_kernel<BP, 32>), grid, dim3(NV_TILE), 0, st, A);
}
// The stages of a checked descriptor on `st`.
static int nv_launch(const rem2d_novelty *n, int stages, hipStream_t st) {
    NvArgs A;
    memset(&A, 0, sizeof(A));
    A.desc = n->desc; A.archive = n->archive; A.total = (long long *)n->total; A.novelty = n->novelty; A.mask = n->add_mask;
    A.threshold = n->add_threshold;
    seed_keys(n->seed, A.key0, A.key1); A.generation = n->generation;
    A.B = n->width; A.G = n->n_rows; A.S = n->group_size; A.k = n->k; A.cap = n->capacity;
    if (stages & NV_SCORE) {
        const dim3 grid((unsigned)(((long long)A.G + NV_TILE - 1) / NV_TILE));
        if (A.B <= 2) nv_launch_score<2>(A, A.k, grid, st);
        else if (A.B <= 4) nv_launch_score<4>(A, A.k, grid, st);
        else if (A.B <= 8) nv_launch_score<8>(A, A.k, grid, st);
        else if (A.B <= 16) nv_launch_score<16>(A, A.k, grid, st);
        else nv_launch_score<32>(A, A.k, grid, st);
        HIP_TRY(hipGetLastError());
    }
    if (stages & NV_ADD) {
        hipLaunchKernelGGL(rem2d_novelty_add_kernel, dim3((unsigned)(A.G / A.S)), dim3(NV_TILE), 0, st, A);
        HIP_TRY(hipGetLastError());
    }
    return REM2D_OK;
}
extern "C" int rem2d_novelty_score(const rem2d_novelty *n, void *stream) { return run(nv_ok, nv_launch, "novelty_score", n, NV_SCORE, stream); }
extern "C" int rem2d_novelty_add(const rem2d_novelty *n, void *stream) { return run(nv_ok, nv_launch, "novelty_add", n, NV_ADD, stream); }
extern "C" int rem2d_novelty_step(const rem2d_novelty *n, void *stream) { return run(nv_ok, nv_launch, "novelty_step", n, NV_SCORE | NV_ADD, stream); }

// ---- MAP-Elites for device policies (include/rem2d_elites.h, csrc/rem2d_elites.h) ----
extern "C" int rem2d_elites_abi_version(void) { return REM2D_ELITES_ABI_VERSION; }
static_assert(REM2D_ELITES_MAX_WIDTH == REM2D_NOVELTY_MAX_WIDTH, "an elite's descriptor row is a score row");
static_assert(REM2D_ELITES_MAX_WIDTH <= WAVE, "rem2d_elites_commit_kernel: a lane per descriptor word");
enum { EL_INSERT = 1, EL_SAMPLE = 2, EL_VARY = 4 };
static bool el_finite(float v) { return std::isfinite(v); }
// Checks the shapes and parameters of an elites descriptor; `s` prefixes the message.  No pointer is looked at.
static int el_shapes_ok(const std::string &s, const rem2d_elites *e) {
    if (!e) return fail(REM2D_E_INVALID, s + "NULL descriptor");
    OK_TRY(net_ok(s, e->d, e->hidden, e->max_bodies));
    if (e->width < 1 || e->width > REM2D_ELITES_MAX_WIDTH)
        return fail(REM2D_E_INVALID, s + "width must be 1.." + std::to_string(REM2D_ELITES_MAX_WIDTH) + ", not " + std::to_string(e->width));
    if (e->n_blocks < 1) return fail(REM2D_E_INVALID, s + "n_blocks must be at least 1, not " + std::to_string(e->n_blocks));
    if (e->n_dims < 1 || e->n_dims > REM2D_ELITES_MAX_DIMS)
        return fail(REM2D_E_INVALID, s + "n_dims must be 1.." + std::to_string(REM2D_ELITES_MAX_DIMS) + ", not " + std::to_string(e->n_dims));
    long long cells = 1;
    for (int i = 0; i < e->n_dims; ++i) {
        const std::string at = "[" + std::to_string(i) + "]";
        if (e->word[i] < 0 || e->word[i] >= e->width)
            return fail(REM2D_E_INVALID, s + "word" + at + " must be 0.." + std::to_string(e->width - 1) + ", not " + std::to_string(e->word[i]));
        if (e->bins[i] < 1) return fail(REM2D_E_INVALID, s + "bins" + at + " must be at least 1, not " + std::to_string(e->bins[i]));
        cells *= (long long)e->bins[i];
        if (cells > (long long)REM2D_ELITES_MAX_CELLS)
            return fail(REM2D_E_INVALID, s + "the product of bins must be at most " + std::to_string(REM2D_ELITES_MAX_CELLS) + " cells");
        if (!el_finite(e->lo[i])) return fail(REM2D_E_INVALID, s + "lo" + at + " must be finite");
        if (!el_finite(e->inv[i]) || !(e->inv[i] > 0.0f)) return fail(REM2D_E_INVALID, s + "inv" + at + " must be finite and positive");
    }
    if ((long long)e->n_blocks * cells > 2147483647ll) return fail(REM2D_E_INVALID, s + "n_blocks times the cells must be at most 2^31 - 1");
    if (e->rate_threshold > (1ull << 32)) return fail(REM2D_E_INVALID, s + "rate_threshold must be at most 2^32");
    if (e->reserved != 0) return fail(REM2D_E_INVALID, s + "reserved must be 0");
    return REM2D_OK;
}
static long long el_cells(const rem2d_elites *e) {
    long long cells = 1;
    for (int i = 0; i < e->n_dims; ++i) cells *= (long long)e->bins[i];
    return cells;
}
static size_t el_scratch_need(const rem2d_elites *e) {
    return (size_t)e->n_blocks * (size_t)el_cells(e) * (sizeof(unsigned long long) + sizeof(int));
}
// The buffers of a grid of `slots` cells (an elites or a cvt descriptor's) in the order both tiers test them: elite_fitness,
// elite_desc, count, then the elite arrays in to[3 .. 6]; false where one of those is NULL.
template <typename D> static bool grid_spans(Span (&to)[7], const D *e, size_t slots, const Net &N) {
    to[0] = span(e->elite_fitness, slots * sizeof(double), "elite_fitness");
    to[1] = span(e->elite_desc, slots * (size_t)e->width * sizeof(float), "elite_desc");
    to[2] = span(e->count, slots * sizeof(int), "count");
    return add4(to + 3, QUAD(e, elite_), "elite_", slots, N);
}
// Checks an elites descriptor for the calls in `stages`.  Nothing it points to is read.
static int el_ok(const char *what, const rem2d_elites *e, int stages) {
    const std::string s = std::string(what) + ": ";
    OK_TRY(el_shapes_ok(s, e));
    const size_t slots = (size_t)e->n_blocks * (size_t)el_cells(e);
    const Net N(e->d, e->hidden, e->max_bodies);
    Span grid[7], *const elite = grid + 3;
    const bool elites = grid_spans(grid, e, slots, N);
    if (stages & EL_INSERT) {
        if (e->group_size < 1) return fail(REM2D_E_INVALID, s + "group_size must be at least 1, not " + std::to_string(e->group_size));
        if ((long long)e->n_blocks * (long long)e->group_size > 2147483647ll)
            return fail(REM2D_E_INVALID, s + "n_blocks * group_size must be at most 2^31 - 1");
    }
    if (stages & (EL_SAMPLE | EL_VARY)) {
        if (e->n_children < 1 || e->n_children % e->n_blocks != 0)
            return fail(REM2D_E_INVALID, s + "n_children must be a positive multiple of n_blocks (" + std::to_string(e->n_blocks) + "), not " + std::to_string(e->n_children));
    }
    if (!e->count) return fail(REM2D_E_INVALID, s + "NULL device pointer (count)");
    if (stages & EL_INSERT) {
        const size_t G = (size_t)e->n_blocks * (size_t)e->group_size;
        if (!e->desc) return fail(REM2D_E_INVALID, s + "NULL device pointer (desc)");
        if (!e->fitness) return fail(REM2D_E_INVALID, s + "NULL device pointer (fitness)");
        if (!e->elite_fitness) return fail(REM2D_E_INVALID, s + "NULL device pointer (elite_fitness)");
        if (!e->elite_desc) return fail(REM2D_E_INVALID, s + "NULL device pointer (elite_desc)");
        if (!e->cell) return fail(REM2D_E_INVALID, s + "NULL device pointer (cell)");
        if (!e->winner) return fail(REM2D_E_INVALID, s + "NULL device pointer (winner)");
        Span src[4];
        if (!add4(src, QUAD(e, ), "the evaluated sets' ", G, N) || !elites) return fail(REM2D_E_INVALID, s + "NULL device pointer (weights)");
        const Span desc = span(e->desc, G * (size_t)e->width * sizeof(float), "desc");
        OK_TRY(apart(s, &desc, 1, grid, 7));
        OK_TRY(apart(s, elite, 4, src, 4));
    }
    if (stages & (EL_SAMPLE | EL_VARY)) {
        if (!e->parent) return fail(REM2D_E_INVALID, s + "NULL device pointer (parent)");
        if (!e->n_filled) return fail(REM2D_E_INVALID, s + "NULL device pointer (n_filled)");
    }
    if (stages & EL_VARY) {
        Span dst[4];
        if (!add4(dst, QUAD(e, child_), "child_", (size_t)e->n_children, N) || !elites) return fail(REM2D_E_INVALID, s + "NULL device pointer (weights)");
        OK_TRY(apart(s, dst, 4, elite, 4));
    }
    return scratch_ok(s, e->scratch, e->scratch_bytes, el_scratch_need(e));
}
// The stages of a checked descriptor on `st`.
static int el_launch(const rem2d_elites *e, int stages, hipStream_t st) {
    ElArgs A;
    memset(&A, 0, sizeof(A));
    const long long C = el_cells(e), slots = (long long)e->n_blocks * C;
    const Net N(e->d, e->hidden, e->max_bodies);
    A.desc = e->desc; A.fitness = e->fitness; A.mask = e->mask;
    A.eliteFitness = e->elite_fitness; A.eliteDesc = e->elite_desc;
    A.count = e->count; A.cell = e->cell; A.winner = e->winner; A.parent = e->parent; A.nFilled = e->n_filled;
    A.key = (unsigned long long *)e->scratch;
    A.row = (int *)(A.key + slots);
    for (int i = 0; i < e->n_dims; ++i) { A.lo[i] = e->lo[i]; A.inv[i] = e->inv[i]; A.word[i] = e->word[i]; A.bins[i] = e->bins[i]; }
    seed_keys(e->seed, A.key0, A.key1); A.generation = e->generation;
    A.nDims = e->n_dims; A.B = e->width; A.M = e->n_blocks; A.S = e->group_size; A.C = (int)C;
    if (stages & EL_INSERT) OK_TRY(insert_launch(rem2d_elites_key_kernel, A, A, N, QUAD(e, ), QUAD(e, elite_), st));
    if (stages & EL_SAMPLE) {
        A.perBlock = e->n_children / e->n_blocks;
        hipLaunchKernelGGL(rem2d_elites_sample_kernel, dim3((unsigned)A.M), dim3(EL_TILE), 0, st, A);
        HIP_TRY(hipGetLastError());
    }
    if (stages & EL_VARY) {
        // rem2d_evolve_vary_kernel as it is: the elite arrays are the "parents", M C bounds p, a workgroup per child
        EvolveArgs E;
        memset(&E, 0, sizeof(E));
        quads(E, N, QUAD(e, elite_), QUAD(e, child_));
        E.parent = e->parent;
        E.rateThreshold = e->rate_threshold;
        E.key0 = A.key0; E.key1 = A.key1; E.generation = e->generation;
        E.G = (int)slots; E.S = 1; E.T = 1; E.elite = 0;
        E.sigma = e->sigma;
        hipLaunchKernelGGL(rem2d_evolve_vary_kernel, dim3((unsigned)e->n_children), dim3(WAVE), 0, st, E);
        HIP_TRY(hipGetLastError());
    }
    return REM2D_OK;
}
extern "C" int64_t rem2d_elites_scratch_bytes(const rem2d_elites *e) {
    OK_TRY(el_shapes_ok("elites_scratch_bytes: ", e));
    return (int64_t)el_scratch_need(e);
}
extern "C" int rem2d_elites_insert(const rem2d_elites *e, void *stream) { return run(el_ok, el_launch, "elites_insert", e, EL_INSERT, stream); }
extern "C" int rem2d_elites_sample(const rem2d_elites *e, void *stream) { return run(el_ok, el_launch, "elites_sample", e, EL_SAMPLE, stream); }
extern "C" int rem2d_elites_emit(const rem2d_elites *e, void *stream) { return run(el_ok, el_launch, "elites_emit", e, EL_SAMPLE | EL_VARY, stream); }

// ---- Centroid archives and the line emitter (include/rem2d_cvt.h, csrc/rem2d_cvt.h) ----
extern "C" int rem2d_cvt_abi_version(void) { return REM2D_CVT_ABI_VERSION; }
static_assert(REM2D_CVT_MAX_WIDTH == REM2D_ELITES_MAX_WIDTH && REM2D_CVT_MAX_CELLS == REM2D_ELITES_MAX_CELLS, "a centroid archive is an elite grid of one dimension");
static_assert(CV_TILE == EL_TILE, "the insertion mixes the two tiers' launches");
enum { CV_ASSIGN = 1, CV_INSERT = 2, CV_LINE = 4 };
// Checks what the assignment looks at of the shapes; `s` prefixes the message.  No pointer is looked at.
static int cv_assign_shapes_ok(const std::string &s, const rem2d_cvt *v) {
    if (!v) return fail(REM2D_E_INVALID, s + "NULL descriptor");
    if (v->width < 1 || v->width > REM2D_CVT_MAX_WIDTH)
        return fail(REM2D_E_INVALID, s + "width must be 1.." + std::to_string(REM2D_CVT_MAX_WIDTH) + ", not " + std::to_string(v->width));
    if (v->n_cells < 1 || v->n_cells > REM2D_CVT_MAX_CELLS)
        return fail(REM2D_E_INVALID, s + "n_cells must be 1.." + std::to_string(REM2D_CVT_MAX_CELLS) + ", not " + std::to_string(v->n_cells));
    if (v->splits < 0 || v->splits > REM2D_CVT_MAX_SPLITS)
        return fail(REM2D_E_INVALID, s + "splits must be 0.." + std::to_string(REM2D_CVT_MAX_SPLITS) + ", not " + std::to_string(v->splits));
    if (v->reserved != 0) return fail(REM2D_E_INVALID, s + "reserved must be 0");
    return REM2D_OK;
}
// Checks the shapes and parameters of a centroid descriptor.  No pointer is looked at.
static int cv_shapes_ok(const std::string &s, const rem2d_cvt *v) {
    OK_TRY(cv_assign_shapes_ok(s, v));
    OK_TRY(net_ok(s, v->d, v->hidden, v->max_bodies));
    if (v->n_blocks < 1) return fail(REM2D_E_INVALID, s + "n_blocks must be at least 1, not " + std::to_string(v->n_blocks));
    if ((long long)v->n_blocks * (long long)v->n_cells > 2147483647ll) return fail(REM2D_E_INVALID, s + "n_blocks times n_cells must be at most 2^31 - 1");
    if (v->group_size > 0 && (long long)v->n_blocks * (long long)v->group_size > 2147483647ll)
        return fail(REM2D_E_INVALID, s + "n_blocks * group_size must be at most 2^31 - 1");
    if (!el_finite(v->sigma_iso) || !el_finite(v->sigma_line)) return fail(REM2D_E_INVALID, s + "sigma_iso and sigma_line must be finite");
    return REM2D_OK;
}
static size_t cv_slots(const rem2d_cvt *v) { return (size_t)v->n_blocks * (size_t)v->n_cells; }
// Checks a centroid descriptor for the call `stage`.  Nothing it points to is read.
static int cv_ok(const char *what, const rem2d_cvt *v, int stage) {
    const std::string s = std::string(what) + ": ";
    OK_TRY(stage == CV_ASSIGN ? cv_assign_shapes_ok(s, v) : cv_shapes_ok(s, v));
    size_t need = 0;
    if (stage == CV_ASSIGN) {
        if (v->n_rows < 1) return fail(REM2D_E_INVALID, s + "n_rows must be at least 1, not " + std::to_string(v->n_rows));
        need = (size_t)v->n_rows * sizeof(unsigned long long);
    } else {
        need = cv_slots(v) * (sizeof(unsigned long long) + sizeof(int));
    }
    const size_t slots = stage == CV_ASSIGN ? 0 : cv_slots(v);
    const Net N(v->d, v->hidden, v->max_bodies); // (the assignment, which does not check them, reads none of it)
    Span grid[7], *const elite = grid + 3;
    const bool elites = grid_spans(grid, v, slots, N);
    if (stage == CV_INSERT) {
        if (v->group_size < 1) return fail(REM2D_E_INVALID, s + "group_size must be at least 1, not " + std::to_string(v->group_size));
        need += (size_t)v->n_blocks * (size_t)v->group_size * sizeof(unsigned long long);
    }
    if (stage == CV_LINE) {
        if (v->n_children < 1 || v->n_children % v->n_blocks != 0)
            return fail(REM2D_E_INVALID, s + "n_children must be a positive multiple of n_blocks (" + std::to_string(v->n_blocks) + "), not " + std::to_string(v->n_children));
    }
    if (stage & (CV_ASSIGN | CV_INSERT)) {
        const size_t rows = stage == CV_ASSIGN ? (size_t)v->n_rows : (size_t)v->n_blocks * (size_t)v->group_size;
        if (!v->centroids) return fail(REM2D_E_INVALID, s + "NULL device pointer (centroids)");
        if (!v->desc) return fail(REM2D_E_INVALID, s + "NULL device pointer (desc)");
        if (!v->cell) return fail(REM2D_E_INVALID, s + "NULL device pointer (cell)");
        const Span in[2] = {span(v->desc, rows * (size_t)v->width * sizeof(float), "desc"),
                            span(v->centroids, (size_t)v->n_cells * (size_t)v->width * sizeof(float), "centroids")};
        const Span out[2] = {span(v->cell, rows * sizeof(int), "cell"), span(v->dist, rows * sizeof(float), "dist")};
        OK_TRY(apart(s, in, 2, out, v->dist ? 2 : 1));
        if (stage == CV_INSERT) {
            if (!v->fitness) return fail(REM2D_E_INVALID, s + "NULL device pointer (fitness)");
            if (!v->elite_fitness) return fail(REM2D_E_INVALID, s + "NULL device pointer (elite_fitness)");
            if (!v->elite_desc) return fail(REM2D_E_INVALID, s + "NULL device pointer (elite_desc)");
            if (!v->count) return fail(REM2D_E_INVALID, s + "NULL device pointer (count)");
            if (!v->winner) return fail(REM2D_E_INVALID, s + "NULL device pointer (winner)");
            Span src[4];
            if (!add4(src, QUAD(v, ), "the evaluated sets' ", rows, N) || !elites) return fail(REM2D_E_INVALID, s + "NULL device pointer (weights)");
            OK_TRY(apart(s, in, 2, grid, 7));
            OK_TRY(apart(s, elite, 4, src, 4));
        }
    }
    if (stage == CV_LINE) {
        if (!v->count) return fail(REM2D_E_INVALID, s + "NULL device pointer (count)");
        if (!v->parent) return fail(REM2D_E_INVALID, s + "NULL device pointer (parent)");
        if (!v->parent2) return fail(REM2D_E_INVALID, s + "NULL device pointer (parent2)");
        if (!v->n_filled) return fail(REM2D_E_INVALID, s + "NULL device pointer (n_filled)");
        Span dst[4];
        if (!add4(dst, QUAD(v, child_), "child_", (size_t)v->n_children, N) || !elites) return fail(REM2D_E_INVALID, s + "NULL device pointer (weights)");
        OK_TRY(apart(s, dst, 4, elite, 4));
    }
    return scratch_ok(s, v->scratch, v->scratch_bytes, need);
}
// The assignment of `rows` rows on `st`: A.best is set.  One launch, or clear + split assign + read-out.
static int cv_assign_launch(CvArgs &A, long long rows, int splits, hipStream_t st) {
    const unsigned tiles = (unsigned)((rows + CV_TILE - 1) / CV_TILE);
    const int chunks = (A.C + CV_TILE - 1) / CV_TILE; // a split below one LDS tile of centroids gains nothing
    if (splits == 0) // the library's choice: about 1024 workgroups where the rows alone give fewer than 512
        splits = tiles >= 512u ? 1 : std::min(chunks, (int)((1024u + tiles - 1u) / tiles));
    A.rows = rows;
    A.splits = splits;
    A.per = (A.C + splits - 1) / splits;
    if (splits > 1) {
        hipLaunchKernelGGL(rem2d_cvt_clear_kernel, dim3(tiles), dim3(CV_TILE), 0, st, A);
        HIP_TRY(hipGetLastError());
    }
    const dim3 grid(tiles, (unsigned)splits);
    if (A.B <= 4) hipLaunchKernelGGL(rem2d_cvt_assign_kernel<4>, grid, dim3(CV_TILE), 0, st, A);
    else if (A.B <= 8) hipLaunchKernelGGL(rem2d_cvt_assign_kernel<8>, grid, dim3(CV_TILE), 0, st, A);
    else if (A.B <= 16) hipLaunchKernelGGL(rem2d_cvt_assign_kernel<16>, grid, dim3(CV_TILE), 0, st, A);
    else hipLaunchKernelGGL(rem2d_cvt_assign_kernel<32>, grid, dim3(CV_TILE), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (splits > 1) {
        hipLaunchKernelGGL(rem2d_cvt_finish_kernel, dim3(tiles), dim3(CV_TILE), 0, st, A);
        HIP_TRY(hipGetLastError());
    }
    return REM2D_OK;
}
// The call `stage` of a checked descriptor on `st`, its stream.
static int cv_launch(const rem2d_cvt *v, int stage, hipStream_t st) {
    CvArgs A;
    memset(&A, 0, sizeof(A));
    A.desc = v->desc; A.centroids = v->centroids; A.cell = v->cell; A.dist = v->dist;
    A.B = v->width; A.C = v->n_cells;
    A.best = (unsigned long long *)v->scratch;
    if (stage == CV_ASSIGN) return cv_assign_launch(A, (long long)v->n_rows, v->splits, st);
    const long long slots = (long long)cv_slots(v);
    A.fitness = v->fitness; A.mask = v->mask; A.count = v->count;
    A.parent = v->parent; A.parent2 = v->parent2; A.nFilled = v->n_filled;
    seed_keys(v->seed, A.key0, A.key1); A.generation = v->generation;
    A.M = v->n_blocks; A.S = v->group_size;
    const Net N(v->d, v->hidden, v->max_bodies);
    if (stage == CV_INSERT) {
        // scratch: best[G] | key[M C] | row[M C]; the elites' kernels see the last two as they see their own scratch
        const long long G = (long long)A.M * (long long)A.S;
        A.key = A.best + G;
        OK_TRY(cv_assign_launch(A, G, v->splits, st));
        ElArgs L;
        memset(&L, 0, sizeof(L));
        L.desc = v->desc; L.fitness = v->fitness; L.mask = v->mask;
        L.eliteFitness = v->elite_fitness; L.eliteDesc = v->elite_desc;
        L.count = v->count; L.cell = v->cell; L.winner = v->winner;
        L.key = A.key; L.row = (int *)(A.key + slots);
        L.B = A.B; L.M = A.M; L.S = A.S; L.C = A.C;
        return insert_launch(rem2d_cvt_key_kernel, A, L, N, QUAD(v, ), QUAD(v, elite_), st);
    }
    // CV_LINE: the draw (its list in the scratch's last M C words, where the elites' sample keeps it), then the variation
    A.list = (int *)((unsigned long long *)v->scratch + slots);
    A.perBlock = v->n_children / v->n_blocks;
    hipLaunchKernelGGL(rem2d_cvt_draw_kernel, dim3((unsigned)A.M), dim3(CV_TILE), 0, st, A);
    HIP_TRY(hipGetLastError());
    CvLine Ln;
    memset(&Ln, 0, sizeof(Ln));
    quads(Ln, N, QUAD(v, elite_), QUAD(v, child_));
    Ln.parent = v->parent; Ln.parent2 = v->parent2;
    Ln.key0 = A.key0; Ln.key1 = A.key1; Ln.generation = v->generation;
    Ln.slots = (int)slots;
    Ln.sigmaIso = v->sigma_iso; Ln.sigmaLine = v->sigma_line;
    hipLaunchKernelGGL(rem2d_cvt_line_kernel, dim3((unsigned)v->n_children), dim3(WAVE), 0, st, Ln);
    HIP_TRY(hipGetLastError());
    return REM2D_OK;
}
extern "C" int64_t rem2d_cvt_scratch_bytes(const rem2d_cvt *v) {
    OK_TRY(cv_shapes_ok("cvt_scratch_bytes: ", v));
    const long long G = v->group_size > 0 ? (long long)v->n_blocks * (long long)v->group_size : 0;
    const long long R = std::max((long long)(v->n_rows > 0 ? v->n_rows : 0), G);
    return (int64_t)(cv_slots(v) * 12) + (int64_t)(8 * R);
}
// (the stream is a member of the descriptor, which may be NULL)
extern "C" int rem2d_cvt_assign(const rem2d_cvt *v) { return run(cv_ok, cv_launch, "cvt_assign", v, CV_ASSIGN, v ? v->stream : nullptr); }
extern "C" int rem2d_cvt_insert(const rem2d_cvt *v) { return run(cv_ok, cv_launch, "cvt_insert", v, CV_INSERT, v ? v->stream : nullptr); }
extern "C" int rem2d_cvt_emit_line(const rem2d_cvt *v) { return run(cv_ok, cv_launch, "cvt_emit_line", v, CV_LINE, v ? v->stream : nullptr); }

// ---- Pareto ranking (include/rem2d_pareto.h, csrc/rem2d_pareto.h) ----
extern "C" int rem2d_pareto_abi_version(void) { return REM2D_PARETO_ABI_VERSION; }
static_assert(REM2D_PARETO_MAX_GROUP == PA_LONG, "a block of the rank fits one workgroup");
static_assert(REM2D_PARETO_MAX_WIDTH == REM2D_NOVELTY_MAX_WIDTH && REM2D_PARETO_MAX_K <= 32, "the local kernel's register bounds and its 32-bit mask");
// The members both calls share.  Nothing the descriptor points to is read.
static int pa_ok(const std::string &s, const rem2d_pareto *p, int max_group) {
    if (!p) return fail(REM2D_E_INVALID, s + "NULL descriptor");
    if (p->n_rows < 1) return fail(REM2D_E_INVALID, s + "n_rows must be at least 1, not " + std::to_string(p->n_rows));
    if (p->group_size < 1 || (max_group && p->group_size > max_group) || p->n_rows % p->group_size != 0)
        return fail(REM2D_E_INVALID, s + "group_size must be " + (max_group ? "1.." + std::to_string(max_group) : std::string("at least 1")) +
                                         " and divide n_rows (" + std::to_string(p->n_rows) + "), not " + std::to_string(p->group_size));
    return REM2D_OK;
}
template <int T> static void pa_launch_rank(const PaArgs &A, int K, dim3 grid, hipStream_t st) {
    if (K == 1) hipLaunchKernelGGL((rem2d_pareto_rank_kernel<1, T>), grid, dim3(T), 0, st, A);
    else if (K == 2) hipLaunchKernelGGL((rem2d_pareto_rank_kernel<2, T>), grid, dim3(T), 0, st, A);
    else if (K == 3) hipLaunchKernelGGL((rem2d_pareto_rank_kernel<3, T>), grid, dim3(T), 0, st, A);
    else hipLaunchKernelGGL((rem2d_pareto_rank_kernel<4, T>), grid, dim3(T), 0, st, A);
}
extern "C" int rem2d_pareto_rank(const rem2d_pareto *p, void *stream) {
    const std::string s = "pareto_rank: ";
    OK_TRY(pa_ok(s, p, REM2D_PARETO_MAX_GROUP));
    if (p->n_obj < 1 || p->n_obj > REM2D_PARETO_MAX_OBJ)
        return fail(REM2D_E_INVALID, s + "n_obj must be 1.." + std::to_string(REM2D_PARETO_MAX_OBJ) + ", not " + std::to_string(p->n_obj));
    if (p->reserved != 0) return fail(REM2D_E_INVALID, s + "reserved must be 0");
    if (!p->obj) return fail(REM2D_E_INVALID, s + "NULL device pointer (obj)");
    const size_t G = (size_t)p->n_rows, M = G / (size_t)p->group_size;
    const Span obj = span(p->obj, G * (size_t)p->n_obj * sizeof(double), "obj");
    const Span out[4] = {span(p->front, G * sizeof(int32_t), "front"), span(p->crowd, G * sizeof(double), "crowd"),
                         span(p->util, G * sizeof(int32_t), "util"), span(p->n_fronts, M * sizeof(int32_t), "n_fronts")};
    for (const Span &o : out) // (each of them may be NULL)
        if (o.at) OK_TRY(apart(s, &o, 1, &obj, 1));
    PaArgs A;
    memset(&A, 0, sizeof(A));
    A.obj = p->obj; A.front = p->front; A.crowd = p->crowd; A.util = p->util; A.nfronts = p->n_fronts;
    A.G = p->n_rows; A.S = p->group_size;
    const long long T = A.S <= PA_SHORT ? PA_SHORT : PA_LONG, P = T / A.S; // whole blocks per workgroup
    const dim3 grid((unsigned)(((long long)M + P - 1) / P));
    if (T == PA_SHORT) pa_launch_rank<PA_SHORT>(A, p->n_obj, grid, (hipStream_t)stream);
    else pa_launch_rank<PA_LONG>(A, p->n_obj, grid, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return REM2D_OK;
}
template <int BP> static void pa_launch_local(const PaArgs &A, dim3 grid, hipStream_t st) {
    if (A.k <= 2) hipLaunchKernelGGL((rem2d_pareto_local_kernel<BP, 2>), grid, dim3(NV_TILE), 0, st, A);
    else if (A.k <= 8) hipLaunchKernelGGL((rem2d_pareto_local_kernel<BP, 8>), grid, dim3(NV_TILE), 0, st, A);
    else if (A.k <= 16) hipLaunchKernelGGL((rem2d_pareto_local_kernel<BP, 16>), grid, dim3(NV_TILE), 0, st, A);
    else hipLaunchKernelGGL((rem2d_pareto_local_kernel<BP, 32>), grid, dim3(NV_TILE), 0, st, A);
}
extern "C" int rem2d_pareto_local(const rem2d_pareto *p, void *stream) {
    const std::string s = "pareto_local: ";
    OK_TRY(pa_ok(s, p, 0));
    if (p->width < 1 || p->width > REM2D_PARETO_MAX_WIDTH)
        return fail(REM2D_E_INVALID, s + "width must be 1.." + std::to_string(REM2D_PARETO_MAX_WIDTH) + ", not " + std::to_string(p->width));
    if (p->k < 1 || p->k > REM2D_PARETO_MAX_K)
        return fail(REM2D_E_INVALID, s + "k must be 1.." + std::to_string(REM2D_PARETO_MAX_K) + ", not " + std::to_string(p->k));
    if (p->reserved != 0) return fail(REM2D_E_INVALID, s + "reserved must be 0");
    if (!p->desc) return fail(REM2D_E_INVALID, s + "NULL device pointer (desc)");
    if (!p->fitness) return fail(REM2D_E_INVALID, s + "NULL device pointer (fitness)");
    if (!p->local) return fail(REM2D_E_INVALID, s + "NULL device pointer (local)");
    const size_t G = (size_t)p->n_rows;
    const Span in[2] = {span(p->desc, G * (size_t)p->width * sizeof(float), "desc"), span(p->fitness, G * sizeof(double), "fitness")};
    const Span out[2] = {span(p->local, G * sizeof(double), "local"), span(p->neighbours, G * sizeof(int32_t), "neighbours")};
    OK_TRY(apart(s, out, p->neighbours ? 2 : 1, in, 2));
    PaArgs A;
    memset(&A, 0, sizeof(A));
    A.desc = p->desc; A.fitness = p->fitness; A.local = p->local; A.neigh = p->neighbours;
    A.G = p->n_rows; A.S = p->group_size; A.B = p->width; A.k = p->k;
    const dim3 grid((unsigned)(((long long)A.G + NV_TILE - 1) / NV_TILE));
    const hipStream_t st = (hipStream_t)stream;
    if (A.B <= 2) pa_launch_local<2>(A, grid, st);
    else if (A.B <= 4) pa_launch_local<4>(A, grid, st);
    else if (A.B <= 8) pa_launch_local<8>(A, grid, st);
    else if (A.B <= 16) pa_launch_local<16>(A, grid, st);
    else pa_launch_local<32>(A, grid, st);
    HIP_TRY(hipGetLastError());
    return REM2D_OK;
}

// ---- observation normalisation (include/rem2d_obsnorm.h, csrc/rem2d_obsnorm.h) ----
extern "C" int rem2d_obsnorm_abi_version(void) { return REM2D_OBSNORM_ABI_VERSION; }
enum { ON_ACC = 1, ON_FREEZE = 2, ON_APPLY = 4 };
static int on_dn(const rem2d_obsnorm *n) { return REM2D_OBS_HEAD + REM2D_OBS_BODY * n->max_bodies + n->n_rays; }
// The refusals of a normaliser's shapes; `s` prefixes the message.  No pointer is looked at.
static int on_shapes_ok(const std::string &s, const rem2d_obsnorm *n) {
    if (!n) return fail(REM2D_E_INVALID, s + "NULL descriptor");
    if (n->max_bodies < 1 || n->max_bodies > REM2D_CONTROL_MAX_BODIES)
        return fail(REM2D_E_INVALID, s + "max_bodies must be 1.." + std::to_string(REM2D_CONTROL_MAX_BODIES) + ", not " + std::to_string(n->max_bodies));
    if (n->n_rays < 0 || n->n_rays > REM2D_SENSE_MAX_RAYS)
        return fail(REM2D_E_INVALID, s + "n_rays must be 0.." + std::to_string(REM2D_SENSE_MAX_RAYS) + ", not " + std::to_string(n->n_rays));
    if (n->n_blocks < 1) return fail(REM2D_E_INVALID, s + "n_blocks must be at least 1, not " + std::to_string(n->n_blocks));
    if (n->group_size < 1) return fail(REM2D_E_INVALID, s + "group_size must be at least 1, not " + std::to_string(n->group_size));
    if ((long long)n->n_blocks * (long long)n->group_size > 0x7fffffffLL)
        return fail(REM2D_E_INVALID, s + "n_blocks * group_size must be at most 2^31 - 1");
    if ((long long)n->n_blocks * (long long)on_dn(n) > 0x7fffffffLL)
        return fail(REM2D_E_INVALID, s + "n_blocks times the words of a row must be at most 2^31 - 1");
    if (n->row_chunk < 0 || n->row_chunk > REM2D_OBSNORM_MAX_CHUNK)
        return fail(REM2D_E_INVALID, s + "row_chunk must be 0.." + std::to_string(REM2D_OBSNORM_MAX_CHUNK) + ", not " + std::to_string(n->row_chunk));
    if (n->reserved != 0) return fail(REM2D_E_INVALID, s + "reserved must be 0, not " + std::to_string(n->reserved));
    return REM2D_OK;
}
// Checks a normaliser for `stages`; `what` prefixes the message.  Nothing it points to is read.
static int on_ok(const char *what, const rem2d_obsnorm *n, int stages) {
    const std::string s = std::string(what) + ": ";
    OK_TRY(on_shapes_ok(s, n));
    if (stages & ON_ACC) {
        if (n->n_rows < 0) return fail(REM2D_E_INVALID, s + "negative row count");
        if (n->n_rows > (int64_t)n->n_blocks * (int64_t)n->group_size)
            return fail(REM2D_E_INVALID, s + std::to_string(n->n_rows) + " rows are more than n_blocks * group_size = " +
                                             std::to_string((long long)n->n_blocks * (long long)n->group_size));
        if (!n->obs) return fail(REM2D_E_INVALID, s + "NULL device pointer (obs)");
        if (n->n_rays > 0 && !n->frac) return fail(REM2D_E_INVALID, s + "NULL device pointer (frac)");
    }
    if (stages & ON_FREEZE) {
        if (n->min_count < 1) return fail(REM2D_E_INVALID, s + "min_count must be at least 1, not " + std::to_string(n->min_count));
        if (!(n->min_var > 0.0f) || !std::isfinite(n->min_var)) return fail(REM2D_E_INVALID, s + "min_var must be positive and finite");
    }
    if (stages & ON_APPLY) {
        if (!(n->clip > 0.0f)) return fail(REM2D_E_INVALID, s + "clip must be greater than 0 (it may be +inf)");
        if (n->context < 0) return fail(REM2D_E_INVALID, s + "context must be at least 0, not " + std::to_string(n->context));
    }
    if (stages & (ON_ACC | ON_FREEZE)) {
        const Span st[4] = {span(n->count, 0, "count"), span(n->s1, 0, "s1"), span(n->s2hi, 0, "s2hi"), span(n->s2lo, 0, "s2lo")};
        for (const Span &x : st) {
            if (!x.at) return fail(REM2D_E_INVALID, s + "NULL device pointer (" + x.name + ")");
            if (x.at % 8 != 0) return fail(REM2D_E_INVALID, s + x.name + " must be 8-byte aligned");
        }
    }
    if (stages & (ON_FREEZE | ON_APPLY)) {
        if (!n->mu) return fail(REM2D_E_INVALID, s + "NULL device pointer (mu)");
        if (!n->inv) return fail(REM2D_E_INVALID, s + "NULL device pointer (inv)");
    }
    return REM2D_OK;
}
template <int WPL> static void on_launch_acc(const OnArgs &A, dim3 grid, size_t slots, hipStream_t st) {
    hipLaunchKernelGGL(rem2d_obsnorm_accumulate_kernel<WPL>, grid, dim3(ON_THREADS), slots * (size_t)(3 * WPL * WAVE + 1) * sizeof(long long), st, A);
}
// The accumulation and / or the tables of a checked descriptor on `st`.
static int on_launch(const rem2d_obsnorm *n, int stages, hipStream_t st) {
    const int Dn = on_dn(n);
    if ((stages & ON_ACC) && n->n_rows > 0) {
        OnArgs A;
        memset(&A, 0, sizeof(A));
        A.obs = n->obs; A.frac = n->frac; A.rowMask = n->row_mask;
        A.count = (long long *)n->count; A.s1 = (long long *)n->s1; A.s2hi = (long long *)n->s2hi; A.s2lo = (long long *)n->s2lo;
        A.nRows = n->n_rows;
        A.nObs = Dn - n->n_rays; A.R = n->n_rays; A.Dn = Dn; A.S = n->group_size;
        // rows of a block per wavefront: the caller's, or 32 -- 2048 wavefronts at 65 536 rows, one wavefront per block of up to 32
        A.rowChunk = std::min(n->group_size, n->row_chunk > 0 ? n->row_chunk : 32);
        A.nChunks = (n->group_size + A.rowChunk - 1) / A.rowChunk;
        A.items = ((n->n_rows + n->group_size - 1) / n->group_size) * (long long)A.nChunks; // (only the blocks that have rows)
        const long long groups = (A.items + ON_WAVES - 1) / ON_WAVES;
        if (groups > 0x7fffffffLL) return fail(REM2D_E_INVALID, "obsnorm: too many rows for one launch");
        const dim3 grid((unsigned)groups);
        const size_t slots = A.nChunks > 1 ? ON_WAVES - 1 : 0;
        if (Dn <= WAVE) on_launch_acc<1>(A, grid, slots, st);
        else if (Dn <= 2 * WAVE) on_launch_acc<2>(A, grid, slots, st);
        else if (Dn <= 4 * WAVE) on_launch_acc<4>(A, grid, slots, st);
        else on_launch_acc<ON_MAX_WPL>(A, grid, slots, st);
        HIP_TRY(hipGetLastError());
    }
    if (stages & ON_FREEZE) {
        OnFreezeArgs F;
        memset(&F, 0, sizeof(F));
        F.count = (const long long *)n->count; F.s1 = (const long long *)n->s1; F.s2hi = (const long long *)n->s2hi; F.s2lo = (const long long *)n->s2lo;
        F.mu = n->mu; F.inv = n->inv;
        F.total = (long long)n->n_blocks * (long long)Dn; F.minCount = n->min_count; F.Dn = Dn; F.minVar = n->min_var;
        hipLaunchKernelGGL(rem2d_obsnorm_freeze_kernel, dim3((unsigned)((F.total + ON_THREADS - 1) / ON_THREADS)), dim3(ON_THREADS), 0, st, F);
        HIP_TRY(hipGetLastError());
    }
    return REM2D_OK;
}
static_assert(REM2D_CONTROL_MAX_BODIES * REM2D_OBS_BODY + REM2D_OBS_HEAD + REM2D_SENSE_MAX_RAYS <= ON_MAX_WPL * WAVE, "a row's words fit the lanes' registers");
extern "C" int rem2d_obsnorm_accumulate(const rem2d_obsnorm *n) { return run(on_ok, on_launch, "obsnorm_accumulate", n, ON_ACC, n ? n->stream : nullptr); }
extern "C" int rem2d_obsnorm_freeze(const rem2d_obsnorm *n) { return run(on_ok, on_launch, "obsnorm_freeze", n, ON_FREEZE, n ? n->stream : nullptr); }
// Checks a normaliser against the policy it is applied to (`memory`: the pass with context words), before anything is launched;
// *q is the recurrent descriptor made of p and the normaliser's context members where memory is set.
static int on_policy_ok(const char *what, const rem2d_obsnorm *n, const rem2d_policy *p, bool memory, rem2d_recurrent *q) {
    const std::string s = std::string(what) + ": ";
    OK_TRY(on_ok(what, n, ON_APPLY));
    if (!p) return fail(REM2D_E_INVALID, s + "NULL policy");
    if (memory) {
        q->p = *p; q->context = n->context; q->reserved = 0; q->memory = n->memory; q->reset = n->reset;
        OK_TRY(recurrent_ok(what, q));
    } else {
        if (n->context != 0) return fail(REM2D_E_INVALID, s + "context must be 0 for a feed-forward policy, not " + std::to_string(n->context));
        OK_TRY(policy_ok(what, p));
    }
    if (p->max_bodies != n->max_bodies || p->n_rays != n->n_rays)
        return fail(REM2D_E_INVALID, s + "the policy has max_bodies " + std::to_string(p->max_bodies) + " and n_rays " + std::to_string(p->n_rays) +
                                         ", the normaliser " + std::to_string(n->max_bodies) + " and " + std::to_string(n->n_rays));
    if (p->n_rows > (int64_t)n->n_blocks * (int64_t)n->group_size)
        return fail(REM2D_E_INVALID, s + std::to_string(p->n_rows) + " rows are more than n_blocks * group_size = " +
                                         std::to_string((long long)n->n_blocks * (long long)n->group_size));
    return REM2D_OK;
}
static PolNorm on_tables(const rem2d_obsnorm *n) { return {n->mu, n->inv, n->clip, n->group_size, on_dn(n)}; }
extern "C" int rem2d_obsnorm_forward(const rem2d_obsnorm *n, const rem2d_policy *p) {
    OK_TRY(on_policy_ok("obsnorm_forward", n, p, false, nullptr));
    const PolNorm nm = on_tables(n);
    return policy_launch(p, (hipStream_t)n->stream, &nm);
}
extern "C" int rem2d_obsnorm_forward_memory(const rem2d_obsnorm *n, const rem2d_policy *p) {
    rem2d_recurrent q;
    OK_TRY(on_policy_ok("obsnorm_forward_memory", n, p, true, &q));
    const PolNorm nm = on_tables(n);
    return recurrent_launch(&q, (hipStream_t)n->stream, &nm);
}
extern "C" int rem2d_worlds_act_normed(rem2d_world *const *worlds, int32_t n_worlds, const rem2d_obsnorm *n, const rem2d_policy *p,
                                       const double *ray_offsets_dev, int32_t accumulate) {
    OK_TRY(worlds_given("act_normed: ", worlds, n_worlds));
    rem2d_recurrent q;
    const bool memory = n && n->context > 0;
    OK_TRY(on_policy_ok("act_normed", n, p, memory, &q));
    rem2d_obsnorm acc = *n; // the accumulation reads what this call's observe and sense write
    acc.obs = p->obs; acc.frac = p->frac; acc.row_mask = p->row_mask; acc.n_rows = p->n_rows;
    if (accumulate) OK_TRY(on_ok("act_normed", &acc, ON_ACC));
    const hipStream_t st = (hipStream_t)n->stream;
    return act("act_normed: ", worlds, n_worlds, p, ray_offsets_dev, st, [&] {
        if (accumulate) OK_TRY(on_launch(&acc, ON_ACC, st));
        const PolNorm nm = on_tables(n);
        return memory ? recurrent_launch(&q, st, &nm) : policy_launch(p, st, &nm);
    });
}

extern "C" int rem2d_world_enable_timing(rem2d_world *w, int32_t on) {
    if (!w) return fail(REM2D_E_INVALID, "world is NULL");
    HIP_TRY(hipSetDevice(w->cfg.device));
    if (on) {
        drain_timing(w);
        const size_t want = on > 1 ? (size_t)on : 4096; // launches that can be timed before the next read-back
        for (EventPool *pool : {&w->evKernel, &w->evStep}) {
            int rc = pool->fill(want);
            if (rc != REM2D_OK) return rc;
        }
    }
    w->timing = on != 0;
    return REM2D_OK;
}
extern "C" int rem2d_world_kernel_time_ms(rem2d_world *w, double *total_ms, int64_t *launches) {
    if (!w) return fail(REM2D_E_INVALID, "world is NULL");
    HIP_TRY(hipSetDevice(w->cfg.device));
    drain_timing(w);
    w->evKernel.report(total_ms, launches);
    return REM2D_OK;
}
#if defined(REM2D_TOI_STAMPS) || defined(REM2D_POS_STAMPS)
// diagnostic builds only: the TOI kernel's / the position solver's cycle counters (toiWork[0..16)), then zeroed
extern "C" int rem2d_world_debug_words(rem2d_world *w, int32_t *out16) {
    HIP_TRY(hipSetDevice(w->cfg.device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out16, w->S.toiWork, 16 * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(w->S.toiWork + 1, 0, 15 * sizeof(int)));
    return REM2D_OK;
}
#endif
extern "C" int rem2d_world_handover_failures(const rem2d_world *w, int64_t *count, int32_t clear) {
    if (!w || !count) return fail(REM2D_E_INVALID, "handover_failures: NULL argument");
    // (pinned host memory the kernels add to at system scope: readable without a device call; what it holds is what the launches
    // that have FINISHED so far reported)
    *count = w->trainFailures ? (int64_t)__atomic_load_n(w->trainFailures, __ATOMIC_RELAXED) : 0;
    if (clear && w->trainFailures) __atomic_store_n(w->trainFailures, 0u, __ATOMIC_RELAXED);
    return REM2D_OK;
}
extern "C" int rem2d_world_step_time_ms(rem2d_world *w, double *total_ms, int64_t *steps) {
    if (!w) return fail(REM2D_E_INVALID, "world is NULL");
    HIP_TRY(hipSetDevice(w->cfg.device));
    drain_timing(w);
    w->evStep.report(total_ms, steps);
    return REM2D_OK;
}

// ---- self-test of the collision geometry on a table of cases (include/rem2d_selftest.h); LAST: its kernel follows every other ----
#include "rem2d_selftest.h"
