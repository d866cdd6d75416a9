// rem2d_stream.h -- streaming evaluation (include/rem2d_stream.h): the slots of creatures whose episode has ended are harvested and
// handed to the next creatures of a pending queue, for a whole population between two steps.
// Part of the single translation unit rem2d.hip (see its header comment); not a stand-alone header.
//
// No step kernel knows about any of this, and there is no arithmetic of its own here: a refilled slot receives what reset_lane
// (rem2d_kernels.h) writes from the 20 morphology words copied into the world's device morphology; the harvest words are copies.
//
// Launch shape: that of rem2d_reset_where_kernel (rem2d_episode.h): CtlTable / ctl_locate, a wavefront = one 64-lane block of ONE
// world, one lane per (creature, lane).  Beside the table, per world: its morphology pointers and env4 base (as EpWorld) and its
// feed -- 20 more pointers, the id array, the cursor and the count: 352 bytes.  Sixteen of them would not fit the 4 KB of kernel
// arguments next to the 1 032-byte CtlTable, so a launch takes STREAM_TABLE = 8 worlds (1 032 + 2 816 + 64 = 3 912 bytes); the rest
// go to further launches on the same stream.  A device-resident feed table was the alternative; it would have to be allocated and
// kept current by somebody, and the call allocates nothing.
//
// Program order inside a wavefront: (1) every lane loads its creature's done / frozen / steps words and occupant[r] and computes
// `ended` -- a creature never spans wavefronts (K <= 64, groups aligned), so all its lanes agree; (2) the root lane writes the harvest
// of id occ; (3) one ballot of the ended root lanes: a wavefront with none leaves (wave-uniform); (4) ONE returning device-scope
// atomicAdd(cursor, popcount) by the first ended root lane, its result broadcast; a root lane's q = that base + its rank among the
// set bits, handed to the creature's other lanes by a shuffle from the root lane; (5) lanes with q < count copy their 20 words and run
// reset_lane on them, root lanes write occupant (and REM2D_F_FROZEN = 1 where the queue is empty).  The loads of (1) and (2) precede
// every store to those words in program order.  Plain vector loads and stores and the one atomic: no LDS, no barrier.  Worlds that
// share a cursor draw from it in whatever order their wavefronts arrive: which pending creature lands where is unspecified, that
// each is handed out once is the atomic's doing.
#ifndef REM2D_STREAM_KERNELS_H
#define REM2D_STREAM_KERNELS_H

#define STREAM_TABLE 8 // worlds per launch (see above)
static_assert(STREAM_TABLE <= CTL_TABLE, "the worlds of a refill launch sit in one CtlTable");

struct StWorld {
    rem2d_morph M; // the device arrays rem2d_world_reset took for this world: WRITTEN at the lanes of refilled slots
    char *env4;    // State::env4
    rem2d_morph F; // the feed: [count * lanes] each
    const int *id; // [count]
    int *cursor;   // pending creatures handed out so far
    int count, pad;
};
struct StTable {
    StWorld w[STREAM_TABLE]; // world i of the launch's CtlTable
};
struct StArgs {
    int *occupant;        // [nRows]
    rem2d_stream_out out; // any member may be nullptr
    long long nIds, nRows;
    unsigned when;
    int maxSteps;
};

// (the morphology of a world is const to every other kernel; this one owns the lanes of the slots it refills)
#define ST_COPY(T, f) (const_cast<T *>(W.M.f))[gl] = W.F.f[src]

__global__ __launch_bounds__(CTL_THREADS) void rem2d_refill_kernel(CtlTable Tb, StTable Ts, StArgs A) {
    CtlLane c;
    if (!ctl_locate(Tb, c)) return;
    const StWorld &W = Ts.w[c.world];
    EpState S;
    S.lane4 = c.S.lane4; S.lane8 = c.S.lane8; S.slot4 = c.S.slot4; S.env4 = W.env4; S.env8 = c.S.env8;
    S.Lp = c.S.Lp; S.Np = c.S.Np;
    const unsigned gl = c.gl, env = c.env;
    const int lane = (int)(threadIdx.x & (WAVE - 1));
    bool ended = false;
    long long r = -1;
    if (c.inWorld) {
        r = c.S.index ? (long long)c.S.index[env] : (long long)env;
        if (r >= 0 && r < A.nRows) {
            const int occ = A.occupant[r];
            const int done = EI(E_DONE), frozen = EI(E_FROZEN), steps = EI(E_STEPS);
            ended = occ >= 0 && (((A.when & REM2D_WHEN_DONE) && done != 0) || ((A.when & REM2D_WHEN_FROZEN) && frozen != 0) ||
                                 ((A.when & REM2D_WHEN_STEPS) && A.maxSteps > 0 && steps >= A.maxSteps));
            if (ended && c.sub == 0 && (long long)occ < A.nIds) { // the harvest of id occ: read here, before any store of step (5)
                if (A.out.fitness) A.out.fitness[occ] = ED(E_FITNESS);
                if (A.out.steps) A.out.steps[occ] = steps;
                if (A.out.err) A.out.err[occ] = EI(E_ERR);
                if (A.out.finished) A.out.finished[occ] = 1;
            }
        }
    }
    const unsigned long long roots = __ballot(ended && c.sub == 0);
    if (roots == 0ull) return;
    const int leader = __ffsll((unsigned long long)roots) - 1;
    int first = 0;
    if (lane == leader) first = atomicAdd(W.cursor, __popcll(roots)); // device scope; one per wavefront
    first = __shfl(first, leader);
    const int q = __shfl(first + __popcll(roots & ((1ull << lane) - 1ull)), c.base); // the root lane's, for all lanes of its creature
    if (!ended) return;
    if (q >= 0 && q < W.count) {
        const size_t src = (size_t)q * (size_t)c.K + (size_t)c.sub;
        ST_COPY(int32_t, shape); ST_COPY(float, hx); ST_COPY(float, hy); ST_COPY(float, x); ST_COPY(float, y); ST_COPY(float, angle);
        ST_COPY(int32_t, parent); ST_COPY(int32_t, jround); ST_COPY(float, ax); ST_COPY(float, ay); ST_COPY(float, bx);
        ST_COPY(float, by); ST_COPY(float, torque); ST_COPY(float, lower); ST_COPY(float, upper); ST_COPY(double, amp);
        ST_COPY(double, phase); ST_COPY(double, freq); ST_COPY(double, offset); ST_COPY(double, istate);
        reset_lane(S, W.M, gl, env, (unsigned)c.sub, true);
        if (c.sub == 0) A.occupant[r] = W.id[q];
    } else if (c.sub == 0) { // the queue is empty: the slot is retired
        A.occupant[r] = -1;
        EI(E_FROZEN) = 1;
    }
}
#undef ST_COPY

#endif
