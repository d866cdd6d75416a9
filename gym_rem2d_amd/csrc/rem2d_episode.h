// rem2d_episode.h -- episode boundaries (include/rem2d_episode.h): masked / conditional reset of single creatures in place, and the
// harvest of the episodes that ended, for a whole population between two steps.
// Part of the single translation unit rem2d.hip (see its header comment); not a stand-alone header.
//
// No step kernel knows about any of this, and there is no arithmetic of its own here: a selected creature receives what
// reset_lane (rem2d_kernels.h) writes -- the body rem2d_reset_kernel runs for every lane of a world --, the harvest words are copies.
//
// Launch shape: that of observe (rem2d_control.h): CtlTable / ctl_locate, a wavefront = one 64-lane block of ONE world, one lane per
// (creature, lane), so every field access is a coalesced load / store.  The morphology pointers of the launch's worlds (and the base
// of their per-creature 4-byte words, which CtlWorld does not carry) sit beside the table in the kernel arguments: 16 x 168 bytes, 3.8
// KB of kernarg in all, read from the kernarg segment with a wave-uniform index.
//
// Program order inside a wavefront: (1) every lane loads its creature's done / frozen / steps words and its row's mask byte and
// computes `selected` -- a creature never spans wavefronts (K <= 64, groups aligned), so all its lanes agree; (2) the root lane
// writes the harvest words of its row; (3) a wavefront without a selected lane leaves (wave-uniform, one ballot); (4) the selected
// lanes run reset_lane.  The loads of (1) and (2) precede every store to those words in program order, which is all a single
// wavefront needs: no LDS, no barrier, no atomics -- one root lane owns one creature and one population row.  Plain vector loads and
// stores only.
#ifndef REM2D_EPISODE_KERNELS_H
#define REM2D_EPISODE_KERNELS_H

struct EpWorld {
    rem2d_morph M; // the device arrays rem2d_world_reset took for this world
    char *env4;    // State::env4 (done, frozen, steps, reward, ... of its creatures)
};
struct EpTable {
    EpWorld w[CTL_TABLE]; // world i of the launch's CtlTable
};
struct EpState { // what reset_lane's accessors go through
    char *lane4, *lane8, *slot4, *env4, *env8;
    unsigned Lp, Np;
};
struct EpArgs {
    const unsigned char *mask; // [nRows] or nullptr
    rem2d_episode_out out;     // any member may be nullptr
    long long nRows;
    unsigned when;
    int maxSteps;
};

__global__ __launch_bounds__(CTL_THREADS) void rem2d_reset_where_kernel(CtlTable Tb, EpTable Te, EpArgs A) {
    CtlLane c;
    if (!ctl_locate(Tb, c)) return;
    const EpWorld &W = Te.w[c.world];
    EpState S;
    S.lane4 = c.S.lane4; S.lane8 = c.S.lane8; S.slot4 = c.S.slot4; S.env4 = W.env4; S.env8 = c.S.env8;
    S.Lp = c.S.Lp; S.Np = c.S.Np;
    const unsigned gl = c.gl, env = c.env;
    bool selected = false;
    if (c.inWorld) {
        const long long r = c.S.index ? (long long)c.S.index[env] : (long long)env;
        if (r >= 0 && r < A.nRows) {
            const int done = EI(E_DONE), frozen = EI(E_FROZEN), steps = EI(E_STEPS);
            const bool ended = A.when == 0u || ((A.when & REM2D_WHEN_DONE) && done != 0) || ((A.when & REM2D_WHEN_FROZEN) && frozen != 0) ||
                               ((A.when & REM2D_WHEN_STEPS) && A.maxSteps > 0 && steps >= A.maxSteps);
            selected = ended && (A.mask == nullptr || A.mask[r] != 0);
            if (c.sub == 0) { // the harvest of row r: read here, before any store of step (4)
                if (A.out.reward) A.out.reward[r] = EF(E_REWARD);
                if (A.out.done) A.out.done[r] = done != 0 ? 1 : 0;
                if (A.out.ended) A.out.ended[r] = selected ? 1 : 0;
                if (selected) {
                    if (A.out.fitness) A.out.fitness[r] = ED(E_FITNESS);
                    if (A.out.steps) A.out.steps[r] = steps;
                    if (A.out.episodes) A.out.episodes[r] = A.out.episodes[r] + 1;
                }
            }
        }
    }
    if (__ballot(selected) == 0ull) return;
    if (selected) reset_lane(S, W.M, gl, env, (unsigned)c.sub, true);
}

#endif
