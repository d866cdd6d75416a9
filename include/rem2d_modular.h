#ifndef REM2D_MODULAR_H
#define REM2D_MODULAR_H

/* Modular device policies for librem2d.so: ONE small controller that runs once per MODULE of a creature instead of once per
 * creature (Pathak et al. 2019; Huang et al. 2020, "shared modular policies").  The same network sees a module's own joint, a few
 * creature-wide words and two short message vectors -- the sum of its children's and its parent's -- and writes that module's joint
 * target and its own next message.  A weight set is therefore tied to no body column and to no morphology: one set drives a
 * population of different trees.  A header of its own: nothing here changes what the feed-forward or the recurrent forward pass
 * computes, what a step, an observation row or a ray fraction holds, or any other ABI version.
 *
 * ---- 1. The topology table (rem2d_worlds_topology) ----
 * int32 topo[out_rows][max_bodies][2], rows in the population order of rem2d_worlds_observe, body b the b-th live lane of the
 * creature exactly as that call counts them:
 *   word 0   the BODY INDEX of the parent of body b; -1 for the root, for a body whose parent has no column < max_bodies, and for
 *            the slots beyond the creature's count
 *   word 1   the lane's shape word (REM2D_F_SHAPE: the one whose being non-zero makes a lane live); 0 for empty slots
 * A row outside [0, out_rows) is skipped.  One launch per 16 worlds.
 *
 * ---- 2. The weight set: how it differs from an ordinary rem2d_policy ----
 * The descriptor embeds a rem2d_policy p.  Its ROW side keeps its meaning: p.max_bodies = MB is the number of body columns of
 * obs [n_rows][8 + 6 MB], targets [n_rows][MB] and valid [n_rows][MB]; p.n_rays = R the columns of frac.  Its WEIGHT side is that
 * of an ordinary set with max_bodies = 1:
 *   w1[Dm][H], b1[H], w2[H][1], b2[1]      Dm = 8 + 6 + R + 2 + 2 K      p.d must be Dm
 * with K = messages.  Limits: 1 <= K <= H, R + 2 + 2 K <= 64, 1 <= rounds <= 8, MB in 1 .. 64.
 *
 * ---- 3. The forward pass (rem2d_modular_forward) ----
 * For population row r with weight set g (resolved as rem2d_policy.h states: index[r], or r), P = rounds:
 *   live(b)  = topo[r][b][1] != 0
 *   par(b)   = topo[r][b][0] if that lies in [0, MB), is not b and is live; otherwise none
 *   m0_b[k]  = reset && reset[r] ? +0.0f : memory[r][b][k] for live b (a substitution, not a product: a NaN in memory does not
 *              survive a reset); a slot that is not live reads +0
 * For round p = 0 .. P-1, for every live body b, from m^p only:
 *   pm_k = m^p_par(b)[k], or +0.0f without a parent
 *   cm_k = +0.0f; then for the live bodies c with par(c) == b in ASCENDING c: cm_k = cm_k + m^p_c[k], each one rounded binary32 add
 *   x    = the Dm words  [ the 8 head words of obs row r | the 6 words of body b | the R ray fractions | (float)topo[r][b][1] |
 *                          (float)(the number of children counted above) | cm_0 .. cm_{K-1} | pm_0 .. pm_{K-1} ]
 *   a_j, h_j, y_0, t_0 exactly as rem2d_policy.h states them over these Dm words in ascending order
 *   m^{p+1}_b[k] = h_k for k < K, as computed, non-finite values included
 * After round P-1: for live b targets[r][b] = (double)t_0, valid[r][b] = isfinite(t_0), memory[r][b][.] = m^P_b; for the slots that
 * are not live targets 0.0, valid 0, memory +0.0f.  Column 0 is written like any other (rem2d_worlds_control ignores it).  A row that
 * the row mask clears, or whose index names no weight set, is skipped entirely: its targets, valid bytes and memory stay as they
 * are.  topo may hold ANY int32 values: nothing is read or written out of bounds for any of them (a 2-cycle of parents makes two
 * bodies each other's parent and child; nothing is followed further than one edge).
 *
 * The arithmetic rules are those of rem2d_policy.h: every product, sum and quotient is one separately, correctly rounded binary32
 * operation, nothing is fused in any build of the library, and there is no transcendental function (tests/modular_model.py
 * reproduces every bit).  Observation normalisation is not applied.
 *
 * Law (a).  One round on row r, body b writes the bits the recurrent forward pass (the recurrent policies' header) writes for a
 * flattened row with max_bodies = 1, obs' = [head | body b], frac' = [frac | shape | children | cm], n_rays' = R + 2 + K,
 * context = K and memory' = pm: the target is its column 0, its new memory the new message.
 * Law (b).  To anything that only moves weights about (the headers of the search operators: selection and mutation, the evolution
 * strategies, the elite grids and the centroid archives) a modular set is an ordinary set with max_bodies = 1 and R + 2 + 2 K
 * ray inputs; that is why that sum is held to the 64 "ray" inputs a feed-forward set may have.
 *
 * In place: a row belongs to exactly one wavefront, which reads all of the row's messages before it writes any of them; no other
 * row's memory is read.
 *
 * ---- 4. The stream ----
 * Both descriptors carry the stream their calls queue on, as rem2d_step_group does, and the descriptor of the centroid archives'
 * header.  All work is queued on that stream, asynchronous, on the device that is current; nothing synchronises; the library
 * allocates nothing and nothing is loaded on a first call. */

#include "rem2d_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REM2D_MODULAR_ABI_VERSION 1
#define REM2D_MODULAR_MAX_ROUNDS 8
#define REM2D_MODULAR_MAX_INPUTS 64 /* R + 2 + 2 K: REM2D_SENSE_MAX_RAYS, law (b) */

/* Where rem2d_worlds_topology writes. */
typedef struct rem2d_topology {
    int32_t max_bodies;    /* MB: 1 .. 64 (REM2D_CONTROL_MAX_BODIES) */
    int32_t reserved;      /* 0 */
    int32_t *out;          /* [out_rows][MB][2], written */
    int64_t out_rows;      /* >= 0 */
    void *stream;          /* the stream the call queues on */
} rem2d_topology;

/* Caller-owned device pointers and the shapes they have. */
typedef struct rem2d_modular {
    rem2d_policy p;        /* as for rem2d_policy_forward, except: p.d == 8 + 6 + p.n_rays + 2 + 2 * messages, w2 is [G][H][1] and
                              b2 [G][1]; p.max_bodies stays MB, the columns of obs / targets / valid */
    int32_t messages;      /* K: 1 .. p.hidden, p.n_rays + 2 + 2 K <= REM2D_MODULAR_MAX_INPUTS */
    int32_t rounds;        /* P: 1 .. REM2D_MODULAR_MAX_ROUNDS */
    const int32_t *topo;   /* [n_rows][MB][2]: what rem2d_worlds_topology wrote (max_bodies = MB), or any values */
    float *memory;         /* [n_rows][MB][K], read and written in place */
    const uint8_t *reset;  /* [n_rows] or NULL: non-zero = this row's messages read as +0.0f */
    void *stream;          /* the stream the calls queue on */
} rem2d_modular;

/* REM2D_MODULAR_ABI_VERSION of the library */
int rem2d_modular_abi_version(void);

/* The topology table of every creature of `worlds` (any number: all lane buckets and step groups of a population; one launch per
 * 16 worlds) into t->out, on t->stream.  Errors are those of rem2d_worlds_observe: REM2D_E_INVALID for a NULL pointer (t and
 * t->out included), n_worlds <= 0, max_bodies or out_rows out of range, reserved != 0 or a world of more than 64 lanes per
 * creature; REM2D_E_STATE before rem2d_world_reset. */
int rem2d_worlds_topology(rem2d_world *const *worlds, int32_t n_worlds, const rem2d_topology *t);

/* The modular forward pass alone, on whatever the rows of q->p.obs / q->p.frac, q->topo and q->memory hold: one kernel on
 * q->stream.  REM2D_E_INVALID for a NULL q, a NULL topo or memory, messages < 1, messages > p.hidden,
 * p.n_rays + 2 + 2 messages > 64, rounds outside 1 .. 8, p.d != 8 + 6 + p.n_rays + 2 + 2 messages, and everything
 * rem2d_policy_forward refuses of p (its rule for d replaced by the one above). */
int rem2d_modular_forward(const rem2d_modular *q);

/* rem2d_worlds_act with the modular pass in the middle: rem2d_worlds_observe into q->p.obs, rem2d_worlds_sense into q->p.frac if
 * p.n_rays > 0, the modular forward pass, and rem2d_worlds_control with q->p.targets / q->p.valid, all on q->stream.  The same
 * number of launches as rem2d_worlds_act.  q->topo is the caller's and is not recomputed here: it must describe the creatures in
 * place.  Everything is checked before the first launch: what rem2d_modular_forward refuses and what rem2d_worlds_act refuses of
 * its worlds and ray offsets. */
int rem2d_worlds_act_modular(rem2d_world *const *worlds, int32_t n_worlds, const rem2d_modular *q, const double *ray_offsets_dev);

#ifdef __cplusplus
}
#endif

#endif /* REM2D_MODULAR_H */
