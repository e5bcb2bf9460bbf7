/* ukf_batch_assign.h -- global nearest-neighbour assignment: the one-to-one assignment of detections to the filters of a SCENE,
 * solved on the device.  An extension of ukf_batch.h (same library, same engine handle, same conventions) in a header of its
 * own: ukf_batch.h and the binding's table for it (abi.py) are pinned entry point by entry point, so what is added beside them
 * is declared beside them -- here, and in abi_assign.py, which tests/test_assign_host.py holds to this header type by type.
 * Plain C99. */
#ifndef UKF_BATCH_ASSIGN_H
#define UKF_BATCH_ASSIGN_H

#include "ukf_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ukfb_innovation_dev, ukfb_associate_sensor_dev and ukfb_update_pda_dev decide PER FILTER: best[i] is filter i's nearest gated
 * candidate, whatever its neighbours picked.  Where several tracks see the same detections (USBL returns, landmark fixes,
 * crossing targets) two filters claim one detection and another detection goes unused.  This call solves the assignment per
 * scene and writes `assign`, an array of the shape and meaning of `best`: ukfb_select_candidates_dev, ukfb_update_dev and
 * ukfb_update_sensor_dev with a per-filter model array work on it unchanged.
 *
 * SCENE s covers the engine slots [a, b), T = b - a tracks, and K = candidates detections: candidate k of every filter of the
 * scene is the scene's detection k, the layout the association calls take.
 *   ragged mode:  scene_start_dev, int32 [scenes + 1], ascending; a = scene_start[s], b = scene_start[s + 1];
 *   uniform mode (scene_start_dev == NULL): tracks_per_scene = T0 in 1 ... 32, scene s is [s T0, min((s + 1) T0, capacity)),
 *                 scenes <= ceil(capacity / T0).
 * Slots outside every scene are not written.
 * INPUT: cost[k][i], [candidates][capacity] in engine precision: the maha or -2 loglik an association call wrote, as it lies in
 * memory.  fp32 costs are promoted to double exactly: the solver runs in fp64 for every engine precision.
 * RULES: a pair (i, k) is ALLOWED iff cost is finite, |cost| <= UKFB_ASSIGN_COST_MAX, and cost <= gate when gate >= 0 (gate is
 * a field of this call, not cfg.gate_chi2: the cost need not be d^2).  miss_i = miss_dev[i] if given, else miss_uniform: the
 * cost of leaving track i without a detection.  A track is ELIGIBLE iff miss_i is finite and |miss_i| <= UKFB_ASSIGN_COST_MAX;
 * an ineligible track gets -1 and takes no part in the solve (an uninitialised or failed filter whose scores are NaN and
 * whose caller wrote NaN there).
 * OBJECTIVE: minimise J = sum over assigned pairs of cost + sum over eligible unassigned tracks of miss_i over the matchings:
 * each track takes at most one detection and each detection at most one track.  miss = gate_chi2 is classical global nearest
 * neighbour; a large miss maximises the number of assignments first.  Any optimum is a correct answer, and the result is
 * DETERMINISTIC: the same inputs give the same bits, whatever the scene's position in its workgroup.
 * LIMITS: T <= UKFB_ASSIGN_MAX_TRACKS, K <= UKFB_ASSOCIATE_MAX_CANDIDATES: the T x (K + T) problem (one private miss column
 * per track) has at most 64 columns.
 * OUTPUTS (any may be NULL, not all): assign [capacity] int32, the detection index or -1, a drop-in for best_dev;
 * owner [scenes][candidates] int32, the engine slot that took detection k or -1 (free detections are where new tracks start);
 * objective [scenes], always double; scene_status [scenes] uint32, UKFB_ASSIGN_OK or UKFB_ASSIGN_BAD_SCENE.
 * BAD SCENES: the offsets live on the device, so the kernel does not trust them: a segment with a < 0, b > capacity, b < a or
 * T > 32 sets UKFB_ASSIGN_BAD_SCENE and writes nothing else; nothing outside a scene's own rows is read or written.  The
 * host-array form knows the offsets and refuses them with UKFB_ERR_OUT_OF_RANGE before any launch.
 * The call is READ-ONLY on the engine, bit for bit, stream-ordered on the engine's stream, and allocates nothing at call
 * time.  Device groups: per shard through ukfb_group_shard.
 * ARGUMENT ERRORS, decided on the host before any launch, nothing written: a NULL in or cost, every output NULL, a non-finite
 * miss_uniform without miss_dev: UKFB_ERR_INVALID_ARG; candidates outside 1 ... 32, tracks_per_scene outside 1 ... 32 in
 * uniform mode, scenes < 0 or more than the mode admits (ragged: capacity + 1, empty scenes included): UKFB_ERR_OUT_OF_RANGE.
 * scenes = 0 is UKFB_OK and launches nothing.
 * Out of scope: JPDA or any weighted joint association; scenes over 32 tracks or 32 detections; scenes of non-contiguous
 * slots (arrange them with ukfb_gather_filters_dev / ukfb_compact_dev); K-best assignments (Murty); fusing the solve into an
 * association kernel; group fan-out calls. */
#define UKFB_ASSIGN_MAX_TRACKS 32
#define UKFB_ASSIGN_COST_MAX 1e100
enum { UKFB_ASSIGN_OK = 0, UKFB_ASSIGN_BAD_SCENE = 1 };
typedef struct ukfb_assign_in {      /* device pointers; gate and miss_uniform are host doubles, by value */
    const void*    cost_dev;         /* [candidates][capacity] engine precision                                    */
    int            candidates;       /* K = 1 ... UKFB_ASSOCIATE_MAX_CANDIDATES                                    */
    int            scenes;           /* >= 0                                                                       */
    const int32_t* scene_start_dev;  /* [scenes + 1] ascending slot offsets, or NULL: uniform mode                 */
    int            tracks_per_scene; /* uniform mode: T0 = 1 ... UKFB_ASSIGN_MAX_TRACKS (ragged mode: ignored)     */
    double         gate;             /* >= 0: pairs with cost > gate are forbidden; < 0 (or NaN): no gate          */
    const void*    miss_dev;         /* [capacity] engine precision, or NULL: miss_uniform serves every track      */
    double         miss_uniform;
} ukfb_assign_in;
typedef struct ukfb_assign_out {     /* device pointers; any may be NULL, not all */
    int32_t*  assign;                /* [capacity]            */
    int32_t*  owner;                 /* [scenes][candidates]  */
    double*   objective;             /* [scenes]              */
    uint32_t* scene_status;          /* [scenes]              */
} ukfb_assign_out;
int ukfb_assign_scenes_dev(ukfb_engine* e, const ukfb_assign_in* in, const ukfb_assign_out* out);
/* host arrays of doubles: cost [candidates][capacity], miss [capacity] or NULL, scene_start [scenes + 1] or NULL; assign is
 * filled with -1 where no scene covers a slot; any output may be NULL, not all.  Synchronises. */
int ukfb_assign_scenes(ukfb_engine* e, int candidates, const double* cost, int scenes, const int32_t* scene_start,
                       int tracks_per_scene, double gate, const double* miss, double miss_uniform, int32_t* assign, int32_t* owner,
                       double* objective, uint32_t* scene_status);

#ifdef __cplusplus
}
#endif

#endif /* UKF_BATCH_ASSIGN_H */
