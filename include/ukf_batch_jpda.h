/* ukf_batch_jpda.h -- joint probabilistic data association: the exact association marginals across the filters of a SCENE,
 * and the sensor-frame update with GIVEN weights.  An extension of ukf_batch.h (same library, same engine handle, same
 * conventions) in a header of its own: ukf_batch.h and the binding's table for it (abi.py) are pinned entry point by entry
 * point, so what is added beside them is declared beside them -- here, and in abi_jpda.py, which tests/test_jpda_host.py holds
 * to this header type by type.  Plain C99. */
#ifndef UKF_BATCH_JPDA_H
#define UKF_BATCH_JPDA_H

#include "ukf_batch.h"
#include "ukf_batch_pda.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ukfb_update_pda_dev (ukf_batch_pda.h) is soft but PER FILTER: each filter spreads its update over its gated candidates as if
 * no other track existed, so two tracks both lean on one return.  ukfb_assign_scenes_dev (ukf_batch_assign.h) is joint but
 * HARD.  JPDA is both: beta_ik is the posterior probability that detection k belongs to track i, summed over all JOINT EVENTS
 * in which no detection serves two tracks.  The chain, all on the device and on the engine's stream:
 *   ukfb_update_pda_dev(commit = 0)  ->  maha, loglik (and the per-filter beta, beta0)
 *   ukfb_jpda_scenes_dev             ->  beta, beta0 overwritten with the joint marginals, scene by scene
 *   ukfb_update_weighted_dev         ->  the PDA combination with those weights, committed
 *
 * ---- ukfb_jpda_scenes_dev: the marginals of every scene -------------------------------------------------------------------
 * SCENE s covers the engine slots [a, b), T = b - a tracks, and K = candidates detections: candidate k of every filter of the
 * scene is the scene's detection k, exactly as for ukfb_assign_scenes_dev:
 *   ragged mode:  scene_start_dev, int32 [scenes + 1], ascending; a = scene_start[s], b = scene_start[s + 1];
 *   uniform mode (scene_start_dev == NULL): tracks_per_scene = T0 in 1 ... UKFB_JPDA_MAX_TRACKS, scene s is
 *                 [s T0, min((s + 1) T0, capacity)), scenes <= ceil(capacity / T0).
 * INPUTS: loglik_dev [candidates][capacity] in engine precision, the loglik an association or PDA call wrote; maha_dev, the
 * same shape, or NULL; gate, a field of this call, not cfg.gate_chi2: < 0 or NaN means no gate, and maha_dev == NULL with
 * gate >= 0 is UKFB_ERR_INVALID_ARG; model_uniform / model_dev [capacity] with the meaning of ukfb_associate_in.model_dev (the
 * sensor model per track: it decides m, and an id this engine does not have counts as m = 3, as the PDA kernel takes it); the
 * rule of ukfb_update_pda_dev.  The host forms ln P_D and a_0 = ln lambda_m + ln(1 - P_D P_G,m) for m = 1 and m = 3 in double
 * and rounds them to the engine's precision, exactly as ukfb_update_pda_dev does.
 * RULES: a pair (i, k) is ALLOWED iff loglik is finite and, with a gate, maha is finite and <= gate.  For an allowed pair
 * l_ik = (ln P_D + double(loglik)) - a_0(m_i), formed in double in that order, and
 * psi_ik = exp(min(l_ik, UKFB_JPDA_LOG_RATIO_MAX)); a forbidden pair has psi_ik = 0.  The cap keeps every sum finite (six
 * factors of e^100 times at most 33^6 events stay inside the fp64 range); no lower cap is needed, the all-miss event has
 * weight 1 and so Z >= 1.  fp32 inputs are promoted to double exactly: the solve is fp64 for every engine precision.
 * DEFINITION: a JOINT EVENT gives every track at most one allowed detection and every detection at most one track; its weight
 * is the product of its psi; Z is the sum over all events.  beta_ik = (weight of the events containing (i, k)) / Z,
 * beta_i0 = (weight of the events in which track i has no detection) / Z.  A track with no allowed pair gets beta_i0 = 1 and
 * does not affect its neighbours.  The marginals are EXACT (a sum over subsets of the scene's tracks, not a sample and not
 * belief propagation), which is why a scene holds at most UKFB_JPDA_MAX_TRACKS tracks.
 * OUTPUTS (any may be NULL, not all): beta [candidates][capacity], engine precision: the marginal of an allowed pair, exactly 0
 * where loglik is finite but the pair is forbidden, NaN where loglik is not finite -- the convention of ukfb_pda_out.beta;
 * beta0 [capacity]; free [scenes][candidates], always double: the probability that detection k belongs to no track,
 * 1 - sum_i beta_ik (where new tracks start); log_z [scenes], always double: ln Z; scene_status [scenes] uint32:
 * UKFB_JPDA_OK, UKFB_JPDA_BAD_SCENE (a < 0, b > capacity, b < a or T > 32: the segment rule of ukfb_assign_scenes_dev; the
 * offsets live on the device, so the kernel does not trust them) or UKFB_JPDA_TOO_LARGE (a well-formed segment of 7 ... 32
 * tracks).  Bad and too-large scenes write their status and NOTHING ELSE, and slots outside every scene are not written:
 * beta and beta0 may therefore be THE VERY ARRAYS the PDA call filled, so that too-large scenes and uncovered slots keep their
 * per-filter PDA weights.  The host-array form knows the offsets and refuses bad ones with UKFB_ERR_OUT_OF_RANGE before any
 * launch.
 * The call is READ-ONLY on the engine, bit for bit, stream-ordered on the engine's stream, allocates nothing at call time, and
 * is DETERMINISTIC: the same inputs give the same bits, whatever the scene's position in its workgroup.  Device groups: per
 * shard through ukfb_group_shard.
 * ARGUMENT ERRORS, decided on the host before any launch, nothing written: a NULL rule, a rule value outside its range,
 * P_D P_G >= 1 for either m, a NULL in or loglik, every output NULL, gate >= 0 without maha: UKFB_ERR_INVALID_ARG; candidates
 * outside 1 ... 32, tracks_per_scene outside 1 ... 6 in uniform mode, scenes < 0 or more than the mode admits (ragged:
 * capacity + 1, empty scenes included): UKFB_ERR_OUT_OF_RANGE.  scenes = 0 is UKFB_OK and launches nothing.
 *
 * ---- ukfb_update_weighted_dev: the PDA combination with weights that are READ, not computed -------------------------------
 * The shared-h sensor-frame update of ukfb_update_pda_dev: the same ukfb_associate_in (a non-zero point_per_candidate is
 * UKFB_ERR_INVALID_ARG), and weight_dev [candidates][capacity] in engine precision.  Per filter:
 *   1. steps 1 - 2 of ukf_batch_pda.h unchanged: z-bar, S = Ls Ls^T, Y, and per candidate nu_k, y_k, d^2_k;
 *   2. w_k = weight_k if the candidate is scored with a finite d^2_k and the weight is finite and > 0, else w_k = 0;
 *      cfg.gate_chi2 PLAYS NO PART: whoever made the weights did the gating.  n_used = the number of w_k > 0;
 *   3. s = sum w_k, c = max(1, s): the weights are used as w_k / c (weight_used), so that a sum that rounding pushed above 1 is
 *      normalised; beta_0 = 1 - s / c;
 *   4. y-bar = sum w y / c, nu-bar likewise (innov_comb), P_y = sum w y y^T / c - y-bar y-bar^T, M = (s / c) I - P_y;
 *   5. Sigma~ = Sigma - Y M Y^T, delta = Y y-bar, (mu, Sigma) = applyDelta(mu, Sigma~, delta).
 * weight_used follows beta's convention: 0 for a finite candidate that is not used, NaN for one that is not scored.
 * STATUS and refusals are those of ukf_batch_pda.h with "G is empty" read as "no weight used": REJECTED_GATE when some
 * candidate is finite and no weight is used: the state is kept bit for bit, beta_0 = 1, innov_comb = 0.  commit = 0 is
 * READ-ONLY, bit for bit.  No filter ever changes a bit of another.
 *
 * Out of scope: scenes over 6 tracks (approximate marginals by belief propagation); packing several small scenes into one
 * wavefront; per-hypothesis candidates; bearings on S^2; fusing the marginals into the update kernel; K-best assignments;
 * group fan-out calls. */
#define UKFB_JPDA_MAX_TRACKS 6
#define UKFB_JPDA_LOG_RATIO_MAX 100.0
enum { UKFB_JPDA_OK = 0, UKFB_JPDA_BAD_SCENE = 1, UKFB_JPDA_TOO_LARGE = 2 };
typedef struct ukfb_jpda_in {        /* device pointers; gate is a host double, by value */
    const void*    loglik_dev;       /* [candidates][capacity] engine precision                                    */
    const void*    maha_dev;         /* [candidates][capacity] engine precision, or NULL (then gate must be off)   */
    int            candidates;       /* K = 1 ... UKFB_ASSOCIATE_MAX_CANDIDATES                                    */
    int            scenes;           /* >= 0                                                                       */
    const int32_t* scene_start_dev;  /* [scenes + 1] ascending slot offsets, or NULL: uniform mode                 */
    int            tracks_per_scene; /* uniform mode: T0 = 1 ... UKFB_JPDA_MAX_TRACKS (ragged mode: ignored)       */
    double         gate;             /* >= 0: pairs with maha > gate are forbidden; < 0 (or NaN): no gate          */
    int            model_uniform;    /* the sensor model of every track, unless model_dev is given                 */
    const int32_t* model_dev;        /* [capacity] sensor model per track, or NULL                                 */
} ukfb_jpda_in;
typedef struct ukfb_jpda_out {       /* device pointers; any may be NULL, not all */
    void*     beta;                  /* [candidates][capacity] engine precision */
    void*     beta0;                 /* [capacity]             engine precision */
    double*   free;                  /* [scenes][candidates]   */
    double*   log_z;                 /* [scenes]               */
    uint32_t* scene_status;          /* [scenes]               */
} ukfb_jpda_out;
int ukfb_jpda_scenes_dev(ukfb_engine* e, const ukfb_jpda_in* in, const ukfb_pda_rule* rule, const ukfb_jpda_out* out);
/* host arrays of doubles: loglik, maha (or NULL) [candidates][capacity], scene_start [scenes + 1] or NULL, model_per_filter
 * [capacity] or NULL; beta and beta0 are filled with NaN where no good scene covers a slot; any output may be NULL, not all.
 * Synchronises. */
int ukfb_jpda_scenes(ukfb_engine* e, int candidates, const double* loglik, const double* maha, int scenes, const int32_t* scene_start,
                     int tracks_per_scene, double gate, int model, const int32_t* model_per_filter, const ukfb_pda_rule* rule,
                     double* beta, double* beta0, double* free, double* log_z, uint32_t* scene_status);

typedef struct ukfb_weighted_out {  /* device pointers, engine precision; any may be NULL */
    void *z_pred, *S;               /* [capacity][3], [capacity][9]   as ukfb_pda_out */
    void *innov, *maha, *loglik;    /* [candidates][capacity][3], [candidates][capacity] x 2 */
    void *weight_used;              /* [candidates][capacity]   w_k / c */
    void *beta0;                    /* [capacity]               1 - s / c */
    void *innov_comb;               /* [capacity][3]            sum_k w_k nu_k / c, first m entries (rest 0) */
    int32_t* n_used;                /* [capacity]               the number of weights used */
    uint32_t* status;
} ukfb_weighted_out;
/* out may be NULL with commit = 1 */
int ukfb_update_weighted_dev(ukfb_engine* e, int model_uniform, const ukfb_associate_in* in, const void* weight_dev, int commit,
                             const ukfb_weighted_out* out);
/* host arrays of doubles, shaped as for ukfb_update_pda: z [candidates][capacity][3], weight [candidates][capacity]; any output
 * may be NULL.  Synchronises. */
int ukfb_update_weighted(ukfb_engine* e, int model, const int32_t* model_per_filter, int candidates, const double* z, const double* Q,
                         const double* mount, const double* mount_uniform, const double* point, const double* point_uniform,
                         const double* weight, int commit, double* z_pred, double* S, double* innov, double* maha, double* loglik,
                         double* weight_used, double* beta0, double* innov_comb, int32_t* n_used, uint32_t* status);

#ifdef __cplusplus
}
#endif

#endif /* UKF_BATCH_JPDA_H */
