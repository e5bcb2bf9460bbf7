// ukf_host.hpp -- the engine's host decisions as pure functions of plain values: configuration checks, process-noise
// classification, measurement-model checks, shard ranges and the event owner pass, multi-cycle plans, packed covariances, workspace sizing, the filter lifecycle's checks and geometry, the delayed-measurement
// update's checks, geometry and lag rule, the relative-measurement update's checks, models and map, the robust update's rule, the late
// sensor-frame sample's checks, input record and map, the probabilistic data association's rule, the joint association's checks and segment rule, and the kernel level of a launch.  No HIP dependency: tests/cpp/host_logic.cpp compiles it with g++ under ASan / UBSan.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../../include/ukf_batch.h"
#include "../../include/ukf_batch_relative.h"
#include "../../include/ukf_batch_robust.h"
#include "../../include/ukf_batch_delayed_sensor.h"
#include "../../include/ukf_batch_pda.h"
#include "../../include/ukf_batch_assign.h"
#include "../../include/ukf_batch_jpda.h"

#if defined(__HIP__)
#define UKFB_HD __host__ __device__ __forceinline__
#else
#define UKFB_HD inline
#endif

#ifndef UKFB_MAX_MULTI_CYCLES
#define UKFB_MAX_MULTI_CYCLES 32   // cycles of one multi-cycle launch with a schedule (the host splits longer ones)
#endif

namespace ukfb {

struct Verdict {   // a return code and, unless UKFB_OK, the text ukfb_last_error() reports
    int rc = UKFB_OK;
    const char* msg = nullptr;
};
// two clauses many checks have: a flag is 0 or 1; a call that commits nothing needs somewhere to write
constexpr bool zero_or_one(int v) { return v == 0 || v == 1; }
inline Verdict nothing_to_compute(int commit, bool has_output) {
    if (commit == 0 && !has_output) return {UKFB_ERR_INVALID_ARG, "commit = 0 with every output NULL: nothing to compute"};
    return {};
}

// ---- configuration ------------------------------------------------------------------------------------------------------
// generic_f64: the fp64 one-wavefront-per-filter layouts are built (make GENERIC_F64=1)
inline bool layout_supported(int precision, int lanes_per_filter, bool generic_f64) {
    if (precision != UKFB_F64 && precision != UKFB_F32) return false;
    if (lanes_per_filter == 0 || lanes_per_filter == 16) return true;
    if (lanes_per_filter != 32 && lanes_per_filter != 64) return false;
    return precision == UKFB_F32 || generic_f64;
}

// ukfb_set_config's checks, in their order; c is normalised in place (lanes_per_filter 0 = 16)
inline Verdict check_config(int precision, bool generic_f64, ukfb_config& c) {
    if (c.lanes_per_filter == 0) c.lanes_per_filter = 16;
    if (c.lanes_per_filter != 16 && c.lanes_per_filter != 32 && c.lanes_per_filter != 64)
        return {UKFB_ERR_INVALID_ARG, "lanes_per_filter must be 16, 32 or 64"};
    if (!layout_supported(precision, c.lanes_per_filter, generic_f64))
        return {UKFB_ERR_INVALID_ARG, "lanes_per_filter 32 / 64 in fp64 is a diagnostic build option (make GENERIC_F64=1)"};
    if (c.mean_max_iter < 1) return {UKFB_ERR_INVALID_ARG, "mean_max_iter must be >= 1"};
    if (!zero_or_one(c.wide_arithmetic)) return {UKFB_ERR_INVALID_ARG, "wide_arithmetic must be 0 or 1"};
    if (!zero_or_one(c.full_update_check)) return {UKFB_ERR_INVALID_ARG, "full_update_check must be 0 or 1"};
    if (c.wide_arithmetic && precision == UKFB_F32 && c.lanes_per_filter != 16)
        return {UKFB_ERR_INVALID_ARG, "wide_arithmetic runs on the tuned layout only (lanes_per_filter 16)"};
    return {};
}

// ---- process noise (D x D, row-major) -----------------------------------------------------------------------------------
// Positive semidefinite? -- of the symmetric matrix the kernels use (they read the lower triangle).  Cholesky with a tolerance: a pivot
// below -tol fails; a pivot within tol must head a column of zeros (a zero direction, e.g. the all-zero default noise).
inline bool is_psd(const double* A, int D) {
    std::vector<double> L(size_t(D) * D, 0.0);
    double dmax = 0.0;
    for (int i = 0; i < D; ++i) dmax = std::max(dmax, std::fabs(A[size_t(i) * D + i]));
    const double tol = 1e-12 * dmax;
    for (int k = 0; k < D; ++k) {
        double x = A[size_t(k) * D + k];
        if (!std::isfinite(x)) return false;
        for (int j = 0; j < k; ++j) x -= L[size_t(k) * D + j] * L[size_t(k) * D + j];
        if (x < -tol) return false;
        const bool zero = x <= tol;
        const double d = zero ? 0.0 : std::sqrt(x);
        L[size_t(k) * D + k] = d;
        for (int i = k + 1; i < D; ++i) {
            double v = A[size_t(i) * D + k];
            if (!std::isfinite(v)) return false;
            for (int j = 0; j < k; ++j) v -= L[size_t(i) * D + j] * L[size_t(k) * D + j];
            if (zero) {
                if (std::fabs(v) > std::sqrt(tol * std::max(dmax, 1e-300)) + 1e-300) return false;
                L[size_t(i) * D + k] = 0.0;
            } else {
                L[size_t(i) * D + k] = v / d;
            }
        }
    }
    return true;
}

// rows / columns 0..5 are zero outside their own 3x3 diagonal block (the blocks the prediction rotates)
inline bool rotated_blocks_uncoupled(const double* A, int D) {
    for (int r = 0; r < D; ++r)
        for (int c = 0; c < 6; ++c)
            if (r / 3 != c / 3 && (A[size_t(r) * D + c] != 0.0 || A[size_t(c) * D + r] != 0.0)) return false;
    return true;
}

// blocks [0:3,0:3] and [3:6,3:6], the ones predictionStepImpl rotates (PoseUKF.cpp:184-185, OrientationUKF.cpp:84-85), are s * I
inline bool rotated_blocks_isotropic(const double* A, int D) {
    bool iso = true;
    for (int b = 0; b < 6; b += 3)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                const double v = A[size_t(b + r) * D + (b + c)];
                iso = iso && (r == c ? v == A[size_t(b) * D + b] : v == 0.0);
            }
    return iso;
}

// ukfb_config::full_update_check: the host-side condition of the short update factorisation -- the batch-uniform process noise as the
// prediction adds it is positive semidefinite.  The prediction rotates the diagonal blocks [0:3] and [3:6] and leaves every other
// entry raw (PoseUKF.cpp:184-185, OrientationUKF.cpp:84-85); that is the congruence blockdiag(rot, rot, I) R blockdiag(rot, rot, I)^T,
// which keeps R semidefinite for any rot (non-unit quaternions included), only when rows / columns 0..5 are zero outside their own
// 3x3 diagonal block.  A semidefinite R with such cross terms can turn indefinite, so it keeps the complete factorisation.  Scaling
// by dt / dt^2 keeps semidefiniteness; Pose acceleration branch: the unrotated R with the velocity block replaced by 2 acc.cov
// (PoseUKF.cpp:190-191) must be semidefinite as well.
inline bool short_update_ok(int model, int D, const double* R, const double* acc_cov) {
    if (!rotated_blocks_uncoupled(R, D) || !is_psd(R, D)) return false;
    if (model != UKFB_MODEL_POSE) return true;
    std::vector<double> Ra(R, R + size_t(D) * D);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Ra[size_t(6 + r) * D + (6 + c)] = 2.0 * acc_cov[r * 3 + c];
    return is_psd(Ra.data(), D);
}

// ---- measurement models -------------------------------------------------------------------------------------------------
inline bool meas_model_ok(int engine_model, int m) {
    if (engine_model == UKFB_MODEL_POSE) return m >= UKFB_MEAS_POS3 && m <= UKFB_MEAS_ANGVEL3;
    return m == UKFB_MEAS_ORIENT_BODYVEL3;
}

// Class of a filter's update in a call: 0 = none (negative / invalid model id: prediction only), 1 = closed form (the eight
// linear sub-state selections of PoseUKF), 2 = sigma-point path (PoseUKF OrientationMeasurement, OrientationUKF body velocity)
UKFB_HD int update_class(int engine_model, int mid) {
    if (engine_model == UKFB_MODEL_POSE) return (mid < 0 || mid > 8) ? 0 : ((mid == 3) ? 2 : 1);
    return (mid == 9) ? 2 : 0;
}

// ---- shards of a device group -------------------------------------------------------------------------------------------
inline int shard_range(int64_t total, int n_shards, int shard, int64_t* first, int64_t* count) {
    if (total < 0 || n_shards <= 0 || shard < 0 || shard >= n_shards) return UKFB_ERR_INVALID_ARG;
    const int64_t base = total / n_shards, extra = total % n_shards;
    if (count) *count = base + (shard < extra ? 1 : 0);
    if (first) *first = shard * base + std::min<int64_t>(shard, extra);
    return UKFB_OK;
}

// [first, first + count) of the batch cut by the shard [shard_first, shard_first + shard_count): (offset inside the caller's
// arrays, offset inside the shard, length)
struct Cut { int64_t src, dst, len; };
inline Cut cut(int64_t shard_first, int64_t shard_count, int64_t first, int64_t count) {
    const int64_t lo = std::max(first, shard_first), hi = std::min(first + count, shard_first + shard_count);
    return {lo - first, lo - shard_first, std::max<int64_t>(0, hi - lo)};
}

// The owner pass of ukfb_group_process_events: owner[i] = the shard of filter[i], counts[r] = the events of shard r (shards as
// shard_range cuts them, at most 255).  UKFB_ERR_OUT_OF_RANGE for an index outside [0, total).
inline int route_events(const int64_t* filter, int64_t n_events, int64_t total, const int64_t* first, const int64_t* count,
                        size_t n_shards, uint8_t* owner, size_t* counts) {
    std::fill(counts, counts + n_shards, size_t(0));
    const double per_filter = double(n_shards) / double(total);   // (a multiply, not a 64-bit division per event)
    for (int64_t i = 0; i < n_events; ++i) {
        const int64_t f = filter[i];
        if (f < 0 || f >= total) return UKFB_ERR_OUT_OF_RANGE;
        size_t r = std::min(n_shards - 1, size_t(double(f) * per_filter));   // shards differ by one filter at most: off by one at most
        while (f < first[r]) --r;
        while (f >= first[r] + count[r]) ++r;
        owner[size_t(i)] = uint8_t(r);
        ++counts[r];
    }
    return UKFB_OK;
}

// ---- multi-cycle calls --------------------------------------------------------------------------------------------------
inline Verdict check_cycle_args(int cycles, int slots, int first_slot) {
    if (cycles < 0 || slots < 1 || first_slot < 0 || first_slot >= slots)
        return {UKFB_ERR_INVALID_ARG, "cycles >= 0, slots >= 1, 0 <= first_slot < slots"};
    return {};
}

// ---- innovation statistics (ukfb_innovation_dev, ukfb_select_candidates_dev) ---------------------------------------------
constexpr int MAX_CANDIDATES = 32;   // two passes of the sixteen lanes of a filter's row (ukf_innovation.hpp)
// per_filter_models: the model ids come from a device array (checked per filter by the kernel: an id the engine's model does
// not have marks the filter INACTIVE, as in ukfb_update_dev); otherwise the one id must be the engine model's.
inline Verdict check_innovation_args(int engine_model, bool per_filter_models, int meas_model_uniform, int candidates, bool has_z,
                                     bool has_Q, const ukfb_innovation_out* out) {
    if (candidates < 1 || candidates > MAX_CANDIDATES) return {UKFB_ERR_INVALID_ARG, "candidates must be 1 ... 32"};
    if (!has_z || !has_Q) return {UKFB_ERR_INVALID_ARG, "z and Q must not be NULL"};
    if (!out) return {UKFB_ERR_INVALID_ARG, "out must not be NULL"};
    if (!out->z_pred && !out->S && !out->innov && !out->maha && !out->loglik && !out->best && !out->status)
        return {UKFB_ERR_INVALID_ARG, "every output of ukfb_innovation_out is NULL: nothing to compute"};
    if (!per_filter_models && !meas_model_ok(engine_model, meas_model_uniform))
        return {UKFB_ERR_WRONG_MODEL, "measurement model id not valid for this engine"};
    return {};
}
inline Verdict check_select_args(int engine_model, bool per_filter_models, int meas_model_uniform, int candidates, bool has_best,
                                 bool has_z, bool has_z_sel) {
    if (candidates < 1 || candidates > MAX_CANDIDATES) return {UKFB_ERR_INVALID_ARG, "candidates must be 1 ... 32"};
    if (!has_best || !has_z || !has_z_sel) return {UKFB_ERR_INVALID_ARG, "best, z and z_sel must not be NULL"};
    if (!per_filter_models && !meas_model_ok(engine_model, meas_model_uniform))
        return {UKFB_ERR_WRONG_MODEL, "measurement model id not valid for this engine"};
    return {};
}

// ---- the row layout of the feature kernels (ukf_row.hpp) ---------------------------------------------------------------------
// One filter per 16-lane row, ROW_FILTERS_PER_GROUP rows per workgroup (one wavefront), every filter with a slice of the
// workgroup's dynamic LDS; ROW_LS: the stride of the columns of a factor and of the rows of a delta table in that slice.
constexpr int ROW_LS = 14, ROW_FILTERS_PER_GROUP = 4;
struct RowGeometry {
    int64_t grid;    // workgroups of four filters
    int lds_bytes;   // dynamic LDS of a workgroup
};
// filter_scalars: LDS of one filter in scalars of the compute type (the *_filter_scalars functions below); compute_size: bytes
// of the scalar the kernel computes in (8: fp64 engines and fp32 engines with wide_arithmetic, else 4)
inline RowGeometry row_geometry(int filter_scalars, int64_t capacity, size_t compute_size) {
    return {(capacity + ROW_FILTERS_PER_GROUP - 1) / ROW_FILTERS_PER_GROUP, int(size_t(ROW_FILTERS_PER_GROUP) * filter_scalars * compute_size)};
}
// A filter's slice is described once: a *_map(S, D) below lists its regions in their order, as offsets in scalars of the compute
// type.  The kernel reads the map as a constexpr object, the host sizes the launch from its PF (*_filter_scalars: -1 where a
// filter does not fit a row).  Every scalar a kernel reads is one it wrote: the pads are never read
// (tests/test_gpu_feature_lds_leftovers.py holds that, family by family, against NaN, Inf and zero leftovers).
constexpr bool row_fits(int S, int D) { return ROW_LS >= D && S <= 16 && D + 1 <= 16; }   // a filter fits one row: every kernel asserts it
struct RowSlice {   // bump counter over a slice
    int used = 0;
    constexpr int take(int n) {
        const int at = used;
        used += n;
        return at;
    }
    // rounded up to a multiple of four, so that every filter's slice starts 16-byte aligned in either precision
    constexpr int size() const { return (used + 3) / 4 * 4; }
    // the recurring regions
    constexpr void factor(int D, int& fac, int& rsp) {   // D * ROW_LS factor columns, then 16 reciprocal pivots
        fac = take(D * ROW_LS);
        rsp = take(16);
    }
    constexpr int table(int D) { return take((2 * D + 1) * ROW_LS); }   // the delta table of 2 D + 1 rows
    constexpr void record(int D, int& mean, int& packed) {   // a mean padded to 16, then a packed covariance padded to even
        mean = take(16);
        packed = take((D * (D + 1) / 2 + 1) / 2 * 2);
    }
    constexpr int rotation() { return take(10); }         // a rotation matrix: 9 (+ 1)
    constexpr int sink() { return take(16); }             // the sink of lane-predicated stores
    constexpr int rows(int D) { return take(D * ROW_LS); }   // D parked rows
};

// ---- filter banks (ukfb_bank_weights_dev, ukfb_bank_combine_dev, ukfb_bank_mix_dev) ---------------------------------------
// An engine of `capacity` filters read as capacity / M tracks of M hypotheses, track-major (hypothesis j of track t = filter
// t * M + j).  One track per 16-lane row, four per wavefront, one wavefront per workgroup (ukf_bank.hpp).
constexpr int BANK_MIN_HYPOTHESES = 2, BANK_MAX_HYPOTHESES = 8, BANK_TRACKS_PER_GROUP = 4;
constexpr double BANK_TRANSITION_ROW_TOL = 1e-12;
inline Verdict check_bank_args(int hypotheses, int64_t capacity) {
    if (hypotheses < BANK_MIN_HYPOTHESES || hypotheses > BANK_MAX_HYPOTHESES)
        return {UKFB_ERR_INVALID_ARG, "hypotheses per track must be 2 ... 8"};
    if (capacity < 0 || capacity % hypotheses != 0)
        return {UKFB_ERR_INVALID_ARG, "the engine's capacity is not a multiple of the hypotheses per track"};
    return {};
}
// row-stochastic [M][M]: finite, non-negative, every row sums to 1 within BANK_TRANSITION_ROW_TOL
inline Verdict check_bank_transition(const double* P, int hypotheses) {
    if (!P) return {UKFB_ERR_INVALID_ARG, "transition must not be NULL"};
    for (int j = 0; j < hypotheses; ++j) {
        double sum = 0.0;
        for (int i = 0; i < hypotheses; ++i) {
            const double v = P[size_t(j) * hypotheses + i];
            if (!std::isfinite(v) || v < 0.0) return {UKFB_ERR_INVALID_ARG, "transition entries must be finite and non-negative"};
            sum += v;
        }
        if (!(std::fabs(sum - 1.0) <= BANK_TRANSITION_ROW_TOL))
            return {UKFB_ERR_INVALID_ARG, "every row of transition must sum to 1 (within 1e-12)"};
    }
    return {};
}
// LDS of one track, in scalars of the compute type: the M records (mean, packed covariance), the M deltas to the mixture's
// mean with their weights, and one output record.  Every scalar a kernel reads is one it wrote
// (tests/test_gpu_feature_lds_leftovers.py::test_bank).
UKFB_HD int bank_track_scalars(int S, int D, int hypotheses) {
    const int PK = D * (D + 1) / 2;
    return (hypotheses * (S + PK + D + 1) + S + PK + 1) / 2 * 2;
}
constexpr int BANK_GROUP_SCALARS = 64;   // per workgroup, in front of the tracks: the transition matrix
struct BankGeometry {
    int64_t tracks, grid;   // grid: workgroups of BANK_TRACKS_PER_GROUP tracks
    int lds_bytes;          // dynamic LDS of a workgroup
};
// compute_size: bytes of the scalar the kernel computes in (8: fp64 engines and fp32 engines with wide_arithmetic, else 4)
inline BankGeometry bank_geometry(int S, int D, int hypotheses, int64_t capacity, size_t compute_size) {
    const int64_t tracks = capacity / hypotheses;
    return {tracks, (tracks + BANK_TRACKS_PER_GROUP - 1) / BANK_TRACKS_PER_GROUP,
            int((size_t(BANK_GROUP_SCALARS) + size_t(BANK_TRACKS_PER_GROUP) * bank_track_scalars(S, D, hypotheses)) * compute_size)};
}

// ---- fixed-interval smoothing (ukfb_history_push_dev, ukfb_smooth_dev) ---------------------------------------------------
// A window of `steps` consecutive slots of a ring of `slots`, oldest first: step c lives in slot (first_slot + c) % slots.  The
// backward pass has steps - 1 steps; a launch covers at most SMOOTH_MAX_BACK of them (their dt travel in the kernel arguments)
// and the next launch starts from the smoothed record the previous one stored.
constexpr int SMOOTH_MAX_BACK = 32;
inline Verdict check_history_args(int slots, int slot, bool has_mu_hist, bool has_cov_hist) {
    if (slots < 1 || slot < 0 || slot >= slots) return {UKFB_ERR_INVALID_ARG, "slots >= 1, 0 <= slot < slots"};
    if (!has_mu_hist || !has_cov_hist) return {UKFB_ERR_INVALID_ARG, "mu_hist and cov_hist must not be NULL"};
    return {};
}
inline Verdict check_smooth_args(int steps, int slots, int first_slot, bool has_dt, bool has_mu_hist, bool has_cov_hist, bool has_mu_out) {
    if (slots < 1 || steps < 2 || steps > slots) return {UKFB_ERR_INVALID_ARG, "2 <= steps <= slots"};
    if (first_slot < 0 || first_slot >= slots) return {UKFB_ERR_INVALID_ARG, "0 <= first_slot < slots"};
    if (!has_dt) return {UKFB_ERR_INVALID_ARG, "dt must not be NULL"};
    if (!has_mu_hist || !has_cov_hist || !has_mu_out) return {UKFB_ERR_INVALID_ARG, "mu_hist, cov_hist and mu_out must not be NULL"};
    return {};
}
struct SmoothLaunch {
    int top_step, top_slot;   // the step whose smoothed record the launch starts from, and its slot
    int back;                 // backward steps: the launch writes steps top_step - 1 ... top_step - back
    int dt_first;             // backward step k of the launch redoes the prediction of dt[dt_first - k]
    bool first;               // the call's first launch: starts from the filtered record of the last step
};
struct SmoothPlan {
    int steps, slots, first_slot;
    SmoothPlan(int steps_, int slots_, int first_slot_) : steps(steps_), slots(slots_), first_slot(first_slot_) {}
    int launches() const { return (steps - 1 + SMOOTH_MAX_BACK - 1) / SMOOTH_MAX_BACK; }
    SmoothLaunch operator[](int k) const {
        const int top = steps - 1 - k * SMOOTH_MAX_BACK;
        return {top, int((int64_t(first_slot) + top) % slots), std::min(SMOOTH_MAX_BACK, top), top - 1, k == 0};
    }
};
struct SmoothMap {
    int LS, FAC, RSP, TAB, GM, MM, CSM, CSP, MUF, PKF, ROT, DUM, SMR, MUP, PF;
};
constexpr SmoothMap smooth_map(int, int D) {
    RowSlice s;
    SmoothMap m{};
    m.LS = ROW_LS;
    s.factor(D, m.FAC, m.RSP);
    m.TAB = s.table(D);   // G (D * LS) and M (D * LS) alias it
    m.GM = m.TAB; m.MM = m.TAB + D * m.LS;
    s.record(D, m.CSM, m.CSP);   // the chain's record
    s.record(D, m.MUF, m.PKF);   // the filtered record
    m.ROT = s.rotation();
    m.DUM = s.sink();
    m.SMR = s.rows(D);     // the rows of Sigma^-, parked between its factorisation and M
    m.MUP = s.take(16);    // mu^-, parked across the solves
    m.PF = s.size();
    return m;
}
constexpr int smooth_filter_scalars(int S, int D) { return S > 16 ? -1 : smooth_map(S, D).PF; }
inline RowGeometry smooth_geometry(int S, int D, int64_t capacity, size_t compute_size) { return row_geometry(smooth_filter_scalars(S, D), capacity, compute_size); }

// ---- forecast (ukfb_forecast_dev) -------------------------------------------------------------------------------------------
// `steps` predictions chained from a start record into a window of a ring of `slots`: step c lives in slot
// (first_slot + c) % slots.  One launch: the time steps (or stamps) of all steps travel in the kernel arguments, so a call
// covers at most FORECAST_MAX_STEPS of them and a longer horizon is chained by the caller.
constexpr int FORECAST_MAX_STEPS = UKFB_FORECAST_MAX_STEPS;
inline Verdict check_forecast_args(int steps, int slots, int first_slot, bool has_dt, bool has_ts, bool has_start_mu, bool has_start_cov,
                                   bool has_mu_out) {
    if (slots < 1 || steps < 1) return {UKFB_ERR_INVALID_ARG, "steps >= 1, slots >= 1"};
    if (first_slot < 0 || first_slot >= slots) return {UKFB_ERR_INVALID_ARG, "0 <= first_slot < slots"};
    if (has_dt == has_ts) return {UKFB_ERR_INVALID_ARG, "exactly one of dt and ts_us must be given"};
    if (has_start_mu != has_start_cov) return {UKFB_ERR_INVALID_ARG, "start_mu and start_cov must be both NULL or both given"};
    if (!has_mu_out) return {UKFB_ERR_INVALID_ARG, "mu_out must not be NULL"};
    if (steps > std::min(slots, FORECAST_MAX_STEPS))
        return {UKFB_ERR_OUT_OF_RANGE, "steps <= min(slots, 32): chain a longer horizon from the last slot of the call before"};
    return {};
}
constexpr int FORECAST_SLICE_PAD = 4;   // keeps the four slices of a workgroup on different banks in either precision
struct ForecastMap {
    int LS, FAC, RSP, TAB, CSM, CSP, ROT, DUM, PF;
};
constexpr ForecastMap forecast_map(int, int D) {
    RowSlice s;
    ForecastMap m{};
    m.LS = ROW_LS;
    s.factor(D, m.FAC, m.RSP);   // (the rows of Sigma^- are parked in the columns while the noise is added)
    m.TAB = s.table(D);
    s.record(D, m.CSM, m.CSP);   // the chain's record
    m.ROT = s.rotation();
    m.DUM = s.sink();
    s.take(FORECAST_SLICE_PAD);
    m.PF = s.size();
    return m;
}
constexpr int forecast_filter_scalars(int S, int D) { return S > 16 ? -1 : forecast_map(S, D).PF; }
inline RowGeometry forecast_geometry(int S, int D, int64_t capacity, size_t compute_size) { return row_geometry(forecast_filter_scalars(S, D), capacity, compute_size); }

// ---- joint state-block measurements (ukfb_update_state_dev) --------------------------------------------------------------
// A measurement is a sub-manifold of the state: the compound of the blocks a mask selects, in state order.  Every block but the
// OrientationState's gravity has three tangent dimensions, so tangent dimension t belongs to block t / 3 in both models.
constexpr int state_meas_blocks(int engine_model) { return engine_model == UKFB_MODEL_POSE ? 4 : 5; }
constexpr bool state_meas_mask_ok(int blocks, int64_t mask) { return mask > 0 && (mask >> blocks) == 0; }
// tangent dimensions of a mask (D: 12 / 13; the last block of OrientationState has one)
inline int state_meas_dim(int D, uint32_t mask) {
    int m = 0;
    for (int t = 0; t < D; ++t) m += int((mask >> (t / 3)) & 1u);
    return m;
}
// per_filter_masks: the masks come from a device array (checked per filter by the kernel: INACTIVE); otherwise the one mask must
// select at least one block and none the model does not have
inline Verdict check_state_meas_args(int engine_model, bool per_filter_masks, uint32_t mask_uniform, bool has_z, bool has_Qz,
                                     double state_inflation, double meas_inflation, int commit, const ukfb_state_meas_out* out) {
    if (!has_z || !has_Qz) return {UKFB_ERR_INVALID_ARG, "z and Qz must not be NULL"};
    if (!zero_or_one(commit)) return {UKFB_ERR_INVALID_ARG, "commit must be 0 or 1"};
    if (!(std::isfinite(state_inflation) && state_inflation >= 1.0) || !(std::isfinite(meas_inflation) && meas_inflation >= 1.0))
        return {UKFB_ERR_INVALID_ARG, "state_inflation and meas_inflation must be finite and >= 1"};
    if (!per_filter_masks && !state_meas_mask_ok(state_meas_blocks(engine_model), int64_t(mask_uniform)))
        return {UKFB_ERR_INVALID_ARG, "block_mask must select at least one block and none beyond the model's (Pose: 4, OrientationState: 5)"};
    return nothing_to_compute(commit, out && (out->maha || out->loglik || out->status));
}
struct StateMeasMap {
    int LS, FAC, RSP, TAB, YM, MUF, PKF, ZM, PKQ, DUM, PF;
};
constexpr StateMeasMap state_meas_map(int, int D) {
    RowSlice s;
    StateMeasMap m{};
    m.LS = ROW_LS;
    s.factor(D, m.FAC, m.RSP);
    m.TAB = s.table(D);   // the solved cross-covariance Y (D * LS) aliases it
    m.YM = m.TAB;
    s.record(D, m.MUF, m.PKF);   // the state: mean, a Sigma packed
    s.record(D, m.ZM, m.PKQ);    // the measurement: mean, b Qz packed
    m.DUM = s.sink();
    m.PF = s.size();
    return m;
}
constexpr int state_meas_filter_scalars(int S, int D) { return S > 16 ? -1 : state_meas_map(S, D).PF; }
inline RowGeometry state_meas_geometry(int S, int D, int64_t capacity, size_t compute_size) { return row_geometry(state_meas_filter_scalars(S, D), capacity, compute_size); }
// A base::samples::RigidBodyState record (49 scalars: position, orientation x y z w, velocity, angular velocity, then the four
// 3 x 3 covariances in that order) as a Pose measurement: z = the record's first 13 scalars as they are, Qz = the four blocks
// on the diagonal of a 12 x 12 matrix (row-major), zero elsewhere
inline void body_state_to_measurement(const double* rec, double* z, double* Qz) {
    for (int s = 0; s < 13; ++s) z[s] = rec[s];
    std::fill(Qz, Qz + 144, 0.0);
    for (int b = 0; b < 4; ++b)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Qz[(3 * b + r) * 12 + 3 * b + c] = rec[13 + 9 * b + 3 * r + c];
}

// ---- sensor-frame measurements (ukfb_update_sensor_dev) -------------------------------------------------------------------
// Measurement models with a mount (lever arm r, sensor -> body rotation qs) and / or a nav-frame point b: ids 0 ... 4 are the
// Pose engine's, 5 ... 7 the OrientationState engine's (UKFB_SENSOR_*).  Bit id of each set: the model reads that input.
constexpr int SENSOR_MODELS = 8;
constexpr unsigned SENSOR_READS_LEVER = 0x2fu;      // POSE_POSITION, POSE_RANGE, POSE_POINT, POSE_VELOCITY, ORIENT_VELOCITY
constexpr unsigned SENSOR_READS_ROTATION = 0x6cu;   // POSE_POINT, POSE_VELOCITY, ORIENT_VELOCITY, ORIENT_NAV_VECTOR
constexpr unsigned SENSOR_READS_POINT = 0x46u;      // POSE_RANGE, POSE_POINT, ORIENT_NAV_VECTOR
constexpr bool sensor_model_ok(int engine_model, int64_t id) {
    return engine_model == UKFB_MODEL_POSE ? (id >= UKFB_SENSOR_POSE_POSITION && id <= UKFB_SENSOR_POSE_NAV_VELOCITY)
                                           : (id >= UKFB_SENSOR_ORIENT_VELOCITY && id <= UKFB_SENSOR_ORIENT_SPECIFIC_FORCE);
}
// dimension of the measurement space (0: no such model)
constexpr int sensor_meas_dim(int64_t id) { return (id < 0 || id >= SENSOR_MODELS) ? 0 : (id == UKFB_SENSOR_POSE_RANGE ? 1 : 3); }
constexpr bool sensor_reads_lever(int64_t id) { return id >= 0 && id < SENSOR_MODELS && ((SENSOR_READS_LEVER >> id) & 1u) != 0; }
constexpr bool sensor_reads_rotation(int64_t id) { return id >= 0 && id < SENSOR_MODELS && ((SENSOR_READS_ROTATION >> id) & 1u) != 0; }
constexpr bool sensor_reads_point(int64_t id) { return id >= 0 && id < SENSOR_MODELS && ((SENSOR_READS_POINT >> id) & 1u) != 0; }
// The record of one filter's inputs as the kernel stages it: z (3), Q row-major (9), mount r then qs (7), point (3); entry i is
// read by model id iff sensor_input_used(id, i).  An entry that is not read is replaced by its neutral value (0; the w of qs: 1)
// before anything computes with it, so that it may hold anything, NaN included.
constexpr int SENSOR_INPUT_Z = 0, SENSOR_INPUT_Q = 3, SENSOR_INPUT_MOUNT = 12, SENSOR_INPUT_POINT = 19, SENSOR_INPUT_SCALARS = 22;
constexpr bool sensor_input_used(int64_t id, int i) {
    const int m = sensor_meas_dim(id);
    return i < 0 ? false
         : i < SENSOR_INPUT_Q ? i < m
         : i < SENSOR_INPUT_MOUNT ? ((i - SENSOR_INPUT_Q) / 3 < m && (i - SENSOR_INPUT_Q) % 3 < m)
         : i < SENSOR_INPUT_MOUNT + 3 ? sensor_reads_lever(id)
         : i < SENSOR_INPUT_POINT ? sensor_reads_rotation(id)
         : i < SENSOR_INPUT_SCALARS ? sensor_reads_point(id) : false;
}
constexpr double sensor_input_neutral(int i) { return i == SENSOR_INPUT_MOUNT + 6 ? 1.0 : 0.0; }
// per_filter_models: the ids come from a device array (checked per filter by the kernel: an id the engine's model does not have
// marks the filter INACTIVE); otherwise the one id must be the engine model's
// The clauses the sensor-frame update, the bearing update and the association share, in their order; what only the
// association has (K candidates, a point per candidate) is neutral in the other two.  The candidate range is judged first and
// alone decides UKFB_ERR_OUT_OF_RANGE; then the NULL rules (point_per_candidate needs point_dev: there is no uniform value for K
// points), then the uniform id, then "nothing to compute".
struct SensorCall {
    int candidates;
    bool has_z, has_Q;
    int q_is_uniform, point_per_candidate;
    bool has_point;
};
inline Verdict check_sensor_call(const SensorCall& c, int commit, bool model_ok, const char* wrong_model, bool has_output) {
    if (c.candidates < 1 || c.candidates > UKFB_ASSOCIATE_MAX_CANDIDATES) return {UKFB_ERR_OUT_OF_RANGE, "candidates must be 1 ... 32"};
    if (!c.has_z || !c.has_Q) return {UKFB_ERR_INVALID_ARG, "z_dev and Q_dev must not be NULL"};
    if (!zero_or_one(c.q_is_uniform)) return {UKFB_ERR_INVALID_ARG, "q_is_uniform must be 0 or 1"};
    if (!zero_or_one(c.point_per_candidate)) return {UKFB_ERR_INVALID_ARG, "point_per_candidate must be 0 or 1"};
    if (c.point_per_candidate && !c.has_point)
        return {UKFB_ERR_INVALID_ARG, "point_per_candidate needs point_dev [candidates][capacity][3]"};
    if (!zero_or_one(commit)) return {UKFB_ERR_INVALID_ARG, "commit must be 0 or 1"};
    if (!model_ok) return {UKFB_ERR_WRONG_MODEL, wrong_model};
    return nothing_to_compute(commit, has_output);
}
template <class Out> bool meas_has_output(const Out* out) {   // ukfb_sensor_out, ukfb_sampled_out: the same six
    return out && (out->z_pred || out->S || out->innov || out->maha || out->loglik || out->status);
}
// the sensor-frame and the bearing update: one candidate, no point per candidate
inline SensorCall sensor_call(const ukfb_sensor_in* in) {
    return {/*candidates*/ 1, in->z_dev != nullptr, in->Q_dev != nullptr, in->q_is_uniform, /*point_per_candidate*/ 0, /*has_point*/ true};
}
inline Verdict check_sensor_args(int engine_model, bool per_filter_models, int model_uniform, const ukfb_sensor_in* in, int commit,
                                 const ukfb_sensor_out* out) {
    if (!in) return {UKFB_ERR_INVALID_ARG, "in must not be NULL"};
    return check_sensor_call(sensor_call(in), commit,
                             per_filter_models || sensor_model_ok(engine_model, model_uniform),
                             "sensor model id not valid for this engine (Pose: 0 ... 4, OrientationState: 5 ... 7)", meas_has_output(out));
}
struct SensorMap {
    int LS, ZS, FAC, RSP, TAB, WT, YM, MUF, PKF, INP, DUM, PF;
};
constexpr SensorMap sensor_map(int, int D) {
    RowSlice s;
    SensorMap m{};
    m.LS = ROW_LS;
    m.ZS = 4;   // row stride of the D x 3 matrices
    s.factor(D, m.FAC, m.RSP);
    m.TAB = s.table(D);   // the commit's; the half differences W and the solved cross-covariance Y (D * ZS each) alias it
    m.WT = m.TAB; m.YM = m.TAB + D * m.ZS;
    s.record(D, m.MUF, m.PKF);   // the state: mean, Sigma packed
    m.INP = s.take(32);          // z, Q, mount, point (SENSOR_INPUT_*), ten pads
    m.DUM = s.sink();
    m.PF = s.size();
    return m;
}
constexpr int sensor_filter_scalars(int S, int D) { return S > 16 ? -1 : sensor_map(S, D).PF; }
inline RowGeometry sensor_geometry(int S, int D, int64_t capacity, size_t compute_size) { return row_geometry(sensor_filter_scalars(S, D), capacity, compute_size); }

// ---- bearing measurements (ukfb_update_bearing_dev) -----------------------------------------------------------------------
// A direction on the sphere S^2 in the sensor frame, h = d / |d|: ids 0, 1 are the Pose engine's, 2 the OrientationState
// engine's (UKFB_BEARING_*).  The input record is the sensor-frame measurements' (SENSOR_INPUT_*): every model reads all of z
// and Q, qs and b; only POSE_POINT reads the lever arm r.
constexpr int BEARING_MODELS = 3;
constexpr bool bearing_model_ok(int engine_model, int64_t id) {
    return engine_model == UKFB_MODEL_POSE ? (id == UKFB_BEARING_POSE_POINT || id == UKFB_BEARING_POSE_NAV_DIRECTION)
                                           : id == UKFB_BEARING_ORIENT_NAV_DIRECTION;
}
constexpr bool bearing_reads_lever(int64_t id) { return id == UKFB_BEARING_POSE_POINT; }
constexpr bool bearing_input_used(int64_t id, int i) {
    return (id < 0 || id >= BEARING_MODELS || i < 0 || i >= SENSOR_INPUT_SCALARS) ? false
         : (i >= SENSOR_INPUT_MOUNT && i < SENSOR_INPUT_MOUNT + 3) ? bearing_reads_lever(id) : true;
}
// per_filter_models: the ids come from a device array (checked per filter by the kernel: an id the engine's model does not have
// marks the filter INACTIVE); otherwise the one id must be the engine model's
inline Verdict check_bearing_args(int engine_model, bool per_filter_models, int model_uniform, const ukfb_sensor_in* in, int commit,
                                  const ukfb_sensor_out* out) {
    if (!in) return {UKFB_ERR_INVALID_ARG, "in must not be NULL"};
    return check_sensor_call(sensor_call(in), commit,
                             per_filter_models || bearing_model_ok(engine_model, model_uniform),
                             "bearing model id not valid for this engine (Pose: 0, 1; OrientationState: 2)", meas_has_output(out));
}
// No map of its own: the slice is the sensor-frame kernel's (sensor_map).  The sphere side (the unit vectors, their logarithms,
// the 3 x 3 statistics) lives in registers.
constexpr int bearing_filter_scalars(int S, int D) { return sensor_filter_scalars(S, D); }
inline RowGeometry bearing_geometry(int S, int D, int64_t capacity, size_t compute_size) { return sensor_geometry(S, D, capacity, compute_size); }

// ---- sensor-frame association (ukfb_associate_sensor_dev) -----------------------------------------------------------------
// The sensor-frame models against K candidates per filter (ukf_associate.hpp): ids, inputs and the LDS map are the
// sensor-frame measurements'.  H hypotheses per filter: K when every candidate brings its own point, else one.
constexpr int ASSOCIATE_MAX_CANDIDATES = UKFB_ASSOCIATE_MAX_CANDIDATES;
constexpr int associate_hypotheses(int candidates, int point_per_candidate) { return point_per_candidate ? candidates : 1; }
// scalars of one output array of a call on `capacity` filters: z_pred / S hold H slots of 3 / 9 a filter, innov K slots of 3,
// maha / loglik K slots of 1 (what the host-array form allocates and copies)
constexpr int64_t associate_out_scalars(int slots, int64_t capacity, int per_filter) { return int64_t(slots) * capacity * per_filter; }
// (the clauses and their order: check_sensor_call)
inline Verdict check_associate_args(int engine_model, bool per_filter_models, int model_uniform, const ukfb_associate_in* in, int commit,
                                    const ukfb_associate_out* out) {
    if (!in) return {UKFB_ERR_INVALID_ARG, "in must not be NULL"};
    return check_sensor_call({in->candidates, in->z_dev != nullptr, in->Q_dev != nullptr, in->q_is_uniform, in->point_per_candidate, in->point_dev != nullptr},
                             commit, per_filter_models || sensor_model_ok(engine_model, model_uniform),
                             "sensor model id not valid for this engine (Pose: 0 ... 4, OrientationState: 5 ... 7)",
                             out && (out->z_pred || out->S || out->innov || out->maha || out->loglik || out->best || out->n_gated || out->status));
}

// ---- user-defined measurement models (ukfb_sigma_points_dev, ukfb_update_sampled_dev) --------------------------------------
// The caller evaluates h on the exported sigma points; the update is finished from the samples Z_i = h(X_i), m = 1 ...
// SAMPLED_MAX_M, one m for the call.
constexpr int SAMPLED_MAX_M = UKFB_SAMPLED_MAX_M;
// The record of one filter's inputs and of S as the kernel keeps them: z (SAMPLED_MAX_M), Q row-major m x m (up to
// SAMPLED_MAX_M^2), then S row-major with row stride SAMPLED_MAX_M, z-bar and nu (SAMPLED_MAX_M each; parked for the outputs)
constexpr int SAMPLED_INPUT_Z = 0, SAMPLED_INPUT_Q = SAMPLED_MAX_M, SAMPLED_INPUT_S = SAMPLED_INPUT_Q + SAMPLED_MAX_M * SAMPLED_MAX_M;
constexpr int SAMPLED_INPUT_ZBAR = SAMPLED_INPUT_S + SAMPLED_MAX_M * SAMPLED_MAX_M, SAMPLED_INPUT_NU = SAMPLED_INPUT_ZBAR + SAMPLED_MAX_M;
constexpr int SAMPLED_INPUT_SCALARS = SAMPLED_INPUT_NU + SAMPLED_MAX_M;
constexpr int SAMPLED_INPUT_REGION = (SAMPLED_INPUT_SCALARS + 15) / 16 * 16;
constexpr bool sampled_m_ok(int64_t m) { return m >= 1 && m <= SAMPLED_MAX_M; }
// scalars of one filter's sigma-point record ([2 D + 1][S]), of its tangent offsets ([2 D + 1][D]) and of its samples ([2 D + 1][m])
constexpr int64_t sampled_points(int D) { return 2 * int64_t(D) + 1; }
inline Verdict check_sigma_points_args(bool has_X, bool has_delta) {
    if (!has_X && !has_delta) return {UKFB_ERR_INVALID_ARG, "X_out_dev and delta_out_dev must not both be NULL"};
    return {};
}
inline Verdict check_sampled_args(const ukfb_sampled_in* in, int commit, const ukfb_sampled_out* out) {
    if (!in) return {UKFB_ERR_INVALID_ARG, "in must not be NULL"};
    if (!in->Z_dev || !in->z_dev || !in->Q_dev) return {UKFB_ERR_INVALID_ARG, "Z_dev, z_dev and Q_dev must not be NULL"};
    if (!zero_or_one(in->q_is_uniform)) return {UKFB_ERR_INVALID_ARG, "q_is_uniform must be 0 or 1"};
    if (!zero_or_one(commit)) return {UKFB_ERR_INVALID_ARG, "commit must be 0 or 1"};
    if (const Verdict v = nothing_to_compute(commit, meas_has_output(out)); v.rc != UKFB_OK) return v;
    if (!sampled_m_ok(in->m)) return {UKFB_ERR_OUT_OF_RANGE, "m must be 1 ... 6 (UKFB_SAMPLED_MAX_M)"};
    return {};
}
struct SampledMap {   // the update
    int LS, ZS, MM, FAC, RSP, TAB, WT, YM, ZST, MUF, PKF, INP, DUM, PF;
};
constexpr SampledMap sampled_map(int, int D) {
    RowSlice s;
    SampledMap m{};
    m.LS = ROW_LS;
    m.MM = SAMPLED_MAX_M;
    m.ZS = m.MM;   // row stride of the D x 6 matrices and of nothing else
    s.factor(D, m.FAC, m.RSP);
    m.TAB = s.table(D);   // the commit's; W, Y (D * ZS each) and the staged samples ((2 D + 1) * m, stride m) alias it
    m.WT = m.TAB; m.YM = m.TAB + D * m.ZS; m.ZST = m.TAB + 2 * D * m.ZS;
    s.record(D, m.MUF, m.PKF);              // the state: mean, Sigma packed
    m.INP = s.take(SAMPLED_INPUT_REGION);   // z, Q, S, z-bar, nu (SAMPLED_INPUT_*), pads
    m.DUM = s.sink();
    m.PF = s.size();
    return m;
}
struct SigmaPointsMap {   // the export
    int LS, FAC, RSP, MUF, PKF, DUM, PF;
};
constexpr SigmaPointsMap sigma_points_map(int, int D) {
    RowSlice s;
    SigmaPointsMap m{};
    m.LS = ROW_LS;
    s.factor(D, m.FAC, m.RSP);
    s.record(D, m.MUF, m.PKF);   // the state: mean, Sigma packed
    m.DUM = s.sink();
    m.PF = s.size();
    return m;
}
constexpr int sampled_filter_scalars(int S, int D) { return S > 16 ? -1 : sampled_map(S, D).PF; }
constexpr int sigma_points_filter_scalars(int S, int D) { return S > 16 ? -1 : sigma_points_map(S, D).PF; }
inline RowGeometry sampled_geometry(int S, int D, int64_t capacity, size_t compute_size) { return row_geometry(sampled_filter_scalars(S, D), capacity, compute_size); }
inline RowGeometry sigma_points_geometry(int S, int D, int64_t capacity, size_t compute_size) { return row_geometry(sigma_points_filter_scalars(S, D), capacity, compute_size); }

// ---- user-defined process models (ukfb_predict_sampled_dev) ----------------------------------------------------------------
// The caller evaluates f on the exported sigma points; the prediction is finished from the samples XX_i = f(X_i) and the caller's
// R.  The launch is the sampled update's: four filters per workgroup, one wavefront.
inline Verdict check_predict_sampled_args(const ukfb_predict_sampled_in* in, int commit, const ukfb_predict_sampled_out* out) {
    if (!in) return {UKFB_ERR_INVALID_ARG, "in must not be NULL"};
    if (!in->XX_dev || !in->R_dev) return {UKFB_ERR_INVALID_ARG, "XX_dev and R_dev must not be NULL"};
    if (!zero_or_one(in->r_is_uniform)) return {UKFB_ERR_INVALID_ARG, "r_is_uniform must be 0 or 1"};
    if (!zero_or_one(commit)) return {UKFB_ERR_INVALID_ARG, "commit must be 0 or 1"};
    return nothing_to_compute(commit, out && (out->mu || out->cov_packed || out->status));
}
struct PredictSampledMap {   // no factor, no reciprocal pivots, no rotation matrix: the kernel factorises nothing
    int LS, SMR, TAB, STG, CSM, CSP, DUM, PF;
};
constexpr PredictSampledMap predict_sampled_map(int, int D) {
    RowSlice s;
    PredictSampledMap m{};
    m.LS = ROW_LS;
    m.SMR = s.rows(D);    // the rows of Sigma^-, parked while R is added
    m.TAB = s.table(D);   // the staged samples ((2 D + 1) * S) alias it
    m.STG = m.TAB;
    s.record(D, m.CSM, m.CSP);   // the predicted record: mean (XX_0 until the mean is formed), Sigma^- packed
    m.DUM = s.sink();
    m.PF = s.size();
    return m;
}
constexpr int predict_sampled_filter_scalars(int S, int D) { return S > 16 ? -1 : predict_sampled_map(S, D).PF; }
inline RowGeometry predict_sampled_geometry(int S, int D, int64_t capacity, size_t compute_size) { return row_geometry(predict_sampled_filter_scalars(S, D), capacity, compute_size); }

// ---- covariance conditioning (ukfb_condition_dev) ----------------------------------------------------------------------------
// Eigenvalue repair of the covariance in its correlation scaling by cyclic Jacobi, round-robin ordering.  The launch is the
// sampled update's: four filters per workgroup, one wavefront.
constexpr int CONDITION_MAX_SWEEPS = 12, CONDITION_SLICE_PAD = 4;
// players of the round-robin schedule (D rounded up to even; the odd D is padded with a decoupled unit row), pairs per step and
// steps per sweep; the first pair of a step is the one that holds the last player: where that player is the padding, the pair is
// the identity and is dropped
constexpr int condition_players(int D) { return (D + 1) / 2 * 2; }
constexpr int condition_first_pair(int D) { return condition_players(D) != D ? 1 : 0; }
constexpr int condition_pairs_per_step(int D) { return condition_players(D) / 2; }
constexpr int condition_steps(int D) { return condition_players(D) - 1; }
inline Verdict check_condition_args(const ukfb_condition_in* in, int commit, const ukfb_condition_out* out) {
    if (!in) return {UKFB_ERR_INVALID_ARG, "in must not be NULL"};
    if (!in->var_floor_dev) return {UKFB_ERR_INVALID_ARG, "var_floor_dev must not be NULL"};
    if (!(in->eig_floor > 0.0 && in->eig_floor < 1.0)) return {UKFB_ERR_INVALID_ARG, "eig_floor must lie in (0, 1)"};   // (NaN fails both)
    if (!zero_or_one(in->renormalize_quaternion))
        return {UKFB_ERR_INVALID_ARG, "renormalize_quaternion must be 0 or 1"};
    if (!zero_or_one(commit)) return {UKFB_ERR_INVALID_ARG, "commit must be 0 or 1"};
    return nothing_to_compute(commit, out && (out->eig_min || out->eig_max || out->mu || out->cov_packed || out->status));
}
// the host form's floor: every entry finite and > 0
inline Verdict check_condition_floor(const double* var_floor, int D) {
    if (!var_floor) return {UKFB_ERR_INVALID_ARG, "var_floor must not be NULL"};
    for (int t = 0; t < D; ++t)
        if (!(var_floor[t] > 0.0 && var_floor[t] <= 1.7976931348623157e308))
            return {UKFB_ERR_INVALID_ARG, "every entry of var_floor must be finite and > 0"};
    return {};
}
struct ConditionMap {
    int LS, ROW, VPB, LAM, SDV, MUF, PKF, DUM, PF;
};
constexpr ConditionMap condition_map(int, int D) {
    RowSlice s;
    ConditionMap m{};
    m.LS = ROW_LS;
    m.ROW = s.rows(D);    // the rows of M J of a step (the row phase's exchange)
    m.VPB = s.rows(D);    // V as every row published it
    m.LAM = s.take(16);   // the eigenvalues
    m.SDV = s.take(16);   // s_t = sqrt(d_t)
    s.record(D, m.MUF, m.PKF);   // the state: mean, Sigma packed
    m.DUM = s.sink();
    s.take(CONDITION_SLICE_PAD);   // keeps the four slices of a workgroup off each other's banks in either precision
    m.PF = s.size();
    return m;
}
constexpr int condition_filter_scalars(int S, int D) { return S > 16 ? -1 : condition_map(S, D).PF; }
inline RowGeometry condition_geometry(int S, int D, int64_t capacity, size_t compute_size) { return row_geometry(condition_filter_scalars(S, D), capacity, compute_size); }

// ---- late samples (ukfb_update_delayed_dev, ukfb_delayed_lag_dev) -----------------------------------------------------------
// The smoother's window with the engine's own state as its last step: the chain runs at most steps - 1 <= SMOOTH_MAX_BACK
// backward steps, all in one launch (their dt travel in the kernel arguments), so steps <= DELAYED_MAX_STEPS.
constexpr int DELAYED_MAX_STEPS = UKFB_DELAYED_MAX_STEPS;
static_assert(DELAYED_MAX_STEPS == SMOOTH_MAX_BACK + 1, "one launch covers the longest window");
inline Verdict check_delayed_args(const ukfb_delayed_in* in, int commit, const ukfb_delayed_out* out) {
    if (!in) return {UKFB_ERR_INVALID_ARG, "in must not be NULL"};
    if (in->slots < 1 || in->steps < 1) return {UKFB_ERR_INVALID_ARG, "steps >= 1, slots >= 1"};
    if (in->first_slot < 0 || in->first_slot >= in->slots) return {UKFB_ERR_INVALID_ARG, "0 <= first_slot < slots"};
    if (in->steps > 1 && !in->dt) return {UKFB_ERR_INVALID_ARG, "dt must not be NULL for a window of more than one step"};
    if (!in->mu_hist_dev || !in->cov_hist_dev) return {UKFB_ERR_INVALID_ARG, "mu_hist_dev and cov_hist_dev must not be NULL"};
    if (!in->z_dev || !in->Q_dev) return {UKFB_ERR_INVALID_ARG, "z_dev and Q_dev must not be NULL"};
    if (!zero_or_one(in->q_is_uniform)) return {UKFB_ERR_INVALID_ARG, "q_is_uniform must be 0 or 1"};
    if (!zero_or_one(commit)) return {UKFB_ERR_INVALID_ARG, "commit must be 0 or 1"};
    if (const Verdict v = nothing_to_compute(commit, out && (out->z_pred || out->S || out->innov || out->maha || out->loglik || out->status ||
                                                             out->mu_out || out->cov_out));
        v.rc != UKFB_OK)
        return v;
    if (in->steps > std::min(in->slots, DELAYED_MAX_STEPS))
        return {UKFB_ERR_OUT_OF_RANGE, "steps <= min(slots, 33): a sample older than that is out of the window"};
    return {};
}
inline Verdict check_delayed_lag_args(int steps, const int64_t* step_ts_us, bool has_samples, bool has_out) {
    if (steps < 1 || !step_ts_us) return {UKFB_ERR_INVALID_ARG, "steps >= 1 and step_ts_us must not be NULL"};
    if (!has_samples || !has_out) return {UKFB_ERR_INVALID_ARG, "sample_ts_us_dev and lag_out_dev must not be NULL"};
    if (steps > DELAYED_MAX_STEPS) return {UKFB_ERR_OUT_OF_RANGE, "steps <= 33"};
    for (int c = 1; c < steps; ++c)
        if (step_ts_us[c] <= step_ts_us[c - 1]) return {UKFB_ERR_INVALID_ARG, "step_ts_us must be strictly increasing"};
    return {};
}
// The lag rule (host and device): l = n - c*, c* the step nearest the sample, ties to the older step; newer than step n: 0;
// older than step 0 by more than half of the first interval: steps (out of the window).  Differences of stamps that are 2^62
// apart would overflow: stamps are microseconds since an epoch, as everywhere in the engine.
UKFB_HD int32_t delayed_lag_of(int steps, const int64_t* step_ts_us, int64_t t) {
    const int n = steps - 1;
    if (t >= step_ts_us[n]) return 0;
    const int64_t first = steps > 1 ? step_ts_us[1] - step_ts_us[0] : 0;
    if (t < step_ts_us[0] && 2 * (step_ts_us[0] - t) > first) return int32_t(steps);
    int best = 0;
    int64_t bd = t > step_ts_us[0] ? t - step_ts_us[0] : step_ts_us[0] - t;
    for (int c = 1; c < steps; ++c) {
        const int64_t d = t > step_ts_us[c] ? t - step_ts_us[c] : step_ts_us[c] - t;
        if (d < bd) {   // strictly nearer: a tie stays with the older step
            bd = d;
            best = c;
        }
    }
    return int32_t(n - best);
}
struct DelayedMap : SmoothMap {   // the smoother's slice, widened
    int ZS, WT, YM, YN, MOP;
};
constexpr DelayedMap delayed_map(int S, int D) {
    DelayedMap m{smooth_map(S, D), 0, 0, 0, 0, 0};
    RowSlice s{m.PF};
    m.ZS = 4;   // row stride of the D x 3 matrices W, Y_s and Y_n in the dead delta table
    m.WT = m.TAB; m.YM = m.TAB + D * m.ZS; m.YN = m.TAB + 2 * D * m.ZS;
    m.MOP = s.rows(D);   // the operator M, row l at MOP + l * LS
    m.PF = s.size();
    return m;
}
constexpr int delayed_filter_scalars(int S, int D) { return S > 16 ? -1 : delayed_map(S, D).PF; }
inline RowGeometry delayed_geometry(int S, int D, int64_t capacity, size_t compute_size) { return row_geometry(delayed_filter_scalars(S, D), capacity, compute_size); }

// ---- relative measurements (ukfb_update_relative_dev) -------------------------------------------------------------------------
// An increment between step n - lag of the delayed update's window and the present, Pose engines only (UKFB_RELATIVE_*).  The
// record of one filter's sample: z = dp (3) then dq (4), Q 6 x 6 row-major in the tangent order (dp, dtheta).
constexpr int RELATIVE_MODELS = 3, RELATIVE_Z = 7, RELATIVE_M = 6;
UKFB_HD bool relative_model_ok(int64_t id) { return id >= UKFB_RELATIVE_POSE && id <= UKFB_RELATIVE_ROTATION; }
constexpr int relative_meas_dim(int64_t id) { return (id < 0 || id >= RELATIVE_MODELS) ? 0 : (id == UKFB_RELATIVE_POSE ? 6 : 3); }
// tangent row / column t of the sample (0 ... 5) is read by model id
constexpr bool relative_reads(int64_t id, int t) {
    return t >= 0 && t < RELATIVE_M && (id == UKFB_RELATIVE_POSE || (id == UKFB_RELATIVE_POSITION && t < 3) || (id == UKFB_RELATIVE_ROTATION && t >= 3));
}
// the clauses of check_delayed_args in their order, with the engine's model judged first: the feature has no kernel for
// OrientationState engines (include/ukf_batch.h says why)
inline Verdict check_relative_args(int engine_model, const ukfb_relative_in* in, int commit, const ukfb_relative_out* out) {
    if (engine_model != UKFB_MODEL_POSE) return {UKFB_ERR_WRONG_MODEL, "relative measurements serve Pose engines only"};
    if (!in) return {UKFB_ERR_INVALID_ARG, "in must not be NULL"};
    if (in->slots < 1 || in->steps < 1) return {UKFB_ERR_INVALID_ARG, "steps >= 1, slots >= 1"};
    if (in->first_slot < 0 || in->first_slot >= in->slots) return {UKFB_ERR_INVALID_ARG, "0 <= first_slot < slots"};
    if (in->steps > 1 && !in->dt) return {UKFB_ERR_INVALID_ARG, "dt must not be NULL for a window of more than one step"};
    if (!in->mu_hist_dev || !in->cov_hist_dev) return {UKFB_ERR_INVALID_ARG, "mu_hist_dev and cov_hist_dev must not be NULL"};
    if (!in->z_dev || !in->Q_dev) return {UKFB_ERR_INVALID_ARG, "z_dev and Q_dev must not be NULL"};
    if (!zero_or_one(in->q_is_uniform)) return {UKFB_ERR_INVALID_ARG, "q_is_uniform must be 0 or 1"};
    if (!zero_or_one(commit)) return {UKFB_ERR_INVALID_ARG, "commit must be 0 or 1"};
    if (const Verdict v = nothing_to_compute(commit, out && (out->z_pred || out->S || out->innov || out->maha || out->loglik || out->status ||
                                                             out->mu_out || out->cov_out));
        v.rc != UKFB_OK)
        return v;
    if (in->steps > std::min(in->slots, DELAYED_MAX_STEPS))
        return {UKFB_ERR_OUT_OF_RANGE, "steps <= min(slots, 33): an increment that starts before that is out of the window"};
    return {};
}
// The delayed update's slice, not one scalar wider: what the update on the pair adds lives in regions the chain leaves dead.
struct RelativeMap : DelayedMap {
    int NR, LE, PRK;   // (ZS, WT, YN: the delayed map's names, with six columns here; YM is not used)
};
// the scores parked across the commit, every filter's own: S packed (21), nu (6), z-bar (7), d^2, ln det S
constexpr int RELATIVE_PARK_S = 0, RELATIVE_PARK_NU = 21, RELATIVE_PARK_ZBAR = 27, RELATIVE_PARK_D2 = 34, RELATIVE_PARK_LNDET = 35;
constexpr int RELATIVE_PARK_SCALARS = 36;
constexpr RelativeMap relative_map(int S, int D) {
    RelativeMap m{delayed_map(S, D), 0, 0, 0};
    m.ZS = RELATIVE_M;   // row stride of the D x 6 matrices W and Y_n in the dead delta table
    m.NR = m.TAB;        // the rows of N = Sigma_n M^T (D * LS), dead before W is written
    m.WT = m.TAB; m.YM = m.TAB; m.YN = m.TAB + D * m.ZS;
    m.LE = m.SMR;        // the columns of L_e (D * LS) in the parked rows of Sigma^-
    m.PRK = m.SMR;       // ... and, once L_e is dead, the scores (RELATIVE_PARK_SCALARS <= D * LS)
    return m;
}
constexpr int relative_filter_scalars(int S, int D) { return S > 16 ? -1 : relative_map(S, D).PF; }
inline RowGeometry relative_geometry(int S, int D, int64_t capacity, size_t compute_size) { return row_geometry(relative_filter_scalars(S, D), capacity, compute_size); }

// ---- late sensor-frame samples (ukfb_update_delayed_sensor_dev) -----------------------------------------------------------------
// The delayed update's window and lag with the sensor-frame measurements' models and inputs (include/ukf_batch_delayed_sensor.h).
// The record of one filter's inputs as the kernel stages it: the sensor-frame record (SENSOR_INPUT_*), then the rotation rate at
// the time of the sample (3), which ORIENT_VELOCITY alone reads; its neutral value is 0.
constexpr int DELAYED_SENSOR_INPUT_RATE = SENSOR_INPUT_SCALARS, DELAYED_SENSOR_INPUT_SCALARS = DELAYED_SENSOR_INPUT_RATE + 3;
constexpr int DELAYED_SENSOR_INPUT_REGION = 32;   // what the staging writes: lane l takes entries l and l + 16
constexpr bool delayed_sensor_input_used(int64_t id, int i) {
    return i < DELAYED_SENSOR_INPUT_RATE ? sensor_input_used(id, i) : (i < DELAYED_SENSOR_INPUT_SCALARS && id == UKFB_SENSOR_ORIENT_VELOCITY);
}
// the window and lag fields of a late sensor-frame sample as the delayed update's own structure (the model fields stay unset)
inline ukfb_delayed_in delayed_window_of(const ukfb_delayed_sensor_in* in) {
    ukfb_delayed_in d{};
    d.steps = in->steps; d.dt = in->dt; d.slots = in->slots; d.first_slot = in->first_slot;
    d.mu_hist_dev = in->mu_hist_dev; d.cov_hist_dev = in->cov_hist_dev; d.in_a_dev = in->in_a_dev; d.in_b_dev = in->in_b_dev;
    d.lag_uniform = in->lag_uniform; d.lag_dev = in->lag_dev;
    d.z_dev = in->z_dev; d.Q_dev = in->Q_dev; d.q_is_uniform = in->q_is_uniform;
    return d;
}
// the clauses of check_delayed_args, then the clauses of check_sensor_call, in that order (a per-filter id is the kernel's to
// judge: INACTIVE)
inline Verdict check_delayed_sensor_args(int engine_model, const ukfb_delayed_sensor_in* in, int commit, const ukfb_delayed_out* out) {
    if (!in) return {UKFB_ERR_INVALID_ARG, "in must not be NULL"};
    const ukfb_delayed_in win = delayed_window_of(in);
    if (const Verdict v = check_delayed_args(&win, commit, out); v.rc != UKFB_OK) return v;
    return check_sensor_call({/*candidates*/ 1, in->z_dev != nullptr, in->Q_dev != nullptr, in->q_is_uniform, /*point_per_candidate*/ 0, /*has_point*/ true},
                             commit, in->model_dev != nullptr || sensor_model_ok(engine_model, in->model_uniform),
                             "sensor model id not valid for this engine (Pose: 0 ... 4, OrientationState: 5 ... 7)",
                             out && (out->z_pred || out->S || out->innov || out->maha || out->loglik || out->status || out->mu_out || out->cov_out));
}
// The delayed update's slice, not one scalar wider: the staged input record lives in the parked rows of Sigma^-, which are dead
// once the chain has ended (the record is written after the loop and read until the statistics are formed).
struct DelayedSensorMap : DelayedMap {
    int INP;
};
constexpr DelayedSensorMap delayed_sensor_map(int S, int D) {
    DelayedSensorMap m{delayed_map(S, D), 0};
    m.INP = m.SMR;   // DELAYED_SENSOR_INPUT_REGION <= D * LS
    return m;
}
constexpr int delayed_sensor_filter_scalars(int S, int D) { return S > 16 ? -1 : delayed_sensor_map(S, D).PF; }
inline RowGeometry delayed_sensor_geometry(int S, int D, int64_t capacity, size_t compute_size) { return row_geometry(delayed_sensor_filter_scalars(S, D), capacity, compute_size); }

// ---- the robust sensor-frame update (ukfb_update_robust_dev) ----------------------------------------------------------------
// The sensor-frame update's arguments and the rule (include/ukf_batch_robust.h).  The rule is judged first: it is the part of
// the call that no other entry point checks.  Models, inputs, LDS map and geometry are the sensor-frame measurements'.
constexpr int ROBUST_MAX_ITER = 64;
inline Verdict check_robust_rule(const ukfb_robust_rule* rule) {
    if (!rule) return {UKFB_ERR_INVALID_ARG, "rule must not be NULL"};
    if (rule->mode != UKFB_ROBUST_MATCH && rule->mode != UKFB_ROBUST_HUBER)
        return {UKFB_ERR_INVALID_ARG, "rule.mode must be UKFB_ROBUST_MATCH or UKFB_ROBUST_HUBER"};
    if (!std::isfinite(rule->chi2_m1) || !(rule->chi2_m1 > 0.0) || !std::isfinite(rule->chi2_m3) || !(rule->chi2_m3 > 0.0))
        return {UKFB_ERR_INVALID_ARG, "rule.chi2_m1 and rule.chi2_m3 must be finite and > 0"};
    if (!std::isfinite(rule->scale_max) || !(rule->scale_max >= 1.0)) return {UKFB_ERR_INVALID_ARG, "rule.scale_max must be finite and >= 1"};
    if (!std::isfinite(rule->tol) || !(rule->tol >= 0.0)) return {UKFB_ERR_INVALID_ARG, "rule.tol must be finite and >= 0"};
    if (rule->max_iter < 1 || rule->max_iter > ROBUST_MAX_ITER) return {UKFB_ERR_INVALID_ARG, "rule.max_iter must be 1 ... 64"};
    return {};
}
inline bool robust_has_output(const ukfb_robust_out* out) {
    return out && (out->z_pred || out->S || out->innov || out->maha0 || out->maha || out->loglik || out->scale || out->iterations || out->status);
}
inline Verdict check_robust_args(int engine_model, bool per_filter_models, int model_uniform, const ukfb_sensor_in* in,
                                 const ukfb_robust_rule* rule, int commit, const ukfb_robust_out* out) {
    if (const Verdict v = check_robust_rule(rule); v.rc != UKFB_OK) return v;
    if (!in) return {UKFB_ERR_INVALID_ARG, "in must not be NULL"};
    return check_sensor_call(sensor_call(in), commit, per_filter_models || sensor_model_ok(engine_model, model_uniform),
                             "sensor model id not valid for this engine (Pose: 0 ... 4, OrientationState: 5 ... 7)", robust_has_output(out));
}

// ---- probabilistic data association (ukfb_update_pda_dev) -------------------------------------------------------------------
// The shared-h association's arguments and the rule (include/ukf_batch_pda.h).  The rule is judged first, as the robust
// update's is; then the candidate range (it alone decides UKFB_ERR_OUT_OF_RANGE), then the mode, then the association's clauses.
// Models, inputs, LDS map and geometry are the sensor-frame measurements'.
inline Verdict check_pda_rule(const ukfb_pda_rule* rule) {
    if (!rule) return {UKFB_ERR_INVALID_ARG, "rule must not be NULL"};
    const auto prob = [](double p) { return std::isfinite(p) && p > 0.0 && p <= 1.0; };
    if (!prob(rule->p_detect)) return {UKFB_ERR_INVALID_ARG, "rule.p_detect must be in (0, 1]"};
    if (!prob(rule->p_gate_m1) || !prob(rule->p_gate_m3)) return {UKFB_ERR_INVALID_ARG, "rule.p_gate_m1 and rule.p_gate_m3 must be in (0, 1]"};
    if (!(rule->p_detect * rule->p_gate_m1 < 1.0) || !(rule->p_detect * rule->p_gate_m3 < 1.0))
        return {UKFB_ERR_INVALID_ARG, "rule.p_detect * rule.p_gate must be < 1 for m = 1 and m = 3"};
    if (!std::isfinite(rule->clutter_m1) || !(rule->clutter_m1 > 0.0) || !std::isfinite(rule->clutter_m3) || !(rule->clutter_m3 > 0.0))
        return {UKFB_ERR_INVALID_ARG, "rule.clutter_m1 and rule.clutter_m3 must be finite and > 0"};
    return {};
}
// what the kernel gets of a checked rule, formed in double: a_0 = ln lambda_m + ln(1 - P_D P_G,m) for m = 1 / m = 3, and ln P_D
struct PdaLogs {
    double a0_m1, a0_m3, ln_pd;
};
inline PdaLogs pda_logs(const ukfb_pda_rule& r) {
    return {std::log(r.clutter_m1) + std::log1p(-r.p_detect * r.p_gate_m1), std::log(r.clutter_m3) + std::log1p(-r.p_detect * r.p_gate_m3),
            std::log(r.p_detect)};
}
inline bool pda_has_output(const ukfb_pda_out* out) {
    return out && (out->z_pred || out->S || out->innov || out->maha || out->loglik || out->beta || out->beta0 || out->innov_comb || out->best ||
                   out->n_gated || out->status);
}
inline Verdict check_pda_args(int engine_model, bool per_filter_models, int model_uniform, const ukfb_associate_in* in, const ukfb_pda_rule* rule,
                              int commit, const ukfb_pda_out* out) {
    if (const Verdict v = check_pda_rule(rule); v.rc != UKFB_OK) return v;
    if (!in) return {UKFB_ERR_INVALID_ARG, "in must not be NULL"};
    if (in->candidates < 1 || in->candidates > UKFB_ASSOCIATE_MAX_CANDIDATES) return {UKFB_ERR_OUT_OF_RANGE, "candidates must be 1 ... 32"};
    if (in->point_per_candidate != 0)
        return {UKFB_ERR_INVALID_ARG, "point_per_candidate must be 0: per-hypothesis candidates combine into a mixture, not PDA"};
    return check_sensor_call({in->candidates, in->z_dev != nullptr, in->Q_dev != nullptr, in->q_is_uniform, 0, in->point_dev != nullptr}, commit,
                             per_filter_models || sensor_model_ok(engine_model, model_uniform),
                             "sensor model id not valid for this engine (Pose: 0 ... 4, OrientationState: 5 ... 7)", pda_has_output(out));
}

// ---- global nearest-neighbour assignment (ukfb_assign_scenes_dev) -------------------------------------------------------------
// One wavefront per scene, ASSIGN_SCENES_PER_GROUP scenes per workgroup, one lane per column of the T x (K + T) problem.  The
// LDS map, stated once for host and device: every scene of a workgroup owns one block of doubles, the staged cost
// cost[i][k] at i * ASSIGN_ROW_STRIDE + k (the odd stride keeps the staging writes, which run along i, off one bank).
constexpr int ASSIGN_SCENES_PER_GROUP = 4, ASSIGN_THREADS = 64 * ASSIGN_SCENES_PER_GROUP;
constexpr int ASSIGN_ROW_STRIDE = UKFB_ASSOCIATE_MAX_CANDIDATES + 1;
struct AssignMap {
    int scene_scalars = UKFB_ASSIGN_MAX_TRACKS * ASSIGN_ROW_STRIDE;   // doubles of one scene's block
    constexpr int cost(int scene_in_group, int track, int k) const { return scene_in_group * scene_scalars + track * ASSIGN_ROW_STRIDE + k; }
    constexpr int scalars() const { return ASSIGN_SCENES_PER_GROUP * scene_scalars; }
    constexpr int bytes() const { return scalars() * int(sizeof(double)); }
};
constexpr AssignMap assign_map() { return {}; }
static_assert(UKFB_ASSIGN_MAX_TRACKS + UKFB_ASSOCIATE_MAX_CANDIDATES <= 64, "one lane per column");
static_assert(assign_map().bytes() <= 65536, "a workgroup's cost blocks fit the LDS a workgroup may have");
// the loops of the solver, bounded by constants: tracks, Dijkstra steps of one sweep (one column is scanned per step), walk back
constexpr int ASSIGN_MAX_STEPS = UKFB_ASSIGN_MAX_TRACKS + UKFB_ASSOCIATE_MAX_CANDIDATES, ASSIGN_MAX_WALK = UKFB_ASSIGN_MAX_TRACKS;
struct AssignGeometry {
    int64_t grid;    // workgroups of ASSIGN_SCENES_PER_GROUP scenes
    int lds_bytes;   // static LDS of a workgroup
};
inline AssignGeometry assign_geometry(int scenes) {
    return {(int64_t(scenes) + ASSIGN_SCENES_PER_GROUP - 1) / ASSIGN_SCENES_PER_GROUP, assign_map().bytes()};
}
// the segment rule: what the kernel asks of offsets it cannot trust, and the host-array form of offsets it can see
UKFB_HD bool assign_segment_ok(int64_t a, int64_t b, int64_t capacity) {
    return a >= 0 && b <= capacity && b >= a && b - a <= UKFB_ASSIGN_MAX_TRACKS;
}
// scene s of uniform mode
UKFB_HD void assign_uniform_segment(int64_t s, int tracks_per_scene, int64_t capacity, int64_t* a, int64_t* b) {
    *a = s * tracks_per_scene;
    *b = *a + tracks_per_scene < capacity ? *a + tracks_per_scene : capacity;
}
// the rules of a pair and of a track
UKFB_HD bool assign_value_ok(double v) { return v >= -UKFB_ASSIGN_COST_MAX && v <= UKFB_ASSIGN_COST_MAX; }   // (false for NaN and +-Inf)
UKFB_HD bool assign_pair_allowed(double cost, double gate) { return assign_value_ok(cost) && !(gate >= 0.0 && cost > gate); }
inline int64_t assign_max_scenes(const ukfb_assign_in* in, int64_t capacity) {
    if (in->scene_start_dev) return capacity + 1;
    return (capacity + in->tracks_per_scene - 1) / in->tracks_per_scene;
}
inline Verdict check_assign_args(int64_t capacity, const ukfb_assign_in* in, const ukfb_assign_out* out) {
    if (!in) return {UKFB_ERR_INVALID_ARG, "in must not be NULL"};
    if (!in->cost_dev) return {UKFB_ERR_INVALID_ARG, "cost must not be NULL"};
    if (!out || (!out->assign && !out->owner && !out->objective && !out->scene_status))
        return {UKFB_ERR_INVALID_ARG, "every output of ukfb_assign_out is NULL: nothing to compute"};
    if (!in->miss_dev && !std::isfinite(in->miss_uniform)) return {UKFB_ERR_INVALID_ARG, "miss_uniform must be finite when miss is NULL"};
    if (in->candidates < 1 || in->candidates > UKFB_ASSOCIATE_MAX_CANDIDATES) return {UKFB_ERR_OUT_OF_RANGE, "candidates must be 1 ... 32"};
    if (!in->scene_start_dev && (in->tracks_per_scene < 1 || in->tracks_per_scene > UKFB_ASSIGN_MAX_TRACKS))
        return {UKFB_ERR_OUT_OF_RANGE, "tracks_per_scene must be 1 ... 32 in uniform mode"};
    if (in->scenes < 0) return {UKFB_ERR_OUT_OF_RANGE, "scenes must be >= 0"};
    if (int64_t(in->scenes) > assign_max_scenes(in, capacity))
        return {UKFB_ERR_OUT_OF_RANGE, "more scenes than the engine has room for (uniform: ceil(capacity / tracks_per_scene); ragged: capacity + 1)"};
    return {};
}
// the host-array form sees the offsets: every segment must pass the kernel's rule, and the offsets ascend
inline Verdict check_assign_offsets(int64_t capacity, int scenes, const int32_t* scene_start) {
    for (int s = 0; s < scenes; ++s)
        if (!assign_segment_ok(scene_start[s], scene_start[s + 1], capacity))
            return {UKFB_ERR_OUT_OF_RANGE, "scene_start: a scene must lie inside [0, capacity), end at or after its start and hold at most 32 tracks"};
    return {};
}

// ---- joint probabilistic data association (ukfb_jpda_scenes_dev, ukfb_update_weighted_dev) --------------------------------------
// One wavefront per scene, JPDA_SCENES_PER_GROUP scenes per workgroup, one lane per SUBSET of the scene's tracks (the lane
// index is the subset's bitmask, 2^6 = 64).  No LDS: psi is staged in registers (lane k holds psi_ik of every track i) and read
// with constant lane indices; the table of the backward recurrence lives in 32 fp64 registers.
constexpr int JPDA_SCENES_PER_GROUP = 4, JPDA_THREADS = 64 * JPDA_SCENES_PER_GROUP;
static_assert((1 << UKFB_JPDA_MAX_TRACKS) == 64, "one lane per subset of the tracks");
static_assert(UKFB_JPDA_MAX_TRACKS <= UKFB_ASSIGN_MAX_TRACKS, "a too-large scene is still a well-formed segment");
struct JpdaGeometry {
    int64_t grid;    // workgroups of JPDA_SCENES_PER_GROUP scenes
    int lds_bytes;   // none
};
inline JpdaGeometry jpda_geometry(int scenes) { return {(int64_t(scenes) + JPDA_SCENES_PER_GROUP - 1) / JPDA_SCENES_PER_GROUP, 0}; }
// the segment rule: assign_segment_ok decides BAD_SCENE (offsets the kernel cannot trust), then the limit of six tracks
UKFB_HD uint32_t jpda_segment_status(int64_t a, int64_t b, int64_t capacity) {
    return !assign_segment_ok(a, b, capacity) ? uint32_t(UKFB_JPDA_BAD_SCENE)
                                              : (b - a > UKFB_JPDA_MAX_TRACKS ? uint32_t(UKFB_JPDA_TOO_LARGE) : uint32_t(UKFB_JPDA_OK));
}
// the rules of a pair: finite (x - x == 0 is false for NaN and +-Inf, on host and device alike)
UKFB_HD bool jpda_finite(double v) { return v - v == 0.0; }
UKFB_HD bool jpda_gate_on(double gate) { return gate >= 0.0; }   // (false for NaN)
UKFB_HD bool jpda_pair_allowed(double loglik, double maha, double gate) {
    return jpda_finite(loglik) && (!jpda_gate_on(gate) || (jpda_finite(maha) && maha <= gate));
}
// m as the PDA kernel takes it: the model's, 3 for an id this engine does not have
UKFB_HD int jpda_kernel_dim(int engine_model, int64_t id) { return sensor_model_ok(engine_model, id) ? sensor_meas_dim(id) : 3; }
inline bool jpda_has_output(const ukfb_jpda_out* out) { return out && (out->beta || out->beta0 || out->free || out->log_z || out->scene_status); }
inline int64_t jpda_max_scenes(const ukfb_jpda_in* in, int64_t capacity) {
    if (in->scene_start_dev) return capacity + 1;
    return (capacity + in->tracks_per_scene - 1) / in->tracks_per_scene;
}
// The rule is judged first, as the PDA update's is; then the INVALID_ARG clauses, then the ranges.
inline Verdict check_jpda_args(int64_t capacity, const ukfb_jpda_in* in, const ukfb_pda_rule* rule, const ukfb_jpda_out* out) {
    if (const Verdict v = check_pda_rule(rule); v.rc != UKFB_OK) return v;
    if (!in) return {UKFB_ERR_INVALID_ARG, "in must not be NULL"};
    if (!in->loglik_dev) return {UKFB_ERR_INVALID_ARG, "loglik must not be NULL"};
    if (!jpda_has_output(out)) return {UKFB_ERR_INVALID_ARG, "every output of ukfb_jpda_out is NULL: nothing to compute"};
    if (!in->maha_dev && jpda_gate_on(in->gate)) return {UKFB_ERR_INVALID_ARG, "a gate >= 0 needs maha"};
    if (in->candidates < 1 || in->candidates > UKFB_ASSOCIATE_MAX_CANDIDATES) return {UKFB_ERR_OUT_OF_RANGE, "candidates must be 1 ... 32"};
    if (!in->scene_start_dev && (in->tracks_per_scene < 1 || in->tracks_per_scene > UKFB_JPDA_MAX_TRACKS))
        return {UKFB_ERR_OUT_OF_RANGE, "tracks_per_scene must be 1 ... 6 in uniform mode"};
    if (in->scenes < 0) return {UKFB_ERR_OUT_OF_RANGE, "scenes must be >= 0"};
    if (int64_t(in->scenes) > jpda_max_scenes(in, capacity))
        return {UKFB_ERR_OUT_OF_RANGE, "more scenes than the engine has room for (uniform: ceil(capacity / tracks_per_scene); ragged: capacity + 1)"};
    return {};
}
// the update with given weights: the shared-h association's arguments and the weights; cfg.gate_chi2 plays no part
inline bool weighted_has_output(const ukfb_weighted_out* out) {
    return out && (out->z_pred || out->S || out->innov || out->maha || out->loglik || out->weight_used || out->beta0 || out->innov_comb ||
                   out->n_used || out->status);
}
inline Verdict check_weighted_args(int engine_model, bool per_filter_models, int model_uniform, const ukfb_associate_in* in, const void* weight,
                                   int commit, const ukfb_weighted_out* out) {
    if (!in) return {UKFB_ERR_INVALID_ARG, "in must not be NULL"};
    if (!weight) return {UKFB_ERR_INVALID_ARG, "weight must not be NULL"};
    if (in->candidates < 1 || in->candidates > UKFB_ASSOCIATE_MAX_CANDIDATES) return {UKFB_ERR_OUT_OF_RANGE, "candidates must be 1 ... 32"};
    if (in->point_per_candidate != 0)
        return {UKFB_ERR_INVALID_ARG, "point_per_candidate must be 0: per-hypothesis candidates combine into a mixture, not PDA"};
    return check_sensor_call({in->candidates, in->z_dev != nullptr, in->Q_dev != nullptr, in->q_is_uniform, 0, in->point_dev != nullptr}, commit,
                             per_filter_models || sensor_model_ok(engine_model, model_uniform),
                             "sensor model id not valid for this engine (Pose: 0 ... 4, OrientationState: 5 ... 7)", weighted_has_output(out));
}

// ---- bounded waits ----------------------------------------------------------------------------------------------------------
// Waiting by polling: hipEventSynchronize / hipStreamSynchronize sleep on an interrupt and were measured to
// wake up to ~55 ms late on a loaded host (1 run in 5), which is longer than the work being waited for.
// The wait is bounded: after a short spin the poll backs off to 50 us sleeps, and gives up
// after UKFB_WAIT_TIMEOUT_S seconds (default 120) so that a kernel that never finishes cannot pin a host core
// forever; the caller reports UKFB_ERR_HIP with "timed out".
constexpr int WAIT_SPINS = 20000;
constexpr double WAIT_TIMEOUT_DEFAULT_S = 120.0;
// the value of UKFB_WAIT_TIMEOUT_S (NULL: unset); anything that is not a positive number is the default
inline double wait_timeout_seconds(const char* s) {
    const double v = s ? std::atof(s) : 0.0;
    return v > 0.0 ? v : WAIT_TIMEOUT_DEFAULT_S;
}
template <class R> struct Waited {
    R result;       // the query's last answer: its ready value, or an error (returned at once)
    bool gave_up;   // still `not_ready` when the timeout ran out
};
template <class Query, class R> Waited<R> wait_polling(Query&& query, R not_ready, int spins, double timeout_s) {
    R r;
    for (int spin = 0; spin < spins; ++spin)
        if ((r = query()) != not_ready) return {r, false};
    const auto t0 = std::chrono::steady_clock::now();
    while ((r = query()) == not_ready) {
        std::this_thread::sleep_for(std::chrono::microseconds(50));
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s) return {r, true};
    }
    return {r, false};
}

// ---- host doubles <-> engine precision ------------------------------------------------------------------------------------
// fp32 engines: arrays of at least this many scalars cross PCIe as doubles and are narrowed / widened on the device, smaller
// ones in a host loop (upload / download, ukf_runtime.hip)
constexpr size_t DEVICE_CONVERT_MIN = 16384;

// ---- packed covariances of the host-array forms ---------------------------------------------------------------------------
// `count` row-major D x D matrices <-> their lower triangles, row by row (entry (r, c), c <= r, at r (r + 1) / 2 + c of D (D + 1) / 2).
// pack_lower reads the lower triangle only; unpack_symmetric writes both triangles.
inline void pack_lower(const double* full, size_t count, int D, double* packed) {
    const size_t d = size_t(D), PK = d * (d + 1) / 2;
    for (size_t i = 0; i < count; ++i)
        for (size_t r = 0; r < d; ++r)
            for (size_t c = 0; c <= r; ++c) packed[i * PK + r * (r + 1) / 2 + c] = full[(i * d + r) * d + c];
}
inline void unpack_symmetric(const double* packed, size_t count, int D, double* full) {
    const size_t d = size_t(D), PK = d * (d + 1) / 2;
    for (size_t i = 0; i < count; ++i)
        for (size_t r = 0; r < d; ++r)
            for (size_t c = 0; c <= r; ++c) {
                const double v = packed[i * PK + r * (r + 1) / 2 + c];
                full[(i * d + r) * d + c] = v;
                full[(i * d + c) * d + r] = v;
            }
}

struct CycleLaunch {
    int first_cycle, cycles, slot;   // slot: the ring slot of first_cycle
    bool status_accumulate;          // the status word is the OR over ALL cycles of the call
};
// The launches of a call: the tuned layout runs multi-cycle launches (with a schedule: up to UKFB_MAX_MULTI_CYCLES each, the
// schedule travels in the kernel arguments); the one-wavefront-per-filter layouts have no multi-cycle kernel, one launch per cycle.
struct CyclePlan {
    int cycles, slots, first_slot;
    bool multi;       // multi-cycle launches (the tuned layout), else one single-cycle launch per cycle
    int per_launch;   // cycles of a launch, the last one's excepted
    CyclePlan(int cycles_, int slots_, int first_slot_, bool tuned, bool schedule)
        : cycles(cycles_), slots(slots_), first_slot(first_slot_), multi(tuned),
          per_launch(!tuned ? 1 : (schedule ? UKFB_MAX_MULTI_CYCLES : std::max(cycles_, 1))) {}
    int launches() const { return int((int64_t(cycles) + per_launch - 1) / per_launch); }
    CycleLaunch operator[](int k) const {
        const int c0 = k * per_launch;
        return {c0, std::min(per_launch, cycles - c0), int((int64_t(first_slot) + c0) % slots), k > 0};
    }
};

// ---- workspace sizing ---------------------------------------------------------------------------------------------------
// model-class buckets (ukf_buckets.hip): blocks of BK_BLOCK filters for the count and scatter kernels
constexpr int BK_THREADS = 256, BK_PER_THREAD = 4, BK_BLOCK = BK_THREADS * BK_PER_THREAD;
constexpr int BUCKET_INLINE_BLOCKS = 2048;   // up to 2 M filters: every scatter block sums 3 x 2048 counts at most
constexpr int64_t BUCKET_MIN_FILTERS = 16384;

inline bool buckets_apply(bool per_filter_models, const ukfb_config& cfg, int64_t cap) {
    return per_filter_models && cfg.bucket_models && cfg.lanes_per_filter == 16 && cap >= BUCKET_MIN_FILTERS && cap <= 0x7fffffff - 16;
}

struct BucketGeometry {
    int blocks;
    int64_t items;        // entries of the list a launch covers: every class padded to a multiple of 4 (an upper bound)
    size_t list;          // entries of the filter list
    size_t count_words;   // [3][blocks] counts, [3][blocks] exclusive prefix sums, [3] totals (+ 1 pad)
    bool inline_scan;     // the scatter blocks sum the counts themselves (no scan launch)
};
inline BucketGeometry bucket_geometry(int64_t n) {
    const int blocks = int((n + BK_BLOCK - 1) / BK_BLOCK);
    // sum of three counts each rounded up to 4 <= n + 9, itself rounded up to whole wavefronts
    return {blocks, (n + 3 + 3 + 3) / 4 * 4, size_t(n) + 16, size_t(6) * blocks + 4, blocks <= BUCKET_INLINE_BLOCKS};
}

struct Carver {   // bump allocator over a workspace (256-byte aligned pieces); a NULL base only measures
    char* base;
    size_t used = 0;
    explicit Carver(void* b) : base(static_cast<char*>(b)) {}
    template <class P> P* take(size_t count) {
        P* p = base ? reinterpret_cast<P*>(base + used) : nullptr;
        used += (count * sizeof(P) + 255) / 256 * 256;
        return p;
    }
};

// ---- filter lifecycle (ukfb_gather_filters_dev / scatter / retire / compact) ------------------------------------------------
// Record movers: one 16-lane row per record, four records per wavefront, LC_THREADS / LC_ROW records per block.  Compact counts
// and ranks groups in blocks of LC_COUNT_BLOCK; its move kernel has a FIXED grid (the pair count is known to the device only).
constexpr int LC_THREADS = 256, LC_ROW = 16, LC_ROWS_PER_BLOCK = LC_THREADS / LC_ROW;
constexpr int LC_PER_THREAD = 4, LC_COUNT_BLOCK = LC_THREADS * LC_PER_THREAD;
constexpr int LC_MOVE_MAX_BLOCKS = 2048, LC_MAX_GROUP = 8;
constexpr int64_t LC_MAX_ITEMS = 0x7fffffff;   // lists and filter indices are int32
// gather and scatter.  has_records: the struct pointer; the has_* / noise flags are those of its fields
inline Verdict check_lifecycle_args(int64_t capacity, int64_t n, bool has_records, bool scatter, bool has_mu, bool has_cov, bool has_noise,
                                    bool noise_per_filter) {
    if (!has_records) return {UKFB_ERR_INVALID_ARG, "the records must not be NULL"};
    if (n < 0 || n > LC_MAX_ITEMS) return {UKFB_ERR_OUT_OF_RANGE, "0 <= n <= INT32_MAX"};
    if (capacity < 1 || capacity > LC_MAX_ITEMS) return {UKFB_ERR_OUT_OF_RANGE, "filter indices are int32: capacity <= INT32_MAX"};
    if (scatter && (!has_mu || !has_cov)) return {UKFB_ERR_INVALID_ARG, "scatter: mu and cov_packed must not be NULL"};
    if (scatter && has_noise && !noise_per_filter)
        return {UKFB_ERR_INVALID_ARG, "scatter: noise records need per-filter noise storage: call ukfb_set_process_noise_per_filter first"};
    return {};
}
inline Verdict check_compact_args(int64_t capacity, int group) {
    if (group < 1 || group > LC_MAX_GROUP) return {UKFB_ERR_INVALID_ARG, "1 <= group <= 8"};
    if (capacity < 1 || capacity > LC_MAX_ITEMS) return {UKFB_ERR_OUT_OF_RANGE, "filter indices are int32: capacity <= INT32_MAX"};
    if (capacity % group != 0) return {UKFB_ERR_INVALID_ARG, "capacity must be a multiple of group"};
    return {};
}
inline int64_t lifecycle_record_blocks(int64_t n) { return (n + LC_ROWS_PER_BLOCK - 1) / LC_ROWS_PER_BLOCK; }
inline int64_t lifecycle_item_blocks(int64_t n) { return (n + LC_THREADS - 1) / LC_THREADS; }
struct LifecycleGeometry {
    int64_t groups;        // G = capacity / group
    int count_blocks;      // blocks of the count and rank kernels
    int move_blocks;       // the move kernel's fixed grid: rows stride over the pairs the device counted
    int64_t pair_cap;      // entries of each of the two pair arrays (holes, movers): min(L, G - L) <= G / 2
    size_t ws_words;       // 32-bit words of the engine's lifecycle workspace (sized for group = 1, so that it serves every group)
    size_t owner_off, counts_off, before_off, totals_off, hole_off, mover_off;   // word offsets of its pieces (64-word aligned)
};
inline LifecycleGeometry lifecycle_geometry(int64_t capacity, int group) {
    LifecycleGeometry g{};
    g.groups = capacity / group;
    g.count_blocks = int((g.groups + LC_COUNT_BLOCK - 1) / LC_COUNT_BLOCK);
    g.pair_cap = g.groups / 2 + 1;
    const int64_t rows = (g.groups / 2) * group;   // the most filters a call can move
    g.move_blocks = int(std::max<int64_t>(1, std::min<int64_t>(lifecycle_record_blocks(rows), LC_MOVE_MAX_BLOCKS)));
    const size_t max_blocks = size_t((capacity + LC_COUNT_BLOCK - 1) / LC_COUNT_BLOCK), max_pairs = size_t(capacity / 2 + 1);
    auto piece = [&g](size_t words) {
        const size_t at = g.ws_words;
        g.ws_words += (words + 63) / 64 * 64;
        return at;
    };
    g.owner_off = piece(size_t(capacity));
    g.counts_off = piece(max_blocks);
    g.before_off = piece(max_blocks);
    g.totals_off = piece(4);
    g.hole_off = piece(max_pairs);
    g.mover_off = piece(max_pairs);
    return g;
}

// bytes of workspace process_events_device needs for n events (an upper bound that does not depend on hipCUB's
// temporary-storage query: 4x the key/value arrays covers rocPRIM's double buffers)
inline size_t events_workspace_bytes(int64_t n) {
    const size_t ne = size_t(n);
    // 4 index + 2 time-key + 2 filter-key + head/start/rank/rank_sorted/off + compact events (int32, int64, int32,
    // 12 scalars of <= 8 bytes) + alignment slack + radix-sort temporaries
    return (4 * 4 + 2 * 8 + 2 * 4 + 5 * 4 + 4 + 8 + 4 + 12 * 8) * ne + 32 * 256 + (size_t(64) << 20) / 4 + 24 * ne;
}

// Split launches (ukf_launch.inc.hpp): direct launches of SPLIT_MIN_FILTERS <= n < split_max filters on an engine with a second
// stream run as two halves; the first covers whole wavefronts of 4 filters
constexpr int64_t SPLIT_MIN_FILTERS = 16384;
inline bool split_launch(bool indirect, bool no_split, bool has_stream_b, bool split_streams, int64_t n, int64_t split_max) {
    return !indirect && !no_split && has_stream_b && split_streams && n >= SPLIT_MIN_FILTERS && n < split_max;
}
inline int64_t split_first_half(int64_t n) { return (n / 2 + 3) / 4 * 4; }

// ---- kernel level of a tuned launch (ukf_kernel16<..., PLAIN>): what the kernel may take as compile-time facts -----------
//   streams only (level 1)  no per-filter timestamps / time steps / activity flags, the accept-any gate, a fresh status word
//   plain        (level 2)  ... and ONE full-3-vector measurement model for the launch (prediction-only launches: level 1 = 2)
// Indirect launches qualify for level 1 when their list is a bucketed filter list (event rounds carry timestamps); multi-cycle
// launches for level 2 when they have no schedule.
struct LaunchFacts {
    bool timestamps = false, dt_array = false, active = false, status_accumulate = false, gate = false;
    bool indirect = false, bucketed = false, multi = false, schedule = false, update = false, meas_per_filter = false;
    int meas_uniform = -1;
};
inline int kernel_level(int engine_model, const LaunchFacts& f) {
    const bool streams_only = !f.timestamps && !f.dt_array && !f.active && !f.status_accumulate && !f.gate &&
                              (!f.multi || !f.schedule) && (!f.indirect || f.bucketed);
    if (!streams_only) return 0;
    const bool full3 = !f.meas_per_filter && (engine_model != UKFB_MODEL_POSE ? f.meas_uniform == UKFB_MEAS_ORIENT_BODYVEL3
                                                                              : (f.meas_uniform == UKFB_MEAS_POS3 ||
                                                                                 f.meas_uniform == UKFB_MEAS_VEL3 ||
                                                                                 f.meas_uniform == UKFB_MEAS_ANGVEL3));
    if (f.indirect) return 1;
    if (f.multi) return full3 ? 2 : 0;
    if (!f.update) return 2;
    return full3 ? 2 : 1;
}

}  // namespace ukfb
