/*
 * msckf_mi355x.h -- C-ABI of the MI355X-native MSCKF measurement-update engine.
 *
 * This is the drop-in boundary for ONE path of the reference
 * (ValerioSpagnoli/Monocular-Visual-Inertial-MSCKF):
 *
 *     MSCKF.update(self, features: Dict[int, Feature]) -> None     src/msckf/MSCKF.py:570-609
 *       + the covariance half of MSCKF.correct(...)                 src/msckf/MSCKF.py:611-614
 *
 * i.e. per-feature residual/Jacobian stack (MSCKF.py:497-552, Camera.py:54-67),
 * left-nullspace projection (:554-559), chi-square gate (:561-568), stacking
 * (:581-588), QR compression (:594-598), Kalman gain (:604-607) and the
 * Joseph-form covariance update with symmetrisation (:612-614).
 * The state injection half of `correct` (:616-661, N+1 3x3 exp-maps) stays on
 * the host (Python, see monocular-visual-inertial-msckf_amd/api.py) unless the
 * nominal state is resident too (msckf_set_nominal ... msckf_commit_inject).
 *
 * Conventions
 *   - plain pointers and sizes, row-major, float64 ("double") unless stated;
 *   - "host" pointers are caller-owned and not retained past the call;
 *   - N = number of camera clones; d = 15 + 6 N is the error-state size, ordered
 *     [dtheta, db_g, dv, db_a, dp | per clone dtheta_c, dp_c]   (MSCKF.py:171, :258-261);
 *   - a clone's *slot* is its position in the reference's ordered
 *     `state.cameras` dict at call time (MSCKF.py:539), NOT its key;
 *   - feature tracks are CSR: view_ptr[F+1] indexes obs_uv / obs_slot;
 *   - return value: 0 = state updated, 1 = no-op (no feature passed the gate or
 *     F == 0: dx = 0, P_out = P, mirrors the early returns MSCKF.py:584-585,
 *     :591-592), < 0 = error (see msckf_strerror).
 *   - one context per host thread; calls on a context are serialised.
 *   - msckf_create starts a few host worker threads per context (CPU work only, no HIP calls: the copies into the
 *     pinned upload image, the validation loop and the covariance staging copies of msckf_update are split over them;
 *     pinned next to the creating thread).  Environment: MSCKF_HOST_THREADS (default 3, 0 = none), MSCKF_HOST_PAR_MIN (smallest batch that is
 *     split, default 1024 features), MSCKF_HOST_SPIN_US (how long idle workers poll before they sleep, default 1000).
 *   - waiting: msckf_update, msckf_get_result, msckf_get_covariance and msckf_sync return with the device drained of
 *     everything their results depend on; msckf_set_features, msckf_set_poses, msckf_commit_covariance, msckf_run,
 *     msckf_run_rows and msckf_run_fix leave their work in the context's stream (host arrays passed in are copied
 *     before the call returns).
 *   - tuning switches of the K5 plan (diagnostics; the defaults are the measured best): MSCKF_LEAF_TARGET (leaf workgroups
 *     aimed at per batch, default 240), MSCKF_LS_BIG_BATCH (from this many features on the 60-column leaves run twelve
 *     wavefronts, default 4000), MSCKF_LS_TALL (90-column leaves with 56-row blocks, default 1; 0 = 32-row blocks).
 */
#ifndef MSCKF_MI355X_H
#define MSCKF_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSCKF_ABI_VERSION 2

#define MSCKF_OK 0
#define MSCKF_NOOP 1
#define MSCKF_ERR_ARG (-1)          /* bad argument / size over the context's capacity      */
#define MSCKF_ERR_HIP (-2)          /* HIP runtime failure (msckf_last_error has the text)  */
#define MSCKF_ERR_NO_DEVICE (-3)    /* no usable gfx950 device                              */
#define MSCKF_ERR_NOT_SPD (-4)      /* the joint innovation covariance S of the stacked rows is
                                       not positive definite: K6-K7 met a pivot that is not a
                                       positive normal number.  dx = 0, P_out = the prior.  (The
                                       reference inverts such an S as it is, MSCKF.py:606;
                                       numpy.linalg.inv raises for an exactly singular one only.)
                                       A single track's gate matrix that is not SPD is no error:
                                       see msckf_stats.not_spd                               */
#define MSCKF_ERR_STATE (-5)        /* call order (e.g. run before set_state/set_features)  */
#define MSCKF_ERR_DUP_SLOT (-6)     /* a track observes the same clone slot twice           */

#define MSCKF_FLAG_TREE_PLAN 1      /* K5: always the merge tree (default: the band pipeline
                                       whenever every track spans <= 15 clone slots,
                                       see msckf_band_rule)                                */

#define MSCKF_FLAG_BAND_ONLY 2      /* K5: tracks of more than 10 clone slots are NOT split: tracks of
                                       11 - 15 slots take the 90-column band tiles, wider ones the merge tree  */

#define MSCKF_FLAG_WIDE_STORE 4     /* a context created with max_track > MSCKF_MAX_TRACK_ROW (fp64) gets the track store:
                                       rows of max_track views.  Without it the msckf_tracks_* calls of such a context
                                       answer MSCKF_ERR_ARG, as they did before the flag existed; with max_track <=
                                       MSCKF_MAX_TRACK_ROW it changes nothing.  With MSCKF_DTYPE_F32 and max_track >
                                       MSCKF_MAX_TRACK_ROW: msckf_create answers MSCKF_ERR_ARG (the f32 stack keeps
                                       MSCKF_MAX_TRACK views a track, rows of more could never be loaded)          */

#define MSCKF_DTYPE_F64 0
#define MSCKF_DTYPE_F32 1

#define MSCKF_MAX_TRACK 31          /* views of a track the NARROW K1-K4 kernels take (k_feature: one lane per measurement
                                       row, 2M+1 rows fit one wavefront); longer tracks go to k_feature_wide            */
#define MSCKF_MAX_TRACK_ROW 32      /* views a row of a NARROW context's track store may hold (max_track <= this): a track of
                                       MSCKF_MAX_TRACK views can take the newest clone's view (msckf_tracks_frame); a batch
                                       track of such a context still holds at most MSCKF_MAX_TRACK.  The per-row kernels
                                       give such a row a 32-lane group.  Above it a context is a wide-track context    */
#define MSCKF_MAX_TRACK_WIDE 64     /* views of a batch track on a context created with max_track > MSCKF_MAX_TRACK_ROW
                                       (fp64 only), and with MSCKF_FLAG_WIDE_STORE of a row of its track store (one
                                       wavefront per row: a row and a batch track have ONE limit there, max_track, and a
                                       full row refuses a further view as a 32-view row does).
                                       k_feature_wide keeps, per workgroup, the track's D, V, Z, r rows and the
                                       packed lower triangle of the gate matrix with the residual row in LDS:
                                       2 V^2 + 43.5 V + 1105 doubles at V views = 12081 doubles = 94.4 KiB at 64 (the
                                       160 KiB of a CU would hold V = 88).  64 is where the other holders of a track end:
                                       k_gather walks a track in two passes of 32 lanes, k_fold's leaves map a track's
                                       slots through 64 words per wavefront, and the gate's strip holds 8 tiles of 16
                                       columns of S (2 V - rank <= 128 rows) in accumulators                            */

typedef struct msckf_ctx msckf_ctx;

typedef struct msckf_config {
    int32_t abi_version;            /* MSCKF_ABI_VERSION                                    */
    int32_t device;                 /* HIP device ordinal                                   */
    int32_t max_clones;             /* capacity: N  (<= 221, else MSCKF_ERR_ARG)            */
    int32_t max_features;           /* capacity: F                                          */
    int32_t max_track;              /* capacity: M  (<= MSCKF_MAX_TRACK_WIDE, else MSCKF_ERR_ARG).  Up to MSCKF_MAX_TRACK: the
                                       batch limit.  MSCKF_MAX_TRACK_ROW: the track store's rows hold that many views, the
                                       batch limit stays MSCKF_MAX_TRACK.  More: the batch limit (fp64; an f32 context keeps
                                       MSCKF_MAX_TRACK), tracks of more than MSCKF_MAX_TRACK views take k_feature_wide and the
                                       merge tree; such a context has a track store on request only (MSCKF_FLAG_WIDE_STORE:
                                       rows of max_track views; without the flag msckf_tracks_*: MSCKF_ERR_ARG) and
                                       a batch with such a track takes no part in a sharded update (MSCKF_ERR_STATE)   */
    int32_t leaf_rows;              /* 0 = default; target stacked rows per QR leaf         */
    int32_t merge_arity;            /* 0 = default; max children per QR tree node           */
    int32_t flags;                  /* MSCKF_FLAG_*; 0 = defaults                           */
    int32_t dtype;                  /* MSCKF_DTYPE_F64 (reference arithmetic, 1e-8 parity) or
                                       MSCKF_DTYPE_F32: fp32 STORAGE of the stacked system (K4 output,
                                       the dominant HBM traffic) and the Joseph covariance update
                                       (MSCKF.py:612-614) on the f32 matrix cores; K1-K3, the QR
                                       accumulators and the Cholesky stay fp64.  Tolerance of this
                                       mode: DESIGN.md section 5 (1e-4 dx / 1e-5 P+)            */
    int32_t reserved0;
} msckf_config;

/* Filled by msckf_get_stats / msckf_update (nullable there). Times are device
 * times from HIP events on the context's stream, in microseconds. */
typedef struct msckf_stats {
    int32_t n_features;
    int32_t n_accepted;
    int32_t n_rejected;             /* reference counter number_of_residuals_discarded_for_gasting_test, MSCKF.py:578 */
    int32_t stacked_rows;           /* m = sum of q_j over accepted features                */
    int32_t n_leaves;
    int32_t n_levels;               /* levels of the K5 plan (tree levels, or leaves + group merge levels + root sweep) */
    int32_t not_spd;                /* tracks whose gate matrix S_j = H_o P H_o^T + sigma^2 I met a pivot that is not > 0
                                       (an indefinite or non-finite S_j; a NaN or infinite inverse-depth point ends here,
                                       a NaN or infinite observation in n_rejected: its S_j is sound, its gamma is NaN).
                                       The contract: such a track is dropped BEFORE the chi-square test, counted here and
                                       NOT in n_rejected, its accepted[] byte is 0, and dx / P_out are those of the batch
                                       without it.  A deliberate departure from the reference, which inverts whatever S_j
                                       it gets and gates on the number that comes out (MSCKF.py:561-568)               */
    int32_t k5_launches;            /* launches they took in the last run (a merge level streamed to the root rides in its launch) */
    float us_total;                 /* whole device pipeline                                */
    float us_feature;               /* K1-K3 kernel                                         */
    float us_qr;                    /* K5 tree                                              */
    float us_gain;                  /* K6-K7 kernels                                        */
    float us_host_prep;             /* host-side sort + tree plan of the last set_features  */
    float us_h2d;                   /* last host->device upload                             */
    float us_d2h;                   /* last device->host download                           */
    float reserved2;
} msckf_stats;

/* ---- lifetime ---------------------------------------------------------- */
int msckf_create(msckf_ctx** out, const msckf_config* cfg);
void msckf_destroy(msckf_ctx* ctx);
const char* msckf_strerror(int code);
const char* msckf_last_error(const msckf_ctx* ctx);   /* text of the last HIP failure */
int msckf_device_count(void);                          /* gfx950 devices visible       */

/* ---- one-shot drop-in: host arrays in, host arrays out ----------------- *
 * Replaces the arithmetic of MSCKF.update (MSCKF.py:570-609) and the
 * covariance update of MSCKF.correct (:612-614).
 *   P        d*d      state.covariance            (MSCKF.py:76)
 *   cam_R    N*9      Camera.T_W_Ci.R  per slot   (Camera.py:10, MSCKF.py:507)
 *   cam_t    N*3      Camera.T_W_Ci.t             (MSCKF.py:508)
 *   cam_R0/t0         Camera.T_W_Ci_null.R / .t   (MSCKF.py:509-510)
 *   gravity  3        state.imu.W_gravity         (MSCKF.py:529-530)
 *   Kinv     9        inverse of self.K           (MSCKF.py:519)
 *   sigma             self.sigma_image            (MSCKF.py:562, :589)
 *   view_ptr F+1, obs_uv 2*sumM (pixels, Feature.keypoints), obs_slot sumM
 *   idp_base F*3, idp_m F*3, idp_rho F  InverseDepthPoint.{base,m,rho} (geometry.py:53-71)
 *   chi2_crit[n_crit]: chi2.ppf(0.95, dof) for dof = 0..n_crit-1 (MSCKF.py:565-566);
 *                      n_crit must exceed 2*max(M)
 * outputs (host): dx[d] = delta_x (MSCKF.py:607), P_out[d*d] = covariance after
 * :613-614, accepted[F] gate result per feature in input order, stats nullable. */
int msckf_update(msckf_ctx* ctx, int32_t N, const double* P,
                 const double* cam_R, const double* cam_t,
                 const double* cam_R0, const double* cam_t0,
                 const double* gravity, const double* Kinv, double sigma,
                 int32_t F, const int32_t* view_ptr, const double* obs_uv,
                 const int32_t* obs_slot, const double* idp_base,
                 const double* idp_m, const double* idp_rho,
                 const double* chi2_crit, int32_t n_crit,
                 double* dx, double* P_out, uint8_t* accepted, msckf_stats* stats);

/* ---- per-view measurement noise ---------------------------------------- *
 * The reference weights every view alike: R_o = sigma^2 I (MSCKF.py:589), and sigma^2 I in the gate (:562).
 * With sigma_view[sumM] (input order of the views, the order of obs_uv; every entry finite and > 0, same
 * units as sigma) the update is the reference's with R_o = blockdiag(sigma_v^2 I_2), and the two rows of
 * view v carry sigma_v^2 in the gate.  It is computed in whitened form: with w_v = sigma / sigma_v (the
 * fp64 quotient, exactly 1 where sigma_v == sigma) the view's residual r_i, its OC-projected H_xi
 * (:532-540) and its H_fi (:536) are multiplied by w_v BEFORE the null-space projection (:550).  The left
 * null space is then that of diag(w) H_f, the projected noise is sigma^2 I again, and gamma, K, dx and P+
 * are those of the R_o form; everything behind K1 is the unweighted code.  sigma_view == sigma everywhere
 * gives bit for bit the result without weights; sigma_view == sigma / c everywhere that of sigma / c.
 *
 * msckf_update_sigma is msckf_update with the array (nullable) behind idp_rho; msckf_update calls it with
 * NULL.  The weights ride in the pinned upload image beside obs_uv, the host workers validate them with the
 * other arrays, and the device brings them into the pipeline's order with the tracks. */
int msckf_update_sigma(msckf_ctx* ctx, int32_t N, const double* P,
                       const double* cam_R, const double* cam_t,
                       const double* cam_R0, const double* cam_t0,
                       const double* gravity, const double* Kinv, double sigma,
                       int32_t F, const int32_t* view_ptr, const double* obs_uv,
                       const int32_t* obs_slot, const double* idp_base,
                       const double* idp_m, const double* idp_rho, const double* sigma_view,
                       const double* chi2_crit, int32_t n_crit,
                       double* dx, double* P_out, uint8_t* accepted, msckf_stats* stats);
/* Resident path: the weights of the loaded batch, after msckf_set_features, msckf_tracks_load or
 * msckf_tracks_load_where (where msckf_set_tracks stands in the call order; like it, it returns with the
 * upload done).  NULL clears them.  They belong to the batch: the next batch load clears them, and so does
 * msckf_set_state (w_v was taken at the sigma it replaces).  msckf_run, msckf_run_compress,
 * msckf_run_timed, msckf_run_select + msckf_run and msckf_replan honour them; msckf_debug_gate reports the
 * weighted gamma.  Errors, with nothing changed: MSCKF_ERR_STATE without a loaded batch, MSCKF_ERR_ARG for
 * an entry that is not finite or not > 0. */
int msckf_set_view_sigma(msckf_ctx* ctx, const double* sigma_view);

/* ---- robust per-view weights (NOT in the reference) --------------------- *
 * The reference's only defence against a bad observation is the gate (MSCKF.py:562-579), all or nothing per
 * track: one mismatched keypoint costs every good view of its track.  With a loss set here, every call that
 * runs K1 (msckf_update, msckf_update_sigma, msckf_run, msckf_run_timed, msckf_run_compress, the retry inside
 * msckf_get_result) first reweights each view once at the linearisation point -- iteratively reweighted least
 * squares with the one iteration an EKF step has -- from the batch's inverse-depth points as they stand (behind
 * msckf_run_select and its refinement), the resident clone poses and K^-1, in fp64 in both dtypes:
 *   e_v     the view's two residual components as K1 forms them (z / z_w - p_xy / p_z, normalised image coordinates)
 *   b_v     the base weight: sigma / sigma_v where per-view noise is in force (above), else 1
 *   s_v   = b_v |e_v|_2 / sigma                       the whitened residual norm
 *   omega   Huber: min(1, k / s)      Cauchy: 1 / (1 + (s / k)^2)
 *   phi_v = max(sqrt(omega(s_v)), w_min)              exactly 1 under Huber up to s_v == k, and 1 where s_v is not finite
 *   w_v   = b_v phi_v                                 what K1 multiplies the view's rows of r, H_x and H_f by
 * A track the run skips (msckf_run_select: no MSCKF_SEL_VALID) keeps w_v = b_v and reports s_v = 0.  Everything
 * behind K1 is the code that runs without the option, and the gate's degrees of freedom stay 2M - rank.  The
 * weights of a run live in an array of their own: the base weights are never overwritten, so repeated runs of
 * one batch form the same weights and never compound them.
 *
 * msckf_set_robust: a setting of the context.  Off after msckf_create; it survives msckf_set_state and batch
 * loads; NULL or loss 0 turns it off, and with it off the engine launches and computes exactly what it did
 * before the option existed.  MSCKF_ERR_ARG, with nothing changed: loss outside 0..2, reserved != 0, k not
 * finite or not > 0, w_min outside (0, 1].  Typical: Huber k = 1.345, Cauchy k = 2.385, w_min = 0.05.
 * msckf_get_view_weights: waits for the stream; w_v and s_v of the last run in the caller's view order (sumM
 * each, the order of obs_uv; any pointer may be NULL) and n_down, the number of views with phi_v < 1.
 * MSCKF_ERR_STATE when the loaded batch's last run did not have the option on, or its results have been voided
 * since (whatever voids msckf_get_result: a new batch, msckf_set_state, propagation, clone bookkeeping). */
#define MSCKF_ROBUST_OFF 0
#define MSCKF_ROBUST_HUBER 1
#define MSCKF_ROBUST_CAUCHY 2
typedef struct msckf_robust_params {
    int32_t loss;        /* MSCKF_ROBUST_* */
    int32_t reserved;    /* 0 */
    double k;            /* the loss's scale, in whitened units (sigmas) */
    double w_min;        /* floor of phi, in (0, 1] */
} msckf_robust_params;
int msckf_set_robust(msckf_ctx* ctx, const msckf_robust_params* params);
int msckf_get_view_weights(msckf_ctx* ctx, double* w, double* s, int32_t* n_down);

/* ---- known landmarks: a prior on a track's point (NOT in the reference) --- *
 * Every track of the reference is a track of an unknown point: K2 projects [r | H_x] onto the left null space
 * of H_f (MSCKF.py:554-559), and a surveyed fiducial or a map point loses its position there.  A Gaussian
 * prior p ~ N(pbar, Sigma_p) on the point of track j is three more rows in front of that projection,
 *     [ H_f     ]     [ H_x ]     [ r                      ]      W^T W = Sigma_p^-1  (W = L^-1, Sigma_p = L L^T)
 *     [ sigma W ]     [ 0   ]     [ sigma W (pbar - p_lin) ]      p_lin = idp_base + idp_m / idp_rho
 * with noise sigma^2 I like every other row: the left null space of the (2M + 3) x 3 block has 2M columns, the
 * projected noise is sigma^2 I again, and the gate (2M degrees of freedom), K5 and K6-K7 are the code that runs
 * without priors.  It is the EKF update with residual r - H_f (pbar - p_lin), Jacobian H_x and noise
 * sigma^2 I + H_f Sigma_p H_f^T; a track of ONE view, which gives no rows without a prior, gives two with one.
 * Units: the prior's columns are K1's H_f as it stands, the block whose negative stands in the clone's position
 * columns (Camera.py:62, :66, MSCKF.py:536), so a shift of the point and the opposite shift of every observing
 * clone are the same thing to the filter; the reference's rho-scaled geometry is kept as it is.
 * Prior rows are not touched by per-view noise or the robust loss: those belong to views.  A prior so loose that
 * K2's rank test finds fewer than three pivots on the augmented block is not stacked: the track is rejected.
 *
 * MSCKF_PRIOR_AT_MEAN linearises a prior track at the prior's mean: rho' = 1 / |pbar - base|,
 * m' = (pbar - base) rho' stand in for the track's m, rho in everything that forms the run's K1 terms (the
 * robust weights' residual norms included).  Where |pbar - base| is not finite or 0 the track keeps its own
 * point.  The batch's m / rho (and the track store's rows) are never overwritten.
 *
 * msckf_set_point_priors (resident path): the priors of the loaded batch, in the caller's track order; NULL
 * clears them.  Call order and lifetime are msckf_set_view_sigma's: after the batch load, before or after
 * msckf_set_tracks / msckf_set_view_sigma / msckf_run_select / msckf_replan, before the run; the next batch
 * load and msckf_set_state clear them; propagation, msckf_set_poses and rows updates leave them.  msckf_run,
 * msckf_run_timed and the retry inside msckf_get_result honour them.  msckf_run_select knows nothing of them:
 * a skipped track stays skipped, a refreshed point becomes p_lin.  msckf_stats.stacked_rows counts 2M for an
 * accepted prior track.  The K5 plan of the loaded batch is made afresh (a prior track brings 2M rows, not
 * 2M - 3).  A prior on a long track that the batch load had split re-sorts the batch with every track in one
 * block (the route of a long track that cannot be split): MSCKF_ERR_STATE where that would lose what
 * msckf_set_tracks or msckf_run_select brought for a caller-supplied batch -- set such priors first.
 * Errors, with nothing changed: MSCKF_ERR_ARG for reserved != 0, unknown flags, a prior whose mean or
 * covariance has an entry that is not finite, whose covariance is not bitwise symmetric or has no Cholesky
 * factor with finite pivots > 0, a prior on a track of more than MSCKF_MAX_TRACK_PRIOR views, or an
 * MSCKF_DTYPE_F32 context; MSCKF_ERR_STATE without a loaded batch or under a group exchange.  While priors
 * are in force msckf_run_compress and the export / merge calls answer MSCKF_ERR_STATE.
 * msckf_update_prior: msckf_update_sigma with the priors behind sigma_view (NULL: msckf_update_sigma itself).
 * msckf_get_prior_distance: waits for the stream; d2[F] (caller's order) of the last run,
 * (pbar - p_lin)^T Sigma_p^-1 (pbar - p_lin) at the run's linearisation point, 0 for a plain or skipped track.
 * MSCKF_ERR_STATE when the loaded batch's last run had no priors or its results have been voided since. */
#define MSCKF_PRIOR_AT_MEAN 1
#define MSCKF_MAX_TRACK_PRIOR 30    /* 2M + 3 rows on 64 lanes */
typedef struct msckf_point_priors {
    const uint8_t* has;     /* F, the caller's track order; 0: a plain track                         */
    const double*  mean;    /* 3F, world frame; read where has[j]                                    */
    const double*  cov;     /* 9F, row-major 3x3; read where has[j]                                  */
    int32_t flags;          /* 0 | MSCKF_PRIOR_AT_MEAN                                               */
    int32_t reserved;       /* 0                                                                     */
} msckf_point_priors;
int msckf_set_point_priors(msckf_ctx* ctx, const msckf_point_priors* priors);
int msckf_update_prior(msckf_ctx* ctx, int32_t N, const double* P,
                       const double* cam_R, const double* cam_t,
                       const double* cam_R0, const double* cam_t0,
                       const double* gravity, const double* Kinv, double sigma,
                       int32_t F, const int32_t* view_ptr, const double* obs_uv,
                       const int32_t* obs_slot, const double* idp_base,
                       const double* idp_m, const double* idp_rho, const double* sigma_view,
                       const msckf_point_priors* priors,
                       const double* chi2_crit, int32_t n_crit,
                       double* dx, double* P_out, uint8_t* accepted, msckf_stats* stats);
int msckf_get_prior_distance(msckf_ctx* ctx, double* d2);

/* ---- resident path: the same update split so inputs can stay in HBM ---- */
/* Upload filter state read by update(): P, clone poses, gravity, K^-1, sigma, chi2 table. */
int msckf_set_state(msckf_ctx* ctx, int32_t N, const double* P,
                    const double* cam_R, const double* cam_t,
                    const double* cam_R0, const double* cam_t0,
                    const double* gravity, const double* Kinv, double sigma,
                    const double* chi2_crit, int32_t n_crit);
/* Upload one feature batch (the `features` dict of MSCKF.update): sorts the
 * tracks by first slot, plans the QR tree and copies everything to HBM.
 * The batch replaces the previous one, gate results included, so the call voids the
 * results of the last run (a rows run too): read and commit a run BEFORE the next
 * batch is loaded; behind it msckf_get_result and both commits return MSCKF_ERR_STATE. */
int msckf_set_features(msckf_ctx* ctx, int32_t F, const int32_t* view_ptr,
                       const double* obs_uv, const int32_t* obs_slot,
                       const double* idp_base, const double* idp_m,
                       const double* idp_rho);
/* Enqueue the whole device pipeline (K1..K7) on the context's stream; async. */
int msckf_run(msckf_ctx* ctx);
/* Enqueue `iters` back-to-back pipelines and time them with HIP events on the
 * context's stream. ms_total = wall between first launch and last completion.
 * If stage_us is non-NULL it receives 3 floats {feature, qr, gain}: the average
 * device time of each stage measured with per-stage events in a second pass. */
int msckf_run_timed(msckf_ctx* ctx, int32_t iters, float* ms_total, float* stage_us);
int msckf_sync(msckf_ctx* ctx);
/* Download results of the last run (any pointer may be NULL). Returns 0 / 1 / <0. */
int msckf_get_result(msckf_ctx* ctx, double* dx, double* P_out, uint8_t* accepted,
                     msckf_stats* stats);
/* Keep the updated covariance as the state for the next update (P <- P_out on device). */
int msckf_commit_covariance(msckf_ctx* ctx);

/* ---- f1: feature selection + triangulation in front of the update ---------- *
 * Replaces MSCKF.get_valid_features (MSCKF.py:458-495): the lost / too-short /
 * parallax tests, intersection_of_lines (geometry.py:274-303), the re-projection
 * into the anchor clone (Camera.py:13-52) and the refresh of the inverse-depth
 * point (geometry.py:61-71).  Candidates are the batch of msckf_set_features
 * (ALL tracks the caller would pass to get_valid_features, same order);
 * msckf_set_tracks adds what that function reads besides the views. */
typedef struct msckf_select_params {
    int32_t min_frames_lost;        /* MSCKFParameters.min_number_of_frames_to_be_lost   (clamped >= 1, MSCKF.py:119) */
    int32_t min_frames_tracked;     /* MSCKFParameters.min_number_of_frames_to_be_tracked (clamped >= 2, MSCKF.py:120) */
    int32_t use_parallax;           /* MSCKFParameters.use_parallax                                       */
    int32_t width, height;          /* Camera.width / .height (Camera.py:24-25)                           */
    int32_t refine_iters;           /* 0: off (the reference's linear point).  1..32: refine the triangulated point on the
                                       device, at most this many Levenberg-Marquardt trials (below); else MSCKF_ERR_ARG */
    double min_parallax_deg;        /* MSCKFParameters.min_parallax                                       */
    double K[9];                    /* Camera.K, row-major (Camera.py:20)                                 */
} msckf_select_params;

#define MSCKF_SEL_VALID 1           /* in valid_features: goes into the update          (MSCKF.py:492) */
#define MSCKF_SEL_LOST 2            /* in lost_features: the caller removes it afterwards (:468, :493)  */
#define MSCKF_SEL_REFRESHED 4       /* inverse-depth point was re-estimated              (:484-488)     */
#define MSCKF_SEL_REFINED 8         /* ... from the refined point (refine_iters > 0), not the linear one */

/* Per-view Feature.lines (line_base / line_dir 3*sumM, line_conf sumM; lines[i] belongs to
 * keypoints[i], MSCKF.py:410) and per-feature lost_for_n_frames / tracked_for_n_frames (F). */
int msckf_set_tracks(msckf_ctx* ctx, const double* line_base, const double* line_dir,
                     const double* line_conf, const int32_t* lost_for, const int32_t* tracked_for);
/* Enqueue the selection kernel (async).  It writes the flags and refreshes the inverse-depth
 * points in HBM; from then on msckf_run / msckf_run_compress process only the MSCKF_SEL_VALID
 * features of the batch (the others report accepted = 0 and are not counted as rejected),
 * until the next msckf_set_features or msckf_clear_selection. */
int msckf_run_select(msckf_ctx* ctx, const msckf_select_params* params);
/* Optional, between msckf_run_select and msckf_run: wait for the flags and plan the QR tree
 * over the valid features only (the plan of msckf_set_features covers every candidate).  Costs
 * one stream sync and the host-side plan; pays off when few candidates are valid. */
int msckf_replan(msckf_ctx* ctx);
int msckf_clear_selection(msckf_ctx* ctx);
/* Download the selection (any pointer may be NULL), input order: flags[F], idp_m[F*3] and
 * idp_rho[F] as they stand after the refresh, world[F*3] = triangulated point (NaN when the
 * feature was not triangulated; the reference's estimated_world_points, MSCKF.py:489). */
int msckf_get_selection(msckf_ctx* ctx, uint8_t* flags, double* idp_m, double* idp_rho, double* world);
/* Refinement of the triangulated points (msckf_select_params.refine_iters > 0; a second launch behind the selection
 * kernel, fp64 in both dtypes).  intersection_of_lines meets Feature.lines, which were stored with the pose each clone had
 * when the view was added; the update linearises about the RESIDENT poses.  For every track flagged MSCKF_SEL_VALID and
 * MSCKF_SEL_REFRESHED the device minimises c(x) = sum_i w_i |z_i - zhat_i(x)|^2 over x = (alpha, beta, rho), the
 * inverse-depth point in the anchor clone a = obs_slot[first view], under the resident poses:
 *     h_i = R_s^T (R_a [alpha, beta, 1]^T + rho (t_a - t_s)),  zhat_i = h_xy / h_z,  z_i = K^-1 [u, v, 1] dehomogenised,
 *     w_i = line_conf[i] -- the weights of the linear step; the per-view noise of msckf_set_view_sigma is NOT used here.
 * Levenberg-Marquardt from the linear point C = R_a^T (world - t_a), x0 = (C_x / C_z, C_y / C_z, 1 / C_z), attempted iff
 * C_z > 0 and every h_z > 0 at x0; lambda0 = 1e-3, (A + lambda diag A) d = g with A = sum w J^T J, g = sum w J^T e; a
 * trial is accepted iff every h_z > 0, it is finite and its cost is strictly smaller (then lambda <- max(lambda / 10,
 * 1e-12), stop when max|d| <= 1e-9 max(1, max|x|); else lambda <- 10 lambda, stop when lambda > 1e8); at most
 * refine_iters trials.  W = t_a + R_a [alpha, beta, 1]^T / rho is kept iff a trial was accepted, rho > 0 and W passes the
 * anchor in-image test of the linear point; then world <- W, idp_m / idp_rho are refreshed from W exactly as from the
 * linear point, and MSCKF_SEL_REFINED is set.  A track that is not kept stays as the linear step left it, and bits 1, 2, 4
 * never depend on refine_iters: the plan, msckf_replan and the update's feature set are those of refine_iters = 0, and the
 * write-back to the track store persists the refined point like any refreshed one.
 * msckf_get_select_refine: per track in input order (any pointer may be NULL) cost0 = c at the linear point, cost1 = c at
 * the result (= cost0 when it was not kept), trials; zeros for a track that was not attempted, and for all of them when the
 * last selection ran with refine_iters == 0.  MSCKF_ERR_STATE without a selection.  Waits for the kernels. */
int msckf_get_select_refine(msckf_ctx* ctx, double* cost0, double* cost1, int32_t* trials);

/* ---- f4: geometric consistency tests of the front end's matches ----------------- *
 * Replaces the per-(match, earlier view) loop of MSCKF.add_camera_measurements (MSCKF.py:332-412): the
 * epipolar test against every earlier view of the matched feature, or the homography test where the two
 * clones are closer than 1 cm.  Candidates are the batch of msckf_set_features (the tracks as they stand
 * BEFORE the new view); matched_uv[2 F] is the keypoint of the newest image matched to each of them (NaN for
 * a feature without a match), R_cur / t_cur the pose T_W_C of the newest clone, K the intrinsics.
 * result[F]: 0 the match is kept (the caller appends the view, :415-421), 1 it failed the epipolar test
 * (number_of_features_discarded_for_epipolar_test, :396), 2 the homography test
 * (number_of_features_discarder_for_homography_test, :378), 3 no match; fail_view[F] (nullable) the index of
 * the view that failed it, -1 otherwise.  Input order.  Blocking. */
typedef struct msckf_assoc_params {
    double K[9];                    /* Camera intrinsics, row-major                                   */
    double R_cur[9], t_cur[3];      /* T_W_Ci of state.cameras[state.imu.id]          (MSCKF.py:288-289) */
    double epipolar_threshold;      /* MSCKFParameters.epipolar_rejection_threshold   (:41)              */
    double homography_threshold;    /* MSCKFParameters.homography_rejection_threshold (:42)              */
} msckf_assoc_params;
int msckf_run_associate(msckf_ctx* ctx, const msckf_assoc_params* params, const double* matched_uv,
                        uint8_t* result, int32_t* fail_view);

/* ---- f2 / f3: the covariance steps either side of the update --------------- *
 * With these the covariance never leaves HBM between frames: msckf_set_state once
 * (N = 0 is allowed: the 15x15 IMU prior), then per IMU sample msckf_propagate, per
 * image msckf_augment -> msckf_set_features [-> msckf_set_tracks / msckf_run_select]
 * -> msckf_run -> msckf_get_result(dx only) -> msckf_commit_covariance ->
 * msckf_set_poses (poses after the host's state injection), and msckf_remove_clones
 * when the window is pruned.  Each call that changes N drops the feature batch. */
/* Covariance half of MSCKF.process_imu (MSCKF.py:236-244): P_II <- Phi P_II Phi^T + Q,
 * P_IC <- Phi P_IC, P_CI <- P_IC^T, P <- (P + P^T)/2.  Phi, Q: 15x15 row-major, built by
 * the host from the IMU state (:179-237; propagation.py does it for the Python mirror). */
int msckf_propagate(msckf_ctx* ctx, const double* Phi, const double* Q);
/* MSCKF.state_augmentation (MSCKF.py:250-265): append a clone with pose (R, t) (its null
 * pose is the same, Camera.py:11) and P <- sym([I; J] P [I; J]^T).  J15 = the 6x15
 * non-zero part of J (:259-261), row-major. */
int msckf_augment(msckf_ctx* ctx, const double* J15, const double* R, const double* t);
/* MSCKF.remove_cameras covariance half (MSCKF.py:751-757): drop the rows/columns and
 * poses of `n` clones given by their slots (positions at call time, any order). */
int msckf_remove_clones(msckf_ctx* ctx, int32_t n, const int32_t* slots);
/* Clone poses after the host applied the state correction (MSCKF.py:642-661). */
int msckf_set_poses(msckf_ctx* ctx, const double* cam_R, const double* cam_t,
                    const double* cam_R0, const double* cam_t0);
/* Download the resident prior covariance (d x d, d = 15 + 6 N) and N; P may be NULL. */
int msckf_get_covariance(msckf_ctx* ctx, double* P, int32_t* N);

/* ---- the nominal state resident beside the covariance --------------------- *
 * With these the filter loop between two msckf_set_features calls needs no host arithmetic and no round trip:
 *   MSCKF.process_imu (all samples of a frame)  -> msckf_propagate_imu      IMU.integrate + Phi, Q + covariance, one call
 *   MSCKF.state_augmentation                    -> msckf_augment_imu        clone pose and J from the resident IMU state
 *   MSCKF.correct                               -> msckf_commit_inject      P <- P+ and the state injection from dx in HBM
 * msckf_set_nominal uploads the record once (after msckf_set_state, which holds the clone poses); every call below
 * returns MSCKF_ERR_STATE before it.  The record is fp64 in both dtypes.
 * The older calls stay legal on such a context: msckf_set_poses (and msckf_set_state) override the clone poses,
 * msckf_augment appends the pose the caller gives; msckf_propagate and msckf_augment leave the IMU record alone (the
 * caller who mixes them keeps it consistent); msckf_remove_clones compacts the device arrays instead of re-uploading
 * the host's copy, which is stale after an injection until msckf_get_nominal refreshes it. */
typedef struct msckf_nominal {
    double R[9], t[3], v[3];        /* IMU.T_W_Ii.R / .t, IMU.v_W_Ii                         (IMU.py:27-28)      */
    double b_g[3], b_a[3];          /* IMU.gyroscope_bias, IMU.accelerometer_bias            (IMU.py:33-34)      */
    double R0[9], t0[3], v0[3];     /* IMU.T_W_Ii_null, IMU.v_W_Ii_null (IMU.py:38-39).  From the first
                                       msckf_propagate_imu on they follow the state, injections included: the
                                       reference holds the same objects for both (MSCKF.py:247-248)              */
    double gravity[3];              /* IMU.W_gravity                                                             */
    double planet_rate[3];          /* IMU.planet_angular_velocity                           (IMU.py:36)         */
    double Qc[144];                 /* continuous_noise_covariance, 12x12 row-major          (MSCKF.py:99-103)   */
    double T_I_C_R[9], T_I_C_t[3];  /* static extrinsics T_W_I^-1 T_W_C                      (MSCKF.py:252)      */
} msckf_nominal;
#define MSCKF_IMU_BATCH_MAX 64      /* samples of one msckf_propagate_imu (they travel in the kernel arguments)  */
int msckf_set_nominal(msckf_ctx* ctx, const msckf_nominal* s);
/* Download the record and the clone poses (cam_R N*9, cam_t N*3, nullable; null poses equal them); drains the stream. */
int msckf_get_nominal(msckf_ctx* ctx, msckf_nominal* s, double* cam_R, double* cam_t);
/* MSCKF.process_imu (MSCKF.py:160-248) for n consecutive RAW samples, 1 <= n <= MSCKF_IMU_BATCH_MAX (else
 * MSCKF_ERR_ARG): gyro, acc n*3, dt n.  The biases are subtracted on the device.  Two launches whatever n is (one
 * before the first clone), asynchronous.  The clone columns see the product of the n transitions, which rounds a few
 * ulp differently from n calls. */
int msckf_propagate_imu(msckf_ctx* ctx, int32_t n, const double* gyro, const double* acc, const double* dt);
/* MSCKF.state_augmentation (MSCKF.py:250-265) from the resident IMU state and T_I_C; asynchronous. */
int msckf_augment_imu(msckf_ctx* ctx);
/* msckf_commit_covariance, then MSCKF.correct's state injection (MSCKF.py:616-661) of this update's dx, read from HBM:
 * IMU state, biases, every clone pose and null pose.  Same return codes; a no-op (1) or failed update (< 0) leaves P
 * and the record untouched.  Asynchronous wherever msckf_commit_covariance is.
 * A run is injected ONCE: a second msckf_commit_inject of the same run returns MSCKF_ERR_STATE and touches neither P nor
 * the record (its dx would be added to the IMU state, the biases and every pose again).  msckf_commit_covariance stays
 * repeatable -- it copies the same P_out --, in front of msckf_commit_inject (which then injects once) and behind it. */
int msckf_commit_inject(msckf_ctx* ctx);

/* ---- direct measurement rows on the resident filter -------------------------- *
 * Every update kernel behind K5 takes T_H = [0 | T]: camera rows, zero on the 15 IMU columns.  These calls take any
 * other measurement -- a zero-velocity update at standstill, a position or velocity fix, a height, a pose from another
 * estimator, a row on a bias -- without leaving the resident path: m rows H (1 <= m <= MSCKF_MAX_ROWS) over the leading
 * n_cols of the d = 15 + 6 N error-state columns (1 <= n_cols <= d, row-major m x n_cols, the columns behind them are
 * zero and cost nothing: n_cols = 15 is the IMU-only case), the residual r[m] and the noise matrix R[m*m]:
 *     S = H P H^T + R = L L^T,   gamma = r^T S^-1 r,   K = P H^T S^-1,   dx = K r,
 *     P+ = (I - K H) P (I - K H)^T + K R K^T, symmetrised              (MSCKF.py:604-607, :612-614 with R for R_n)
 * Sign convention: r = z - h(nominal state), the measured value minus the predicted one.  Always fp64, also on an
 * MSCKF_DTYPE_F32 context.  Two launches, asynchronous like msckf_run, and the result lands where msckf_run's does:
 * msckf_get_result returns dx, P_out and stats (accepted may be NULL; accepted[0] is the verdict; n_features = 1,
 * n_accepted / n_rejected = 1 / 0 or 0 / 1, stacked_rows = m), msckf_commit_covariance / msckf_commit_inject keep it.
 * chi2_crit > 0 gates the update: it is applied iff gamma <= chi2_crit (<= 0: not gated); a NaN gamma (a non-finite r)
 * is a rejection either way.  A rejected update is a no-op: return code 1 from the three readers, dx = 0, P_out = the
 * prior.  A pivot of S that is not a positive normal number (R indefinite, or a non-finite H or R) is
 * MSCKF_ERR_NOT_SPD from the readers, P and the nominal state unchanged.  Two runs on the same inputs give the same
 * bits, and P_out is bit-symmetric.
 * The loaded feature batch is not touched: after a rows update is committed, msckf_run is the camera update of that
 * batch on the new P and the new poses.
 * Errors, nothing launched: MSCKF_ERR_STATE without msckf_set_state; MSCKF_ERR_ARG for m or n_cols out of range, a
 * null pointer, or an R that is not bitwise symmetric. */
#define MSCKF_MAX_ROWS 32
int msckf_run_rows(msckf_ctx* ctx, int32_t m, int32_t n_cols, const double* H, const double* r,
                   const double* R, double chi2_crit);
/* Three rows on the resident nominal state (msckf_set_nominal first, else MSCKF_ERR_STATE): the device forms
 * r = z - t_WI (columns 12..14: the error state is ordered theta, b_g, v, b_a, p, as msckf_commit_inject reads dx)
 * or r = z - v (columns 6..8) in stream order, behind whatever msckf_propagate_imu left
 * pending, with no read-back.  z[3], R[9] (bitwise symmetric); `which` unknown: MSCKF_ERR_ARG.  A zero-velocity update is
 * MSCKF_FIX_VELOCITY with z = 0. */
#define MSCKF_FIX_POSITION 1
#define MSCKF_FIX_VELOCITY 2
int msckf_run_fix(msckf_ctx* ctx, int32_t which, const double* z, const double* R, double chi2_crit);
/* gamma and the verdict (1 applied, 0 rejected or not SPD -- gamma is NaN then) of the last rows run; waits for it.
 * MSCKF_ERR_STATE when the last run was not a rows run.  Either pointer may be NULL. */
int msckf_get_rows_gate(msckf_ctx* ctx, double* gamma, int32_t* applied);

/* ---- the track store: views and bases resident, batches by track id -------- *
 * The feature batch is the last input of the resident loop that depends on the clone poses: every Line.base is the
 * clone's own position array (MSCKF.py:410, :430-431) and every InverseDepthPoint.base that of the clone the track was
 * created in (geometry.py:55), so both move with each injection.  The store keeps every floating-point field of the
 * tracks in HBM (fp64 in both dtypes; capacity max_features tracks x max_track views, allocated on first use; on a context with
 * max_track > MSCKF_MAX_TRACK_ROW only with MSCKF_FLAG_WIDE_STORE, else every call of this section answers MSCKF_ERR_ARG) and which
 * track has views in which clone slots on the host, inside the context.  A frame sends its new keypoints
 * (msckf_tracks_observe) and asks for a batch by track id (msckf_tracks_load); the bases are resolved on the device from
 * the resident clone positions.  Works on any context with a state; the "newest clone" is slot N - 1.
 *   MSCKF.add_camera_measurements :403-411, :420-434  -> msckf_tracks_observe
 *   MSCKF.get_valid_features / update candidates      -> msckf_tracks_load      (= msckf_set_features + msckf_set_tracks)
 *   MSCKF.remove_features :739-741                    -> msckf_tracks_remove
 *   MSCKF.remove_cameras :760-779                     -> msckf_remove_clones    (views dropped, slots renumbered, anchors frozen)
 * msckf_run_select on a batch that came from the store writes the refreshed m / rho of the MSCKF_SEL_REFRESHED tracks back
 * to their rows (the reference's refresh persists, :488), in the stream behind the selection kernel; deleting tracks
 * (msckf_tracks_remove, msckf_remove_clones) ends that for the loaded batch, so select first, as the reference does.
 * msckf_set_state empties the store (slots lose their meaning); msckf_set_poses, msckf_augment and msckf_augment_imu leave
 * it alone.  An erroring call leaves the store exactly as it was.  A caller who never uses these calls sees no change. */
int msckf_tracks_reset(msckf_ctx* ctx);
/* One view of the newest clone for each listed track: dir = R_new (K^-1 [u, v, 1]) with the resident rotation and the K^-1
 * of msckf_set_state, conf = score.  An unknown id creates a track: anchor = the newest clone, m = dir / |dir|
 * (geometry.py:56-58), rho = 0.1 (:59).  Asynchronous.  MSCKF_ERR_STATE when N = 0; MSCKF_ERR_DUP_SLOT when a track already
 * has a view of the newest clone or an id appears twice; MSCKF_ERR_ARG past either capacity (or a negative id). */
int msckf_tracks_observe(msckf_ctx* ctx, int32_t n, const int32_t* ids, const double* uv /*2n*/, const double* score /*n*/);
/* Delete tracks.  An unknown (or repeated) id: MSCKF_ERR_ARG, nothing deleted. */
int msckf_tracks_remove(msckf_ctx* ctx, int32_t n, const int32_t* ids);
/* The effect of msckf_set_features + msckf_set_tracks for the listed tracks in the listed order (the input order of
 * accepted[], flags[] and msckf_get_selection), with the same plan: line_base = the resident position of each view's clone,
 * idp_base = that of the anchor clone or the frozen base; lost_for / tracked_for are the front end's counters.  Asynchronous
 * wherever msckf_set_features is.  MSCKF_ERR_ARG for an unknown or repeated id. */
int msckf_tracks_load(msckf_ctx* ctx, int32_t F, const int32_t* ids, const int32_t* lost_for, const int32_t* tracked_for);
/* One track as it stands on the device (tests, logging; blocking; any output may be NULL): M views, slots[M], uv[2M],
 * dir[3M], conf[M], line_base[3M] and idp_base[3] resolved as msckf_tracks_load would, idp_m[3], idp_rho, anchor_slot
 * (-1 once the anchor is frozen). */
int msckf_tracks_get(msckf_ctx* ctx, int32_t id, int32_t* M, int32_t* slots, double* uv, double* dir, double* conf,
                     double* line_base, double* idp_base, double* idp_m, double* idp_rho, int32_t* anchor_slot);
int msckf_tracks_count(msckf_ctx* ctx, int32_t* n_tracks, int32_t* n_views);
/* The ids of the tracks the last msckf_remove_clones deleted (left without a view): up to `cap` of them into ids;
 * returns how many there were (>= 0). */
int msckf_tracks_dropped(msckf_ctx* ctx, int32_t* ids, int32_t cap);

/* ---- frame intake on the store: test the matches, append, keep the counters ---- *
 * MSCKF.add_camera_measurements :332-438 with the matcher's output as input: the listed (track id, keypoint, score) pairs
 * are tested against every stored view of their track (the tests of msckf_run_associate) with the RESIDENT poses -- the
 * newest clone is slot N - 1, so the call is correct straight behind msckf_augment_imu or msckf_commit_inject --, the
 * pairs that pass are appended as msckf_tracks_observe appends them (the stored bits are equal) and unknown ids create
 * tracks.  result[n]: 0 appended (tracked_for += 1, lost_for = 0, :411-412), 1 / 2 failed the epipolar / homography test
 * (nothing appended, lost_for += 1, :400), 4 created (tracked_for = 1, lost_for = 0); 3 is not used, as the codes are
 * msckf_run_associate's.  fail_view[n] (nullable): the first view that failed, -1.  Every stored track that is not listed
 * gets lost_for += 1 (:438).  Blocking: the store's integer mirror needs the results.  The reference's two early returns
 * (:286 no clone of the IMU's id, :320 no previous descriptors) are the caller's: do not call then.
 * The counters lost_for_n_frames / tracked_for_n_frames live beside the mirror, two ints per track: msckf_tracks_observe
 * counts as an append for the listed tracks and leaves the others alone, msckf_tracks_load neither reads nor writes them,
 * they die with the track, msckf_tracks_reset and msckf_set_state clear them, msckf_remove_clones leaves them alone.
 * Errors, nothing changed: MSCKF_ERR_STATE when N = 0; MSCKF_ERR_DUP_SLOT for an id listed twice or a track that already
 * has a view of the newest clone; MSCKF_ERR_ARG for a negative id, a non-finite keypoint, a singular K, more fresh ids than
 * free rows, or a listed known track that already holds max_track views. */
typedef struct msckf_frame_params {
    double K[9];                    /* intrinsics, row-major (the context only holds K^-1)            */
    double epipolar_threshold;      /* MSCKFParameters.epipolar_rejection_threshold                   */
    double homography_threshold;    /* MSCKFParameters.homography_rejection_threshold                 */
} msckf_frame_params;
int msckf_tracks_frame(msckf_ctx* ctx, const msckf_frame_params* params, int32_t n, const int32_t* ids,
                       const double* uv /*2n*/, const double* score /*n*/, uint8_t* result /*n*/, int32_t* fail_view /*n, nullable*/);
/* msckf_tracks_load with the stored counters for every track (n_slots == 0: process_features' candidates, MSCKF.py:453) or
 * every track with at least one view in one of the listed clone slots (both prune paths, :669-674, :726-731), in the
 * order the tracks were created (the reference's dict order, :461, :670, :727).  *F_out tracks; their ids go to ids_out in
 * that order: the input order of accepted[], flags[] and msckf_get_selection.  No candidate: as msckf_tracks_load(F = 0).
 * MSCKF_ERR_ARG when there are more than `cap` of them (nothing loaded) or a slot is outside [0, N). */
int msckf_tracks_load_where(msckf_ctx* ctx, int32_t n_slots, const int32_t* slots, int32_t* F_out, int32_t* ids_out, int32_t cap);
/* The stored counters of the listed tracks (either output nullable).  An unknown id: MSCKF_ERR_ARG. */
int msckf_tracks_counters(msckf_ctx* ctx, int32_t n, const int32_t* ids, int32_t* lost_for, int32_t* tracked_for);
/* Views per clone slot, views[N]: number_of_features_per_camera of prune_poorest_camera_states (:712-716); a zero is a
 * clone of get_cameras_without_features (:781-790). */
int msckf_tracks_clone_views(msckf_ctx* ctx, int32_t* views /*N*/);

/* ---- frame intake from descriptors: match on the device against the store ---- *
 * A frame travels as (keypoints, descriptors, scores); the store answers with track ids and result codes.  Behind every
 * view the store then keeps its descriptor ([T][V][64] fp32, XFeat's dtype; desc_dim D in 1..64, rows zero-padded), and
 * per track one match row ([T][64] fp32): the reference's last_camera_measurement table (MSCKF.py:436-444).  The row is a
 * SNAPSHOT, recomputed only at the end of an intake as fp32(sum_v fp64(d_v) conf_v / sum_v conf_v) over the track's views
 * in view order (:439); msckf_remove_clones compacts the per-view descriptors (:766) and leaves the row stale until the
 * next intake, as the reference does; on an empty store (:291-311) the row is the raw descriptor, bit for bit (:311).
 * Both arrays are allocated by the first msckf_tracks_match_frame.  The store's D is set by the first successful intake
 * and cleared by msckf_tracks_reset / msckf_set_state.
 * The matching rule (XFeat.match, mutual nearest neighbour): A = the rows of the live tracks in the order the tracks were
 * created, B = the frame; S = A B^T in fp32 (v_mfma_f32_16x16x4_f32; no normalisation), m12[i] = argmax_j S[i][j],
 * m21[j] = argmax_i S[i][j], ties to the lowest index (the earliest-created track); (i, m12[i]) is a match iff
 * m21[m12[i]] == i and S[i][m12[i]] > min_cosine_similarity (strict; compared in double).
 * Errors, nothing changed: MSCKF_ERR_ARG for D outside 1..64 or different from the store's D, a non-finite descriptor, a
 * negative first_new_id or a new id that collides with a live one, more creations than free rows; MSCKF_ERR_STATE when
 * N = 0 or the store holds a track with a view that has no descriptor (tracks fed by msckf_tracks_observe or
 * msckf_tracks_frame are such tracks); otherwise those of msckf_tracks_frame. */
/* Match only, the store is untouched: track_id_out[n] = the matched track's id or -1, sim_out[n] (nullable) = the pair's
 * similarity, 0 where unmatched.  Blocking. */
int msckf_tracks_match(msckf_ctx* ctx, double min_cosine_similarity, int32_t desc_dim, int32_t n, const float* desc /*n*D*/,
                       int32_t* track_id_out /*n*/, float* sim_out /*n, nullable*/);
typedef struct msckf_match_params {
    double K[9];                    /* as msckf_frame_params                                            */
    double epipolar_threshold;
    double homography_threshold;
    double min_cosine_similarity;   /* MSCKFParameters.min_cosine_similarity                            */
    int32_t desc_dim;               /* D                                                                */
    int32_t first_new_id;           /* created tracks get first_new_id, +1, ... in ascending keypoint order */
} msckf_match_params;
/* The else-branch of MSCKF.add_camera_measurements (:315-444): match; the matched pairs go through msckf_tracks_frame's
 * path (codes 0 / 1 / 2, same stored bits, same counters); every unmatched keypoint creates a track (code 4), ids in
 * ascending keypoint order (np.setdiff1d, FeatureExtractor.py:72); lost_for += 1 for every unmatched track (:438); all
 * rows are recomputed.  ids_out[n]: the track each keypoint went to or created.  Returns 1 with NOTHING changed when
 * n == 0 (:286) or no pair matched (:320: no new tracks, no counters, no rows).  On an empty store everything is created
 * and the rows are raw.  Blocking. */
int msckf_tracks_match_frame(msckf_ctx* ctx, const msckf_match_params* params, int32_t n, const float* desc /*n*D*/,
                             const double* uv /*2n*/, const double* score /*n*/, int32_t* ids_out /*n*/, uint8_t* result /*n*/,
                             int32_t* fail_view /*n, nullable*/, float* sim_out /*n, nullable*/);
/* ---- the match's search window and distinctiveness margin (NOT in the reference; off by default) ---- *
 * On repeated texture two tracks with near-equal descriptors break each other's mutuality or pair with each other's
 * keypoints, and everything downstream can only discard the damage a view or a track at a time.  Two options of the
 * context, both off after msckf_create: search_radius (pixels; 0 = off; +inf is legal) and min_margin (0 = off).
 * THE RULE.  A, B, S = A B^T in fp32 as above.  allowed(i, j): the radius is off, or
 * (u_j - u^_i)^2 + (v_j - v^_i)^2 <= radius^2, formed in double, where (u_j, v_j) is keypoint j of the frame and
 * (u^_i, v^_i) the LAST stored keypoint of table track i: view count - 1 of its row as it stands in the store when the
 * match runs (behind an append the appended keypoint; behind msckf_remove_clones the last view that survived).
 * S'[i][j] = S[i][j] where allowed, else -inf.  m12[i] = argmax_j S'[i][.], lowest index among equals, or none when no j
 * is allowed; s1 = that maximum; s2 = the largest S'[i][j] over j != m12[i], -inf when there is none.  The same per
 * column: m21, c1, c2.  Each table element gets a reason code, the first that applies:
 *   1  no keypoint inside the window
 *   2  m21[m12[i]] != i (not mutual)
 *   3  not s1 > min_cosine_similarity (strict; compared in double on the fp32 value, as without the options)
 *   4  the margin is on and not (s1 - s2 > min_margin and c1 - c2 > min_margin), c1 / c2 those of column m12[i];
 *      strict, in double on the fp32 values; a second best of -inf passes
 *   0  the pair (i, m12[i])
 * With radius = +inf and margin 0 the rule is the plain one.  Everything behind the pairs is unchanged: the numbering of
 * the unmatched keypoints, msckf_tracks_frame's path, the counters, the descriptors and rows, and the return of 1 with
 * nothing changed for a frame in which no pair survives.
 * msckf_tracks_set_match_options: NULL turns both off; MSCKF_ERR_ARG, with nothing changed, for a negative or NaN value.
 * The options are STICKY: a setting of the context, which msckf_tracks_reset and msckf_set_state do not clear.  With both
 * off, msckf_tracks_match and msckf_tracks_match_frame launch exactly the kernels and form exactly the bits they did
 * before the options existed; with either on they run k_match_last_uv (window only), k_match_argmax_opt twice and
 * k_match_resolve_opt (k_match.h). */
typedef struct msckf_match_options {
    double search_radius;           /* pixels around the track's last keypoint; 0 = off                 */
    double min_margin;              /* best minus second-best similarity, row and column; 0 = off       */
} msckf_match_options;
int msckf_tracks_set_match_options(msckf_ctx* ctx, const msckf_match_options* options);
/* msckf_tracks_match with the frame's keypoints, uv[2 n]: the match-only probe under the window.  Its checks are those
 * of msckf_tracks_match, and MSCKF_ERR_ARG for a non-finite keypoint.  msckf_tracks_match itself has no keypoints: it
 * answers MSCKF_ERR_STATE while a radius is on; with a margin only, it applies the margin. */
int msckf_tracks_match_at(msckf_ctx* ctx, double min_cosine_similarity, int32_t desc_dim, int32_t n, const float* desc /*n*D*/,
                          const double* uv /*2n*/, int32_t* track_id_out /*n*/, float* sim_out /*n, nullable*/);
/* The table of the last call that ran a match (msckf_tracks_match, _match_at, _match_frame with n > 0 on a store that
 * holds tracks), in creation order: *T_out elements; the track id and the reason code of the first min(*T_out, cap) of
 * them (ids_out, why_out: nullable when that is 0).  Without the options the codes are 0 / 2 / 3, derived on the host.
 * Empty behind msckf_tracks_reset and msckf_set_state.  Blocking. */
int msckf_tracks_match_report(msckf_ctx* ctx, int32_t* T_out, int32_t* ids_out, uint8_t* why_out, int32_t cap);
/* One track's descriptors as they stand on the device (blocking; any output may be NULL): its match row, row[D], its M
 * views and their descriptors, views[M*D] (room for max_track * D).  MSCKF_ERR_ARG: unknown id; MSCKF_ERR_STATE: the
 * track has a view without a descriptor. */
int msckf_tracks_descriptor(msckf_ctx* ctx, int32_t id, float* row /*D*/, int32_t* M, float* views /*M*D*/);

/* ---- feature-sharded path (one context per GPU / rank) ------------------ *
 * Each rank holds a shard of the features and the full state.  It runs K1-K5
 * locally and exports its compressed block [R | Q^T r]: (6N) x (6N+1) doubles,
 * upper triangular, row-major.  After the blocks are gathered on the root
 * (RCCL gather, done by the host), the root merges them (QR of the stacked
 * triangles) and runs K6-K7.  `device_ptr` != 0 means the buffer is HBM. */
int msckf_run_compress(msckf_ctx* ctx);                 /* K1-K5 on the local shard, async */
size_t msckf_block_doubles(const msckf_ctx* ctx);       /* 6N * (6N + 1)                   */
int msckf_export_block(msckf_ctx* ctx, void* dst, int device_ptr, int32_t* n_accepted);
int msckf_run_merge_gain(msckf_ctx* ctx, const void* blocks, int32_t n_blocks, int device_ptr,
                         int32_t total_accepted /* sum of the shards' n_accepted */);

/* Group exchange (the 60-column band pipeline: every track spans <= 10 slots and N <= 37, msckf_band_rule): instead of its root block a
 * rank exports the triangles of its first-slot groups, one record of N flags, its accepted count and N slots
 * of 60 x 61 doubles (the triangle of group s covers the fixed window of min(10, N - s) slots).  The rank then stops in front
 * of its root sweep (msckf_run_compress) and the root folds, per group, the triangles of all shards and
 * runs ONE root sweep and K6-K7 -- a constant number of steps instead of log2(G) dense merges.
 * msckf_set_group_exchange must precede msckf_set_features; msckf_export_groups returns MSCKF_ERR_STATE
 * when the batch was planned as a merge tree (then use msckf_export_block / msckf_run_merge_gain). */
int msckf_set_group_exchange(msckf_ctx* ctx, int on);
/* The longest track of the WHOLE batch in clone slots (last slot - first slot + 1 over every shard; 0 = not told).
 * With it every shard lays its record out for the sweep mode of the whole batch (msckf_band_rule), whatever its own
 * tracks look like, and the group exchange also covers the ring-buffered modes: N > 37 clones (60-column slots) and
 * tracks of 11 - 15 slots (90-column slots, BASELINE.json configs[4]: N = 50, track 15).  Without it only the
 * 60-column k_sweep form (every track <= 10 slots, N <= 37) is exchanged as group records.  Same value on every
 * rank; call before msckf_set_features. */
int msckf_set_exchange_span(msckf_ctx* ctx, int32_t max_span);
/* The planner's rule, for callers that must agree on the exchange format BEFORE sharding a batch: > 0 when a
 * batch of tracks spanning at most `max_span` clone slots over N clones is planned as the band pipeline on
 * this context (1 k_sweep, 2 k_wsweep<4> with the band in a ring, 3 k_wsweep<6> with 90-column tiles; group
 * records work for all three once msckf_set_exchange_span told the span), 0 when it gets the merge tree
 * (MSCKF_FLAG_TREE_PLAN, tracks wider than 15 slots): then use msckf_export_block.
 * NB (changed in round 3, same ABI version): the value is the sweep mode + 1, not a boolean -- test `> 0`, never
 * `== 1` (a caller that did fell back to root blocks for the two ring modes). */
int msckf_band_rule(const msckf_ctx* ctx, int32_t N, int32_t max_span);
size_t msckf_group_record_doubles(const msckf_ctx* ctx);   /* N + 1 + gate-byte doubles (msckf_set_exchange_mask) + N * 3660 (8190 with 90-column slots)
                                                            + 1 + rows x (6N + 1) with msckf_set_exchange_split */
int msckf_export_groups(msckf_ctx* ctx, void* dst, int device_ptr, int32_t* n_accepted /* nullable */);

/* Split records: long tracks (more than 10 clone slots) split under the group exchange as on one GPU.
 * msckf_exchange_split_rule evaluates the WHOLE batch (every rank passes the same arguments and gets the same answer,
 * no collective): out[0] 1 when the batch is exchanged as split records, out[1] the band span after the split (what
 * msckf_set_exchange_span must be told; the longest track when not split), out[2] the remainder rows one record holds
 * (the largest shard's sum of 3 per view group of its long tracks, rounded up to 16), out[3] the whole batch's bound
 * on them.  `flags` (nullable, n_shards x N bytes) receives the first-slot groups of every shard's record (narrow
 * blocks start at their view group's first slot) for msckf_run_merge_groups_flags.  ctx may be null (defaults).
 * Not split: a long track with views out of slot order, more than 31 views or more than 6 groups, a batch mostly of
 * 11 - 15-slot tracks, more remainder rows than K6-K7 takes as they are. */
int msckf_exchange_split_rule(const msckf_ctx* ctx, int32_t N, int32_t F, const int32_t* view_ptr, const int32_t* obs_slot,
                              int32_t n_shards, const int32_t* bounds /* [n_shards + 1] */, int32_t out[4], uint8_t* flags);
/* Record capacity for split records (out[2] and out[3] of the rule; 0 = off, today's records): msckf_set_features splits
 * long tracks with the group exchange on, the record grows by a remainder section [count word | rows x (6N + 1)]
 * (msckf_group_record_doubles), rank 0's merge takes those rows as K6-K7's second source.  Same values on every rank;
 * call before msckf_set_features. */
int msckf_set_exchange_split(msckf_ctx* ctx, int32_t rows_per_record, int32_t rows_total);
int msckf_run_merge_groups(msckf_ctx* ctx, const void* records, int32_t n_records, int device_ptr,
                           int32_t total_accepted /* < 0: the sum of the counts in the records */);

/* Variant of msckf_run_merge_groups without any device-to-host traffic: `flags` (n_records x N bytes, host,
 * nullable) says which first-slot groups each record carries -- every rank sees the whole batch, so the host
 * side knows it (shard.py computes it from the partition) -- and the shards' accepted counts are summed on the
 * device (msckf_get_result reads the sum with the results).  flags == NULL reads the record heads back like
 * msckf_run_merge_groups. */
int msckf_run_merge_groups_flags(msckf_ctx* ctx, const void* records, int32_t n_records, int device_ptr,
                                 const uint8_t* flags);

/* The gate results of a sharded update (the boundary's accepted[F] and the reference counter
 * number_of_residuals_discarded_for_gasting_test, MSCKF.py:578) ride with the exchange instead of a collective of
 * their own.  `bounds` (n_shards + 1 ints, host, bounds[0] = 0): shard r holds the features [bounds[r], bounds[r+1])
 * of the whole batch in input order; the same on every rank.  From then on (call it before msckf_set_features)
 *   - a shard's group record carries its gate bytes behind the accepted count (ceil(max shard size / 8) doubles),
 *   - the merging rank (msckf_run_merge_groups[_flags] with n_records = n_shards) lays the gate bytes of the whole
 *     batch behind P_out, so that status (64 B: Cholesky status words, total accepted, F_total) | dx | P_out | gate
 *     bytes is ONE contiguous HBM range of msckf_result_range_doubles() doubles at msckf_device_pointer(ctx, 5):
 *     one broadcast hands every rank the complete result,
 *   - msckf_get_shared_result reads that range on ANY rank (after the broadcast) and derives the same return code
 *     on all of them (0 / 1 no-op / MSCKF_ERR_NOT_SPD): accepted[F_total] in input order of the whole batch,
 *     stats->n_accepted / n_rejected / not_spd filled.
 * n_shards = 0 switches it off.  With the root-block fallback exchange (msckf_run_merge_gain) the caller places
 * the gate bytes at msckf_device_pointer(ctx, 6) itself (shard.py does). */
int msckf_set_exchange_mask(msckf_ctx* ctx, int32_t n_shards, const int32_t* bounds);
size_t msckf_result_range_doubles(const msckf_ctx* ctx);
int msckf_get_shared_result(msckf_ctx* ctx, double* dx, double* P_out, uint8_t* accepted, msckf_stats* stats);

/* ---- RCCL exchange behind the C-ABI (one context = one rank = one GPU; no PyTorch on the data path) ---- *
 * The one exchange of the sharded update (gather of the compressed blocks to rank 0,
 * broadcast of dx | P+ back) on librccl, loaded with dlopen at the first call (a single-GPU process never
 * loads it).  Bootstrap: rank 0 calls msckf_comm_unique_id and hands the 128 bytes to the other ranks by any
 * side channel (shard.py uses a file); every rank then calls msckf_comm_init.  All collectives are enqueued on
 * the context's stream, behind the kernels that produce their operands; buffers are HBM addresses. */
#define MSCKF_COMM_ID_BYTES 128
#define MSCKF_ERR_COMM (-7)         /* RCCL failure (msckf_last_error has the text)                      */
int msckf_comm_unique_id(void* id_out /* MSCKF_COMM_ID_BYTES */);
int msckf_comm_init(msckf_ctx* ctx, int32_t rank, int32_t world, const void* id);   /* (ctx, rank, world, id) */
int msckf_comm_destroy(msckf_ctx* ctx);
/* rank `root` receives world x count doubles (rank r's at recv + r * count); recv is ignored elsewhere. */
int msckf_comm_gather(msckf_ctx* ctx, const void* send, void* recv, size_t count, int32_t root);
int msckf_comm_broadcast(msckf_ctx* ctx, void* buf, size_t count, int32_t root);
/* In-place all-reduce of `count` doubles; op 0 = sum, 1 = max. */
int msckf_comm_allreduce(msckf_ctx* ctx, void* buf, size_t count, int32_t op);
/* An HBM scratch buffer owned by the context (grown on demand, contents undefined): receive side of the gather. */
void* msckf_comm_buffer(msckf_ctx* ctx, size_t bytes);
/* Blocking copies between host memory and an HBM address, ordered on the context's stream (staging of the
 * root-block fallback exchange; the group exchange needs neither). */
int msckf_comm_put(msckf_ctx* ctx, void* dst_device, const void* src_host, size_t bytes);
int msckf_comm_get(msckf_ctx* ctx, void* dst_host, const void* src_device, size_t bytes);

/* Copy dx[d] and P_out[d*d] of the last run into caller buffers that may live in HBM
 * (device_ptr != 0), e.g. the send buffer of the broadcast that follows the merge. */
int msckf_export_result(msckf_ctx* ctx, void* dx_dst, void* P_dst, int device_ptr);
/* Replace the prior covariance P (d*d) from a host or HBM buffer (non-root ranks after
 * the broadcast; also the hand-over point for a device-resident propagation step). */
int msckf_import_covariance(msckf_ctx* ctx, const void* P, int device_ptr);

/* ---- introspection for tests (device intermediates, host copies) -------- */
/* gamma[F] (gate statistic), qdim[F] (dof = projected rows), in input order. */
int msckf_debug_gate(msckf_ctx* ctx, double* gamma, int32_t* qdim);
/* The gate's verdict per track as k_feature wrote it, input order: 1 accepted, 0 rejected by the chi-square test, 2 gate
 * matrix not SPD (msckf_stats.not_spd), 3 not selected by msckf_run_select -- msckf_get_result's accepted[] folds 0 / 2 / 3
 * into 0.  n_blocks (nullable): the narrow and remainder blocks of the batch's split long tracks; block_codes / block_track
 * (nullable, n_blocks entries each): the byte every block inherited and the input index of its track. */
int msckf_debug_gate_codes(msckf_ctx* ctx, uint8_t* codes, int32_t* n_blocks, uint8_t* block_codes, int32_t* block_track);
/* Final compressed system: T (6N x 6N, upper triangular) and r_n (6N). */
int msckf_debug_compressed(msckf_ctx* ctx, double* T, double* rn);
/* Diagnostics: out == NULL enables per-node cycle stamps in the fold kernel; otherwise copies
 * 8 int64 per tree node {setup, staging, steps, total (100 MHz ticks), w, rows, -, -}. */
int msckf_debug_fold_stamps(msckf_ctx* ctx, long long* out, int32_t max_nodes);
/* Average device time of the selection (HIP events, `iters` re-launches of the last msckf_run_select -- the selection
 * kernel and, with refine_iters > 0, the refinement behind it; both are idempotent). */
int msckf_debug_time_select(msckf_ctx* ctx, int32_t iters, float* us_per_launch);
/* How the current batch's long tracks (more than 10 clone slots) were planned: out[0] long tracks that were split
 * (two-level nullspace basis), out[1] their narrow blocks, out[2] rows their remainder blocks may hold,
 * out[3] what K6-K7 does with those rows under the CURRENT plan: 0 nothing apart (no long track, or one plan for every
 * block), 1 takes them as they are (dense second source), 2 takes the root of their own merge tree in a second launch;
 * out[4] levels of that tree, out[5] entries of the sorted arrays (tracks + blocks), out[6] 1: band plan, out[7] sweep mode. */
int msckf_debug_split(msckf_ctx* ctx, int32_t out[8]);
/* Tests: remainder rows up to which K6-K7 takes them as they are (default 3840; < 0 restores it).  Applies to the
 * batches loaded afterwards. */
int msckf_debug_set_rem_direct_rows(msckf_ctx* ctx, int32_t rows);
/* Raw device pointers (as integers) for zero-copy interop: which = 0 dx (dx[d] | P_out[d*d] are contiguous for the
 * CURRENT d = 15 + 6 N: the range is re-seated whenever N changes), 1 P_out, 2 root block [T | r_n], 3 the shard's
 * group record (msckf_set_group_exchange), 4 the prior covariance P, 5 the result range (status 64 B | dx | P_out |
 * gate bytes, msckf_set_exchange_mask), 6 its gate bytes. */
uint64_t msckf_device_pointer(msckf_ctx* ctx, int which);
void* msckf_stream(msckf_ctx* ctx);                     /* hipStream_t of the context */

#ifdef __cplusplus
}
#endif
#endif /* MSCKF_MI355X_H */
