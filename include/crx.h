/*
 * crx.h -- C ABI of libcrx, the MI355X-native batched optimal-control solver behind
 * HybridRobotics/car-racing's planner / MPC-CBF hot path.
 *
 * The reference has NO native boundary for this path: the boundary is three Python call sites
 * that build a CasADi `Opti` problem and hand it to IPOPT.  Each entry point below replaces one
 * of them (file:line into /root/reference/car_racing); INTEGRATION.md shows the ctypes stub a
 * reference maintainer would add at exactly those lines.
 *
 *   crx_planner_solve      <- planning/overtake_traj_planner.py:248-379  generate_traj_per_region
 *                             (Opti build :263-334, opti.solve() :359-364, fallback :365-374),
 *                             batched over what the reference forks one process per region for
 *                             (:182-197)
 *   crx_select             <- planning/overtake_traj_planner.py:205-246  region selection
 *   crx_planner_plan       <- planning/overtake_traj_planner.py:162-246  solve_optimization_problem
 *                             (= crx_planner_solve over all regions + crx_select, one launch chain)
 *   crx_cbf_solve          <- control/control.py:476-607 mpccbf  and  control/control.py:251-473
 *                             mpc_multi_agents  (same NLP family; the latter with a per-stage target)
 *
 * Conventions
 *   - plain C, no torch / HIP types in any signature; all arrays C-contiguous, float64 / int32.
 *   - `*_dev` variants take DEVICE pointers (e.g. torch tensor .data_ptr()) and a stream handle
 *     (hipStream_t passed as void*, NULL = default stream); they enqueue work and return without
 *     synchronising.  The non-`_dev` variants take HOST pointers, stage through library-owned
 *     device buffers and block until the result is back.
 *   - the caller owns every buffer; the library never keeps a pointer after a call returns.
 *   - return value: 0 on success, negative crx_err on a CALL failure (bad argument, no device,
 *     HIP error; text via crx_last_error()).  A problem that does not converge is NOT a call
 *     failure: it is reported per problem in status[] (crx_status), with X/U holding the last
 *     iterate (mpccbf / mpc_multi_agents consume the last iterate, control.py:600-603,458-469) or
 *     the reference's synthetic fall-back trajectory (planner, overtake_traj_planner.py:365-374).
 *   - not fork-safe (a HIP context does not survive fork()); callers must replace the reference's
 *     Process fan-out (:182-197) with ONE batched call from the parent.
 *
 * State order  x = [vx, vy, wz, epsi, s, ey]   (utils/constants.py:1, control/lmpc_helper.py:133-138)
 * Input order  u = [delta, a]                  (system/vehicle_dynamics.py:10-11)
 */
#ifndef CRX_H
#define CRX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRX_VERSION 400 /* 0.4.0 (additive, same number): crx_field_prep_tracks, crx_field_prep_tracks_dev, crx_mixed_prep_tracks, crx_mixed_prep_tracks_dev,
                          crx_race_stats_laps_dev (field races and mixed fields on one track per race) -- new entry points only.
                          0.4.0 (additive, same number): crx_plant_step_tracks, crx_plant_step_tracks_dev, crx_plant_step_tracks_plain_dev,
                          crx_cbf_prep_laps_dev and CRX_MAX_TRACKS (one track per vehicle: a track set in the plant, one lap length per race in the
                          MPC-CBF prep) -- new entry points only.
                          0.4.0 (additive, same number): crx_mixed_desc, crx_mixed_desc_default, crx_mixed_prep, crx_mixed_prep_dev, crx_mixed_commit_dev and
                          CRX_POLICY_* (mixed fields: every car of a race under its own controller) -- new entry points only.
                          0.4.0 (additive, same number): crx_field_traffic, crx_field_traffic_dev (field games: the racing game's traffic arrays when every car of
                          a race plays it) -- new entry points only.
                          0.4.0 (additive, same number): crx_seed_commit_dev, crx_seed_log_dev and CRX_SEED_* (seed laps: every car's own PID lap and
                          MPC-LTI lap become its own safe set) -- new entry points only.
                          0.4.0 (additive, same number): crx_stats_desc, crx_stats_desc_default, crx_race_stats_reset, crx_race_stats_reset_dev,
                          crx_race_stats, crx_race_stats_dev, crx_race_stats_summary, crx_race_stats_summary_dev and the CRX_STATS_* layout
                          (per-car race statistics of every closed loop) -- new entry points only.
                          0.4.0 (additive, same number): crx_field_desc, crx_field_desc_default, crx_field_prep, crx_field_prep_dev (field races: every
                          car of a race drives itself) -- new entry points only.
                          0.4.0 (additive, same number): crx_plant_step_params, crx_plant_step_params_dev, crx_plant_step_params_plain_dev and
                          CRX_PLANT_NPARAM (one BicycleDynamicsParam set per vehicle) -- new entry points only.
                          0.4.0 (additive, same number): crx_planner_models_reach_dev, crx_planner_solve_models, crx_planner_solve_models_dev,
                          crx_planner_plan_models, crx_planner_plan_models_dev, CRX_PLANNER_MODEL_REACH_DOUBLES -- new entry points only.
                          0.4.0 (additive, same number): crx_cbf_models_reach_dev, crx_cbf_solve_models, crx_cbf_solve_models_dev,
                          CRX_CBF_MODEL_REACH_DOUBLES; CRX_SINGULAR also from these -- new entry points only.
                          0.4.0 (additive, same number): crx_lqr_desc, crx_lqr_desc_default, crx_lqr_design, crx_lqr_design_dev, crx_lqr_step_dev,
                          crx_ilqr_solve_models, crx_ilqr_solve_models_dev; CRX_SINGULAR also from crx_lqr_design -- new entry points only.
                          0.4.0 (additive, same number): crx_sysid_desc, crx_sysid_desc_default, crx_sysid_fit, crx_sysid_fit_dev,
                          crx_sysid_workspace_bytes, crx_pid_log_dev and status CRX_SINGULAR -- new entry points only.
                          0.4.0 (additive, same number): crx_ilqr_desc, crx_ilqr_desc_default, crx_ilqr_solve, crx_ilqr_solve_dev and
                          CRX_ILQR_MAX_N -- new entry points only, every earlier signature and struct layout unchanged.
                          0.4.0: NOT layout-compatible with 0.3.x -- crx_ipm_opts grew by IPOPT's three UNSCALED termination tolerances
                          (`dual_inf_tol`, `constr_viol_tol`, `compl_inf_tol`: "converged" now means IPOPT's complete test, not the scaled error
                          alone) and by `stall_iters` (the stall rule's budget, a kernel constant until 0.3.x; crx_cbf_desc_default picks it and
                          `restore_iters` by problem class).
                          0.3.0: crx_allgather_winners_dev takes the winners' status and the winner record is SURVEY 8e's {int32 flag; int32
                          status; double X[N+1][6]} (same 632 B at N = 12; 0.2.x: the flag as a double, no status) -- the only signature that
                          changed; every other entry point and every struct layout is 0.2.x's.
                          0.2.1: same ABI as 0.2.0; the crash path of the MPC-CBF NLPs (crx_ipm_opts.slack_start = 2) takes the crash start's barrier
                          parameter from its complementarity and keeps the convexified inertia retry between probes -- other iterates, same end
                          points or other KKT points on crash states; every problem off the crash path is bit-identical to 0.2.0.
                          0.2.0: NOT layout-compatible with 0.1.x -- crx_ipm_opts grew by `reach_screen` and `slack_start` (every descriptor
                          embeds it), the process-global switches crx_set_reach_screen / crx_set_cbf_slack_start / crx_set_timing /
                          crx_last_kernel_ms are gone (options travel in the descriptor, timing is an object: crx_timer_*), new status
                          CRX_STALLED (what CRX_INFEASIBLE used to report without a proof), CRX_MAX_OBS 3 -> 6 (CRX_MAX_VEH = 3 for the planner side).
                          (0.1.3: per-obstacle dimensions, plant noise, crx_game_*, crx_comm_* (RCCL), dispatch order, crx_streams_*;
                           0.1.2: infeasibility certificates, *_masked_dev, CRX_SKIPPED, crx_track_prep_dev;
                           0.1.1: restoration phase, CRX_RESTORED, crx_ipm_opts.restore_iters) */
#define CRX_NX 6
#define CRX_NU 2
#define CRX_MAX_N 24       /* horizon limit (reference runs N=10/12; BASELINE configs go to 20) */
#define CRX_MAX_OBS 6      /* obstacles per MPC-CBF NLP (n_obs_max of crx_cbf_desc).  The reference admits any number (control.py:524-562
                              loops over every vehicle in the window); its scenarios race 3 cars (overtake_planner_test.py).  Up to 3 run on
                              the tuned instantiations, 4..6 on ONE generic instantiation per horizon class (correct, slow: twice the
                              register file).  A caller with more keeps the nearest (crx.hostprep.pack_obstacles warns). */
#define CRX_MAX_VEH 6      /* vehicles of interest per planner scenario (n_veh_max of the scene / prep / select descriptors); regions = + 1.  The
                              reference plans around every vehicle get_overtake_flag returns (overtake_traj_planner.py:62-92); its scenarios race
                              3 cars.  [0.3.0: 3 -> 6, = CRX_MAX_OBS: the tracking NLP behind the planner takes the same vehicles as obstacles.]
                              A scene with more keeps the nearest (crx_scene reports `overflow`). */
#define CRX_MAX_REGIONS (CRX_MAX_VEH + 1)
#define CRX_LMPC_MAX_N 16 /* horizon limit of crx_lmpc_solve (its dense factors share one LDS slice) */
#define CRX_MAX_SS 60      /* safe-set points per learning-MPC QP (reference: 44) */
#define CRX_ILQR_MAX_N 64  /* horizon limit of crx_ilqr_solve (one stage per lane in the derivative phase; reference: 50) */

typedef enum crx_err {
    CRX_OK = 0,
    CRX_ERR_ARG = -1,      /* NULL pointer, N out of range, batch < 0, ... */
    CRX_ERR_NO_DEVICE = -2,
    CRX_ERR_HIP = -3,
    CRX_ERR_NOT_INIT = -4
} crx_err;

typedef enum crx_status {
    CRX_CONVERGED = 0,     /* KKT error <= tol */
    CRX_MAX_ITER = 1,      /* iteration cap, or the line search failed at a point that satisfies the constraints; last iterate returned */
    CRX_INFEASIBLE = 2,    /* PROVED infeasible: a bound already violated by the fixed x0 (quirk Q9 / the planner's ey_0 rows), the
                              reachability screen, or the Farkas certificate over the input box (problems whose rows are all linear:
                              planner QPs, 0-obstacle NLPs, first attempts of the learning-MPC QP).  Never a heuristic. */
    CRX_RESTORED = 3,      /* MPC-CBF NLPs only: the solve went through its crash path (restart from a feasible interior point, or
                              the closed-form slack restoration) and used up opts.restore_iters further iterations without
                              converging.  The returned iterate satisfies every CBF row through its slacks sigma but is not optimal. */
    CRX_SKIPPED = 4,       /* *_masked_dev launches only: active[b] == 0, the problem was left alone (outputs untouched) */
    CRX_STALLED = 5,       /* gave up WITHOUT a proof at a point that still violates its constraints: no acceptable step (IPOPT:
                              "restoration failed" / "converged to a point of local infeasibility"), or multipliers past 1e12 (IPOPT's
                              divergence heuristic).  libcrx <= 0.1.3 reported these as CRX_INFEASIBLE.  Like every status != 0 it
                              selects the reference's "solver failed" branch (control.py:600-603: keep the last iterate;
                              overtake_traj_planner.py:365-374: the fall-back trajectory). */
    CRX_SINGULAR = 6,      /* crx_sysid_fit: a zero or non-finite pivot in the LU of X'X + lamb I, where numpy.linalg.inv raises
                              LinAlgError; W, A, B and err are NaN.  crx_lqr_design: a non-finite model, iterate or gain, or a zero or
                              non-finite determinant of R + B'PB; K and P are NaN */
    CRX_OUT_OF_DOMAIN = 7  /* crx_path_plan (plan_status only): the scenario cannot be planned from its data -- a look-up falls above the
                              optimal-trajectory table, where the reference raises (interp1d bounds_error: the Bezier end point, quirk P2,
                              or the target speed, quirk P8), or an input it reads is not finite.  flag -1, target NaN */
} crx_status;

/* Interior-point options.  Defaults (crx_ipm_opts_default) restate IPOPT 3.x defaults that the
 * reference inherits by passing only print options (control.py:593, overtake_traj_planner.py:335). */
typedef struct crx_ipm_opts {
    double tol;            /* 1e-8  convergence tolerance on the scaled KKT error (IPOPT `tol`); since 0.4.0 necessary, not sufficient: see
                              dual_inf_tol / constr_viol_tol / compl_inf_tol at the end of this struct */
    int32_t max_iter;      /* 200   (IPOPT: 3000; capped, status CRX_MAX_ITER beyond) */
    int32_t restore_iters; /* 50 / 25  (by problem class: see stall_iters below) iterations allowed after the first restoration (CRX_RESTORED beyond); < 0: no restoration
                              phase at all (a failed line search then ends the solve, as in libcrx 0.1.0) */
    double mu_init;        /* 0.1   */
    double kappa_eps;      /* 10    barrier sub-problem tolerance factor */
    double kappa_mu;       /* 0.2   linear decrease factor */
    double theta_mu;       /* 1.5   superlinear decrease power */
    double tau_min;        /* 0.99  fraction-to-the-boundary */
    double slack_push;     /* 1e-2  initial slack floor (bound_push) */
    double grad_scale_max; /* 100   gradient-based row scaling target (nlp_scaling_max_gradient) */
    int32_t reach_screen;  /* 1     reachability screens (0 = off: every problem goes through the interior-point iteration).
                              Planner QPs: the inputs are boxed, so ey_j cannot leave [free response -+ reach_j], reach_j =
                              sum_{m<j} |e_ey' A^m B| (delta_max, a_max)'; a region whose ey bound at some stage lies outside that
                              interval by more than 1e-6 has no feasible trajectory -- a proof, independent of the other rows -- and
                              is answered before the iteration is set up: CRX_INFEASIBLE, iters 0, kkt +inf, X = the reference's
                              fall-back trajectory, cost +inf.  Learning-MPC QP: the same for the first attempt's terminal set
                              (x_N = SS lambd needs component c of x_N inside [min_j SS_cj, max_j SS_cj]); the attempt is skipped,
                              the relaxed second attempt runs as it would have. */
    int32_t slack_start;   /* 2     start of the MPC-CBF NLPs whose slacks cannot stay at zero (crash states: the ego inside, or about to
                              enter, an obstacle's safety set; 3..8 % of the BASELINE draws).  The reference passes no initial guess
                              (control.py:593-599), IPOPT starts at u = 0, sigma = 0 and would enter its restoration phase.
                              0: that start only; a solve that stalls is restored in closed form (slacks raised at the current
                                 inputs) -- libcrx 0.1.x behaviour;
                              1: the slacks start at provable lower bounds of their optimal values (0.1.3's optional switch);
                              2: CRASH PATH (default).  (i) A problem whose slacks are PROVABLY positive at every admissible input
                                 (reach of (s, ey) under the boxed inputs) does not start at zero: the best of a 5 x 5 grid of constant
                                 input pairs by f(u) + w sum sigma(u), sigma(u) = the minimal slack cascade for that u, with that
                                 cascade pushed strictly inside -- a feasible interior point; its barrier parameter starts at a tenth of
                                 the point's mean complementarity (not below mu_init), not at mu_init.  (ii) A solve that started at zero and
                                 stalls on violated CBF rows (no acceptable step, jam, 100 iterations still infeasible) restarts ONCE
                                 from such a point instead of being abandoned.  (iii) On the crash path a reduced Hessian of the wrong
                                 inertia is first retried WITHOUT the reverse-convex part of the CBF curvature (positive definite by
                                 construction) before IPOPT's delta_w schedule; after an iteration that needed that, the next ones start
                                 without it and every 4th of such a run tries the exact Hessian first again.  Problems that never enter the crash path are untouched,
                                 bit for bit.  BASELINE configs[1]: 95.7 -> 100 % of the 256 NLPs converge, longest solve 58 -> 38
                                 iterations; configs[3]: 92.5 -> 98.9 % (oracle). 
                              3: EAGER crash path (0.2.1).  As 2, but EVERY problem whose zero start violates a CBF row starts from the point, not
                                 only the provable crash states (the restart of 2 then never fires).  Faster -- BASELINE configs[1]: longest
                                 solve 36 -> 30 iterations, 0.47 -> 0.39 ms per 256 NLPs; configs[3]: 99.2 -> 99.5 % converged -- and further from the
                                 reference: a near-miss that the zero start solves ends at the local minimum IPOPT reaches from zero, and at
                                 another one from the candidate point; the reference's recorded closed loop is reproduced step by step with 2,
                                 not with 3. */
    /* [0.4.0] IPOPT's complete termination test.  IPOPT accepts a point only if the scaled error is <= tol AND three UNSCALED
     * quantities are below their own tolerances (IpOptErrorConvCheck.cpp; the reference runs IPOPT on defaults, control.py:593,
     * overtake_traj_planner.py:335).  "Unscaled" = without the s_d / s_c normalisation of the error measure and with the
     * gradient-based row scaling of the CBF rows undone (rows in the reference's units).  Until 0.3.x libcrx stopped on the scaled
     * error alone: a crash state with multipliers of 1e7..1e9 (s_d of 1e4..1e7) was reported converged with a complementarity of
     * 2.5e-4 (configs[1]) / 5.5e-4 (configs[3]) -- beyond the 1e-4 IPOPT (and north_star) allow. */
    double dual_inf_tol;    /* 1     max |reduced Lagrangian gradient|, unscaled                (IPOPT dual_inf_tol) */
    double constr_viol_tol; /* 1e-4  max |c_j - t_j| with the row scaling undone               (IPOPT constr_viol_tol) */
    double compl_inf_tol;   /* 1e-4  max t_j nu_j                                              (IPOPT compl_inf_tol) */
    int32_t stall_iters;    /* 100 / 50  MPC-CBF NLPs: a solve that started at the reference's zero point and is still infeasible (by 1e-6)
                              after this many iterations is sent to the crash restart / the closed-form restoration.  A
                              kernel constant until 0.3.x (50 in 0.1..0.2, 100 in 0.3).  crx_ipm_opts_default: 100; crx_cbf_desc_default
                              chooses (stall_iters, restore_iters) by problem class: (50, 25) for N <= 12 with at most one obstacle slot --
                              the class of BASELINE configs[1], where a healthy solve is done after 30 iterations --, (100, 50) for every
                              longer horizon or more obstacles (configs[3]: healthy solves of 53..86 iterations).  With the defaults a
                              solve ends after at most stall_iters + 1 + restore_iters (76 / 151) iterations when it went through a
                              restoration, 1 + 3 restore_iters (76 / 151) when it started on the crash path: below max_iter in both. */
    int32_t qp_method;      /* 0     [0.4.0] the solver-kernel problems whose rows are all linear and whose cost is a convex quadratic -- planner region QPs, MPC-CBF
                              NLPs without an obstacle slot -- have ONE solution, so the path to it is free:
                              0: Mehrotra's predictor-corrector (one factorisation and two solves per iteration, no line search): 6.5 iterations
                                 per region QP instead of 10.3, BASELINE configs[2] 0.285 -> 0.247 ms per 4096 QPs;
                              1: IPOPT's monotone barrier + filter line search, as libcrx <= 0.3 ran them (A/B runs).
                              Same starting point, same termination test, same infeasibility proofs either way.  Problems with CBF rows ignore it; so do
                              the learning-MPC QP and the path planner's QPs (measured on the oracle: 15.5 -> 11.5 iterations against a second solve of
                              a third of an iteration -- no gain). */
} crx_ipm_opts;

/* ---- planner region QP (overtake_traj_planner.py:263-334) ------------------------------------ */
typedef struct crx_planner_desc {
    int32_t N;             /* num_horizon_planner (utils/base.py:391) */
    int32_t reserved0;
    double A[36];          /* row-major 6x6, racing_game_param.matrix_A (:272) */
    double B[12];          /* row-major 6x2, racing_game_param.matrix_B (:273) */
    double w_ref;          /* 20   weight on (ey-ey_bez)^2 and (s-s_ref)^2          (:333-334) */
    double w_dey;          /* 30   weight on (ey_k-ey_{k-1})^2, k=2..N-1            (:325-327) */
    double w_prog;         /* 200  weight on -(s_N - s_0)                           (:328) */
    double vx_max;         /* 5.0  vx_{k+1} <= vx_max                               (:276) */
    double delta_max;      /* 0.5                                                   (:280-281) */
    double a_max;          /* 1.5                                                   (:283-284) */
    double dt_ref;         /* 0.1  literal time step in s_ref and the window test   (:296,:330) */
    double fallback_gain;  /* 1.1  speed factor of the fall-back trajectory         (:367-368) */
    crx_ipm_opts opts;
} crx_planner_desc;

/* ---- MPC-CBF NLP (control.py:492-591 / :270-382) --------------------------------------------- */
typedef struct crx_cbf_desc {
    int32_t N;             /* num_horizon (utils/base.py:281) / num_horizon_ctrl (:390) */
    int32_t n_obs_max;     /* leading dimension of the obstacle arrays, <= CRX_MAX_OBS */
    int32_t per_stage_target; /* 0: xt is [batch][6] (mpccbf); 1: xt is [batch][N+1][6] (mpc_multi_agents :373-382) */
    int32_t degree;        /* 6 (control.py:528 / :312); accepted: 2, 4, 6, 8 */
    double A[36];
    double B[12];
    double Q[6];           /* diag(matrix_Q)  (utils/base.py:277 / :384) */
    double R[2];           /* diag(matrix_R)  (utils/base.py:278 / :385) */
    double delta_max;      /* system_param.delta_max (utils/base.py:709) */
    double a_max;
    double v_min;
    double v_max;
    double ey_max;         /* track.width (control.py:585-586) */
    double alpha;          /* 0.8 mpc_cbf_param.alpha / 0.6 literal (control.py:285) */
    double margin;         /* 0.2 (control.py:527) / 0.15 (:311) */
    double l_sum;          /* l_agent + l_obs (control.py:532-535) = 0.4; per-obstacle values: crx_cbf_solve_dims */
    double w_sum;          /* w_agent + w_obs = 0.2 */
    double w_slack;        /* 1e4 (control.py:560,562) */
    crx_ipm_opts opts;
} crx_cbf_desc;

/* ---- learning-MPC QP (control.py:610-730) ------------------------------------------------------ */
typedef struct crx_lmpc_desc {
    int32_t N;             /* lmpc_param.num_horizon (utils/base.py:359), 12 */
    int32_t n_ss_max;      /* leading dimension of ss / qfun / lambda (num_ss_points, utils/base.py:357), <= CRX_MAX_SS */
    double Q[6];           /* diag(matrix_Q)  (utils/base.py:353; zero by default) */
    double R[2];           /* diag(matrix_R)  (:354)  [1, 0.25] */
    double dR[2];          /* diag(matrix_dR) (:356)  [4, 0] */
    double x_track[6];     /* [5,0,0,0,0,0] (control.py:649) */
    double v_max;          /* vx_i <= v_max, i < N      (control.py:658) */
    double ey_max;         /* |ey_i| <= lap_width, i < N (:659-660) */
    double delta_max;      /* (:662-663) */
    double a_max;          /* (:665-666) */
    double w_x0;           /* 1e4: weight of the squared initial-state relaxation, used by the second attempt only
                              (see crx_lmpc_solve) */
    crx_ipm_opts opts;
} crx_lmpc_desc;

/* ---- iLQR of the ego racer (control/control.py:64-195 ilqr, control/ilqr_helper.py:4-55) ----------------------------------
 * Quirks of the reference kept on purpose (crx_ilqr.hip names them at the lines that implement them):
 *   I1  the obstacle is the LAST non-ego vehicle in `vehicles` order (control.py:99-104 overwrites obs_traj in its loop); its
 *       dimensions always come from the vehicle named "car1" (:106-109).  The reference raises NameError with no other vehicle;
 *       here n_obs = 0 means no barrier term (a deviation).  The kernel sums the barrier terms of n_obs obstacles (what the
 *       helper's comment intends, ilqr_helper.py:33); the control.ilqr mirror passes exactly one, as the reference does.
 *   I2  stage derivatives cover stages 0..N-1 only (ilqr_helper.py:29): the terminal Vx, Vxx are stage N-1's running derivatives
 *       (control.py:136-137), so stage N-1 enters twice and stage N never enters the backward pass.  Stage N enters the cost.
 *   I3  the cost of the accept and stop tests has no barrier term: sum_{k<N} (x_k-xt)'Q(x_k-xt) + u_k'Ru_k + (x_N-xt)'Q(x_N-xt).
 *   I4  Qux = B' Vxx A with no l_ux (:145); Vx = Qx - K' Quu k, Vxx = Qxx - K' Quu K use the UNREGULARISED Quu (:158-159); k, K use
 *       V diag(1 / (max(l_i, 0) + lamb)) V' (:147-151).
 *   I5  barrier of degree 2, h = 1 + margin - d' P d, P = diag(1/l_sum^2, 1/w_sum^2) on (ds, dey); gradient q1 q2 e^{q2 h} h',
 *       Hessian q1 q2^2 e^{q2 h} h' h'^T (Gauss-Newton, no -2P term; ilqr_helper.py:36-52); ds = s_k - s_obs,k - lap_off with
 *       lap_off = (int(s_ego / L) - int(s_obs,0 / L)) L (int() truncates toward zero; the obstacle's cycle from its stage 0 only).
 *   I6  no warm start: every call starts from u = 0 (:86); no input or state bounds.
 * Stops: CRX_CONVERGED = relative decrease below eps after an accepted step (the reference prints "Convergence achieved",
 * :181-183); CRX_STALLED = lamb > lamb_max (:187-188); CRX_MAX_ITER = max_iter backward passes.  iters counts backward passes
 * (= the reference's get_cost_derivation calls). */
typedef struct crx_ilqr_desc {
    int32_t N;             /* ilqr_param.num_horizon (utils/base.py:175), 1..CRX_ILQR_MAX_N; 50 */
    int32_t max_iter;      /* ilqr_param.max_iter (:174), 150 */
    int32_t n_obs_max;     /* leading dimension of obs_s / obs_ey / lap_off, 0..CRX_MAX_OBS */
    int32_t pad_;
    double A[36];          /* matrix_A, row-major (:168; data/sys/LTI/matrix_A.csv) */
    double B[12];          /* matrix_B, row-major 6x2 (:169) */
    double Q[36];          /* matrix_Q, full (:170) diag(10, 0, 0, 4, 0, 40) */
    double R[4];           /* matrix_R, full (:171) diag(0.1, 0.1) */
    double eps;            /* 0.01  relative-decrease stop (control.py:80) */
    double lamb_init;      /* 1     (:81) */
    double lamb_factor;    /* 10    (:82) */
    double lamb_max;       /* 1000  (:83) */
    double margin;         /* 0.15  safety_margin (ilqr_helper.py:25) */
    double q1, q2;         /* 2.5, 2.5 (ilqr_helper.py:26-27) */
    double l_sum;          /* l_agent + l_obs, half lengths (control.py:106-108): 0.4 */
    double w_sum;          /* w_agent + w_obs, half widths (:107-109): 0.2 */
} crx_ilqr_desc;

/* Defaults above; A, B copied when non-NULL (zero otherwise). */
void crx_ilqr_desc_default(crx_ilqr_desc* d, int N, const double* A, const double* B);
/* x0 [batch][6], xt [batch][6]; obs_s, obs_ey [batch][n_obs_max][N+1]; lap_off [batch][n_obs_max]; n_obs [batch] in
 * [0, n_obs_max].  X [batch][N+1][6], U [batch][N][2]: the accepted trajectory (the reference returns U[0], control.py:195);
 * cost [batch]: its barrier-free cost (I3); status [batch]; iters [batch]. */
int crx_ilqr_solve(const crx_ilqr_desc* d, int batch, const double* x0, const double* xt, const double* obs_s, const double* obs_ey,
                   const double* lap_off, const int32_t* n_obs, double* X, double* U, double* cost, int32_t* status, int32_t* iters);
/* device pointers; active [batch] as in the masked launches (NULL = all; 0 = CRX_SKIPPED, outputs untouched) */
int crx_ilqr_solve_dev(const crx_ilqr_desc* d, int batch, const int32_t* active, const double* x0, const double* xt,
                       const double* obs_s, const double* obs_ey, const double* lap_off, const int32_t* n_obs, double* X, double* U,
                       double* cost, int32_t* status, int32_t* iters, void* stream);

/* Per-problem models: crx_ilqr_solve / crx_ilqr_solve_dev with model_A [batch][6][6] and model_B [batch][6][2] after x0.  Problem b
 * runs on (model_A[b], model_B[b]); d->A and d->B are ignored.  Both NULL: the shared launch of d->A, d->B, bit for bit; one NULL
 * is CRX_ERR_ARG.  A problem fed a copy of d's model gives the bits of the shared launch. */
int crx_ilqr_solve_models(const crx_ilqr_desc* d, int batch, const double* x0, const double* model_A, const double* model_B,
                          const double* xt, const double* obs_s, const double* obs_ey, const double* lap_off, const int32_t* n_obs,
                          double* X, double* U, double* cost, int32_t* status, int32_t* iters);
int crx_ilqr_solve_models_dev(const crx_ilqr_desc* d, int batch, const int32_t* active, const double* x0, const double* model_A,
                              const double* model_B, const double* xt, const double* obs_s, const double* obs_ey,
                              const double* lap_off, const int32_t* n_obs, double* X, double* U, double* cost, int32_t* status,
                              int32_t* iters, void* stream);

/* ---- LQR tracking controller (control/control.py:28-61 lqr) for a batch of models --------------------------------------------
 * The reference's Riccati fixed point, one design per model (A, B):
 *     P = Q
 *     repeat at most max_iter times:
 *         P' = A'PA - A'(PB) inv(R + B'(PB)) B'P A + Q
 *         if max|P' - P| < eps: stop, and discard P'
 *         P = P'
 *     K = inv(B'PB + R) B'P A
 * in the operation order of the host mirror control._lqr_gain.  Semantics of the reference kept on purpose:
 *   L1  the gain comes from the P in hand when the test passes, not from the iterate that passed it (:49-53); max_iter = 0 gives
 *       the gain of P = Q.
 *   L2  P is never symmetrised; A'(PB) and B'P are formed separately.  A transposed shortcut such as (B'PA)' for A'PB lets the
 *       asymmetry of P grow and lands on other iterates and other iteration counts.
 *   L3  the stop test is strict: < eps on the max-norm of the full 6x6 difference.  The 2x2 inverse is the plain adjugate over the
 *       determinant.
 *   L4  status: CRX_CONVERGED = the test passed; CRX_MAX_ITER = max_iter steps without passing, K is still the gain of the last P
 *       (what the reference silently returns); CRX_SINGULAR = a non-finite entry in A, B, an iterate or K, or a zero or non-finite
 *       determinant: K and P are NaN, no path leaves a finite wrong number.  The loop is bounded by max_iter whatever the data.
 * iters = the Riccati steps computed (the reference's loop count; the step that passes or fails counts; 0 for a non-finite
 * model).  A design is bit-identical whatever the batch and the model's position in it. */
typedef struct crx_lqr_desc {
    int32_t max_iter;      /* 50    LQRTrackingParam.max_iter (utils/base.py) */
    int32_t pad_;
    double Q[36];          /* matrix_Q, full: diag(10, 0, 0, 4, 0, 40) */
    double R[4];           /* matrix_R, full: diag(0.1, 0.1) */
    double eps;            /* 0.01  (control.py:44) */
} crx_lqr_desc;

/* Defaults above. */
void crx_lqr_desc_default(crx_lqr_desc* d);
/* Host pointers.  A [batch][6][6], B [batch][6][2] (always per problem; one model = batch 1); K [batch][2][6]; P [batch][6][6]
 * (the P behind K) may be NULL; iters, status [batch]. */
int crx_lqr_design(const crx_lqr_desc* d, int batch, const double* A, const double* B, double* K, double* P, int32_t* iters,
                   int32_t* status);
/* device pointers; active [batch] as in the masked launches (NULL = all; 0 = CRX_SKIPPED, outputs untouched) */
int crx_lqr_design_dev(const crx_lqr_desc* d, int batch, const int32_t* active, const double* A, const double* B, double* K, double* P,
                       int32_t* iters, int32_t* status, void* stream);
/* u[b] = -K[b] (xcurv[b] - xt[b]): K [batch][2][6], xcurv, xt [batch][6], u [batch][2]; six-term sums in ascending index order. */
int crx_lqr_step_dev(int batch, const double* K, const double* xcurv, const double* xt, double* u, void* stream);

/* ---- LTI system identification (system/system_identification.py:4-43 linear_regression, get_udata) ------------------------
 * Batched ridge regression of x_{k+1} on (x_k, u_k) over packed logs, FP64 on the device.  Semantics of the reference kept:
 *   S1  rows used: Y = x[2:T], X = [x[1:T-1] | u[1:T-1]] of each log (first_row = 1: row 0 is dropped), T - 2 pairs for a log of
 *       T rows; pairs never cross two logs.  A group (a contiguous run of logs) pools the pairs of its logs into one fit.
 *   S2  no unwrapping: the lap wrap of s stays in the data, as logged.
 *   S3  W = inv(X'X + lamb I) (X'Y): the inverse is formed as numpy does (LU with partial pivoting, solved against I), then
 *       multiplied; no direct solve.  A zero or non-finite pivot is CRX_SINGULAR (numpy raises LinAlgError).
 *   S4  A = W'[:, 0:6], B = W'[:, 6:8]; err = [max_rows(XW - Y); min_rows(XW - Y)], [2][6] (NaN propagates, as numpy's max).
 *   S5  get_udata (the lap-by-lap assembly of ego.inputs and lap_inputs) stays on the host (crx.montecarlo.PidLaps logs u in
 *       the layout it produces: u[k] = the input applied in the step that produced x[k]).
 * Summation: (log, chunk) tiles of chunk_rows pairs, one workgroup each; lanes accumulate their pairs in ascending order, the
 * wave reduces with crx_wave.h's fixed butterfly, the waves in ascending order.  The tiles of a group are summed by the group's
 * solve workgroup: the group's logs are dealt to its 256 lanes in turn (log j to lane j mod 256), a lane adds its logs' tiles
 * log ascending, tile ascending, then the lanes are reduced as above.  The order depends on the group's own logs and
 * chunk_rows only: a fit is bit-identical whatever the batch, the position of its logs in it and the other groups launched
 * with it.  No atomics. */
typedef struct crx_sysid_desc {
    double lamb;           /* 1e-9: ridge coefficient (system_identification_test.py:42) */
    int32_t first_row;     /* 1: first log row that enters X (S1) */
    int32_t chunk_rows;    /* 8192: pairs per tile (part of the summation order; 64..65536, a multiple of 256) */
    int32_t reserved[4];   /* 0 */
} crx_sysid_desc;

/* Defaults above. */
void crx_sysid_desc_default(crx_sysid_desc* d);
/* Host pointers.  x [rows][6], u [rows][2] packed logs; log l is rows log_offset[l] .. log_offset[l+1]-1 (int64, non-decreasing,
 * log_offset[0] >= 0, rows = log_offset[n_logs]).  group_offset [n_groups+1] (int32, non-decreasing from 0 to n_logs): group g
 * pools logs group_offset[g] .. group_offset[g+1]-1; NULL = one group per log (n_groups must then equal n_logs).
 * Outputs per group: A [g][6][6], B [g][6][2], err [g][2][6], n_pairs [g] (int64), status [g]: CRX_CONVERGED (0), CRX_SKIPPED
 * (no pair in the group), CRX_SINGULAR; A, B, err are NaN unless the status is 0. */
int crx_sysid_fit(const crx_sysid_desc* d, int n_logs, const int64_t* log_offset, const int32_t* group_offset, int n_groups,
                  const double* x, const double* u, double* A, double* B, double* err, int64_t* n_pairs, int32_t* status);
/* Bytes of device workspace crx_sysid_fit_dev needs for n_logs logs of at most max_log_rows rows in n_groups groups. */
size_t crx_sysid_workspace_bytes(const crx_sysid_desc* d, int n_logs, int n_groups, int64_t max_log_rows);
/* Device pointers.  Same arrays; max_log_rows bounds every log's length (the tiles of a log are laid out in the workspace at a
 * stride of ceil(max_log_rows / chunk_rows)); workspace of ws_bytes >= crx_sysid_workspace_bytes(...) bytes.  The offsets are
 * not validated on the device: they must satisfy the host entry point's rules and max_log_rows. */
int crx_sysid_fit_dev(const crx_sysid_desc* d, int n_logs, const int64_t* log_offset, const int32_t* group_offset, int n_groups,
                      int64_t max_log_rows, const double* x, const double* u, void* workspace, size_t ws_bytes, double* A, double* B,
                      double* err, int64_t* n_pairs, int32_t* status, void* stream);
/* One control step of PIDTracking (control/control.py:15-25 pid; utils/base.py PIDTracking) for a batch of vehicles, with the
 * log row of the step before it.  xcurv [batch][6]: the state the plant just produced.  row >= 0: x_log[b][row] = xcurv[b] and
 * u_log[b][row] = u_prev[b] (logs [batch][T][6] / [batch][T][2], row < T); row < 0: nothing is logged.  u_next [batch][2] (may be
 * NULL) = pid(xcurv[b]) with the target (vt[b], eyt[b]): delta = -0.6 (ey - eyt) - 0.9 epsi, a = 1.5 (vt - vx). */
int crx_pid_log_dev(int batch, int T, int row, const double* vt, const double* eyt, const double* xcurv, const double* u_prev,
                    double* u_next, double* x_log, double* u_log, void* stream);

/* ---- region selection (overtake_traj_planner.py:205-246) ------------------------------------- */
typedef struct crx_select_desc {
    int32_t N;
    int32_t n_veh_max;     /* leading dimension V of the obstacle arrays; regions R = V + 1 */
    double veh_length;     /* 0.4 */
    double veh_width;      /* 0.2 */
    double lap_length;     /* obstacle s is wrapped `while s > lap_length` (:216-217) */
    double w_prog;         /* 10  (:209) */
    double w_coll;         /* 100 (:223,:237) */
    double w_switch;       /* 100 (:243) */
} crx_select_desc;

/* ---- planner host prep on the device (planner_helper.py:43-153, overtake_traj_planner.py:277-324) ---- */
typedef struct crx_prep_desc {
    int32_t N;             /* num_horizon_planner */
    int32_t n_veh_max;     /* leading dimension V of the per-vehicle arrays; regions R = V + 1 */
    int32_t n_opt;         /* rows of the optimal-trajectory table (data/optimal_traj/xcurv_*.csv) */
    int32_t reserved0;
    double prediction_factor; /* 0.5  racing_game_param.planning_prediction_factor (planner_helper.py:51-53) */
    double lookahead;      /* 4.0  literal in the end point s3 = s0 + factor * max|dv| + 4 (:51-53) */
    double track_width;    /* track.width */
    double lap_length;
    double veh_length;     /* 0.4 */
    double veh_width;      /* 0.2 */
    double safety_margin;  /* 0.15 (overtake_traj_planner.py:288) */
    double dt_ref;         /* 0.1  literal time step of the window test (:296) */
} crx_prep_desc;

/* ---- plant of the simulator (system/vehicle_dynamics.py:4-49, utils/base.py:897-942) ------------------ */
#define CRX_PLANT_NPARAM 10 /* doubles per vehicle of a `params` array: m, lf, lr, Iz, Df, Cf, Bf, Dr, Cr, Br (BicycleDynamicsParam.get_params()) */
typedef struct crx_plant_desc {
    int32_t n_sub;         /* 100: explicit Euler sub-steps per control step (`while (i+1)*0.001 <= timestep`, base.py:905) */
    int32_t n_seg;         /* rows of the track table point_and_tangent (racing_env.py:17-120) */
    double dt_sub;         /* 0.001 (base.py:899) */
    double lap_length;
    double m, lf, lr, Iz;  /* BicycleDynamicsParam (base.py:686-697): 1.98, 0.125, 0.125, 0.024 */
    double Df, Cf, Bf;     /* front Pacejka: 0.8*m*g/2, 1.25, 1.0 */
    double Dr, Cr, Br;     /* rear  Pacejka */
} crx_plant_desc;

/* ---- overtake PATH planner QP (planning/overtake_path_planner.py:199-318) ------------------------------- */
typedef struct crx_path_desc {
    int32_t N;             /* num_horizon_planner: N+1 lateral offsets per candidate path */
    int32_t reserved0;
    double alpha;          /* racing_game_param.alpha: weight of the Bezier reference; 1 - alpha on the optimal line (:248-250) */
    double w_rate;         /* 100: weight on (ey_j - ey_{j-1})^2 (:252-253) */
    crx_ipm_opts opts;
} crx_path_desc;

/* library management */
int crx_version(void);
/* device >= 0: HIP device ordinal.  There is no CPU back-end in this library: a missing device is
 * an error (CRX_ERR_NO_DEVICE), never a silent fall-back. */
int crx_init(int device);
void crx_shutdown(void);
const char* crx_last_error(void);
int crx_device_count(void);

void crx_ipm_opts_default(crx_ipm_opts* o);
void crx_planner_desc_default(crx_planner_desc* d, int N, const double* A, const double* B);
void crx_cbf_desc_default(crx_cbf_desc* d, int N, int n_obs_max, const double* A, const double* B);
void crx_select_desc_default(crx_select_desc* d, int N, int n_veh_max, double lap_length);
void crx_lmpc_desc_default(crx_lmpc_desc* d, int N, int n_ss_max);
void crx_path_desc_default(crx_path_desc* d, int N, double alpha);
void crx_plant_desc_default(crx_plant_desc* d, int n_seg, double lap_length);
void crx_prep_desc_default(crx_prep_desc* d, int N, int n_veh_max, int n_opt, double track_width, double lap_length);

/*
 * Planner region QPs.  One problem per (scenario, region).
 *   x0      [batch][6]      ego.xcurv, raw (quirk Q5: the start-line-wrapped copy is only used by
 *                           the host when it builds ey_lb)
 *   bez_s   [batch][N+1]    Bezier reference polyline, s coordinates   (bezier_xcurvs[r,:,0])
 *   bez_ey  [batch][N+1]    ... ey coordinates                         (bezier_xcurvs[r,:,1])
 *   ey_lb   [batch][N]      effective lower bound on ey_k, k=0..N-1: max of -(ey_ub) and the
 *                           neighbour constraints active at k (:286-324, quirk Q2)
 *   ey_ub   [batch]         track.width - 0.5*veh_width (:277-278)
 *   X       [batch][N+1][6] out: solution, or fall-back trajectory when status != 0
 *   U       [batch][N][2]   out: inputs (zeros with the fall-back)
 *   cost    [batch]         out: sol.value(cost) (:364); +inf with the fall-back (:374)
 *   status  [batch]         out: crx_status
 *   kkt     [batch]         out: final scaled KKT error
 *   iters   [batch]         out: interior-point iterations
 */
int crx_planner_solve(const crx_planner_desc* d, int batch, const double* x0, const double* bez_s,
                      const double* bez_ey, const double* ey_lb, const double* ey_ub, double* X,
                      double* U, double* cost, int32_t* status, double* kkt, int32_t* iters);
int crx_planner_solve_dev(const crx_planner_desc* d, int batch, const double* x0,
                          const double* bez_s, const double* bez_ey, const double* ey_lb,
                          const double* ey_ub, double* X, double* U, double* cost, int32_t* status,
                          double* kkt, int32_t* iters, void* stream);

/*
 * Region selection.  Scenario i has n_veh[i] <= V sorted vehicles and n_veh[i]+1 regions.
 *   X        [n_scen][V+1][N+1][6]  per-region trajectories (solution_xvar, transposed)
 *   obs_s    [n_scen][V][N+1]       predicted s of sorted vehicle v (obs_infos[name][4,:])
 *   obs_ey   [n_scen][V][N+1]
 *   old_flag [n_scen]               previous direction_flag, -1 for None (:238-243)
 *   flag     [n_scen]               out: direction_flag (first arg-min, :244)
 *   sel_cost [n_scen][V+1]          out: cost_selection (regions >= n_veh+1: +inf)
 *   best_X   [n_scen][N+1][6]       out: traj_xcurv (:245)
 */
int crx_select(const crx_select_desc* d, int n_scen, const int32_t* n_veh, const double* X,
               const double* obs_s, const double* obs_ey, const int32_t* old_flag, int32_t* flag,
               double* sel_cost, double* best_X);
int crx_select_dev(const crx_select_desc* d, int n_scen, const int32_t* n_veh, const double* X,
                   const double* obs_s, const double* obs_ey, const int32_t* old_flag,
                   int32_t* flag, double* sel_cost, double* best_X, void* stream);

/*
 * One planner step for n_scen scenarios: all V+1 region QPs of every scenario (crx_planner_solve with
 * batch = n_scen*(V+1), scenario-major) followed by crx_select on the same stream, X staying on the
 * device in between.  Replaces solve_optimization_problem (overtake_traj_planner.py:162-246).
 * Arrays as in crx_planner_solve (leading dimension n_scen*(V+1)) and crx_select.
 */
int crx_planner_plan(const crx_planner_desc* d, const crx_select_desc* sd, int n_scen, const double* x0,
                     const double* bez_s, const double* bez_ey, const double* ey_lb, const double* ey_ub,
                     const int32_t* n_veh, const double* obs_s, const double* obs_ey, const int32_t* old_flag,
                     double* X, double* U, double* cost, int32_t* status, double* kkt, int32_t* iters,
                     int32_t* flag, double* sel_cost, double* best_X);
int crx_planner_plan_dev(const crx_planner_desc* d, const crx_select_desc* sd, int n_scen, const double* x0,
                         const double* bez_s, const double* bez_ey, const double* ey_lb, const double* ey_ub,
                         const int32_t* n_veh, const double* obs_s, const double* obs_ey,
                         const int32_t* old_flag, double* X, double* U, double* cost, int32_t* status,
                         double* kkt, int32_t* iters, int32_t* flag, double* sel_cost, double* best_X,
                         void* stream);
/* masked launch (see crx_cbf_solve_masked_dev): active [n_scen] on the device, 0 = none of this scenario's region QPs is
 * solved (their status = CRX_SKIPPED, X / U / cost untouched); the selection still runs for every scenario and, for a
 * skipped one, works on whatever X holds -- the caller ignores flag / best_X of the scenarios it masked out. */
int crx_planner_plan_masked_dev(const crx_planner_desc* d, const crx_select_desc* sd, int n_scen, const int32_t* active,
                                const double* x0, const double* bez_s, const double* bez_ey, const double* ey_lb,
                                const double* ey_ub, const int32_t* n_veh, const double* obs_s, const double* obs_ey,
                                const int32_t* old_flag, double* X, double* U, double* cost, int32_t* status, double* kkt,
                                int32_t* iters, int32_t* flag, double* sel_cost, double* best_X, void* stream);
/* One LTI model per region QP (a fleet of identified cars in the racing game: crx_sysid_fit leaves the models on the device).  Problem b is
 * solved with model_A [b][6][6], model_B [b][6][2] -- indexed exactly like x0, so a planner step brings n_scen * (V + 1) models, each scenario's
 * repeated for its V + 1 regions (there is no divisor: the caller expands once, 48 doubles per region).  d->A, d->B are not read.  Besides the
 * model the reachability screen needs, per problem, the free-response rows and input reach of ey at stages 0 .. N - 1 (what the library computes
 * on the host for the descriptor's model): model_reach, CRX_PLANNER_MODEL_REACH_DOUBLES(batch) doubles owned by the caller,
 * [batch][CRX_MAX_N][7] = (e_ey' A^j (6), reach_gain[j]), zero for j >= N, filled by crx_planner_models_reach_dev.  It depends on the models
 * and on d's N, delta_max, a_max only: a closed loop computes it once.  For copies of d's model it equals the descriptor's table bit for bit,
 * and the solve then equals the shared launch bit for bit at N = 10 / 12 (tuned kernels on both sides); every other horizon runs the general
 * (run-time horizon) kernel with models, also at N = 20 where the shared launch has a tuned one: same KKT point to solver tolerance.
 *   crx_planner_models_reach_dev   the table, one launch.
 *   crx_planner_solve_models_dev   = crx_planner_solve_dev + active ([batch], 0 = CRX_SKIPPED, outputs untouched; or NULL) and (model_A, model_B,
 *                                  model_reach) after x0.  All three NULL: the shared launch; any other mix of NULLs is CRX_ERR_ARG.
 *   crx_planner_solve_models       host pointers (model_A, model_B both or neither); stages them and computes the table itself.
 *   crx_planner_plan_models_dev    = crx_planner_plan_masked_dev + the three arrays after x0, leading dimension n_scen * (V + 1).
 *   crx_planner_plan_models        host pointers, as crx_planner_solve_models.
 * A problem whose model has a non-finite entry (a failed fit) is not iterated and is not an argument error: it answers as every failed region
 * QP does (overtake_traj_planner.py:365-374) -- X the fall-back trajectory, U 0, cost +inf -- with status CRX_SINGULAR, iters 0, kkt inf, so the
 * selection treats it like an infeasible region. */
#define CRX_PLANNER_MODEL_REACH_DOUBLES(batch) ((size_t)(batch) * CRX_MAX_N * 7)
int crx_planner_models_reach_dev(const crx_planner_desc* d, int batch, const double* model_A, const double* model_B, double* model_reach,
                                 void* stream);
int crx_planner_solve_models_dev(const crx_planner_desc* d, int batch, const int32_t* active, const double* x0, const double* model_A,
                                 const double* model_B, const double* model_reach, const double* bez_s, const double* bez_ey,
                                 const double* ey_lb, const double* ey_ub, double* X, double* U, double* cost, int32_t* status, double* kkt,
                                 int32_t* iters, void* stream);
int crx_planner_solve_models(const crx_planner_desc* d, int batch, const double* x0, const double* model_A, const double* model_B,
                             const double* bez_s, const double* bez_ey, const double* ey_lb, const double* ey_ub, double* X, double* U,
                             double* cost, int32_t* status, double* kkt, int32_t* iters);
int crx_planner_plan_models_dev(const crx_planner_desc* d, const crx_select_desc* sd, int n_scen, const int32_t* active,
                                const double* x0, const double* model_A, const double* model_B, const double* model_reach,
                                const double* bez_s, const double* bez_ey, const double* ey_lb, const double* ey_ub,
                                const int32_t* n_veh, const double* obs_s, const double* obs_ey, const int32_t* old_flag, double* X,
                                double* U, double* cost, int32_t* status, double* kkt, int32_t* iters, int32_t* flag, double* sel_cost,
                                double* best_X, void* stream);
int crx_planner_plan_models(const crx_planner_desc* d, const crx_select_desc* sd, int n_scen, const double* x0, const double* model_A,
                            const double* model_B, const double* bez_s, const double* bez_ey, const double* ey_lb,
                            const double* ey_ub, const int32_t* n_veh, const double* obs_s, const double* obs_ey,
                            const int32_t* old_flag, double* X, double* U, double* cost, int32_t* status, double* kkt, int32_t* iters,
                            int32_t* flag, double* sel_cost, double* best_X);

/*
 * Planner host prep on the device: per scenario, the cubic Bezier reference of
 * every region (planner_helper.get_bezier_control_points :43-135 and get_bezier_curve :138-153, sampled
 * as overtake_traj_planner.py:105-111) and the per-stage ey bounds with the obstacle windows
 * (overtake_traj_planner.py:277-324, quirks Q2/Q5), written directly in the layout crx_planner_solve reads.
 *   x_wrapped [S][6]   start-line-wrapped ego state (xcurv_ego: control points :49,95 and window test :296)
 *   x_raw     [S][6]   ego.xcurv as stored on the vehicle (becomes x0 of every region, :266, quirk Q5)
 *   n_veh     [S]      vehicles of interest, 0..V
 *   veh_info  [S][V][3] rows (s, max ey over the prediction, min ey) in ITERATION order (quirk Q4, :87-92)
 *   max_dv    [S]      agent_info.max_delta_v (planner_helper.py:177-201)
 *   obs_s, obs_ey [S][V][N+1]  predictions of the SORTED vehicles
 *   opt_s, opt_ey [n_opt]      columns 4 and 5 of the optimal-trajectory table (shared by all scenarios;
 *                              precondition: the end point s3 lies inside the table, else the reference raises)
 * outputs, S*(V+1) leading dimension, scenario-major: x0 [.][6], bez_s, bez_ey [.][N+1], ey_lb [.][N], ey_ub [.]
 */
int crx_planner_prep(const crx_prep_desc* d, int n_scen, const double* x_wrapped, const double* x_raw,
                     const int32_t* n_veh, const double* veh_info, const double* max_dv, const double* obs_s,
                     const double* obs_ey, const double* opt_s, const double* opt_ey, double* x0, double* bez_s,
                     double* bez_ey, double* ey_lb, double* ey_ub);
int crx_planner_prep_dev(const crx_prep_desc* d, int n_scen, const double* x_wrapped, const double* x_raw,
                         const int32_t* n_veh, const double* veh_info, const double* max_dv, const double* obs_s,
                         const double* obs_ey, const double* opt_s, const double* opt_ey, double* x0,
                         double* bez_s, double* bez_ey, double* ey_lb, double* ey_ub, void* stream);

/*
 * The front of OvertakeTrajPlanner on the device (remainder): per scenario
 *   which vehicles are of interest   get_overtake_flag -> planner_helper.check_ego_agent_distance (:218-266)
 *   the reference's partial ey "sort" overtake_traj_planner.py:66-76 (quirk Q3: every vehicle is compared with the CURRENT FIRST only)
 *   veh_info rows (s, max ey, min ey)  :87-92, in ITERATION order although consumed as if sorted (quirk Q4)
 *   agent_info.max_delta_v            planner_helper.get_agent_info (:177-201)
 *   predictions of the sorted vehicles  obs_infos[name][4:6, :] (:77-85)
 * Outputs are exactly the vehicle inputs of crx_planner_prep and crx_select.
 *   ego_xcurv [S][6]         the ego vehicle's state (the vehicle object's xcurv: both tests read it)
 *   n_all     [S]            vehicles in the scenario besides the ego, 0..n_all_max, in the reference's dict order
 *   veh_xcurv [S][VA][6]     their current states;  pred_s, pred_ey [S][VA][N+1]  their predictions (get_trajectory_nsteps rows 4, 5)
 *   n_veh [S]                out: vehicles of interest (the planner runs iff > 0);  overflow [S]: of-interest vehicles beyond
 *                            n_veh_max that were dropped (the reference has no limit; libcrx plans around at most CRX_MAX_VEH).
 *                            On overflow the n_veh_max vehicles NEAREST to the ego along the closed lap are kept (ties to the
 *                            earlier one), in dict order -- the closest car is never the one dropped.
 *   order [S][V]             out: vehicle index (0..n_all-1) of sorted vehicle k, -1 beyond n_veh
 *   veh_info [S][V][3], max_dv [S], obs_s, obs_ey [S][V][N+1]   out
 */
typedef struct crx_scene_desc {
    int32_t N;
    int32_t n_all_max;       /* VA: leading dimension of the vehicle arrays */
    int32_t n_veh_max;       /* V <= CRX_MAX_VEH */
    int32_t reserved0;
    double safety_factor;    /* 4.5  RacingGameParam.safety_factor */
    double prediction_factor;/* 0.5  planning_prediction_factor */
    double veh_length;       /* 0.4  ego.param.length */
    double lap_length;
} crx_scene_desc;
void crx_scene_desc_default(crx_scene_desc* d, int N, int n_all_max, int n_veh_max, double lap_length);
int crx_planner_scene(const crx_scene_desc* d, int n_scen, const double* ego_xcurv, const int32_t* n_all, const double* veh_xcurv,
                      const double* pred_s, const double* pred_ey, int32_t* n_veh, int32_t* overflow, int32_t* order,
                      double* veh_info, double* max_dv, double* obs_s, double* obs_ey);
int crx_planner_scene_dev(const crx_scene_desc* d, int n_scen, const double* ego_xcurv, const int32_t* n_all,
                          const double* veh_xcurv, const double* pred_s, const double* pred_ey, int32_t* n_veh,
                          int32_t* overflow, int32_t* order, double* veh_info, double* max_dv, double* obs_s, double* obs_ey,
                          void* stream);

/*
 * One control step of the plant for a batch of vehicles: n_sub explicit Euler
 * sub-steps of the dynamic bicycle with Pacejka tyres (system/vehicle_dynamics.py:4-49) in global and
 * curvilinear coordinates, the curvature looked up from the track table at every sub-step
 * (racing_env.py:225-246), exactly DynamicBicycleModel.forward_dynamics (base.py:897-942).  The reference's bounded
 * process noise (:929-939; ON by default, car_racing/tests/overtake_planner_test.py:41-42 makes zero-noise opt-in) is
 * applied by crx_plant_step_noise_dev from standard-normal draws the CALLER supplies (its RNG, its seed):
 *   noise_z [batch][3] or NULL   z ~ N(0,1) per vehicle for (vx, vy, wz); the kernel forms clip(0.01 z0, +-0.05),
 *                                clip(0.01 z1, +-0.1), clip(0.005 z2, +-0.05) and adds HALF of each to the curvilinear
 *                                velocities only (xglob_next keeps the noise-free ones, as the reference does).  NULL = zero noise.
 *   track [n_seg][6] rows (x, y, psi, s_start, length, curvature);  xglob, xcurv [batch][6];  u [batch][2]
 * crx_plant_step_wrap_dev additionally applies the lap bookkeeping of ModelBase.update_memory (base.py:795-819):
 * s > lap_length -> s -= lap_length, laps[b] += 1 (laps may be NULL).  u_stride = doubles between the inputs of
 * consecutive vehicles (2 for a packed array, 2N to read u_0 straight out of a crx_cbf_solve U array).
 */
int crx_plant_step_wrap_dev(const crx_plant_desc* d, int batch, const double* track, const double* xglob,
                            const double* xcurv, const double* u, int u_stride, double* xglob_next, double* xcurv_next,
                            int32_t* laps, void* stream);
int crx_plant_step_noise_dev(const crx_plant_desc* d, int batch, const double* track, const double* xglob,
                             const double* xcurv, const double* u, int u_stride, const double* noise_z, double* xglob_next,
                             double* xcurv_next, int32_t* laps, void* stream);
int crx_plant_step(const crx_plant_desc* d, int batch, const double* track, const double* xglob, const double* xcurv,
                   const double* u, double* xglob_next, double* xcurv_next);
int crx_plant_step_dev(const crx_plant_desc* d, int batch, const double* track, const double* xglob,
                       const double* xcurv, const double* u, double* xglob_next, double* xcurv_next, void* stream);
/*
 * The same step with one parameter set per vehicle (system/vehicle_dynamics.py:6 takes the set as its first argument; the
 * reference's simulator always passes the defaults, base.py:906):
 *   params [batch][CRX_PLANT_NPARAM] or NULL   row b = (m, lf, lr, Iz, Df, Cf, Bf, Dr, Cr, Br) of vehicle b, the order of
 *                                              BicycleDynamicsParam.get_params().  With params given, the descriptor's ten values
 *                                              are not used by the step, but the descriptor must still be a valid one.
 * crx_plant_step_params_dev is crx_plant_step_noise_dev with `params` (lap bookkeeping, optional noise_z and laps); with
 * params == NULL it IS crx_plant_step_noise_dev.  crx_plant_step_params_plain_dev and the host-pointer crx_plant_step_params are
 * crx_plant_step_dev / crx_plant_step with `params` (no lap bookkeeping, no noise); with params == NULL they are those.
 * crx_plant_step_params reads the rows and refuses (CRX_ERR_ARG, the first offending vehicle in crx_last_error()) one with
 * m <= 0, Iz <= 0 or a non-finite value.  The `_dev` entries cannot read device memory: a bad row gives THAT vehicle non-finite
 * states (1 / m, 1 / Iz and the tyre forces enter its own lane only) and touches no other vehicle.
 */
int crx_plant_step_params_dev(const crx_plant_desc* d, int batch, const double* track, const double* xglob,
                              const double* xcurv, const double* u, int u_stride, const double* noise_z, const double* params,
                              double* xglob_next, double* xcurv_next, int32_t* laps, void* stream);
int crx_plant_step_params_plain_dev(const crx_plant_desc* d, int batch, const double* track, const double* xglob,
                                    const double* xcurv, const double* u, const double* params, double* xglob_next,
                                    double* xcurv_next, void* stream);
int crx_plant_step_params(const crx_plant_desc* d, int batch, const double* track, const double* xglob, const double* xcurv,
                          const double* u, const double* params, double* xglob_next, double* xcurv_next);
/*
 * The same step with every vehicle on a track of its own.  A TRACK SET is four plain arrays:
 *   tracks [n_tracks][seg_stride][6]   table t holds track t's rows as `track` above; rows n_seg[t] .. seg_stride - 1 are padding, never read
 *   n_seg [n_tracks] (int32), lap_length [n_tracks]; n_tracks in [1, CRX_MAX_TRACKS], seg_stride in [1, 64]
 *   track_id [batch] (int32)           vehicle b drives on track track_id[b]: its curvature lookup, and its lap bookkeeping with lap_length[track_id[b]]
 * d->n_seg and d->lap_length are not used by the step, but the descriptor must still be a valid one (as for `params`, which may be NULL:
 * the descriptor's ten values).  crx_plant_step_tracks_dev is crx_plant_step_params_dev on a track set (lap bookkeeping, optional noise_z
 * and laps); crx_plant_step_tracks_plain_dev and the host-pointer crx_plant_step_tracks have no lap bookkeeping and no noise.  The rows of a
 * launch whose vehicles all name the same track are the bits of the one-table entries on that table.
 * crx_plant_step_tracks reads its arrays and refuses (CRX_ERR_ARG, the first offender in crx_last_error()) a track_id outside [0, n_tracks),
 * an n_seg[t] outside [1, seg_stride], a lap length that is not positive and finite, and a bad parameter row.  The `_dev` entries cannot read
 * device memory: a vehicle with a track_id outside [0, n_tracks) gets non-finite states (its lap counter is left alone) and touches no other
 * vehicle -- the id never becomes an address; an n_seg[t] is clamped to [0, seg_stride].
 * The tables are read from LDS per lane: a wavefront whose vehicles sit on different tracks reads different rows in the scan, one whose
 * vehicles share a track reads one row (a broadcast).  A batch sorted by track makes every wavefront but a few uniform.
 */
#define CRX_MAX_TRACKS 8
int crx_plant_step_tracks_dev(const crx_plant_desc* d, int batch, int n_tracks, int seg_stride, const double* tracks, const int32_t* n_seg,
                              const double* lap_length, const int32_t* track_id, const double* xglob, const double* xcurv, const double* u,
                              int u_stride, const double* noise_z, const double* params, double* xglob_next, double* xcurv_next,
                              int32_t* laps, void* stream);
int crx_plant_step_tracks_plain_dev(const crx_plant_desc* d, int batch, int n_tracks, int seg_stride, const double* tracks,
                                    const int32_t* n_seg, const double* lap_length, const int32_t* track_id, const double* xglob,
                                    const double* xcurv, const double* u, const double* params, double* xglob_next, double* xcurv_next,
                                    void* stream);
int crx_plant_step_tracks(const crx_plant_desc* d, int batch, int n_tracks, int seg_stride, const double* tracks, const int32_t* n_seg,
                          const double* lap_length, const int32_t* track_id, const double* xglob, const double* xcurv, const double* u,
                          const double* params, double* xglob_next, double* xcurv_next);

/*
 * Overtake PATH planner: one 1-D QP per candidate region
 * (overtake_path_planner.py:199-318).  Variables ey_0..ey_N along fixed s samples;
 *   cost  sum_j (1-alpha)(ey_j - opt_j)^2 + alpha (ey_j - bez_j)^2  +  w_rate sum_{j>=1} (ey_j - ey_{j-1})^2      (:246-253)
 *   ey_0 = e0 (:258), ey_N = eN (:261), lb_j <= ey_j <= ub_j (track box :263-264 and the neighbours' side rows :265-297,
 *   merged by the caller; a row the reference skips is +-inf)
 *   opt, bez, lb, ub [batch][N+1];  e0, eN [batch];  E [batch][N+1];  cost [batch] (inf unless converged, :311)
 * status CRX_INFEASIBLE: an end point violates its own box or lb_j > ub_j somewhere (the reference then keeps IPOPT's
 * debug iterate, :310; here E holds the end points joined by the box-clipped Bezier reference).
 */
int crx_path_solve(const crx_path_desc* d, int batch, const double* opt, const double* bez, const double* lb,
                   const double* ub, const double* e0, const double* eN, double* E, double* cost, int32_t* status,
                   double* kkt, int32_t* iters);
int crx_path_solve_dev(const crx_path_desc* d, int batch, const double* opt, const double* bez, const double* lb,
                       const double* ub, const double* e0, const double* eN, double* E, double* cost, int32_t* status,
                       double* kkt, int32_t* iters, void* stream);

/*
 * The overtake PATH planner around its QPs, on the device (remainder): from the outputs of
 * crx_planner_scene to a flag and a target trajectory.  Restates planning/overtake_path_planner.py (line numbers into it unless another
 * file is named) operation by operation, products and sums rounded separately (no contraction).  Its quirks are kept, not repaired:
 *   P1  obstacle rows (s, max ey, min ey) are indexed by SORTED vehicle (:60-75; the trajectory planner's iteration order, quirk Q4, does
 *       not apply): s = veh_xcurv[s][order[k]][4], the vehicle's current state; max / min over the sorted prediction obs_ey[s][k][0..N].
 *   P2  control points: get_bezier_control_points (planner_helper.py:43-135) on the P1 rows and the WRAPPED ego state; the end point is
 *       s3 = s0 + prediction_factor max_dv + lookahead (:78-87), its ey the optimal line's; polylines sampled at t = j (1/N) (:88-100).
 *       An end point above the optimal-trajectory table raises in the reference: CRX_OUT_OF_DOMAIN here.
 *   P3  span = max_s + safety_factor veh_length + prediction_factor max_dv - ego_s_raw (:117-127, :230-240); max_s from get_agent_info
 *       (planner_helper.py:177-201): every s <= next_lap_range gets + lap_length (a literal 20 that fits l_shape, applied to every car),
 *       the maximum is then wrapped with `while > lap_length`.
 *   P4  sample position s_tmp = ego_s_raw + span j / N; `while >= lap_length` subtract; if <= opt_s[0] it becomes opt_s[0]; then it is
 *       clipped into the s-range of REGION 0's polyline, for every region (:241-245).  opt[r][j] = the optimal line's ey at s_tmp,
 *       bez[r][j] = the clipped linear interpolation of region r's polyline at s_tmp (:249-251).
 *   P5  side rows (:266-299): front / rear = s +- safety_factor veh_length, each wrapped with `while > lap_length` (:184-197); a row is
 *       active iff not (s_tmp < rear or s_tmp > front) -- no wrap awareness: rear > front is an empty window.  The left neighbour
 *       (sorted[r-1]) bounds from above with min ey - safety_factor veh_width, the right one (sorted[r]) from below with
 *       max ey + safety_factor veh_width; at j = 0 a row the raw ego ey is already beyond is skipped; strict inequalities are taken as
 *       non-strict; rows are merged with the track box +-track_width.
 *   P6  end points: e0 = the raw ego ey, eN = the Bezier end point's ey (cps[r][3][1]).
 *   P7  selection (:313-317): the FIRST minimum of the region costs, +inf for every region that did not converge; all +inf: flag 0, and E
 *       of region 0 is what crx_path_kernel wrote for a failed QP (its documented fall-back).
 *   P8  target (:113-143, :173-182): target[j][5] = E[flag][j]; target[j][4] = ego_s_raw + span j / N, unwrapped; vx_target = the optimal
 *       trajectory's vx at s_q (three-way case :129-137); delta_t = 2 (s_N - x_w[4]) / (vx_target + x_w[0]);
 *       a = clip((vx_target - x_w[0]) / delta_t, +-a_max_plan); row 0 = the whole wrapped state x_w; vx_j = sqrt(x_w[0]^2 + 2 a
 *       (target[j][4] - x_w[4])) for j = 0..N-1, AFTER row 0 was overwritten; row N's vx stays 0; every other column 0.  A negative
 *       radicand is NaN, as in numpy.  s_q above the table raises in the reference: CRX_OUT_OF_DOMAIN here.
 */
typedef struct crx_pathprep_desc {
    int32_t N;               /* num_horizon_planner */
    int32_t n_veh_max;       /* V <= CRX_MAX_VEH: leading dimension of order / obs_ey; regions = V + 1 */
    int32_t n_opt;           /* rows of the optimal-trajectory table */
    int32_t n_all_max;       /* VA: leading dimension of veh_xcurv (crx_scene_desc.n_all_max) */
    double safety_factor;    /* 4.5  P3, P5 */
    double prediction_factor;/* 0.5  P2, P3 */
    double lookahead;        /* 4.0  P2: the literal of planner_helper.py:51-53 */
    double next_lap_range;   /* 20.0 P3: the literal of planner_helper.py:178 */
    double track_width;      /* P2, P5 */
    double lap_length;
    double veh_length;       /* 0.4  P3, P5 */
    double veh_width;        /* 0.2  P2, P5 */
    double a_max_plan;       /* 1.5  P8: the literal of :140 */
} crx_pathprep_desc;
void crx_pathprep_desc_default(crx_pathprep_desc* d, int N, int n_veh_max, int n_all_max, int n_opt, double track_width, double lap_length);
/*
 * crx_path_prep: P1-P6, written directly in the layout crx_path_solve reads (leading dimension S (V+1), scenario-major).
 *   x_wrapped, x_raw [S][6];  n_veh [S], order [S][V], max_dv [S], obs_ey [S][V][N+1]: outputs of crx_planner_scene;
 *   veh_xcurv [S][VA][6]: the vehicles' current states (the scene's input);  opt_s, opt_ey [n_opt]: columns 4, 5 of the table
 *   opt, bez, lb, ub [S(V+1)][N+1];  e0, eN [S(V+1)];  span [S]                                                         out
 * Regions beyond n_veh[s] repeat region n_veh[s] (never selected).  A scenario with n_veh == 0 is not planned (the reference never plans
 * then; max_s is undefined): its outputs keep their contents.  A CRX_OUT_OF_DOMAIN scenario (P2, or a non-finite input) gets NaN in
 * every output, which its QPs answer with CRX_INFEASIBLE.  n_veh and order are clamped into range (device data cannot be validated).
 */
int crx_path_prep(const crx_pathprep_desc* d, int n_scen, const double* x_wrapped, const double* x_raw, const int32_t* n_veh,
                  const int32_t* order, const double* veh_xcurv, const double* max_dv, const double* obs_ey, const double* opt_s,
                  const double* opt_ey, double* opt, double* bez, double* lb, double* ub, double* e0, double* eN, double* span);
int crx_path_prep_dev(const crx_pathprep_desc* d, int n_scen, const double* x_wrapped, const double* x_raw, const int32_t* n_veh,
                      const int32_t* order, const double* veh_xcurv, const double* max_dv, const double* obs_ey, const double* opt_s,
                      const double* opt_ey, double* opt, double* bez, double* lb, double* ub, double* e0, double* eN, double* span,
                      void* stream);
/*
 * crx_path_plan: one path-planner step, crx_path_prep -> the region QPs (crx_path_kernel's source under a per-QP mask) -> P7, P8, three
 * launches on one stream.  Inputs of crx_path_prep plus opt_vx [n_opt] (column 0 of the table) and active [S] (may be NULL = all).
 *   E [S(V+1)][N+1], cost, status, kkt, iters [S(V+1)]   per region, as crx_path_solve
 *   flag [S], target [S][N+1][6], plan_status [S]        per scenario; plan_status = 0, CRX_SKIPPED or CRX_OUT_OF_DOMAIN
 * Scenarios that must not be planned -- n_veh[s] == 0 or active[s] == 0: every region answers status CRX_SKIPPED with cost +inf
 * (iters 0; E, kkt untouched), flag -1, plan_status CRX_SKIPPED, target untouched.  CRX_OUT_OF_DOMAIN: flag -1, target NaN.
 * The device entry leaves the prep arrays and the QP mask where the caller can read them: opt .. span as crx_path_prep_dev, and
 * qp_active [S(V+1)] int32.  The host entry keeps them in its staging.
 */
int crx_path_plan(const crx_pathprep_desc* d, const crx_path_desc* qd, int n_scen, const int32_t* active, const double* x_wrapped,
                  const double* x_raw, const int32_t* n_veh, const int32_t* order, const double* veh_xcurv, const double* max_dv,
                  const double* obs_ey, const double* opt_s, const double* opt_ey, const double* opt_vx, double* E, double* cost,
                  int32_t* status, double* kkt, int32_t* iters, int32_t* flag, double* target, int32_t* plan_status);
int crx_path_plan_dev(const crx_pathprep_desc* d, const crx_path_desc* qd, int n_scen, const int32_t* active, const double* x_wrapped,
                      const double* x_raw, const int32_t* n_veh, const int32_t* order, const double* veh_xcurv, const double* max_dv,
                      const double* obs_ey, const double* opt_s, const double* opt_ey, const double* opt_vx, double* opt, double* bez,
                      double* lb, double* ub, double* e0, double* eN, double* span, int32_t* qp_active, double* E, double* cost,
                      int32_t* status, double* kkt, int32_t* iters, int32_t* flag, double* target, int32_t* plan_status, void* stream);

/*
 * Obstacle arrays of control.mpccbf for scripted cars, built on the device (used by device-resident race loops):
 * predictions s_o(t + j dt) = v_o (t + j dt) + s0_o, ey_o constant, j = 0..N, from the cars' clock t
 * (NoDynamicsModel.get_trajectory_nsteps, utils/base.py:879-886, quirk Q6); window filter
 * dist_obs - 2 vx < dist_ego < dist_obs + 2 vx on the lap-folded positions and lap offsets
 * (num_cycle_ego - num_cycle_obs) * lap_length (control/control.py:499-523, 538-540); kept cars packed to the
 * front in vehicle order, the rest zero.  Outputs are exactly the obstacle inputs of crx_cbf_solve.
 *   xcurv [batch][6];  car_s0, car_v, car_ey [batch][V];  obs_s, obs_ey [batch][V][N+1];  lap_off [batch][V];  n_obs [batch]
 */
int crx_cbf_prep_dev(int N, int V, double lap_length, double t, double dt, double safety_time, int batch,
                     const double* xcurv, const double* car_s0, const double* car_v, const double* car_ey,
                     double* obs_s, double* obs_ey, double* lap_off, int32_t* n_obs, void* stream);
/* The same with the races of a launch on tracks of their own: race b folded and offset by lap_length[b] ([batch], device). */
int crx_cbf_prep_laps_dev(int N, int V, const double* lap_length, double t, double dt, double safety_time, int batch,
                          const double* xcurv, const double* car_s0, const double* car_v, const double* car_ey,
                          double* obs_s, double* obs_ey, double* lap_off, int32_t* n_obs, void* stream);

/*
 * Field races: the obstacle arrays of control.mpccbf when EVERY car of a race drives itself.  n_races races of C = n_cars cars
 * (1 <= C <= CRX_MAX_OBS + 1, V = C - 1): each car is the ego of its own NLP and an obstacle of the V others, so one call prepares
 * the n_races * C problems of ONE crx_cbf_solve* launch, race-major, car-minor.  One kernel launch, two phases:
 *   predictions   every car by the zero-input roll-out the reference's driven model offers its opponents
 *                 (racing/offboard.py:51-94, DynamicBicycleModel.get_estimation / get_trajectory_nsteps(N + 1)): N + 1 times
 *                   v_long = (vx cos(epsi) - vy sin(epsi)) / (1 - curv ey);  epsi += dt (wz - v_long curv);  s += dt v_long;
 *                   ey += dt (vx sin(epsi) + vy cos(epsi))          (every right-hand side on the old state; vx, vy, wz constant)
 *                 with curv looked up at the old s folded into one lap, and `while s > L: s -= L` after every step (:90-91)
 *   obstacles     per ego, the other cars in car order: window test dist_obs - safety_time vx < dist_ego < dist_obs + safety_time vx on
 *                 the lap-folded positions and lap offset (num_cycle_ego - num_cycle_obs) lap_length, both from column 0 of the
 *                 prediction (control/control.py:499-523, 538-540; int() truncates toward zero); kept cars packed to the front, the rest zero
 *   track [n_seg][6] (the plant's segment table);  xcurv [R][C][6];  car_dims [R][C][2] (length, width of every car) or NULL
 *   pred_s, pred_ey [R][C][N+1]                                                     out: what the reference logs as the prediction
 *   obs_s, obs_ey [R][C][V][N+1];  lap_off [R][C][V];  n_obs [R][C]                 out: the obstacle inputs of crx_cbf_solve*, batch R C
 *   obs_dims [R][C][V][2]    out, non-NULL iff car_dims (with C == 1 it holds nothing and may be NULL either way): kept slot = (l_ego / 2 + l_obs / 2, w_ego / 2 + w_obs / 2) (control.py:532-535),
 *                            slots >= n_obs zero; the obs_dims argument of crx_cbf_solve_dims / crx_cbf_solve_models*
 *   clear [R][C]             out, may be NULL: min over the other cars of (ds / l_sum)^degree + (dey / w_sum)^degree at the CURRENT states,
 *                            ds = (s_ego - s_obs + L / 2) mod L - L / 2 (the sign of L), l_sum, w_sum from car_dims or the descriptor's
 *                            pair; below 1 is contact; +inf when C == 1
 * With C == 1 the obs_* / lap_off arrays hold nothing and may be NULL.  Device-resident car_dims cannot be validated: a non-positive or
 * non-finite length / width counts as the descriptor's l_sum / w_sum; the host-pointer entry refuses such rows.  A car with a
 * non-finite state gets non-finite predictions, is kept by nobody and keeps nobody; it touches no other car.
 * Accuracy: the roll-out is the reference's float64 arithmetic up to the rounding of sin / cos and of fused multiply-adds (1e-12 against
 * the reference's own rows, tests/golden/field_pred.npz) -- wherever the expression is well conditioned.  It divides by 1 - curv ey: a
 * roll-out that drifts towards the centre of a curve (ey -> 1 / curv, off any track) amplifies every rounding error without bound, here
 * as in the reference.
 * Quirks kept:
 *   F1  all cars of a step see the same snapshot, the states at the start of the step.  The reference's off-board simulator steps its
 *       vehicles one after the other (offboard.py:124-127) and its real-time nodes run asynchronously: neither defines a lockstep field.
 *       The snapshot is this library's definition; it is what lets one solver launch serve a whole step.
 *   F2  column 0 of a prediction is one estimated step AHEAD of the current state (offboard.py:83-89); the window test and the lap
 *       offset use that column (control.py:518-519).
 *   F3  the wrap after every step: an opponent that crosses the line inside the horizon jumps by -L in obs_s, and the rows reach the
 *       solver as the reference builds them (together with quirk Q1).
 *   F4  the global half of get_estimation is not computed (its doubled assignment of component 4 included): mpccbf discards it.
 *   F5  obstacles come in car-index order, skipping the ego: the reference's dict order.
 *   F6  s exactly on a segment boundary takes the first matching segment, like the plant; the reference raises there (int() of a
 *       two-element index array).
 *   F7  this is the realtime_flag == True construction of control.mpccbf; with realtime_flag == False the reference calls
 *       get_trajectory_nsteps(time, timestep, n), which its DynamicBicycleModel does not accept.
 */
typedef struct crx_field_desc {
    int32_t N;            /* horizon, 1 .. CRX_MAX_N: N + 1 prediction columns */
    int32_t n_cars;       /* C, 1 .. CRX_MAX_OBS + 1 */
    int32_t n_seg;        /* rows of the track table, 1 .. 64 */
    int32_t degree;       /* 6: exponent of `clear` (2, 4, 6 or 8) */
    double lap_length;
    double dt;            /* 0.1 */
    double safety_time;   /* 2.0 (control.py:499) */
    double l_sum;         /* 0.4: l_ego / 2 + l_obs / 2 where no car_dims are given */
    double w_sum;         /* 0.2 */
} crx_field_desc;
void crx_field_desc_default(crx_field_desc* d, int N, int n_cars, int n_seg, double lap_length);
int crx_field_prep(const crx_field_desc* d, int n_races, const double* track, const double* xcurv, const double* car_dims, double* pred_s,
                   double* pred_ey, double* obs_s, double* obs_ey, double* lap_off, int32_t* n_obs, double* obs_dims, double* clear);
int crx_field_prep_dev(const crx_field_desc* d, int n_races, const double* track, const double* xcurv, const double* car_dims, double* pred_s,
                       double* pred_ey, double* obs_s, double* obs_ey, double* lap_off, int32_t* n_obs, double* obs_dims, double* clear,
                       void* stream);
/*
 * Field races on ONE TRACK PER RACE: a race is on one track and all its cars share it; the races of a launch may be on different tracks.
 * crx_field_prep_tracks[_dev] is crx_field_prep[_dev] with a track set in place of `track`: tracks, n_seg, lap_length as the plant's
 * (crx_plant_step_tracks_dev, same limits) and the id PER RACE, race_track [n_races] (int32).  Race r is rolled out over table
 * race_track[r], and wrapped, folded, windowed, lap-offset and `clear`-ed with lap_length[race_track[r]].  d->n_seg and d->lap_length are
 * not used, but the descriptor must still be a valid one.  The rows of the races that name track t are the bits of crx_field_prep_dev on
 * table t over those races, wherever they stand in the launch.  For the plant the cars' ids are race_track[r] repeated n_cars times.
 * The host-pointer entry reads its arrays and refuses (CRX_ERR_ARG, the first offender in crx_last_error()) a race_track outside
 * [0, n_tracks), an n_seg[t] outside [1, seg_stride] and a lap length that is not positive and finite.  The `_dev` entry cannot read device
 * memory: the id is compared, never used as an address -- every car of a race whose id is outside [0, n_tracks) gets NaN prediction rows,
 * n_obs = 0, zero slots, lap_off = 0 and clear = NaN, and touches no other race; an n_seg[t] is clamped to [0, seg_stride].
 */
int crx_field_prep_tracks(const crx_field_desc* d, int n_races, int n_tracks, int seg_stride, const double* tracks, const int32_t* n_seg,
                          const double* lap_length, const int32_t* race_track, const double* xcurv, const double* car_dims, double* pred_s,
                          double* pred_ey, double* obs_s, double* obs_ey, double* lap_off, int32_t* n_obs, double* obs_dims, double* clear);
int crx_field_prep_tracks_dev(const crx_field_desc* d, int n_races, int n_tracks, int seg_stride, const double* tracks, const int32_t* n_seg,
                              const double* lap_length, const int32_t* race_track, const double* xcurv, const double* car_dims, double* pred_s,
                              double* pred_ey, double* obs_s, double* obs_ey, double* lap_off, int32_t* n_obs, double* obs_dims, double* clear,
                              void* stream);

/*
 * Field games: the traffic arrays of the racing game (LMPCRacingGame.calc_input: learning MPC, overtake planner + tracking NLP when a car
 * is near) when EVERY car of a race plays it.  n_races races of C = n_cars cars (1 <= C <= CRX_MAX_VEH + 1, V = C - 1), race-major and
 * car-minor as in crx_field_prep: each car is the ego of its own scenario and a vehicle of the V others.  One kernel launch, two phases:
 *   predictions   every car by the zero-input roll-out of crx_field_prep (racing/offboard.py:51-94), the same code: the same bits
 *   traffic       per ego, the other cars in car order, skipping the ego (F5): the car's current state and its roll-out rows, copied --
 *                 what OvertakeTrajPlanner.get_local_traj takes of a driven opponent on its `else` branch, get_trajectory_nsteps(N + 1)
 *                 (planning/overtake_traj_planner.py:77-85)
 *   track [n_seg][6];  xcurv [R][C][6]
 *   pred_s_car, pred_ey_car [R][C][N+1]                       out: every car's own roll-out (= pred_s, pred_ey of crx_field_prep)
 *   veh_xcurv [R C][V][6];  pred_s, pred_ey [R C][V][N+1]     out: slot v of ego c is car v + (v >= c) of its race
 *   n_all [R C]                                               out: V
 * The outputs are the veh_xcurv, pred_s, pred_ey, n_all inputs of crx_planner_scene_dev for n_scen = R C, n_all_max = n_veh_max = V
 * (V <= CRX_MAX_VEH: the scene never overflows), where crx_game_traffic_dev supplies them for scripted cars.  With C == 1 the per-ego
 * arrays hold nothing and may be NULL, and n_all is 0.  The descriptor is crx_field_prep's, validated as there; safety_time, degree,
 * l_sum and w_sum are not read.
 * Quirks kept (F1-F3, F6 as in crx_field_prep):
 *   F1  snapshot: all cars see the states at the start of the step; the reference steps its vehicles one after the other.
 *   F2  column 0 of a prediction is one estimated step AHEAD of the current state.
 *   F3  the prediction is wrapped after every roll-out step: an opponent that crosses the line inside the horizon jumps by -L, where the
 *       scripted cars of crx_game_traffic_dev are unwrapped (Q6).  The rows reach the planner and the tracking prep as the reference
 *       builds them.
 *   F6  s exactly on a segment boundary takes the first matching segment, like the plant.
 *   G1  every car is "ego" in its own problem, although the reference's helpers hard-code vehicles["ego"] (planner_helper.py:185).
 *   G2  the tracking NLP behind the planner consumes the same roll-out rows through the scene and crx_track_prep_dev.
 *       control.mpc_multi_agents hard-codes realtime_flag = False (control.py:288-298) and its call form there,
 *       get_trajectory_nsteps(time, timestep, n), is one the driven model does not accept; the roll-out is the realtime_flag == True form
 *       of the same lines.
 *   G3  a car with a non-finite state has non-finite rows.  check_ego_agent_distance is all comparisons, so nobody counts it as a vehicle
 *       of interest, and it touches no other car's outputs.
 */
int crx_field_traffic(const crx_field_desc* d, int n_races, const double* track, const double* xcurv, double* pred_s_car, double* pred_ey_car,
                      double* veh_xcurv, double* pred_s, double* pred_ey, int32_t* n_all);
int crx_field_traffic_dev(const crx_field_desc* d, int n_races, const double* track, const double* xcurv, double* pred_s_car,
                          double* pred_ey_car, double* veh_xcurv, double* pred_s, double* pred_ey, int32_t* n_all, void* stream);

/*
 * Mixed fields: every car of a race under its OWN controller, as the reference's simulator holds them (CarRacingSim.add_vehicle,
 * ModelBase.set_ctrl_policy with PIDTracking / LQRTracking / MPCTracking / iLQRRacing / MPCCBFRacing, racing/offboard.py:14-45; sim()
 * steps all of them together, :114-131).  policy [R][C], int32, one code per car:
 */
#define CRX_POLICY_NONE 0     /* applies zero input: a car that coasts */
#define CRX_POLICY_PID 1      /* control.pid (control/control.py:15-25) */
#define CRX_POLICY_LQR 2      /* control.lqr: u = -K (x - xt) */
#define CRX_POLICY_MPC_LTI 3  /* control.mpc_lti: the MPC-CBF NLP with its obstacle count forced to 0 (MPCTrackingParam and MPCCBFRacingParam share Q and R) */
#define CRX_POLICY_MPCCBF 4   /* control.mpccbf */
#define CRX_POLICY_ILQR 5     /* control.ilqr */
#define CRX_POLICY_COUNT 6
/*
 * crx_mixed_prep[_dev]: ONE launch for n_races races of C = n_cars cars (race-major, car-minor, as in crx_field_prep) that serves every
 * policy of the step: the roll-out of every car, the obstacle arrays of one crx_cbf_solve* launch over all R C cars (mask m_nlp) and
 * those of one crx_ilqr_solve* launch over all R C cars (mask m_ilqr).  V = C - 1, NP = max(N, N_ilqr).
 *   track [n_seg][6];  xcurv [R][C][6];  policy [R][C];  car_dims [R][C][2] or NULL
 *   pred_s, pred_ey [R][C][NP+1]     out: every car's zero-input roll-out, whatever its policy; columns 0 .. N are pred_s, pred_ey of
 *                                    crx_field_prep (the same function, run further)
 *   the NLP family      obs_s, obs_ey [R C][V][N+1];  lap_off [R C][V];  n_obs [R C];  obs_dims [R C][V][2] iff car_dims;  m_nlp [R C]
 *                       An MPCCBF car gets exactly crx_field_prep's arrays (window test, lap offset, packing: F1-F7).  Every other
 *                       car gets n_obs = 0 and zero slots.  m_nlp = 1 for MPC_LTI and MPCCBF cars, else 0.
 *   the iLQR family     (N_ilqr > 0; with N_ilqr == 0 all five may be NULL and none is written)
 *                       il_obs_s, il_obs_ey [R C][V][N_ilqr+1];  il_lap_off [R C][V];  il_n_obs [R C];  m_ilqr [R C]
 *                       An ILQR car gets the other cars of its race in car order with NO distance window (control.ilqr applies
 *                       none), columns 0 .. N_ilqr of their roll-outs, lap_off = (trunc(s_ego / L) - trunc(pred_s[o][0] / L)) L (I5),
 *                       packed to the front: all of them with ilqr_obstacles = 1, the LAST other car in car order alone with
 *                       ilqr_obstacles = 0 (quirk I1).  A car whose state has a non-finite component is kept by nobody -- with
 *                       ilqr_obstacles = 0, a non-finite last other car leaves il_n_obs = 0 -- and an ILQR car with such a state keeps
 *                       nobody.  Every other car gets il_n_obs = 0 and zero slots.  m_ilqr = 1 for ILQR cars, else 0.
 *   clear [R C]         out, may be NULL: as crx_field_prep's
 * With C == 1 the [V] arrays hold nothing and may be NULL.  A policy code outside 0 .. CRX_POLICY_COUNT - 1 counts as CRX_POLICY_NONE;
 * device-resident codes cannot be validated on the host (the host-pointer entry refuses them), they are compared and index nothing.
 * Quirks kept:
 *   F1-F3, F6  as in crx_field_prep: snapshot, column 0 one step ahead, the wrap after every roll-out step, the first matching segment.
 *   M1  the roll-out handed to iLQR is the realtime_flag == True form.  control.ilqr calls get_trajectory_nsteps(time, timestep, n)
 *       (control.py:99-104), which the driven model does not accept: the situation of G2.
 *   M2  iLQR has ONE l_sum / w_sum per launch, its descriptor's (I1: the reference takes them from "car1"); car_dims feeds the NLP
 *       family and `clear` only.
 */
typedef struct crx_mixed_desc {
    int32_t N;               /* horizon of the NLP family, 1 .. CRX_MAX_N */
    int32_t N_ilqr;          /* horizon of the iLQR family, 0 .. CRX_ILQR_MAX_N; 0: no iLQR arrays */
    int32_t n_cars;          /* C, 1 .. CRX_MAX_OBS + 1 */
    int32_t n_seg;           /* rows of the track table, 1 .. 64 */
    int32_t degree;          /* 6: exponent of `clear` (2, 4, 6 or 8) */
    int32_t ilqr_obstacles;  /* 0: quirk I1, the last other car in car order only (control.py:99-104); 1: all others */
    double lap_length;
    double dt;               /* 0.1 */
    double safety_time;      /* 2.0 (control.py:499) */
    double l_sum;            /* 0.4 */
    double w_sum;            /* 0.2 */
} crx_mixed_desc;
void crx_mixed_desc_default(crx_mixed_desc* d, int N, int N_ilqr, int n_cars, int n_seg, double lap_length);
int crx_mixed_prep(const crx_mixed_desc* d, int n_races, const double* track, const double* xcurv, const int32_t* policy, const double* car_dims,
                   double* pred_s, double* pred_ey, double* obs_s, double* obs_ey, double* lap_off, int32_t* n_obs, double* obs_dims,
                   int32_t* m_nlp, double* il_obs_s, double* il_obs_ey, double* il_lap_off, int32_t* il_n_obs, int32_t* m_ilqr, double* clear);
int crx_mixed_prep_dev(const crx_mixed_desc* d, int n_races, const double* track, const double* xcurv, const int32_t* policy,
                       const double* car_dims, double* pred_s, double* pred_ey, double* obs_s, double* obs_ey, double* lap_off, int32_t* n_obs,
                       double* obs_dims, int32_t* m_nlp, double* il_obs_s, double* il_obs_ey, double* il_lap_off, int32_t* il_n_obs,
                       int32_t* m_ilqr, double* clear, void* stream);
/*
 * Mixed fields on one track per race: crx_mixed_prep[_dev] with the track set and race_track [n_races] of crx_field_prep_tracks[_dev], same
 * rules; the iLQR family's il_lap_off (quirk I5) is computed with the race's own lap length too.  A race whose id is outside [0, n_tracks)
 * (`_dev` entry) gets, besides the rows stated there, m_nlp = m_ilqr = 0, il_n_obs = 0, il_lap_off = 0 and zero iLQR slots: no solver runs
 * for it.
 */
int crx_mixed_prep_tracks(const crx_mixed_desc* d, int n_races, int n_tracks, int seg_stride, const double* tracks, const int32_t* n_seg,
                          const double* lap_length, const int32_t* race_track, const double* xcurv, const int32_t* policy, const double* car_dims,
                          double* pred_s, double* pred_ey, double* obs_s, double* obs_ey, double* lap_off, int32_t* n_obs, double* obs_dims,
                          int32_t* m_nlp, double* il_obs_s, double* il_obs_ey, double* il_lap_off, int32_t* il_n_obs, int32_t* m_ilqr,
                          double* clear);
int crx_mixed_prep_tracks_dev(const crx_mixed_desc* d, int n_races, int n_tracks, int seg_stride, const double* tracks, const int32_t* n_seg,
                              const double* lap_length, const int32_t* race_track, const double* xcurv, const int32_t* policy,
                              const double* car_dims, double* pred_s, double* pred_ey, double* obs_s, double* obs_ey, double* lap_off,
                              int32_t* n_obs, double* obs_dims, int32_t* m_nlp, double* il_obs_s, double* il_obs_ey, double* il_lap_off,
                              int32_t* il_n_obs, int32_t* m_ilqr, double* clear, void* stream);
/*
 * crx_mixed_commit_dev: after the solver launches, before the plant: u [batch][2] and ctrl_status [batch] from each car's own law, every
 * operation rounded on its own (no fused multiply-add).  x [batch][6] is the state the step starts from.
 *   PID               u = (-0.6 (x[5] - eyt) - 0.9 x[3], 1.5 (vt - x[0])), vt, eyt [batch]: crx_seed_commit_dev's law      CRX_CONVERGED
 *   LQR               u = -K (x - xt), K [batch][2][6], xt [batch][6]; the sum runs c = 0 .. 5 as crx_lqr_step_dev's      CRX_CONVERGED
 *   MPC_LTI, MPCCBF   U_nlp[b * nlp_stride + 0, 1]: stage 0 of the plan (nlp_stride = 2 N for a solver's U)                 nlp_status[b]
 *   ILQR              U_ilqr[b * ilqr_stride + 0, 1]                                                                        ilqr_status[b]
 *   NONE              zero                                                                                                  CRX_SKIPPED
 * The last iterate of a failed solve is applied, as control.py:600-603 does.  A policy code out of range applies zero and reports
 * CRX_SKIPPED.  Each family's pair of arrays -- (vt, eyt), (K, xt), (U_nlp, nlp_status), (U_ilqr, ilqr_status) -- may be NULL, both or
 * neither: a car whose family is NULL applies zero and reports CRX_SKIPPED.  Strides of given families are >= 2.
 */
int crx_mixed_commit_dev(int batch, const int32_t* policy, const double* x, const double* vt, const double* eyt, const double* K,
                         const double* xt, const double* U_nlp, int nlp_stride, const int32_t* nlp_status, const double* U_ilqr,
                         int ilqr_stride, const int32_t* ilqr_status, double* u, int32_t* ctrl_status, void* stream);

/*
 * Inputs of control.mpc_multi_agents' NLP (crx_cbf_solve with per_stage_target = 1) from the planner's outputs, on the device
 * (device-resident race loops): per-stage targets xt_i = [vx_0, 0, 0, 0, 0, f_traj(clip(s_0 + dt_ref i vx_0))] from the
 * selected trajectory (control/control.py:373-382; f_traj = linear interpolation of its (s, ey) samples) and the obstacle
 * arrays: the sorted vehicles' predictions filtered by the +-safety_time*vx window on the lap-folded positions, lap
 * offsets, kept vehicles packed to the front (control.py:293-309, 311-319).  Horizon of the controller = horizon of the
 * planner here (the reference's defaults: 10 and 10).
 *   x [batch][6];  n_veh [batch];  obs_s_in, obs_ey_in [batch][V][N+1] (crx_planner_scene order);  traj [batch][N+1][6] (best_X)
 *   xt [batch][N+1][6];  obs_s, obs_ey [batch][V][N+1];  lap_off [batch][V];  n_obs [batch]
 */
int crx_track_prep_dev(int N, int V, double lap_length, double safety_time, double dt_ref, int batch, const double* x,
                       const int32_t* n_veh, const double* obs_s_in, const double* obs_ey_in, const double* traj, double* xt,
                       double* obs_s, double* obs_ey, double* lap_off, int32_t* n_obs, void* stream);

/*
 * Learning-MPC QPs: control.lmpc (control.py:610-730) after its safe-set
 * selection (:625-639), one problem per batch entry.  LTV affine model x_{i+1} = A_i x_i + B_i u_i + C_i
 * as estimated by the caller (utils/base.py:585-622).
 *   x0 [batch][6], u_old [batch][2]; A [batch][N][36], B [batch][N][12], C [batch][N][6] (row-major);
 *   ss [batch][6][n_ss_max] (columns = safe-set points, :636-638), qfun [batch][n_ss_max], n_ss [batch] in
 *   [1, n_ss_max].
 *   X [batch][N+1][6], U [batch][N][2], lambda [batch][n_ss_max], cost [batch] (the reference's cost :698).
 * status: CRX_CONVERGED = KKT point of the reference's QP (terminal state inside the safe-set hull).
 *   The reference pins its terminal slack to zero (:694-695), so its QP is infeasible whenever the
 *   regression model cannot reach the hull from xcurv; the reference then applies IPOPT's restoration
 *   state (:711-722), which is solver-internal: a least-violation point of ALL equalities of the
 *   full-space problem.  On the recorded infeasible instances the cheapest such violation is a ~1e-2
 *   shift of the initial-state equality (:650).  libcrx therefore repeats a failed problem with that
 *   equality relaxed, x_0 = xcurv + w, cost += w_x0 * w'w, terminal constraint kept; X is the plan from
 *   xcurv + w, U its inputs, status CRX_INFEASIBLE when the first attempt ended by a PROOF (a bound the fixed x_0 violates,
 *   the terminal-set reachability screen, the Farkas certificate over input box x unit simplex) and CRX_STALLED when it ended
 *   without one (multiplier divergence, iteration cap, stagnation on the noise floor, no acceptable step) [0.3.0; <= 0.2.1
 *   reported both as CRX_INFEASIBLE].  A relaxed attempt that does not converge either keeps its own status (1 / 5).
 */
int crx_lmpc_solve(const crx_lmpc_desc* d, int batch, const double* x0, const double* u_old, const double* A,
                   const double* B, const double* C, const double* ss, const double* qfun, const int32_t* n_ss,
                   double* X, double* U, double* lambda, double* cost, int32_t* status, double* kkt,
                   int32_t* iters);
int crx_lmpc_solve_dev(const crx_lmpc_desc* d, int batch, const double* x0, const double* u_old, const double* A,
                       const double* B, const double* C, const double* ss, const double* qfun,
                       const int32_t* n_ss, double* X, double* U, double* lambda, double* cost,
                       int32_t* status, double* kkt, int32_t* iters, void* stream);
/* masked launch: see crx_cbf_solve_masked_dev */
int crx_lmpc_solve_masked_dev(const crx_lmpc_desc* d, int batch, const int32_t* active, const double* x0, const double* u_old,
                              const double* A, const double* B, const double* C, const double* ss, const double* qfun,
                              const int32_t* n_ss, double* X, double* U, double* lambda, double* cost, int32_t* status,
                              double* kkt, int32_t* iters, void* stream);

/*
 * Host work in front of the learning-MPC QP, on the device (second half): per race, the
 * N local LTV stage models of LMPCRacingGame.estimate_ABC (utils/base.py:585-622 -> control/lmpc_helper.py:26-189:
 * kernel-weighted least squares for the vx / vy / wz rows from the two previous laps, analytic Jacobian of the Euler
 * step for the epsi / s / ey rows) and the safe-set points and cost-to-go control.lmpc selects (control.py:625-639 ->
 * lmpc_helper.py:278-293).  Outputs are exactly the A, B, C, ss, qfun inputs of crx_lmpc_solve.
 *   ss_xcurv [batch][n_laps][n_points][6], u_ss [batch][n_laps][n_points][2], qfun [batch][n_laps][n_points]
 *            the sampled safe set (LMPCRacingGame.ss_xcurv / u_ss / Qfun, stored lap-major here)
 *   time_ss  [batch][n_laps]   samples per stored lap;  iter [batch]   index of the running lap (>= 2)
 *   x        [batch][6]        current state (start-line wrapped, as LMPCRacingGame.calc_input passes it)
 *   lin_points [batch][N+1][6], lin_input [batch][N][2]   linearisation points; with from_plan != 0 they are the X and U
 *            of the previous crx_lmpc_solve and are shifted by one stage here (control.py:726-728)
 *   track    [n_seg][6]        rows (x, y, psi, s_start, length, curvature)
 *   A [batch][N][36], B [batch][N][12], C [batch][N][6];  ss_sel [batch][6][M], q_sel [batch][M], M = n_ss_laps * n_ss_per_lap
 *   status   [batch]           0, or 1 if a stage's normal matrix was singular (no stored sample near its linearisation
 *                              point; the reference's cvxopt raises there).  The three regression rows of such a stage are
 *                              left UNTOUCHED in A, B, C: a device-resident loop that reuses its buffers keeps the previous
 *                              step's model of the stage.
 * The reference's normal equations reach condition numbers of 3e11: coefficients agree with the reference's to ~1e-5
 * relative only (any two LAPACK routes differ that much); what the models predict at their own query points agrees tightly.
 */
typedef struct crx_lmpcprep_desc {
    int32_t N;              /* 12   LMPCRacingParam.num_horizon */
    int32_t n_points;       /* rows per lap in the safe-set arrays */
    int32_t n_laps;         /* laps per race in the safe-set arrays */
    int32_t n_ss_per_lap;   /* 22   num_ss_points / num_ss_iter (control.py:627-632) */
    int32_t n_ss_laps;      /* 2    num_ss_iter */
    int32_t max_neighbours; /* 40   utils/base.py:605 */
    int32_t n_seg;          /* rows of the track table */
    int32_t shift;          /* 0    LMPCRacingParam.shift */
    double bandwidth;       /* 5.0  lmpc_helper.py:42 */
    double scale[5];        /* 0.1, 1, 1, 1, 1   feature scaling of the distance (:49-57) */
    double dt;              /* control period */
    double lap_length;
} crx_lmpcprep_desc;
void crx_lmpcprep_desc_default(crx_lmpcprep_desc* d, int N, int n_points, int n_laps, int n_seg, double dt, double lap_length);
int crx_lmpc_prep(const crx_lmpcprep_desc* d, int batch, const double* ss_xcurv, const double* u_ss, const double* qfun,
                  const int32_t* time_ss, const int32_t* iter, const double* x, const double* lin_points,
                  const double* lin_input, int from_plan, const double* track, double* A, double* B, double* C,
                  double* ss_sel, double* q_sel, int32_t* status);
int crx_lmpc_prep_dev(const crx_lmpcprep_desc* d, int batch, const double* ss_xcurv, const double* u_ss, const double* qfun,
                      const int32_t* time_ss, const int32_t* iter, const double* x, const double* lin_points,
                      const double* lin_input, int from_plan, const double* track, double* A, double* B, double* C,
                      double* ss_sel, double* q_sel, int32_t* status, void* stream);
/* masked launch: see crx_cbf_solve_masked_dev (status[b] = CRX_SKIPPED for the races left alone) */
int crx_lmpc_prep_masked_dev(const crx_lmpcprep_desc* d, int batch, const int32_t* active, const double* ss_xcurv, const double* u_ss,
                             const double* qfun, const int32_t* time_ss, const int32_t* iter, const double* x, const double* lin_points,
                             const double* lin_input, int from_plan, const double* track, double* A, double* B, double* C,
                             double* ss_sel, double* q_sel, int32_t* status, void* stream);
/* LMPCRacingGame.add_point (utils/base.py:624-629): the running lap extends the previous lap's safe set past the finish
 * line -- row time_ss[iter-1] + step + 1 of lap iter-1 becomes x + (0,0,0,0,lap_length,0) / u.  Device-resident race loops. */
int crx_lmpc_addpoint_dev(const crx_lmpcprep_desc* d, int batch, double* ss_xcurv, double* u_ss, const int32_t* time_ss,
                          const int32_t* iter, const int32_t* step, const double* x, const double* u, int u_stride,
                          void* stream);
/* LMPCRacingGame.add_trajectory (utils/base.py:631-656), for the races of a device-resident loop that have just crossed the
 * finish line (crossed[b] != 0; the others are left alone): the running lap, logged as the simulator logs it
 * (update_memory, base.py:795-819: log_x [batch][n_points][6] with n_log[b] states, the last one the crossing state with
 * s > lap_length; log_u [batch][n_points][2] with n_log[b] - 1 inputs), becomes lap iter[b] of the race's safe set --
 * states, inputs, time_ss = n_log - 1, Qfun = compute_cost (lmpc_helper.py:11-23) + the reference's count-down pass over
 * the whole column (:647-649) -- then iter[b] += 1, step[b] = 0 (time_in_iter), and the log restarts with x[b] (the wrapped
 * state the new lap starts from), n_log[b] = 1.  status[b] = 1: the race's safe set is full (iter == n_laps), nothing stored. */
int crx_lmpc_addtraj_dev(const crx_lmpcprep_desc* d, int batch, const int32_t* crossed, double* log_x, const double* log_u,
                         int32_t* n_log, double* ss_xcurv, double* u_ss, double* qfun, int32_t* time_ss, int32_t* iter,
                         int32_t* step, const double* x, int32_t* status, void* stream);

/*
 * MPC-CBF NLPs.
 *   x0      [batch][6]
 *   xt      [batch][6] or [batch][N+1][6]   tracking target(s) (d->per_stage_target)
 *   obs_s   [batch][n_obs_max][N+1]         obstacle prediction rows 4 of obs_traj
 *   obs_ey  [batch][n_obs_max][N+1]         rows 5
 *   lap_off [batch][n_obs_max]              (num_cycle_ego - num_cycle_obs) * lap_length; applied
 *                                           to h_i only, not to h_{i+1} (quirk Q1, control.py:539-542)
 *   n_obs   [batch]                         obstacles inside the +-2*vx window (control.py:520-523)
 *   X [batch][N+1][6], U [batch][N][2], sigma [batch][n_obs_max][N+1] (cbf_slack), cost, status,
 *   kkt, iters as above.  No fall-back: the last iterate is returned (control.py:600-603).
 */
int crx_cbf_solve(const crx_cbf_desc* d, int batch, const double* x0, const double* xt,
                  const double* obs_s, const double* obs_ey, const double* lap_off,
                  const int32_t* n_obs, double* X, double* U, double* sigma, double* cost,
                  int32_t* status, double* kkt, int32_t* iters);
int crx_cbf_solve_dev(const crx_cbf_desc* d, int batch, const double* x0, const double* xt,
                      const double* obs_s, const double* obs_ey, const double* lap_off,
                      const int32_t* n_obs, double* X, double* U, double* sigma, double* cost,
                      int32_t* status, double* kkt, int32_t* iters, void* stream);
/* Per-obstacle dimensions.  The reference takes (l_obs, w_obs) from every obstacle vehicle's own CarParam (control.py:529-535);
 * crx_cbf_desc carries ONE pair (l_sum, w_sum) for the common case of identical cars.  obs_dims [batch][n_obs_max][2] =
 * (l_agent + l_obs, w_agent + w_obs) of every obstacle slot of every problem overrides it (slots >= n_obs[b] are not read);
 * NULL = the descriptor's pair for all.  `active` as in the masked launch below (NULL: all).  Precondition: positive, finite
 * entries -- the host-pointer entry point checks and fails the call; the *_dev variants cannot (device memory) and let a
 * non-positive or non-finite entry fall back to the descriptor's pair. */
int crx_cbf_solve_dims(const crx_cbf_desc* d, int batch, const double* x0, const double* xt, const double* obs_s,
                       const double* obs_ey, const double* lap_off, const int32_t* n_obs, const double* obs_dims, double* X,
                       double* U, double* sigma, double* cost, int32_t* status, double* kkt, int32_t* iters);
int crx_cbf_solve_dims_dev(const crx_cbf_desc* d, int batch, const int32_t* active, const double* x0, const double* xt,
                           const double* obs_s, const double* obs_ey, const double* lap_off, const int32_t* n_obs,
                           const double* obs_dims, double* X, double* U, double* sigma, double* cost, int32_t* status, double* kkt,
                           int32_t* iters, void* stream);
/* Dispatch order.  The workgroups of a launch start in launch order and a launch ends with its slowest problem: when the problems
 * that need many iterations are listed first -- a closed loop knows them: the iteration counts of the previous control step -- the
 * launch no longer waits for a straggler that started last (BASELINE configs[3], 16384 NLPs of 8..166 iterations on 1024 resident
 * slots: list scheduling in index order 398 iteration-units, longest first 338).  order [batch] int32 on the device = a permutation of
 * 0..batch-1: workgroup i solves problem order[i]; results land at the problem's own index; NULL = index order.  Entries are
 * clamped to [0, batch); a non-permutation solves some problems twice and others not at all (the caller's business).
 * crx_cbf_solve_ordered_dev is the superset entry point (mask, order, per-obstacle dimensions; each may be NULL). */
int crx_cbf_solve_ordered_dev(const crx_cbf_desc* d, int batch, const int32_t* active, const int32_t* order, const double* x0,
                              const double* xt, const double* obs_s, const double* obs_ey, const double* lap_off,
                              const int32_t* n_obs, const double* obs_dims, double* X, double* U, double* sigma, double* cost,
                              int32_t* status, double* kkt, int32_t* iters, void* stream);
/* One LTI model per problem (a fleet of identified cars: crx_sysid_fit leaves model_A [batch][6][6], model_B [batch][6][2] on the device).
 * Problem b is solved with ITS model; d->A, d->B are not read.  Besides the model the solver needs how far the boxed inputs can move s and ey
 * of every stage (what it computes on the host for the descriptor's model): model_reach, CRX_CBF_MODEL_REACH_DOUBLES(batch) doubles owned by
 * the caller, filled by crx_cbf_models_reach_dev.  The table depends on the models and on d's N, delta_max, a_max only: a closed loop
 * computes it once.  For copies of d's model it equals the descriptor's table bit for bit.  The solve then equals the shared launch bit for
 * bit wherever both run the same instantiation class: tuned kernels exist with models for zero or one obstacle slot at N = 10 / 12 and
 * three slots at N = 20 (exponent 6); every other shape runs the general (run-time horizon / exponent) kernels with models, also where
 * the shared launch has a tuned one (two slots at N = 10 / 12 / 20, zero or one at N = 20, three at N = 10 / 12, other horizons of a
 * custom CRX_NFIX_LIST): the same iteration through another instantiation, same KKT point to solver tolerance, at the general
 * kernels' speed (1.5 .. 2x slower than tuned ones).
 *   crx_cbf_solve_models_dev   = crx_cbf_solve_ordered_dev + (model_A, model_B, model_reach) after x0.  All three NULL: the shared launch;
 *                                any other mix of NULLs is CRX_ERR_ARG.  Every (N, n_obs_max, degree, per_stage_target) of the shared launch.
 *   crx_cbf_solve_models       host pointers (model_A, model_B both or neither); stages them and computes the table itself.
 * A problem whose model has a non-finite entry (a failed fit) is not iterated: status CRX_SINGULAR, iters 0, kkt inf, X / U / sigma / cost NaN
 * -- on both paths; it is not an argument error.  The planner region QP takes per-problem models through crx_planner_solve_models* /
 * crx_planner_plan_models*; the two-wave diagnostics kernel stays single-model. */
#define CRX_CBF_MODEL_REACH_DOUBLES(batch) ((size_t)(batch) * 2 * (CRX_MAX_N + 1))
int crx_cbf_models_reach_dev(const crx_cbf_desc* d, int batch, const double* model_A, const double* model_B, double* model_reach, void* stream);
int crx_cbf_solve_models_dev(const crx_cbf_desc* d, int batch, const int32_t* active, const int32_t* order, const double* x0,
                             const double* model_A, const double* model_B, const double* model_reach, const double* xt,
                             const double* obs_s, const double* obs_ey, const double* lap_off, const int32_t* n_obs,
                             const double* obs_dims, double* X, double* U, double* sigma, double* cost, int32_t* status, double* kkt,
                             int32_t* iters, void* stream);
int crx_cbf_solve_models(const crx_cbf_desc* d, int batch, const double* x0, const double* model_A, const double* model_B, const double* xt,
                         const double* obs_s, const double* obs_ey, const double* lap_off, const int32_t* n_obs, const double* obs_dims,
                         double* X, double* U, double* sigma, double* cost, int32_t* status, double* kkt, int32_t* iters);
/* The order itself, computed on the device (one launch, a stable counting sort; equal keys keep index order):
 *   crx_order_longest_first_dev  from the iteration counts of the previous solve of these problems (iters [batch], e.g. the iters
 *                                output of the previous control step), longest first;
 *   crx_cbf_order_dev            with no previous solve, from the problem's own inputs (the arrays of crx_cbf_solve_dev): the
 *                                barrier h = (ds/l)^degree + (dey/w)^degree - 1 - margin (control.py:529-537) of the START state
 *                                and of the un-steered PATH (s_0 + j A[4][0] vx_0 along the target ey).  First the cars that start
 *                                inside a safety ellipse (deepest first: the NLPs that need the restoration phase), then those
 *                                whose path enters one, then the rest, nearest first.
 * Problems with active[b] == 0 go last (active may be NULL).  Measured on BASELINE configs[3] (16384 NLPs, one launch): DESIGN.md
 * section 5.6. */
int crx_order_longest_first_dev(int batch, const int32_t* iters, const int32_t* active, int32_t* order, void* stream);
int crx_cbf_order_dev(const crx_cbf_desc* d, int batch, const int32_t* active, const double* x0, const double* xt,
                      const double* obs_s, const double* obs_ey, const double* lap_off, const int32_t* n_obs, const double* obs_dims,
                      int32_t* order, void* stream);
int crx_lmpc_solve_ordered_dev(const crx_lmpc_desc* d, int batch, const int32_t* active, const int32_t* order, const double* x0,
                               const double* u_old, const double* A, const double* B, const double* C, const double* ss,
                               const double* qfun, const int32_t* n_ss, double* X, double* U, double* lambda, double* cost,
                               int32_t* status, double* kkt, int32_t* iters, void* stream);
/* Masked launches (device-resident loops in which every problem of the batch takes ONE of several branches per step, e.g.
 * LMPCRacingGame.calc_input, utils/base.py:456-583: overtake planner + tracking NLP, or learning-MPC): active [batch]
 * int32 on the device, 0 = this problem is not part of the launch -- its wavefront returns at once, status[b] =
 * CRX_SKIPPED, iters[b] = 0, every other output of problem b keeps its previous contents.  active == NULL: all. */
int crx_cbf_solve_masked_dev(const crx_cbf_desc* d, int batch, const int32_t* active, const double* x0, const double* xt,
                             const double* obs_s, const double* obs_ey, const double* lap_off, const int32_t* n_obs, double* X,
                             double* U, double* sigma, double* cost, int32_t* status, double* kkt, int32_t* iters, void* stream);

/*
 * Device-resident racing-game loop: the bookkeeping of LMPCRacingGame.calc_input (utils/base.py:456-583)
 * and of the simulator between the solver launches, so that a control step of B races is a fixed sequence of libcrx launches with
 * nothing returning to the host (crx.montecarlo.GameLaps: traffic -> scene -> masks -> prep -> plan -> track prep -> tracking NLP |
 * regression -> learning-MPC QP -> commit -> add_point -> plant -> log -> add_trajectory).
 *   crx_game_traffic_dev  scripted cars s(t) = v t + s0, ey(t) = ey (NoDynamicsModel, base.py:847-890) at their clock t: states
 *                         veh_xcurv [B][n_cars][6] (s wrapped once past the line like update_memory keeps it) and predictions
 *                         pred_s, pred_ey [B][n_cars][N+1] at t + j dt (unwrapped: quirk Q6) -- the inputs of crx_planner_scene_dev
 *   crx_game_masks_dev    m_overtake = (n_veh > 0), m_lmpc = 1 - m_overtake: the `active` masks of the masked launches; with
 *                         overflow / overflow_seen (both may be NULL) the scene stage's dropped-vehicle counts are accumulated
 *                         per race, so that a sweep can report whether the n_veh_max slots ever were too few
 *   crx_game_commit_dev   after the solves, per race from the branch it is in (overtake == NULL: every race drives by learning MPC):
 *                         u [B][2] the input to apply (u_0 of the tracking NLP U_track [B][Np][2] or of the learning-MPC QP
 *                         U_lmpc [B][N][2]); u_prev <- u_old; learning-MPC branch only: u_old <- u_0, lin_points [B][N+1][6] /
 *                         lin_input [B][N][2] <- the plan X_lmpc / U_lmpc shifted by one stage, last stage repeated
 *                         (control.py:726-728), step_no += 1; addpoint_step = the step index crx_lmpc_addpoint_dev takes (negative in
 *                         the overtake branch: no point is added, utils/base.py:546-551); old_flag <- flag or -1 (may be NULL)
 *   crx_game_log_dev      after the plant: crossed [B] = lap counter advanced; the new state (s unwrapped if it crossed) and the
 *                         applied input appended to the race's lap log log_x [B][n_points][6], log_u [B][n_points][2], n_log += 1
 *                         (ModelBase.update_memory) -- the inputs of crx_lmpc_addtraj_dev
 * A race keeps n_laps laps of safe set (crx_lmpcprep_desc.n_laps); when they are full crx_lmpc_addtraj_dev reports status 1 and the
 * race goes on racing on its last two laps (the reference allocates for the number of laps it is asked to run, utils/base.py:631-656).
 */
int crx_game_traffic_dev(int N, int batch, int n_cars, double lap_length, double t, double dt, const double* car_s0,
                         const double* car_v, const double* car_ey, double* veh_xcurv, double* pred_s, double* pred_ey,
                         void* stream);
int crx_game_masks_dev(int batch, const int32_t* n_veh, const int32_t* overflow, int32_t* m_overtake, int32_t* m_lmpc,
                       int32_t* overflow_seen, void* stream);
int crx_game_commit_dev(int N, int Np, int batch, const int32_t* overtake, const double* U_track, const double* X_lmpc,
                        const double* U_lmpc, const int32_t* flag, double* u, double* u_old, double* u_prev, double* lin_points,
                        double* lin_input, int32_t* step_no, int32_t* addpoint_step, int32_t* old_flag, void* stream);
int crx_game_log_dev(int batch, int n_points, double lap_length, const double* xcurv, const double* u, const int32_t* laps,
                     int32_t* laps_prev, double* log_x, double* log_u, int32_t* n_log, int32_t* crossed, void* stream);

/*
 * Seed laps (crx.montecarlo.SeedLaps): the two laps in front of the learning MPC, per car.  The reference's racing game drives lap 0
 * under PID and lap 1 under MPC-LTI and hands both to LMPCRacingGame.add_trajectory before the first learning-MPC lap
 * (tests/auto_racing_game_test.py:48-73); the learning MPC's stage models, terminal set and cost-to-go are those two laps.  Here every
 * car of a batch does that with ITS plant parameters and ITS controller model, so that a fleet of different cars learns from its own
 * data.  One control step is crx_cbf_solve[_models]_dev with zero obstacle slots (= control.mpc_lti) under active = m_mpc ->
 * crx_seed_commit_dev -> crx_plant_step_wrap_dev -> crx_seed_log_dev -> crx_lmpc_addtraj_dev(crossed, ...), the last one unchanged: lap 0
 * becomes safe-set lap 0 (iter 0 -> 1), lap 1 becomes lap 1 (iter -> 2), and it restarts the log from the wrapped state.
 *
 * Per-car state, [batch] int32 each, owned by the caller: phase (0 = PID lap, 1 = MPC-LTI lap, 2 = seeded, 3 = failed; start: 0),
 * seed_status (bit flags CRX_SEED_*; start: 0), m_mpc (the `active` mask of the NEXT solver launch; start: 0).  Thread b touches car b's
 * elements only; the cars finish at different steps and do not wait for each other.
 *
 * crx_seed_commit_dev, after the solver launch and before the plant, writes u [batch][2] from x [batch][6], the state the step starts from:
 *   S1  phase 0: u = control.pid (control/control.py:15-25): u0 = -0.6 * (ey - eyt) - 0.9 * epsi, u1 = 1.5 * (vt - vx), with vt, eyt [batch]
 *       per car, every operation rounded on its own as NumPy does (crx_pid_log_dev states the same law but is compiled with
 *       contraction and can differ from this by an ulp; it is left as it is, for its bits).
 *   S2  phase 1: u = U_mpc[b][0] (U_mpc [batch][N][2], the solver's plan).  mpc_status[b] != CRX_CONVERGED sets seed_status |=
 *       CRX_SEED_MPC_FAILED: the reference has no handler there (control/control.py:242, the solver's exception propagates and ends the
 *       run); a batch cannot raise for one car, so the last iterate is applied and the flag says so.
 *   S3  phase >= 2: u = (0, 0).
 * crx_seed_log_dev, after the plant and before crx_lmpc_addtraj_dev, is given both state pairs of the plant's ping-pong: xcurv_prev,
 * xglob_prev (what the plant read) and xcurv, xglob (what it wrote, which this entry may overwrite), all [batch][6]:
 *   S4  a car in phase >= 2 at entry is frozen: xcurv[b] <- xcurv_prev[b], xglob[b] <- xglob_prev[b], laps[b] <- laps_prev[b],
 *       crossed[b] = 0, and nothing else of the car is touched.  (It is stepped from the same state every step, so a car that stands
 *       next to the line would otherwise "cross" at every step.)  A seeded car therefore stands at its hand-over state: the start state
 *       of its first learning-MPC lap.
 *   S5  a car in phase 0 or 1: exactly the assignments of crx_game_log_dev (one device function serves both): crossed[b] = laps[b] >
 *       laps_prev[b]; laps_prev[b] <- laps[b]; the new state, with s unwrapped by lap_length if it crossed, to log_x[b][min(n_log,
 *       n_points - 1)]; the applied input to log_u[b][n_log - 1]; n_log += 1 (ModelBase.update_memory, utils/base.py:795-819).
 *   S6  then the phase: on a crossing, phase += 1 (0 -> 1: racing/offboard.py's one_lap sim ends, the test script changes the
 *       controller, tests/auto_racing_game_test.py:50-52; 1 -> 2: :58-68).  Otherwise, if n_log == n_points after the append -- no row
 *       is left for the next state -- phase = 3 and seed_status |= CRX_SEED_LOG_FULL.  Finally m_mpc[b] = (phase == 1).
 */
#define CRX_SEED_MPC_FAILED 1   /* S2: a step of the MPC-LTI lap applied an iterate that had not converged */
#define CRX_SEED_LOG_FULL 2     /* S6: a lap did not reach the line within n_points - 1 steps */
int crx_seed_commit_dev(int N, int batch, const int32_t* phase, const double* vt, const double* eyt, const double* x, const double* U_mpc,
                        const int32_t* mpc_status, int32_t* seed_status, double* u, void* stream);
int crx_seed_log_dev(int batch, int n_points, double lap_length, const double* xcurv_prev, const double* xglob_prev, double* xcurv,
                     double* xglob, const double* u, int32_t* laps, int32_t* laps_prev, double* log_x, double* log_u, int32_t* n_log,
                     int32_t* crossed, int32_t* phase, int32_t* seed_status, int32_t* m_mpc, void* stream);

/*
 * Race statistics (crx.montecarlo.RaceStats): what a closed-loop Monte-Carlo is run for -- contacts, cars that left the track, lap
 * times, overtakes -- accumulated per car on the device, ONE launch per sample, and reduced to one fixed record per group of cars by
 * one more.  A sample shows the kernel the cars' states as they are: the caller takes sample 0 on the initial states and one sample
 * after every control step.  Thread b owns car b; no car's bad state touches another car's statistics.
 *
 * State: two caller-owned device arrays, FIELD-major (field f of car b at [f * batch + b]):
 *   stat_i [CRX_STATS_NI][batch] int32                   stat_d [CRX_STATS_ND + n_opp_max][batch] float64
 * with the fields below; "(v)" is the value crx_race_stats_reset_dev writes.
 *   N_SAMPLES        samples taken on a finite state (0)
 *   NONFINITE_STEP   first sample whose xcurv row had a non-finite entry (-1)
 *   OFF_STEP, OFF_SAMPLES          first sample with |ey| > track_width, strictly (-1); how many such samples (0)
 *   CONTACT_STEP, CONTACT_SAMPLES  first sample with clear < 1, strictly (-1); how many such samples (0)
 *   N_LAPS, LAPS_PREV              line crossings seen since the reset (0); laps[b] at the last sample (laps[b] at the reset)
 *   LAP_STEP + k, k < CRX_STATS_MAX_LAPS   sample at which crossing number k was seen (-1); later crossings only count in N_LAPS.
 *                    A lap counter that advanced by d > 1 between two samples is d crossings seen at that sample
 *   PASSES, PASSED   overtakes made and suffered, S3 (0)
 *   FLAG_SAMPLES     samples with flag[b] != 0, when a flag array is given (0)
 *   MIN_CLEAR        running minimum of clear, S2 (+inf)          EY_MAX   running maximum of |ey| (0)
 *   SUM_EY2, SUM_DV2 running sums of ey * ey and of (vx - xt[b][0])^2, the latter only when xt is given (0); summed per car in
 *                    sample order
 *   DS_PREV + j, j < n_opp_max     lap-folded signed gap to opponent j at the previous sample (NaN)
 *
 * S1  Opponents.  Scripted mode (n_cars == 0): opponent j of car b is the scripted car (car_s0, car_v, car_ey)[b][j] at the clock t,
 *     s_opp = car_v * t + car_s0 (multiply, then add), ey_opp = car_ey; j < n_opp[b] clipped to [0, n_opp_max] (n_opp NULL: all
 *     n_opp_max); l_sum, w_sum from the descriptor.  n_opp_max == 0: a car on its own (clear = +inf, no passes).
 *     Field mode (n_cars = C >= 1): batch = n_races * C, race-major and car-minor; the opponents of a car are the C - 1 other cars of
 *     its race in car order, skipping itself, all read from the same xcurv; n_opp_max >= C - 1.  With car_dims [n_races][C][2] the
 *     pair (ego, o) has l_sum = l_e / 2 + l_o / 2, w_sum = w_e / 2 + w_o / 2 as in crx_field_prep (a non-positive or non-finite
 *     entry takes the descriptor's value).
 * S2  clear, the `clear` of crx_field_prep restated, every operation rounded on its own (no fused multiply-add):
 *     m = fmod(s_ego - s_opp + L/2, L); if (m < 0) m += L; ds = m - L/2; a = ds / l_sum; b = (ey_ego - ey_opp) / w_sum;
 *     pa, pb = the `degree`-fold products of a and of b, starting from 1.0; h = pa + pb; clear = the minimum of h over the
 *     opponents, +inf with none.
 * S3  Overtakes compare p = DS_PREV[j] with the new ds when both are finite: p < 0 && ds >= 0 && ds - p < L/2 counts one in PASSES,
 *     p >= 0 && ds < 0 && p - ds < L/2 one in PASSED (the `< L/2` keeps the sign flip of a car half a lap away from counting); then
 *     DS_PREV[j] = ds.
 * S4  Non-finite data.  A car whose own row is non-finite at a sample records NONFINITE_STEP if that is still -1; its lap counters
 *     update all the same (they are integers); its DS_PREV[*] become NaN; nothing else changes at that sample.  An opponent whose s
 *     or ey is non-finite is skipped for clear and gets DS_PREV = NaN.
 *
 * crx_race_stats_summary_dev reduces the cars of each group (group [batch] int32 in [0, n_groups), a car with another value belongs to
 * no group; NULL: one group of all cars) to sum_i [n_groups][CRX_STATS_SUM_NI] int64 and sum_d [n_groups][CRX_STATS_SUM_ND] float64.
 * Every sum is an integer sum, so the record is exact and independent of the order of the cars:
 *   CARS; NONFINITE, OFF, CONTACT = cars whose ..._STEP >= 0; CLEAN = cars with none of the three; LAPS_HIST + k, k = 0..8 = cars with
 *   N_LAPS == k (the last bin: 8 or more); PASSES, PASSED, FLAG_SAMPLES, N_SAMPLES = sums over the cars;
 *   LAP1_SUM, _MIN, _MAX, _COUNT over the first lap time LAP_STEP[0] of the cars that have one; LAP2_* over the second lap time
 *   LAP_STEP[1] - LAP_STEP[0] of the cars that have one (count 0: sum 0, min and max -1);
 *   sum_d: MIN_CLEAR = the group's minimum of MIN_CLEAR (+inf without cars), EY_MAX = its maximum of EY_MAX (0 without cars).
 * Percentiles stay with the caller: one copy of `batch` int32.
 *
 * Refused with CRX_ERR_ARG (before the library's state is looked at): a bad descriptor, batch < 0, scripted arrays (car_s0, car_v,
 * car_ey, n_opp) in field mode or car_dims in scripted mode, n_opp_max > 0 in scripted mode without all three car arrays, batch not a
 * multiple of n_cars in field mode, a group without n_groups >= 1, a NULL array that the call needs.  The host-pointer entries stage
 * through the _dev ones; stat_i and stat_d are updated in place.
 */
#define CRX_STATS_MAX_LAPS 8
#define CRX_STATS_I_N_SAMPLES 0
#define CRX_STATS_I_NONFINITE_STEP 1
#define CRX_STATS_I_OFF_STEP 2
#define CRX_STATS_I_OFF_SAMPLES 3
#define CRX_STATS_I_CONTACT_STEP 4
#define CRX_STATS_I_CONTACT_SAMPLES 5
#define CRX_STATS_I_N_LAPS 6
#define CRX_STATS_I_LAPS_PREV 7
#define CRX_STATS_I_LAP_STEP 8   /* .. 8 + CRX_STATS_MAX_LAPS - 1 */
#define CRX_STATS_I_PASSES 16
#define CRX_STATS_I_PASSED 17
#define CRX_STATS_I_FLAG_SAMPLES 18
#define CRX_STATS_NI 19
#define CRX_STATS_D_MIN_CLEAR 0
#define CRX_STATS_D_EY_MAX 1
#define CRX_STATS_D_SUM_EY2 2
#define CRX_STATS_D_SUM_DV2 3
#define CRX_STATS_D_DS_PREV 4    /* .. 4 + n_opp_max - 1 */
#define CRX_STATS_ND 4
#define CRX_STATS_MAX_OPP 32
#define CRX_STATS_SUM_CARS 0
#define CRX_STATS_SUM_NONFINITE 1
#define CRX_STATS_SUM_OFF 2
#define CRX_STATS_SUM_CONTACT 3
#define CRX_STATS_SUM_CLEAN 4
#define CRX_STATS_SUM_LAPS_HIST 5   /* .. 5 + CRX_STATS_MAX_LAPS */
#define CRX_STATS_SUM_PASSES 14
#define CRX_STATS_SUM_PASSED 15
#define CRX_STATS_SUM_FLAG_SAMPLES 16
#define CRX_STATS_SUM_N_SAMPLES 17
#define CRX_STATS_SUM_LAP1_SUM 18
#define CRX_STATS_SUM_LAP1_MIN 19
#define CRX_STATS_SUM_LAP1_MAX 20
#define CRX_STATS_SUM_LAP1_COUNT 21
#define CRX_STATS_SUM_LAP2_SUM 22
#define CRX_STATS_SUM_LAP2_MIN 23
#define CRX_STATS_SUM_LAP2_MAX 24
#define CRX_STATS_SUM_LAP2_COUNT 25
#define CRX_STATS_SUM_NI 26
#define CRX_STATS_SUM_D_MIN_CLEAR 0
#define CRX_STATS_SUM_D_EY_MAX 1
#define CRX_STATS_SUM_ND 2
typedef struct crx_stats_desc {
    int32_t n_opp_max;    /* opponent slots per car, 0 .. CRX_STATS_MAX_OPP: rows of DS_PREV */
    int32_t n_cars;       /* 0: scripted mode; 1 .. CRX_MAX_OBS + 1: field mode, cars per race */
    int32_t degree;       /* exponent of the super-ellipse: 2, 4, 6 or 8 */
    int32_t pad;
    double lap_length;    /* L */
    double track_width;   /* off track: |ey| > track_width (+inf: never) */
    double l_sum, w_sum;  /* half-sums of the lengths and widths of a pair of cars */
} crx_stats_desc;
/* degree 6, l_sum 0.4, w_sum 0.2 */
void crx_stats_desc_default(crx_stats_desc* d, int n_opp_max, int n_cars, double lap_length, double track_width);
int crx_race_stats_reset_dev(const crx_stats_desc* d, int batch, const int32_t* laps, int32_t* stat_i, double* stat_d, void* stream);
int crx_race_stats_dev(const crx_stats_desc* d, int batch, int sample, double t, const double* xcurv, const int32_t* laps,
                       const double* car_s0, const double* car_v, const double* car_ey, const int32_t* n_opp,
                       const double* car_dims, const double* xt, const int32_t* flag, int32_t* stat_i, double* stat_d,
                       void* stream);
/* crx_race_stats_dev with one lap length per car, lap_length [batch] on the device (the cars of a launch on tracks of their own), field mode
 * and scripted mode alike; d->lap_length is not used but must be valid.  A car whose lap length is not positive and finite is counted as a
 * non-finite row.  Reset and summary read no lap length: they serve both. */
int crx_race_stats_laps_dev(const crx_stats_desc* d, int batch, int sample, double t, const double* lap_length, const double* xcurv,
                            const int32_t* laps, const double* car_s0, const double* car_v, const double* car_ey, const int32_t* n_opp,
                            const double* car_dims, const double* xt, const int32_t* flag, int32_t* stat_i, double* stat_d, void* stream);
int crx_race_stats_summary_dev(const crx_stats_desc* d, int batch, const int32_t* group, int n_groups, const int32_t* stat_i,
                               const double* stat_d, int64_t* sum_i, double* sum_d, void* stream);
int crx_race_stats_reset(const crx_stats_desc* d, int batch, const int32_t* laps, int32_t* stat_i, double* stat_d);
int crx_race_stats(const crx_stats_desc* d, int batch, int sample, double t, const double* xcurv, const int32_t* laps,
                   const double* car_s0, const double* car_v, const double* car_ey, const int32_t* n_opp, const double* car_dims,
                   const double* xt, const int32_t* flag, int32_t* stat_i, double* stat_d);
int crx_race_stats_summary(const crx_stats_desc* d, int batch, const int32_t* group, int n_groups, const int32_t* stat_i,
                           const double* stat_d, int64_t* sum_i, double* sum_d);

/*
 * Multi-GPU: problems are independent and a planner sweep is sharded by scenario, so the path has
 * exactly ONE exchange step -- an all-gather of the fixed-size winner records {int32 flag; int32 status; double X[N+1][6]} (8 + 48 (N + 1) bytes =
 * 632 B at N = 12) -- issued on RCCL (ncclAllGather over xGMI).  One process per GPU.  The caller owns the rendezvous:
 * rank 0 calls crx_comm_get_unique_id and carries the CRX_COMM_ID_BYTES bytes to the other ranks by whatever it has (MPI,
 * a file, torch.distributed's store); every rank then calls crx_comm_init_rank on the device it gave crx_init (collective:
 * returns when all ranks arrived).  RCCL is resolved at run time (a copy the process already holds, e.g. PyTorch's, else
 * /opt/rocm's); libcrx does not link it.
 *   crx_allgather_winners_dev  packs this rank's n_local winners (flag [n_local] int32, best_X [n_local][N+1][6] -- the
 *       outputs of crx_select / crx_planner_plan -- and status [n_local] int32, the crx_status of the WINNING region's QP, i.e.
 *       status[s * n_regions + flag[s]] of crx_planner_solve: a consumer on another rank can tell a fall-back winner,
 *       overtake_traj_planner.py:365-374, from a solved one; NULL: the field is 0) into send [n_max][rec] (rows past n_local zero:
 *       ragged shards are padded to the largest, n_max, which every rank derives from (n_total, world) alone) and gathers every
 *       rank's block into recv [world][n_max][rec], in rank order, on `stream`.  rec = 1 + 6 (N + 1) 8-byte words; word 0 of a record
 *       holds the two int32 {flag, status} (little endian: flag in the low half), words 1.. the trajectory.  (libcrx <= 0.2.1 carried
 *       the flag as a double in word 0 and no status; 0.3.0 changed the signature.)
 */
#define CRX_COMM_ID_BYTES 128
int crx_comm_get_unique_id(void* id /* [CRX_COMM_ID_BYTES] */);
int crx_comm_init_rank(const void* id, int world, int rank);
int crx_comm_world(void);   /* 0 without a communicator */
int crx_comm_rank(void);    /* -1 without a communicator */
int crx_comm_destroy(void);
int crx_allgather_winners_dev(int n_local, int n_max, int N, const int32_t* flag, const int32_t* status, const double* best_X,
                              double* send, double* recv, void* stream);

/* Streams for device-resident loops that overlap independent launches (the two branches of a racing-game step, concurrent
 * sub-batches of races: crx.montecarlo).  Streams only overlap when they sit on different HARDWARE queues; the HIP runtime hands
 * its GPU_MAX_HW_QUEUES queues (default 4; set the variable before the process touches the GPU) to streams round-robin IN
 * CREATION ORDER.  A framework's stream pool is created interleaved with streams the caller never sees (PyTorch: low- and
 * high-priority pool entries alternate), so consecutive pool streams share queues in a pattern that depends on what the process
 * did before: measured on the 4096-race racing game with two sub-batches, 3.24 ms per step or 3.5 / 3.8 / 4.6 ms depending only
 * on how many pool streams had been handed out earlier (tools/stream_offset_probe.py; which streams share a queue is not a
 * simple function of the creation order either: tools/queue_probe.py).  crx_streams_create therefore MEASURES: it creates n + 8
 * non-blocking streams on the device of crx_init, runs pairs of 150 us single-wavefront spin kernels on them (two streams on
 * different queues finish a pair in the time of one kernel, two on the same queue in the time of two) and returns n streams of
 * which the first *n_concurrent were seen to overlap pairwise (all n when the runtime has that many queues; the rest share);
 * the other candidates are destroyed.  About 30 ms, once.  Pass them as the `stream` argument of the *_dev entry points
 * (PyTorch: torch.cuda.ExternalStream).  crx_streams_destroy synchronises and destroys them. */
int crx_streams_create(int n, void** streams /* [n] out */, int* n_concurrent /* out, may be NULL */);
int crx_streams_destroy(int n, void** streams);

/* Device time of what a caller enqueues between two marks on ONE stream, measured with a pair of HIP events the timer object owns
 * (bench.py's roofline: the solver launch alone).  crx_timer_begin / _end record on `stream` (the stream the bracketed *_dev call
 * is given); crx_timer_ms blocks until the second event has happened and returns the elapsed milliseconds, < 0 on error.  No global
 * state: any number of timers may be live on any number of streams and threads. */
int crx_timer_create(void** timer /* out */);
int crx_timer_destroy(void* timer);
int crx_timer_begin(void* timer, void* stream);
int crx_timer_end(void* timer, void* stream);
double crx_timer_ms(void* timer);

#ifdef __cplusplus
}
#endif
#endif /* CRX_H */
