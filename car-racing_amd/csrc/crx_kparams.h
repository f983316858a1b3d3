// crx_kparams.h -- internal launch descriptors shared by crx_kernels.hip and crx_api.hip.
// Not part of the public ABI (include/crx.h is).
#ifndef CRX_KPARAMS_H
#define CRX_KPARAMS_H
#include <stdint.h>

#include "../../include/crx.h"

struct crx_kparams {
    int N, batch, mode /* 0 planner QP, 1 CBF NLP */, per_stage_target, n_obs_max, degree;
    double A[36], B[12];
    double wq[6], wr[2];
    double w_dey, w_prog, w_slack;
    double delta_max, a_max, v_min, v_max, ey_max;
    double alpha, margin, l_sum, w_sum;
    double dt_ref, fallback_gain;
    crx_ipm_opts opts;
    // planner inputs (device pointers)
    const double *x0, *bez_s, *bez_ey, *ey_lb, *ey_ub;
    // cbf inputs
    const double *xt, *obs_s, *obs_ey, *lap_off;
    const int32_t* n_obs;
    const double* obs_dims;  // optional [batch][n_obs_max][2]: (l_agent + l_obs, w_agent + w_obs) per obstacle slot; NULL: l_sum, w_sum
    // outputs
    double *X, *U, *sigma, *cost, *kkt;
    int32_t *status, *iters;
    // optional per-iteration trace of ONE problem (diagnostics): trace[it][8]
    double* trace;
    int trace_problem, trace_rows;
    int poison;   // diagnostics: fill the LDS slice with NaN before set-up (catches reads of stale LDS)
    int kkt_unscaled;   // diagnostics (crx_debug_kkt_unscaled): kkt[b] of a CONVERGED solve = an UNSCALED KKT quantity (no s_d, CBF rows in the reference's units): 1 max, 2 dual, 3 violation, 4 complementarity
    int spec_idle;      // diagnostics (crx_debug_speculation(2)): the two-wave kernel with its second wave never asked
    const int32_t* active;   // optional [batch / active_div]: 0 = leave this problem alone (status CRX_SKIPPED, outputs untouched)
    int active_div;          // problems per mask entry (planner: the regions of a scenario share one entry); 0 or 1: one each
    const int32_t* order;    // optional [batch]: workgroup i solves problem order[i] (longest-first dispatch); NULL: i
    // planner QP: reachability screen (crx_kernels.hip, first thing the kernel does).  reach_row[j] = e_ey' A^j: the free response
    // of ey_j is reach_row[j] . x0; reach_gain[j] = sum_{m<j} |e_ey' A^m B| (delta_max, a_max)': how far the inputs can move it
    int reach_screen;
    double reach_gain[CRX_MAX_N + 1];
    double reach_row[CRX_MAX_N][6];
    // CBF NLP: the slacks start at provable lower bounds of their optimal values (crx_kernels.hip, set-up).  reach_gain (ey) and
    // reach_s (s) [j] = how far the boxed inputs can move the coordinate of stage j from its free response
    int slack_start;
    double reach_s[CRX_MAX_N + 1];
};

// crx_solve_kernel with ONE LTI model per problem (crx_kernels_models.hip; the CBF NLP, and the planner QP without obstacle slots).  Derived, so
// that crx_kparams -- which every solver kernel takes by value -- keeps its size and the shared-model code objects stay what they are; the helpers
// keep taking const crx_kparams&.  A, B, reach_s, reach_gain and reach_row of the base are not read by these kernels.
struct crx_kparams_models : crx_kparams {
    const double *model_A, *model_B;   // [batch][36], [batch][12]
    // mode says which layout model_reach holds (no second pointer):
    //   1 (CBF NLP)     [batch][2][CRX_MAX_N + 1]: reach_s, reach_gain of each problem's model (crx_cbf_reach_kernel)
    //   0 (planner QP)  [batch][CRX_MAX_N][7]: stage j = e_ey' A^j (6), then reach_gain[j] (crx_planner_reach_kernel)
    const double* model_reach;
};

struct crx_lmpc_kparams {
    int N, batch, n_ss_max;
    double Q[6], R[2], dR[2], x_track[6];
    double v_max, ey_max, delta_max, a_max, w_x0;
    crx_ipm_opts opts;
    const double *x0, *u_old, *A, *B, *C, *ss, *qfun;
    const int32_t* n_ss;
    double *X, *U, *lambda, *cost, *kkt;
    int32_t *status, *iters;
    double* trace;   // optional per-iteration phase cycles of ONE problem (diagnostics): trace[it][16]
    int trace_problem, trace_rows;
    int poison;      // diagnostics: fill the LDS slice with NaN before set-up
    const int32_t* active;   // optional [batch]: 0 = leave this problem alone (status CRX_SKIPPED, outputs untouched)
    const int32_t* order;    // optional [batch]: workgroup i solves problem order[i] (longest-first dispatch); NULL: i
    int reach_screen;        // terminal-set reachability screen of the first attempt (crx_lmpc.hip)
};

struct crx_select_kparams {
    int N, V, n_scen;
    double veh_length, veh_width, lap_length, w_prog, w_coll, w_switch;
    const int32_t* n_veh;
    const double *X, *obs_s, *obs_ey;
    const int32_t* old_flag;
    int32_t* flag;
    double *sel_cost, *best_X;
};

// ---- crx_prep.hip: what turns raw scenarios into the arrays a solver reads ----
struct crx_prep_kparams {
    int N, V, n_scen, n_opt;
    double prediction_factor, lookahead, track_width, lap_length, veh_length, veh_width, safety_margin, dt_ref;
    const double *x_wrapped, *x_raw, *veh_info, *max_dv, *obs_s, *obs_ey, *opt_s, *opt_ey;
    const int32_t* n_veh;
    double *x0, *bez_s, *bez_ey, *ey_lb, *ey_ub;
};

struct crx_scene_kparams {
    crx_scene_desc d;
    int n_scen;
    const double *ego_xcurv, *veh_xcurv, *pred_s, *pred_ey;
    const int32_t* n_all;
    int32_t *n_veh, *overflow, *order;
    double *veh_info, *max_dv, *obs_s, *obs_ey;
};

struct crx_trackprep_kparams {
    int N, V, batch;
    double lap_length, safety_time, dt_ref;
    const double *x, *obs_s_in, *obs_ey_in, *traj;
    const int32_t* n_veh;
    double *xt, *obs_s, *obs_ey, *lap_off;
    int32_t* n_obs;
};

struct crx_cbfprep_kparams {
    int N, V, batch;
    double lap_length, t, dt, safety_time;
    const double *xcurv, *car_s0, *car_v, *car_ey;
    double *obs_s, *obs_ey, *lap_off;
    int32_t* n_obs;
};

// crx_cbfprep_laps_kernel.  Derived, so that crx_cbfprep_kparams -- which crx_cbfprep_kernel takes by value -- keeps its size.
struct crx_cbfprep_kparams_laps : crx_cbfprep_kparams {
    const double* lap_lengths;   // [batch]: race b's own lap length; lap_length of the base is unused
};

// The NLP family's obstacle arrays of the n_races * n_cars egos of a field, in crx_cbf_solve_dev's layout (nlp_ego_pass, crx_prep.hip)
struct crx_nlp_obs {
    double *obs_s, *obs_ey, *lap_off;         // [n_races * n_cars][n_cars - 1][N + 1] twice, [..][n_cars - 1]
    int32_t* n_obs;
    double *obs_dims, *clear;                 // obs_dims: written iff car_dims; clear: optional
};

// crx_field_prep_kernel (crx_prep.hip): predictions of every car of every race and the obstacle arrays of the n_races * n_cars NLPs
struct crx_field_kparams {
    crx_field_desc d;
    int n_races;
    const double *track, *xcurv, *car_dims;   // car_dims: optional [n_races][n_cars][2] (length, width); NULL: d.l_sum, d.w_sum for every pair
    double *pred_s, *pred_ey;
    crx_nlp_obs nlp;
};

// crx_field_traffic_kernel (crx_prep.hip): predictions of every car of every race and, per ego, the other cars of its race as the scene's inputs
struct crx_field_traffic_kparams {
    crx_field_desc d;                          // safety_time, degree, l_sum, w_sum are not read
    int n_races;
    const double *track, *xcurv;
    double *pred_s_car, *pred_ey_car;          // [n_races][n_cars][N+1]
    double *veh_xcurv, *pred_s, *pred_ey;      // [n_races * n_cars][n_cars - 1][6], [..][n_cars - 1][N+1] twice; hold nothing (may be NULL) with one car
    int32_t* n_all;                            // [n_races * n_cars] = n_cars - 1
};

// crx_mixed_prep_kernel (crx_prep.hip): the roll-out of every car of every race and, per ego, the obstacle arrays of the solver family its policy names
struct crx_mixed_kparams {
    crx_mixed_desc d;
    int n_races;
    const double *track, *xcurv, *car_dims;    // car_dims: optional, as in crx_field_kparams
    const int32_t* policy;                     // [n_races][n_cars] CRX_POLICY_*
    double *pred_s, *pred_ey;                  // [n_races][n_cars][max(N, N_ilqr) + 1]
    crx_nlp_obs nlp;                           // the NLP family
    int32_t* m_nlp;
    double *il_obs_s, *il_obs_ey, *il_lap_off; // the iLQR family, [..][n_cars - 1][N_ilqr + 1] ...; touched iff N_ilqr > 0
    int32_t *il_n_obs, *m_ilqr;
};

// One track per RACE (crx_field_prep_tracks_kernel, crx_mixed_prep_tracks_kernel; crx_prep.hip): the track set of crx_plant_kparams_tracks with the
// id per race.  `track` of the base is the set's tracks [n_tracks][seg_stride][6]; d.n_seg and d.lap_length of the base are unused.
struct crx_race_tracks {
    int n_tracks, seg_stride;            // n_tracks in [1, CRX_MAX_TRACKS], seg_stride in [1, CRX_PLANT_MAX_SEG]
    const int32_t *n_seg, *race_track;   // [n_tracks], [n_races]
    const double* lap_length;            // [n_tracks]
};
// Derived, so that crx_field_kparams and crx_mixed_kparams -- which the one-track kernels take by value -- keep their size.
struct crx_field_kparams_tracks : crx_field_kparams {
    crx_race_tracks set;
};
struct crx_mixed_kparams_tracks : crx_mixed_kparams {
    crx_race_tracks set;
};

// ---- crx_path.hip: crx_path_kernel, the path QP (crx_path_qp.h) without a mask ----
struct crx_path_kparams {
    int N, batch;
    double alpha, w_rate;
    crx_ipm_opts opts;
    const double *opt, *bez, *lb, *ub, *e0, *eN;
    double *E, *cost, *kkt;
    int32_t *status, *iters;
};

// ---- crx_pathplan.hip: the overtake PATH planner around its QPs ----
// crx_path_masked_kernel (crx_path_qp.h once more, with a per-QP mask).  Derived, so that crx_path_kparams -- which crx_path_kernel takes by
// value -- keeps its size and the code object behind crx_path_solve stays what it is.
struct crx_path_kparams_masked : crx_path_kparams {
    const int32_t* active;   // optional [batch]: 0 = this QP is not solved: status CRX_SKIPPED, cost +inf, iters 0, E and kkt untouched.  NULL: all
};

// crx_pathprep_kernel / crx_pathselect_kernel
struct crx_pathplan_kparams {
    crx_pathprep_desc d;
    int n_scen;
    const double *x_wrapped, *x_raw, *veh_xcurv, *max_dv, *obs_ey, *opt_s, *opt_ey, *opt_vx;
    const int32_t *n_veh, *order, *active;   // active: optional [n_scen], fused step only
    // prep outputs = inputs of the QP launch
    double *opt, *bez, *lb, *ub, *e0, *eN, *span;
    int32_t* qp_active;                      // optional [n_scen * (V + 1)]: the mask crx_path_masked_kernel runs under (fused step)
    // selection
    const double *E, *cost;
    int32_t *flag, *plan_status;
    double* target;
};

// ---- crx_plant.hip: the four inclusions of crx_plant_step.h ----
#define CRX_PLANT_MAX_SEG 64   // rows of a track's segment table a kernel keeps in LDS (the plant, crx_field_prep_kernel, crx_field_traffic_kernel)
struct crx_plant_kparams {
    crx_plant_desc d;
    int batch, u_stride, wrap;
    const double *track, *xglob, *xcurv, *u;
    double *xglob_next, *xcurv_next;
    int32_t* laps;
    const double* noise_z;   // optional [batch][3] standard-normal draws: the bounded process noise of base.py:929-939
};

// crx_plant_cars_kernel.  Derived, so that crx_plant_kparams -- which crx_plant_kernel takes by value -- keeps its size and
// the code object behind the shared-parameter launches stays what it is.
struct crx_plant_kparams_cars : crx_plant_kparams {
    const double* params;   // [batch][CRX_PLANT_NPARAM]: m, lf, lr, Iz, Df, Cf, Bf, Dr, Cr, Br of each vehicle; d's ten values are unused
};

// crx_plant_tracks_kernel / crx_plant_tracks_cars_kernel.  Derived once more, for the same reason.  `track` of the base is the set's
// tracks [n_tracks][seg_stride][6]; d.n_seg and d.lap_length are unused; params NULL: d's ten values (crx_plant_tracks_kernel).
struct crx_plant_kparams_tracks : crx_plant_kparams_cars {
    int n_tracks, seg_stride;          // n_tracks in [1, CRX_MAX_TRACKS], seg_stride in [1, CRX_PLANT_MAX_SEG]
    const int32_t *n_seg, *track_id;   // [n_tracks], [batch]
    const double* lap_length;          // [n_tracks]
};

// ---- crx_lmpcprep.hip ----
struct crx_lmpcprep_kparams {
    crx_lmpcprep_desc d;
    int batch, from_plan;
    const double *ss_xcurv, *u_ss, *qfun;
    const int32_t *time_ss, *iter;
    const double *x, *lin_points, *lin_input, *track;
    double *A, *B, *C, *ss_sel, *q_sel;
    int32_t* status;
    const int32_t* active;   // optional [batch]: 0 = leave this race alone (status CRX_SKIPPED, outputs untouched)
};

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
hipError_t crx_launch_solve(const crx_kparams& kp, int nobs_template, hipStream_t st);
hipError_t crx_launch_solve_models(const crx_kparams_models& kp, int nobs_template, hipStream_t st);   // crx_kernels_models_{plan,obs,gen}.hip: plan -> obs -> general unit
hipError_t crx_launch_cbf_reach(int N, int batch, double delta_max, double a_max, const double* model_A, const double* model_B, double* model_reach, hipStream_t st);
hipError_t crx_launch_planner_reach(int N, int batch, double delta_max, double a_max, const double* model_A, const double* model_B, double* model_reach, hipStream_t st);
hipError_t crx_launch_solve_spec(const crx_kparams& kp, hipStream_t st);   // crx_kernels_spec.hip: the two-wave instantiations <1, 12, 6, {12, 10}, 1>
hipError_t crx_launch_select(const crx_select_kparams& sp, hipStream_t st);
hipError_t crx_launch_debug_reduce(const double* in, double* out, hipStream_t st);
hipError_t crx_launch_lmpc_addtraj(const crx_lmpcprep_desc& d, int batch, const int32_t* crossed, double* log_x, const double* log_u,
                                   int32_t* n_log, double* ss_xcurv, double* u_ss, double* qfun, int32_t* time_ss, int32_t* iter,
                                   int32_t* step, const double* x, int32_t* status, hipStream_t st);
size_t crx_solve_lds_bytes(int N, int nobs_template);
int crx_solve_resident_per_cu(int N, int nobs_template);
// crx_prep.hip
hipError_t crx_launch_prep(const crx_prep_kparams& pp, hipStream_t st);
hipError_t crx_launch_scene(const crx_scene_kparams& sp, hipStream_t st);
hipError_t crx_launch_trackprep(const crx_trackprep_kparams& tp, hipStream_t st);
hipError_t crx_launch_cbfprep(const crx_cbfprep_kparams& cp, hipStream_t st);
hipError_t crx_launch_cbfprep_laps(const crx_cbfprep_kparams_laps& cp, hipStream_t st);
hipError_t crx_launch_field_prep(const crx_field_kparams& fp, hipStream_t st);
hipError_t crx_launch_field_traffic(const crx_field_traffic_kparams& tp, hipStream_t st);
hipError_t crx_launch_mixed_prep(const crx_mixed_kparams& mp, hipStream_t st);
hipError_t crx_launch_field_prep_tracks(const crx_field_kparams_tracks& fp, hipStream_t st);
hipError_t crx_launch_mixed_prep_tracks(const crx_mixed_kparams_tracks& mp, hipStream_t st);
// crx_plant.hip
hipError_t crx_launch_plant(const crx_plant_kparams& pk, hipStream_t st);
hipError_t crx_launch_plant_cars(const crx_plant_kparams_cars& pk, hipStream_t st);
hipError_t crx_launch_plant_tracks(const crx_plant_kparams_tracks& pk, hipStream_t st);
// crx_path.hip
hipError_t crx_launch_path(const crx_path_kparams& pp, hipStream_t st);
// crx_pathplan.hip
hipError_t crx_launch_path_masked(const crx_path_kparams_masked& pp, hipStream_t st);
hipError_t crx_launch_pathprep(const crx_pathplan_kparams& pp, hipStream_t st);
hipError_t crx_launch_pathselect(const crx_pathplan_kparams& pp, hipStream_t st);

// crx_order.hip: dispatch order of a solver launch (include/crx.h, "Dispatch order"): a stable counting sort of the batch by a 257-valued key
struct crx_order_kparams {
    int batch, mode;             // mode 0: iteration counts of the previous solve, descending; 1: smallest start barrier, ascending
    const int32_t *iters, *active;
    int32_t* order;
    int V, stride, degree, per_stage_target;   // mode 1: obstacle slots, N + 1, exponent of the ellipse, layout of xt
    double margin, l_sum, w_sum, ds_per_vx;    // ds_per_vx = A[4][0]: progress per stage and unit speed
    const double *x0, *xt, *obs_s, *obs_ey, *lap_off, *obs_dims;
    const int32_t* n_obs;
};
hipError_t crx_launch_order(const crx_order_kparams& op, hipStream_t st);

// crx_game.hip: device-resident racing-game loop: the bookkeeping between the solver launches (crx.montecarlo.GameLaps / LmpcLaps)
struct crx_game_kparams {
    int N, Np, batch, n_cars, n_points;
    double lap_length, t, dt;
    // traffic
    const double *car_s0, *car_v, *car_ey;
    double *veh_xcurv, *pred_s, *pred_ey;
    // masks
    const int32_t *n_veh, *overflow;
    int32_t *m_overtake, *m_lmpc, *overflow_seen;
    // commit
    const int32_t* overtake;
    const double *U_track, *X_lmpc, *U_lmpc;
    const int32_t* flag;
    double *u, *u_old, *u_prev, *lin_points, *lin_input;
    int32_t *step_no, *addpoint_step, *old_flag;
    // log
    const double* xcurv;
    const int32_t* laps;
    int32_t *laps_prev, *n_log, *crossed;
    double *log_x, *log_u;
};
hipError_t crx_launch_game(int which, const crx_game_kparams& gp, hipStream_t st);
// crx_game.hip: seed laps (crx.montecarlo.SeedLaps, include/crx.h S1-S6): each car's PID lap and MPC-LTI lap become its own safe set
struct crx_seed_kparams {
    int batch, n_points, u_stride;                     // u_stride: doubles between the plans of two cars in U_mpc (2 N)
    double lap_length;
    int32_t *phase, *seed_status, *m_mpc;              // [batch] each
    // commit
    const double *vt, *eyt, *x, *U_mpc;                // x [batch][6]: the state the step starts from
    const int32_t* mpc_status;
    double* u;                                         // [batch][2]; the log reads it
    // log
    const double *xcurv_prev, *xglob_prev;             // what the plant read
    double *xcurv, *xglob;                             // what the plant wrote
    int32_t *laps, *laps_prev, *n_log, *crossed;
    double *log_x, *log_u;
};
hipError_t crx_launch_seed(int which, const crx_seed_kparams& sp, hipStream_t st);   // 0 commit, 1 log
// crx_game.hip: mixed fields (crx.montecarlo.MixedRaces, include/crx.h "Mixed fields"): each car's input from its own controller's law
struct crx_mixed_commit_kparams {
    int batch, nlp_stride, ilqr_stride;                // strides: doubles between the plans of two cars in U_nlp / U_ilqr
    const int32_t* policy;                             // [batch] CRX_POLICY_*
    const double* x;                                   // [batch][6]: the state the step starts from
    const double *vt, *eyt;                            // PID: [batch] each, both or neither
    const double *K, *xt;                              // LQR: [batch][2][6], [batch][6], both or neither
    const double *U_nlp, *U_ilqr;                      // the solver families' plans
    const int32_t *nlp_status, *ilqr_status;           // [batch] each; each goes with its plan
    double* u;                                         // [batch][2]
    int32_t* ctrl_status;                              // [batch]
};
hipError_t crx_launch_mixed_commit(const crx_mixed_commit_kparams& cp, hipStream_t st);
// crx_game.hip: per-car race statistics of every closed loop (crx.montecarlo.RaceStats): reset, one sample, the batch summary
struct crx_stats_kparams {
    crx_stats_desc d;
    int batch, sample, n_groups;
    double t;                                          // scripted mode: the scripted cars' clock at this sample
    const double *xcurv, *car_s0, *car_v, *car_ey;     // xcurv [batch][6]; scripted mode: [batch][n_opp_max] each
    const double *car_dims, *xt;                       // optional: field mode [n_races][n_cars][2] (length, width); [batch][6]
    const int32_t *laps, *n_opp, *flag, *group;        // n_opp, flag, group: optional [batch]
    int32_t* stat_i;                                   // [CRX_STATS_NI][batch]
    double* stat_d;                                    // [CRX_STATS_ND + n_opp_max][batch]
    long long* sum_i;                                  // summary: [n_groups][CRX_STATS_SUM_NI]
    double* sum_d;                                     //          [n_groups][CRX_STATS_SUM_ND]
};
hipError_t crx_launch_race_stats(int which, const crx_stats_kparams& sp, hipStream_t st);   // 0 reset, 1 one sample, 2 summary
// crx_race_stats_laps_kernel.  Derived, so that crx_stats_kparams -- which the three kernels above take by value -- keeps its size.
struct crx_stats_kparams_laps : crx_stats_kparams {
    const double* lap_lengths;                         // [batch]: car b's own lap length; d.lap_length is unused
};
hipError_t crx_launch_race_stats_laps(const crx_stats_kparams_laps& sp, hipStream_t st);   // one sample
// crx_lmpc.hip, crx_lmpcprep.hip
hipError_t crx_launch_lmpc(const crx_lmpc_kparams& kp, hipStream_t st);
hipError_t crx_launch_lmpcprep(const crx_lmpcprep_kparams& kp, hipStream_t st);
size_t crx_lmpcprep_lds_bytes(int n_points);
hipError_t crx_launch_lmpc_addpoint(const crx_lmpcprep_desc& d, int batch, double* ss_xcurv, double* u_ss, const int32_t* time_ss,
                                    const int32_t* iter, const int32_t* step, const double* x, const double* u, int u_stride,
                                    hipStream_t st);
size_t crx_lmpc_lds_bytes(int N, int n_ss_max);
int crx_lmpc_resident_per_cu(int N, int n_ss_max);
// iLQR (crx_ilqr.hip)
struct crx_ilqr_kparams {
    int N, batch, n_obs_max, max_iter;
    double A[36], B[12], Q[36], R[4];
    double eps, lamb_init, lamb_factor, lamb_max, margin, q1, q2, l_sum, w_sum;
    const double *x0, *xt, *obs_s, *obs_ey, *lap_off;
    const int32_t *n_obs, *active;
    double *X, *U, *cost;
    int32_t *status, *iters;
    // optional per-problem models [batch][36], [batch][12] (both or neither): the LDS copies of A, B come from them, A and B above are unused
    const double *model_A, *model_B;
};
hipError_t crx_launch_ilqr(const crx_ilqr_kparams& kp, hipStream_t st);
size_t crx_ilqr_lds_bytes(int N);
int crx_ilqr_resident_per_cu(int N);
// LQR design and control law (crx_lqr.hip)
struct crx_lqr_kparams {
    int batch, max_iter;
    double Q[36], R[4], eps;
    const double *A, *B;       // [batch][36], [batch][12]
    const int32_t* active;     // optional [batch]: 0 = leave this model alone (status CRX_SKIPPED, outputs untouched)
    double *K, *P;             // [batch][12]; [batch][36] or NULL
    int32_t *status, *iters;
};
hipError_t crx_launch_lqr_design(const crx_lqr_kparams& kp, hipStream_t st);
hipError_t crx_launch_lqr_step(int batch, const double* K, const double* xcurv, const double* xt, double* u, hipStream_t st);
// system identification (crx_sysid.hip)
struct crx_sysid_kparams {
    int n_logs, n_groups, first_row, chunk, tpl;   // tpl = tile slots per log in the workspace
    double lamb;
    const int64_t* log_off;
    const int32_t* grp_off;   // NULL = one group per log
    const double *x, *u;
    double *ws_gram, *ws_res, *ws_W;
    double *A, *B, *err;
    int64_t* n_pairs;
    int32_t* status;
};
hipError_t crx_launch_sysid(const crx_sysid_kparams& kp, hipStream_t st);
struct crx_pid_kparams {
    int batch, T, row;
    const double *vt, *eyt, *xcurv, *u_prev;
    double *u_next, *x_log, *u_log;
};
hipError_t crx_launch_pid_log(const crx_pid_kparams& kp, hipStream_t st);

// the launch the small kernels share (crx_prep, crx_plant, crx_path, crx_pathplan): nothing for n = 0, else a 1-D grid with `per_block` of the n
// elements to a block of `threads` threads (a thread each: per_block = threads; a wavefront per problem: per_block = 1, threads = WAVE)
template <typename P>
static inline hipError_t crx_launch_1d(void (*kernel)(const P), int n, int per_block, int threads, hipStream_t st, const P& p) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(kernel, dim3((n + per_block - 1) / per_block), dim3(threads), 0, st, p);
    return hipGetLastError();
}
#endif
#endif
