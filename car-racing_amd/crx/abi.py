"""ctypes mirror of include/crx.h (struct layouts + argument marshalling).

Pure declarations: no library is loaded here.  `Binding` wraps any CDLL that exports the crx entry
points under a given symbol prefix, so the same marshalling code drives libcrx (prefix "crx_") and,
in tests only, the CPU oracle (prefix "crx_oracle_").
"""
import ctypes as C

import numpy as np

CRX_MAX_N = 24
CRX_ILQR_MAX_N = 64   # horizon limit of crx_ilqr_solve
CRX_MAX_OBS = 6     # obstacles per MPC-CBF NLP
CRX_MAX_VEH = 6     # vehicles of interest per planner scenario (= CRX_MAX_OBS)

CRX_CONVERGED, CRX_MAX_ITER, CRX_INFEASIBLE, CRX_RESTORED, CRX_SKIPPED, CRX_STALLED = 0, 1, 2, 3, 4, 5
CRX_SINGULAR = 6    # crx_sysid_fit, crx_lqr_design
CRX_OUT_OF_DOMAIN = 7   # crx_path_plan's plan_status: a look-up above the optimal-trajectory table (the reference raises) or a non-finite input


class IpmOpts(C.Structure):
    _fields_ = [
        ("tol", C.c_double),
        ("max_iter", C.c_int32),
        ("restore_iters", C.c_int32),
        ("mu_init", C.c_double),
        ("kappa_eps", C.c_double),
        ("kappa_mu", C.c_double),
        ("theta_mu", C.c_double),
        ("tau_min", C.c_double),
        ("slack_push", C.c_double),
        ("grad_scale_max", C.c_double),
        ("reach_screen", C.c_int32),
        ("slack_start", C.c_int32),
        ("dual_inf_tol", C.c_double),      # [0.4.0] IPOPT's complete termination test: the three UNSCALED tolerances
        ("constr_viol_tol", C.c_double),
        ("compl_inf_tol", C.c_double),
        ("stall_iters", C.c_int32),        # [0.4.0] the stall rule's budget (a kernel constant until 0.3.x)
        ("qp_method", C.c_int32),          # [0.4.0] 0 = Mehrotra predictor-corrector for the all-linear problems, 1 = IPOPT-style filter line search
    ]


# Options that differ from the defaults for every descriptor built through default_opts() from now on (bench.py's
# --no-reach-screen / --slack-start, A/B tools).  Options travel in the descriptor: libcrx has no process-global switches.
OPTS_OVERRIDE = {}


def default_opts(**kw):
    """IPOPT defaults the reference inherits (control.py:593 passes print options only) + libcrx's own two switches
    (include/crx.h crx_ipm_opts: reach_screen = 1, slack_start = 2)."""
    o = IpmOpts(1e-8, 200, 50, 0.1, 10.0, 0.2, 1.5, 0.99, 1e-2, 100.0, 1, 2, 1.0, 1e-4, 1e-4, 100, 0)
    for k, v in {**OPTS_OVERRIDE, **kw}.items():
        setattr(o, k, v)
    return o


def cbf_class_budgets(N, n_obs_max):
    """(stall_iters, restore_iters) crx_cbf_desc_default picks for a problem class; explicit OPTS_OVERRIDE entries win."""
    kw = {"stall_iters": 50, "restore_iters": 25} if (int(N) <= 12 and int(n_obs_max) <= 1) else {"stall_iters": 100, "restore_iters": 50}
    return {k: v for k, v in kw.items() if k not in OPTS_OVERRIDE}


class PlannerDesc(C.Structure):
    _fields_ = [
        ("N", C.c_int32),
        ("reserved0", C.c_int32),
        ("A", C.c_double * 36),
        ("B", C.c_double * 12),
        ("w_ref", C.c_double),
        ("w_dey", C.c_double),
        ("w_prog", C.c_double),
        ("vx_max", C.c_double),
        ("delta_max", C.c_double),
        ("a_max", C.c_double),
        ("dt_ref", C.c_double),
        ("fallback_gain", C.c_double),
        ("opts", IpmOpts),
    ]


class CbfDesc(C.Structure):
    _fields_ = [
        ("N", C.c_int32),
        ("n_obs_max", C.c_int32),
        ("per_stage_target", C.c_int32),
        ("degree", C.c_int32),
        ("A", C.c_double * 36),
        ("B", C.c_double * 12),
        ("Q", C.c_double * 6),
        ("R", C.c_double * 2),
        ("delta_max", C.c_double),
        ("a_max", C.c_double),
        ("v_min", C.c_double),
        ("v_max", C.c_double),
        ("ey_max", C.c_double),
        ("alpha", C.c_double),
        ("margin", C.c_double),
        ("l_sum", C.c_double),
        ("w_sum", C.c_double),
        ("w_slack", C.c_double),
        ("opts", IpmOpts),
    ]


class LmpcDesc(C.Structure):
    _fields_ = [
        ("N", C.c_int32),
        ("n_ss_max", C.c_int32),
        ("Q", C.c_double * 6),
        ("R", C.c_double * 2),
        ("dR", C.c_double * 2),
        ("x_track", C.c_double * 6),
        ("v_max", C.c_double),
        ("ey_max", C.c_double),
        ("delta_max", C.c_double),
        ("a_max", C.c_double),
        ("w_x0", C.c_double),
        ("opts", IpmOpts),
    ]


class IlqrDesc(C.Structure):
    _fields_ = [
        ("N", C.c_int32),
        ("max_iter", C.c_int32),
        ("n_obs_max", C.c_int32),
        ("pad_", C.c_int32),
        ("A", C.c_double * 36),
        ("B", C.c_double * 12),
        ("Q", C.c_double * 36),
        ("R", C.c_double * 4),
        ("eps", C.c_double),
        ("lamb_init", C.c_double),
        ("lamb_factor", C.c_double),
        ("lamb_max", C.c_double),
        ("margin", C.c_double),
        ("q1", C.c_double),
        ("q2", C.c_double),
        ("l_sum", C.c_double),
        ("w_sum", C.c_double),
    ]


class LqrDesc(C.Structure):
    _fields_ = [
        ("max_iter", C.c_int32),
        ("pad_", C.c_int32),
        ("Q", C.c_double * 36),
        ("R", C.c_double * 4),
        ("eps", C.c_double),
    ]


class SysidDesc(C.Structure):
    _fields_ = [
        ("lamb", C.c_double),
        ("first_row", C.c_int32),
        ("chunk_rows", C.c_int32),
        ("reserved", C.c_int32 * 4),
    ]


class PrepDesc(C.Structure):
    _fields_ = [
        ("N", C.c_int32),
        ("n_veh_max", C.c_int32),
        ("n_opt", C.c_int32),
        ("reserved0", C.c_int32),
        ("prediction_factor", C.c_double),
        ("lookahead", C.c_double),
        ("track_width", C.c_double),
        ("lap_length", C.c_double),
        ("veh_length", C.c_double),
        ("veh_width", C.c_double),
        ("safety_margin", C.c_double),
        ("dt_ref", C.c_double),
    ]


class LmpcPrepDesc(C.Structure):
    _fields_ = [
        ("N", C.c_int32), ("n_points", C.c_int32), ("n_laps", C.c_int32), ("n_ss_per_lap", C.c_int32),
        ("n_ss_laps", C.c_int32), ("max_neighbours", C.c_int32), ("n_seg", C.c_int32), ("shift", C.c_int32),
        ("bandwidth", C.c_double), ("scale", C.c_double * 5), ("dt", C.c_double), ("lap_length", C.c_double),
    ]


def lmpcprep_desc(N, n_points, n_laps, n_seg, dt, lap_length, n_ss_per_lap=22, n_ss_laps=2, max_neighbours=40, shift=0):
    """Literals of control/lmpc_helper.py:42-57, utils/base.py:605 and LMPCRacingParam (utils/base.py:351-376)."""
    return LmpcPrepDesc(int(N), int(n_points), int(n_laps), int(n_ss_per_lap), int(n_ss_laps), int(max_neighbours), int(n_seg),
                        int(shift), 5.0, _arr(C.c_double, 5, (0.1, 1.0, 1.0, 1.0, 1.0)), float(dt), float(lap_length))


class SceneDesc(C.Structure):
    _fields_ = [("N", C.c_int32), ("n_all_max", C.c_int32), ("n_veh_max", C.c_int32), ("reserved0", C.c_int32),
                ("safety_factor", C.c_double), ("prediction_factor", C.c_double), ("veh_length", C.c_double), ("lap_length", C.c_double)]


def scene_desc(N, n_all_max, n_veh_max, lap_length, safety_factor=4.5, prediction_factor=0.5, veh_length=0.4):
    """RacingGameParam.safety_factor / planning_prediction_factor, CarParam.length (utils/base.py:379-408, :700)."""
    return SceneDesc(int(N), int(n_all_max), int(n_veh_max), 0, safety_factor, prediction_factor, veh_length, float(lap_length))


class PathDesc(C.Structure):
    _fields_ = [("N", C.c_int32), ("reserved0", C.c_int32), ("alpha", C.c_double), ("w_rate", C.c_double), ("opts", IpmOpts)]


class PathPrepDesc(C.Structure):
    _fields_ = [("N", C.c_int32), ("n_veh_max", C.c_int32), ("n_opt", C.c_int32), ("n_all_max", C.c_int32),
                ("safety_factor", C.c_double), ("prediction_factor", C.c_double), ("lookahead", C.c_double), ("next_lap_range", C.c_double),
                ("track_width", C.c_double), ("lap_length", C.c_double), ("veh_length", C.c_double), ("veh_width", C.c_double),
                ("a_max_plan", C.c_double)]


def pathprep_desc(N, n_veh_max, n_all_max, n_opt, track_width, lap_length, safety_factor=4.5, prediction_factor=0.5, veh_length=0.4,
                  veh_width=0.2):
    """RacingGameParam.safety_factor / planning_prediction_factor, CarParam (utils/base.py:379-408, :700) and the literals of
    planner_helper.py:51-53, :178 and overtake_path_planner.py:140 (include/crx.h crx_pathprep_desc)."""
    return PathPrepDesc(int(N), int(n_veh_max), int(n_opt), int(n_all_max), safety_factor, prediction_factor, 4.0, 20.0, float(track_width),
                        float(lap_length), veh_length, veh_width, 1.5)


class PlantDesc(C.Structure):
    _fields_ = [
        ("n_sub", C.c_int32),
        ("n_seg", C.c_int32),
        ("dt_sub", C.c_double),
        ("lap_length", C.c_double),
        ("m", C.c_double), ("lf", C.c_double), ("lr", C.c_double), ("Iz", C.c_double),
        ("Df", C.c_double), ("Cf", C.c_double), ("Bf", C.c_double),
        ("Dr", C.c_double), ("Cr", C.c_double), ("Br", C.c_double),
    ]


class FieldDesc(C.Structure):
    _fields_ = [("N", C.c_int32), ("n_cars", C.c_int32), ("n_seg", C.c_int32), ("degree", C.c_int32), ("lap_length", C.c_double),
                ("dt", C.c_double), ("safety_time", C.c_double), ("l_sum", C.c_double), ("w_sum", C.c_double)]


def field_desc(N, n_cars, n_seg, lap_length, dt=0.1, safety_time=2.0, degree=6, l_sum=0.4, w_sum=0.2):
    """crx_field_desc_default: the literal safety_time of control.mpccbf (control.py:499), degree of :528, CarParam's dimensions."""
    return FieldDesc(int(N), int(n_cars), int(n_seg), int(degree), float(lap_length), float(dt), float(safety_time), float(l_sum), float(w_sum))


# include/crx.h "Mixed fields": one policy code per car
POLICY_NONE, POLICY_PID, POLICY_LQR, POLICY_MPC_LTI, POLICY_MPCCBF, POLICY_ILQR = range(6)
POLICY_NAMES = ("none", "pid", "lqr", "mpc_lti", "mpccbf", "ilqr")


def policy_codes(policy):
    """int32 array of CRX_POLICY_* codes, in the shape given, from codes or names (POLICY_NAMES, any case); anything else is a ValueError."""
    a = np.asarray(policy)
    if a.dtype.kind in "US":
        names = [str(s).lower() for s in a.reshape(-1)]
        bad = sorted(set(names) - set(POLICY_NAMES))
        if bad:
            raise ValueError("unknown policy name(s) %s: one of %s" % (bad, POLICY_NAMES))
        return np.array([POLICY_NAMES.index(s) for s in names], dtype=np.int32).reshape(a.shape)
    if a.dtype.kind not in "iu" or a.size and (a.min() < 0 or a.max() >= len(POLICY_NAMES)):
        raise ValueError("policy: integer codes 0 .. %d or names %s" % (len(POLICY_NAMES) - 1, POLICY_NAMES))
    return np.ascontiguousarray(a, dtype=np.int32)


class MixedDesc(C.Structure):
    _fields_ = [("N", C.c_int32), ("N_ilqr", C.c_int32), ("n_cars", C.c_int32), ("n_seg", C.c_int32), ("degree", C.c_int32),
                ("ilqr_obstacles", C.c_int32), ("lap_length", C.c_double), ("dt", C.c_double), ("safety_time", C.c_double), ("l_sum", C.c_double),
                ("w_sum", C.c_double)]


def mixed_desc(N, N_ilqr, n_cars, n_seg, lap_length, ilqr_obstacles=0, dt=0.1, safety_time=2.0, degree=6, l_sum=0.4, w_sum=0.2):
    """crx_mixed_desc_default: field_desc's values; N_ilqr = 0: no iLQR arrays; ilqr_obstacles = 0: the last other car only (quirk I1), 1: all."""
    return MixedDesc(int(N), int(N_ilqr), int(n_cars), int(n_seg), int(degree), int(ilqr_obstacles), float(lap_length), float(dt),
                     float(safety_time), float(l_sum), float(w_sum))


class StatsDesc(C.Structure):
    _fields_ = [("n_opp_max", C.c_int32), ("n_cars", C.c_int32), ("degree", C.c_int32), ("pad", C.c_int32), ("lap_length", C.c_double),
                ("track_width", C.c_double), ("l_sum", C.c_double), ("w_sum", C.c_double)]


def stats_desc(n_opp_max, n_cars, lap_length, track_width, degree=6, l_sum=0.4, w_sum=0.2):
    """crx_stats_desc_default.  n_cars = 0: scripted opponents, n_opp_max of them per car; n_cars = C >= 1: field mode, n_opp_max >= C - 1."""
    return StatsDesc(int(n_opp_max), int(n_cars), int(degree), 0, float(lap_length), float(track_width), float(l_sum), float(w_sum))


# include/crx.h "Race statistics": the rows of stat_i [STATS_NI, batch] int32 and stat_d [STATS_ND + n_opp_max, batch] float64 ...
CRX_STATS_MAX_LAPS, CRX_STATS_MAX_OPP = 8, 32
STATS_I = dict(n_samples=0, nonfinite_step=1, off_step=2, off_samples=3, contact_step=4, contact_samples=5, n_laps=6, laps_prev=7,
               lap_step=8, passes=16, passed=17, flag_samples=18)          # lap_step: CRX_STATS_MAX_LAPS rows
STATS_NI = 19
STATS_D = dict(min_clear=0, ey_max=1, sum_ey2=2, sum_dv2=3, ds_prev=4)     # ds_prev: n_opp_max rows
STATS_ND = 4
# ... and of the summary record sum_i [n_groups, STATS_SUM_NI] int64, sum_d [n_groups, STATS_SUM_ND] float64
STATS_SUM_I = dict(cars=0, nonfinite=1, off=2, contact=3, clean=4, laps_hist=5, passes=14, passed=15, flag_samples=16, n_samples=17,
                   lap1_sum=18, lap1_min=19, lap1_max=20, lap1_count=21, lap2_sum=22, lap2_min=23, lap2_max=24, lap2_count=25)   # laps_hist: 9 bins
STATS_SUM_NI = 26
STATS_SUM_D = dict(min_clear=0, ey_max=1)
STATS_SUM_ND = 2

_PV, _PD = C.c_void_p, C.POINTER(StatsDesc)
STATS_ARGTYPES = {
    "stats_desc_default": [_PD, C.c_int, C.c_int, C.c_double, C.c_double],
    "race_stats_reset_dev": [_PD, C.c_int, _PV, _PV, _PV, _PV],
    "race_stats_dev": [_PD, C.c_int, C.c_int, C.c_double] + [_PV] * 12,
    "race_stats_laps_dev": [_PD, C.c_int, C.c_int, C.c_double] + [_PV] * 13,
    "race_stats_summary_dev": [_PD, C.c_int, _PV, C.c_int, _PV, _PV, _PV, _PV, _PV],
    "race_stats_reset": [_PD, C.c_int, _PV, _PV, _PV],
    "race_stats": [_PD, C.c_int, C.c_int, C.c_double] + [_PV] * 11,
    "race_stats_summary": [_PD, C.c_int, _PV, C.c_int, _PV, _PV, _PV, _PV],
}


def bind_stats(lib, prefix="crx_"):
    """argtypes / restype of the race-statistics family on a loaded library (the clock t travels as a double by value)."""
    for name, argtypes in STATS_ARGTYPES.items():
        fn = getattr(lib, prefix + name)
        fn.argtypes = argtypes
        fn.restype = None if name == "stats_desc_default" else C.c_int


# include/crx.h "Seed laps": the per-car phase and the bits of seed_status
SEED_PID, SEED_MPC, SEED_DONE, SEED_FAILED = 0, 1, 2, 3
CRX_SEED_MPC_FAILED, CRX_SEED_LOG_FULL = 1, 2
SEED_ARGTYPES = {
    "seed_commit_dev": [C.c_int, C.c_int] + [_PV] * 9,
    "seed_log_dev": [C.c_int, C.c_int, C.c_double] + [_PV] * 15,
}


def bind_seed(lib, prefix="crx_"):
    """argtypes / restype of the seed-lap entries on a loaded library (lap_length travels as a double by value)."""
    for name, argtypes in SEED_ARGTYPES.items():
        fn = getattr(lib, prefix + name)
        fn.argtypes = argtypes
        fn.restype = C.c_int


def stats_summary_record(sum_i, sum_d):
    """The summary arrays of one group as a dict by field name (laps_hist: the 9 bins)."""
    rec = {k: int(sum_i[i]) for k, i in STATS_SUM_I.items() if k != "laps_hist"}
    rec["laps_hist"] = [int(v) for v in sum_i[STATS_SUM_I["laps_hist"]:STATS_SUM_I["laps_hist"] + CRX_STATS_MAX_LAPS + 1]]
    rec.update({k: float(sum_d[i]) for k, i in STATS_SUM_D.items()})
    return rec


class SelectDesc(C.Structure):
    _fields_ = [
        ("N", C.c_int32),
        ("n_veh_max", C.c_int32),
        ("veh_length", C.c_double),
        ("veh_width", C.c_double),
        ("lap_length", C.c_double),
        ("w_prog", C.c_double),
        ("w_coll", C.c_double),
        ("w_switch", C.c_double),
    ]


def _arr(ctype, n, values):
    return (ctype * n)(*[float(v) for v in np.asarray(values, dtype=float).reshape(-1)])


def planner_desc(N, A, B, opts=None):
    """Constants hard-coded in the reference's planner (overtake_traj_planner.py:276-334,367)."""
    return PlannerDesc(
        int(N), 0, _arr(C.c_double, 36, A), _arr(C.c_double, 12, B),
        20.0, 30.0, 200.0, 5.0, 0.5, 1.5, 0.1, 1.1, opts or default_opts(),
    )


def cbf_desc(N, n_obs_max, A, B, Q=(10.0, 0.0, 0.0, 4.0, 0.0, 40.0), R=(0.1, 0.1), alpha=0.8,
             margin=0.2, ey_max=1.0, per_stage_target=False, delta_max=0.5, a_max=1.0, v_min=0.0,
             v_max=10.0, l_sum=0.4, w_sum=0.2, w_slack=1e4, degree=6, opts=None):
    """Defaults = MPCCBFRacingParam / SystemParam / CarParam (utils/base.py:272-291,708-713,699-705)
    and the literals in control.mpccbf (control.py:527-528,560).  Without `opts` the budgets follow the problem class like
    crx_cbf_desc_default (include/crx.h crx_ipm_opts.stall_iters): (50, 25) for N <= 12 with at most one obstacle slot, (100, 50) otherwise."""
    if opts is None:
        opts = default_opts(**cbf_class_budgets(N, n_obs_max))
    return CbfDesc(
        int(N), int(n_obs_max), int(bool(per_stage_target)), int(degree),
        _arr(C.c_double, 36, A), _arr(C.c_double, 12, B), _arr(C.c_double, 6, Q),
        _arr(C.c_double, 2, R), delta_max, a_max, v_min, v_max, ey_max, alpha, margin, l_sum,
        w_sum, w_slack, opts or default_opts(),
    )


def lmpc_desc(N=12, n_ss_max=44, Q=(0.0,) * 6, R=(1.0, 0.25), dR=(4.0, 0.0), x_track=(5.0, 0, 0, 0, 0, 0),
              v_max=10.0, ey_max=1.0, delta_max=0.5, a_max=1.0, w_x0=1e4, opts=None):
    """Defaults = LMPCRacingParam (utils/base.py:350-376), SystemParam (:708-713) and the literal
    x_track of control.lmpc (control.py:649)."""
    return LmpcDesc(int(N), int(n_ss_max), _arr(C.c_double, 6, Q), _arr(C.c_double, 2, R), _arr(C.c_double, 2, dR),
                    _arr(C.c_double, 6, x_track), v_max, ey_max, delta_max, a_max, w_x0, opts or default_opts())


def ilqr_desc(N, A, B, Q=np.diag([10.0, 0.0, 0.0, 4.0, 0.0, 40.0]), R=np.diag([0.1, 0.1]), max_iter=150, n_obs_max=1,
              eps=0.01, lamb_init=1.0, lamb_factor=10.0, lamb_max=1000.0, margin=0.15, q1=2.5, q2=2.5, l_sum=0.4, w_sum=0.2):
    """Defaults = iLQRRacingParam / CarParam (utils/base.py) and the literals of control.ilqr (control.py:80-83) and
    ilqr_helper.get_cost_derivation (ilqr_helper.py:25-27).  Q, R are full matrices (a 1-D argument is a diagonal)."""
    Q, R = np.asarray(Q, dtype=float), np.asarray(R, dtype=float)
    Q = np.diag(Q) if Q.ndim == 1 else Q
    R = np.diag(R) if R.ndim == 1 else R
    return IlqrDesc(int(N), int(max_iter), int(n_obs_max), 0, _arr(C.c_double, 36, A), _arr(C.c_double, 12, B),
                    _arr(C.c_double, 36, Q), _arr(C.c_double, 4, R), eps, lamb_init, lamb_factor, lamb_max, margin, q1, q2,
                    l_sum, w_sum)


def lqr_desc(Q=np.diag([10.0, 0.0, 0.0, 4.0, 0.0, 40.0]), R=np.diag([0.1, 0.1]), max_iter=50, eps=0.01):
    """Defaults = LQRTrackingParam (utils/base.py) and the literal eps of control.lqr (control.py:44).  Q, R are full matrices (a 1-D
    argument is a diagonal)."""
    Q, R = np.asarray(Q, dtype=float), np.asarray(R, dtype=float)
    Q = np.diag(Q) if Q.ndim == 1 else Q
    R = np.diag(R) if R.ndim == 1 else R
    return LqrDesc(int(max_iter), 0, _arr(C.c_double, 36, Q), _arr(C.c_double, 4, R), float(eps))


def lqr_models(A, B, batch=None):
    """(A [Bn,6,6], B [Bn,6,2]) float64 from one model (6,6), (6,2) -- repeated `batch` times when given -- or per-problem models."""
    A, B = np.asarray(A, dtype=_D), np.asarray(B, dtype=_D)
    if A.ndim == 2 and B.ndim == 2:
        A, B = A[None], B[None]
        if batch is not None:
            A, B = np.repeat(A, batch, axis=0), np.repeat(B, batch, axis=0)
    Bn = A.shape[0] if batch is None else batch
    return _in(A, _D, (Bn, 6, 6)), _in(B, _D, (Bn, 6, 2))


def cbf_models(models, batch):
    """(A [batch,6,6], B [batch,6,2]) contiguous float64 from a per-problem model pair of host arrays; anything else -- another
    shape, another dtype, not a pair -- is a ValueError (no silent conversion: a float32 model is a caller's mistake)."""
    try:
        A, B = models
    except (TypeError, ValueError):
        raise ValueError("models must be a pair (A [batch,6,6], B [batch,6,2])")
    A, B = np.asarray(A), np.asarray(B)
    if A.dtype != np.float64 or B.dtype != np.float64:
        raise ValueError("models must be float64, got %s, %s" % (A.dtype, B.dtype))
    return _in(A, _D, (batch, 6, 6)), _in(B, _D, (batch, 6, 2))


def sysid_desc(lamb=1e-9, first_row=1, chunk_rows=8192):
    """crx_sysid_desc_default: lamb of system_identification_test.py:42; first_row = 1 drops row 0 (S1)."""
    return SysidDesc(float(lamb), int(first_row), int(chunk_rows))


def sysid_offsets(x, offsets):
    """(x [rows,6], int64 log offsets [n_logs+1]) from a [T,6] log with offsets None, a [B,T,6] batch of equal logs, or packed rows
    with explicit offsets."""
    x = np.asarray(x, dtype=_D)
    if offsets is None:
        if x.ndim == 3:
            offsets = np.arange(x.shape[0] + 1, dtype=np.int64) * x.shape[1]
            x = x.reshape(-1, 6)
        else:
            offsets = np.array([0, x.shape[0]], dtype=np.int64)
    return x, np.ascontiguousarray(offsets, dtype=np.int64)


def prep_desc(N, n_veh_max, n_opt, track_width, lap_length, prediction_factor=0.5, veh_length=0.4, veh_width=0.2):
    """planner_helper.py:51-53 and overtake_traj_planner.py:288,296 literals."""
    return PrepDesc(int(N), int(n_veh_max), int(n_opt), 0, prediction_factor, 4.0, track_width, lap_length,
                    veh_length, veh_width, 0.15, 0.1)


def path_desc(N, alpha, w_rate=100.0, opts=None):
    """overtake_path_planner.py:246-253 literals."""
    return PathDesc(int(N), 0, float(alpha), float(w_rate), opts or default_opts())


def plant_desc(n_seg, lap_length, timestep=0.1, dt_sub=0.001):
    """BicycleDynamicsParam defaults (utils/base.py:686-697) and the sub-step loop of base.py:899-905."""
    n_sub = 0
    while (n_sub + 1) * dt_sub <= timestep:
        n_sub += 1
    D = 0.8 * 1.98 * 9.81 / 2.0
    return PlantDesc(n_sub, int(n_seg), dt_sub, lap_length, 1.98, 0.125, 0.125, 0.024, D, 1.25, 1.0, D, 1.25, 1.0)


CRX_PLANT_NPARAM = 10
PLANT_PARAM_NAMES = ("m", "lf", "lr", "Iz", "Df", "Cf", "Bf", "Dr", "Cr", "Br")   # BicycleDynamicsParam.get_params() (utils/base.py), = the PlantDesc fields


def plant_params(batch, dynamics_params=None):
    """[batch, 10] float64 rows (m, lf, lr, Iz, Df, Cf, Bf, Dr, Cr, Br) for the `params` argument of the plant entries: None = the
    BicycleDynamicsParam defaults for every car (the ten values of plant_desc), one object with get_params() = that set for every car, a
    sequence of `batch` such objects = one set per car."""
    if dynamics_params is None:
        d = plant_desc(1, 1.0)
        rows = [[getattr(d, n) for n in PLANT_PARAM_NAMES]] * batch
    elif hasattr(dynamics_params, "get_params"):
        rows = [list(dynamics_params.get_params())] * batch
    else:
        rows = [list(p.get_params()) for p in dynamics_params]
        if len(rows) != batch:
            raise ValueError("plant_params: %d parameter sets for %d cars" % (len(rows), batch))
    return _in(np.array(rows, dtype=np.float64).reshape(batch, CRX_PLANT_NPARAM), _D, (batch, CRX_PLANT_NPARAM))


CRX_MAX_TRACKS = 8
CRX_PLANT_MAX_SEG = 64


class TrackSet:
    """The track set of the plant's `tracks` entries (include/crx.h): tracks [n_tracks, seg_stride, 6] float64 (table t's rows
    n_seg[t] .. seg_stride - 1 are zero padding, never read), n_seg [n_tracks] int32, lap_length [n_tracks] float64."""

    def __init__(self, tracks, n_seg, lap_length):
        self.tracks, self.n_seg, self.lap_length = tracks, n_seg, lap_length
        self.n_tracks, self.seg_stride = int(tracks.shape[0]), int(tracks.shape[1])

    def table(self, t):
        """Track t's own rows [n_seg[t], 6], without the padding."""
        return self.tracks[t, :self.n_seg[t]]


def track_set(tables, lap_lengths, seg_stride=None):
    """TrackSet of a list of segment tables [n_seg_t, 6] (ClosedTrack.point_and_tangent) and their lap lengths.  seg_stride: rows per table
    in the packed array, default the longest table's.  Refuses more than CRX_MAX_TRACKS tracks, a table without rows or with more than
    seg_stride <= 64 of them, a row that has not 6 columns, and a lap length that is not positive and finite."""
    tables = list(tables)
    lap = np.ascontiguousarray(lap_lengths, dtype=np.float64).reshape(-1)
    if not 1 <= len(tables) <= CRX_MAX_TRACKS:
        raise ValueError("track_set: %d tracks outside [1, %d]" % (len(tables), CRX_MAX_TRACKS))
    if lap.shape[0] != len(tables):
        raise ValueError("track_set: %d lap lengths for %d tracks" % (lap.shape[0], len(tables)))
    rows = []
    for t, tab in enumerate(tables):
        try:
            a = np.array(tab, dtype=np.float64)
        except ValueError:
            raise ValueError("track_set: track %d is ragged, expected rows of 6 columns" % t) from None
        if a.ndim != 2 or a.shape[1] != 6 or a.shape[0] < 1:
            raise ValueError("track_set: track %d has shape %s, expected [n_seg >= 1, 6]" % (t, a.shape))
        rows.append(a)
    stride = max(a.shape[0] for a in rows) if seg_stride is None else int(seg_stride)
    if not 1 <= stride <= CRX_PLANT_MAX_SEG:
        raise ValueError("track_set: seg_stride %d outside [1, %d]" % (stride, CRX_PLANT_MAX_SEG))
    for t, a in enumerate(rows):
        if a.shape[0] > stride:
            raise ValueError("track_set: track %d has %d rows, more than seg_stride %d" % (t, a.shape[0], stride))
        if not (np.isfinite(lap[t]) and lap[t] > 0.0):
            raise ValueError("track_set: lap length of track %d must be positive and finite, got %r" % (t, float(lap[t])))
    tracks = np.zeros((len(rows), stride, 6))
    for t, a in enumerate(rows):
        tracks[t, :a.shape[0]] = a
    return TrackSet(tracks, np.array([a.shape[0] for a in rows], dtype=np.int32), lap)


def select_desc(N, n_veh_max, lap_length, veh_length=0.4, veh_width=0.2):
    """overtake_traj_planner.py:209,223,243 literals."""
    return SelectDesc(int(N), int(n_veh_max), veh_length, veh_width, lap_length, 10.0, 100.0, 100.0)


_D = np.float64
_I = np.int32


def _in(a, dtype, shape):
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.shape != tuple(shape):
        raise ValueError("expected shape %s, got %s" % (tuple(shape), a.shape))
    return a


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Binding:
    """Host-pointer entry points of a library exporting <prefix>planner_solve / cbf_solve / select."""

    def __init__(self, lib, prefix):
        self.lib, self.prefix = lib, prefix
        for name in ("planner_solve", "cbf_solve", "select", "lmpc_solve", "planner_prep", "plant_step", "path_solve", "ilqr_solve",
                     "ilqr_solve_models", "lqr_design", "sysid_fit", "cbf_solve_models", "planner_solve_models", "planner_plan",
                     "planner_plan_models", "path_prep", "path_plan", "plant_step_params", "field_prep", "field_traffic", "mixed_prep",
                     "plant_step_tracks", "field_prep_tracks", "mixed_prep_tracks"):
            if hasattr(lib, prefix + name):
                getattr(lib, prefix + name).restype = C.c_int
        if hasattr(lib, prefix + "race_stats_dev"):
            bind_stats(lib, prefix)
        if hasattr(lib, prefix + "seed_log_dev"):
            bind_seed(lib, prefix)
        self._check = None

    def race_stats_reset(self, desc, laps):
        """crx_race_stats_reset: (stat_i [STATS_NI, Bn] int32, stat_d [STATS_ND + n_opp_max, Bn] float64) at their reset values."""
        laps = np.ascontiguousarray(laps, dtype=_I)
        Bn = laps.shape[0]
        stat_i, stat_d = np.zeros((STATS_NI, Bn), dtype=_I), np.zeros((STATS_ND + desc.n_opp_max, Bn))
        self._call("race_stats_reset", C.byref(desc), Bn, _p(laps), _p(stat_i), _p(stat_d))
        return stat_i, stat_d

    def race_stats(self, desc, sample, t, xcurv, laps, stat_i, stat_d, car_s0=None, car_v=None, car_ey=None, n_opp=None, car_dims=None,
                   xt=None, flag=None):
        """crx_race_stats (include/crx.h S1-S4): one sample of every car; stat_i, stat_d (C-contiguous, as race_stats_reset returns
        them) are updated in place.  Optional arrays are passed as they are given -- the library refuses the combinations it does not take."""
        xcurv = np.ascontiguousarray(xcurv, dtype=_D).reshape(-1, 6)
        Bn, V = xcurv.shape[0], desc.n_opp_max
        opt = lambda a, dtype, shape: None if a is None else _p(_in(a, dtype, shape))   # noqa: E731
        if stat_i.dtype != _I or stat_d.dtype != _D or not stat_i.flags.c_contiguous or not stat_d.flags.c_contiguous \
                or stat_i.shape != (STATS_NI, Bn) or stat_d.shape != (STATS_ND + V, Bn):
            raise ValueError("stat_i, stat_d: expected C-contiguous int32 %s and float64 %s" % ((STATS_NI, Bn), (STATS_ND + V, Bn)))
        self._call("race_stats", C.byref(desc), Bn, int(sample), float(t), _p(xcurv), _p(_in(laps, _I, (Bn,))), opt(car_s0, _D, (Bn, V)),
                   opt(car_v, _D, (Bn, V)), opt(car_ey, _D, (Bn, V)), opt(n_opp, _I, (Bn,)),
                   None if car_dims is None else _p(_in(np.asarray(car_dims, dtype=_D).reshape(-1, 2), _D, (Bn, 2))), opt(xt, _D, (Bn, 6)),
                   opt(flag, _I, (Bn,)), _p(stat_i), _p(stat_d))
        return stat_i, stat_d

    def race_stats_summary(self, desc, stat_i, stat_d, group=None, n_groups=1):
        """crx_race_stats_summary: (sum_i [G, STATS_SUM_NI] int64, sum_d [G, STATS_SUM_ND] float64), G = n_groups with a group array, else 1."""
        Bn = stat_i.shape[1]
        G = max(int(n_groups), 1) if group is not None else 1
        sum_i, sum_d = np.zeros((G, STATS_SUM_NI), dtype=np.int64), np.zeros((G, STATS_SUM_ND))
        self._call("race_stats_summary", C.byref(desc), Bn, None if group is None else _p(_in(group, _I, (Bn,))), int(n_groups),
                   _p(np.ascontiguousarray(stat_i, dtype=_I)), _p(np.ascontiguousarray(stat_d, dtype=_D)), _p(sum_i), _p(sum_d))
        return sum_i, sum_d

    def _call(self, name, *args):
        rc = getattr(self.lib, self.prefix + name)(*args)
        if rc != 0:
            msg = ""
            if hasattr(self.lib, self.prefix + "last_error"):
                f = getattr(self.lib, self.prefix + "last_error")
                f.restype = C.c_char_p
                msg = (f() or b"").decode()
            raise RuntimeError("%s%s failed: rc=%d %s" % (self.prefix, name, rc, msg))

    def planner_solve(self, desc, x0, bez_s, bez_ey, ey_lb, ey_ub, models=None):
        """crx_planner_solve.  models = (A (Bn,6,6), B (Bn,6,2)) float64: crx_planner_solve_models, region QP b on its own model (desc.A,
        desc.B are ignored); a QP whose model has a non-finite entry reports CRX_SINGULAR with the fall-back trajectory and cost inf."""
        N = desc.N
        x0 = np.ascontiguousarray(x0, dtype=_D)
        Bn = x0.shape[0]
        x0 = _in(x0, _D, (Bn, 6))
        bez_s = _in(bez_s, _D, (Bn, N + 1))
        bez_ey = _in(bez_ey, _D, (Bn, N + 1))
        ey_lb = _in(ey_lb, _D, (Bn, N))
        ey_ub = _in(ey_ub, _D, (Bn,))
        out = dict(
            X=np.zeros((Bn, N + 1, 6)), U=np.zeros((Bn, N, 2)), cost=np.zeros(Bn),
            status=np.zeros(Bn, dtype=_I), kkt=np.zeros(Bn), iters=np.zeros(Bn, dtype=_I),
        )
        if models is not None:
            mA, mB = cbf_models(models, Bn)
            self._call(
                "planner_solve_models", C.byref(desc), C.c_int(Bn), _p(x0), _p(mA), _p(mB), _p(bez_s), _p(bez_ey), _p(ey_lb),
                _p(ey_ub), _p(out["X"]), _p(out["U"]), _p(out["cost"]), _p(out["status"]), _p(out["kkt"]), _p(out["iters"]),
            )
            return out
        self._call(
            "planner_solve", C.byref(desc), C.c_int(Bn), _p(x0), _p(bez_s), _p(bez_ey), _p(ey_lb),
            _p(ey_ub), _p(out["X"]), _p(out["U"]), _p(out["cost"]), _p(out["status"]),
            _p(out["kkt"]), _p(out["iters"]),
        )
        return out

    def ilqr_solve(self, desc, x0, xt, obs_s, obs_ey, lap_off, n_obs, models=None):
        """crx_ilqr_solve.  x0, xt (Bn,6); obs_s, obs_ey (Bn,V,N+1); lap_off (Bn,V); n_obs (Bn,) with V = desc.n_obs_max.
        models = (A (Bn,6,6), B (Bn,6,2)): crx_ilqr_solve_models, problem b on its own model (desc.A, desc.B are ignored).
        Returns X (Bn,N+1,6), U (Bn,N,2), cost, status, iters."""
        N, V = desc.N, desc.n_obs_max
        x0 = np.ascontiguousarray(x0, dtype=_D)
        Bn = x0.shape[0]
        x0 = _in(x0, _D, (Bn, 6))
        xt = _in(xt, _D, (Bn, 6))
        obs_s = _in(obs_s, _D, (Bn, V, N + 1))
        obs_ey = _in(obs_ey, _D, (Bn, V, N + 1))
        lap_off = _in(lap_off, _D, (Bn, V))
        n_obs = _in(n_obs, _I, (Bn,))
        out = dict(X=np.zeros((Bn, N + 1, 6)), U=np.zeros((Bn, N, 2)), cost=np.zeros(Bn), status=np.zeros(Bn, dtype=_I),
                   iters=np.zeros(Bn, dtype=_I))
        if models is not None:
            mA, mB = _in(models[0], _D, (Bn, 6, 6)), _in(models[1], _D, (Bn, 6, 2))
            self._call("ilqr_solve_models", C.byref(desc), C.c_int(Bn), _p(x0), _p(mA), _p(mB), _p(xt), _p(obs_s), _p(obs_ey),
                       _p(lap_off), _p(n_obs), _p(out["X"]), _p(out["U"]), _p(out["cost"]), _p(out["status"]), _p(out["iters"]))
            return out
        self._call("ilqr_solve", C.byref(desc), C.c_int(Bn), _p(x0), _p(xt), _p(obs_s), _p(obs_ey), _p(lap_off), _p(n_obs),
                   _p(out["X"]), _p(out["U"]), _p(out["cost"]), _p(out["status"]), _p(out["iters"]))
        return out

    def lqr_design(self, desc, A, B, want_P=True):
        """crx_lqr_design.  A (Bn,6,6), B (Bn,6,2), or one model (6,6), (6,2).  Returns K (Bn,2,6), P (Bn,6,6) (the P behind K;
        absent with want_P False), iters, status."""
        A, B = lqr_models(A, B)
        Bn = A.shape[0]
        out = dict(K=np.zeros((Bn, 2, 6)), iters=np.zeros(Bn, dtype=_I), status=np.zeros(Bn, dtype=_I))
        if want_P:
            out["P"] = np.zeros((Bn, 6, 6))
        self._call("lqr_design", C.byref(desc), C.c_int(Bn), _p(A), _p(B), _p(out["K"]), _p(out["P"]) if want_P else None,
                   _p(out["iters"]), _p(out["status"]))
        return out

    def sysid_fit(self, desc, x, u, offsets=None, group_offsets=None):
        """crx_sysid_fit.  x [rows,6], u [rows,2] packed logs with int64 offsets [n_logs+1] (or a [T,6] log / [B,T,6] batch and
        offsets None); group_offsets int32 [n_groups+1] or None (one fit per log).  Returns A (G,6,6), B (G,6,2), err (G,2,6),
        n_pairs (G,) int64, status (G,)."""
        x, offsets = sysid_offsets(x, offsets)
        u = np.asarray(u, dtype=_D).reshape(-1, 2)
        n_logs = offsets.shape[0] - 1
        x = _in(x, _D, (x.shape[0], 6))
        u = _in(u, _D, (x.shape[0], 2))
        go = None
        if group_offsets is not None:
            go = np.ascontiguousarray(group_offsets, dtype=_I)
        G = n_logs if go is None else go.shape[0] - 1
        out = dict(A=np.zeros((G, 6, 6)), B=np.zeros((G, 6, 2)), err=np.zeros((G, 2, 6)), n_pairs=np.zeros(G, dtype=np.int64),
                   status=np.zeros(G, dtype=_I))
        self._call("sysid_fit", C.byref(desc), C.c_int(n_logs), _p(offsets), _p(go) if go is not None else None, C.c_int(G), _p(x),
                   _p(u), _p(out["A"]), _p(out["B"]), _p(out["err"]), _p(out["n_pairs"]), _p(out["status"]))
        return out

    def cbf_solve(self, desc, x0, xt, obs_s, obs_ey, lap_off, n_obs, obs_dims=None, models=None):
        """crx_cbf_solve; with obs_dims (Bn, V, 2) = (l_agent + l_obs, w_agent + w_obs) per obstacle slot: crx_cbf_solve_dims.
        models = (A (Bn,6,6), B (Bn,6,2)) float64: crx_cbf_solve_models, problem b on its own model (desc.A, desc.B are ignored); a
        problem whose model has a non-finite entry reports CRX_SINGULAR with NaN outputs."""
        N, V = desc.N, desc.n_obs_max
        x0 = np.ascontiguousarray(x0, dtype=_D)
        Bn = x0.shape[0]
        x0 = _in(x0, _D, (Bn, 6))
        xt = _in(xt, _D, (Bn, N + 1, 6) if desc.per_stage_target else (Bn, 6))
        obs_s = _in(obs_s, _D, (Bn, V, N + 1))
        obs_ey = _in(obs_ey, _D, (Bn, V, N + 1))
        lap_off = _in(lap_off, _D, (Bn, V))
        n_obs = _in(n_obs, _I, (Bn,))
        out = dict(
            X=np.zeros((Bn, N + 1, 6)), U=np.zeros((Bn, N, 2)), sigma=np.zeros((Bn, V, N + 1)),
            cost=np.zeros(Bn), status=np.zeros(Bn, dtype=_I), kkt=np.zeros(Bn),
            iters=np.zeros(Bn, dtype=_I),
        )
        if models is not None:
            mA, mB = cbf_models(models, Bn)
            if obs_dims is not None:
                obs_dims = _in(obs_dims, _D, (Bn, V, 2))
            self._call(
                "cbf_solve_models", C.byref(desc), C.c_int(Bn), _p(x0), _p(mA), _p(mB), _p(xt), _p(obs_s), _p(obs_ey),
                _p(lap_off), _p(n_obs), _p(obs_dims) if obs_dims is not None else None, _p(out["X"]), _p(out["U"]), _p(out["sigma"]),
                _p(out["cost"]), _p(out["status"]), _p(out["kkt"]), _p(out["iters"]),
            )
            return out
        if obs_dims is not None:
            obs_dims = _in(obs_dims, _D, (Bn, V, 2))
            self._call(
                "cbf_solve_dims", C.byref(desc), C.c_int(Bn), _p(x0), _p(xt), _p(obs_s), _p(obs_ey),
                _p(lap_off), _p(n_obs), _p(obs_dims), _p(out["X"]), _p(out["U"]), _p(out["sigma"]), _p(out["cost"]),
                _p(out["status"]), _p(out["kkt"]), _p(out["iters"]),
            )
            return out
        self._call(
            "cbf_solve", C.byref(desc), C.c_int(Bn), _p(x0), _p(xt), _p(obs_s), _p(obs_ey),
            _p(lap_off), _p(n_obs), _p(out["X"]), _p(out["U"]), _p(out["sigma"]), _p(out["cost"]),
            _p(out["status"]), _p(out["kkt"]), _p(out["iters"]),
        )
        return out

    def select(self, desc, n_veh, X, obs_s, obs_ey, old_flag):
        N, V = desc.N, desc.n_veh_max
        n_veh = np.ascontiguousarray(n_veh, dtype=_I)
        S = n_veh.shape[0]
        X = _in(X, _D, (S, V + 1, N + 1, 6))
        obs_s = _in(obs_s, _D, (S, V, N + 1))
        obs_ey = _in(obs_ey, _D, (S, V, N + 1))
        old_flag = _in(old_flag, _I, (S,))
        out = dict(flag=np.zeros(S, dtype=_I), sel_cost=np.zeros((S, V + 1)), best_X=np.zeros((S, N + 1, 6)))
        self._call(
            "select", C.byref(desc), C.c_int(S), _p(n_veh), _p(X), _p(obs_s), _p(obs_ey),
            _p(old_flag), _p(out["flag"]), _p(out["sel_cost"]), _p(out["best_X"]),
        )
        return out

    def planner_plan(self, desc, sdesc, x0, bez_s, bez_ey, ey_lb, ey_ub, n_veh, obs_s, obs_ey, old_flag, models=None):
        """Fused planner step (crx_planner_plan): all region QPs of every scenario + the selection.
        Arrays of the QP part have leading dimension S*(V+1), scenario-major.  Only libcrx exports it;
        the oracle composes planner_solve + select (tests compare the two).
        models = (A (S,6,6), B (S,6,2)) float64, one model per SCENARIO: crx_planner_plan_models, every region QP of scenario i on
        model i (expanded here to the C ABI's one model per region QP; desc.A, desc.B are ignored)."""
        N, V = desc.N, sdesc.n_veh_max
        n_veh = np.ascontiguousarray(n_veh, dtype=_I)
        S = n_veh.shape[0]
        Bn = S * (V + 1)
        x0 = _in(x0, _D, (Bn, 6))
        bez_s = _in(bez_s, _D, (Bn, N + 1))
        bez_ey = _in(bez_ey, _D, (Bn, N + 1))
        ey_lb = _in(ey_lb, _D, (Bn, N))
        ey_ub = _in(ey_ub, _D, (Bn,))
        obs_s = _in(obs_s, _D, (S, V, N + 1))
        obs_ey = _in(obs_ey, _D, (S, V, N + 1))
        old_flag = _in(old_flag, _I, (S,))
        out = dict(
            X=np.zeros((Bn, N + 1, 6)), U=np.zeros((Bn, N, 2)), cost=np.zeros(Bn),
            status=np.zeros(Bn, dtype=_I), kkt=np.zeros(Bn), iters=np.zeros(Bn, dtype=_I),
            flag=np.zeros(S, dtype=_I), sel_cost=np.zeros((S, V + 1)), best_X=np.zeros((S, N + 1, 6)),
        )
        if models is not None:
            mA, mB = cbf_models(models, S)
            mA, mB = np.repeat(mA, V + 1, axis=0), np.repeat(mB, V + 1, axis=0)
            self._call(
                "planner_plan_models", C.byref(desc), C.byref(sdesc), C.c_int(S), _p(x0), _p(mA), _p(mB), _p(bez_s), _p(bez_ey),
                _p(ey_lb), _p(ey_ub), _p(n_veh), _p(obs_s), _p(obs_ey), _p(old_flag), _p(out["X"]),
                _p(out["U"]), _p(out["cost"]), _p(out["status"]), _p(out["kkt"]), _p(out["iters"]),
                _p(out["flag"]), _p(out["sel_cost"]), _p(out["best_X"]),
            )
            return out
        self._call(
            "planner_plan", C.byref(desc), C.byref(sdesc), C.c_int(S), _p(x0), _p(bez_s), _p(bez_ey),
            _p(ey_lb), _p(ey_ub), _p(n_veh), _p(obs_s), _p(obs_ey), _p(old_flag), _p(out["X"]),
            _p(out["U"]), _p(out["cost"]), _p(out["status"]), _p(out["kkt"]), _p(out["iters"]),
            _p(out["flag"]), _p(out["sel_cost"]), _p(out["best_X"]),
        )
        return out

    def lmpc_solve(self, desc, x0, u_old, A, B, Cm, ss, qfun, n_ss=None):
        """crx_lmpc_solve.  A (Bn,N,6,6), B (Bn,N,6,2), Cm (Bn,N,6), ss (Bn,6,M), qfun (Bn,M)."""
        N, M = desc.N, desc.n_ss_max
        x0 = np.ascontiguousarray(x0, dtype=_D)
        Bn = x0.shape[0]
        x0 = _in(x0, _D, (Bn, 6))
        u_old = _in(u_old, _D, (Bn, 2))
        A = _in(np.asarray(A, dtype=_D).reshape(Bn, N, 36), _D, (Bn, N, 36))
        B = _in(np.asarray(B, dtype=_D).reshape(Bn, N, 12), _D, (Bn, N, 12))
        Cm = _in(np.asarray(Cm, dtype=_D).reshape(Bn, N, 6), _D, (Bn, N, 6))
        ss = _in(ss, _D, (Bn, 6, M))
        qfun = _in(qfun, _D, (Bn, M))
        n_ss = np.full(Bn, M, dtype=_I) if n_ss is None else _in(n_ss, _I, (Bn,))
        out = dict(
            X=np.zeros((Bn, N + 1, 6)), U=np.zeros((Bn, N, 2)), lam=np.zeros((Bn, M)), cost=np.zeros(Bn),
            status=np.zeros(Bn, dtype=_I), kkt=np.zeros(Bn), iters=np.zeros(Bn, dtype=_I),
        )
        self._call(
            "lmpc_solve", C.byref(desc), C.c_int(Bn), _p(x0), _p(u_old), _p(A), _p(B), _p(Cm), _p(ss), _p(qfun),
            _p(n_ss), _p(out["X"]), _p(out["U"]), _p(out["lam"]), _p(out["cost"]), _p(out["status"]),
            _p(out["kkt"]), _p(out["iters"]),
        )
        return out

    def lmpc_prep(self, desc, ss_xcurv, u_ss, qfun, time_ss, it, x, lin_points, lin_input, track, from_plan=False, seed=None):
        """crx_lmpc_prep: stage models + safe-set selection.  ss_xcurv (Bn,L,P,6), u_ss (Bn,L,P,2), qfun (Bn,L,P).
        A, B, C are in/out (a singular stage keeps its three regression rows): `seed` = (A, B, C) to start from, else zeros."""
        N, P, L, M = desc.N, desc.n_points, desc.n_laps, desc.n_ss_per_lap * desc.n_ss_laps
        x = np.ascontiguousarray(x, dtype=_D)
        Bn = x.shape[0]
        ss_xcurv, u_ss, qfun = _in(ss_xcurv, _D, (Bn, L, P, 6)), _in(u_ss, _D, (Bn, L, P, 2)), _in(qfun, _D, (Bn, L, P))
        time_ss, it, x = _in(time_ss, _I, (Bn, L)), _in(it, _I, (Bn,)), _in(x, _D, (Bn, 6))
        lin_points, lin_input = _in(lin_points, _D, (Bn, N + 1, 6)), _in(lin_input, _D, (Bn, N, 2))
        track = _in(track, _D, (desc.n_seg, 6))
        out = dict(A=np.zeros((Bn, N, 6, 6)), B=np.zeros((Bn, N, 6, 2)), C=np.zeros((Bn, N, 6)), ss=np.zeros((Bn, 6, M)),
                   qfun=np.zeros((Bn, M)), status=np.zeros(Bn, dtype=_I))
        if seed is not None:
            out["A"], out["B"], out["C"] = (_in(a, _D, out[k].shape).copy() for k, a in zip("ABC", seed))
        getattr(self.lib, self.prefix + "lmpc_prep").restype = C.c_int
        self._call("lmpc_prep", C.byref(desc), C.c_int(Bn), _p(ss_xcurv), _p(u_ss), _p(qfun), _p(time_ss), _p(it), _p(x),
                   _p(lin_points), _p(lin_input), C.c_int(int(bool(from_plan))), _p(track), _p(out["A"]), _p(out["B"]),
                   _p(out["C"]), _p(out["ss"]), _p(out["qfun"]), _p(out["status"]))
        return out

    def planner_scene(self, desc, ego_xcurv, n_all, veh_xcurv, pred_s, pred_ey):
        """crx_planner_scene: interest test, partial sort, veh_infos, max_delta_v, predictions in sorted order."""
        N1, VA, V = desc.N + 1, desc.n_all_max, desc.n_veh_max
        n_all = np.ascontiguousarray(n_all, dtype=_I)
        S = n_all.shape[0]
        ego_xcurv, veh_xcurv = _in(ego_xcurv, _D, (S, 6)), _in(veh_xcurv, _D, (S, VA, 6))
        pred_s, pred_ey = _in(pred_s, _D, (S, VA, N1)), _in(pred_ey, _D, (S, VA, N1))
        out = dict(n_veh=np.zeros(S, dtype=_I), overflow=np.zeros(S, dtype=_I), order=np.zeros((S, V), dtype=_I), veh_info=np.zeros((S, V, 3)),
                   max_dv=np.zeros(S), obs_s=np.zeros((S, V, N1)), obs_ey=np.zeros((S, V, N1)))
        getattr(self.lib, self.prefix + "planner_scene").restype = C.c_int
        self._call("planner_scene", C.byref(desc), C.c_int(S), _p(ego_xcurv), _p(n_all), _p(veh_xcurv), _p(pred_s), _p(pred_ey),
                   _p(out["n_veh"]), _p(out["overflow"]), _p(out["order"]), _p(out["veh_info"]), _p(out["max_dv"]), _p(out["obs_s"]),
                   _p(out["obs_ey"]))
        return out

    def planner_prep(self, desc, x_wrapped, x_raw, n_veh, veh_info, max_dv, obs_s, obs_ey, opt_s, opt_ey):
        """crx_planner_prep: Bezier references + ey bounds of every region, in crx_planner_solve's layout."""
        N, V, T = desc.N, desc.n_veh_max, desc.n_opt
        n_veh = np.ascontiguousarray(n_veh, dtype=_I)
        S = n_veh.shape[0]
        R = V + 1
        x_wrapped, x_raw = _in(x_wrapped, _D, (S, 6)), _in(x_raw, _D, (S, 6))
        veh_info = _in(veh_info, _D, (S, V, 3))
        max_dv = _in(max_dv, _D, (S,))
        obs_s, obs_ey = _in(obs_s, _D, (S, V, N + 1)), _in(obs_ey, _D, (S, V, N + 1))
        opt_s, opt_ey = _in(opt_s, _D, (T,)), _in(opt_ey, _D, (T,))
        out = dict(x0=np.zeros((S * R, 6)), bez_s=np.zeros((S * R, N + 1)), bez_ey=np.zeros((S * R, N + 1)),
                   ey_lb=np.zeros((S * R, N)), ey_ub=np.zeros(S * R))
        self._call("planner_prep", C.byref(desc), C.c_int(S), _p(x_wrapped), _p(x_raw), _p(n_veh), _p(veh_info),
                   _p(max_dv), _p(obs_s), _p(obs_ey), _p(opt_s), _p(opt_ey), _p(out["x0"]), _p(out["bez_s"]),
                   _p(out["bez_ey"]), _p(out["ey_lb"]), _p(out["ey_ub"]))
        return out

    def plant_step(self, desc, track, xglob, xcurv, u, params=None):
        """crx_plant_step: one control step of the zero-noise plant for a batch of vehicles.  params [Bn,10] float64 (plant_params):
        crx_plant_step_params, vehicle b on its own BicycleDynamicsParam set (desc's ten values are ignored); a row with m <= 0, Iz <= 0
        or a non-finite value is refused."""
        xglob = np.ascontiguousarray(xglob, dtype=_D)
        Bn = xglob.shape[0]
        track = _in(track, _D, (desc.n_seg, 6))
        xglob, xcurv, u = _in(xglob, _D, (Bn, 6)), _in(xcurv, _D, (Bn, 6)), _in(u, _D, (Bn, 2))
        out = dict(xglob=np.zeros((Bn, 6)), xcurv=np.zeros((Bn, 6)))
        if params is not None:
            params = _in(params, _D, (Bn, CRX_PLANT_NPARAM))
            self._call("plant_step_params", C.byref(desc), C.c_int(Bn), _p(track), _p(xglob), _p(xcurv), _p(u), _p(params),
                       _p(out["xglob"]), _p(out["xcurv"]))
            return out
        self._call("plant_step", C.byref(desc), C.c_int(Bn), _p(track), _p(xglob), _p(xcurv), _p(u), _p(out["xglob"]),
                   _p(out["xcurv"]))
        return out

    def plant_step_tracks(self, desc, tracks, track_id, xglob, xcurv, u, params=None):
        """crx_plant_step_tracks: the zero-noise step with vehicle b on track track_id[b] of the TrackSet `tracks` (track_set); desc's
        n_seg and lap_length are not used.  A track_id outside [0, n_tracks) is refused, as a bad params row is."""
        xglob = np.ascontiguousarray(xglob, dtype=_D)
        Bn = xglob.shape[0]
        tab = _in(tracks.tracks, _D, (tracks.n_tracks, tracks.seg_stride, 6))
        n_seg, lap = _in(tracks.n_seg, _I, (tracks.n_tracks,)), _in(tracks.lap_length, _D, (tracks.n_tracks,))
        track_id = _in(track_id, _I, (Bn,))
        xglob, xcurv, u = _in(xglob, _D, (Bn, 6)), _in(xcurv, _D, (Bn, 6)), _in(u, _D, (Bn, 2))
        if params is not None:
            params = _in(params, _D, (Bn, CRX_PLANT_NPARAM))
        out = dict(xglob=np.zeros((Bn, 6)), xcurv=np.zeros((Bn, 6)))
        self._call("plant_step_tracks", C.byref(desc), C.c_int(Bn), C.c_int(tracks.n_tracks), C.c_int(tracks.seg_stride), _p(tab), _p(n_seg),
                   _p(lap), _p(track_id), _p(xglob), _p(xcurv), _p(u), None if params is None else _p(params), _p(out["xglob"]),
                   _p(out["xcurv"]))
        return out

    @staticmethod
    def _race_track_args(tracks, race_track, xcurv, n_cars):
        """The arguments that stand in place of `track` in the `tracks` entries of the field families: n_tracks, seg_stride, the set's three
        arrays and race_track (R,), R read off xcurv as the entries' wrappers read it."""
        R = np.asarray(xcurv).size // (6 * n_cars)
        return [C.c_int(tracks.n_tracks), C.c_int(tracks.seg_stride), _in(tracks.tracks, _D, (tracks.n_tracks, tracks.seg_stride, 6)),
                _in(tracks.n_seg, _I, (tracks.n_tracks,)), _in(tracks.lap_length, _D, (tracks.n_tracks,)), _in(race_track, _I, (R,))]

    def field_prep(self, desc, track, xcurv, car_dims=None, clear=True):
        """crx_field_prep (include/crx.h F1-F7): the predictions of every car of every race and the obstacle arrays of the R * C NLPs.
        track (n_seg,6); xcurv (R,C,6) or (R*C,6); car_dims (R,C,2) = (length, width) per car, or None.  Returns pred_s, pred_ey
        (R,C,N+1), obs_s, obs_ey (R,C,V,N+1), lap_off (R,C,V), n_obs (R,C) with V = C - 1; obs_dims (R,C,V,2) with car_dims; clear (R,C)
        unless clear is False."""
        return self._field_prep("field_prep", [_in(track, _D, (desc.n_seg, 6))], desc, xcurv, car_dims, clear)

    def field_prep_tracks(self, desc, tracks, race_track, xcurv, car_dims=None, clear=True):
        """crx_field_prep_tracks: field_prep with race r on track race_track[r] of the TrackSet `tracks` (track_set); race_track (R,) int32;
        desc's n_seg and lap_length are not used.  A race_track outside [0, n_tracks) is refused."""
        return self._field_prep("field_prep_tracks", self._race_track_args(tracks, race_track, xcurv, desc.n_cars), desc, xcurv, car_dims, clear)

    def _field_prep(self, entry, track_args, desc, xcurv, car_dims, clear):
        """field_prep / field_prep_tracks: track_args, c_ints and arrays, is what the entry takes between n_races and xcurv."""
        N1, Cn = desc.N + 1, desc.n_cars
        V = Cn - 1
        xcurv = np.ascontiguousarray(xcurv, dtype=_D)
        R = xcurv.size // (6 * Cn)
        xcurv = _in(xcurv.reshape(R, Cn, 6), _D, (R, Cn, 6))
        out = dict(pred_s=np.zeros((R, Cn, N1)), pred_ey=np.zeros((R, Cn, N1)), obs_s=np.zeros((R, Cn, V, N1)), obs_ey=np.zeros((R, Cn, V, N1)),
                   lap_off=np.zeros((R, Cn, V)), n_obs=np.zeros((R, Cn), dtype=_I))
        if car_dims is not None:
            car_dims = _in(car_dims, _D, (R, Cn, 2))
            out["obs_dims"] = np.zeros((R, Cn, V, 2))
        if clear:
            out["clear"] = np.zeros((R, Cn))
        self._call(entry, C.byref(desc), C.c_int(R), *[a if isinstance(a, C.c_int) else _p(a) for a in track_args], _p(xcurv),
                   _p(car_dims) if car_dims is not None else None, *[_p(out[k]) for k in ("pred_s", "pred_ey", "obs_s", "obs_ey", "lap_off", "n_obs")],
                   _p(out["obs_dims"]) if car_dims is not None else None, _p(out["clear"]) if clear else None)
        return out

    def field_traffic(self, desc, track, xcurv):
        """crx_field_traffic (include/crx.h "Field games", F1-F3, F6, G1-G3): the racing game's traffic arrays when every car of a race plays
        it.  track (n_seg,6); xcurv (R,C,6) or (R*C,6).  Returns pred_s_car, pred_ey_car (R,C,N+1): every car's zero-input roll-out; veh_xcurv
        (R*C,V,6), pred_s, pred_ey (R*C,V,N+1), n_all (R*C,) with V = C - 1: per ego the other cars of its race in car order, the inputs of
        planner_scene for R*C scenarios."""
        N1, Cn = desc.N + 1, desc.n_cars
        V = Cn - 1
        track = _in(track, _D, (desc.n_seg, 6))
        xcurv = np.ascontiguousarray(xcurv, dtype=_D)
        R = xcurv.size // (6 * Cn)
        xcurv = _in(xcurv.reshape(R, Cn, 6), _D, (R, Cn, 6))
        out = dict(pred_s_car=np.zeros((R, Cn, N1)), pred_ey_car=np.zeros((R, Cn, N1)), veh_xcurv=np.zeros((R * Cn, V, 6)),
                   pred_s=np.zeros((R * Cn, V, N1)), pred_ey=np.zeros((R * Cn, V, N1)), n_all=np.zeros(R * Cn, dtype=_I))
        self._call("field_traffic", C.byref(desc), C.c_int(R), _p(track), _p(xcurv),
                   *[_p(out[k]) for k in ("pred_s_car", "pred_ey_car", "veh_xcurv", "pred_s", "pred_ey", "n_all")])
        return out

    def mixed_prep(self, desc, track, xcurv, policy, car_dims=None, clear=True):
        """crx_mixed_prep (include/crx.h "Mixed fields"): the roll-out of every car of every race and the solver inputs of each car's own policy.
        track (n_seg,6); xcurv (R,C,6) or (R*C,6); policy (R,C) codes or names; car_dims (R,C,2) or None.  Returns pred_s, pred_ey
        (R,C,NP+1), NP = max(N, N_ilqr); obs_s, obs_ey (R,C,V,N+1), lap_off (R,C,V), n_obs, m_nlp (R,C), obs_dims (R,C,V,2) with car_dims; with
        N_ilqr > 0 il_obs_s, il_obs_ey (R,C,V,N_ilqr+1), il_lap_off (R,C,V), il_n_obs, m_ilqr (R,C); clear (R,C) unless clear is False."""
        return self._mixed_prep("mixed_prep", [_in(track, _D, (desc.n_seg, 6))], desc, xcurv, policy, car_dims, clear)

    def mixed_prep_tracks(self, desc, tracks, race_track, xcurv, policy, car_dims=None, clear=True):
        """crx_mixed_prep_tracks: mixed_prep with race r on track race_track[r] of the TrackSet `tracks` (track_set); race_track (R,) int32;
        desc's n_seg and lap_length are not used.  A race_track outside [0, n_tracks) is refused."""
        return self._mixed_prep("mixed_prep_tracks", self._race_track_args(tracks, race_track, xcurv, desc.n_cars), desc, xcurv, policy, car_dims,
                                clear)

    def _mixed_prep(self, entry, track_args, desc, xcurv, policy, car_dims, clear):
        """mixed_prep / mixed_prep_tracks: track_args as in _field_prep."""
        N1, NI1, Cn = desc.N + 1, desc.N_ilqr + 1, desc.n_cars
        V, NP1 = Cn - 1, max(N1, NI1)
        xcurv = np.ascontiguousarray(xcurv, dtype=_D)
        R = xcurv.size // (6 * Cn)
        xcurv = _in(xcurv.reshape(R, Cn, 6), _D, (R, Cn, 6))
        policy = _in(policy_codes(policy), _I, (R, Cn))
        out = dict(pred_s=np.zeros((R, Cn, NP1)), pred_ey=np.zeros((R, Cn, NP1)), obs_s=np.zeros((R, Cn, V, N1)), obs_ey=np.zeros((R, Cn, V, N1)),
                   lap_off=np.zeros((R, Cn, V)), n_obs=np.zeros((R, Cn), dtype=_I), m_nlp=np.zeros((R, Cn), dtype=_I))
        if car_dims is not None:
            car_dims = _in(car_dims, _D, (R, Cn, 2))
            out["obs_dims"] = np.zeros((R, Cn, V, 2))
        if desc.N_ilqr > 0:
            out.update(il_obs_s=np.zeros((R, Cn, V, NI1)), il_obs_ey=np.zeros((R, Cn, V, NI1)), il_lap_off=np.zeros((R, Cn, V)),
                       il_n_obs=np.zeros((R, Cn), dtype=_I), m_ilqr=np.zeros((R, Cn), dtype=_I))
        if clear:
            out["clear"] = np.zeros((R, Cn))
        opt = lambda k: _p(out[k]) if k in out else None   # noqa: E731
        self._call(entry, C.byref(desc), C.c_int(R), *[a if isinstance(a, C.c_int) else _p(a) for a in track_args], _p(xcurv), _p(policy),
                   _p(car_dims) if car_dims is not None else None,
                   *[opt(k) for k in ("pred_s", "pred_ey", "obs_s", "obs_ey", "lap_off", "n_obs", "obs_dims", "m_nlp", "il_obs_s", "il_obs_ey",
                                      "il_lap_off", "il_n_obs", "m_ilqr", "clear")])
        return out

    def path_solve(self, desc, opt, bez, lb, ub, e0, eN):
        """crx_path_solve: the 1-D QPs of the overtake path planner, one per candidate region."""
        N = desc.N
        e0 = np.ascontiguousarray(e0, dtype=_D)
        Bn = e0.shape[0]
        opt, bez, lb, ub = (_in(a, _D, (Bn, N + 1)) for a in (opt, bez, lb, ub))
        e0, eN = _in(e0, _D, (Bn,)), _in(eN, _D, (Bn,))
        out = dict(E=np.zeros((Bn, N + 1)), cost=np.zeros(Bn), status=np.zeros(Bn, dtype=_I), kkt=np.zeros(Bn),
                   iters=np.zeros(Bn, dtype=_I))
        self._call("path_solve", C.byref(desc), C.c_int(Bn), _p(opt), _p(bez), _p(lb), _p(ub), _p(e0), _p(eN), _p(out["E"]),
                   _p(out["cost"]), _p(out["status"]), _p(out["kkt"]), _p(out["iters"]))
        return out

    def _path_inputs(self, desc, x_wrapped, x_raw, n_veh, order, veh_xcurv, max_dv, obs_ey, opt_s, opt_ey):
        N, V, VA, T = desc.N, desc.n_veh_max, desc.n_all_max, desc.n_opt
        n_veh = np.ascontiguousarray(n_veh, dtype=_I)
        S = n_veh.shape[0]
        return S, (_in(x_wrapped, _D, (S, 6)), _in(x_raw, _D, (S, 6)), n_veh, _in(order, _I, (S, V)), _in(veh_xcurv, _D, (S, VA, 6)),
                   _in(max_dv, _D, (S,)), _in(obs_ey, _D, (S, V, N + 1)), _in(opt_s, _D, (T,)), _in(opt_ey, _D, (T,)))

    def path_prep(self, desc, x_wrapped, x_raw, n_veh, order, veh_xcurv, max_dv, obs_ey, opt_s, opt_ey):
        """crx_path_prep (include/crx.h P1-P6): from the outputs of planner_scene to the arrays of path_solve, every region of every
        scenario.  Returns opt, bez, lb, ub (S*(V+1), N+1), e0, eN (S*(V+1),), span (S,); a scenario without vehicles keeps the NaN the
        arrays are created with."""
        S, ins = self._path_inputs(desc, x_wrapped, x_raw, n_veh, order, veh_xcurv, max_dv, obs_ey, opt_s, opt_ey)
        Bn, N1 = S * (desc.n_veh_max + 1), desc.N + 1
        out = dict(opt=np.full((Bn, N1), np.nan), bez=np.full((Bn, N1), np.nan), lb=np.full((Bn, N1), np.nan), ub=np.full((Bn, N1), np.nan),
                   e0=np.full(Bn, np.nan), eN=np.full(Bn, np.nan), span=np.full(S, np.nan))
        self._call("path_prep", C.byref(desc), C.c_int(S), *[_p(a) for a in ins], *[_p(out[k]) for k in ("opt", "bez", "lb", "ub", "e0", "eN", "span")])
        return out

    def path_plan(self, desc, qdesc, x_wrapped, x_raw, n_veh, order, veh_xcurv, max_dv, obs_ey, opt_s, opt_ey, opt_vx, active=None, target=None):
        """crx_path_plan (include/crx.h P1-P8): prep, the region QPs and the selection with its target trajectory.  active (S,) int32 or
        None; target (S, N+1, 6): what the skipped scenarios keep (default NaN).  Returns E (S*(V+1), N+1), cost, status, kkt, iters
        (S*(V+1),), flag (S,), target (S, N+1, 6), plan_status (S,)."""
        S, ins = self._path_inputs(desc, x_wrapped, x_raw, n_veh, order, veh_xcurv, max_dv, obs_ey, opt_s, opt_ey)
        Bn, N1 = S * (desc.n_veh_max + 1), desc.N + 1
        opt_vx = _in(opt_vx, _D, (desc.n_opt,))
        if active is not None:
            active = _in(active, _I, (S,))
        out = dict(E=np.full((Bn, N1), np.nan), cost=np.zeros(Bn), status=np.zeros(Bn, dtype=_I), kkt=np.full(Bn, np.nan),
                   iters=np.zeros(Bn, dtype=_I), flag=np.zeros(S, dtype=_I),
                   target=np.full((S, N1, 6), np.nan) if target is None else _in(target, _D, (S, N1, 6)).copy(),
                   plan_status=np.zeros(S, dtype=_I))
        self._call("path_plan", C.byref(desc), C.byref(qdesc), C.c_int(S), _p(active) if active is not None else None, *[_p(a) for a in ins],
                   _p(opt_vx), *[_p(out[k]) for k in ("E", "cost", "status", "kkt", "iters", "flag", "target", "plan_status")])
        return out
