"""A/B of two builds of the C ABI layer (csrc/crx_api.hip), not of the kernels: what a build REFUSES and what it RETURNS.
Usage: [CRX_LIB=...] python tools/abi_ab.py TAG;  python tools/abi_ab.py --compare A B   (dumps under tools/ab/, or ABI_AB_OUT=DIR)

Part 1, refusals: a fixed table of malformed calls against every host-pointer entry point and the _dev entry points of the same
families (the masked / ordered / dims / wrap / noise variants included) -- a NULL descriptor, every out-of-range descriptor field
the library tests, a negative batch, each NULL array, out-of-range per-element values (host-pointer side) and the empty call.
One line per call: (return code, crx_last_error()).  Every entry of the table is refused -- or, for the empty call, answered --
before any launch, so nothing here reaches a kernel; as a second line of defence the _dev calls carry the address of one zeroed
device block.  Without a GPU the table still runs: the families that look at the device first all answer CRX_ERR_NOT_INIT; the field
families (crx_field_prep, crx_field_traffic, crx_mixed_prep, crx_mixed_commit_dev) refuse on their arguments alone, with calls that have two
things wrong at once to pin the order of their checks.
Part 2, results (GPU only): each of the 12 host-pointer entry points once on a small valid input (the synthetic draws and
tests/golden/*.npz, as smoke() uses them), every output array dumped; crx_lmpc_prep with a non-zero seed for A, B, C.
--compare: the two dumps line for line and array for array, bit for bit; exit status 1 on any difference."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, ROOT + "/car-racing_amd"]
OUT = os.path.join(os.environ.get("ABI_AB_OUT") or ROOT + "/tools/ab", "abi_ab_%s")   # dumps: git-ignored; ABI_AB_OUT=DIR puts them elsewhere
if sys.argv[1] == "--compare":
    ta, tb = sys.argv[2], sys.argv[3]
    la, lb = open(OUT % ta + ".txt").read().splitlines(), open(OUT % tb + ".txt").read().splitlines()
    diff = [i for i in range(max(len(la), len(lb))) if i >= len(la) or i >= len(lb) or la[i] != lb[i]]
    for i in diff[:20]:
        print("  line %d:\n    %s\n    %s" % (i + 1, la[i] if i < len(la) else "-", lb[i] if i < len(lb) else "-"))
    print("refusals: %d lines of %s, %d of %s: %s" % (len(la), ta, len(lb), tb, "IDENTICAL" if not diff else "%d DIFFERENT" % len(diff)))
    bad = []
    if os.path.exists(OUT % ta + ".npz") or os.path.exists(OUT % tb + ".npz"):
        a, b = np.load(OUT % ta + ".npz"), np.load(OUT % tb + ".npz")
        bad = [k for k in sorted(set(a.files) | set(b.files)) if k not in a.files or k not in b.files or a[k].tobytes() != b[k].tobytes()]
        print("results: %d arrays of %s, %d of %s: %s" % (len(a.files), ta, len(b.files), tb, "IDENTICAL" if not bad else "DIFFERENT in %s" % bad))
    else:
        print("results: not dumped (no GPU)")
    sys.exit(1 if diff or bad else 0)

import crx   # noqa: E402
from crx import abi, synth   # noqa: E402

TAG = sys.argv[1]
L = crx.lib()
HAVE_GPU = L.crx_device_count() > 0
gpu = crx.init(0) if HAVE_GPU else None
A, B = synth.load_AB()
D, I, Q = np.float64, np.int32, np.int64
if HAVE_GPU:
    import torch
    _block = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")   # every _dev array argument: never reached, but valid if it were
    DEV = _block.data_ptr()
else:
    _block = np.zeros(4096, dtype=np.uint8)
    DEV = _block.ctypes.data
lines = []


def z(*shape, dtype=D):
    return np.zeros(shape, dtype=dtype)


class NullDesc:
    pass


def marshal(v, dev):
    if v is None or isinstance(v, NullDesc):
        return None
    if isinstance(v, np.ndarray):
        return C.c_void_p(DEV if dev else v.ctypes.data)
    if isinstance(v, C.Structure):
        return C.byref(v)
    if isinstance(v, float):
        return C.c_double(v)
    if isinstance(v, tuple):      # ("i64", value), ("size", value), ("ptr", address)
        return {"i64": C.c_int64, "size": C.c_size_t, "ptr": C.c_void_p}[v[0]](v[1])
    return C.c_int(v)


def call(entry, sig, vals, label, dev):
    fn = getattr(L, entry)
    fn.restype = C.c_int
    rc = fn(*[marshal(vals.get(k), dev) for k in sig])
    lines.append("%-30s %-44s rc=%d %s" % (entry, label, rc, (L.crx_last_error() or b"").decode() if rc else ""))


def copy_vals(vals):
    out = {}
    for k, v in vals.items():
        if isinstance(v, np.ndarray):
            out[k] = v.copy()
        elif isinstance(v, C.Structure):
            out[k] = type(v).from_buffer_copy(v)
        else:
            out[k] = v
    return out


def setf(desc_key, path, value):
    def m(v):
        o = v[desc_key]
        *head, last = path.split(".")
        for h in head:
            o = getattr(o, h)
        if "[" in last:
            name, idx = last[:-1].split("[")
            getattr(o, name)[int(idx)] = value
        else:
            setattr(o, last, value)
    return m


def setv(key, value):
    def m(v):
        v[key] = value
    return m


def setel(key, idx, value):
    def m(v):
        v[key].reshape(-1)[idx] = value
    return m


OPTS = [("tol", 0.0), ("max_iter", 0), ("mu_init", 0.0), ("tau_min", 0.0), ("tau_min", 1.0), ("slack_push", 0.0), ("kappa_mu", 0.0), ("kappa_mu", 1.0),
        ("theta_mu", 1.0), ("grad_scale_max", 0.0), ("slack_start", -1), ("slack_start", 4), ("dual_inf_tol", 0.0), ("constr_viol_tol", 0.0),
        ("compl_inf_tol", 0.0), ("stall_iters", 0), ("qp_method", -1), ("qp_method", 2)]


def family(good, entries, fields, arrays, batch_key="batch", desc_key="d", host_cases=(), dev_cases=()):
    """entries: [(symbol, signature, is_dev)].  fields: [(path, value)] on the descriptor.  arrays: the names whose NULL is refused."""
    for entry, sig, dev in entries:
        cases = [("desc NULL", setv(desc_key, NullDesc()))]
        cases += [("%s=%r" % f, setf(desc_key, *f)) for f in fields]
        cases += [("%s=-1" % batch_key, setv(batch_key, -1)), ("%s=0" % batch_key, setv(batch_key, 0)),
                  ("%s=0, arrays NULL" % batch_key, lambda v: [v.update({k: None for k in arrays}), v.update({batch_key: 0})])]
        cases += [("%s NULL" % a, setv(a, None)) for a in arrays if a in sig]
        cases += list(dev_cases if dev else host_cases)
        for label, mut in cases:
            if isinstance(mut, tuple):      # (only for these entries, mutation)
                if entry not in mut[0]:
                    continue
                mut = mut[1]
            v = copy_vals(good)
            mut(v)
            call(entry, sig, v, label, dev)


# ---- planner ----------------------------------------------------------------------------------------------------------
N = 10
pl_arr = ["x0", "bez_s", "bez_ey", "ey_lb", "ey_ub", "X", "U", "cost", "status", "kkt", "iters"]
pl_good = dict(d=abi.planner_desc(N, A, B), batch=1, x0=z(1, 6), bez_s=z(1, N + 1), bez_ey=z(1, N + 1), ey_lb=z(1, N), ey_ub=z(1), X=z(1, N + 1, 6),
               U=z(1, N, 2), cost=z(1), status=z(1, dtype=I), kkt=z(1), iters=z(1, dtype=I))
family(pl_good, [("crx_planner_solve", ["d", "batch"] + pl_arr, False), ("crx_planner_solve_dev", ["d", "batch"] + pl_arr + ["stream"], True)],
       [("N", 2), ("N", 25)] + [("opts." + k, v) for k, v in OPTS], pl_arr)

# ---- MPC-CBF ----------------------------------------------------------------------------------------------------------
cb_in, cb_out = ["x0", "xt", "obs_s", "obs_ey", "lap_off", "n_obs"], ["X", "U", "sigma", "cost", "status", "kkt", "iters"]
cb_good = dict(d=abi.cbf_desc(N, 1, A, B), batch=1, x0=z(1, 6), xt=z(1, 6), obs_s=z(1, 1, N + 1), obs_ey=z(1, 1, N + 1), lap_off=z(1, 1),
               n_obs=z(1, dtype=I), obs_dims=np.ones((1, 1, 2)), X=z(1, N + 1, 6), U=z(1, N, 2), sigma=z(1, 1, N + 1), cost=z(1), status=z(1, dtype=I),
               kkt=z(1), iters=z(1, dtype=I))
cb_good["n_obs"][0] = 1
family(cb_good,
       [("crx_cbf_solve", ["d", "batch"] + cb_in + cb_out, False),
        ("crx_cbf_solve_dims", ["d", "batch"] + cb_in + ["obs_dims"] + cb_out, False),
        ("crx_cbf_solve_dev", ["d", "batch"] + cb_in + cb_out + ["stream"], True),
        ("crx_cbf_solve_masked_dev", ["d", "batch", "active"] + cb_in + cb_out + ["stream"], True),
        ("crx_cbf_solve_dims_dev", ["d", "batch", "active"] + cb_in + ["obs_dims"] + cb_out + ["stream"], True),
        ("crx_cbf_solve_ordered_dev", ["d", "batch", "active", "order"] + cb_in + ["obs_dims"] + cb_out + ["stream"], True)],
       [("N", 2), ("N", 25), ("n_obs_max", -1), ("n_obs_max", 7), ("degree", 0), ("degree", 3), ("degree", 10), ("alpha", 0.0), ("alpha", 1.5),
        ("opts.tol", 0.0), ("opts.qp_method", 2)], cb_in + cb_out,
       host_cases=[("n_obs[0]=-1", setel("n_obs", 0, -1)), ("n_obs[0]=2", setel("n_obs", 0, 2)),
                   ("obs_dims[0][0]=(0,1)", (("crx_cbf_solve_dims",), setel("obs_dims", 0, 0.0))),
                   ("obs_dims[0][0]=(1,-1)", (("crx_cbf_solve_dims",), setel("obs_dims", 1, -1.0)))])

# ---- selection --------------------------------------------------------------------------------------------------------
V = 2
se_arr = ["n_veh", "X", "obs_s", "obs_ey", "old_flag", "flag", "sel_cost", "best_X"]
se_good = dict(d=abi.select_desc(N, V, 20.0), n_scen=1, n_veh=z(1, dtype=I), X=z(1, V + 1, N + 1, 6), obs_s=z(1, V, N + 1), obs_ey=z(1, V, N + 1),
               old_flag=z(1, dtype=I), flag=z(1, dtype=I), sel_cost=z(1, V + 1), best_X=z(1, N + 1, 6))
se_fields = [("N", 0), ("N", 25), ("n_veh_max", -1), ("n_veh_max", 7), ("lap_length", 0.0), ("lap_length", float("inf")), ("veh_length", -1.0),
             ("veh_width", -1.0)]
nveh_cases = [("n_veh[0]=-1", setel("n_veh", 0, -1)), ("n_veh[0]=3", setel("n_veh", 0, V + 1))]
family(se_good, [("crx_select", ["d", "n_scen"] + se_arr, False), ("crx_select_dev", ["d", "n_scen"] + se_arr + ["stream"], True)], se_fields, se_arr,
       batch_key="n_scen", host_cases=nveh_cases)

# ---- fused planner step: two descriptors ------------------------------------------------------------------------------
R = V + 1
pp_in = ["x0", "bez_s", "bez_ey", "ey_lb", "ey_ub", "n_veh", "obs_s", "obs_ey", "old_flag"]
pp_out = ["X", "U", "cost", "status", "kkt", "iters", "flag", "sel_cost", "best_X"]
pp_good = dict(d=abi.planner_desc(N, A, B), sd=abi.select_desc(N, V, 20.0), n_scen=1, x0=z(R, 6), bez_s=z(R, N + 1), bez_ey=z(R, N + 1), ey_lb=z(R, N),
               ey_ub=z(R), n_veh=z(1, dtype=I), obs_s=z(1, V, N + 1), obs_ey=z(1, V, N + 1), old_flag=z(1, dtype=I), X=z(R, N + 1, 6), U=z(R, N, 2),
               cost=z(R), status=z(R, dtype=I), kkt=z(R), iters=z(R, dtype=I), flag=z(1, dtype=I), sel_cost=z(1, R), best_X=z(1, N + 1, 6))
pp_entries = [("crx_planner_plan", ["d", "sd", "n_scen"] + pp_in + pp_out, False),
              ("crx_planner_plan_dev", ["d", "sd", "n_scen"] + pp_in + pp_out + ["stream"], True),
              ("crx_planner_plan_masked_dev", ["d", "sd", "n_scen", "active"] + pp_in + pp_out + ["stream"], True)]
# (the _dev entry points look at the selection's arrays only after the QP launch: their table stops at the planner's arrays)
family(pp_good, pp_entries[:1], [("N", 12), ("opts.tol", 0.0)], pp_in + pp_out, batch_key="n_scen", host_cases=nveh_cases)
family(pp_good, pp_entries[1:], [("N", 12), ("opts.tol", 0.0)], pl_arr, batch_key="n_scen",
       dev_cases=[("n_scen * (n_veh_max + 1) overflows", setv("n_scen", 1 << 30))])
family(pp_good, pp_entries, [("N", 11)] + se_fields[2:], [], batch_key="n_scen", desc_key="sd")
for entry, sig, dev in pp_entries:
    v = copy_vals(pp_good)
    v["d"].N = v["sd"].N = 2       # the horizons agree, the selection admits 2, the planner QP does not
    call(entry, sig, v, "both N=2", dev)

# ---- overtake path QP ---------------------------------------------------------------------------------------------------
pa_arr = ["opt", "bez", "lb", "ub", "e0", "eN", "E", "cost", "status", "kkt", "iters"]
pa_good = dict(d=abi.path_desc(N, 0.5), batch=1, opt=z(1, N + 1), bez=z(1, N + 1), lb=z(1, N + 1), ub=z(1, N + 1), e0=z(1), eN=z(1), E=z(1, N + 1),
               cost=z(1), status=z(1, dtype=I), kkt=z(1), iters=z(1, dtype=I))
family(pa_good, [("crx_path_solve", ["d", "batch"] + pa_arr, False), ("crx_path_solve_dev", ["d", "batch"] + pa_arr + ["stream"], True)],
       [("N", 1), ("N", 25), ("alpha", -0.1), ("alpha", 1.1), ("w_rate", -1.0), ("opts.max_iter", 0)], pa_arr)

# ---- plant ------------------------------------------------------------------------------------------------------------
pt_arr = ["track", "xglob", "xcurv", "u", "xglob_next", "xcurv_next"]
pt_good = dict(d=abi.plant_desc(4, 20.0), batch=1, track=z(4, 6), xglob=z(1, 6), xcurv=z(1, 6), u=z(1, 2), u_stride=2, xglob_next=z(1, 6),
               xcurv_next=z(1, 6), laps=z(1, dtype=I))
family(pt_good,
       [("crx_plant_step", ["d", "batch"] + pt_arr, False), ("crx_plant_step_dev", ["d", "batch"] + pt_arr + ["stream"], True),
        ("crx_plant_step_wrap_dev", ["d", "batch", "track", "xglob", "xcurv", "u", "u_stride", "xglob_next", "xcurv_next", "laps", "stream"], True),
        ("crx_plant_step_noise_dev", ["d", "batch", "track", "xglob", "xcurv", "u", "u_stride", "noise_z", "xglob_next", "xcurv_next", "laps", "stream"], True)],
       [("n_sub", -1), ("n_seg", 0), ("n_seg", 65), ("lap_length", 0.0), ("m", 0.0), ("Iz", 0.0)], pt_arr,
       dev_cases=[("u_stride=1", (("crx_plant_step_wrap_dev", "crx_plant_step_noise_dev"), setv("u_stride", 1)))])

# ---- planner prep -----------------------------------------------------------------------------------------------------
pr_sig = ["x_wrapped", "x_raw", "n_veh", "veh_info", "max_dv", "obs_s", "obs_ey", "opt_s", "opt_ey", "x0", "bez_s", "bez_ey", "ey_lb", "ey_ub"]
pr_good = dict(d=abi.prep_desc(N, V, 5, 1.0, 20.0), n_scen=1, x_wrapped=z(1, 6), x_raw=z(1, 6), n_veh=z(1, dtype=I), veh_info=z(1, V, 3), max_dv=z(1),
               obs_s=z(1, V, N + 1), obs_ey=z(1, V, N + 1), opt_s=z(5), opt_ey=z(5), x0=z(R, 6), bez_s=z(R, N + 1), bez_ey=z(R, N + 1), ey_lb=z(R, N),
               ey_ub=z(R))
family(pr_good, [("crx_planner_prep", ["d", "n_scen"] + pr_sig, False), ("crx_planner_prep_dev", ["d", "n_scen"] + pr_sig + ["stream"], True)],
       [("N", 2), ("N", 25), ("n_veh_max", -1), ("n_veh_max", 7), ("n_opt", 1), ("lap_length", 0.0), ("track_width", 0.0)], pr_sig, batch_key="n_scen",
       host_cases=nveh_cases)

# ---- learning-MPC QP --------------------------------------------------------------------------------------------------
NL, M = 4, 4
lm_sig = ["x0", "u_old", "A", "B", "C", "ss", "qfun", "n_ss", "X", "U", "lambda", "cost", "status", "kkt", "iters"]
lm_good = dict(d=abi.lmpc_desc(NL, M), batch=1, x0=z(1, 6), u_old=z(1, 2), A=z(1, NL, 36), B=z(1, NL, 12), C=z(1, NL, 6), ss=z(1, 6, M), qfun=z(1, M),
               n_ss=np.full(1, M, dtype=I), X=z(1, NL + 1, 6), U=z(1, NL, 2), cost=z(1), status=z(1, dtype=I), kkt=z(1), iters=z(1, dtype=I))
lm_good["lambda"] = z(1, M)
family(lm_good,
       [("crx_lmpc_solve", ["d", "batch"] + lm_sig, False), ("crx_lmpc_solve_dev", ["d", "batch"] + lm_sig + ["stream"], True),
        ("crx_lmpc_solve_masked_dev", ["d", "batch", "active"] + lm_sig + ["stream"], True),
        ("crx_lmpc_solve_ordered_dev", ["d", "batch", "active", "order"] + lm_sig + ["stream"], True)],
       [("N", 1), ("N", 17), ("n_ss_max", 0), ("n_ss_max", 61), ("R[0]", 0.0), ("R[1]", 0.0), ("dR[0]", -1.0), ("dR[1]", -1.0), ("Q[3]", -1.0), ("w_x0", 0.0),
        ("opts.stall_iters", 0)], lm_sig, host_cases=[("n_ss[0]=0", setel("n_ss", 0, 0)), ("n_ss[0]=5", setel("n_ss", 0, M + 1))])

# ---- learning-MPC prep ------------------------------------------------------------------------------------------------
P, LAPS = 8, 2
lp_sig = ["ss_xcurv", "u_ss", "qfun", "time_ss", "iter", "x", "lin_points", "lin_input", "from_plan", "track", "A", "B", "C", "ss_sel", "q_sel", "status"]
lp_arr = [k for k in lp_sig if k != "from_plan"]
lp_good = dict(d=abi.lmpcprep_desc(NL, P, LAPS, 4, 0.1, 20.0, n_ss_per_lap=2, n_ss_laps=2, max_neighbours=4), batch=1, ss_xcurv=z(1, LAPS, P, 6),
               u_ss=z(1, LAPS, P, 2), qfun=z(1, LAPS, P), time_ss=np.full((1, LAPS), P, dtype=I), iter=np.full(1, 2, dtype=I), x=z(1, 6),
               lin_points=z(1, NL + 1, 6), lin_input=z(1, NL, 2), from_plan=0, track=z(4, 6), A=z(1, NL, 36), B=z(1, NL, 12), C=z(1, NL, 6), ss_sel=z(1, 6, 4),
               q_sel=z(1, 4), status=z(1, dtype=I))
family(lp_good,
       [("crx_lmpc_prep", ["d", "batch"] + lp_sig, False), ("crx_lmpc_prep_dev", ["d", "batch"] + lp_sig + ["stream"], True),
        ("crx_lmpc_prep_masked_dev", ["d", "batch", "active"] + lp_sig + ["stream"], True)],
       [("N", 1), ("N", 17), ("n_points", 1), ("n_points", 65536), ("n_points", 65535), ("n_laps", 1), ("n_ss_laps", 0), ("n_ss_laps", 3), ("n_ss_per_lap", 0),
        ("n_ss_per_lap", 31), ("max_neighbours", 0), ("max_neighbours", 65), ("n_seg", 0), ("bandwidth", 0.0), ("dt", 0.0), ("lap_length", 0.0),
        ("lap_length", float("inf"))], lp_arr,
       host_cases=[("iter[0]=1", setel("iter", 0, 1)), ("iter[0]=3", setel("iter", 0, 3)), ("time_ss[0][0]=1", setel("time_ss", 0, 1)),
                   ("time_ss[0][1]=9", setel("time_ss", 1, P + 1))])

# ---- iLQR (argument errors come before the device check) --------------------------------------------------------------
NI = 5
il_sig = ["x0", "xt", "obs_s", "obs_ey", "lap_off", "n_obs", "X", "U", "cost", "status", "iters"]
il_good = dict(d=abi.ilqr_desc(NI, A, B), batch=1, x0=z(1, 6), xt=z(1, 6), obs_s=z(1, 1, NI + 1), obs_ey=z(1, 1, NI + 1), lap_off=z(1, 1), n_obs=z(1, dtype=I),
               X=z(1, NI + 1, 6), U=z(1, NI, 2), cost=z(1), status=z(1, dtype=I), iters=z(1, dtype=I))
family(il_good, [("crx_ilqr_solve", ["d", "batch"] + il_sig, False), ("crx_ilqr_solve_dev", ["d", "batch", "active"] + il_sig + ["stream"], True)],
       [("N", 0), ("N", 65), ("n_obs_max", -1), ("n_obs_max", 7), ("max_iter", -1), ("lamb_init", 0.0), ("lamb_factor", 0.0), ("eps", -1.0), ("l_sum", 0.0),
        ("w_sum", 0.0)], il_sig, host_cases=[("n_obs[0]=-1", setel("n_obs", 0, -1)), ("n_obs[0]=2", setel("n_obs", 0, 2))])

# ---- system identification (likewise) -----------------------------------------------------------------------------------
sy_out = ["A", "B", "err", "n_pairs", "status"]
sy_good = dict(d=abi.sysid_desc(), n_logs=2, log_offset=np.array([0, 5, 10], dtype=Q), group_offset=np.array([0, 1, 2], dtype=I), n_groups=2,
               max_log_rows=("i64", 5), x=z(10, 6), u=z(10, 2), workspace=z(1024), ws_bytes=("size", 8192), A=z(2, 36), B=z(2, 12), err=z(2, 12),
               n_pairs=z(2, dtype=Q), status=z(2, dtype=I))
sy_host = ["d", "n_logs", "log_offset", "group_offset", "n_groups", "x", "u"] + sy_out
sy_dev = ["d", "n_logs", "log_offset", "group_offset", "n_groups", "max_log_rows", "x", "u", "workspace", "ws_bytes"] + sy_out + ["stream"]
family(sy_good, [("crx_sysid_fit", sy_host, False), ("crx_sysid_fit_dev", sy_dev, True)],
       [("lamb", -1.0), ("lamb", float("inf")), ("first_row", -1), ("chunk_rows", 128), ("chunk_rows", 300), ("chunk_rows", 131072)],
       ["log_offset", "x", "u"] + sy_out, batch_key="n_groups",
       host_cases=[("n_logs=-1", setv("n_logs", -1)), ("group_offset NULL, n_groups=1", lambda v: v.update(group_offset=None, n_groups=1)),
                   ("log_offset[0]=-1", setel("log_offset", 0, -1)), ("log_offset decreases", setel("log_offset", 1, 12)),
                   ("group_offset[0]=1", setel("group_offset", 0, 1)), ("group_offset[n_groups]=1", setel("group_offset", 2, 1)),
                   ("group_offset decreases", lambda v: v["group_offset"].__setitem__(slice(None), [0, 3, 2]))],
       dev_cases=[("n_logs=-1", setv("n_logs", -1)), ("group_offset NULL, n_groups=1", lambda v: v.update(group_offset=None, n_groups=1)),
                  ("max_log_rows=-1", setv("max_log_rows", ("i64", -1))), ("n_logs * tiles overflows", setv("max_log_rows", ("i64", 1 << 43))),
                  ("workspace NULL", setv("workspace", None)), ("ws_bytes=0", setv("ws_bytes", ("size", 0))), ("x misaligned", setv("x", ("ptr", DEV + 8)))])

# ---- planner scene ----------------------------------------------------------------------------------------------------
VA = 4
sc_sig = ["ego_xcurv", "n_all", "veh_xcurv", "pred_s", "pred_ey", "n_veh", "overflow", "order", "veh_info", "max_dv", "obs_s", "obs_ey"]
sc_good = dict(d=abi.scene_desc(N, VA, V, 20.0), n_scen=1, ego_xcurv=z(1, 6), n_all=z(1, dtype=I), veh_xcurv=z(1, VA, 6), pred_s=z(1, VA, N + 1),
               pred_ey=z(1, VA, N + 1), n_veh=z(1, dtype=I), overflow=z(1, dtype=I), order=z(1, V, dtype=I), veh_info=z(1, V, 3), max_dv=z(1),
               obs_s=z(1, V, N + 1), obs_ey=z(1, V, N + 1))
family(sc_good, [("crx_planner_scene", ["d", "n_scen"] + sc_sig, False), ("crx_planner_scene_dev", ["d", "n_scen"] + sc_sig + ["stream"], True)],
       [("N", 0), ("N", 25), ("n_all_max", 0), ("n_all_max", 65), ("n_veh_max", 0), ("n_veh_max", 7), ("lap_length", 0.0), ("lap_length", float("inf"))],
       sc_sig, batch_key="n_scen", host_cases=[("n_all[0]=-1", setel("n_all", 0, -1)), ("n_all[0]=5", setel("n_all", 0, VA + 1))])

# ---- fields of driven cars: field prep, field traffic, mixed prep (arguments first, the device after), mixed commit ----------------
RF, CF, NS, NIL = 2, 3, 4, 5
BF, VF = RF * CF, CF - 1
fd_fields = [("N", 0), ("N", 25), ("n_cars", 0), ("n_cars", 8), ("n_seg", 0), ("n_seg", 65), ("degree", 0), ("degree", 3), ("degree", 10),
             ("lap_length", 0.0), ("lap_length", float("inf")), ("dt", 0.0), ("l_sum", 0.0), ("w_sum", float("nan"))]
fp_arr = ["track", "xcurv", "car_dims", "pred_s", "pred_ey", "obs_s", "obs_ey", "lap_off", "n_obs", "obs_dims"]
fp_good = dict(d=abi.field_desc(N, CF, NS, 20.0), n_races=RF, track=z(NS, 6), xcurv=z(BF, 6), car_dims=np.ones((RF, CF, 2)), pred_s=z(BF, N + 1),
               pred_ey=z(BF, N + 1), obs_s=z(BF, VF, N + 1), obs_ey=z(BF, VF, N + 1), lap_off=z(BF, VF), n_obs=z(BF, dtype=I), obs_dims=z(BF, VF, 2),
               clear=z(BF))
# (two things wrong at once: the order of the checks decides which message wins)
dims_cases = [("car_dims, obs_dims NULL", lambda v: v.update(car_dims=None, obs_dims=None)),
              ("n_cars=1, obs arrays NULL", lambda v: [setf("d", "n_cars", 1)(v), v.update(obs_s=None, obs_ey=None, lap_off=None, obs_dims=None)]),
              ("n_cars=0, n_races=-1", lambda v: [setf("d", "n_cars", 0)(v), v.update(n_races=-1)]),
              ("obs_dims NULL, xcurv NULL", lambda v: v.update(obs_dims=None, xcurv=None))]
host_dims_cases = [("car_dims[0][1]=(0,1)", setel("car_dims", 2, 0.0)), ("car_dims[1][2]=(1,inf)", setel("car_dims", 11, float("inf"))),
                   ("car_dims[0][0]=(-1,1), pred_s NULL", lambda v: [setel("car_dims", 0, -1.0)(v), v.update(pred_s=None)])]
family(fp_good, [("crx_field_prep", ["d", "n_races"] + fp_arr + ["clear"], False), ("crx_field_prep_dev", ["d", "n_races"] + fp_arr + ["clear", "stream"], True)],
       fd_fields, fp_arr, batch_key="n_races", host_cases=dims_cases + host_dims_cases, dev_cases=dims_cases)
ft_arr = ["track", "xcurv", "pred_s_car", "pred_ey_car", "veh_xcurv", "pred_s", "pred_ey", "n_all"]
ft_good = dict(d=abi.field_desc(N, CF, NS, 20.0), n_races=RF, track=z(NS, 6), xcurv=z(BF, 6), pred_s_car=z(BF, N + 1), pred_ey_car=z(BF, N + 1),
               veh_xcurv=z(BF, VF, 6), pred_s=z(BF, VF, N + 1), pred_ey=z(BF, VF, N + 1), n_all=z(BF, dtype=I))
family(ft_good, [("crx_field_traffic", ["d", "n_races"] + ft_arr, False), ("crx_field_traffic_dev", ["d", "n_races"] + ft_arr + ["stream"], True)],
       fd_fields, ft_arr, batch_key="n_races",
       host_cases=[("n_cars=1, per-ego arrays NULL", lambda v: [setf("d", "n_cars", 1)(v), v.update(veh_xcurv=None, pred_s=None, pred_ey=None)])])
mp_arr = ["track", "xcurv", "policy", "car_dims", "pred_s", "pred_ey", "obs_s", "obs_ey", "lap_off", "n_obs", "obs_dims", "m_nlp", "il_obs_s", "il_obs_ey",
          "il_lap_off", "il_n_obs", "m_ilqr"]
mp_good = dict(fp_good, d=abi.mixed_desc(N, NIL, CF, NS, 20.0), policy=z(BF, dtype=I), pred_s=z(BF, N + 1), pred_ey=z(BF, N + 1), m_nlp=z(BF, dtype=I),
               il_obs_s=z(BF, VF, NIL + 1), il_obs_ey=z(BF, VF, NIL + 1), il_lap_off=z(BF, VF), il_n_obs=z(BF, dtype=I), m_ilqr=z(BF, dtype=I))
il_null = dict(il_obs_s=None, il_obs_ey=None, il_lap_off=None, il_n_obs=None, m_ilqr=None)
mixed_cases = dims_cases + [("N_ilqr=0, iLQR arrays NULL", lambda v: [setf("d", "N_ilqr", 0)(v), v.update(il_null)]),
                            ("N_ilqr=-1, n_cars=0", lambda v: [setf("d", "N_ilqr", -1)(v), setf("d", "n_cars", 0)(v)]),
                            ("ilqr_obstacles=2, dt=0", lambda v: [setf("d", "ilqr_obstacles", 2)(v), setf("d", "dt", 0.0)(v)]),
                            ("m_ilqr NULL, m_nlp NULL", lambda v: v.update(m_ilqr=None, m_nlp=None)),
                            ("n_cars=1, [V] arrays NULL", lambda v: [setf("d", "n_cars", 1)(v), v.update(obs_s=None, obs_ey=None, lap_off=None, obs_dims=None,
                                                                                                       il_obs_s=None, il_obs_ey=None, il_lap_off=None)])]
family(mp_good, [("crx_mixed_prep", ["d", "n_races"] + mp_arr + ["clear"], False), ("crx_mixed_prep_dev", ["d", "n_races"] + mp_arr + ["clear", "stream"], True)],
       fd_fields + [("N_ilqr", -1), ("N_ilqr", 65), ("ilqr_obstacles", -1), ("ilqr_obstacles", 2)], mp_arr, batch_key="n_races",
       host_cases=mixed_cases + host_dims_cases + [("policy[0]=-1", setel("policy", 0, -1)), ("policy[5]=6", setel("policy", 5, 6)),
                                                   ("car_dims[0][0]=(0,1), il_n_obs NULL", lambda v: [setel("car_dims", 0, 0.0)(v), v.update(il_n_obs=None)]),
                                                   ("car_dims[0][0]=(0,1), policy[0]=9", lambda v: [setel("car_dims", 0, 0.0)(v), setel("policy", 0, 9)(v)])],
       dev_cases=mixed_cases)
mc_sig = ["batch", "policy", "x", "vt", "eyt", "K", "xt", "U_nlp", "nlp_stride", "nlp_status", "U_ilqr", "ilqr_stride", "ilqr_status", "u", "ctrl_status", "stream"]
mc_good = dict(batch=BF, policy=z(BF, dtype=I), x=z(BF, 6), vt=z(BF), eyt=z(BF), K=z(BF, 2, 6), xt=z(BF, 6), U_nlp=z(BF, N, 2), nlp_stride=2 * N,
               nlp_status=z(BF, dtype=I), U_ilqr=z(BF, NIL, 2), ilqr_stride=2 * NIL, ilqr_status=z(BF, dtype=I), u=z(BF, 2), ctrl_status=z(BF, dtype=I))
for label, mut in ([("good", lambda v: None), ("batch=-1", setv("batch", -1)), ("batch=0", setv("batch", 0)), ("nlp_stride=1", setv("nlp_stride", 1)),
                    ("ilqr_stride=0", setv("ilqr_stride", 0)), ("batch=-1, eyt NULL", lambda v: v.update(batch=-1, eyt=None)),
                    ("every family NULL", lambda v: v.update(vt=None, eyt=None, K=None, xt=None, U_nlp=None, nlp_status=None, U_ilqr=None, ilqr_status=None))]
                   + [("%s NULL" % a, setv(a, None)) for a in mc_sig if isinstance(mc_good.get(a), np.ndarray)]):
    v = copy_vals(mc_good)
    mut(v)
    call("crx_mixed_commit_dev", mc_sig, v, label, True)

os.makedirs(os.path.dirname(OUT), exist_ok=True)
open(OUT % TAG + ".txt", "w").write("\n".join(lines) + "\n")
print("%s: %d malformed / empty calls dumped (%s)" % (TAG, len(lines), "GPU" if HAVE_GPU else "no GPU: not initialised"))
if not HAVE_GPU:
    sys.exit(0)

# ---- part 2: every host-pointer entry point once on a valid input ----------------------------------------------------------
from utils import racing_env   # noqa: E402

out = {}


def keep(name, r):
    for k, v in r.items():
        out[name + "/" + k] = np.asarray(v)


p = synth.cfg2_mpccbf(32)
dc = abi.cbf_desc(p["N"], 1, A, B, alpha=p["alpha"], margin=p["margin"])
cargs = [p[k] for k in ("x0", "xt", "obs_s", "obs_ey", "lap_off", "n_obs")]
keep("cbf_solve", gpu.cbf_solve(dc, *cargs))
keep("cbf_solve_dims", gpu.cbf_solve(dc, *cargs, obs_dims=np.tile(np.array([0.45, 0.25]), (32, 1, 1))))
q = synth.cfg3_planner(8, N=12)
dp, ds = abi.planner_desc(12, A, B), abi.select_desc(12, q["V"], q["lap_length"])
pargs = [q[k] for k in ("x0", "bez_s", "bez_ey", "ey_lb", "ey_ub")]
rp = gpu.planner_solve(dp, *pargs)
keep("planner_solve", rp)
sargs = [q[k] for k in ("n_veh", "obs_s", "obs_ey", "old_flag")]
keep("select", gpu.select(ds, q["n_veh"], rp["X"].reshape(q["n_scen"], q["V"] + 1, 13, 6), q["obs_s"], q["obs_ey"], q["old_flag"]))
keep("planner_plan", gpu.planner_plan(dp, ds, *pargs, *sargs))
w = q["raw"]
keep("planner_prep", gpu.planner_prep(abi.prep_desc(12, q["V"], len(w["opt_s"]), w["track_width"], w["lap_length"]), w["x"], w["x"], w["n_veh"],
                                      w["veh_info"], w["max_dv"], w["obs_s"], w["obs_ey"], w["opt_s"], w["opt_ey"]))
rng = np.random.default_rng(7)
S, VA = 8, 5
ego = np.stack([rng.uniform(0.5, 2.0, S), np.zeros(S), np.zeros(S), np.zeros(S), rng.uniform(0, 15, S), rng.uniform(-0.5, 0.5, S)], axis=1)
veh = np.zeros((S, VA, 6))
veh[..., 0], veh[..., 4], veh[..., 5] = rng.uniform(0.3, 1.5, (S, VA)), ego[:, None, 4] + rng.uniform(-3, 6, (S, VA)), rng.uniform(-0.8, 0.8, (S, VA))
pred_s = veh[..., 4, None] + 0.1 * np.arange(13) * veh[..., 0, None]
keep("planner_scene", gpu.planner_scene(abi.scene_desc(12, VA, 3, q["lap_length"]), ego, rng.integers(0, VA + 1, S).astype(I), veh, pred_s,
                                        np.repeat(veh[..., 5, None], 13, axis=2)))
track = racing_env.ClosedTrack(np.genfromtxt(ROOT + "/data/track_layout/l_shape.csv", delimiter=","), track_width=1.0)
tab = track.point_and_tangent
xc = np.stack([rng.uniform(0.3, 2.0, 16), rng.normal(0, 0.05, 16), rng.normal(0, 0.3, 16), rng.uniform(-0.2, 0.2, 16),
               rng.uniform(0.0, track.lap_length, 16), rng.uniform(-0.8, 0.8, 16)], axis=1)
xg = np.stack([xc[:, 0], xc[:, 1], xc[:, 2], rng.uniform(-3, 3, 16), rng.uniform(-5, 5, 16), rng.uniform(-5, 5, 16)], axis=1)
keep("plant_step", gpu.plant_step(abi.plant_desc(tab.shape[0], track.lap_length), tab, xg, xc, np.stack([rng.uniform(-0.5, 0.5, 16), rng.uniform(-1, 1, 16)], axis=1)))
opt = rng.uniform(-0.3, 0.3, (8, 11))
keep("path_solve", gpu.path_solve(abi.path_desc(10, 0.5), opt, opt + rng.uniform(-0.1, 0.1, (8, 11)), np.full((8, 11), -0.8), np.full((8, 11), 0.8),
                                  opt[:, 0].copy(), opt[:, -1].copy()))
g = np.load(ROOT + "/tests/golden/racing_game.npz")
dl = abi.lmpc_desc(N=g["lmpc/A"].shape[1], n_ss_max=g["lmpc/ss"].shape[2])
keep("lmpc_solve", gpu.lmpc_solve(dl, *[g["lmpc/" + k][:8] for k in ("x", "u_old", "A", "B", "C", "ss", "qfun")]))
ss = np.ascontiguousarray(g["ss/ss0"].transpose(2, 0, 1))[None]
us = np.ascontiguousarray(g["ss/u0"].transpose(2, 0, 1))[None]
qf = np.ascontiguousarray(g["ss/Qfun0"].T)[None]
dpp = abi.lmpcprep_desc(12, ss.shape[2], ss.shape[1], tab.shape[0], 0.1, track.lap_length)
lin_points = ss[0, 0, 1:14][None].copy()
pa = [ss, us, qf, g["ss/time_ss"].astype(I)[None], np.array([2], dtype=I), g["lmpc/x"][:1], lin_points, us[0, 0, 1:13][None], tab]
seed = (rng.normal(size=(1, 12, 6, 6)), rng.normal(size=(1, 12, 6, 2)), rng.normal(size=(1, 12, 6)))
keep("lmpc_prep", gpu.lmpc_prep(dpp, *pa, seed=seed))
lin_points[0, 4, 0] += 400.0       # a singular stage: its three regression rows come back as the seed had them
pa[6] = lin_points
keep("lmpc_prep_singular", gpu.lmpc_prep(dpp, *pa, seed=seed))
p1 = synth.cfg2_mpccbf(8, N=20)
keep("ilqr_solve", gpu.ilqr_solve(abi.ilqr_desc(20, A, B, max_iter=30), p1["x0"], p1["xt"], p1["obs_s"], p1["obs_ey"], p1["lap_off"], p1["n_obs"]))
xs = np.cumsum(rng.normal(0, 0.1, (3, 400, 6)), axis=1)
keep("sysid_fit", gpu.sysid_fit(abi.sysid_desc(chunk_rows=256), xs, rng.normal(0, 0.3, (3, 400, 2))))
keep("sysid_fit_grouped", gpu.sysid_fit(abi.sysid_desc(), xs, rng.normal(0, 0.3, (3, 400, 2)), group_offsets=np.array([0, 2, 3])))
np.savez(OUT % TAG + ".npz", **out)
print("%s: %d output arrays of %d valid host-pointer calls dumped" % (TAG, len(out), len({k.split("/")[0] for k in out})))
