"""Record what the reference decides exactly ON the edges of its front-end comparisons into tests/golden/front_edges.npz.

Run in the build container only (the reference does not exist on the GPU box):

    python tests/golden/tools/make_front_edges.py

The kernels between the raw race state and a solver launch (crx_scene_kernel, crx_prep_kernel, crx_select_kernel,
crx_trackprep_kernel, crx_cbfprep_kernel / crx_cbfprep_laps_kernel, crx_game_traffic_kernel) are comparisons: `<=`, `>=`, strict `<`,
the first arg-min, int() toward zero, `while s > L`.  Every case here puts one of them on its edge, or one np.nextafter to either
side, and records what the reference's own, unmodified code does there -- driven through ref_harness with namespace stand-ins for
the vehicles, the recording casadi stand-in (the NLPs are recorded, never solved: Opti.solve hands back the trajectories the case
crafted) and, for the scripted cars, the reference's NoDynamicsModel itself.

Exactness.  Lap length 16.0 (32.0 in the second window group), dyadic positions, speeds, times and car dimensions (0.5 x 0.25, so
l^2 + w^2 = 0.3125), so that the deciding quantity is exact in binary floating point and a fused multiply-add cannot change a
decision.  `_pin` checks it case by case: the deciding expression is evaluated with fractions.Fraction over the doubles the case
holds; the exact value must be zero or at least a quarter of the smallest operand's spacing away from zero (a rounding of an
intermediate moves the value by at most half a spacing of that intermediate; the one-ulp cases sit a whole spacing of an operand
away, squares shrink that by at most two), and the exact decision must be the one the reference returned.  A case that fails is a
construction error and stops the tool; nothing is dropped.  The only non-dyadic numbers are the reference's own literals 0.15
(safety_margin) and 0.1 (the planner's stage time): they enter as the doubles they are.

The file holds data only -- inputs, recorded outputs, case names; a case is named after the comparison it pins.  Groups:
    interest/           ego_v, ego_s, agent_v, agent_s -> want                       check_ego_agent_distance == get_overtake_flag
    overflow/           ego, n_all, veh, V             (no recorded answer: the policy is the library's own)
    plan{N}/            x_raw, x_wrapped, n_all, veh, pred_s, pred_ey -> interest, order, veh_info, max_dv, bez, active;
                        has_X, X, old_flag -> flag      get_overtake_flag, get_local_traj, generate_traj_per_region, selection
    win{N}_{L}/         x, car_s0, car_v, car_ey (t, dt) -> pred_s, pred_ey, n_obs, kept, lap_off (control.mpccbf);
                        mma_n_veh, mma_pred_s, mma_pred_ey -> mma_n_obs, mma_kept, mma_lap_off (control.mpc_multi_agents)
    target{N}/          x, traj -> xt_ey               control.mpc_multi_agents' f_traj(s_tmp)
    traffic/            s0, v, ey (t, dt) -> x, pred_s, pred_ey      NoDynamicsModel.forward_one_step, get_trajectory_nsteps
"""
import contextlib
import io
import os
import sys
import types
import zipfile
from fractions import Fraction as Fr

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.normpath(os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import ref_harness  # noqa: E402

M = ref_harness.install()
import sympy as sp  # noqa: E402

base, control, casadi, planner_mod, ph = M["base"], M["control"], M["casadi"], M["planner"], M["planner_helper"]

LEN, WID, TW = 0.5, 0.25, 1.0
C15 = 0.15                      # the reference's safety_margin literal
UP, DN = np.inf, -np.inf
NS = types.SimpleNamespace
COUNTS = {}                     # (stage, pinned comparison) -> cases


def nxt(x, to):
    return float(np.nextafter(x, to))


def _pin(stage, what, exact, operands, decision, rule):
    """The self-check of the docstring.  rule(exact) -> the decision in exact arithmetic."""
    exact = Fr(exact)
    sp_min = min(Fr(float(np.spacing(abs(float(o))))) for o in operands if float(o) != 0.0)
    assert exact == 0 or abs(exact) >= sp_min / 4, (stage, what, float(exact), float(sp_min))
    assert bool(rule(exact)) == bool(decision), (stage, what, float(exact), decision)
    COUNTS[(stage, what)] = COUNTS.get((stage, what), 0) + 1


def _count(stage, what):
    COUNTS[(stage, what)] = COUNTS.get((stage, what), 0) + 1


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


# ---- stand-ins ------------------------------------------------------------------------------------------------------------------
class _Proc:   # the fork fan-out of overtake_traj_planner.py:177-197, in this process
    def __init__(self, target, args):
        self.target, self.args = target, args

    def start(self):
        self.target(*self.args)

    def join(self):
        pass


class _Mgr:
    def dict(self):
        return {}


planner_mod.Process, planner_mod.Manager = _Proc, _Mgr
OPTIS, HANDBACK = [], []


def _solve(opti):
    """Opti.solve: record the problem, hand back the crafted trajectory of this region (zeros when the case crafts none)."""
    z = np.zeros(opti.nvar)
    k = len(OPTIS)
    if k < len(HANDBACK):
        z[: HANDBACK[k].size] = HANDBACK[k].reshape(-1)   # xvar is column-major: variable 6 j + r is X[j, r]
    OPTIS.append(opti)
    return z, dict(success=True)


casadi.Opti.solver_fn = staticmethod(_solve)
casadi.Opti.hook = None


def make_track(L):
    return NS(lap_length=L, width=TW, point_and_tangent=np.zeros((1, 6)), get_global_position=lambda s, ey: (0.0, 0.0),
              get_orientation=lambda s, ey: 0.0)


def car_param():
    return NS(length=LEN, width=WID)


def walk(node, out):
    """All (var, a, b) of sub(sub(var, const a), const b) inside a recorded expression."""
    if not isinstance(node, casadi.Node):
        return
    if (node.op == "sub" and isinstance(node.a, casadi.Node) and node.a.op == "sub" and isinstance(node.a.a, casadi.Node) and node.a.a.op == "var"
            and node.a.b.op == "const" and isinstance(node.b, casadi.Node) and node.b.op == "const"):
        out.append((node.a.a.a, node.a.b.a, node.b.a))
    for c in (node.a, node.b):
        walk(c, out)


# ---- interest -------------------------------------------------------------------------------------------------------------------
def interest_exact(ev, es, av, as_, L):
    dv = abs(Fr(ev) - Fr(av))
    sa, se = Fr(as_), Fr(es)
    while sa > L:
        sa -= Fr(L)
    while se > L:
        se -= Fr(L)
    ahead, behind = Fr(4.5) * Fr(LEN) + Fr(0.5) * dv, Fr(LEN)
    atoms = [ahead - (sa - se), sa - se, ahead - (sa + Fr(L) - se), sa + Fr(L) - se, behind - (se - sa), se - sa, behind - (se + Fr(L) - sa), se + Fr(L) - sa]
    dec = any(atoms[2 * i] >= 0 and atoms[2 * i + 1] >= 0 for i in range(4))
    return atoms, dec


def gen_interest(L):
    par = NS(safety_factor=4.5, planning_prediction_factor=0.5)
    cases = []

    def add(name, es, as_, dv=0.0):
        cases.append((name + ("/dv%g" % dv), 1.0, es, 1.0 - dv, as_))

    def three(name, es, as_, dv=0.0, vary="agent", step=None):
        """The edge and one step to either side: np.nextafter of the varied position, or `step` where the deciding sum lives at a
        coarser spacing (s_a + L)."""
        for tag, to in (("below", DN), ("at", None), ("above", UP)):
            e, a = es, as_
            if to is not None:
                if vary == "agent":
                    a = nxt(as_, to) if step is None else as_ + (step if to == UP else -step)
                else:
                    e = nxt(es, to) if step is None else es + (step if to == UP else -step)
            add("%s/%s" % (name, tag), e, a, dv)

    for dv in (0.0, 0.25):
        ah = 4.5 * LEN + 0.5 * dv
        three("c1_dist:s_a-s_e<=ahead", 4.0, 4.0 + ah, dv)
        three("c2_dist:s_a+L-s_e<=ahead", 15.0, ah - 1.0, dv, step=float(np.spacing(L)))
        three("c3_dist:s_e-s_a<=len", 4.0, 4.0 - LEN, dv)
        three("c4_dist:s_e+L-s_a<=len", 0.25, L - 0.25, dv)
        three("c1c3_order:s_a==s_e", 4.0, 4.0, dv)
        three("c2_order:s_a+L==s_e", L, 0.0, dv, vary="ego")
        three("c4_order:s_a==s_e+L", 0.0, L, dv)
        three("ego_at_L_not_wrapped:c2_dist", L, L + ah, dv, step=float(np.spacing(L)))                 # the agent past the line wraps, the ego at L does not
        three("ego_nextafter_L_wraps:c1_dist", nxt(L, UP), float(np.spacing(L)) + ah, dv)
        three("agent_at_L_not_wrapped:c1_dist", L - ah, L, dv, vary="ego")
        three("agent_at_L_not_wrapped:c3_order", L, L, dv)
    names, rows, want = [], [], []
    for name, ev, es, av, as_ in cases:
        ego, ag = NS(xcurv=np.array([ev, 0, 0, 0, es, 0.0]), param=car_param()), NS(xcurv=np.array([av, 0, 0, 0, as_, 0.0]), param=car_param())
        got = bool(ph.check_ego_agent_distance(ego, ag, par, L))
        pl = planner_mod.OvertakeTrajPlanner(par)
        pl.vehicles, pl.agent_name, pl.track = {"ego": ego, "car1": ag}, "ego", make_track(L)
        flag, vi = pl.get_overtake_flag(ego.xcurv)
        assert flag == got and (list(vi) == ["car1"]) == got
        atoms, dec = interest_exact(ev, es, av, as_, L)
        assert dec == got, name
        for a in atoms:
            assert a == 0 or abs(a) >= Fr(float(np.spacing(min(abs(es) or 1.0, abs(as_) or 1.0, LEN)))) / 4, name
        _count("interest", name.split("/")[0])
        names.append(name), rows.append((ev, es, av, as_)), want.append(got)
    rows = np.array(rows)
    return {"interest/names": np.array(names), "interest/ego_v": rows[:, 0], "interest/ego_s": rows[:, 1], "interest/agent_v": rows[:, 2],
            "interest/agent_s": rows[:, 3], "interest/want": np.array(want)}


# ---- overflow: inputs only ------------------------------------------------------------------------------------------------------
def gen_overflow(L):
    names, V, ego, n_all, veh = [], [], [], [], []

    def add(name, v, es, cars):
        names.append("norecord/" + name), V.append(v), ego.append([1.0, 0, 0, 0, es, 0.0]), n_all.append(len(cars))
        rows = np.zeros((8, 6))
        for i, (s, ey) in enumerate(cars):
            rows[i] = (1.0, 0, 0, 0, s, ey)
        veh.append(rows)
        _count("overflow", name.split("/")[0])

    # four of interest for three slots; candidates 0 and 3 are equidistant (0.25 ahead, 0.25 behind): the earlier one stays
    add("equidistant_ahead_behind:dist<bd/V3", 3, 4.0, [(4.25, 0.5), (4.125, 0.25), (4.0625, 0.0), (3.75, -0.25)])
    add("equidistant_behind_ahead:dist<bd/V3", 3, 4.0, [(3.75, 0.5), (4.125, 0.25), (4.0625, 0.0), (4.25, -0.25)])
    # across the start line: ego at 0.125, one 0.25 ahead (0.375), one 0.25 behind (L - 0.125)
    add("equidistant_across_line:dist<bd/V3", 3, 0.125, [(0.375, 0.5), (0.25, 0.25), (0.1875, 0.0), (L - 0.125, -0.25)])
    add("equidistant_across_line_rev:dist<bd/V3", 3, 0.125, [(L - 0.125, 0.5), (0.25, 0.25), (0.1875, 0.0), (0.375, -0.25)])
    add("two_dropped:overflow_counts/V3", 3, 4.0, [(4.5, 0.5), (4.125, 0.25), (4.25, 0.0), (4.375, -0.25), (4.0625, 0.125)])
    add("all_equidistant:first_kept/V3", 3, 4.0, [(4.25, 0.5), (3.75, 0.25), (4.25, 0.0), (3.75, -0.25), (4.25, 0.125)])
    cars8 = [(4.5, 0.5), (4.125, 0.25), (4.25, 0.0), (4.375, -0.25), (4.0625, 0.125), (3.75, 0.375), (4.25, -0.5), (3.875, 0.0625)]
    add("eight_around_six_slots:dist<bd/V6", 6, 4.0, cars8)
    add("seven_around_six_slots:equidistant_last/V6", 6, 4.0, cars8[:5] + [(3.5, 0.375), (4.5, -0.5)])
    return {"overflow/names": np.array(names), "overflow/V": np.array(V, dtype=np.int32), "overflow/ego": np.array(ego),
            "overflow/n_all": np.array(n_all, dtype=np.int32), "overflow/veh": np.array(veh)}


# ---- planner scenes: sort, Bezier, ey windows, selection ------------------------------------------------------------------------
def opt_table(L):
    s = np.array([0.5] + [float(i) for i in range(1, int(L) + 1)])
    ey = np.array([((5 * i) % 7 - 3) / 16.0 for i in range(len(s))])
    return s, ey


def run_plan(L, N, case):
    """One scene through get_overtake_flag -> get_local_traj (-> generate_traj_per_region per region -> selection)."""
    N1 = N + 1
    opt_s, opt_ey = opt_table(L)
    opt = np.zeros((len(opt_s), 6))
    opt[:, 4], opt[:, 5] = opt_s, opt_ey
    par = NS(num_horizon_planner=N, timestep=0.1, planning_prediction_factor=0.5, safety_factor=4.5, bezier_order=3, matrix_A=np.eye(6),
             matrix_B=np.zeros((6, 2)))
    track = make_track(L)
    x_raw, x_wr = np.array(case["x_raw"], float), np.array(case["x_wrapped"], float)
    vehicles = {"ego": NS(xcurv=x_raw.copy(), param=car_param(), no_dynamics=False)}
    K = len(case["cars"])
    veh, ps, pe = np.zeros((4, 6)), np.zeros((4, N1)), np.zeros((4, N1))
    for i, c in enumerate(case["cars"]):
        veh[i] = c["x"]
        ps[i] = c["ps"] if "ps" in c else c["x"][4] + 0.0 * np.arange(N1)   # (standing predictions: no stage lands near a window edge by accident)
        pe[i] = c["pe"] if "pe" in c else c["x"][5]
        traj = np.zeros((6, N1))
        traj[4], traj[5] = ps[i], pe[i]
        vehicles["car%d" % i] = NS(xcurv=veh[i].copy(), param=car_param(), no_dynamics=True,
                                   get_trajectory_nsteps=lambda *a, _t=traj: (_t.copy(), None))
    pl = planner_mod.OvertakeTrajPlanner(par)
    pl.vehicles, pl.agent_name, pl.track, pl.opti_traj_xcurv = vehicles, "ego", track, opt
    flag, interest = pl.get_overtake_flag(x_wr)
    rec = dict(x_raw=x_raw, x_wrapped=x_wr, n_all=K, veh=veh, pred_s=ps, pred_ey=pe,
               interest=np.zeros(4, dtype=bool), order=np.full(4, -1, dtype=np.int32), veh_info=np.zeros((4, 3)), max_dv=0.0,
               bez=np.zeros((5, N1, 2)), active=np.zeros((5, N, 2), dtype=bool), has_X="X" in case, X=np.zeros((5, N1, 6)),
               old_flag=-1 if case.get("old_flag") is None else case["old_flag"], flag=-1)
    for n in interest:
        rec["interest"][int(n[3:])] = True
    assert flag, case["name"]
    seen = {}
    real = ph.get_bezier_control_points

    def spy(vi_, veh_info_list, agent_info, *a):
        seen["veh_info"], seen["max_dv"] = np.array(veh_info_list), agent_info.max_delta_v
        return real(vi_, veh_info_list, agent_info, *a)

    planner_mod.get_bezier_control_points = spy
    del OPTIS[:], HANDBACK[:]
    if "X" in case:
        HANDBACK.extend(np.asarray(x, float) for x in case["X"])
        rec["X"][: len(case["X"])] = case["X"]
    try:
        res = quiet(pl.get_local_traj, x_wr, 0.0, interest, None, None, None, None, case.get("old_flag"))
    finally:
        planner_mod.get_bezier_control_points = real
    order = [int(n[3:]) for n in res[3]]
    V = len(order)
    assert len(OPTIS) == V + 1
    rec["order"][:V], rec["veh_info"][:V], rec["max_dv"] = order, seen["veh_info"], seen["max_dv"]
    rec["bez"][: V + 1] = pl.bezier_xcurvs
    rec["flag"] = int(res[2])
    if case["name"].startswith("bezier/s"):   # the end point's two comparisons, on the exact s3 (no rounding on the way to it)
        s3 = Fr(float(x_wr[4])) + Fr(0.5) * Fr(float(seen["max_dv"])) + 4
        assert Fr(float(pl.bezier_xcurvs[0, N, 0])) == s3, case["name"]
        ops = (float(s3), L, float(x_wr[4]))
        _pin("bezier", "s3>=L(exact)", s3 - Fr(L), ops, s3 >= L, lambda e: e >= 0)
        s_end = s3 - Fr(L) if s3 >= L else s3
        _pin("bezier", "s_end<=opt_s[0](exact)", Fr(float(opt_s[0])) - s_end, ops, s_end <= Fr(float(opt_s[0])), lambda e: e >= 0)
        assert any(Fr(float(v)) == s_end for v in opt_s) == ("/at" in case["name"] and "s3==L" not in case["name"]), case["name"]
    for r, opti in enumerate(OPTIS):
        for con in opti.cons:
            got = []
            if con.kind != "ge" or con.node.op != "sub" or not isinstance(con.node.a, casadi.Node) or con.node.a.op != "sub":
                continue
            walk(con.node, got)
            for var, a, b in got[:1]:
                assert var % 6 == 5 and b == WID + C15
                k = var // 6
                sides = [sd for sd, v in ((0, r - 1), (1, r)) if 0 <= v < V and pe[order[v], k] == a]
                assert sides, (case["name"], r, k)
                for sd in sides:   # (two neighbours with the same ey at stage k: told apart below by the exact window test)
                    rec["active"][r, k, sd] = True
    # the exact window test decides which side when both neighbours share an ey, and pins every recorded decision
    for r in range(V + 1):
        for k in range(N):
            s_nom = x_wr[4] + k * 0.1 * x_wr[0]
            for sd, v in ((0, r - 1), (1, r)):
                if not 0 <= v < V:
                    continue
                os_ = Fr(float(ps[order[v], k]))
                while os_ > L:
                    os_ -= Fr(L)
                lo, hi = Fr(s_nom) - (os_ - Fr(LEN) - Fr(C15)), (os_ + Fr(LEN) + Fr(C15)) - Fr(s_nom)
                inside = lo >= 0 and hi >= 0
                if rec["active"][r, k, sd] and not inside:
                    other = rec["active"][r, k, 1 - sd]
                    assert other, (case["name"], r, k, sd)
                    rec["active"][r, k, sd] = False
                assert bool(rec["active"][r, k, sd]) == inside, (case["name"], r, k, sd)
                if case.get("pins_window"):
                    ops = (s_nom, float(os_), C15)
                    _pin("ey_window", "s_nom>=os-win", lo, ops, lo >= 0, lambda e: e >= 0)
                    _pin("ey_window", "s_nom<=os+win", hi, ops, hi >= 0, lambda e: e >= 0)
    return rec


def sel_exact(L, N, rec, name):
    """Exact selection: every circle value pinned, the first arg-min of the exact costs must be the recorded flag."""
    order = [int(v) for v in rec["order"] if v >= 0]
    V = len(order)
    costs = []
    for r in range(V + 1):
        X = rec["X"][r]
        c = Fr(-10) * (Fr(float(X[N, 4])) - Fr(float(X[0, 4]))) if np.isfinite(X[[0, N], 4]).all() else None
        for v in (r - 1, r):
            if not 0 <= v < V:
                continue
            for j in range(N + 1):
                os_ = Fr(float(rec["pred_s"][order[v], j]))
                while os_ > L:
                    os_ -= Fr(L)
                xs, xe = float(X[j, 4]), float(X[j, 5])
                if np.isnan(xs) or np.isnan(xe):
                    c += 100                                     # `nan >= 0` is False in the reference: a hit
                    _count("select", "nan_point_is_hit:!(h>=0)")
                    continue
                if np.isinf(xs) or np.isinf(xe):
                    _count("select", "inf_point_is_no_hit:inf>=0")   # inf ** 2 >= 0 is True
                    continue
                ds, de = Fr(xs) - os_, Fr(xe) - Fr(float(rec["pred_ey"][order[v], j]))
                h = ds * ds + de * de - Fr(LEN) ** 2 - Fr(WID) ** 2
                if abs(h) < Fr(1, 2):
                    _pin("select", "circle:h>=0", h, (float(ds), float(de), LEN, WID), h >= 0, lambda e: e >= 0)
                c += 0 if h >= 0 else 100
        if rec["old_flag"] >= 0 and rec["old_flag"] != r:
            c += 100
        costs.append(c)
    best = costs.index(min(costs))
    assert best == rec["flag"], (name, costs, rec["flag"])
    if sum(1 for c in costs if c == min(costs)) > 1:
        _count("select", "equal_cost:first_wins(c<best)")
    return best


def gen_plan(L, N):
    N1 = N + 1
    cases = []

    def car(s, ey, v=1.0, **kw):
        return dict(x=[v, 0, 0, 0, s, ey], **kw)

    def ego(s, ey=0.125, v=1.0, raw=None):
        return dict(x_wrapped=[v, 0, 0, 0, s, ey], x_raw=[v, 0, 0, 0, s if raw is None else raw, ey])

    def add(name, e, cars, **kw):
        cases.append(dict(name=name, cars=cars, **e, **kw))
        _count(name.split("/")[0], name.split("/")[1])

    q = 0.25
    wave = lambda base_, amp: base_ + amp * ((np.arange(N1) % 3) - 1) / 8.0   # noqa: E731  a prediction whose max and min differ
    # -- partial sort: the new vehicle against the CURRENT FIRST, `>=` to the front
    add("sort/equal_ey_goes_front:e>=first/two", ego(4.0), [car(5.0, q, pe=wave(q, 1)), car(5.5, q, 0.75, pe=wave(q, 2))])
    add("sort/equal_ey_goes_front:e>=first/three_all_equal", ego(4.0), [car(5.0, q), car(5.5, q, 0.75), car(4.5, q, 1.25)])
    add("sort/equal_ey_goes_front:e>=first/pair_then_lower", ego(4.0), [car(5.0, q, pe=wave(q, 1)), car(5.5, q, pe=wave(q, 2)), car(4.5, 0.0, pe=wave(0.0, 3))])
    add("sort/equal_ey_goes_front:e>=first/lower_then_equal", ego(4.0), [car(5.0, q), car(5.5, 0.0, 0.5), car(4.5, q)])
    add("sort/equal_ey_goes_front:e>=first/four_equal_in_pairs", ego(4.0), [car(5.0, q, pe=wave(q, 1)), car(5.5, 0.0, pe=wave(0.0, 2)), car(4.5, q, 0.5, pe=wave(q, 3)), car(4.375, 0.0)])
    add("sort/equal_ey_goes_front:e>=first/four_all_equal", ego(4.0), [car(5.0, q), car(5.5, q), car(4.5, q), car(4.375, q)])
    add("sort/ulp_above_first_goes_front:e>=first/two", ego(4.0), [car(5.0, q), car(5.5, nxt(q, UP))])
    add("sort/ulp_below_first_goes_back:e>=first/two", ego(4.0), [car(5.0, q), car(5.5, nxt(q, DN))])
    add("sort/veh_info_in_iteration_order/not_of_interest_between", ego(4.0), [car(5.0, 0.0, pe=wave(0.0, 1)), car(12.0, 0.5), car(5.5, q, 0.5, pe=wave(q, 2)), car(4.5, q, pe=wave(q, 3))])
    add("sort/max_dv_equal_speeds:fmax/all_at_ego_speed", ego(4.0), [car(5.0, q), car(5.5, 0.0)])
    add("sort/max_dv_equal_speeds:fmax/equal_dv_either_sign", ego(4.0), [car(5.0, q, 0.75), car(5.5, 0.0, 1.25)])
    # -- Bezier end point
    e2 = float(np.spacing(L))
    for tag, d in (("below", -e2 / 4), ("at", 0.0), ("above", e2)):   # (below: one spacing of the values under L; above: one of L)
        add("bezier/s3==L:s3>=L/%s" % tag, ego(L - 4.0 + d), [car(L - 3.0, -q)])
        add("bezier/s3==L:s3>=L/dv0.5/%s" % tag, ego(L - 4.25 + d), [car(L - 3.125, -q, 0.5)])
        add("bezier/s_end==opt_s[0]:s_end<=opt_s[0]/%s" % tag, ego(L - 3.5 + (d if d >= 0 else -e2)), [car(L - 3.0, -q)])
        add("bezier/s_end_on_interior_node:xs[hi]<x/%s" % tag, ego(2.0 + float(np.sign(d)) * float(np.spacing(6.0))), [car(3.0, -q)])
    add("bezier/raw_state_copied_not_wrapped/x0", ego(2.0, raw=2.0 + L), [car(3.0, -q), car(3.5, q)])
    add("bezier/middle_region_between_two/e12", ego(2.0), [car(3.0, -q, pe=wave(-q, 1)), car(3.5, q, pe=wave(q, 2)), car(2.5, 0.0, pe=wave(0.0, 1))])
    # -- ey windows: X = 0.25 - c and os = 0.75 make s_nom == os - len - c exact; Y = 2^-10 + c and os = 2^-10 - 0.5 the upper edge
    X0, Y0, m = 0.25 - C15, 2.0 ** -10 + C15, 2.0 ** -10
    assert Fr(X0) == Fr(0.25) - Fr(C15) and Fr(Y0) == Fr(m) + Fr(C15)
    for tag, to in (("below", DN), ("at", None), ("above", UP)):
        x = X0 if to is None else nxt(X0, to)
        y = Y0 if to is None else nxt(Y0, to)
        add("ey_window/s_nom==os-win:left_and_right/%s" % tag, ego(x, v=0.0), [car(x + 1.0, q, 0.0, ps=np.full(N1, 0.75))], pins_window=True)
        add("ey_window/s_nom==os+win:left_and_right/%s" % tag, ego(y, v=0.0), [car(y + 1.0, q, 0.0, ps=np.full(N1, m - 0.5))], pins_window=True)
        far = np.full(N1, 8.0)
        add("ey_window/s_nom==os-win:stage0_only/%s" % tag, ego(x), [car(x + 1.0, q, ps=np.r_[0.75, far[1:]])], pins_window=True)
        add("ey_window/s_nom==os+win:stage0_only/%s" % tag, ego(y), [car(y + 1.0, q, ps=np.r_[m - 0.5, far[1:]])], pins_window=True)
    add("ey_window/both_neighbours_inside:fmax/higher_left", ego(X0 + 0.5, v=0.0), [car(1.5, 0.5, 0.0, ps=np.full(N1, 0.75)), car(1.25, -q, 0.0, ps=np.full(N1, 0.5))], pins_window=True)
    add("ey_window/both_neighbours_inside:fmax/equal_ey_rows", ego(X0 + 0.5, v=0.0), [car(1.5, q, 0.0, ps=np.full(N1, 0.75)), car(1.25, q, 0.0, ps=np.full(N1, 0.5))], pins_window=True)
    add("ey_window/prediction_at_L_not_wrapped:os>L/inside", ego(L - 0.25, v=0.0), [car(L - 0.125, q, 0.0, ps=np.full(N1, L))], pins_window=True)
    add("ey_window/prediction_at_L_plus_half_wraps:os>L/inside", ego(0.25, v=0.0), [car(0.5, q, 0.0, ps=np.full(N1, L + 0.5))], pins_window=True)
    add("ey_window/prediction_ulp_above_L_wraps:os>L/outside", ego(L - 0.25, v=0.0), [car(L - 0.125, q, 0.0, ps=np.full(N1, nxt(L, UP)))], pins_window=True)
    # -- selection: the obstacle stands at (5, 0); region trajectories run 1.0 beside it except for the crafted point j = 3
    def traj(P, pt=None, s_start=4.0, ey=1.0):
        Xr = np.zeros((N1, 6))
        Xr[:, 0], Xr[:, 4], Xr[:, 5] = 1.0, s_start + P * np.arange(N1) / N, ey
        Xr[N, 4] = s_start + P
        if pt is not None:
            Xr[3, 4], Xr[3, 5] = pt
        return Xr

    one = [car(5.0, 0.0, 0.0, ps=np.full(N1, 5.0))]
    for tag, pt in (("on_circle_s", (5.5, q)), ("on_circle_behind", (4.5, -q)), ("ulp_inside_s", (nxt(5.5, DN), q)), ("on_circle_ey_major", (5.25, 0.5)), ("ulp_inside_ey", (5.25, nxt(0.5, DN))),
                    ("ulp_outside_s", (nxt(5.5, UP), q)), ("ulp_outside_ey", (5.25, nxt(0.5, UP))), ("nonfinite_ey", (5.5, np.nan)), ("inf_ey", (5.5, np.inf))):
        add("select/circle:h>=0/right_neighbour_of_region0/%s" % tag, ego(4.0), one, X=[traj(2.5, pt), traj(2.0)])          # a hit on region 0 hands the win to region 1
        add("select/circle:h>=0/left_neighbour_of_region1/%s" % tag, ego(4.0), one, X=[traj(2.0), traj(2.5, pt)])
    add("select/equal_cost:first_wins(c<best)/two_regions", ego(4.0), one, X=[traj(2.5), traj(2.5)])
    add("select/equal_cost:first_wins(c<best)/three_regions", ego(4.0), [car(5.0, 0.0, 0.0, ps=np.full(N1, 5.0)), car(5.5, -q, 0.0, ps=np.full(N1, 5.5))],
        X=[traj(2.0), traj(2.5), traj(2.5)])
    for tag, old in (("old_unset", None), ("old_is_winner", 0), ("old_is_other_tie", 1)):
        add("select/switch_penalty:old!=r/%s" % tag, ego(4.0), one, X=[traj(12.5), traj(2.5)], old_flag=old)
    add("select/switch_penalty:old!=r/old_0_other_cheaper_by_100_tie", ego(4.0), one, X=[traj(2.5), traj(12.5)], old_flag=0)
    add("select/switch_penalty:old!=r/hit_plus_switch_tie", ego(4.0), one, X=[traj(22.5, (5.0, 0.0)), traj(2.5)], old_flag=1)
    add("select/prediction_at_L_not_wrapped:os>L/on_circle", ego(L - 1.0), [car(L - 0.5, 0.0, 0.0, ps=np.full(N1, L))],
        X=[traj(2.5, (L + 0.5, q), s_start=L - 1.0), traj(2.0, s_start=L - 1.0)])
    add("select/prediction_at_L_not_wrapped:os>L/ulp_inside", ego(L - 1.0), [car(L - 0.5, 0.0, 0.0, ps=np.full(N1, L))],
        X=[traj(2.5, (nxt(L + 0.5, DN), q), s_start=L - 1.0), traj(2.0, s_start=L - 1.0)])   # (a hit only while 16.0 stays 16.0)
    add("select/prediction_at_L_plus_half_wraps:os>L/on_circle", ego(0.25), [car(0.5, 0.0, 0.0, ps=np.full(N1, L + 0.5))],
        X=[traj(2.5, (1.0, q), s_start=0.25), traj(2.0, s_start=0.25)])
    add("select/prediction_at_L_plus_half_wraps:os>L/ulp_inside", ego(0.25), [car(0.5, 0.0, 0.0, ps=np.full(N1, L + 0.5))],
        X=[traj(2.5, (nxt(1.0, DN), q), s_start=0.25), traj(2.0, s_start=0.25)])
    recs = []
    for c in cases:
        r = run_plan(L, N, c)
        if r["has_X"]:
            sel_exact(L, N, r, c["name"])
        recs.append(r)
    out = {"plan%d/names" % N: np.array([c["name"] for c in cases])}
    for k in recs[0]:
        a = np.array([r[k] for r in recs])
        out["plan%d/%s" % (N, k)] = a.astype(np.int32) if a.dtype == np.int64 else a
    return out


# ---- obstacle window of both controllers ----------------------------------------------------------------------------------------
T_NOW, DT = 8.0, 0.125
T = sp.symbols("t")


def scripted(track, name, s0, v, ey, t):
    c = base.NoDynamicsModel(name=name, param=base.CarParam(length=LEN, width=WID))
    c.set_track(track)
    c.set_timestep(DT)
    c.set_state_curvilinear_func(T, v * T + s0, ey + 0.0 * T)
    c.time = t
    c.xcurv, c.xglob = c.get_estimation(t)
    return c


def gen_window(L, N):
    N1 = N + 1
    track = make_track(L)
    cases = []

    def add(name, x_s, cars, vx=1.0, n_veh=3):
        cases.append((name, [vx, 0, 0, 0, x_s, 0.0], cars, n_veh))

    far = [(10.0, 0.0, 0.5), (11.0, 0.0, -0.5)]                      # (s0, v, ey): folded 10 and 11, outside every window used here
    st = lambda s, ey=0.25: (s, 0.0, ey)                              # noqa: E731  a car standing at s
    add("lower:dist_ego>dist_obs-margin/at_out", 4.0, [st(6.0)] + far)
    add("lower:dist_ego>dist_obs-margin/ulp_inside", 4.0, [st(nxt(6.0, DN))] + far)
    add("lower:dist_ego>dist_obs-margin/ulp_outside", 4.0, [st(nxt(6.0, UP))] + far)
    add("lower:dist_ego>dist_obs-margin/moving_car_at_out", 4.0, [(2.0, 0.5, 0.25)] + far)
    add("upper:dist_ego<dist_obs+margin/at_out", 4.0, [st(2.0)] + far)
    add("upper:dist_ego<dist_obs+margin/ulp_inside", 4.0, [st(2.0 + float(np.spacing(4.0)))] + far)   # (one spacing of the sum dist_obs + margin = 4)
    add("upper:dist_ego<dist_obs+margin/ulp_outside", 4.0, [st(2.0 - float(np.spacing(4.0)) / 2)] + far)
    add("ego_at_L:int(s_over_L)/laps1", L, [st(1.0)] + far)
    add("ego_at_L:int(s_over_L)/ulp_below_laps0", nxt(L, DN), [st(1.0), st(L - 1.0, -0.25), far[0]])
    add("ego_at_2L:int(s_over_L)/laps2", 2 * L, [st(1.0)] + far)
    add("ego_at_2L:int(s_over_L)/ulp_below_laps1", nxt(2 * L, DN), [st(1.0), st(L - 1.0, -0.25), far[0]])
    add("obstacle_at_L:int(s_over_L)/laps1", 1.0, [st(L)] + far)
    add("obstacle_at_L:int(s_over_L)/ulp_below_laps0", 1.0, [st(nxt(L, DN))] + far)
    add("obstacle_negative_s:int()_toward_zero/kept", 0.0, [st(-4.0), (10.0, 0.0, 0.5), (11.0, 0.0, -0.5)], vx=2.5)
    add("obstacle_negative_s:int()_toward_zero/at_minus_L", 1.0, [st(-L), (10.0, 0.0, 0.5), (11.0, 0.0, -0.5)])
    add("obstacle_negative_s:int()_toward_zero/ulp_above_minus_L", 1.0, [st(nxt(-L, UP)), (10.0, 0.0, 0.5), (11.0, 0.0, -0.5)])
    add("packing/middle_kept", 4.0, [far[0], st(4.5), far[1]])
    add("packing/all_kept", 4.0, [st(4.5), st(3.5, -0.25), (0.25, 0.5, 0.5)])
    add("packing/first_and_last_kept", 4.0, [st(4.5), far[0], st(3.5, -0.25)])
    add("packing/two_sorted_vehicles_only", 4.0, [st(4.5), st(3.5, -0.25), st(4.25, 0.5)], n_veh=2)
    add("packing/stopped_ego_keeps_nobody", 4.0, [st(4.0), st(4.5, -0.25), far[0]], vx=0.0)
    par = NS(num_horizon=N, num_horizon_ctrl=N, alpha=0.8, matrix_A=np.eye(6), matrix_B=np.zeros((6, 2)), matrix_Q=np.eye(6), matrix_R=np.eye(2))
    sysp = NS(delta_max=0.5, a_max=1.0, v_max=10.0, v_min=0.0)
    tr = np.zeros((N1, 6))
    tr[:, 4] = np.arange(N1) * 1.0
    keys = ("x", "car_s0", "car_v", "car_ey", "pred_s", "pred_ey", "n_obs", "kept", "lap_off", "mma_n_veh", "mma_pred_s", "mma_pred_ey", "mma_n_obs",
            "mma_kept", "mma_lap_off")
    out = {k: [] for k in keys}
    for name, x, cars, n_veh in cases:
        x = np.array(x)
        vehicles = {"ego": NS(xcurv=x.copy(), param=car_param())}
        for i, (s0, v, ey) in enumerate(cars):
            vehicles["car%d" % i] = scripted(track, "car%d" % i, s0, v, ey, T_NOW)
        names = ["car%d" % i for i in range(3)]

        def kept_of(opti, preds, who):
            n = opti.vars[2][2][0]
            kept, off = np.full(3, -1, dtype=np.int32), np.zeros(3)
            for c in range(n):
                got = []
                walk(opti.cons[6 + c * (2 * N + 1)].node, got)
                hit = [(a, b) for var, a, b in got if var == 4]
                assert hit, name
                a, b = hit[0]
                idx = [i for i in who if preds[i][4, 0] == a]
                assert len(idx) == 1, (name, a)
                kept[c], off[c] = idx[0], b
            return n, kept, off

        # control.mpccbf: every vehicle but the ego, predictions at the launch's dt
        preds = [vehicles[n].get_trajectory_nsteps(T_NOW, DT, N1)[0] for n in names]
        del OPTIS[:], HANDBACK[:]
        quiet(control.mpccbf, x, np.array([1.0, 0, 0, 0, 0, 0.0]), par, vehicles, "ego", L, T_NOW, DT, False, track, sysp)
        n, kept, off = kept_of(OPTIS[-1], preds, range(3))
        # control.mpc_multi_agents: the sorted vehicles, predictions at its own 0.1
        mpreds = [vehicles[n].get_trajectory_nsteps(T_NOW, 0.1, N1)[0] for n in names]
        del OPTIS[:]
        quiet(control.mpc_multi_agents, x, par, track, None, None, None, sysp, target_traj_xcurv=tr, vehicles=vehicles, agent_name="ego",
              direction_flag=0, target_traj_xglob=None, sorted_vehicles=names[:n_veh], time=T_NOW)
        mn, mkept, moff = kept_of(OPTIS[-1], mpreds, range(n_veh))
        # the exact window, pinned
        se, vx = Fr(float(x[4])), Fr(float(x[0]))
        nce = int(se / Fr(L))
        for i in range(3):
            so = Fr(float(preds[i][4, 0]))
            assert so == Fr(cars[i][1]) * Fr(T_NOW) + Fr(cars[i][0]), name             # v t + s0 came out exact
            nco = int(so / Fr(L))
            lo, hi = (se - nce * Fr(L)) - ((so - nco * Fr(L)) - 2 * vx), ((so - nco * Fr(L)) + 2 * vx) - (se - nce * Fr(L))
            ops = (float(x[4]), float(so) or 1.0, float(x[0]) or 1.0)
            is_kept = i in kept[:n]
            tag = name.split("/")[0]
            _pin("window", tag if tag.startswith("lower") else "dist_ego>dist_obs-margin(all)", lo, ops, lo > 0, lambda e: e > 0)
            _pin("window", tag if tag.startswith("upper") else "dist_ego<dist_obs+margin(all)", hi, ops, hi > 0, lambda e: e > 0)
            assert is_kept == (lo > 0 and hi > 0), (name, i)
            if is_kept:
                assert Fr(float(off[list(kept).index(i)])) == (nce - nco) * Fr(L), name
            if i < n_veh:
                assert (i in mkept[:mn]) == is_kept, name
        if not tag.startswith(("lower", "upper")):
            _count("window", tag)
        for k, v in zip(keys, (x, [c[0] for c in cars], [c[1] for c in cars], [c[2] for c in cars], [p[4] for p in preds], [p[5] for p in preds], n, kept,
                               off, n_veh, [p[4] for p in mpreds], [p[5] for p in mpreds], mn, mkept, moff)):
            out[k].append(v)
    g = "win%d_%d/" % (N, int(L))
    res = {g + "names": np.array([c[0] for c in cases])}
    for k in keys:
        a = np.array(out[k])
        res[g + k] = a.astype(np.int32) if a.dtype.kind == "i" else a.astype(np.float64)
    return res


# ---- per-stage targets ----------------------------------------------------------------------------------------------------------
def gen_target(L, N):
    N1 = N + 1
    track = make_track(L)
    tr = np.zeros((N1, 6))
    tr[:, 4] = 4.0 + 0.25 * np.arange(N1)
    tr[:, 5] = ((3 * np.arange(N1)) % 8 - 4) / 16.0
    first, last = float(tr[0, 4]), float(tr[-1, 4])
    cases = []
    for tag, s in (("first_node:s<s_lo", first), ("last_node:s>=s_hi", last), ("interior_node:xs[hi]<x", 5.0)):
        for t2, to in (("below", DN), ("at", None), ("above", UP)):
            cases.append(("%s/%s/stopped" % (tag, t2), 0.0, s if to is None else nxt(s, to)))
    cases += [("clipped_below_first:s<s_lo/stopped", 0.0, 3.5), ("clipped_above_last:s>=s_hi/stopped", 0.0, last + 1.0),
              ("first_node:s<s_lo/at/vx1_crosses_nodes", 1.0, first), ("first_node:s<s_lo/at/vx2.5_runs_past_last", 2.5, first),
              ("clipped_below_first:s<s_lo/vx1_enters_table", 1.0, 3.5), ("interior_node:xs[hi]<x/at/vx2.5_lands_on_nodes", 2.5, 4.25)]
    par = NS(num_horizon_ctrl=N, matrix_A=np.eye(6), matrix_B=np.zeros((6, 2)), matrix_Q=np.eye(6), matrix_R=np.eye(2))
    sysp = NS(delta_max=0.5, a_max=1.0, v_max=10.0, v_min=0.0)
    real = control.interp1d
    xs, eys = [], []
    for name, vx, s in cases:
        x = np.array([vx, 0, 0, 0, s, 0.0])
        calls = []

        def rec_interp(a, b, *aa, **kw):
            f = real(a, b, *aa, **kw)

            def g(v):
                r = f(v)
                calls.append((float(v), float(r)))
                return r
            return g

        control.interp1d = rec_interp
        del OPTIS[:], HANDBACK[:]
        try:
            quiet(control.mpc_multi_agents, x, par, track, None, None, None, sysp, target_traj_xcurv=tr, vehicles={"ego": NS(xcurv=x, param=car_param())},
                  agent_name="ego", direction_flag=0, target_traj_xglob=None, sorted_vehicles=[], time=0.0)
        finally:
            control.interp1d = real
        assert len(calls) == N1, name
        xs.append(x), eys.append([c[1] for c in calls])
        _count("target", name.split("/")[0])
    g = "target%d/" % N
    return {g + "names": np.array([c[0] for c in cases]), g + "x": np.array(xs), g + "traj": tr, g + "xt_ey": np.array(eys)}


# ---- scripted traffic -----------------------------------------------------------------------------------------------------------
def gen_traffic(L, N=12):
    track = make_track(L)
    e1, e2 = float(np.spacing(L)), float(np.spacing(2 * L))
    cases = [("lands_at_L:s>L/at", 1.5, 4.0, 0.25), ("lands_at_L:s>L/ulp_above", 0.0, L + e1, 0.25), ("lands_at_L:s>L/ulp_below", 0.0, L - e1 / 4, 0.25),
             ("lands_at_L:s>L/moving_ulp_above", 1.5, 4.0 + e1, 0.25), ("lands_at_2L:ceil(s_over_L)-1/at", 3.5, 4.0, -0.25),
             ("lands_at_2L:ceil(s_over_L)-1/ulp_below", 0.0, 2 * L - e2 / 4, -0.25), ("between_L_and_2L/at_1.5L", 2.5, 4.0, 0.5),
             ("between_L_and_2L/standing", 0.0, 1.5 * L, 0.5), ("v==0/inside_lap", 0.0, 4.0, -0.5), ("v==0/at_L", 0.0, L, -0.5), ("v==0/at_2L", 0.0, 2 * L, -0.5),
             ("before_the_line/moving", 0.5, 4.0, 0.125), ("negative_s/standing", 0.0, -4.0, 0.125)]
    xs, ps, pe = [], [], []
    for name, v, s0, ey in cases:
        c = base.NoDynamicsModel(name="car", param=base.CarParam(length=LEN, width=WID))
        c.set_track(track)
        c.set_timestep(DT)
        c.set_state_curvilinear_func(T, v * T + s0, ey + 0.0 * T)
        c.time = T_NOW - DT
        c.forward_one_step(False)
        assert c.time == T_NOW
        exact = Fr(v) * Fr(T_NOW) + Fr(s0)
        want = exact - Fr(L) if exact > L else exact
        assert Fr(float(c.xcurv[4])) == want, (name, c.xcurv[4])
        _pin("traffic", name.split("/")[0], exact - Fr(L), (float(exact) or 1.0, L), exact > L, lambda e: e > 0)
        tr = c.get_trajectory_nsteps(None, DT, N + 1)[0]
        xs.append(np.array(c.xcurv, dtype=float)), ps.append(tr[4]), pe.append(tr[5])
    return {"traffic/names": np.array([c[0] for c in cases]), "traffic/v": np.array([c[1] for c in cases]), "traffic/s0": np.array([c[2] for c in cases]),
            "traffic/ey": np.array([c[3] for c in cases]), "traffic/x": np.array(xs), "traffic/pred_s": np.array(ps), "traffic/pred_ey": np.array(pe)}


def save(path, out):
    """np.savez_compressed with fixed member dates: the file regenerates byte for byte."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(out[k], order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type, info.external_attr = zipfile.ZIP_DEFLATED, 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


if __name__ == "__main__":
    L = 16.0
    opt_s, opt_ey = opt_table(L)
    out = dict(L=np.array(L), length=np.array(LEN), width=np.array(WID), track_width=np.array(TW), t=np.array(T_NOW), dt=np.array(DT), opt_s=opt_s,
               opt_ey=opt_ey)
    out.update(gen_interest(L))
    out.update(gen_overflow(L))
    for N in (10, 12):
        out.update(gen_plan(L, N))
        out.update(gen_window(L, N))
        out.update(gen_window(2 * L, N))
        out.update(gen_target(L, N))
    out.update(gen_traffic(L))
    path = os.path.join(OUT, "front_edges.npz")
    save(path, out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))
    stage = None
    for (st_, what), n in sorted(COUNTS.items()):
        if st_ != stage:
            print("%s" % st_)
            stage = st_
        print("    %-58s %4d" % (what, n))
    print("cases: " + ", ".join("%s %d" % (k[:-6], len(v)) for k, v in sorted(out.items()) if k.endswith("/names")))
