"""Draws and host yardsticks shared by tests/test_path_plan_cpu.py and tests/test_gpu_path_plan.py.

The yardstick of the path-planner kernels is the HOST MIRROR planning/overtake_path_planner.py (pinned to the reference's recording by
test_overtake_path_step) with planning/planner_helper.py, driven here scenario by scenario on plain arrays; the scene in front of it is
the CPU oracle's crx_oracle_planner_scene (pinned to the reference and to the mirror in tests/test_host_mirror.py).  Everything is
computed once per process and must not be modified by a test.
"""
import functools
import types

import numpy as np

from crx import abi, hostprep, synth
from planning import overtake_path_planner as opp
from planning import planner_helper as ph

L_SHAPE = synth.LAP_L_SHAPE
SF, PF, VL, VW = 4.5, 0.5, 0.4, 0.2          # safety_factor, planning_prediction_factor, CarParam length / width
ALPHA = 0.98                                 # racing_game_param.alpha

# draw: (scenarios, N, V, seed, track width, factor on the cars' offsets)
DRAWS = {"a": (256, 10, 3, 3, 1.0, 1.0), "b": (256, 10, 3, 3, 2.5, 2.2), "c": (128, 10, 2, 5, 2.5, 2.2), "d": (128, 7, 2, 11, 2.0, 2.0),
         "e": (64, 12, 3, 13, 2.5, 2.2)}
PROBED = ("a", "b", "c", "d")                # the draws whose flags and side-row patterns are unambiguous (test_path_plan_cpu.py)


@functools.lru_cache(maxsize=None)
def draw(name):
    """Raw scenarios of a draw: ego state (raw and start-line-wrapped), every car's current state and prediction, the table."""
    S, N, V, seed, tw, scale = DRAWS[name]
    w = synth.cfg3_raw(S, N=N, seed=seed, V=V, track_width=tw)
    L = float(w["lap_length"])
    x_raw = w["x"].copy()
    cars = w["cars"].copy()                  # (s0, v, ey)
    cars[:, :, 2] *= scale
    n_all = np.full(S, V, dtype=np.int32)
    if name == "e":
        rng = np.random.default_rng(131)
        x_raw[:, 4] = rng.uniform(15.0, 19.0, S)                      # s_tmp and s_N cross the start line
        x_raw[::9, 4] = L + rng.uniform(0.01, 0.3, len(x_raw[::9]))    # raw states just past the line: the wrapped copy differs
        dv = np.abs(x_raw[:, 0, None] - cars[:, :, 1])
        cars[:, :, 0] = x_raw[:, 4, None] + rng.uniform(0.0, 1.0, (S, V)) * (SF * VL + PF * dv)
        n_all = rng.integers(0, V + 1, S).astype(np.int32)            # 0..3 vehicles
        n_all[0] = V
        x_raw[0, 4], cars[0, 0, 0] = 17.5, 18.5                       # scenario 0: s + 1.8 wraps, s - 1.8 does not: rear > front (P5)
    x_wrapped = x_raw.copy()
    x_wrapped[:, 4] = np.where(x_raw[:, 4] > L, x_raw[:, 4] - L, x_raw[:, 4])
    veh = np.zeros((S, V, 6))
    veh[:, :, 0] = cars[:, :, 1]
    veh[:, :, 4] = np.where(cars[:, :, 0] > L, cars[:, :, 0] - L, cars[:, :, 0])     # vehicles keep s in (0, L] (update_memory)
    veh[:, :, 5] = cars[:, :, 2]
    j = np.arange(N + 1)
    pred_s = cars[:, :, 0, None] + 0.1 * j[None, None, :] * cars[:, :, 1, None]
    pred_ey = np.repeat(cars[:, :, 2, None], N + 1, axis=2)                                  # cfg3_raw: constant offsets
    if name == "e":
        pred_ey = pred_ey + 0.01 * np.sin(j[None, None, :] + cars[:, :, 0, None])            # max and min over the prediction differ (P1)
    return dict(name=name, S=S, N=N, V=V, L=L, tw=float(tw), x_raw=x_raw, x_wrapped=x_wrapped, n_all=n_all, veh=veh, pred_s=pred_s,
                pred_ey=pred_ey, opt=w["opt"], opt_s=np.ascontiguousarray(w["opt"][:, 4]), opt_ey=np.ascontiguousarray(w["opt"][:, 5]),
                opt_vx=np.ascontiguousarray(w["opt"][:, 0]))


def descs(d):
    return (abi.scene_desc(d["N"], d["V"], d["V"], d["L"]), abi.pathprep_desc(d["N"], d["V"], d["V"], d["opt"].shape[0], d["tw"], d["L"]),
            abi.path_desc(d["N"], ALPHA))


@functools.lru_cache(maxsize=None)
def scene(name):
    """The scene stage on the CPU oracle: n_veh, order, max_dv, obs_ey (sorted predictions)."""
    import oracle

    d = draw(name)
    return oracle.load().planner_scene(descs(d)[0], d["x_wrapped"], d["n_all"], d["veh"], d["pred_s"], d["pred_ey"])


def _vehicle(x):
    return types.SimpleNamespace(xcurv=x, param=types.SimpleNamespace(length=VL, width=VW))


@functools.lru_cache(maxsize=None)
def mirror_prep(name):
    """path_qp_inputs of the mirror for every scenario: opt, bez, lb, ub [S,R,N+1], e0, eN [S,R] (NaN beyond n_veh + 1 regions and for
    scenarios that are not planned), span [S], raised [S] (the mirror raised: P2), edge [S] = smallest distance of an s sample to a
    front / rear range edge."""
    d, sc = draw(name), scene(name)
    S, N, V, L = d["S"], d["N"], d["V"], d["L"]
    R = V + 1
    out = {k: np.full((S, R, N + 1), np.nan) for k in ("opt", "bez", "lb", "ub")}
    out.update(e0=np.full((S, R), np.nan), eN=np.full((S, R), np.nan), span=np.full(S, np.nan), raised=np.zeros(S, dtype=bool),
               edge=np.full(S, np.inf))
    for s in range(S):
        nv = int(sc["n_veh"][s])
        if nv == 0:
            continue
        order = [int(v) for v in sc["order"][s, :nv]]
        vehicles = {"ego": _vehicle(d["x_raw"][s]), **{v: _vehicle(d["veh"][s, v]) for v in order}}
        info = ph.get_agent_info(vehicles, order, types.SimpleNamespace(lap_length=L))
        obs_infos = np.array([[d["veh"][s, v, 4], sc["obs_ey"][s, k].max(), sc["obs_ey"][s, k].min()] for k, v in enumerate(order)])   # P1
        try:
            cps = ph.bezier_control_points(nv, obs_infos, info.max_delta_v, PF, d["tw"], L, VW, d["opt"], d["x_wrapped"][s])
        except ValueError:
            out["raised"][s] = True
            continue
        bez = ph.bezier_polylines(cps, N)
        q = opp.path_qp_inputs(d["x_raw"][s, 4], d["x_raw"][s, 5], obs_infos, info, cps, bez, d["opt_s"], d["opt_ey"], N, d["tw"], L, SF, PF, VL, VW)
        for k, a in zip(("opt", "bez", "lb", "ub", "e0", "eN"), q):
            out[k][s, :nv + 1] = a
        out["span"][s] = info.max_s + SF * VL + PF * info.max_delta_v - d["x_raw"][s, 4]
        # the samples' distance to the range edges (P4, P5), for the probe of the CPU test
        front, rear = hostprep.wrap_above(obs_infos[:, 0] + SF * VL, L), hostprep.wrap_above(obs_infos[:, 0] - SF * VL, L)
        for j in range(N + 1):
            s_tmp = d["x_raw"][s, 4] + out["span"][s] * j / N
            while s_tmp >= L:
                s_tmp -= L
            s_tmp = np.clip(max(s_tmp, d["opt_s"][0]), bez[0, 0, 0], bez[0, -1, 0])
            out["edge"][s] = min(out["edge"][s], np.abs(front - s_tmp).min(), np.abs(rear - s_tmp).min())
    return out


def host_select(d, sc, span, E, cost):
    """P7 and P8 in numpy, as the mirror's get_local_path (:91-115) and get_speed_info: flag [S], target [S,N+1,6], raised [S].
    E [S,R,N+1], cost [S,R] (inf for a region that did not converge); scenarios without vehicles: flag -1, target NaN."""
    S, N, L, opt = d["S"], d["N"], d["L"], d["opt"]
    flag, target, raised = np.full(S, -1, dtype=np.int32), np.full((S, N + 1, 6), np.nan), np.zeros(S, dtype=bool)
    for s in range(S):
        nv = int(sc["n_veh"][s])
        if nv == 0 or not np.isfinite(span[s]):
            raised[s] = nv > 0
            continue
        costs = [float(c) for c in cost[s, :nv + 1]]
        f = costs.index(min(costs))
        xw, ego_s = d["x_wrapped"][s], d["x_raw"][s, 4]
        t = np.zeros((N + 1, 6))
        for j in range(N + 1):
            t[j, 4] = ego_s + span[s] * j / N
            t[j, 5] = E[s, f, j]
        s_end = t[-1, 4]
        if s_end >= L:
            s_q = opt[0, 4] if s_end - L < opt[0, 4] else s_end - L
        elif s_end < opt[0, 4]:
            s_q = opt[0, 4]
        else:
            s_q = s_end
        if s_q > opt[-1, 4]:
            raised[s] = True
            continue
        vx_t = hostprep.interp_clipped(opt[:, 4], opt[:, 0], s_q)
        delta_t = 2 * (s_end - xw[4]) / (vx_t + xw[0])
        a = np.clip((vx_t - xw[0]) / delta_t, -1.5, 1.5)
        t[0, :] = xw
        with np.errstate(invalid="ignore"):
            for j in range(N):
                t[j, 0] = (xw[0] ** 2 + 2 * a * (t[j, 4] - xw[4])) ** 0.5
        flag[s], target[s] = f, t
    return flag, target, raised
