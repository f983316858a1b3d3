"""Plain restatements of the kernels between the raw race state and a solver launch, as loops over one scene / race at a time
in the reference's expression order: the second reference of tests/test_front_edges_cpu.py and tests/test_gpu_front_edges.py,
which is neither the CPU oracle nor crx.hostprep.  numpy only, no package imports.

    interest, scene        crx_scene_kernel        planner_helper.py:218-266, overtake_traj_planner.py:29-42, :66-92
    prep                   crx_prep_kernel         planner_helper.py:43-153, overtake_traj_planner.py:105-111, :277-324
    select                 crx_select_kernel       overtake_traj_planner.py:205-246
    window, track_prep     crx_trackprep_kernel    control.py:291-309, :373-382
    cbf_prep               crx_cbfprep_kernel, crx_cbfprep_laps_kernel     control.py:499-523, utils/base.py:879-886
    traffic                crx_game_traffic_kernel utils/base.py:795-819, :847-890

Every comparison is written as the reference writes it (`<=` / `>=` / strict `<`, `int()` toward zero, `while s > L`).  Where the
library has a policy of its own (more vehicles of interest than slots; counts clamped; regions past a scene's vehicles) the rule is
the one stated in crx_prep.hip and include/crx.h.
"""
import numpy as np


def wrap_above(s, L):
    while s > L:
        s = s - L
    return s


def interest(ego_v, ego_s, agent_v, agent_s, L, length=0.4, safety_factor=4.5, prediction_factor=0.5):
    """check_ego_agent_distance (planner_helper.py:218-266)."""
    delta_v = abs(ego_v - agent_v)
    s_agent, s_ego = wrap_above(agent_s, L), wrap_above(ego_s, L)
    ahead = safety_factor * length + prediction_factor * delta_v
    behind = 1.0 * length + 0 * prediction_factor * delta_v
    return bool(
        (s_agent - s_ego <= ahead and s_agent >= s_ego)
        or (s_agent + L - s_ego <= ahead and s_agent + L >= s_ego)
        or (-s_agent + s_ego <= behind and s_agent <= s_ego)
        or (-s_agent + s_ego + L <= behind and s_agent <= s_ego + L)
    )


def scene(ego, n_all, veh, pred_s, pred_ey, L, V, length=0.4, safety_factor=4.5, prediction_factor=0.5):
    """One scene of crx_planner_scene.  ego [6], veh [VA,6], pred_s / pred_ey [VA,N+1]; V slots."""
    N1 = pred_s.shape[1]
    hit = [v for v in range(n_all) if interest(ego[0], ego[4], veh[v, 0], veh[v, 4], L, length, safety_factor, prediction_factor)]
    over = 0
    if len(hit) > V:   # the library's policy: the V nearest on the closed lap, ties to the earlier one, kept in dict order
        s_e = wrap_above(ego[4], L)

        def gap(v):
            g = wrap_above(veh[v, 4], L) - s_e
            return min(abs(g), min(abs(g + L), abs(g - L)))
        left, keep = list(hit), []
        for _ in range(V):
            best = left[0]
            for v in left[1:]:
                if gap(v) < gap(best):
                    best = v
            keep.append(best)
            left.remove(best)
        over = len(hit) - V
        hit = sorted(keep)
    order = []
    for v in hit:   # overtake_traj_planner.py:70-76: compared with the CURRENT FIRST only
        if not order:
            order.append(v)
        elif veh[v, 5] >= veh[order[0], 5]:
            order.insert(0, v)
        elif veh[v, 5] <= veh[order[0], 5]:
            order.append(v)
    out = dict(n_veh=len(hit), overflow=over, order=np.full(V, -1, dtype=np.int32), veh_info=np.zeros((V, 3)), max_dv=0.0,
               obs_s=np.zeros((V, N1)), obs_ey=np.zeros((V, N1)))
    for k, v in enumerate(hit):   # iteration order (:87-92)
        out["veh_info"][k] = (veh[v, 4], max(pred_ey[v]), min(pred_ey[v]))
    for k, v in enumerate(order):
        out["order"][k] = v
        out["max_dv"] = max(out["max_dv"], abs(ego[0] - veh[v, 0]))
        out["obs_s"][k], out["obs_ey"][k] = pred_s[v], pred_ey[v]
    return out


def interp1d(xs, ys, x):
    """scipy interp1d(kind="linear"): searchsorted-left, index clipped to [1, n - 1], slope form."""
    hi = 0
    while hi < len(xs) and xs[hi] < x:
        hi += 1
    hi = min(max(hi, 1), len(xs) - 1)
    lo = hi - 1
    slope = (ys[hi] - ys[lo]) / (xs[hi] - xs[lo])
    return slope * (x - xs[lo]) + ys[lo]


def prep(x_wrapped, x_raw, n_veh, veh_info, max_dv, obs_s, obs_ey, opt_s, opt_ey, N, V, track_width, L, prediction_factor=0.5,
         lookahead=4.0, veh_length=0.4, veh_width=0.2, safety_margin=0.15, dt_ref=0.1):
    """One scene of crx_planner_prep.  Returns bez_s, bez_ey [V+1,N+1], ey_lb [V+1,N], active [V+1,N,2] (is the left / right
    neighbour's window closed around stage k), ey_ub [V+1], x0 [V+1,6]."""
    R = V + 1
    nv = min(max(int(n_veh), 0), V)
    s0 = x_wrapped[4]
    s3 = s0 + prediction_factor * max_dv + lookahead
    if s0 > s3:
        s1 = (s3 + L - s0) / 3.0 + s0
        s2 = 2.0 * (s3 + L - s0) / 3.0 + s0
        s3 = s3 + L
    else:
        s1 = (s3 - s0) / 3.0 + s0
        s2 = 2.0 * (s3 - s0) / 3.0 + s0
    if s3 >= L:
        e3 = opt_ey[0] if s3 - L <= opt_s[0] else interp1d(opt_s, opt_ey, s3 - L)
    else:
        e3 = opt_ey[0] if s3 <= opt_s[0] else interp1d(opt_s, opt_ey, s3)
    e0 = x_wrapped[5]
    out = dict(bez_s=np.zeros((R, N + 1)), bez_ey=np.zeros((R, N + 1)), ey_lb=np.zeros((R, N)), active=np.zeros((R, N, 2), dtype=bool),
               ey_ub=np.full(R, track_width - 0.5 * veh_width), x0=np.tile(np.asarray(x_raw, dtype=float), (R, 1)))
    for r in range(R):
        rr = min(r, nv)   # regions past the scene's vehicles repeat the last one
        if nv == 0:
            e12 = e3
        elif rr == 0:
            e12 = 0.8 * track_width - (-veh_info[rr, 1] - 0.5 * veh_width) * 0.2
        elif rr == nv:
            e12 = -0.8 * track_width + ((veh_info[rr - 1, 1] - 0.5 * veh_width)) * 0.2
        else:
            e12 = 0.7 * (veh_info[rr, 1] + 0.5 * veh_width) + 0.3 * (veh_info[rr - 1, 1] - 0.5 * veh_width)
        for j in range(N + 1):
            t = j * (1.0 / N)
            out["bez_s"][r, j] = s0 * ((1 - t) ** 3) + 3 * s1 * t * ((1 - t) ** 2) + 3 * s2 * (t ** 2) * (1 - t) + s3 * (t ** 3)
            out["bez_ey"][r, j] = e0 * ((1 - t) ** 3) + 3 * e12 * t * ((1 - t) ** 2) + 3 * e12 * (t ** 2) * (1 - t) + e3 * (t ** 3)
        for k in range(N):
            lb = -track_width + 0.5 * veh_width
            s_nom = x_wrapped[4] + k * dt_ref * x_wrapped[0]
            for side, v in enumerate((r - 1, r)):
                if v < 0 or v >= nv:
                    continue
                os_ = wrap_above(obs_s[v, k], L)
                if (s_nom >= os_ - veh_length - safety_margin) & (s_nom <= os_ + veh_length + safety_margin):
                    out["active"][r, k, side] = True
                    lb = max(lb, obs_ey[v, k] + veh_width + safety_margin)
            out["ey_lb"][r, k] = lb
    return out


def select(n_veh, X, obs_s, obs_ey, old_flag, N, V, L, veh_length=0.4, veh_width=0.2):
    """One scene of crx_select.  X [V+1,N+1,6].  old_flag < 0: None.  A point whose circle value is not >= 0 (a NaN included) is a hit."""
    R = V + 1
    nv = min(max(int(n_veh), 0), V)
    cost = np.full(R, np.inf)
    for r in range(nv + 1):
        c = -10 * (X[r, N, 4] - X[r, 0, 4])
        for v in (r - 1, r):
            if v < 0 or v >= nv:
                continue
            for j in range(N + 1):
                os_ = wrap_above(obs_s[v, j], L)
                diffs, diffey = X[r, j, 4] - os_, X[r, j, 5] - obs_ey[v, j]
                if diffs ** 2 + diffey ** 2 - veh_length ** 2 - veh_width ** 2 >= 0:
                    c += 0
                else:
                    c += 100
        if old_flag >= 0 and old_flag != r:
            c += 100
        cost[r] = c
    flag = 0
    for r in range(1, nv + 1):   # list.index(min(...)): the first smallest
        if cost[r] < cost[flag]:
            flag = r
    return dict(flag=flag, sel_cost=cost, best_X=X[flag].copy())


def window(s_ego, vx, s_obs, L, safety_time=2.0):
    """control.py:291-292, :304-308 / :500-503, :518-522: (kept, lap offset) of one obstacle."""
    margin = vx * safety_time
    num_cycle_ego = int(s_ego / L)
    dist_ego = s_ego - num_cycle_ego * L
    num_cycle_obs = int(s_obs / L)
    dist_obs = s_obs - num_cycle_obs * L
    keep = (dist_ego > dist_obs - margin) & (dist_ego < dist_obs + margin)
    return bool(keep), (num_cycle_ego - num_cycle_obs) * L


def _pack(rows, V, N1):
    out = dict(obs_s=np.zeros((V, N1)), obs_ey=np.zeros((V, N1)), lap_off=np.zeros(V), n_obs=len(rows))
    for n, (s, e, off) in enumerate(rows):
        out["obs_s"][n], out["obs_ey"][n], out["lap_off"][n] = s, e, off
    return out


def track_prep(x, n_veh, obs_s_in, obs_ey_in, traj, N, V, L, safety_time=2.0, dt_ref=0.1):
    """One race of crx_track_prep_dev.  obs_*_in [V,N+1] in scene order, traj [N+1,6]."""
    vx = x[0]
    xt = np.zeros((N + 1, 6))
    ts, te = traj[:, 4], traj[:, 5]
    for i in range(N + 1):
        s_tmp = vx * dt_ref * i + x[4]
        if s_tmp < ts[0]:
            s_tmp = ts[0]
        if s_tmp >= ts[-1]:
            s_tmp = ts[-1]
        xt[i] = (vx, 0, 0, 0, 0, interp1d(ts, te, s_tmp))
    rows = []
    for v in range(min(max(int(n_veh), 0), V)):
        keep, off = window(x[4], vx, obs_s_in[v, 0], L, safety_time)
        if keep:
            rows.append((obs_s_in[v], obs_ey_in[v], off))
    out = _pack(rows, V, N + 1)
    out["xt"] = xt
    return out


def cbf_prep(xcurv, car_s0, car_v, car_ey, t, dt, N, L, safety_time=2.0):
    """One race of crx_cbf_prep_dev / crx_cbf_prep_laps_dev (L: the race's own lap length).  car_* [V]."""
    V = len(car_s0)
    rows = []
    for v in range(V):
        s = np.array([car_v[v] * (t + j * dt) + car_s0[v] for j in range(N + 1)])
        e = np.array([car_ey[v] + 0.0 * (t + j * dt) for j in range(N + 1)])
        keep, off = window(xcurv[4], xcurv[0], s[0], L, safety_time)
        if keep:
            rows.append((s, e, off))
    return _pack(rows, V, N + 1)


def traffic(car_s0, car_v, car_ey, t, dt, N, L):
    """One scripted car of crx_game_traffic_dev: the state after forward_dynamics + update_memory (s taken back by one lap once it
    is past the line) and the unwrapped predictions at t + j dt."""
    s = car_v * t + car_s0
    if s > L:
        s = s - L
    x = np.array([car_v, 0.0, 0.0, 0.0, s, car_ey])
    ps = np.array([car_v * (t + j * dt) + car_s0 for j in range(N + 1)])
    pe = np.array([car_ey + 0.0 * (t + j * dt) for j in range(N + 1)])
    return x, ps, pe
