"""NumPy restatement of crx_field_traffic (include/crx.h "Field games", quirks F1-F3, F5, F6, G1-G3), written from its specification with
plain loops on top of tests/field_model.predict: every car's zero-input roll-out, and per ego the other cars of its race in car order --
their current states and their roll-out rows, copied.  Also the windows of check_ego_agent_distance (planning/planner_helper.py:218-266),
which a test uses to place cars inside each other's view.  Nothing of the product is imported."""
import numpy as np

import field_model as fm


def traffic(track, L, xcurv, N, dt=0.1):
    """xcurv [R, C, 6] -> pred_s_car, pred_ey_car [R, C, N+1]; veh_xcurv [R*C, V, 6], pred_s, pred_ey [R*C, V, N+1], n_all [R*C] (int32) with
    V = C - 1; plus `edge` and `cond` [R, C] of field_model.predict, what a draw is filtered by."""
    x = np.asarray(xcurv, dtype=float)
    R, C = x.shape[:2]
    V = C - 1
    ps, pe, edge, cond = fm.predict(track, L, x, N + 1, dt)
    veh = np.zeros((R * C, V, 6))
    pred_s, pred_ey = np.zeros((R * C, V, N + 1)), np.zeros((R * C, V, N + 1))
    for r in range(R):
        for e in range(C):
            v = 0
            for o in range(C):                       # car order, skipping the ego (F5)
                if o == e:
                    continue
                veh[r * C + e, v] = x[r, o]
                pred_s[r * C + e, v] = ps[r, o]
                pred_ey[r * C + e, v] = pe[r, o]
                v += 1
    return dict(pred_s_car=ps, pred_ey_car=pe, veh_xcurv=veh, pred_s=pred_s, pred_ey=pred_ey, n_all=np.full(R * C, V, dtype=np.int32),
                edge=edge, cond=cond)


def _wrap_above(s, L):
    while s > L:
        s -= L
    return s


def of_interest(ego, veh, L, veh_length=0.4, safety_factor=4.5, prediction_factor=0.5):
    """check_ego_agent_distance (planner_helper.py:218-266) for one ego state and one other vehicle's state: is the vehicle inside the ego's
    window -- ahead within safety_factor * length + prediction_factor * |dv|, or behind within one length, also across the line?  All
    comparisons: a NaN on either side answers False (G3)."""
    s_e, s_a = _wrap_above(float(ego[4]), L), _wrap_above(float(veh[4]), L)
    ahead = safety_factor * veh_length + prediction_factor * abs(float(ego[0]) - float(veh[0]))
    behind = 1.0 * veh_length
    return bool((s_a - s_e <= ahead and s_a >= s_e) or (s_a + L - s_e <= ahead and s_a + L >= s_e) or
                (s_e - s_a <= behind and s_a <= s_e) or (s_e + L - s_a <= behind and s_a <= s_e + L))
