"""NumPy restatement of crx_field_prep (include/crx.h, quirks F1-F7), written from its specification and batch-vectorised: the
predictions of every car of every race, the window test, the packing, the per-slot dimensions and `clear`.  Nothing of the product is
imported.  predict() and obstacles() are separate so that the second half can be fed someone else's predictions (the mirror's)."""
import numpy as np


def wrap_above(s, L):
    """`while s > L: s -= L`, element-wise; a non-finite entry stays what it is."""
    s = np.array(s, dtype=float)
    with np.errstate(invalid="ignore"):
        while True:
            over = (s > L) & np.isfinite(s)
            if not over.any():
                return s
            s = np.where(over, s - L, s)


def wrap_below(s, L):
    """`while s < 0: s += L`, element-wise."""
    s = np.array(s, dtype=float)
    with np.errstate(invalid="ignore"):
        while True:
            under = (s < 0) & np.isfinite(s)
            if not under.any():
                return s
            s = np.where(under, s + L, s)


def curvature(track, L, s):
    """Curvature at s folded into one lap: the first segment with lo <= s <= hi (F6); no segment (a NaN): 0.  Also returns the distance of
    the folded s to the nearest segment end."""
    lo, hi = track[:, 3], track[:, 3] + track[:, 4]
    sw = wrap_below(wrap_above(s, L), L)
    with np.errstate(invalid="ignore"):
        hit = (sw[..., None] >= lo) & (sw[..., None] <= hi)
    first = np.argmax(hit, axis=-1)
    curv = np.where(hit.any(axis=-1), track[first, 5], 0.0)
    edge = np.minimum(np.abs(sw[..., None] - lo), np.abs(sw[..., None] - hi)).min(axis=-1)
    return curv, edge


def predict(track, L, xcurv, n, dt=0.1):
    """n zero-input Euler steps of the curvilinear state (racing/offboard.py:51-94) for every row of xcurv [..., 6]: every right-hand side on
    the old state in the reference's expression order, the lap wrap after every step, the roll-out continuing from the wrapped value.
    Returns pred_s, pred_ey [..., n], `edge` [...]: the smallest distance of a visited s to a segment end or to the lap length, and `cond`
    [...]: the smallest |1 - curv ey| the roll-out divides by.  The curvilinear frame is singular at ey = 1 / curv (the centre of the
    curve): near it v_long, and with it every rounding error made so far, is amplified by 1 / (1 - curv ey)^2, and two correct float64
    implementations stop agreeing to 1e-12 (measured against an 80-bit roll-out: this model's own error is 2e-14 for cond >= 0.5 and
    2e-12 at cond = 3e-3).  A car ON a track of half-width 0.8 has cond >= 1 - 0.7 * 0.8 = 0.44 on these layouts."""
    x = np.asarray(xcurv, dtype=float)
    vx, vy, wz = x[..., 0], x[..., 1], x[..., 2]
    epsi, s, ey = x[..., 3].copy(), x[..., 4].copy(), x[..., 5].copy()
    ps, pe = np.zeros(x.shape[:-1] + (n,)), np.zeros(x.shape[:-1] + (n,))
    edge, cond = np.full(x.shape[:-1], np.inf), np.full(x.shape[:-1], np.inf)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(n):
            curv, e = curvature(track, L, s)
            v_long = (vx * np.cos(epsi) - vy * np.sin(epsi)) / (1 - curv * ey)
            epsi_n = epsi + dt * (wz - v_long * curv)
            s_n = s + dt * v_long
            ey_n = ey + dt * (vx * np.sin(epsi) + vy * np.cos(epsi))
            edge = np.fmin(edge, np.fmin(e, np.abs(s_n - L)))
            cond = np.fmin(cond, np.abs(1 - curv * ey))
            epsi, s, ey = epsi_n, wrap_above(s_n, L), ey_n
            ps[..., j], pe[..., j] = s, ey
    return ps, pe, edge, cond


def others(C):
    """[C, C-1]: for ego e, the other cars in car order (F5)."""
    return np.array([[o for o in range(C) if o != e] for e in range(C)], dtype=np.int64).reshape(C, C - 1)


def _dim(v, dflt):
    with np.errstate(invalid="ignore"):
        return np.where(~(v > 0.0) | ~np.isfinite(v), dflt, v)


def pair_dims(car_dims, l_sum=0.4, w_sum=0.2):
    """[R, C, V, 2]: (l_e / 2 + l_o / 2, w_e / 2 + w_o / 2) of every (ego, other) pair (control.py:532-535); a non-positive or non-finite
    length / width counts as l_sum / w_sum."""
    d = np.asarray(car_dims, dtype=float)
    d = np.stack([_dim(d[..., 0], l_sum), _dim(d[..., 1], w_sum)], axis=-1)
    return d[:, :, None, :] / 2 + d[:, others(d.shape[1])] / 2


def obstacles(pred_s, pred_ey, xcurv, L, safety_time=2.0, car_dims=None, l_sum=0.4, w_sum=0.2):
    """The obstacle arrays of the R * C NLPs from the predictions [R, C, N+1] and the current states [R, C, 6]: window test and lap offset on
    column 0 (F2; control.py:499-523, 538-540, int() toward zero), kept cars packed to the front in car order, the rest zero.  Returns a dict
    with obs_s, obs_ey [R,C,V,N+1], lap_off [R,C,V], n_obs [R,C] (int32), obs_dims [R,C,V,2] with car_dims, and `gap` [R,C]: the smallest
    distance of a window comparison to its threshold (and of the ego's s to a multiple of the lap length, where int() jumps)."""
    x = np.asarray(xcurv, dtype=float)
    R, C = x.shape[:2]
    V, oth = C - 1, others(C)
    os_all, oe_all = pred_s[:, oth], pred_ey[:, oth]                       # [R, C, V, N+1]
    with np.errstate(invalid="ignore"):
        margin = safety_time * x[..., 0]
        nce = np.trunc(x[..., 4] / L)
        dist_ego = x[..., 4] - nce * L
        s0 = os_all[..., 0]
        nco = np.trunc(s0 / L)
        dist_obs = s0 - nco * L
        lower, upper = dist_obs - margin[..., None], dist_obs + margin[..., None]
        keep = (dist_ego[..., None] > lower) & (dist_ego[..., None] < upper)
        off = (nce[..., None] - nco) * L
        gap = np.fmin(np.abs(dist_ego[..., None] - lower), np.abs(dist_ego[..., None] - upper))
        gap = np.fmin.reduce(gap, axis=-1, initial=np.inf)
        gap = np.fmin(gap, np.abs(x[..., 4] - np.round(x[..., 4] / L) * L))
    order = np.argsort(~keep, axis=-1, kind="stable")
    n = keep.sum(axis=-1).astype(np.int32)
    live = np.arange(V) < n[..., None]
    take = lambda a: np.take_along_axis(a, order.reshape(order.shape + (1,) * (a.ndim - 3)), axis=2)   # noqa: E731
    out = dict(obs_s=np.where(live[..., None], take(os_all), 0.0), obs_ey=np.where(live[..., None], take(oe_all), 0.0),
               lap_off=np.where(live, take(off), 0.0), n_obs=n, gap=gap)
    if car_dims is not None:
        out["obs_dims"] = np.where(live[..., None], take(pair_dims(car_dims, l_sum, w_sum)), 0.0)
    return out


def clear(xcurv, L, degree=6, car_dims=None, l_sum=0.4, w_sum=0.2):
    """[R, C]: min over the other cars of (ds / l_sum)^degree + (dey / w_sum)^degree at the current states, ds = (s_e - s_o + L / 2) % L -
    L / 2; a NaN never lowers it; +inf when C == 1."""
    x = np.asarray(xcurv, dtype=float)
    oth = others(x.shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        ds = (x[..., 4][..., None] - x[:, oth, 4] + L / 2) % L - L / 2
        dey = x[..., 5][..., None] - x[:, oth, 5]
        ls, ws = (l_sum, w_sum) if car_dims is None else np.moveaxis(pair_dims(car_dims, l_sum, w_sum), -1, 0)
        h = (ds / ls) ** degree + (dey / ws) ** degree
    return np.fmin.reduce(h, axis=-1, initial=np.inf)


def prep(track, L, xcurv, N, dt=0.1, safety_time=2.0, degree=6, car_dims=None, l_sum=0.4, w_sum=0.2):
    """All of crx_field_prep for xcurv [R, C, 6]: pred_s, pred_ey, obs_s, obs_ey, lap_off, n_obs, (obs_dims,) clear -- plus `edge`, `cond` and `gap`
    [R, C], what a draw is filtered by."""
    x = np.asarray(xcurv, dtype=float)
    ps, pe, edge, cond = predict(track, L, x, N + 1, dt)
    out = obstacles(ps, pe, x, L, safety_time, car_dims, l_sum, w_sum)
    out.update(pred_s=ps, pred_ey=pe, edge=edge, cond=cond, clear=clear(x, L, degree, car_dims, l_sum, w_sum))
    return out
