"""NumPy model of the race statistics (include/crx.h "Race statistics", S1-S4), written from the specification with plain loops per
car, sample and opponent -- not from the kernel.  Every floating-point operation is one NumPy float64 operation (no fused
multiply-add), so the kernel, which is compiled with contraction off, must reproduce the bits.

    st = reset(batch, n_opp_max, laps)
    sample(st, k, xcurv, laps, L, track_width, ...)        # in place; scripted mode or field mode (n_cars > 0)
    summary(st, group, n_groups)                           # list of records (dicts), one per group
"""
import numpy as np

MAX_LAPS = 8
INT_FIELDS = ("n_samples", "nonfinite_step", "off_step", "off_samples", "contact_step", "contact_samples", "n_laps", "laps_prev",
              "passes", "passed", "flag_samples")
RESET_I = dict(n_samples=0, nonfinite_step=-1, off_step=-1, off_samples=0, contact_step=-1, contact_samples=0, n_laps=0, passes=0,
               passed=0, flag_samples=0)


def reset(batch, n_opp_max, laps):
    st = {k: np.full(batch, v, dtype=np.int32) for k, v in RESET_I.items()}
    st["laps_prev"] = np.array(laps, dtype=np.int32).copy()
    st["lap_step"] = np.full((MAX_LAPS, batch), -1, dtype=np.int32)
    st["min_clear"] = np.full(batch, np.inf)
    st["ey_max"] = np.zeros(batch)
    st["sum_ey2"] = np.zeros(batch)
    st["sum_dv2"] = np.zeros(batch)
    st["ds_prev"] = np.full((n_opp_max, batch), np.nan)
    return st


def dim_or_default(v, dflt):
    return dflt if (not (v > 0.0) or not np.isfinite(v)) else v


def gap(s_ego, s_opp, L):
    """the lap-folded signed gap: fmod, a negative remainder moved up by L, minus half a lap"""
    with np.errstate(invalid="ignore"):
        m = np.fmod(np.float64(s_ego) - np.float64(s_opp) + L / 2, L)
    if m < 0:
        m = m + L
    return m - L / 2


def ellipse(ds, dey, l_sum, w_sum, degree):
    a, b = np.float64(ds) / np.float64(l_sum), np.float64(dey) / np.float64(w_sum)
    pa, pb = np.float64(1.0), np.float64(1.0)
    for _ in range(degree):
        pa, pb = pa * a, pb * b
    return pa + pb


def sample(st, k, xcurv, laps, L, track_width, t=0.0, car_s0=None, car_v=None, car_ey=None, n_opp=None, n_cars=0, car_dims=None, xt=None,
           flag=None, degree=6, l_sum=0.4, w_sum=0.2):
    xcurv = np.asarray(xcurv, dtype=np.float64).reshape(-1, 6)
    Bn, V = xcurv.shape[0], st["ds_prev"].shape[0]
    L = np.float64(L)
    dims = None if car_dims is None else np.asarray(car_dims, dtype=np.float64).reshape(-1, 2)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(Bn):
            x = xcurv[b]
            # lap counters: integers, whatever the state is
            d = int(laps[b]) - int(st["laps_prev"][b])
            st["laps_prev"][b] = laps[b]
            if d > 0:
                for q in range(d):
                    if st["n_laps"][b] + q < MAX_LAPS:
                        st["lap_step"][st["n_laps"][b] + q, b] = k
                st["n_laps"][b] += d
            if not np.all(np.isfinite(x)):
                if st["nonfinite_step"][b] < 0:
                    st["nonfinite_step"][b] = k
                st["ds_prev"][:, b] = np.nan
                continue
            st["n_samples"][b] += 1
            vx, s_e, ey_e = x[0], x[4], x[5]
            if abs(ey_e) > track_width:
                if st["off_step"][b] < 0:
                    st["off_step"][b] = k
                st["off_samples"][b] += 1
            st["ey_max"][b] = max(st["ey_max"][b], abs(ey_e))
            st["sum_ey2"][b] = st["sum_ey2"][b] + ey_e * ey_e
            if xt is not None:
                dv = vx - xt[b][0]
                st["sum_dv2"][b] = st["sum_dv2"][b] + dv * dv
            # the opponents of this car: (slot, s, ey, l_sum, w_sum)
            opp = []
            if n_cars > 0:
                r, c = divmod(b, n_cars)
                for j, o in enumerate(o for o in range(n_cars) if o != c):
                    ro = r * n_cars + o
                    ls, ws = l_sum, w_sum
                    if dims is not None:
                        ls = dim_or_default(dims[b, 0], l_sum) / 2 + dim_or_default(dims[ro, 0], l_sum) / 2
                        ws = dim_or_default(dims[b, 1], w_sum) / 2 + dim_or_default(dims[ro, 1], w_sum) / 2
                    opp.append((j, xcurv[ro, 4], xcurv[ro, 5], ls, ws))
            else:
                n = V if n_opp is None else min(max(int(n_opp[b]), 0), V)
                for j in range(n):
                    opp.append((j, np.float64(car_v[b][j]) * np.float64(t) + np.float64(car_s0[b][j]), car_ey[b][j], l_sum, w_sum))
            clear = np.inf
            for j, s_o, ey_o, ls, ws in opp:
                if not (np.isfinite(s_o) and np.isfinite(ey_o)):
                    st["ds_prev"][j, b] = np.nan
                    continue
                ds = gap(s_e, s_o, L)
                h = ellipse(ds, ey_e - ey_o, ls, ws, degree)
                if h < clear:
                    clear = h
                p = st["ds_prev"][j, b]
                if np.isfinite(p) and np.isfinite(ds):
                    if p < 0 and ds >= 0 and ds - p < L / 2:
                        st["passes"][b] += 1
                    if p >= 0 and ds < 0 and p - ds < L / 2:
                        st["passed"][b] += 1
                st["ds_prev"][j, b] = ds
            if clear < st["min_clear"][b]:
                st["min_clear"][b] = clear
            if clear < 1.0:
                if st["contact_step"][b] < 0:
                    st["contact_step"][b] = k
                st["contact_samples"][b] += 1
            if flag is not None and flag[b] != 0:
                st["flag_samples"][b] += 1
    return st


def summary(st, group=None, n_groups=1):
    Bn = st["n_samples"].shape[0]
    recs = []
    for g in range(n_groups if group is not None else 1):
        cars = [b for b in range(Bn) if group is None or group[b] == g]
        nf = [st["nonfinite_step"][b] >= 0 for b in cars]
        off = [st["off_step"][b] >= 0 for b in cars]
        hit = [st["contact_step"][b] >= 0 for b in cars]
        lap1 = [int(st["lap_step"][0, b]) for b in cars if st["lap_step"][0, b] >= 0]
        lap2 = [int(st["lap_step"][1, b]) - int(st["lap_step"][0, b]) for b in cars if st["lap_step"][0, b] >= 0 and st["lap_step"][1, b] >= 0]
        rec = dict(cars=len(cars), nonfinite=sum(nf), off=sum(off), contact=sum(hit),
                   clean=sum(not (a or b or c) for a, b, c in zip(nf, off, hit)),
                   laps_hist=[sum(min(int(st["n_laps"][b]), MAX_LAPS) == k for b in cars) for k in range(MAX_LAPS + 1)])
        for name in ("passes", "passed", "flag_samples", "n_samples"):
            rec[name] = sum(int(st[name][b]) for b in cars)
        for name, v in (("lap1", lap1), ("lap2", lap2)):
            rec[name + "_sum"], rec[name + "_count"] = sum(v), len(v)
            rec[name + "_min"], rec[name + "_max"] = (min(v), max(v)) if v else (-1, -1)
        rec["min_clear"] = float(min([st["min_clear"][b] for b in cars], default=np.inf))
        rec["ey_max"] = float(max([st["ey_max"][b] for b in cars], default=0.0))
        recs.append({k: (int(v) if isinstance(v, (bool, np.bool_, np.integer)) else v) for k, v in rec.items()})
    return recs
