"""The launches tests/test_front_edges_cpu.py and tests/test_gpu_front_edges.py make of tests/golden/front_edges.npz, and what a
result must equal: the reference's recorded answer where the fixture has one, tests/front_model.py everywhere.  numpy only.

A `batch` is a dict of the input arrays of one entry in the C ABI's layout, `names` (one per scene / race) and `rec`, the recorded
answers.  The check_* functions take the result of the entry as the numpy wrappers return it (a dict of arrays) and raise on the
first case that differs, naming it.  Decisions, integers and copies are held bit for bit; Bezier polylines to 1e-14 and per-stage
targets to 1e-13, the bounds tests/test_gpu_parity.py holds the same kernels to on recorded scenarios.
"""
import os

import numpy as np

import front_model as fm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "front_edges.npz")
BEZ_TOL, TARGET_TOL = 1e-14, 1e-13
SAFETY_MARGIN = 0.15


def load():
    z = np.load(GOLDEN, allow_pickle=False)
    return {k: z[k] for k in z.files}


def group(Z, g):
    return {k[len(g) + 1:]: v for k, v in Z.items() if k.startswith(g + "/")}


def _eq(a, b, what):
    np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=what)


# ---- crx_planner_scene ----------------------------------------------------------------------------------------------------------
def scene_batch(Z, N, VA, V):
    """Every interest case (one car around), every plan{N} scene that fits VA cars and V slots, every overflow case for V slots."""
    L, N1 = float(Z["L"]), N + 1
    names, ego, n_all, veh, ps, pe, rec = [], [], [], [], [], [], []
    it = group(Z, "interest")
    for i, nm in enumerate(it["names"]):
        v = np.zeros((VA, 6))
        v[0] = (it["agent_v"][i], 0, 0, 0, it["agent_s"][i], 0.25)
        names.append("interest/" + str(nm)), ego.append([it["ego_v"][i], 0, 0, 0, it["ego_s"][i], 0.0]), n_all.append(1), veh.append(v)
        ps.append(np.zeros((VA, N1))), pe.append(np.full((VA, N1), 0.25))
        rec.append(dict(n_veh=int(it["want"][i])))
    pl = group(Z, "plan%d" % N)
    for i, nm in enumerate(pl["names"]):
        K, nv = int(pl["n_all"][i]), int(pl["interest"][i].sum())
        if K > VA or nv > V:
            continue
        v, s, e = np.zeros((VA, 6)), np.zeros((VA, N1)), np.zeros((VA, N1))
        v[:K], s[:K], e[:K] = pl["veh"][i, :K], pl["pred_s"][i, :K], pl["pred_ey"][i, :K]
        names.append("plan/" + str(nm)), ego.append(pl["x_raw"][i]), n_all.append(K), veh.append(v), ps.append(s), pe.append(e)
        rec.append(dict(n_veh=nv, order=pl["order"][i, :nv], veh_info=pl["veh_info"][i, :nv], max_dv=pl["max_dv"][i],
                        interest=np.nonzero(pl["interest"][i])[0]))
    ov = group(Z, "overflow")
    for i, nm in enumerate(ov["names"]):
        K = int(ov["n_all"][i])
        if int(ov["V"][i]) != V or K > VA:
            continue
        v = np.zeros((VA, 6))
        v[:K] = ov["veh"][i, :K]
        e = np.tile(v[:, 5:6], (1, N1))
        names.append("overflow/" + str(nm)), ego.append(ov["ego"][i]), n_all.append(K), veh.append(v), ps.append(np.tile(v[:, 4:5], (1, N1))), pe.append(e)
        rec.append(None)
    return dict(names=names, ego=np.array(ego), n_all=np.array(n_all, dtype=np.int32), veh=np.array(veh), pred_s=np.array(ps), pred_ey=np.array(pe),
                rec=rec, L=L, N=N, VA=VA, V=V, length=float(Z["length"]))


SCENE_KEYS = ("n_veh", "overflow", "order", "veh_info", "max_dv", "obs_s", "obs_ey")


def scene_model(b):
    out = [fm.scene(b["ego"][i], int(b["n_all"][i]), b["veh"][i], b["pred_s"][i], b["pred_ey"][i], b["L"], b["V"], length=b["length"])
           for i in range(len(b["names"]))]
    return {k: np.array([o[k] for o in out]) for k in SCENE_KEYS}


def check_scene(res, b, model=None):
    model = scene_model(b) if model is None else model
    for i, nm in enumerate(b["names"]):
        r = b["rec"][i]
        if r is not None:   # the reference's own decisions
            assert res["n_veh"][i] == r["n_veh"] and res["overflow"][i] == 0, (nm, res["n_veh"][i], r["n_veh"])
            if "order" in r:
                nv = r["n_veh"]
                _eq(res["order"][i, :nv], r["order"], nm + ": sorted order")
                _eq(res["veh_info"][i, :nv], r["veh_info"], nm + ": veh_info")
                assert res["max_dv"][i] == r["max_dv"], (nm, "max_dv")
                _eq(res["obs_s"][i, :nv], b["pred_s"][i][r["order"]], nm + ": obs_s")
                _eq(res["obs_ey"][i, :nv], b["pred_ey"][i][r["order"]], nm + ": obs_ey")
        for k in SCENE_KEYS:
            _eq(res[k][i], model[k][i], "%s: %s against the model" % (nm, k))


# ---- crx_planner_prep -----------------------------------------------------------------------------------------------------------
def prep_batch(Z, N, V):
    pl = group(Z, "plan%d" % N)
    N1 = N + 1
    keep = [i for i in range(len(pl["names"])) if int(pl["interest"][i].sum()) <= V]
    b = dict(names=[str(pl["names"][i]) for i in keep], x_wrapped=pl["x_wrapped"][keep], x_raw=pl["x_raw"][keep], N=N, V=V, L=float(Z["L"]),
             opt_s=Z["opt_s"], opt_ey=Z["opt_ey"], length=float(Z["length"]), width=float(Z["width"]), track_width=float(Z["track_width"]),
             max_dv=pl["max_dv"][keep], rec=[])
    S = len(keep)
    b["n_veh"], b["veh_info"] = np.zeros(S, dtype=np.int32), np.zeros((S, V, 3))
    b["obs_s"], b["obs_ey"] = np.zeros((S, V, N1)), np.zeros((S, V, N1))
    for q, i in enumerate(keep):
        nv = int(pl["interest"][i].sum())
        order = pl["order"][i, :nv]
        b["n_veh"][q] = nv
        b["veh_info"][q, :nv] = pl["veh_info"][i, :nv]
        b["obs_s"][q, :nv], b["obs_ey"][q, :nv] = pl["pred_s"][i][order], pl["pred_ey"][i][order]
        b["rec"].append(dict(nv=nv, bez=pl["bez"][i, :nv + 1], active=pl["active"][i, :nv + 1]))
    return b


PREP_KEYS = ("bez_s", "bez_ey", "ey_lb", "ey_ub", "x0", "active")


def prep_model(b):
    out = [fm.prep(b["x_wrapped"][i], b["x_raw"][i], b["n_veh"][i], b["veh_info"][i], b["max_dv"][i], b["obs_s"][i], b["obs_ey"][i], b["opt_s"],
                   b["opt_ey"], b["N"], b["V"], b["track_width"], b["L"], veh_length=b["length"], veh_width=b["width"]) for i in range(len(b["names"]))]
    return {k: np.array([o[k] for o in out]) for k in PREP_KEYS}


def lb_from_active(b, i, active):
    """The bounds the recorded decisions imply: max over the closed windows of ey_obs + width + margin, else the track's."""
    nv, N = b["rec"][i]["nv"], b["N"]
    lb = np.full((nv + 1, N), -b["track_width"] + 0.5 * b["width"])
    for r in range(nv + 1):
        for k in range(N):
            for side, v in enumerate((r - 1, r)):
                if active[r, k, side]:
                    lb[r, k] = max(lb[r, k], b["obs_ey"][i, v, k] + b["width"] + SAFETY_MARGIN)
    return lb


def check_prep(res, b, model=None):
    """res in crx_planner_prep's layout: arrays with leading dimension S (V + 1)."""
    model = prep_model(b) if model is None else model
    S, R, N = len(b["names"]), b["V"] + 1, b["N"]
    bez_s, bez_ey, lb = res["bez_s"].reshape(S, R, N + 1), res["bez_ey"].reshape(S, R, N + 1), res["ey_lb"].reshape(S, R, N)
    ub, x0 = res["ey_ub"].reshape(S, R), res["x0"].reshape(S, R, 6)
    for i, nm in enumerate(b["names"]):
        r = b["rec"][i]
        nv = r["nv"]
        np.testing.assert_allclose(bez_s[i, :nv + 1], r["bez"][:, :, 0], rtol=0, atol=BEZ_TOL, err_msg=nm + ": bez_s against the reference")
        np.testing.assert_allclose(bez_ey[i, :nv + 1], r["bez"][:, :, 1], rtol=0, atol=BEZ_TOL, err_msg=nm + ": bez_ey against the reference")
        _eq(lb[i, :nv + 1], lb_from_active(b, i, r["active"]), nm + ": ey_lb against the reference's windows")
        np.testing.assert_allclose(bez_s[i], model["bez_s"][i], rtol=0, atol=BEZ_TOL, err_msg=nm + ": bez_s against the model")
        np.testing.assert_allclose(bez_ey[i], model["bez_ey"][i], rtol=0, atol=BEZ_TOL, err_msg=nm + ": bez_ey against the model")
        _eq(lb[i], model["ey_lb"][i], nm + ": ey_lb against the model")
        _eq(ub[i], model["ey_ub"][i], nm + ": ey_ub")
        _eq(x0[i], model["x0"][i], nm + ": x0")


# ---- crx_select -----------------------------------------------------------------------------------------------------------------
def select_batch(Z, N, V):
    pl = group(Z, "plan%d" % N)
    N1 = N + 1
    keep = [i for i in range(len(pl["names"])) if pl["has_X"][i] and int(pl["interest"][i].sum()) <= V]
    S = len(keep)
    b = dict(names=[str(pl["names"][i]) for i in keep], N=N, V=V, L=float(Z["L"]), length=float(Z["length"]), width=float(Z["width"]),
             n_veh=np.zeros(S, dtype=np.int32), X=np.zeros((S, V + 1, N1, 6)), obs_s=np.zeros((S, V, N1)), obs_ey=np.zeros((S, V, N1)),
             old_flag=pl["old_flag"][keep].astype(np.int32), rec=pl["flag"][keep])
    for q, i in enumerate(keep):
        nv = int(pl["interest"][i].sum())
        order = pl["order"][i, :nv]
        b["n_veh"][q] = nv
        b["X"][q, :nv + 1] = pl["X"][i, :nv + 1]
        b["obs_s"][q, :nv], b["obs_ey"][q, :nv] = pl["pred_s"][i][order], pl["pred_ey"][i][order]
    return b


SELECT_KEYS = ("flag", "sel_cost", "best_X")


def select_model(b):
    out = [fm.select(b["n_veh"][i], b["X"][i], b["obs_s"][i], b["obs_ey"][i], int(b["old_flag"][i]), b["N"], b["V"], b["L"], b["length"], b["width"])
           for i in range(len(b["names"]))]
    return {k: np.array([o[k] for o in out]) for k in SELECT_KEYS}


def check_select(res, b, model=None):
    model = select_model(b) if model is None else model
    for i, nm in enumerate(b["names"]):
        assert res["flag"][i] == b["rec"][i], (nm, "flag", res["flag"][i], "the reference chose", b["rec"][i])
        _eq(res["best_X"][i], b["X"][i, b["rec"][i]], nm + ": best_X")            # (NaN == NaN in assert_array_equal)
        for k in SELECT_KEYS:
            _eq(res[k][i], model[k][i], "%s: %s against the model" % (nm, k))


# ---- obstacle windows: crx_cbf_prep(_laps)_dev and crx_track_prep_dev -------------------------------------------------------------
PAD_CARS = ((8.0, 0.0, 0.375), (8.5, 0.0, -0.375), (9.0, 0.0, 0.625))   # standing cars outside every window of the fixture


def cbf_batch(Z, N, laps, V=3):
    """laps: the lap lengths whose window groups go into the launch, e.g. (16,) or (16, 32): race b folds by lap[b]."""
    b = dict(names=[], x=[], car_s0=[], car_v=[], car_ey=[], lap=[], rec=[], N=N, V=V, t=float(Z["t"]), dt=float(Z["dt"]))
    for L in laps:
        w = group(Z, "win%d_%d" % (N, L))
        for i, nm in enumerate(w["names"]):
            pad = np.array(PAD_CARS[: V - 3]).reshape(-1, 3)
            b["names"].append("L%d/%s" % (L, nm)), b["x"].append(w["x"][i]), b["lap"].append(float(L))
            b["car_s0"].append(np.r_[w["car_s0"][i], pad[:, 0]]), b["car_v"].append(np.r_[w["car_v"][i], pad[:, 1]])
            b["car_ey"].append(np.r_[w["car_ey"][i], pad[:, 2]])
            n = int(w["n_obs"][i])
            kept = w["kept"][i, :n]
            b["rec"].append(dict(n_obs=n, obs_s=w["pred_s"][i][kept], obs_ey=w["pred_ey"][i][kept], lap_off=w["lap_off"][i, :n]))
    for k in ("x", "car_s0", "car_v", "car_ey", "lap"):
        b[k] = np.array(b[k], dtype=np.float64)
    return b


NLP_KEYS = ("obs_s", "obs_ey", "lap_off", "n_obs")


def cbf_model(b):
    out = [fm.cbf_prep(b["x"][i], b["car_s0"][i], b["car_v"][i], b["car_ey"][i], b["t"], b["dt"], b["N"], b["lap"][i]) for i in range(len(b["names"]))]
    return {k: np.array([o[k] for o in out]) for k in NLP_KEYS}


def _check_packed(res, i, nm, r, V):
    n = r["n_obs"]
    assert res["n_obs"][i] == n, (nm, "n_obs", res["n_obs"][i], "the reference kept", n)
    _eq(res["obs_s"][i, :n], r["obs_s"], nm + ": kept predictions (s)")
    _eq(res["obs_ey"][i, :n], r["obs_ey"], nm + ": kept predictions (ey)")
    _eq(res["lap_off"][i, :n], r["lap_off"], nm + ": lap offsets")
    assert not res["obs_s"][i, n:].any() and not res["obs_ey"][i, n:].any() and not res["lap_off"][i, n:].any(), (nm, "the rest is zeroed")


def check_cbf(res, b, model=None):
    model = cbf_model(b) if model is None else model
    for i, nm in enumerate(b["names"]):
        _check_packed(res, i, nm, b["rec"][i], b["V"])
        for k in NLP_KEYS:
            _eq(res[k][i], model[k][i], "%s: %s against the model" % (nm, k))


def track_batch(Z, N, V=3):
    """The window cases as control.mpc_multi_agents saw them (its own predictions, the sorted vehicles only) on a fixed trajectory,
    then the per-stage target cases with no vehicle."""
    N1 = N + 1
    w, tg = group(Z, "win%d_16" % N), group(Z, "target%d" % N)
    b = dict(names=[], x=[], n_veh=[], obs_s_in=[], obs_ey_in=[], traj=[], rec=[], N=N, V=V, L=float(Z["L"]))
    for i, nm in enumerate(w["names"]):
        s, e = np.zeros((V, N1)), np.zeros((V, N1))
        s[:3], e[:3] = w["mma_pred_s"][i], w["mma_pred_ey"][i]
        b["names"].append("window/" + str(nm)), b["x"].append(w["x"][i]), b["n_veh"].append(int(w["mma_n_veh"][i])), b["obs_s_in"].append(s)
        b["obs_ey_in"].append(e), b["traj"].append(tg["traj"])
        n = int(w["mma_n_obs"][i])
        kept = w["mma_kept"][i, :n]
        b["rec"].append(dict(n_obs=n, obs_s=s[kept], obs_ey=e[kept], lap_off=w["mma_lap_off"][i, :n]))
    for i, nm in enumerate(tg["names"]):
        b["names"].append("target/" + str(nm)), b["x"].append(tg["x"][i]), b["n_veh"].append(0), b["obs_s_in"].append(np.zeros((V, N1)))
        b["obs_ey_in"].append(np.zeros((V, N1))), b["traj"].append(tg["traj"])
        b["rec"].append(dict(n_obs=0, obs_s=np.zeros((0, N1)), obs_ey=np.zeros((0, N1)), lap_off=np.zeros(0), xt_ey=tg["xt_ey"][i]))
    for k in ("x", "obs_s_in", "obs_ey_in", "traj"):
        b[k] = np.array(b[k], dtype=np.float64)
    b["n_veh"] = np.array(b["n_veh"], dtype=np.int32)
    return b


def track_model(b):
    out = [fm.track_prep(b["x"][i], b["n_veh"][i], b["obs_s_in"][i], b["obs_ey_in"][i], b["traj"][i], b["N"], b["V"], b["L"]) for i in range(len(b["names"]))]
    return {k: np.array([o[k] for o in out]) for k in NLP_KEYS + ("xt",)}


def check_track(res, b, model=None):
    model = track_model(b) if model is None else model
    for i, nm in enumerate(b["names"]):
        r = b["rec"][i]
        _check_packed(res, i, nm, r, b["V"])
        if "xt_ey" in r:
            np.testing.assert_allclose(res["xt"][i, :, 5], r["xt_ey"], rtol=0, atol=TARGET_TOL, err_msg=nm + ": targets against the reference")
        _eq(res["xt"][i, :, :5], model["xt"][i, :, :5], nm + ": xt columns 0..4")
        np.testing.assert_allclose(res["xt"][i, :, 5], model["xt"][i, :, 5], rtol=0, atol=TARGET_TOL, err_msg=nm + ": targets against the model")
        for k in NLP_KEYS:
            _eq(res[k][i], model[k][i], "%s: %s against the model" % (nm, k))


# ---- crx_game_traffic_dev -------------------------------------------------------------------------------------------------------
def traffic_batch(Z, N, shape):
    """The scripted cars as [races, cars] = shape (the cases fill it row by row; it must hold them all exactly)."""
    tr = group(Z, "traffic")
    n = len(tr["names"])
    assert shape[0] * shape[1] == n
    return dict(names=[str(x) for x in tr["names"]], s0=tr["s0"].reshape(shape), v=tr["v"].reshape(shape), ey=tr["ey"].reshape(shape), N=N,
                L=float(Z["L"]), t=float(Z["t"]), dt=float(Z["dt"]), rec=dict(x=tr["x"], pred_s=tr["pred_s"][:, :N + 1], pred_ey=tr["pred_ey"][:, :N + 1]))


TRAFFIC_KEYS = ("veh_xcurv", "pred_s", "pred_ey")


def traffic_model(b):
    out = [fm.traffic(s0, v, ey, b["t"], b["dt"], b["N"], b["L"]) for s0, v, ey in zip(b["s0"].ravel(), b["v"].ravel(), b["ey"].ravel())]
    return {k: np.array([o[j] for o in out]) for j, k in enumerate(TRAFFIC_KEYS)}


def check_traffic(res, b, model=None):
    """res: veh_xcurv [n,6], pred_s, pred_ey [n,N+1], flattened over (race, car)."""
    model = traffic_model(b) if model is None else model
    for i, nm in enumerate(b["names"]):
        _eq(res["veh_xcurv"][i], b["rec"]["x"][i], nm + ": state against the reference")
        _eq(res["pred_s"][i], b["rec"]["pred_s"][i], nm + ": pred_s against the reference")
        _eq(res["pred_ey"][i], b["rec"]["pred_ey"][i], nm + ": pred_ey against the reference")
        for k in TRAFFIC_KEYS:
            _eq(res[k][i], model[k][i], "%s: %s against the model" % (nm, k))
