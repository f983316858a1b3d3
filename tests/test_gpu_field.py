"""Field races on the GPU: crx_field_prep_dev against the numpy model (tests/field_model.py) and the reference-recorded predictions
(tests/golden/field_pred.npz), its independence of the launch's shape, and crx.montecarlo.FieldRaces against the lone-car loop it must
reduce to, against the mirrored class surface, and in a long noisy sweep."""
import os

import numpy as np
import pytest

import conftest
import field_model as fm

pytestmark = pytest.mark.gpu

R_PREP = 37   # not a multiple of 256 // C for any C in 1 .. 7
N_FIXED = 4   # the races of a draw that are constructed, not drawn


@pytest.fixture(scope="module")
def gpu():
    import crx

    return crx.init(0)


def _track(name, width=0.8):
    from utils import racing_env

    return racing_env.ClosedTrack(np.genfromtxt(os.path.join(conftest.ROOT, "data/track_layout/%s.csv" % name), delimiter=","), track_width=width)


def _car(rng, s, vx=None, ey=None):
    return np.array([rng.uniform(0.3, 2.0) if vx is None else vx, rng.uniform(-0.2, 0.2), rng.uniform(-0.6, 0.6), rng.uniform(-0.3, 0.3), s,
                     rng.uniform(-0.6, 0.6) if ey is None else ey])


def _drawn_race(rng, L, C):
    """C cars within 6 m behind and ahead of a point drawn over the lap: some inside each other's windows, some outside, some bunches
    across the line."""
    return np.array([_car(rng, (rng.uniform(0.0, L) + rng.uniform(0.0, 6.0)) % L) for _ in range(C)])


def _keeps(m, r, e, o):
    """Does car e of race r keep car o?  (Its prediction row stands in one of e's live slots.)"""
    return any(np.array_equal(m["obs_s"][r, e, v], m["pred_s"][r, o]) for v in range(m["n_obs"][r, e]))


def _fixed_race(rng, L, C, which):
    """Race `which` of a draw (see draw()); the components the construction leaves free are drawn."""
    x = _drawn_race(rng, L, C)
    if which == 3:
        x[C - 1] = np.nan
    if C < 2 or which == 3:
        return x
    if which == 0:
        x[0], x[1] = _car(rng, L + 5.013, vx=1.2), _car(rng, 5.617, vx=0.8)
        if C >= 4:
            x[C - 2], x[C - 1] = _car(rng, L - 0.311, vx=1.0), _car(rng, 0.207, vx=1.0)
    elif which == 1:
        x[0], x[1] = _car(rng, L - 1.503, vx=1.5), _car(rng, L - 0.409, vx=1.0)
    elif which == 2:
        x = np.array([_car(rng, 3.137 + 0.25 * c, vx=1.2 if c == 0 else 0.5) for c in range(C)])
    return x


def draw(name, C, N, seed, R=R_PREP):
    """xcurv [R, C, 6], car_dims [R, C, 2] and the model's answer.  Races 0 .. 3 are constructed (as far as C cars allow):
      0  the ego (car 0) carries a whole lap in s and the car in front of it does not: a kept car with lap offset L.  (An ego just
         below L with the opponent just past the line cannot give a non-zero offset: column 0 of a prediction is wrapped into one lap,
         so only an ego with s >= L has one.  That pair is race 0's last two cars when C >= 4: neither keeps the other.)
      1  car 1 crosses the line inside the horizon and car 0, behind it, keeps it: a kept row that jumps by -L (F3)
      2  all cars bunched at 0.25 m spacing, car 0 fast: it has every other car in its window (six of them at C = 7)
      3  the last car's state is NaN
    The other races are drawn.  A race is drawn again -- a constructed one in its free components -- while a window comparison lies
    within 1e-9 of its threshold, a visited s within 1e-9 of a segment end or of the lap length, or a roll-out comes near the singularity
    of the curvilinear frame (|1 - curv ey| < 0.4, which no car on the track reaches: field_model.predict says why 1e-12 ends there)."""
    track = _track(name)
    tab, L = track.point_and_tangent, track.lap_length
    rng = np.random.default_rng(seed)
    race = lambda r: _fixed_race(rng, L, C, r) if r < N_FIXED else _drawn_race(rng, L, C)   # noqa: E731
    x = np.array([race(r) for r in range(R)])
    dims = np.stack([rng.uniform(0.3, 0.5, (R, C)), rng.uniform(0.15, 0.25, (R, C))], axis=-1)
    for _ in range(200):
        m = fm.prep(tab, L, x, N, car_dims=dims)
        bad = (m["edge"].min(axis=1) < 1e-9) | (m["gap"].min(axis=1) < 1e-9) | (m["cond"].min(axis=1) < 0.4)
        if not bad.any():
            break
        for r in np.nonzero(bad)[0]:
            x[r] = race(r)
    else:
        raise AssertionError("the draw does not settle: %s" % np.nonzero(bad)[0])
    # the constructed cases are what they were built to be
    if C >= 2:
        assert m["n_obs"][0, 0] >= 1 and m["lap_off"][0, 0, 0] == L
        assert m["n_obs"][1, 0] >= 1 and (np.diff(m["obs_s"][1, 0, 0]) < -0.5 * L).any()
        assert m["n_obs"][2, 0] == C - 1
        kept = m["n_obs"][N_FIXED:].sum()
        assert 0 < kept < (R - N_FIXED) * C * (C - 1)                            # cars inside and outside each other's windows
        assert _keeps(m, 0, 0, 1) and _keeps(m, 1, 0, 1)
    if C >= 4:
        assert not _keeps(m, 0, C - 2, C - 1) and not _keeps(m, 0, C - 1, C - 2)   # the pair across the line does not see each other
    assert np.isnan(m["pred_s"][3, C - 1]).all() and m["n_obs"][3, C - 1] == 0
    assert np.isfinite(np.delete(m["pred_s"].reshape(-1, N + 1), 3 * C + C - 1, axis=0)).all() and not np.isnan(m["obs_s"]).any()
    return tab, L, x, dims, m


def _run(desc, tab, x, dims=None, clear=True, n_races=None):
    """One crx_field_prep_dev launch; returns host arrays shaped as the model's."""
    import torch

    from crx import torch_api

    R, C = x.shape[:2]
    V, N1 = C - 1, desc.N + 1
    dev = torch.device("cuda", 0)
    ws = torch_api.FieldWorkspace(desc, R, dev, dims=dims is not None, clear=clear)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)   # noqa: E731
    torch_api.field_prep_dev(desc, t(tab), t(x.reshape(R * C, 6)), ws, car_dims=None if dims is None else t(dims))
    torch.cuda.synchronize()
    out = dict(pred_s=ws.pred_s, pred_ey=ws.pred_ey, obs_s=ws.obs_s.reshape(R, C, V, N1), obs_ey=ws.obs_ey.reshape(R, C, V, N1),
               lap_off=ws.lap_off.reshape(R, C, V), n_obs=ws.n_obs.reshape(R, C))
    if dims is not None:
        out["obs_dims"] = ws.obs_dims.reshape(R, C, V, 2)
    if clear:
        out["clear"] = ws.clear.reshape(R, C)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


@pytest.mark.parametrize("C", [1, 2, 4, 7])
def test_field_prep_matches_model(gpu, C):
    from crx import abi

    for name in ("l_shape", "m_shape"):
        for N in (10, 24):
            tab, L, x, dims, m_dims = draw(name, C, N, 100 * C + N)
            m_plain = fm.prep(tab, L, x, N)
            desc = abi.field_desc(N, C, tab.shape[0], L)
            for use_dims in (False, True):
                for clear in (False, True):
                    tag = (name, C, N, use_dims, clear)
                    m = m_dims if use_dims else m_plain
                    g = _run(desc, tab, x, dims if use_dims else None, clear)
                    assert g["n_obs"].dtype == np.int32 and np.array_equal(g["n_obs"], m["n_obs"]), tag
                    for k in ("pred_s", "pred_ey", "obs_s", "obs_ey", "lap_off"):
                        np.testing.assert_allclose(g[k], m[k], rtol=0, atol=1e-12, equal_nan=True, err_msg=str(tag + (k,)))
                    if use_dims:
                        assert np.array_equal(g["obs_dims"], m["obs_dims"]), tag
                    if clear:
                        np.testing.assert_allclose(g["clear"], m["clear"], rtol=1e-12, atol=0, err_msg=str(tag))
                        assert np.isinf(g["clear"]).all() == (C == 1)
                    # the NaN car poisons only its own predictions and is kept by nobody
                    nan_row = np.isnan(g["pred_s"]).any(axis=-1)
                    assert nan_row.sum() == 1 and nan_row[3, C - 1] and np.isnan(g["pred_s"][3, C - 1]).all() and np.isnan(g["pred_ey"][3, C - 1]).all(), tag
                    assert not np.isnan(g["obs_s"]).any() and not np.isnan(g["obs_ey"]).any() and g["n_obs"][3, C - 1] == 0, tag


def test_field_prep_reference_rows(gpu):
    """The states the reference's own DynamicBicycleModel predicted from, as single-car races and as the cars of mixed races of four."""
    from crx import abi

    z = np.load(os.path.join(conftest.GOLDEN, "field_pred.npz"), allow_pickle=False)
    for name in (str(t) for t in z["tracks"]):
        track = _track(name)
        tab, L = track.point_and_tangent, track.lap_length
        for N in (12, 24):
            g = "%s_N%d" % (name, N)
            x, ps, pe = z[g + "/xcurv"], z[g + "/pred_s"], z[g + "/pred_ey"]
            n = x.shape[0]
            for C in (1, 4):
                out = _run(abi.field_desc(N, C, tab.shape[0], L), tab, x.reshape(n // C, C, 6))
                np.testing.assert_allclose(out["pred_s"].reshape(n, N + 1), ps, rtol=0, atol=1e-12, err_msg="%s C=%d" % (g, C))
                np.testing.assert_allclose(out["pred_ey"].reshape(n, N + 1), pe, rtol=0, atol=1e-12, err_msg="%s C=%d" % (g, C))


def test_field_prep_independence(gpu):
    """A race's outputs depend on nothing but the race: not on the other races, on how many there are, or on where it sits in the launch;
    and the host-pointer entry gives the bits of the device entry."""
    import crx
    from crx import abi

    C, N, R = 4, 10, 150                                     # three blocks: 64 + 64 + 22 races
    tab, L, x, dims, m = draw("l_shape", C, N, 77, R=R)
    desc = abi.field_desc(N, C, tab.shape[0], L)
    full = _run(desc, tab, x, dims)
    assert np.array_equal(full["n_obs"], m["n_obs"]) and np.array_equal(full["obs_dims"], m["obs_dims"])
    for k in ("pred_s", "pred_ey", "obs_s", "obs_ey", "lap_off"):
        np.testing.assert_allclose(full[k], m[k], rtol=0, atol=1e-12, equal_nan=True, err_msg=k)
    again = _run(desc, tab, x, dims)
    for k in full:
        assert _same_bits(full[k], again[k]), k
    perm = np.random.default_rng(3).permutation(R)
    shuffled = _run(desc, tab, x[perm], dims[perm])
    for k in full:
        assert _same_bits(shuffled[k], full[k][perm]), k
    for pick in ([130], [2, 149, 70], list(range(60, 140))):   # other launch sizes, other blocks, other places in a block
        part = _run(desc, tab, x[pick], dims[pick])
        for k in full:
            assert _same_bits(part[k], full[k][pick]), (k, pick)
    host = crx.field_prep(desc, tab, x, dims)
    for k in full:
        assert _same_bits(np.asarray(host[k]), full[k]), k
    plain_host, plain = gpu.field_prep(desc, tab, x, None, clear=False), _run(desc, tab, x, None, clear=False)
    assert sorted(plain_host) == sorted(plain)
    for k in plain:
        assert _same_bits(np.asarray(plain_host[k]), plain[k]), k


def _globals(track, x):
    """Global states that go with curvilinear ones [n, 6] (velocities copied, pose from the track)."""
    g = np.array(x, dtype=float)
    for i in range(g.shape[0]):
        g[i, 3] = track.get_orientation(x[i, 4], x[i, 5]) + x[i, 3]
        g[i, 4], g[i, 5] = track.get_global_position(x[i, 4], x[i, 5])
    return g


def test_field_of_one_is_the_lone_car_loop(gpu, AB):
    """FieldRaces with one car per race = that car under cbf_solve_dev without obstacle slots + plant_step_wrap_dev, bit for bit."""
    import torch

    from crx import abi, montecarlo, torch_api

    track = _track("l_shape", 1.0)
    tab, L = track.point_and_tangent, track.lap_length
    n, N, steps = 8, 10, 40
    rng = np.random.default_rng(8)
    x0 = np.zeros((n, 6))
    x0[:, 0], x0[:, 4], x0[:, 5] = rng.uniform(0.2, 1.0, n), rng.uniform(0.0, L - 1.0, n), rng.uniform(-0.3, 0.3, n)
    x0[0, 4] = L - 0.8                                                   # one car crosses the line inside the 40 steps
    g0 = _globals(track, x0)
    vt = rng.uniform(0.6, 1.2, (n, 1))
    r = montecarlo.field_races(tab, L, track.width, AB[0], AB[1], x0, g0, 1, steps, vt=vt, N=N)
    assert r["xcurv"].shape == (steps + 1, n, 6) and (r["n_obs"] == 0).all() and np.isinf(r["min_clear"]).all() and r["laps"][0] == 1

    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), **f64).clone()   # noqa: E731
    desc = abi.cbf_desc(N, 0, AB[0], AB[1], alpha=0.8, margin=0.2, ey_max=track.width)
    plant = abi.plant_desc(tab.shape[0], L, timestep=0.1)
    ws = torch_api.CbfWorkspace(desc, n, dev)
    xt = np.zeros((n, 6))
    xt[:, 0] = vt[:, 0]
    xc, xg, xt, tabd = t(x0), t(g0), t(xt), t(tab)
    xcn, xgn = torch.empty_like(xc), torch.empty_like(xg)
    laps = torch.zeros(n, dtype=torch.int32, device=dev)
    none = (torch.zeros((n, 0, N + 1), **f64), torch.zeros((n, 0, N + 1), **f64), torch.zeros((n, 0), **f64), torch.zeros(n, dtype=torch.int32, device=dev))
    xs, us, st = [xc.clone()], [], []
    for _ in range(steps):
        torch_api.cbf_solve_dev(desc, xc, xt, *none, ws=ws)
        torch_api.plant_step_wrap_dev(plant, tabd, xg, xc, ws.U, 2 * N, xgn, xcn, laps)
        xg, xgn, xc, xcn = xgn, xg, xcn, xc
        xs.append(xc.clone()); us.append(ws.U[:, 0, :].clone()); st.append(ws.status.clone())
    lone = [torch.stack(a).cpu().numpy() for a in (xs, us, st)]
    assert np.array_equal(r["xcurv"], lone[0]) and np.array_equal(r["u"], lone[1]) and np.array_equal(r["status"], lone[2])
    assert np.array_equal(r["laps"], laps.cpu().numpy())


def test_field_closed_loop_retraces_the_mirror(gpu, AB):
    """Four identical races of three cars closing up on l_shape against the same field through the mirrored class surface: per step the
    states are snapshot into three mirror DynamicBicycleModel objects (F1), control.mpccbf(realtime_flag=True) plans every car on the
    snapshot, then forward_dynamics and the lap bookkeeping.  atol = 1e-3 on xcurv: what test_batched_closed_loop_races grants the same
    batched-versus-class-surface comparison."""
    from control import control
    from crx import hostprep, montecarlo
    from racing import offboard
    from utils import base

    track = _track("l_shape", 1.0)
    tab, L = track.point_and_tangent, track.lap_length
    R, C, N, steps = 4, 3, 10, 60
    vt = np.array([1.0, 0.8, 0.6])                                       # from back to front
    x1 = np.zeros((C, 6))
    x1[:, 0], x1[:, 4], x1[:, 5] = 0.5 * vt, 1.0 + 1.2 * np.arange(C), [0.15, -0.15, 0.15]
    g1 = _globals(track, x1)
    r = montecarlo.field_races(tab, L, track.width, AB[0], AB[1], np.tile(x1, (R, 1)), np.tile(g1, (R, 1)), C, steps, vt=np.tile(vt, (R, 1)), N=N)
    xb = r["xcurv"].reshape(steps + 1, R, C, 6)
    assert np.isfinite(xb).all()
    for k in ("xcurv", "u", "status", "n_obs"):                          # identical races, identical bits
        a = r[k].reshape((r[k].shape[0], R, C) + r[k].shape[2:])
        assert np.array_equal(a[:, 1:], np.repeat(a[:, :1], R - 1, axis=1)), k
    nb = r["n_obs"].reshape(steps, R, C)
    assert nb.max() == C - 1 and nb.min() == 0                           # the windows do fill as the cars close up

    def mirror(name, xc, xg):
        car = offboard.DynamicBicycleModel(name=name, param=base.CarParam(), system_param=base.SystemParam())
        car.set_track(track); car.set_timestep(0.1); car.set_zero_noise()
        car.set_state_curvilinear(np.array(xc, dtype=float)); car.set_state_global(np.array(xg, dtype=float))
        return car

    names = ["car%d" % c for c in range(C)]
    cars = {n_: mirror(n_, x1[c], g1[c]) for c, n_ in enumerate(names)}
    params = [base.MPCCBFRacingParam(matrix_A=AB[0], matrix_B=AB[1], vt=vt[c], num_horizon=N, alpha=0.8) for c in range(C)]
    log, n_host = [x1.copy()], []
    for _ in range(steps):
        snap = {n_: mirror(n_, cars[n_].xcurv, cars[n_].xglob) for n_ in names}
        counts = []
        for c, n_ in enumerate(names):
            xtarget = np.array([vt[c], 0, 0, 0, 0, 0.0]).reshape(6, 1)
            cars[n_].u = control.mpccbf(snap[n_].xcurv, xtarget, params[c], snap, n_, L, 0.0, 0.1, True, track, base.SystemParam())
            s0 = np.array([[snap[o].get_trajectory_nsteps(N + 1)[0][4, 0] for o in names if o != n_]])
            counts.append(int(hostprep.cbf_window(snap[n_].xcurv[None], s0, L)[0].sum()))
        for n_ in names:
            cars[n_].forward_dynamics(False)
            cars[n_].update_memory()
        log.append(np.array([cars[n_].xcurv for n_ in names]))
        n_host.append(counts)
    log, n_host = np.array(log), np.array(n_host)
    for race in (0, 3):
        assert np.array_equal(nb[:, race], n_host), race
        np.testing.assert_allclose(xb[:, race], log, rtol=0, atol=1e-3, err_msg="race %d" % race)


def test_field_sweep_bookkeeping(gpu, AB):
    """64 races of four different cars (own target speed, own controller model, own plant parameters), noise on, 150 steps: what the loop
    logs is finite and consistent.  No converged share and no contact count is asserted: the CBF rows are soft and this loop is new;
    tools/field_bench.py reports both."""
    from crx import abi, montecarlo, synth

    def family(n, s, seed):                                  # copies of the default model, perturbed as tests/test_gpu_cbf_models.py does
        g = np.random.default_rng(seed)
        return (np.array([AB[0] * (1 + s * g.standard_normal((6, 6))) for _ in range(n)]),
                np.array([AB[1] * (1 + s * g.standard_normal((6, 2))) for _ in range(n)]))

    track = _track("l_shape", 1.0)
    tab, L = track.point_and_tangent, track.lap_length
    R, C, N, steps = 64, 4, 10, 150
    rng = np.random.default_rng(64)
    x0 = np.zeros((R, C, 6))
    x0[..., 0] = 0.3
    x0[..., 4] = (rng.uniform(0.0, L, (R, 1)) + 1.5 * np.arange(C)[None, :]) % L
    x0[..., 5] = rng.choice([-0.3, -0.1, 0.1, 0.3], (R, C))
    g0 = _globals(track, x0.reshape(-1, 6))
    vt = rng.uniform(0.5, 1.0, (R, C))
    r = montecarlo.field_races(tab, L, track.width, AB[0], AB[1], x0, g0, C, steps, vt=vt, N=N, noise_seed=7, models=family(R * C, 1e-2, 9),
                               plant_params=synth.fleet_plant_params(R * C, 0.3, 10), log_every=1)
    for k in ("xcurv", "u", "min_clear"):
        assert np.isfinite(r[k]).all(), k
    assert r["xcurv"].shape == (steps + 1, R * C, 6) and r["status"].shape == (steps, R * C) and r["min_clear"].shape == (R * C,)
    documented = (abi.CRX_CONVERGED, abi.CRX_MAX_ITER, abi.CRX_INFEASIBLE, abi.CRX_RESTORED, abi.CRX_STALLED, abi.CRX_SINGULAR)
    assert np.isin(r["status"], documented).all(), np.unique(r["status"])
    assert (r["n_obs"] >= 0).all() and (r["n_obs"] <= C - 1).all() and (r["iters"] >= 0).all()
    # laps: whenever s falls by most of a lap from one logged state to the next, that car finished a lap -- and never otherwise
    crossings = (np.diff(r["xcurv"][:, :, 4], axis=0) < -0.5 * L).cumsum(axis=0)
    assert (np.diff(crossings, axis=0) >= 0).all() and np.array_equal(crossings[-1], r["laps"]) and r["laps"].min() >= 0
    # min_clear: the minimum of `clear` over the states the 150 steps started from
    host = np.min([fm.clear(x.reshape(R, C, 6), L) for x in r["xcurv"][:steps]], axis=0).reshape(-1)
    np.testing.assert_allclose(r["min_clear"], host, rtol=1e-12, atol=0)
    print("field sweep: converged share %.4f, contacts (min_clear < 1) %d of %d cars, laps %d .. %d" % (
        (r["status"] == 0).mean(), int((r["min_clear"] < 1).sum()), R * C, r["laps"].min(), r["laps"].max()))
