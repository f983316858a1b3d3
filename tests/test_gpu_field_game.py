"""Field games on the GPU: crx_field_traffic_dev against the numpy model (tests/field_game_model.py) and against crx_field_prep_dev, whose
roll-out it shares; its host twin; a non-finite car (G3) through the scene; montecarlo.grid_start against the bookkeeping launches it
stands for; and montecarlo.FieldGames -- against the lone learning car it must reduce to, with two cars that meet, and under RaceStats."""
import os

import numpy as np
import pytest

import conftest
import field_game_model as fgm
import race_stats_model as rsm
from test_gpu_field import _drawn_race, _fixed_race, _globals, _same_bits, _track

pytestmark = pytest.mark.gpu

# a block holds 256 // C whole races: a partial tail AND a second block at C = 7 (36 races per block) and C = 4 (64)
R_OF = {1: 3, 2: 3, 4: 65, 7: 37}


@pytest.fixture(scope="module")
def gpu():
    import crx

    return crx.init(0)


def _dev(a, dtype=None):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=torch.device("cuda", 0)).clone()


def draw(name, C, N, seed, R):
    """xcurv [R, C, 6] drawn as tests/test_gpu_field.py draws it -- races 0 .. 3 constructed (a car a lap ahead in s, a car that crosses the
    line inside the horizon, a bunch, a NaN car), the others drawn -- and the model's answer.  A race is drawn again while a visited s lies
    within 1e-9 of a segment end or of the lap length, or a roll-out comes near the singularity of the curvilinear frame
    (|1 - curv ey| < 0.4): field_model.predict says why 1e-12 ends there."""
    track = _track(name)
    tab, L = track.point_and_tangent, track.lap_length
    rng = np.random.default_rng(seed)
    race = lambda r: _fixed_race(rng, L, C, r) if r < 4 else _drawn_race(rng, L, C)   # noqa: E731
    x = np.array([race(r) for r in range(R)])
    for _ in range(200):
        m = fgm.traffic(tab, L, x, N)
        bad = (m["edge"].min(axis=1) < 1e-9) | (m["cond"].min(axis=1) < 0.4)
        if not bad.any():
            break
        for r in np.nonzero(bad)[0]:
            x[r] = race(r)
    else:
        raise AssertionError("the draw does not settle: %s" % np.nonzero(bad)[0])
    if C >= 2:
        assert (np.diff(m["pred_s_car"][1, 1]) < -0.5 * L).any()                 # a gathered row that jumps by -L (F3)
    if R >= 4:
        assert np.isnan(m["pred_s_car"][3, C - 1]).all()
    return tab, L, x, m


def _run(desc, tab, x):
    """One crx_field_traffic_dev launch; returns host arrays shaped as the model's."""
    import torch

    from crx import torch_api

    R, C = x.shape[:2]
    ws = torch_api.FieldTrafficWorkspace(desc, R, torch.device("cuda", 0))
    torch_api.field_traffic_dev(desc, _dev(tab), _dev(x.reshape(R * C, 6)), ws)
    torch.cuda.synchronize()
    V = C - 1
    return {k: getattr(ws, k).cpu().numpy()[:, :V] if k in ("veh_xcurv", "pred_s", "pred_ey") else getattr(ws, k).cpu().numpy()
            for k in ("pred_s_car", "pred_ey_car", "veh_xcurv", "pred_s", "pred_ey", "n_all")}


@pytest.mark.parametrize("C", [1, 2, 4, 7])
def test_field_traffic_matches_model(gpu, C):
    """pred_* within 1e-12 of the model (the bound of DESIGN section 14); veh_xcurv and every gathered row exact copies, as bits; and the
    per-car roll-out rows are, bit for bit, those of crx_field_prep_dev on the same inputs: one roll-out, two kernels."""
    import torch

    from crx import abi, torch_api

    R = R_OF[C]
    oth = fgm.fm.others(C)
    for name in ("l_shape", "m_shape"):
        for N in (10, 24):
            tag = (name, C, N)
            tab, L, x, m = draw(name, C, N, 1000 + 100 * C + N, R)
            desc = abi.field_desc(N, C, tab.shape[0], L)
            g = _run(desc, tab, x)
            assert g["n_all"].dtype == np.int32 and np.array_equal(g["n_all"], np.full(R * C, C - 1)), tag
            for k in ("pred_s_car", "pred_ey_car", "pred_s", "pred_ey"):
                assert g[k].shape == m[k].shape, tag + (k,)
                np.testing.assert_allclose(g[k], m[k], rtol=0, atol=1e-12, equal_nan=True, err_msg=str(tag + (k,)))
            assert _same_bits(g["veh_xcurv"], m["veh_xcurv"]), tag
            assert _same_bits(g["veh_xcurv"].reshape(R, C, C - 1, 6), x[:, oth]), tag
            assert _same_bits(g["pred_s"].reshape(R, C, C - 1, N + 1), g["pred_s_car"][:, oth]), tag
            assert _same_bits(g["pred_ey"].reshape(R, C, C - 1, N + 1), g["pred_ey_car"][:, oth]), tag
            fws = torch_api.FieldWorkspace(desc, R, torch.device("cuda", 0))
            torch_api.field_prep_dev(desc, _dev(tab), _dev(x.reshape(R * C, 6)), fws)
            torch.cuda.synchronize()
            assert _same_bits(fws.pred_s.cpu().numpy(), g["pred_s_car"]) and _same_bits(fws.pred_ey.cpu().numpy(), g["pred_ey_car"]), tag
            if R >= 4:      # the NaN car: its own rows, and its slot in the three other cars' arrays; nobody else's
                nan_car = np.isnan(g["pred_s_car"]).any(axis=-1)
                assert nan_car.sum() == 1 and nan_car[3, C - 1], tag
                assert np.isnan(g["pred_s"]).any(axis=-1).sum() == C - 1 and np.isnan(g["veh_xcurv"]).any(axis=-1).sum() == C - 1, tag


def test_field_traffic_host_twin(gpu):
    import crx
    from crx import abi

    C, N, R = 4, 10, R_OF[4]
    tab, L, x, m = draw("l_shape", C, N, 4242, R)
    desc = abi.field_desc(N, C, tab.shape[0], L)
    dev, host = _run(desc, tab, x), crx.field_traffic(desc, tab, x)
    assert sorted(host) == sorted(dev)
    for k in dev:
        assert _same_bits(np.asarray(host[k]), dev[k]), k
    one = gpu.field_traffic(abi.field_desc(N, 1, tab.shape[0], L), tab, x[:3, :1])
    assert one["veh_xcurv"].shape == (3, 0, 6) and (one["n_all"] == 0).all() and _same_bits(one["pred_s_car"], dev["pred_s_car"][:3, :1])


def test_nan_car_is_nobodys_vehicle_of_interest(gpu):
    """G3: four cars bunched inside each other's windows, car 2 with a non-finite state.  Through the scene, no other car's `order` holds its
    slot, the three others still see each other, and their rows are finite."""
    import torch

    from crx import abi, torch_api

    track = _track("l_shape")
    tab, L = track.point_and_tangent, track.lap_length
    C, N, nan = 4, 10, 2
    x = np.zeros((1, C, 6))
    x[0, :, 0], x[0, :, 4], x[0, :, 5] = 1.0, 3.0 + 0.12 * np.arange(C), [0.3, -0.3, 0.0, 0.1]   # all within one length of each other
    x[0, nan] = np.nan
    for e in range(C):
        for o in range(C):
            if o != e:
                assert fgm.of_interest(x[0, e], x[0, o], L) == (nan not in (e, o))
    dev = torch.device("cuda", 0)
    desc, scene = abi.field_desc(N, C, tab.shape[0], L), abi.scene_desc(N, C - 1, C - 1, L)
    ws = torch_api.FieldTrafficWorkspace(desc, 1, dev)
    xc = _dev(x.reshape(C, 6))
    torch_api.field_traffic_dev(desc, _dev(tab), xc, ws)
    sws = torch_api.planner_scene_dev(scene, xc, ws.n_all, ws.veh_xcurv, ws.pred_s, ws.pred_ey)
    torch.cuda.synchronize()
    n_veh, order, overflow = sws.n_veh.cpu().numpy(), sws.order.cpu().numpy(), sws.overflow.cpu().numpy()
    ps, pe = ws.pred_s_car.cpu().numpy()[0], ws.pred_ey_car.cpu().numpy()[0]
    assert np.isnan(ps[nan]).all() and np.isnan(pe[nan]).all()
    assert np.isfinite(np.delete(ps, nan, axis=0)).all() and np.isfinite(np.delete(pe, nan, axis=0)).all()
    assert n_veh[nan] == 0 and (overflow == 0).all()
    for e in range(C):
        if e == nan:
            continue
        slot = nan - (nan > e)                                               # where the NaN car sits in ego e's arrays
        assert n_veh[e] == C - 2 and slot not in order[e, :n_veh[e]].tolist(), (e, order[e])
        assert np.isfinite(sws.obs_s.cpu().numpy()[e, :n_veh[e]]).all()


# ---- grid_start and the loop ---------------------------------------------------------------------------------------------------------
def _nominal(Bn):
    """The nominal car's safe set (tests/golden/racing_game.npz) tiled for Bn cars, as the inputs of LmpcLaps / grid_start by name."""
    import helpers

    g = np.load(os.path.join(conftest.GOLDEN, "racing_game.npz"), allow_pickle=False)
    track = _track("l_shape", 1.0)
    d, ss, us, qf, time_ss, lin_points, lin_input = helpers.lmpc_lap_setup(g, track)
    tile = lambda a: np.tile(a[None], (Bn,) + (1,) * a.ndim)   # noqa: E731
    inp = dict(ss_xcurv=tile(ss), u_ss=tile(us), qfun=tile(qf), time_ss=tile(time_ss), it=np.full(Bn, 2, dtype=np.int32),
               xcurv0=np.tile(g["lmpc/x"][0], (Bn, 1)), xglob0=np.tile(g["lap1/xglob"][-1], (Bn, 1)), lin_points=tile(lin_points),
               lin_input=tile(lin_input))
    return track, d, inp


def test_grid_start_is_what_the_kernels_do(gpu):
    """The definition: from ss[b,j,0], k[b] steps of game_commit_dev (the plan X[m] = ss[b,j,i+m], U[m] = us[b,j,i+m]), lmpc_addpoint_dev and
    game_log_dev (the new state ss[b,j,i+1]) -- the launches of LmpcLaps.step around its solver and plant -- leave grid_start's arrays, bit
    for bit.  All cars take every launch; car b's arrays are read when it has taken k[b] of them."""
    import torch

    from crx import montecarlo, torch_api

    Bn, k = 4, np.array([0, 1, 5, 9])
    track, d, inp = _nominal(Bn)
    N, P, L = d.N, d.n_points, track.lap_length
    dev = torch.device("cuda", 0)
    t = {name: _dev(a) for name, a in inp.items()}
    got = montecarlo.grid_start(t, k, track)
    for name in ("ss_xcurv", "xcurv0", "log_x"):
        assert got[name].is_cuda and got[name].dtype == torch.float64, name
    j = 1
    assert (inp["it"] == j + 1).all() and k.max() <= inp["time_ss"][0, j] - N - 1
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    ss, us = t["ss_xcurv"].clone(), t["u_ss"].clone()
    lap_x, lap_u = ss[:, j].clone(), us[:, j].clone()
    x = torch.where(_dev(k > 0)[:, None], lap_x[:, 0], t["xcurv0"]).contiguous()      # a car that does not move stays where it was handed over
    step_no, addpoint_step, n_log = torch.zeros(Bn, **i32), torch.zeros(Bn, **i32), torch.ones(Bn, **i32)
    u, u_old, u_prev = torch.zeros((Bn, 2), **f64), torch.zeros((Bn, 2), **f64), torch.zeros((Bn, 2), **f64)
    lin_points, lin_input = t["lin_points"].clone(), t["lin_input"].clone()
    log_x, log_u = torch.zeros((Bn, P, 6), **f64), torch.zeros((Bn, P, 2), **f64)
    log_x[:, 0] = x
    laps, laps_prev, crossed = torch.zeros(Bn, **i32), torch.zeros(Bn, **i32), torch.zeros(Bn, **i32)
    state = dict(ss_xcurv=ss, u_ss=us, xcurv0=x, lin_points=lin_points, lin_input=lin_input, step_no=step_no, n_log=n_log, log_x=log_x,
                 log_u=log_u, u_old=u_old, u_prev=u_prev)
    taken = {}
    for i in range(int(k.max()) + 1):
        for b in np.nonzero(k == i)[0]:
            taken[b] = {name: (x if name == "xcurv0" else a)[b].clone() for name, a in state.items()}
        if i == k.max():
            break
        X, U = lap_x[:, i:i + N + 1].contiguous(), lap_u[:, i:i + N].contiguous()
        torch_api.game_commit_dev(N, N, None, None, X, U, None, u, u_old, u_prev, lin_points, lin_input, step_no, addpoint_step, None)
        torch_api.lmpc_addpoint_dev(d, ss, us, t["time_ss"], t["it"], addpoint_step, x, u, 2)
        x = lap_x[:, i + 1].contiguous()
        torch_api.game_log_dev(L, x, u, laps, laps_prev, log_x, log_u, n_log, crossed)
    torch.cuda.synchronize()
    assert sorted(taken) == list(range(Bn))
    for b in range(Bn):
        for name, a in taken[b].items():
            assert got[name].dtype == a.dtype and torch.equal(got[name][b], a), (b, name)
            if a.dtype == torch.float64:
                assert np.array_equal(got[name][b].cpu().numpy().view(np.uint64), a.cpu().numpy().view(np.uint64)), (b, name)
    for name in ("qfun", "time_ss", "it"):
        assert torch.equal(got[name], t[name]), name
    # the global pose: the arithmetic of tests/test_gpu_field.py::_globals on the moved cars, the hand-over pose on the other
    xg = got["xglob0"].cpu().numpy()
    assert _same_bits(xg[1:], _globals(track, got["xcurv0"].cpu().numpy()[1:])) and _same_bits(xg[0], inp["xglob0"][0])
    # the cars stand apart
    assert (np.diff(got["xcurv0"].cpu().numpy()[:, 4]) > 0).all()


def test_field_of_one_is_the_lone_learning_car(gpu, AB):
    """FieldGames with one car per race and k = 0 against LmpcLaps on the same inputs, zero noise, 12 steps: no vehicle, so every step takes
    the learning-MPC branch, and xcurv, u and the safe set agree in bits."""
    import torch

    import scenarios
    from crx import montecarlo

    Bn, steps = 3, 12
    track, d, inp = _nominal(Bn)
    inp["xcurv0"][:, 0] += [0.0, 0.01, -0.02]
    inp["xglob0"][:, 0] = inp["xcurv0"][:, 0]
    tab, L = track.point_and_tangent, track.lap_length
    opt = scenarios.table("optimal_traj", "xcurv_l_shape")
    game = montecarlo.FieldGames(tab, L, track.width, AB[0], AB[1], opt, 1, **montecarlo.grid_start(inp, np.zeros(Bn, dtype=np.int32), track))
    lone = montecarlo.LmpcLaps(tab, L, track.width, **inp)
    for s in range(steps):
        game.step(); lone.step()
        assert int(game.m_ot.sum()) == 0 and int(game.m_lm.sum()) == Bn, s
        assert torch.equal(game.lm.xc, lone.xc) and torch.equal(game.u, lone.u), s
    for name in ("ss", "us", "qf", "time_ss", "it", "xg", "u_old", "step_no", "log_x", "log_u", "n_log", "laps"):
        assert torch.equal(getattr(game.lm, name), getattr(lone, name)), name
    assert (game.fws.n_all == 0).all() and int(game.overflow_seen.sum()) == 0


K_REAR = 20


def _meeting(R):
    """R copies of a race of two nominal cars about 1 m apart on their mpc-lti lap: car 0 K_REAR steps in, car 1 at the first step that is
    1 m further.  Checked on the CPU before anything is launched: the rear car has the front car inside its window (4.5 lengths + half the
    speed difference ahead), the front car does not have the rear car in its own (one length behind)."""
    from crx import montecarlo

    track, d, inp = _nominal(2 * R)
    s = inp["ss_xcurv"][0, 1, :, 4]
    k_front = int(np.nonzero(s[:inp["time_ss"][0, 1]] >= s[K_REAR] + 1.0)[0][0])
    k = np.tile([K_REAR, k_front], R)
    grid = montecarlo.grid_start(inp, k, track)
    x = grid["xcurv0"].numpy().reshape(R, 2, 6)
    assert 1.0 <= x[0, 1, 4] - x[0, 0, 4] <= 1.2
    assert fgm.of_interest(x[0, 0], x[0, 1], track.lap_length) and not fgm.of_interest(x[0, 1], x[0, 0], track.lap_length)
    m = fgm.traffic(track.point_and_tangent, track.lap_length, x, 10)
    assert np.isfinite(m["pred_s"]).all() and m["cond"].min() > 0.4
    return track, grid


def _field_game(AB, track, grid, **kw):
    import scenarios
    from crx import montecarlo

    opt = scenarios.table("optimal_traj", "xcurv_l_shape")
    return montecarlo.FieldGames(track.point_and_tangent, track.lap_length, track.width, AB[0], AB[1], opt, 2, **grid, **kw)


@pytest.fixture(scope="module")
def met(gpu, AB):
    """Two identical races of two cars that meet, 40 steps, zero noise, stepped through RaceStats: the logs of both tests below."""
    import torch

    from crx import montecarlo

    R, steps = 2, 40
    track, grid = _meeting(R)
    game = _field_game(AB, track, grid)
    stats = montecarlo.RaceStats(game)
    log = []
    snap = lambda: log.append((game.lm.xc.clone(), game.lm.laps.clone(), game.m_ot.clone(), game.u.clone(), game.old_flag.clone()))   # noqa: E731
    stats.update(); snap()
    for _ in range(steps):
        stats.step(); snap()
    torch.cuda.synchronize()
    host = [tuple(a.cpu().numpy() for a in row) for row in log]
    return dict(track=track, R=R, steps=steps, stats=stats, log=host, game=game)


def test_cars_meet(gpu, AB, met):
    R, steps, log = met["R"], met["steps"], met["log"]
    x = np.array([row[0] for row in log])                                    # [steps+1, R*2, 6]
    m_ot = np.array([row[2] for row in log[1:]])                             # the branch of step k is log[k + 1]'s mask
    u = np.array([row[3] for row in log[1:]])
    assert np.isfinite(x).all() and np.isfinite(u).all()
    assert m_ot[0, 0] == 1                                                   # the rear car plans around the front car from the first step
    assert (m_ot == 0).any() and (m_ot == 1).any()                           # both branches ran
    for a in (x, m_ot, u):
        a = a.reshape((a.shape[0], R, 2) + a.shape[2:])
        assert np.array_equal(a[:, 1], a[:, 0])                              # the two races carry the same bits
    # race 0 equals the same race run alone
    track, grid = _meeting(1)
    out = _run_alone(AB, track, grid, steps)
    assert np.array_equal(out["xcurv"], x[:, :2]) and np.array_equal(out["u"], u[:, :2]) and np.array_equal(out["overtake"], m_ot[:, :2] != 0)


def _run_alone(AB, track, grid, steps):
    import scenarios
    from crx import montecarlo

    opt = scenarios.table("optimal_traj", "xcurv_l_shape")
    inputs = {n: grid[n] for n in ("ss_xcurv", "u_ss", "qfun", "time_ss", "it", "xcurv0", "xglob0", "lin_points", "lin_input")}
    fields = {n: a for n, a in grid.items() if n not in inputs}
    return montecarlo.field_games(track.point_and_tangent, track.lap_length, track.width, AB[0], AB[1], opt, 2, *inputs.values(), steps, **fields)


def test_race_stats_of_a_field_game(gpu, met):
    """RaceStats attaches to FieldGames with no statistics code of its own: the counters equal tests/race_stats_model.py replayed on the
    logged states in field mode, integers exactly."""
    from test_gpu_race_stats import F64_FIELDS, INT_FIELDS

    track, R, steps, stats, log = met["track"], met["R"], met["steps"], met["stats"], met["log"]
    assert stats.n_updates == steps + 1 and (stats.desc.n_cars, stats.desc.n_opp_max, stats.desc.l_sum, stats.desc.w_sum) == (2, 1, 0.4, 0.2)
    st = rsm.reset(2 * R, 1, np.zeros(2 * R, dtype=np.int32))
    for k, (xc, laps, m_ot, _, _) in enumerate(log):
        rsm.sample(st, k, xc, laps, track.lap_length, track.width, n_cars=2, flag=m_ot)
    got = stats.per_car()
    for name in INT_FIELDS:
        assert np.array_equal(got[name], st[name]), (name, got[name], st[name])
    for name in F64_FIELDS:
        assert np.array_equal(got[name], st[name], equal_nan=True), (name, got[name], st[name])
    assert (got["n_samples"] == steps + 1).all()
    rec = stats.summary()
    assert rec == rsm.summary(st)[0] and rec["cars"] == 2 * R
