"""The overtake path planner on the device (crx_path_prep, crx_path_plan, GameLaps(planner="path"): include/crx.h P1-P8) against the
host mirror planning/overtake_path_planner.py, on the draws of tests/path_plan_cases.py (tests/test_path_plan_cpu.py probes them: on
draws a-d every flag and every side-row pattern is unambiguous, so every scenario is compared, none excluded).

Tolerances are the project's own: 1e-13 closed-form device prep against the host (test_device_prep), 1e-7 on E and rtol 1e-9 on cost
(test_path_planner_qps), 5e-6 on the target against the reference's recording (test_overtake_path_step)."""
import numpy as np
import pytest
import torch

import conftest
import path_plan_cases as cases

pytestmark = pytest.mark.gpu
SENT = 7.0   # what the arrays a skipped scenario must leave alone are filled with


@pytest.fixture(scope="module")
def gpu():
    import crx

    return crx.init()


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _dev_inputs(d, n_all=None, x_raw=None, x_wrapped=None, veh=None):
    """Scene on the device -> the tensors path_prep_dev / path_plan_dev take, in their order."""
    from crx import torch_api

    sd = cases.descs(d)[0]
    xw = _t(d["x_wrapped"] if x_wrapped is None else x_wrapped)
    xr = _t(d["x_raw"] if x_raw is None else x_raw)
    vh = _t(d["veh"] if veh is None else veh)
    sw = torch_api.planner_scene_dev(sd, xw, _t(d["n_all"] if n_all is None else n_all, torch.int32), _t(d["veh"]), _t(d["pred_s"]),
                                     _t(d["pred_ey"]))
    return sw, [xw, xr, sw.n_veh, sw.order, vh, sw.max_dv, sw.obs_ey, _t(d["opt_s"]), _t(d["opt_ey"])]


def _ws(d, S=None):
    from crx import torch_api

    ws = torch_api.PathPlanWorkspace(cases.descs(d)[1], d["S"] if S is None else S, "cuda")
    for a in (ws.opt, ws.bez, ws.lb, ws.ub, ws.e0, ws.eN, ws.span, ws.E, ws.kkt, ws.target):
        a.fill_(SENT)
    return ws


OUT = ("opt", "bez", "lb", "ub", "e0", "eN", "span", "qp_active", "E", "cost", "status", "kkt", "iters", "flag", "target", "plan_status")


def _host(ws, names=OUT):
    torch.cuda.synchronize()
    return {k: getattr(ws, k).cpu().numpy().copy() for k in names}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8 if a.dtype.itemsize == 1 else {4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _check_prep(d, sc, m, got, untouched):
    S, N1, V, tw = d["S"], d["N"] + 1, d["V"], d["tw"]
    R = V + 1
    g = {**{k: got[k].reshape(S, R, N1) for k in ("opt", "bez", "lb", "ub")}, **{k: got[k].reshape(S, R) for k in ("e0", "eN")}}
    worst = 0.0
    for s in range(S):
        nv = int(sc["n_veh"][s])
        if nv == 0:                                          # not planned: contents kept
            for k in g:
                assert untouched(g[k][s]), (s, k)
            assert untouched(got["span"][s:s + 1]), s
            continue
        if m["raised"][s]:                                   # the mirror raised (P2): the device answers NaN
            assert all(np.isnan(g[k][s]).all() for k in g) and np.isnan(got["span"][s]), s
            continue
        for k in g:
            err = np.abs(g[k][s, :nv + 1] - m[k][s, :nv + 1]).max()
            worst = max(worst, err)
            assert err <= 1e-13, (s, k, err)
            for r in range(nv + 1, R):                       # regions beyond the vehicles repeat the last one
                np.testing.assert_array_equal(g[k][s, r], g[k][s, nv])
        assert abs(got["span"][s] - m["span"][s]) <= 1e-13, s
        side_dev = (g["lb"][s, :nv + 1] != -tw) | (g["ub"][s, :nv + 1] != tw)
        side_ref = (m["lb"][s, :nv + 1] != -tw) | (m["ub"][s, :nv + 1] != tw)
        np.testing.assert_array_equal(side_dev, side_ref, err_msg="scenario %d" % s)
    return worst


@pytest.mark.parametrize("name", list(cases.DRAWS))
def test_prep_against_host_mirror(gpu, orc, name):
    """Test 1: opt, bez, lb, ub, e0, eN, span within 1e-13 of the mirror's path_qp_inputs, identical side-row pattern, through the
    device entry (behind the scene kernel) and the host-pointer entry.  Draw e: scenarios without vehicles keep their contents."""
    from crx import torch_api

    d, sc, m = cases.draw(name), cases.scene(name), cases.mirror_prep(name)
    sw, ins = _dev_inputs(d)
    ws = torch_api.path_prep_dev(cases.descs(d)[1], *ins, ws=_ws(d))
    got = _host(ws, OUT[:7])
    np.testing.assert_array_equal(sw.n_veh.cpu().numpy(), sc["n_veh"])          # the device scene = the oracle's
    np.testing.assert_array_equal(sw.order.cpu().numpy(), sc["order"])
    np.testing.assert_array_equal(sw.obs_ey.cpu().numpy(), sc["obs_ey"])
    worst = _check_prep(d, sc, m, got, lambda a: (a == SENT).all())
    print("draw %s: largest prep deviation from the mirror %.3g" % (name, worst))
    if name == "e":
        assert (sc["n_veh"] == 0).sum() >= 4 and len(set(sc["n_veh"])) == 4
        front, rear = cases.hostprep.wrap_above(d["veh"][0, 0, 4] + 1.8, d["L"]), cases.hostprep.wrap_above(d["veh"][0, 0, 4] - 1.8, d["L"])
        assert rear > front                                                        # the crafted wrapped rear range is in the draw
    h = gpu.path_prep(cases.descs(d)[1], d["x_wrapped"], d["x_raw"], sc["n_veh"], sc["order"], d["veh"], sc["max_dv"], sc["obs_ey"],
                      d["opt_s"], d["opt_ey"])
    _check_prep(d, sc, m, h, lambda a: np.isnan(a).all())
    planned = np.repeat(sc["n_veh"] > 0, d["V"] + 1)
    for k in OUT[:6]:                                                              # one kernel behind both entries: same bits
        np.testing.assert_array_equal(_bits(h[k][planned]), _bits(got[k][planned]))


@pytest.mark.parametrize("name", list(cases.DRAWS))
def test_fused_step_against_composition(gpu, name):
    """Test 2: crx_path_plan_dev against crx_path_prep_dev -> crx_path_solve_dev (every QP, unmasked) -> P7, P8 in numpy."""
    from crx import abi, torch_api

    d, sc = cases.draw(name), cases.scene(name)
    S, N, R = d["S"], d["N"], d["V"] + 1
    _, pd, qd = cases.descs(d)
    _, ins = _dev_inputs(d)
    ref = _host(torch_api.path_solve_dev(qd, torch_api.path_prep_dev(pd, *ins, ws=_ws(d))), OUT[:7] + ("E", "cost", "status", "kkt", "iters"))
    planned = sc["n_veh"] > 0
    pq = np.repeat(planned, R)
    cost_ref = np.where(pq, ref["cost"], np.inf).reshape(S, R)
    flag_ref, target_ref, raised = cases.host_select(d, sc, ref["span"], ref["E"].reshape(S, R, N + 1), cost_ref)
    got = _host(torch_api.path_plan_dev(pd, qd, *ins, _t(d["opt_vx"]), ws=_ws(d)))
    # regions
    np.testing.assert_array_equal(got["status"][pq], ref["status"][pq])
    assert (got["status"][~pq] == abi.CRX_SKIPPED).all() and np.isinf(got["cost"][~pq]).all() and (got["E"][~pq] == SENT).all()
    np.testing.assert_array_equal(got["qp_active"], pq.astype(np.int32))
    ok = pq & (ref["status"] == 0)
    assert ok.sum() >= S // 4
    np.testing.assert_allclose(got["E"][ok], ref["E"][ok], rtol=0, atol=1e-7)
    np.testing.assert_allclose(got["cost"][ok], ref["cost"][ok], rtol=1e-9)
    assert np.isinf(got["cost"][pq & ~ok]).all()
    # scenarios
    good = planned & ~raised
    np.testing.assert_array_equal(got["flag"], flag_ref)
    assert (got["plan_status"][good] == 0).all() and (got["plan_status"][~planned] == abi.CRX_SKIPPED).all()
    assert (got["plan_status"][planned & raised] == abi.CRX_OUT_OF_DOMAIN).all() and np.isnan(got["target"][planned & raised]).all()
    assert (got["target"][~planned] == SENT).all()
    T, Tr = got["target"][good], target_ref[good]
    np.testing.assert_allclose(T[:, :, 4], Tr[:, :, 4], rtol=0, atol=1e-13)
    np.testing.assert_allclose(T[:, :, 0], Tr[:, :, 0], rtol=0, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(T[:, :, 5], Tr[:, :, 5], rtol=0, atol=1e-7)
    np.testing.assert_array_equal(_bits(T[:, 0, :]), _bits(d["x_wrapped"][good]))               # row 0 = the wrapped state, exactly
    assert (T[:, N, 0] == 0.0).all() and (T[:, 1:, 1:4] == 0.0).all()
    if name == "a":                                                                              # P7: all regions failed -> flag 0, its fall-back E
        allinf = np.isinf(cost_ref).all(axis=1)
        assert allinf.sum() >= 100 and (got["flag"][allinf] == 0).all()
        Eg, Er = got["E"].reshape(S, R, N + 1), ref["E"].reshape(S, R, N + 1)
        np.testing.assert_array_equal(_bits(Eg[allinf, 0]), _bits(Er[allinf, 0]))
        np.testing.assert_array_equal(_bits(got["target"][allinf][:, 1:, 5]), _bits(Er[allinf, 0][:, 1:]))
    if name == "b":
        assert (np.bincount(got["flag"], minlength=R) > 0).all()
    # the host-pointer entry: the same three kernels behind the staging
    h = gpu.path_plan(pd, qd, d["x_wrapped"], d["x_raw"], sc["n_veh"], sc["order"], d["veh"], sc["max_dv"], sc["obs_ey"], d["opt_s"], d["opt_ey"],
                      d["opt_vx"], target=np.full((S, N + 1, 6), SENT))
    for k in ("cost", "status", "iters", "flag", "target", "plan_status"):
        np.testing.assert_array_equal(_bits(h[k]), _bits(got[k]), err_msg=k)
    np.testing.assert_array_equal(_bits(h["E"][pq]), _bits(got["E"][pq]))
    assert np.isnan(h["E"][~pq]).all()


def test_goldens(gpu, golden_path):
    """Test 3: the reference's recorded scenarios through scene -> fused step: its direction_flag, its target trajectory."""
    from crx import abi, torch_api

    opt = np.genfromtxt(conftest.ROOT + "/data/optimal_traj/xcurv_l_shape.csv", delimiter=",")
    checked = compared = 0
    for name in golden_path.names:
        g = golden_path.case(name)
        if not bool(g["overtake_flag"]):
            continue
        N, VA, L = int(g["N"]), len(g["veh_names"]), float(g["lap_length"])
        V = min(VA, abi.CRX_MAX_VEH)
        sd = abi.scene_desc(N, VA, V, L)
        pd, qd = abi.pathprep_desc(N, V, VA, opt.shape[0], float(g["width"]), L), abi.path_desc(N, float(g["alpha"]))
        x, veh = _t(g["x"][None]), _t(g["veh_xcurv"][None])
        pred_ey = _t(np.repeat(g["cars"][None, :, 2, None], N + 1, axis=2))       # scripted cars: constant offsets
        sw = torch_api.planner_scene_dev(sd, x, _t([VA], torch.int32), veh, torch.zeros_like(pred_ey), pred_ey)
        ws = torch_api.path_plan_dev(pd, qd, x, x, sw.n_veh, sw.order, veh, sw.max_dv, sw.obs_ey, _t(opt[:, 4]), _t(opt[:, 5]), _t(opt[:, 0]))
        r = _host(ws, ("flag", "target", "plan_status", "status"))
        names = [str(n) for n in g["veh_names"]]
        assert [names[i] for i in sw.order.cpu().numpy()[0, :int(sw.n_veh[0])]] == [str(n) for n in g["sorted_vehicles"]], name
        assert r["plan_status"][0] == 0 and r["flag"][0] == int(g["direction_flag"]), name
        if g["region_success"][r["flag"][0]]:
            np.testing.assert_allclose(r["target"][0], g["traj_xcurv"], rtol=0, atol=5e-6, err_msg=name)
            compared += 1
        checked += 1
    assert checked >= 6 and compared >= 4


def _plan(d, ins, opt_vx, S, active=None):
    from crx import torch_api

    _, pd, qd = cases.descs(d)
    return _host(torch_api.path_plan_dev(pd, qd, *ins, opt_vx, ws=_ws(d, S), active=active))


PER_REGION = ("opt", "bez", "lb", "ub", "e0", "eN", "qp_active", "E", "cost", "status", "kkt", "iters")
PER_SCEN = ("span", "flag", "target", "plan_status")


def _rows(r, idx, R):
    """The outputs of scenarios idx, as one dict of arrays (regions expanded)."""
    q = (np.asarray(idx)[:, None] * R + np.arange(R)[None, :]).reshape(-1)
    return {**{k: r[k][q] for k in PER_REGION}, **{k: r[k][idx] for k in PER_SCEN}}


def _same_bits(a, b, what):
    for k in a:
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg="%s: %s" % (what, k))


def _check_skipped(r, idx, R, what):
    from crx import abi

    got = _rows(r, idx, R)
    assert (got["status"] == abi.CRX_SKIPPED).all() and np.isinf(got["cost"]).all() and (got["iters"] == 0).all(), what
    assert (got["flag"] == -1).all() and (got["plan_status"] == abi.CRX_SKIPPED).all() and (got["qp_active"] == 0).all(), what
    assert (got["target"] == SENT).all() and (got["E"] == SENT).all(), what


def test_locality(gpu):
    """Test 4: a scenario's outputs depend on that scenario alone -- draw b rolled by 5 scenarios, scenarios [3:9] alone, every third
    scenario masked: every unmasked scenario keeps its bits; masked ones and those without vehicles are skipped as documented."""
    d = cases.draw("b")
    S, R = d["S"], d["V"] + 1
    n_all = d["n_all"].copy()
    n_all[[4, 7, 100]] = 0                                   # three scenarios without vehicles
    _, ins = _dev_inputs(d, n_all=n_all)
    opt_vx = _t(d["opt_vx"])
    base = _plan(d, ins, opt_vx, S)
    empty, full = np.array([4, 7, 100]), np.setdiff1d(np.arange(S), [4, 7, 100])
    _check_skipped(base, empty, R, "no vehicles")
    assert (base["plan_status"][full] == 0).all() and (base["flag"][full] >= 0).all()
    rolled = _plan(d, [torch.roll(a, 5, 0).contiguous() for a in ins[:7]] + ins[7:], opt_vx, S)
    _same_bits(_rows(rolled, (np.arange(S) + 5) % S, R), _rows(base, np.arange(S), R), "rolled by 5")
    part = _plan(d, [a[3:9].contiguous() for a in ins[:7]] + ins[7:], opt_vx, 6)
    _same_bits(_rows(part, np.arange(6), R), _rows(base, np.arange(3, 9), R), "scenarios [3:9]")
    active = np.ones(S, dtype=np.int32)
    active[::3] = 0
    masked = _plan(d, ins, opt_vx, S, active=_t(active))
    on = np.nonzero(active)[0]
    _same_bits(_rows(masked, on, R), _rows(base, on, R), "every third masked")
    _check_skipped(masked, np.nonzero(active == 0)[0], R, "masked")


def test_non_finite_input(gpu):
    """Test 5: a NaN in one scenario's raw state, an inf in one car's state of another: ordinary input validation -- the launch
    succeeds, those two scenarios end with a non-zero status and no finite target, every other scenario keeps its bits."""
    from crx import abi

    d, sc = cases.draw("c"), cases.scene("c")
    S, R = d["S"], d["V"] + 1
    _, ins = _dev_inputs(d)
    opt_vx = _t(d["opt_vx"])
    base = _plan(d, ins, opt_vx, S)
    x_raw, veh = d["x_raw"].copy(), d["veh"].copy()
    x_raw[11, 4] = np.nan
    veh[50, sc["order"][50, 1], 4] = np.inf
    _, bad_ins = _dev_inputs(d, x_raw=x_raw, veh=veh)         # (the scene saw the clean states: same vehicles, same order)
    got = _plan(d, bad_ins, opt_vx, S)
    hit, rest = np.array([11, 50]), np.setdiff1d(np.arange(S), [11, 50])
    assert (got["plan_status"][hit] == abi.CRX_OUT_OF_DOMAIN).all() and (got["flag"][hit] == -1).all()
    assert not np.isfinite(got["target"][hit]).any()
    q = (hit[:, None] * R + np.arange(R)[None, :]).reshape(-1)
    assert (got["status"][q] == abi.CRX_INFEASIBLE).all() and np.isinf(got["cost"][q]).all() and (got["iters"][q] == 0).all()
    _same_bits(_rows(got, rest, R), _rows(base, rest, R), "scenarios beside the non-finite ones")


def _game(golden_racing_game, AB, Bn, **kw):
    import helpers
    import scenarios
    from crx import montecarlo

    A, B = AB
    g = golden_racing_game
    track = scenarios.make_track("l_shape", 1.0)
    opt = scenarios.table("optimal_traj", "xcurv_l_shape")
    _, ss, us, qf, time_ss, lin_points, lin_input = helpers.lmpc_lap_setup(g, track)
    x0 = np.tile(g["lmpc/x"][0], (Bn, 1)); xg0 = np.tile(g["lap1/xglob"][-1], (Bn, 1))
    rng = np.random.default_rng(61)
    s0 = x0[:, 4, None] + np.array([1.0, 2.2])[None, :]                          # two scripted cars 1.0 and 2.2 m ahead
    v = rng.uniform(0.3, 0.6, (Bn, 2))
    ey = rng.choice([-0.6, -0.3, 0.0, 0.3, 0.6], (Bn, 2))
    tile = lambda a: np.tile(a[None], (Bn,) + (1,) * a.ndim)   # noqa: E731
    r = montecarlo.GameLaps(track.point_and_tangent, track.lap_length, track.width, A, B, opt, tile(ss), tile(us), tile(qf), tile(time_ss),
                            np.full(Bn, 2, dtype=np.int32), x0, xg0, tile(lin_points), tile(lin_input), s0, v, ey, noise_seed=5, **kw)
    return r, track, opt, (s0, v, ey), x0


def _run(r, steps):
    xs, fl, ot = [r.lm.xc.clone()], [], []
    for _ in range(steps):
        r.step()
        xs.append(r.lm.xc.clone()); fl.append(r.old_flag.clone()); ot.append(r.overtake.clone())
    torch.cuda.synchronize()
    return torch.stack(xs).cpu().numpy(), torch.stack(fl).cpu().numpy(), torch.stack(ot).cpu().numpy().astype(bool)


def test_game_laps_path_planner(gpu, AB, golden_racing_game, capsys):
    """Test 6: GameLaps(planner="path"), 16 races behind two scripted cars, 30 steps: finite, on the track, a flag in 0..V wherever a
    race is in the overtake branch; at step 0 flag and target of three races are OvertakePathPlanner.get_local_path's on the same state
    (mirror classes); planner="traj" retraces the loop built without the argument bit for bit."""
    import sympy as sp

    from planning import overtake_path_planner
    from racing import offboard
    from utils import base

    Bn, steps = 16, 30
    r, track, opt, (s0, v, ey), x0 = _game(golden_racing_game, AB, Bn, planner="path")
    r.step()
    torch.cuda.synchronize()
    flag0, target0, ps0 = r.ppws.flag.cpu().numpy().copy(), r.ppws.target.cpu().numpy().copy(), r.ppws.plan_status.cpu().numpy().copy()
    nveh0 = r.sws.n_veh.cpu().numpy().copy()
    assert r.overtake.cpu().numpy().all() and (ps0 == 0).all() and (nveh0 >= 1).all()
    t = sp.symbols("t")
    for b in (0, 5, 11):
        par = base.RacingGameParam(timestep=0.1, num_horizon_planner=10, num_horizon_ctrl=10, alpha=0.98)
        ego = offboard.DynamicBicycleModel(name="ego", param=base.CarParam(), system_param=base.SystemParam())
        ego.set_state_curvilinear(x0[b].copy()); ego.set_state_global(np.zeros(6))
        ego.set_track(track); ego.set_timestep(0.1)
        vehicles = {"ego": ego}
        for c in range(2):
            car = offboard.NoDynamicsModel(name="car%d" % (c + 1), param=base.CarParam())
            car.set_track(track); car.set_timestep(0.1)
            car.set_state_curvilinear_func(t, float(v[b, c]) * t + float(s0[b, c]), float(ey[b, c]) + 0.0 * t)
            vehicles[car.name] = car
        pl = overtake_path_planner.OvertakePathPlanner(par)
        pl.vehicles, pl.agent_name, pl.track, pl.opti_traj_xcurv = vehicles, "ego", track, opt
        hit, interest = pl.get_overtake_flag(x0[b].copy())
        assert hit and len(interest) == nveh0[b]
        traj, _, dflag = pl.get_local_path(x0[b].copy(), 0.0, interest)[:3]
        assert flag0[b] == dflag, b
        np.testing.assert_allclose(target0[b], traj, rtol=0, atol=5e-6, err_msg="race %d" % b)
    capsys.readouterr()
    x, fl, ot = _run(r, steps - 1)
    assert np.isfinite(x).all() and np.abs(x[:, :, 5]).max() <= track.width
    assert ot.sum() >= Bn and ((fl[ot] >= 0) & (fl[ot] <= r.V)).all() and (fl[~ot] == -1).all()
    # the default is today's loop
    ra = _game(golden_racing_game, AB, Bn, planner="traj")[0]
    rb = _game(golden_racing_game, AB, Bn)[0]
    xa, fa, oa = _run(ra, steps)
    xb, fb, ob = _run(rb, steps)
    np.testing.assert_array_equal(_bits(xa), _bits(xb))
    np.testing.assert_array_equal(fa, fb)
    np.testing.assert_array_equal(oa, ob)
