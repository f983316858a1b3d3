"""Field games without a GPU: the numpy model of crx_field_traffic (tests/field_game_model.py) against the rows the reference's own driven
model predicted (tests/golden/field_pred.npz); the launch sequence of montecarlo.FieldGames.step (the stand-in of
tests/test_montecarlo_sequence_cpu.py); montecarlo.grid_start on CPU tensors against a per-car loop written from its definition; the
argument refusals of crx_field_traffic."""
import ctypes
import os

import numpy as np
import pytest
import torch

import conftest
import field_game_model as fgm
from test_montecarlo_sequence_cpu import BN, LAP, N_LMPC, PLAN, TAB, WIDTH, Recorder, _check_plant, _game, _game_step, _plant_pairs

CRX_ERR_ARG, CRX_ERR_NOT_INIT = -1, -4


def _track(name, width=0.8):
    from utils import racing_env

    return racing_env.ClosedTrack(np.genfromtxt(os.path.join(conftest.ROOT, "data/track_layout/%s.csv" % name), delimiter=","), track_width=width)


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
def test_model_rows_are_the_reference_rows():
    """The 160 recorded states as races of one and of four: every car's roll-out within 1e-12 of the reference's own rows (the bound of
    DESIGN section 14), and every gathered row the roll-out row of the right car, the ego skipped, in car order."""
    z = np.load(os.path.join(conftest.GOLDEN, "field_pred.npz"), allow_pickle=False)
    n_states = 0
    for name in (str(t) for t in z["tracks"]):
        track = _track(name)
        tab, L = track.point_and_tangent, track.lap_length
        for N in (12, 24):
            g = "%s_N%d" % (name, N)
            x, ps, pe = z[g + "/xcurv"], z[g + "/pred_s"], z[g + "/pred_ey"]
            n = x.shape[0]
            n_states += n
            for C in (1, 4):
                m = fgm.traffic(tab, L, x.reshape(n // C, C, 6), N)
                np.testing.assert_allclose(m["pred_s_car"].reshape(n, N + 1), ps, rtol=0, atol=1e-12, err_msg="%s C=%d" % (g, C))
                np.testing.assert_allclose(m["pred_ey_car"].reshape(n, N + 1), pe, rtol=0, atol=1e-12, err_msg="%s C=%d" % (g, C))
                assert m["n_all"].dtype == np.int32 and (m["n_all"] == C - 1).all()
                assert m["veh_xcurv"].shape == (n, C - 1, 6) and m["pred_s"].shape == (n, C - 1, N + 1) and m["pred_ey"].shape == (n, C - 1, N + 1)
                if C == 4:
                    # ego 2 of race r sees cars 0, 1, 3 of race r
                    for r in (0, n // C - 1):
                        assert np.array_equal(m["veh_xcurv"][4 * r + 2], x[4 * r + np.array([0, 1, 3])])
                        np.testing.assert_allclose(m["pred_s"][4 * r + 2], ps[4 * r + np.array([0, 1, 3])], rtol=0, atol=1e-12)
                        np.testing.assert_allclose(m["pred_ey"][4 * r + 2], pe[4 * r + np.array([0, 1, 3])], rtol=0, atol=1e-12)
    assert n_states == 160


def test_of_interest_windows():
    """check_ego_agent_distance's windows as the model states them: 4.5 lengths + half the speed difference ahead, one length behind, both
    across the line; a NaN is never of interest (G3)."""
    L = 20.0
    car = lambda s, vx=1.0: np.array([vx, 0, 0, 0, s, 0.0])   # noqa: E731
    assert fgm.of_interest(car(5.0), car(6.7), L) and not fgm.of_interest(car(5.0), car(6.9), L)            # 4.5 * 0.4 = 1.8 ahead
    assert fgm.of_interest(car(5.0, 1.4), car(7.0, 1.0), L)                                                 # + 0.5 * 0.4
    assert fgm.of_interest(car(5.0), car(4.7), L) and not fgm.of_interest(car(5.0), car(4.5), L)            # 0.4 behind
    assert fgm.of_interest(car(19.5), car(0.5), L) and fgm.of_interest(car(0.1), car(19.9), L)              # across the line
    assert not fgm.of_interest(car(5.0), car(np.nan), L) and not fgm.of_interest(car(np.nan), car(5.0), L)


# ---- the loop's launch sequence ----------------------------------------------------------------------------------------------------------
def _field_inputs(Bn):
    Lp, P = 4, 30
    return (np.zeros((Bn, Lp, P, 6)), np.zeros((Bn, Lp, P, 2)), np.zeros((Bn, Lp, P)), np.full((Bn, Lp), 20, dtype=np.int32),
            np.full(Bn, 2, dtype=np.int32), np.zeros((Bn, 6)), np.zeros((Bn, 6)), np.zeros((Bn, N_LMPC + 1, 6)), np.zeros((Bn, N_LMPC, 2)))


def _field_step(planner):
    return ["field_traffic_dev"] + _game_step(planner)[1:]


@pytest.mark.parametrize("planner", ["traj", "path"])
def test_field_games_step(AB, monkeypatch, planner):
    from crx import montecarlo

    rec = Recorder()
    monkeypatch.setattr(montecarlo, "torch_api", rec)
    R, C = 2, 3
    grid = dict(step_no=np.arange(R * C), n_log=np.arange(R * C) + 1, u_old=np.full((R * C, 2), 0.25))
    g = montecarlo.FieldGames(TAB, LAP, WIDTH, AB[0], AB[1], np.zeros((7, 6)), C, *_field_inputs(R * C), N=N_LMPC, device="cpu", planner=planner,
                              **grid)
    g.overlap = False
    lm = g.lm
    assert rec.take()[0] == []
    assert (g.n_races, g.n_cars, g.V, g.VA) == (R, C, C - 1, C - 1) and lm.batch == R * C
    assert (g.fdesc.N, g.fdesc.n_cars, g.fdesc.n_seg, g.fdesc.lap_length) == (g.Np, C, TAB.shape[0], LAP)
    assert (g.scene.n_all_max, g.scene.n_veh_max) == (C - 1, C - 1)
    # the grid fields reached `lm`; the others are those of a lap just begun
    assert lm.step_no.tolist() == list(range(R * C)) and lm.n_log.tolist() == list(range(1, R * C + 1)) and (lm.u_old == 0.25).all()
    assert lm.step_no.dtype == torch.int32 and (lm.u_prev == 0).all() and (lm.log_u == 0).all()
    assert len(_field_step(planner)) == (14 if planner == "traj" else 13)
    for _ in range(2):
        before = _plant_pairs(lm)
        g.step()
        names, args = rec.take()
        assert names == _field_step(planner)
        tr, sc = args["field_traffic_dev"], args["planner_scene_dev"]
        assert tr["desc"] is g.fdesc and tr["track"] is lm.tab and tr["xcurv"] is before[1] and tr["ws"] is g.fws
        assert sc["ego_xcurv"] is before[1] and sc["n_all"] is g.fws.n_all and sc["veh_xcurv"] is g.fws.veh_xcurv
        assert sc["pred_s"] is g.fws.pred_s and sc["pred_ey"] is g.fws.pred_ey and sc["ws"] is g.sws and sc["desc"] is g.scene
        if planner == "path":
            assert args["path_plan_dev"]["veh_xcurv"] is g.fws.veh_xcurv
        assert args["game_masks_dev"]["m_overtake"] is g.m_ot and args[PLAN[planner][-1]]["active"] is g.m_ot
        assert args["cbf_solve_dev"]["active"] is g.m_ot and args["lmpc_solve_dev"]["active"] is g.m_lm
        assert args["lmpc_prep_dev"]["lin_points"] is g.lin_points and args["lmpc_prep_dev"]["from_plan"] is False
        assert args["game_commit_dev"]["u"] is g.u and args["lmpc_addpoint_dev"]["x"] is before[1]
        _check_plant(lm, before, args["plant_step_wrap_dev"], args["cbf_solve_dev"]["x0"])
        assert args["game_log_dev"]["xcurv"] is lm.xc and args["lmpc_addtraj_dev"]["x"] is lm.xc
    # RaceStats sees a field: the other cars of the race, CarParam's dimensions, the branch mask as the flag
    inp = g.stats_inputs()
    assert inp["n_cars"] == C and (inp["l_sum"], inp["w_sum"]) == (0.4, 0.2) and inp["flag"] is g.m_ot and inp["xcurv"] is lm.xc
    assert inp.get("car_s0") is None and inp["laps"] is lm.laps
    # a GameLaps built beside it still launches what it launched
    game = _game(AB, planner)
    rec.take()
    game.step()
    names, args = rec.take()
    assert names == _game_step(planner)
    assert args["game_traffic_dev"]["car_s0"] is game.s0 and args["planner_scene_dev"]["veh_xcurv"] is game.veh
    assert args["planner_scene_dev"]["pred_s"] is game.pred_s and args["planner_scene_dev"]["n_all"] is game.n_all


def test_field_of_one_and_refusals(AB, monkeypatch):
    from crx import abi, montecarlo

    rec = Recorder()
    monkeypatch.setattr(montecarlo, "torch_api", rec)
    g = montecarlo.FieldGames(TAB, LAP, WIDTH, AB[0], AB[1], np.zeros((7, 6)), 1, *_field_inputs(BN), N=N_LMPC, device="cpu")
    g.overlap = False
    # one idle slot for the scene's arrays; the kernel reports n_all = 0
    assert (g.V, g.VA, g.fdesc.n_cars, g.n_races) == (1, 1, 1, BN) and tuple(g.fws.veh_xcurv.shape) == (BN, 1, 6) and (g.fws.n_all == 0).all()
    g.step()
    assert rec.take()[0] == _field_step("traj")
    for bad in (0, abi.CRX_MAX_VEH + 2):
        with pytest.raises(ValueError):
            montecarlo.FieldGames(TAB, LAP, WIDTH, AB[0], AB[1], np.zeros((7, 6)), bad, *_field_inputs(BN * 2), N=N_LMPC, device="cpu")
    with pytest.raises(ValueError):
        montecarlo.FieldGames(TAB, LAP, WIDTH, AB[0], AB[1], np.zeros((7, 6)), 2, *_field_inputs(3), N=N_LMPC, device="cpu")
    out = montecarlo.field_games(TAB, LAP, WIDTH, AB[0], AB[1], np.zeros((7, 6)), 3, *_field_inputs(6), 3, device="cpu")
    assert list(out) == ["xcurv", "u", "overtake", "flag", "laps", "traj_status"]
    assert out["xcurv"].shape == (4, 6, 6) and out["u"].shape == (3, 6, 2) and out["overtake"].shape == (3, 6) and out["overtake"].dtype == np.bool_
    assert out["flag"].dtype == np.int32 and out["laps"].shape == (6,) and out["traj_status"].shape == (6,)


# ---- grid_start --------------------------------------------------------------------------------------------------------------------------
class _Track:
    """The three members grid_start reads of the mirror's ClosedTrack, with an arithmetic the test can restate."""
    lap_length = 19.5

    def get_global_position(self, s, ey):
        return 2.0 * s + ey, s - 3.0 * ey

    def get_orientation(self, s, ey):
        return 0.125 * s - ey


def _grid_inputs(seed=0):
    """B = 5 cars with safe sets of their own: laps of two different lengths, it = 2 or 3, distinct numbers everywhere."""
    rng = np.random.default_rng(seed)
    Bn, Lp, P, N = 5, 4, 64, 6
    ss, us, qf = rng.standard_normal((Bn, Lp, P, 6)), rng.standard_normal((Bn, Lp, P, 2)), rng.standard_normal((Bn, Lp, P))
    ss[:, :, 3, 1] = -0.0                                                            # add_point's x + 0.0 turns it into +0.0
    time_ss = np.full((Bn, Lp), 10000, dtype=np.int32)
    it = np.array([2, 3, 2, 3, 2], dtype=np.int32)
    for b in range(Bn):
        time_ss[b, :it[b]] = 21 if b % 2 else 17
    return dict(ss_xcurv=ss, u_ss=us, qfun=qf, time_ss=time_ss, it=it, xcurv0=rng.standard_normal((Bn, 6)), xglob0=rng.standard_normal((Bn, 6)),
                lin_points=ss[:, 0, 1:N + 2].copy(), lin_input=us[:, 0, 1:N + 1].copy()), N


def _grid_by_definition(inp, k, track, N):
    """grid_start's definition, car by car: drive k steps of lap j = it - 1 again through the three bookkeeping rules -- the commit (applied
    input, u_prev <- u_old <- u, the plan shifted by a stage with its last one repeated, the step counter), add_point (row time_ss + step + 1
    of lap j: x + (0,0,0,0,L,0), u) and the lap log (the new state and the applied input)."""
    out = {name: np.array(a) for name, a in inp.items()}
    Bn, _, P, _ = out["ss_xcurv"].shape
    out.update(step_no=np.zeros(Bn, dtype=np.int32), n_log=np.ones(Bn, dtype=np.int32), log_x=np.zeros((Bn, P, 6)), log_u=np.zeros((Bn, P, 2)),
               u_old=np.zeros((Bn, 2)), u_prev=np.zeros((Bn, 2)))
    out["log_x"][:, 0] = inp["xcurv0"]
    for b in range(Bn):
        if k[b] == 0:
            continue
        j = inp["it"][b] - 1
        lap_x, lap_u, T = inp["ss_xcurv"][b, j].copy(), inp["u_ss"][b, j].copy(), inp["time_ss"][b, j]
        x = lap_x[0]
        out["log_x"][b, 0] = x
        for i in range(k[b]):
            X, U = lap_x[i:i + N + 1], lap_u[i:i + N]
            u = U[0]
            out["u_prev"][b], out["u_old"][b] = out["u_old"][b], u
            out["lin_points"][b] = np.concatenate([X[1:], X[-1:]])
            out["lin_input"][b] = np.concatenate([U[1:], U[-1:]])
            row = T + out["step_no"][b] + 1
            out["step_no"][b] += 1
            if row < P:
                out["ss_xcurv"][b, j, row] = x + np.array([0, 0, 0, 0, track.lap_length, 0.0])
                out["u_ss"][b, j, row] = u
            x = lap_x[i + 1]
            out["log_x"][b, out["n_log"][b]], out["log_u"][b, out["n_log"][b] - 1] = x, u
            out["n_log"][b] += 1
        out["xcurv0"][b] = x
        out["xglob0"][b, 0:3] = x[0:3]
        out["xglob0"][b, 3] = track.get_orientation(x[4], x[5]) + x[3]
        out["xglob0"][b, 4], out["xglob0"][b, 5] = track.get_global_position(x[4], x[5])
    return out


def _bits(a):
    a = a.numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def test_grid_start_is_its_definition():
    from crx import montecarlo

    inp, N = _grid_inputs()
    track = _Track()
    T = inp["time_ss"][np.arange(5), inp["it"] - 1]
    assert sorted(set(T.tolist())) == [17, 21]
    k = np.array([0, 1, 2, 7, T[4] - N - 1], dtype=np.int32)
    want = _grid_by_definition(inp, k, track, N)
    for given in (inp, {name: torch.as_tensor(a) for name, a in inp.items()}):          # host arrays, or tensors
        got = montecarlo.grid_start(given, k, track)
        assert sorted(got) == sorted(want)
        for name in want:
            g = got[name]
            assert torch.is_tensor(g) and tuple(g.shape) == want[name].shape and g.numpy().dtype == want[name].dtype, name
            assert np.array_equal(_bits(g), _bits(want[name])), name
    # what the list in DESIGN section 17 says of the moved cars
    got = {name: a.numpy() for name, a in got.items()}
    for b in (1, 2, 3, 4):
        j, kb = inp["it"][b] - 1, int(k[b])
        assert np.array_equal(got["xcurv0"][b], inp["ss_xcurv"][b, j, kb]) and got["step_no"][b] == kb and got["n_log"][b] == kb + 1
        assert np.array_equal(got["lin_points"][b, :N], inp["ss_xcurv"][b, j, kb:kb + N]) and np.array_equal(got["lin_points"][b, N], got["lin_points"][b, N - 1])
        assert np.array_equal(got["lin_input"][b, :N - 1], inp["u_ss"][b, j, kb:kb + N - 1]) and np.array_equal(got["lin_input"][b, N - 1], got["lin_input"][b, N - 2])
        assert np.array_equal(got["log_x"][b, :kb + 1], inp["ss_xcurv"][b, j, :kb + 1]) and (got["log_x"][b, kb + 1:] == 0).all()
        assert np.array_equal(got["u_old"][b], inp["u_ss"][b, j, kb - 1])
        assert np.array_equal(got["u_prev"][b], inp["u_ss"][b, j, kb - 2] if kb >= 2 else np.zeros(2))
        assert np.array_equal(got["ss_xcurv"][b, j, T[b] + 1:T[b] + 1 + kb, 4], inp["ss_xcurv"][b, j, :kb, 4] + track.lap_length)
        assert np.array_equal(got["ss_xcurv"][b, j, T[b] + 1 + kb:], inp["ss_xcurv"][b, j, T[b] + 1 + kb:])      # nothing beyond the k rows
    assert not np.signbit(got["ss_xcurv"][3, inp["it"][3] - 1, T[3] + 1 + 3, 1])        # -0.0 + 0.0, as the kernel adds
    # the other laps, and car 0, are untouched
    assert np.array_equal(_bits(got["ss_xcurv"][0]), _bits(inp["ss_xcurv"][0])) and np.array_equal(_bits(got["ss_xcurv"][1, 0]), _bits(inp["ss_xcurv"][1, 0]))
    assert np.array_equal(_bits(got["qfun"]), _bits(inp["qfun"])) and np.array_equal(got["time_ss"], inp["time_ss"])


def test_grid_start_identity_and_range():
    from crx import montecarlo

    inp, N = _grid_inputs(1)
    given = {name: torch.as_tensor(a) for name, a in inp.items()}
    got = montecarlo.grid_start(given, np.zeros(5, dtype=np.int32), _Track())
    for name, a in given.items():
        assert got[name] is a, name                                                     # k = 0: the inputs themselves
    assert (got["step_no"] == 0).all() and (got["n_log"] == 1).all() and torch.equal(got["log_x"][:, 0], given["xcurv0"])
    assert (got["log_x"][:, 1:] == 0).all() and (got["log_u"] == 0).all() and (got["u_old"] == 0).all() and (got["u_prev"] == 0).all()
    T = inp["time_ss"][np.arange(5), inp["it"] - 1]
    for b, bad in ((0, -1), (2, T[2] - N), (4, 1000)):
        k = np.zeros(5, dtype=np.int32)
        k[b] = bad
        with pytest.raises(ValueError):
            montecarlo.grid_start(given, k, _Track())
    with pytest.raises(ValueError):
        montecarlo.grid_start(given, np.zeros(4, dtype=np.int32), _Track())
    montecarlo.grid_start(given, T - N - 1, _Track())                                   # the last admissible k of every car


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_field_traffic_symbols_and_refusals():
    import crx
    from crx import abi

    lib = crx.lib()
    src = open(os.path.join(conftest.ROOT, "include", "crx.h")).read()
    for n in ("crx_field_traffic", "crx_field_traffic_dev"):
        assert hasattr(lib, n) and n + "(" in src, n
        getattr(lib, n).restype = ctypes.c_int
    assert lib.crx_version() == 400
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    R, C, N, S = 3, 4, 10, 9
    names = ("track", "xcurv", "pred_s_car", "pred_ey_car", "veh_xcurv", "pred_s", "pred_ey", "n_all")

    def arrays(C=C):
        V = C - 1
        return dict(track=np.ones((S, 6)), xcurv=np.ones((R, C, 6)), pred_s_car=np.ones((R, C, N + 1)), pred_ey_car=np.ones((R, C, N + 1)),
                    veh_xcurv=np.ones((R * C, V, 6)), pred_s=np.ones((R * C, V, N + 1)), pred_ey=np.ones((R * C, V, N + 1)),
                    n_all=np.zeros(R * C, dtype=np.int32))

    def call(d, a, n_races=R, dev=False):
        ptrs = [p(a[k]) for k in names]
        if dev:
            return lib.crx_field_traffic_dev(ctypes.byref(d) if d is not None else None, ctypes.c_int(n_races), *ptrs, None)
        return lib.crx_field_traffic(ctypes.byref(d) if d is not None else None, ctypes.c_int(n_races), *ptrs)

    def refused(d, a, what, **kw):
        for dev in (False, True):
            assert call(d, a, dev=dev, **kw) == CRX_ERR_ARG, (what, dev)
            assert lib.crx_last_error(), what

    good = lambda **kw: abi.field_desc(N, C, S, 19.25, **kw)   # noqa: E731
    refused(None, arrays(), "desc")
    for bad_N in (0, abi.CRX_MAX_N + 1):
        refused(abi.field_desc(bad_N, C, S, 19.25), arrays(), "N")
    for bad_C in (0, abi.CRX_MAX_VEH + 2):
        refused(abi.field_desc(N, bad_C, S, 19.25), arrays(), "n_cars")
        assert b"n_cars" in lib.crx_last_error()
    for bad_S in (0, 65):
        refused(abi.field_desc(N, C, bad_S, 19.25), arrays(), "n_seg")
    for bad in (0.0, -1.0, np.inf, np.nan):
        refused(abi.field_desc(N, C, S, bad), arrays(), "lap_length")
        refused(good(dt=bad), arrays(), "dt")
    refused(good(), arrays(), "n_races", n_races=-1)
    for hole in names:
        refused(good(), dict(arrays(), **{hole: None}), hole)
        assert b"NULL" in lib.crx_last_error()
    if not torch.cuda.is_available():      # well-formed calls get as far as the library's state and never compute without a device
        one = arrays(C=1)
        for d, a in ((good(), arrays()), (abi.field_desc(N, 1, S, 19.25), dict(one, veh_xcurv=None, pred_s=None, pred_ey=None)),
                     (abi.field_desc(abi.CRX_MAX_N, abi.CRX_MAX_VEH + 1, 64, 19.25), arrays(C=abi.CRX_MAX_VEH + 1))):
            for dev in (False, True):
                assert call(d, a, dev=dev) == CRX_ERR_NOT_INIT, (d.N, d.n_cars, dev)
