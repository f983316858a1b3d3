"""The launch sequence of every closed loop of crx.montecarlo, without a GPU and without the library: crx.montecarlo.torch_api is replaced
by a stand-in that records each wrapper call (`*_dev`, longest_first) with its arguments and launches nothing.  Pinned per loop: (a) which
wrappers one control step calls, in which order, and (b) which tensor goes where -- the plant reads xg / xc and writes xg_next / xc_next,
the two pairs then exchange bindings, and the step's solver launch was given the tensor that is xc_next afterwards (bench.py re-issues
that launch on it).  The bit-identity tests of the GPU suite hang on exactly these sequences."""
import inspect

import numpy as np
import pytest
import torch

from crx import montecarlo, torch_api

BN, N_LMPC = 3, 12
TAB, LAP, WIDTH = np.zeros((5, 6)), 20.0, 1.0


class _Models:
    """CbfModels without the library: holds the models and records the reach-table launch of the real constructor."""

    def __init__(self, rec, desc, A, B):
        self.A, self.B = A, B
        rec.calls.append(("crx_cbf_models_reach_dev", dict(desc=desc, A=A, B=B)))


class Recorder:
    """Stands in for crx.torch_api: workspace classes and constants are the real ones; every `*_dev` wrapper and longest_first is recorded as
    (name, arguments by parameter name) and returns what its caller goes on with."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        real = getattr(torch_api, name)
        if name == "CbfModels":
            return lambda desc, A, B: _Models(self, desc, A, B)
        if name == "new_streams":
            return lambda n, device=None: ([None] * n, 0)
        if not (name.endswith("_dev") or name == "longest_first"):
            return real
        sig = inspect.signature(real)

        def record(*a, **kw):
            args = sig.bind(*a, **kw)
            args.apply_defaults()
            args = dict(args.arguments)
            self.calls.append((name, args))
            if name == "longest_first":
                return torch.zeros(args["iters"].shape[0], dtype=torch.int32)
            if name == "lqr_design_dev":
                return torch_api.LqrWorkspace(args["A"].shape[0], args["A"].device)
            if name == "plant_step_dev":
                return args["xglob"].clone(), args["xcurv"].clone()
            return args.get("ws")

        return record

    def take(self):
        """The calls recorded since the last take(): (names, {name: arguments}; a name called twice keeps its last arguments)."""
        calls, self.calls = self.calls, []
        return [n for n, _ in calls], dict(calls)


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(montecarlo, "torch_api", r)
    return r


def _plant_pairs(loop):
    return loop.xg, loop.xc, loop.xg_next, loop.xc_next


def _check_plant(loop, before, plant_args, solver_x=None):
    """The plant launch read xg / xc and wrote xg_next / xc_next as they were bound before the step, on the loop's plant descriptor and
    track table; the step then swapped both pairs; the solver launch was given what is xc_next now."""
    xg, xc, xg_next, xc_next = before
    assert plant_args["desc"] is loop.plant and plant_args["track"] is loop.tab and plant_args["laps"] is loop.laps
    assert plant_args["xglob"] is xg and plant_args["xcurv"] is xc
    assert plant_args["xglob_next"] is xg_next and plant_args["xcurv_next"] is xc_next
    assert loop.xg is xg_next and loop.xc is xc_next and loop.xg_next is xg and loop.xc_next is xc
    if solver_x is not None:
        assert solver_x is loop.xc_next


def _cars(V):
    return np.full((BN, V), 3.0), np.full((BN, V), 0.2), np.zeros((BN, V))


def _races(AB, **kw):
    z = np.zeros((BN, 6))
    return montecarlo.MpccbfRaces(TAB, LAP, WIDTH, AB[0], AB[1], z, z, *_cars(2), device="cpu", **kw)


def _lmpc_inputs():
    L, P = 4, 30
    return (np.zeros((BN, L, P, 6)), np.zeros((BN, L, P, 2)), np.zeros((BN, L, P)), np.full((BN, L), 20, dtype=np.int32),
            np.full(BN, 2, dtype=np.int32), np.zeros((BN, 6)), np.zeros((BN, 6)), np.zeros((BN, N_LMPC + 1, 6)), np.zeros((BN, N_LMPC, 2)))


def _lmpc(**kw):
    return montecarlo.LmpcLaps(TAB, LAP, WIDTH, *_lmpc_inputs(), N=N_LMPC, device="cpu", **kw)


def _game(AB, planner):
    g = montecarlo.GameLaps(TAB, LAP, WIDTH, AB[0], AB[1], np.zeros((7, 6)), *_lmpc_inputs(), *_cars(3), N=N_LMPC, device="cpu",
                            planner=planner)
    g.overlap = False
    return g


LMPC_STEP = ["lmpc_prep_dev", "lmpc_solve_dev", "game_commit_dev", "lmpc_addpoint_dev", "plant_step_wrap_dev", "game_log_dev", "lmpc_addtraj_dev"]
LMPC_STEP_TORCH = ["lmpc_prep_dev", "lmpc_solve_dev", "lmpc_addpoint_dev", "plant_step_wrap_dev", "lmpc_addtraj_dev"]
PLAN = {"traj": ["planner_prep_dev", "planner_plan_dev"], "path": ["path_plan_dev"]}


def _game_step(planner):
    return (["game_traffic_dev", "planner_scene_dev", "game_masks_dev"] + PLAN[planner] + ["track_prep_dev", "cbf_solve_dev"] + LMPC_STEP)


def _game_step_torch(planner):
    return ["planner_scene_dev"] + PLAN[planner] + ["track_prep_dev", "cbf_solve_dev"] + LMPC_STEP_TORCH


@pytest.mark.parametrize("models", [False, True])
def test_mpccbf_races(rec, AB, models):
    kw = dict(models=(np.tile(AB[0], (BN, 1, 1)), np.tile(AB[1], (BN, 1, 1)))) if models else {}
    r = _races(AB, **kw)
    assert rec.take()[0] == (["crx_cbf_models_reach_dev"] if models else [])
    before = _plant_pairs(r)
    r.step()
    names, args = rec.take()
    assert names == ["cbf_prep_dev", "cbf_solve_dev", "plant_step_wrap_dev"]
    assert args["cbf_prep_dev"]["xcurv"] is before[1]
    assert args["cbf_solve_dev"]["order"] is None and args["cbf_solve_dev"]["models"] is r.models and (r.models is not None) == models
    assert args["plant_step_wrap_dev"]["u"] is r.ws.U and args["plant_step_wrap_dev"]["u_stride"] == 2 * r.N
    assert args["plant_step_wrap_dev"]["noise_z"] is None
    _check_plant(r, before, args["plant_step_wrap_dev"], args["cbf_solve_dev"]["x0"])
    xg, xc = r.xg, r.xc
    r.step_glue()
    names, args = rec.take()
    assert names == ["cbf_solve_dev", "plant_step_dev"]
    assert args["cbf_solve_dev"]["x0"] is xc and args["plant_step_dev"]["xglob"] is xg and args["plant_step_dev"]["xcurv"] is xc
    assert args["plant_step_dev"]["desc"] is r.plant


def test_mpccbf_races_longest_first(rec, AB):
    r = _races(AB, noise_seed=5)
    r.dispatch = "longest_first"
    before = _plant_pairs(r)
    r.step()
    names, args = rec.take()
    assert names == ["cbf_prep_dev", "longest_first", "cbf_solve_dev", "plant_step_wrap_dev"]
    assert args["longest_first"]["iters"] is r.ws.iters and args["longest_first"]["active"] is None
    assert args["cbf_solve_dev"]["order"] is not None
    assert tuple(args["plant_step_wrap_dev"]["noise_z"].shape) == (BN, 3)          # seeded: one draw per step
    _check_plant(r, before, args["plant_step_wrap_dev"], args["cbf_solve_dev"]["x0"])


def test_ilqr_races(rec, AB):
    z = np.zeros((BN, 6))
    r = montecarlo.IlqrRaces(TAB, LAP, AB[0], AB[1], z, z, np.full(BN, 3.0), np.full(BN, 0.2), np.zeros(BN), N=12, device="cpu")
    assert rec.take()[0] == []
    before = _plant_pairs(r)
    r.step()
    names, args = rec.take()
    assert names == ["ilqr_solve_dev", "plant_step_wrap_dev"]
    assert args["plant_step_wrap_dev"]["u"] is r.ws.U and args["plant_step_wrap_dev"]["u_stride"] == 2 * r.N
    _check_plant(r, before, args["plant_step_wrap_dev"], args["ilqr_solve_dev"]["x0"])


def test_lqr_laps(rec, AB):
    z = np.zeros((BN, 6))
    r = montecarlo.LqrLaps(TAB, LAP, z, z, AB[0], AB[1], device="cpu")
    names, args = rec.take()
    assert names == ["lqr_design_dev"] and args["lqr_design_dev"]["A"] is r.A and args["lqr_design_dev"]["B"] is r.B
    before = _plant_pairs(r)
    r.step()
    names, args = rec.take()
    assert names == ["lqr_step_dev", "plant_step_wrap_dev"]
    assert args["lqr_step_dev"]["K"] is r.K and args["lqr_step_dev"]["u"] is r.u
    assert args["plant_step_wrap_dev"]["u"] is r.u and args["plant_step_wrap_dev"]["u_stride"] == 2
    _check_plant(r, before, args["plant_step_wrap_dev"], args["lqr_step_dev"]["xcurv"])


def test_pid_laps(rec):
    z, T = np.zeros((BN, 6)), 4
    noise_z = torch.arange(T * BN * 3, dtype=torch.float64).reshape(T, BN, 3)
    r = montecarlo.PidLaps(TAB, LAP, z, z, T, noise_z=noise_z, noise_seed=3, device="cpu")
    assert rec.take()[0] == ["pid_log_dev"]
    gen_state = r.noise.gen.get_state()
    for k in range(2):
        before, u = _plant_pairs(r), r.u
        r.step()
        names, args = rec.take()
        assert names == ["plant_step_wrap_dev", "pid_log_dev"]
        assert torch.equal(args["plant_step_wrap_dev"]["noise_z"], noise_z[k])
        assert args["plant_step_wrap_dev"]["noise_z"].data_ptr() == r.noise_z[k].data_ptr()
        assert args["plant_step_wrap_dev"]["u"] is u and args["plant_step_wrap_dev"]["u_stride"] == 2
        _check_plant(r, before, args["plant_step_wrap_dev"])
        assert args["pid_log_dev"]["xcurv"] is r.xc and args["pid_log_dev"]["row"] == k and args["pid_log_dev"]["u_next"] is r.u
    assert torch.equal(r.noise.gen.get_state(), gen_state)                         # a given noise_z leaves the loop's generator alone
    # without noise_z the same generator is drawn from, once per step
    r = montecarlo.PidLaps(TAB, LAP, z, z, T, noise_seed=3, device="cpu")
    rec.take()
    r.step()
    assert tuple(rec.take()[1]["plant_step_wrap_dev"]["noise_z"].shape) == (BN, 3)
    assert not torch.equal(r.noise.gen.get_state(), gen_state)


@pytest.mark.parametrize("torch_glue", [False, True])
def test_lmpc_laps(rec, torch_glue):
    r = _lmpc()
    assert rec.take()[0] == []
    for k in range(2):
        before = _plant_pairs(r)
        r.step(torch_glue=torch_glue)
        names, args = rec.take()
        assert names == (LMPC_STEP_TORCH if torch_glue else LMPC_STEP)
        prep, qp, addpoint, plant = (args[n] for n in ("lmpc_prep_dev", "lmpc_solve_dev", "lmpc_addpoint_dev", "plant_step_wrap_dev"))
        assert prep["desc"] is r.pdesc and prep["ws"] is r.pws and prep["x"] is before[1] and prep["active"] is None
        if k == 0:      # the linearisation points handed over, then the previous plan
            assert prep["lin_points"] is r.lin_points and prep["lin_input"] is r.lin_input and prep["from_plan"] is False
        else:
            assert prep["lin_points"] is r.ws.X and prep["lin_input"] is r.ws.U and prep["from_plan"] is True
        assert qp["u_old"] is r.u_old and qp["ws"] is r.ws and qp["order"] is None and qp["active"] is None
        assert qp["A"] is r.pws.A and qp["ss"] is r.pws.ss and qp["n_ss"] is r.n_ss
        assert addpoint["desc"] is r.pdesc and addpoint["x"] is before[1]
        if torch_glue:
            assert addpoint["step"] is r.step_no and addpoint["u"] is r.ws.U and addpoint["u_stride"] == 2 * N_LMPC
        else:
            assert addpoint["step"] is r.addpoint_step and addpoint["u"] is r.u and addpoint["u_stride"] == 2
            assert args["game_log_dev"]["xcurv"] is r.xc and args["game_log_dev"]["u"] is r.u
        assert plant["u"] is addpoint["u"] and plant["u_stride"] == addpoint["u_stride"]
        _check_plant(r, before, plant, qp["x0"])
        assert args["lmpc_addtraj_dev"]["x"] is r.xc and r.k == k + 1
    r = _lmpc()
    r.dispatch = "longest_first"
    r.step()
    names, args = rec.take()
    assert names == LMPC_STEP[:1] + ["longest_first"] + LMPC_STEP[1:]
    assert args["longest_first"]["iters"] is r.ws.iters and args["lmpc_solve_dev"]["order"] is not None


@pytest.mark.parametrize("planner", ["traj", "path"])
def test_game_laps(rec, AB, planner):
    g = _game(AB, planner)
    lm = g.lm
    assert rec.take()[0] == []
    target = g.selws.best_X if planner == "traj" else g.ppws.target
    for k in range(2):
        before = _plant_pairs(lm)
        g.step()
        names, args = rec.take()
        assert names == _game_step(planner)
        assert args["game_masks_dev"]["m_overtake"] is g.m_ot and args["game_masks_dev"]["m_lmpc"] is g.m_lm
        assert args[PLAN[planner][-1]]["active"] is g.m_ot
        assert args["track_prep_dev"]["traj"] is target and args["track_prep_dev"]["xt"] is g.xt
        assert args["cbf_solve_dev"]["active"] is g.m_ot and args["cbf_solve_dev"]["ws"] is g.tws and args["cbf_solve_dev"]["order"] is None
        prep, qp, addpoint = args["lmpc_prep_dev"], args["lmpc_solve_dev"], args["lmpc_addpoint_dev"]
        # the game plans from its own linearisation points, every step
        assert prep["lin_points"] is g.lin_points and prep["lin_input"] is g.lin_input and prep["from_plan"] is False
        assert prep["active"] is g.m_lm and qp["active"] is g.m_lm and qp["u_old"] is lm.u_old and qp["order"] is None
        assert args["game_commit_dev"]["u"] is g.u and args["game_commit_dev"]["flag"] is g.flag
        assert addpoint["step"] is lm.addpoint_step and addpoint["u"] is g.u and addpoint["u_stride"] == 2 and addpoint["x"] is before[1]
        assert args["plant_step_wrap_dev"]["u"] is g.u and args["plant_step_wrap_dev"]["u_stride"] == 2
        _check_plant(lm, before, args["plant_step_wrap_dev"], args["cbf_solve_dev"]["x0"])
        assert qp["x0"] is lm.xc_next and args["game_log_dev"]["u"] is g.u and args["game_log_dev"]["xcurv"] is lm.xc
    assert lm.k == 0                                                               # advanced by LmpcLaps.step only
    before = _plant_pairs(lm)
    g.step_torch()
    names, args = rec.take()
    assert names == _game_step_torch(planner)
    assert args["track_prep_dev"]["traj"] is target
    assert args["lmpc_prep_dev"]["lin_points"] is g.lin_points and args["lmpc_prep_dev"]["from_plan"] is False
    assert args["cbf_solve_dev"]["active"] is args[PLAN[planner][-1]]["active"]
    assert torch.equal(args["cbf_solve_dev"]["active"] + args["lmpc_solve_dev"]["active"], torch.ones(BN, dtype=torch.int32))
    assert args["lmpc_addpoint_dev"]["u"] is g.u and args["lmpc_addpoint_dev"]["u_stride"] == 2
    _check_plant(lm, before, args["plant_step_wrap_dev"], args["cbf_solve_dev"]["x0"])
    assert lm.k == 0


def test_game_laps_longest_first(rec, AB):
    """dispatch is read from the GameLaps (where bench.py sets it), for both masked solver launches."""
    g = _game(AB, "traj")
    g.dispatch = "longest_first"
    g.step()
    names = [n for n, _ in rec.calls]
    want = _game_step("traj")
    for solver in ("cbf_solve_dev", "lmpc_solve_dev"):
        want.insert(want.index(solver), "longest_first")
    assert names == want
    orders = [a for n, a in rec.calls if n == "longest_first"]
    assert orders[0]["iters"] is g.tws.iters and orders[0]["active"] is g.m_ot
    assert orders[1]["iters"] is g.lm.ws.iters and orders[1]["active"] is g.m_lm
    args = dict(rec.calls)
    assert args["cbf_solve_dev"]["order"] is not None and args["lmpc_solve_dev"]["order"] is not None


def test_run_and_log_functions(rec, AB):
    """The run-to-the-end functions: keys, shapes and dtypes of what they return."""
    z, cars = np.zeros((BN, 6)), _cars(2)
    out = montecarlo.mpccbf_races(TAB, LAP, WIDTH, AB[0], AB[1], z, z, *cars, 4, device="cpu", log_every=2)
    assert list(out) == ["xcurv", "u", "status", "laps"]
    assert out["xcurv"].shape == (3, BN, 6) and out["u"].shape == (2, BN, 2) and out["status"].shape == (2, BN) and out["laps"].shape == (BN,)
    assert out["status"].dtype == np.int32 and out["laps"].dtype == np.int32
    out = montecarlo.ilqr_races(TAB, LAP, AB[0], AB[1], z, z, np.full(BN, 3.0), np.full(BN, 0.2), np.zeros(BN), 4, N=12, device="cpu", log_every=2)
    assert list(out) == ["xcurv", "u", "status", "iters", "laps"]
    assert out["xcurv"].shape == (3, BN, 6) and out["u"].shape == (2, BN, 2) and out["iters"].shape == (2, BN)
    out = montecarlo.lqr_laps(TAB, LAP, z, z, 4, AB[0], AB[1], device="cpu", log_every=2)
    assert list(out) == ["xcurv", "u", "K", "design_status", "design_iters", "laps"]
    assert out["xcurv"].shape == (3, BN, 6) and out["u"].shape == (2, BN, 2) and out["K"].shape == (BN, 2, 6)
    out = montecarlo.lmpc_laps(TAB, LAP, WIDTH, *_lmpc_inputs(), 3, N=N_LMPC, device="cpu")
    assert list(out) == ["xcurv", "u", "status", "prep_status", "laps", "traj_status"]
    assert out["xcurv"].shape == (4, BN, 6) and out["u"].shape == (3, BN, 2) and out["prep_status"].shape == (3, BN)
    assert out["traj_status"].shape == (BN,) and out["traj_status"].dtype == np.int32
    s0, v, ey = _cars(3)
    v[:] = 0.5
    rec.take()
    out = montecarlo.game_laps(TAB, LAP, WIDTH, AB[0], AB[1], np.zeros((7, 6)), *_lmpc_inputs(), s0, v, ey, 3, device="cpu")
    assert list(out) == ["xcurv", "u", "overtake", "flag", "cars_s", "laps", "traj_status", "scene_overflow"]
    assert out["xcurv"].shape == (4, BN, 6) and out["u"].shape == (3, BN, 2) and out["cars_s"].shape == (3, BN, 3)
    assert out["overtake"].shape == (3, BN) and out["overtake"].dtype == np.bool_ and out["flag"].dtype == np.int32
    assert out["scene_overflow"].shape == (BN,)
    # cars_s is the scripted cars' s BEFORE the step: the first row is at t = 0
    assert np.array_equal(out["cars_s"][0], s0) and np.allclose(out["cars_s"][1], s0 + 0.5 * 0.1)
