"""Race statistics without a GPU: the numpy model (tests/race_stats_model.py) against the per-step torch formulation tools/multi_tests.py
carried before the statistics moved into the library; what the host-pointer entries refuse; the descriptor's layout; and the launch
sequence of montecarlo.RaceStats on the loops it attaches to."""
import ctypes
import os

import numpy as np
import pytest
import torch

import race_stats_model as rsm
from test_montecarlo_sequence_cpu import BN, LAP, TAB, WIDTH, Recorder, _game, _game_step, _races

ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    import crx
    from crx import abi

    if not os.path.exists(crx.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    L = crx.lib()
    abi.bind_stats(L)
    return L


def test_model_reproduces_the_torch_formulation():
    """B = 7 races against V = 3 scripted cars over 40 samples, s over several laps.  The block between the markers is the statistics code
    of tools/multi_tests.py as it stood (r.lm.xc -> xc, r.lm.laps -> laps_now, r.t -> t, r.overtake -> overtake), on CPU tensors."""
    Bn, V, T, L, width = 7, 3, 40, 19.25, 1.0
    rng = np.random.default_rng(11)
    cs0, cv, cey = rng.uniform(0.0, 3 * L, (Bn, V)), rng.uniform(0.0, 1.5, (Bn, V)), rng.uniform(-0.8, 0.8, (Bn, V))
    s_total = rng.uniform(0.0, L, Bn)
    laps0 = np.zeros(Bn, dtype=np.int32)
    q = dict(cs0=torch.as_tensor(cs0), cv=torch.as_tensor(cv), cey=torch.as_tensor(cey), prev=torch.as_tensor(laps0).clone(),
             ncross=torch.zeros(Bn, dtype=torch.int32), t1=torch.zeros(Bn, dtype=torch.int32), t2=torch.zeros(Bn, dtype=torch.int32),
             gap=torch.full((Bn,), 1e9, dtype=torch.float64), off=torch.zeros(Bn, dtype=torch.bool),
             eymax=torch.zeros(Bn, dtype=torch.float64), ot=torch.zeros(Bn, dtype=torch.int64))
    st = rsm.reset(Bn, V, laps0)
    t = 0.0
    for k in range(T):
        s_total = s_total + rng.uniform(0.0, 4.0, Bn)           # up to a fifth of a lap per sample: ~4 laps over the run
        x = rng.uniform(-1.0, 1.0, (Bn, 6))
        x[:, 4], x[:, 5] = np.fmod(s_total, L), rng.uniform(-1.3, 1.3, Bn)
        x[:2, 5] *= 0.7                                         # two cars that stay on the track
        laps_np = np.floor(s_total / L).astype(np.int32)
        flag_np = (rng.uniform(size=Bn) < 0.4).astype(np.int32)
        t += 0.1
        xc, laps_now, overtake = torch.as_tensor(x), torch.as_tensor(laps_np), torch.as_tensor(flag_np)
        # ---- tools/multi_tests.py ----
        cars = q["cv"] * t + q["cs0"]
        ds = torch.remainder(xc[:, 4:5] - cars + 0.5 * L, L) - 0.5 * L
        de = xc[:, 5:6] - q["cey"]
        q["gap"] = torch.minimum(q["gap"], ((ds / 0.4) ** 6 + (de / 0.2) ** 6).min(dim=1).values)   # >= 1: no contact
        q["off"] |= xc[:, 5].abs() > width
        q["eymax"] = torch.maximum(q["eymax"], xc[:, 5].abs())
        q["ot"] += overtake.long()
        crossed = laps_now > q["prev"]
        q["t1"] = torch.where(crossed & (q["ncross"] == 0), k + 1, q["t1"])
        q["t2"] = torch.where(crossed & (q["ncross"] == 1), k + 1, q["t2"])
        q["ncross"] += crossed.int()
        q["prev"] = laps_now.clone()
        # ---- end ----
        rsm.sample(st, k + 1, x, laps_np, L, width, t=t, car_s0=cs0, car_v=cv, car_ey=cey, flag=flag_np)
    ncross, t1, t2 = (q[n].numpy() for n in ("ncross", "t1", "t2"))
    assert ncross.max() >= 3 and (ncross >= 2).all()               # several laps, and no sample advanced a counter by two
    assert np.array_equal(st["n_laps"], ncross)
    assert np.array_equal(st["lap_step"][0], t1) and np.array_equal(st["lap_step"][1], t2)
    assert np.array_equal(st["off_step"] >= 0, q["off"].numpy()) and q["off"].sum() == Bn - 2
    assert np.array_equal(st["ey_max"], q["eymax"].numpy())
    assert np.array_equal(st["flag_samples"], q["ot"].numpy())
    np.testing.assert_allclose(st["min_clear"], q["gap"].numpy(), rtol=1e-13, atol=0)
    assert np.array_equal(st["n_samples"], np.full(Bn, T)) and (st["nonfinite_step"] == -1).all()


def test_desc_default_matches_the_mirror(lib):
    from crx import abi

    for n_opp_max, n_cars in ((3, 0), (6, 7), (0, 0)):
        d = abi.StatsDesc()
        lib.crx_stats_desc_default(ctypes.byref(d), n_opp_max, n_cars, 19.25, 0.8)
        assert bytes(d) == bytes(abi.stats_desc(n_opp_max, n_cars, 19.25, 0.8))
    assert ctypes.sizeof(abi.StatsDesc) == 48


def _host_call(lib, d, Bn, car=True, n_opp=False, dims=False, entry="race_stats", group=False, n_groups=1):
    """One call of a host-pointer entry on zero arrays, with the optional arrays named; returns the status."""
    V = d.n_opp_max
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    si, sd = np.zeros((19, max(Bn, 1)), dtype=np.int32), np.zeros((4 + max(V, 0), max(Bn, 1)))
    if entry == "race_stats_summary":
        return lib.crx_race_stats_summary(ctypes.byref(d), Bn, p(np.zeros(max(Bn, 1), dtype=np.int32)) if group else None, n_groups, p(si), p(sd),
                                          p(np.zeros((max(n_groups, 1), 26), dtype=np.int64)), p(np.zeros((max(n_groups, 1), 2))))
    cars = [p(np.zeros((max(Bn, 1), max(V, 1)))) if car else None for _ in range(3)]
    return lib.crx_race_stats(ctypes.byref(d), Bn, 0, 0.0, p(np.zeros((max(Bn, 1), 6))), p(np.zeros(max(Bn, 1), dtype=np.int32)), *cars,
                              p(np.zeros(max(Bn, 1), dtype=np.int32)) if n_opp else None, p(np.zeros((max(Bn, 1), 2))) if dims else None,
                              None, None, p(si), p(sd))


def test_argument_refusals(lib):
    """Every rule of the family's argument check, through the host-pointer entries; each is refused with CRX_ERR_ARG whether or not the
    library has a device (the check comes before CRX_ERR_NOT_INIT), and the well-formed call next to it is not."""
    from crx import abi

    good = abi.stats_desc(3, 0, 19.25, 1.0)
    assert _host_call(lib, good, 4) != ERR_ARG
    # a bad descriptor
    for kw in (dict(n_opp_max=-1), dict(n_opp_max=33), dict(n_cars=8), dict(n_cars=-1), dict(degree=5), dict(degree=10), dict(lap_length=0.0),
               dict(lap_length=float("nan")), dict(track_width=-1.0), dict(track_width=float("nan")), dict(l_sum=0.0), dict(w_sum=float("inf"))):
        d = abi.stats_desc(3, 0, 19.25, 1.0)
        for k, v in kw.items():
            setattr(d, k, v)
        assert _host_call(lib, d, 4) == ERR_ARG, kw
        assert lib.crx_last_error()
    assert _host_call(lib, abi.stats_desc(1, 3, 19.25, 1.0), 6, car=False) == ERR_ARG        # field mode: fewer slots than opponents
    assert lib.crx_race_stats(None, 0, 0, 0.0, *([None] * 11)) == ERR_ARG
    assert _host_call(lib, good, -1) == ERR_ARG
    # scripted arrays in field mode, or the other way round
    field = abi.stats_desc(2, 3, 19.25, 1.0)
    assert _host_call(lib, field, 6, car=False) != ERR_ARG and _host_call(lib, field, 6, car=False, dims=True) != ERR_ARG
    assert _host_call(lib, field, 6, car=True) == ERR_ARG
    assert _host_call(lib, field, 6, car=False, n_opp=True) == ERR_ARG
    assert _host_call(lib, good, 4, dims=True) == ERR_ARG
    # scripted mode with opponents but without the three car arrays; with none it is a car on its own
    assert _host_call(lib, good, 4, car=False) == ERR_ARG
    assert _host_call(lib, abi.stats_desc(0, 0, 19.25, 1.0), 4, car=False) != ERR_ARG
    # field mode: whole races only
    assert _host_call(lib, field, 7, car=False) == ERR_ARG
    # a group without n_groups >= 1
    assert _host_call(lib, good, 4, entry="race_stats_summary", group=True, n_groups=0) == ERR_ARG
    assert _host_call(lib, good, 4, entry="race_stats_summary", group=True, n_groups=2) != ERR_ARG
    assert _host_call(lib, good, 4, entry="race_stats_summary") != ERR_ARG
    # NULL state
    assert lib.crx_race_stats_reset(ctypes.byref(good), 4, np.zeros(4, dtype=np.int32).ctypes.data_as(ctypes.c_void_p), None, None) == ERR_ARG


@pytest.fixture
def rec(monkeypatch):
    from crx import montecarlo

    r = Recorder()
    monkeypatch.setattr(montecarlo, "torch_api", r)
    return r


def _check_stats_call(st, call, xc, laps, sample):
    assert call["desc"] is st.desc and call["ws"] is st.ws and call["sample"] == sample
    assert call["xcurv"] is xc and call["laps"] is laps


def test_race_stats_sequence_mpccbf(rec, AB):
    from crx import montecarlo

    r = _races(AB)
    rec.take()
    st = montecarlo.RaceStats(r)
    names, args = rec.take()
    assert names == ["race_stats_reset_dev"] and args["race_stats_reset_dev"]["laps"] is r.laps
    assert (st.desc.n_opp_max, st.desc.n_cars, st.desc.lap_length, st.desc.track_width) == (2, 0, LAP, WIDTH)
    st.update()
    names, args = rec.take()
    assert names == ["race_stats_dev"] and args["race_stats_dev"]["t"] == 0.0
    _check_stats_call(st, args["race_stats_dev"], r.xc, r.laps, 0)
    for k in range(2):
        st.step()
        names, args = rec.take()
        assert names == ["cbf_prep_dev", "cbf_solve_dev", "plant_step_wrap_dev", "race_stats_dev"]
        call = args["race_stats_dev"]
        _check_stats_call(st, call, r.xc, r.laps, k + 1)
        assert call["xcurv"] is args["plant_step_wrap_dev"]["xcurv_next"]          # the state after the step ...
        assert call["t"] == r.t and call["t"] > 0.0                                # ... against the scripted cars at the clock after it
        assert call["car_s0"] is r.s0 and call["car_v"] is r.v and call["car_ey"] is r.ey and call["xt"] is r.xt
        assert call["car_dims"] is None and call["flag"] is None and call["n_opp"] is None
    r.step()                                                                       # the loop alone: exactly what it launched before
    assert rec.take()[0] == ["cbf_prep_dev", "cbf_solve_dev", "plant_step_wrap_dev"]


def test_race_stats_sequence_field(rec, AB):
    from crx import montecarlo

    z = np.zeros((6, 6))
    dims = np.full((2, 3, 2), 0.3)
    r = montecarlo.FieldRaces(TAB, LAP, WIDTH, AB[0], AB[1], z, z, 3, device="cpu", car_dims=dims)
    rec.take()
    st = montecarlo.RaceStats(r)
    assert rec.take()[0] == ["race_stats_reset_dev"]
    assert (st.desc.n_opp_max, st.desc.n_cars) == (2, 3)
    st.step()
    names, args = rec.take()
    assert names == ["field_prep_dev", "cbf_solve_dev", "plant_step_wrap_dev", "race_stats_dev"]
    call = args["race_stats_dev"]
    _check_stats_call(st, call, r.xc, r.laps, 0)
    assert call["xcurv"] is args["plant_step_wrap_dev"]["xcurv_next"] and call["car_dims"] is r.car_dims
    assert call["car_s0"] is None and call["car_v"] is None and call["car_ey"] is None and call["xt"] is r.xt


@pytest.mark.parametrize("planner", ["traj", "path"])
def test_race_stats_sequence_game(rec, AB, planner):
    from crx import montecarlo

    g = _game(AB, planner)
    rec.take()
    st = montecarlo.RaceStats(g, group=np.array([0, 1, 1]), n_groups=2)
    assert rec.take()[0] == ["race_stats_reset_dev"]
    assert st.desc.n_opp_max == 3 and st.desc.n_cars == 0 and st.group.dtype == torch.int32
    st.update()
    rec.take()
    for k in range(2):
        st.step()
        names, args = rec.take()
        assert names == _game_step(planner) + ["race_stats_dev"]
        call = args["race_stats_dev"]
        _check_stats_call(st, call, g.lm.xc, g.lm.laps, k + 1)
        assert call["xcurv"] is args["plant_step_wrap_dev"]["xcurv_next"] and call["t"] == g.t
        assert call["flag"] is g.m_ot and call["car_s0"] is g.s0 and call["xt"] is None
    g.step()
    assert rec.take()[0] == _game_step(planner)


def test_every_loop_answers_stats_inputs(rec, AB):
    from crx import montecarlo
    from test_montecarlo_sequence_cpu import _lmpc

    z = np.zeros((BN, 6))
    loops = [_races(AB), _lmpc(), _game(AB, "traj"), montecarlo.FieldRaces(TAB, LAP, WIDTH, AB[0], AB[1], z, z, 3, device="cpu"),
             montecarlo.IlqrRaces(TAB, LAP, AB[0], AB[1], z, z, np.full(BN, 3.0), np.full(BN, 0.2), np.zeros(BN), N=12, device="cpu"),
             montecarlo.PidLaps(TAB, LAP, z, z, 4, device="cpu"), montecarlo.LqrLaps(TAB, LAP, z, z, AB[0], AB[1], device="cpu")]
    for loop in loops:
        inp = loop.stats_inputs()
        assert tuple(inp["xcurv"].shape) == (BN, 6) and inp["laps"].dtype == torch.int32 and inp["lap_length"] == LAP, type(loop).__name__
        st = montecarlo.RaceStats(loop, track_width=0.7)
        assert st.desc.track_width == 0.7 and st.ws.stat_i.shape == (19, BN) and st.ws.stat_d.shape == (4 + st.desc.n_opp_max, BN)
        assert st.ws.lap_step.shape == (8, BN) and st.ws.ds_prev.shape == (st.desc.n_opp_max, BN)
        assert st.ws.min_clear.data_ptr() == st.ws.stat_d.data_ptr() and st.ws.passes.data_ptr() == st.ws.stat_i[16].data_ptr()
    assert montecarlo.RaceStats(loops[4]).desc.track_width == float("inf")
