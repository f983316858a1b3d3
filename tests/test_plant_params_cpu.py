"""One BicycleDynamicsParam set per car, the parts that need no GPU: (1) the oracle -- and the host mirror -- reproduce the reference's own
vehicle_dynamics on NON-default parameters (tests/golden/plant_params.npz, tests/golden/tools/make_plant_params.py), which makes
"the oracle at batch 1 with the descriptor's ten fields set to row b" the per-car reference of tests/test_gpu_plant_params.py; (2)
abi.plant_params; (3) every closed loop of crx.montecarlo hands its plant_params to the plant launch and launches what it launched
before."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import conftest
import plant_params_ref as ref
from test_montecarlo_sequence_cpu import BN, LAP, N_LMPC, TAB, WIDTH, Recorder, _cars, _lmpc_inputs

from crx import abi, montecarlo, synth


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(conftest.GOLDEN, "plant_params.npz"))


# ---- 1. the oracle on non-default parameters ---------------------------------------------------------------------------------------
def test_fixture_covers_the_parameter_space(G):
    P = np.vstack([G["step/params"], G["pid/params"][None]])
    f = P / abi.plant_params(1)[0]
    assert P.shape == (41, 10) and (f >= 0.7).all() and (f <= 1.3).all() and f.min() < 0.75 and f.max() > 1.25
    for a, b in ((1, 2), (4, 7), (5, 8), (6, 9)):   # lf / lr, Df / Dr, Cf / Cr, Bf / Br
        assert (P[:, a] != P[:, b]).all()


def test_oracle_single_steps(orc, G):
    """40 single Euler steps, each on its own parameter set, one segment carrying the recorded curvature: the bound of
    test_oracle_golden.test_plant_step."""
    worst = 0.0
    for i in range(G["step/u"].shape[0]):
        d = ref.desc_with(abi.plant_desc(1, 1e9, timestep=0.001), G["step/params"][i])
        tr = np.array([[0, 0, 0, -1e9, 3e9, G["step/curv"][i]]])
        r = orc.plant_step(d, tr, G["step/xglob"][i:i + 1], G["step/xcurv"][i:i + 1], G["step/u"][i:i + 1])
        worst = max(worst, np.abs(r["xglob"][0] - G["step/xglob_next"][i]).max(), np.abs(r["xcurv"][0] - G["step/xcurv_next"][i]).max())
        np.testing.assert_allclose(r["xglob"][0], G["step/xglob_next"][i], rtol=0, atol=1e-15)
        np.testing.assert_allclose(r["xcurv"][0], G["step/xcurv_next"][i], rtol=0, atol=1e-15)
    print("oracle, 40 single steps on non-default parameters: worst deviation %.3g" % worst)


def test_oracle_pid_loop(orc, G):
    from control import control

    tr = ref.track(0.8)
    d = ref.desc_with(abi.plant_desc(tr.point_and_tangent.shape[0], tr.lap_length), G["pid/params"])
    assert d.n_sub == 100
    xg, xc = np.zeros((1, 6)), np.zeros((1, 6))
    worst = 0.0
    for k in range(G["pid/xcurv_log"].shape[0]):
        u = control.pid(xc[0], np.array([0.8, 0, 0, 0, 0, 0.0]))
        r = orc.plant_step(d, tr.point_and_tangent, xg, xc, u[None])
        xg, xc = r["xglob"], r["xcurv"]
        worst = max(worst, np.abs(xc[0] - G["pid/xcurv_log"][k]).max(), np.abs(xg[0] - G["pid/xglob_log"][k]).max())
        np.testing.assert_allclose(xc[0], G["pid/xcurv_log"][k], rtol=0, atol=1e-13)
        np.testing.assert_allclose(xg[0], G["pid/xglob_log"][k], rtol=0, atol=1e-13)
    print("oracle, 30-step PID loop on a non-default car: worst deviation %.3g" % worst)
    # the per-car helper the GPU tests use says the same
    og, oc = ref.oracle_cars(orc, abi.plant_desc(tr.point_and_tangent.shape[0], tr.lap_length), tr.point_and_tangent, np.zeros((1, 6)),
                             np.zeros((1, 6)), control.pid(np.zeros(6), np.array([0.8, 0, 0, 0, 0, 0.0]))[None], G["pid/params"][None])
    np.testing.assert_allclose(oc[0], G["pid/xcurv_log"][0], rtol=0, atol=1e-13)
    ogz, ocz = ref.oracle_cars(orc, abi.plant_desc(tr.point_and_tangent.shape[0], tr.lap_length), tr.point_and_tangent, np.zeros((1, 6)),
                               np.zeros((1, 6)), control.pid(np.zeros(6), np.array([0.8, 0, 0, 0, 0, 0.0]))[None], G["pid/params"][None],
                               z=np.zeros((1, 3)))
    assert np.array_equal(ocz, oc) and np.array_equal(ogz, og)          # zero draws = the plain step


def test_mirror_single_steps(G):
    """system.vehicle_dynamics honours its first argument (the mirror's simulator, like the reference's, never passes anything but the
    defaults)."""
    from system import vehicle_dynamics as vd

    class Par:
        def __init__(self, row):
            self.row = row

        def get_params(self):
            return tuple(float(v) for v in self.row)

    for i in range(G["step/u"].shape[0]):
        g, c = vd.vehicle_dynamics(Par(G["step/params"][i]), G["step/curv"][i], G["step/xglob"][i], G["step/xcurv"][i], 0.001, G["step/u"][i])
        np.testing.assert_allclose(g, G["step/xglob_next"][i], rtol=0, atol=1e-15)
        np.testing.assert_allclose(c, G["step/xcurv_next"][i], rtol=0, atol=1e-15)


def test_noisy_case_has_no_car_on_the_line(orc):
    """The inputs of the GPU suite's noise / wrap test (plant_params_ref.noisy_case): the oracle alone puts no car within 1e-9 of the lap
    length (where the GPU's last-place differences could flip the wrap), and the wrap does act."""
    tr = ref.track()
    tab, L = tr.point_and_tangent, tr.lap_length
    B = 300
    xc, xg, U, z, near = ref.noisy_case(B, L)
    P = synth.fleet_plant_params(B, 0.3, ref.NOISY_SEED)
    _, oc = ref.oracle_cars(orc, abi.plant_desc(tab.shape[0], L), tab, xg, xc, np.ascontiguousarray(U[:, 0, :]), P, z)
    assert (np.abs(oc[:, 4] - L) > 1e-9).all()
    _, crossed = ref.wrap(oc, L)
    assert near.sum() == 100 and 20 <= crossed.sum() <= 80 and not crossed[~near].any()
    clipped = np.abs(z * np.array([0.01, 0.01, 0.005])) > np.array([0.05, 0.1, 0.05])
    assert clipped[:, 0].any() and clipped[:, 1].any() and clipped[:, 2].any() and (~clipped).all(axis=1).sum() >= 100


# ---- 2. abi.plant_params ------------------------------------------------------------------------------------------------------------
def test_plant_params_defaults_are_the_descriptor():
    import crx

    d = abi.PlantDesc()
    crx.lib().crx_plant_desc_default(C.byref(d), C.c_int(7), C.c_double(19.0))
    P = abi.plant_params(3)
    assert P.shape == (3, abi.CRX_PLANT_NPARAM) and P.dtype == np.float64 and P.flags["C_CONTIGUOUS"]
    for b in range(3):
        assert P[b].tobytes() == ref.desc_row(d).tobytes()
    assert ref.desc_row(abi.plant_desc(7, 19.0)).tobytes() == P[0].tobytes()
    assert synth.fleet_plant_params(5, 0.0, 3).tobytes() == abi.plant_params(5).tobytes()


def test_plant_params_order_and_shapes():
    from utils import base

    class Par:
        def __init__(self, k):
            self.k = k

        def get_params(self):
            return tuple(10.0 * self.k + i for i in range(10))   # m = 10 k, lf = 10 k + 1, ... Br = 10 k + 9

    one = abi.plant_params(4, Par(2))
    assert np.array_equal(one, np.tile(20.0 + np.arange(10), (4, 1)))
    many = abi.plant_params(3, [Par(0), Par(1), Par(2)])
    assert np.array_equal(many, 10.0 * np.arange(3)[:, None] + np.arange(10)[None, :])
    # the mirror's own parameter class: get_params() order is the descriptor's field order
    dyn = base.CarParam().dynamics_param
    assert abi.plant_params(2, dyn).tobytes() == abi.plant_params(2).tobytes()
    assert tuple(n for n, _ in abi.PlantDesc._fields_[4:]) == abi.PLANT_PARAM_NAMES == ref.NAMES
    with pytest.raises(ValueError):
        abi.plant_params(3, [Par(0), Par(1)])
    with pytest.raises(ValueError):
        abi.plant_params(1, [Par(0), Par(1)])


def test_fleet_plant_params():
    P = synth.fleet_plant_params(200, 0.3, 4)
    f = P / abi.plant_params(1)[0]
    assert P.shape == (200, 10) and (f > 0.7).all() and (f < 1.3).all() and f.min() < 0.71 and f.max() > 1.29
    assert abs(np.corrcoef(f[:, 1], f[:, 2])[0, 1]) < 0.25                  # independent per entry (lf, lr)
    assert np.array_equal(P, synth.fleet_plant_params(200, 0.3, 4)) and not np.array_equal(P, synth.fleet_plant_params(200, 0.3, 5))


# ---- 3. launch sequences --------------------------------------------------------------------------------------------------------------
@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(montecarlo, "torch_api", r)
    return r


def _build(kind, AB, **kw):
    z = np.zeros((BN, 6))
    if kind == "mpccbf":
        return montecarlo.MpccbfRaces(TAB, LAP, WIDTH, AB[0], AB[1], z, z, *_cars(2), device="cpu", **kw)
    if kind == "ilqr":
        return montecarlo.IlqrRaces(TAB, LAP, AB[0], AB[1], z, z, np.full(BN, 3.0), np.full(BN, 0.2), np.zeros(BN), N=12, device="cpu", **kw)
    if kind == "lmpc":
        return montecarlo.LmpcLaps(TAB, LAP, WIDTH, *_lmpc_inputs(), N=N_LMPC, device="cpu", **kw)
    if kind == "game":
        g = montecarlo.GameLaps(TAB, LAP, WIDTH, AB[0], AB[1], np.zeros((7, 6)), *_lmpc_inputs(), *_cars(3), N=N_LMPC, device="cpu", **kw)
        g.overlap = False
        return g
    if kind == "pid":
        return montecarlo.PidLaps(TAB, LAP, z, z, 4, device="cpu", **kw)
    assert kind == "lqr"
    return montecarlo.LqrLaps(TAB, LAP, z, z, AB[0], AB[1], device="cpu", **kw)


@pytest.mark.parametrize("kind", ["mpccbf", "ilqr", "lmpc", "game", "pid", "lqr"])
@pytest.mark.parametrize("as_tensor", [False, True])
def test_loops_hand_plant_params_to_the_plant(rec, AB, kind, as_tensor):
    P = synth.fleet_plant_params(BN, 0.3, 1)
    plain = _build(kind, AB)
    built_plain = rec.take()[0]
    plain.step()
    names_plain, args_plain = rec.take()
    assert args_plain["plant_step_wrap_dev"]["params"] is None
    assert (plain.lm if kind == "game" else plain).plant_params is None
    loop = _build(kind, AB, plant_params=torch.as_tensor(P) if as_tensor else P)
    assert rec.take()[0] == built_plain
    holder = loop.lm if kind == "game" else loop          # GameLaps hands it to its inner LmpcLaps, which holds the plant
    assert torch.is_tensor(holder.plant_params) and holder.plant_params.dtype == torch.float64 and holder.plant_params.is_contiguous()
    assert np.array_equal(holder.plant_params.numpy(), P)
    for _ in range(2):
        loop.step()
        names, args = rec.take()
        assert names == names_plain
        assert args["plant_step_wrap_dev"]["params"] is holder.plant_params
        assert args["plant_step_wrap_dev"]["desc"] is holder.plant
    if kind == "mpccbf":
        loop.step_glue()
        assert rec.take()[1]["plant_step_dev"]["params"] is loop.plant_params
        plain.step_glue()
        assert rec.take()[1]["plant_step_dev"]["params"] is None


def test_plant_params_shape_is_checked(rec, AB):
    with pytest.raises(ValueError):
        _build("lqr", AB, plant_params=np.ones((BN + 1, 10)))
    with pytest.raises(ValueError):
        _build("pid", AB, plant_params=np.ones((BN, 9)))


def test_run_functions_take_plant_params(rec, AB):
    P = synth.fleet_plant_params(BN, 0.3, 2)
    z, cars = np.zeros((BN, 6)), _cars(2)

    def plant_params_seen():
        seen = [a["params"] for n, a in rec.calls if n == "plant_step_wrap_dev"]
        rec.take()
        return seen

    montecarlo.mpccbf_races(TAB, LAP, WIDTH, AB[0], AB[1], z, z, *cars, 2, device="cpu", plant_params=P)
    montecarlo.ilqr_races(TAB, LAP, AB[0], AB[1], z, z, np.full(BN, 3.0), np.full(BN, 0.2), np.zeros(BN), 2, N=12, device="cpu", plant_params=P)
    montecarlo.lqr_laps(TAB, LAP, z, z, 2, AB[0], AB[1], device="cpu", plant_params=P)
    montecarlo.lmpc_laps(TAB, LAP, WIDTH, *_lmpc_inputs(), 2, N=N_LMPC, device="cpu", plant_params=P)
    montecarlo.game_laps(TAB, LAP, WIDTH, AB[0], AB[1], np.zeros((7, 6)), *_lmpc_inputs(), *_cars(3), 2, device="cpu", plant_params=P)
    montecarlo.pid_laps(TAB, LAP, z, z, 2, device="cpu", plant_params=P)
    seen = plant_params_seen()
    assert len(seen) == 12 and all(s is not None and np.array_equal(s.numpy(), P) for s in seen)
