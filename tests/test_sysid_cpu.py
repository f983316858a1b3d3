"""System identification without a GPU: the mirror's system_identification module and PID simulation against the reference's
own identification experiment (tests/golden/sysid.npz, recorded by tests/golden/tools/make_sysid.py), and the C ABI of
crx_sysid_fit."""
import ctypes
import os

import numpy as np
import pytest

import conftest


@pytest.fixture(scope="module")
def S():
    return np.load(os.path.join(conftest.GOLDEN, "sysid.npz"))


@pytest.fixture(scope="module")
def lib():
    import crx

    if not os.path.exists(crx.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return crx.lib()


def mirror_run(S, name, monkeypatch):
    """The mirror's simulation of the recorded scenario, its plant noise fed the recorded draws in call order."""
    from racing import offboard
    from utils import base, racing_env

    draws = iter(S[name + "/z"].reshape(-1).tolist())
    monkeypatch.setattr(np.random, "randn", lambda: next(draws))
    track = racing_env.ClosedTrack(S["track_spec"], track_width=1.0)
    x0 = S[name + "/x0"]
    ego = offboard.DynamicBicycleModel(name="ego", param=base.CarParam(edgecolor="black"))
    ego.set_state_curvilinear(x0.copy())
    ego.set_state_global(x0.copy())
    ego.set_ctrl_policy(offboard.PIDTracking(vt=float(S[name + "/vt"])))
    ego.ctrl_policy.set_timestep(float(S[name + "/dt"]))
    ego.set_track(track)
    sim = offboard.CarRacingSim()
    sim.set_timestep(float(S[name + "/dt"]))
    sim.set_track(track)
    sim.add_vehicle(ego)
    ego.ctrl_policy.set_racing_sim(sim)
    sim.sim(sim_time=int(S[name + "/steps"]) * float(S[name + "/dt"]))
    assert next(draws, None) is None   # every recorded draw taken, none missing
    return ego


@pytest.mark.parametrize("name", ["long", "short"])
def test_mirror_simulation_retraces_reference(S, name, monkeypatch):
    from system import system_identification

    ego = mirror_run(S, name, monkeypatch)
    x = np.stack(ego.xcurv_log, axis=0)
    assert x.shape == S[name + "/x"].shape
    assert np.abs(x - S[name + "/x"]).max() <= 1e-12
    assert ego.laps == int(S[name + "/laps"])
    u = system_identification.get_udata(ego)
    assert np.abs(u - S[name + "/u"]).max() <= 1e-12


@pytest.mark.parametrize("name", ["long", "short"])
def test_mirror_regression_matches_reference(S, name):
    from system import system_identification

    A, B, err = system_identification.linear_regression(S[name + "/x"], S[name + "/u"], float(S[name + "/lamb"]))
    W = max(np.abs(S[name + "/A"]).max(), np.abs(S[name + "/B"]).max())
    assert np.abs(A - S[name + "/A"]).max() <= 1e-12 * W
    assert np.abs(B - S[name + "/B"]).max() <= 1e-12 * W
    assert np.abs(err - S[name + "/err"]).max() <= 1e-12
    # S2: the lap wraps stay in the data -- the s column's largest residual is a lap jump
    assert S[name + "/err"][0, 4] > 0.9 * float(S[name + "/lap_length"]) or int(S[name + "/laps"]) < 2


def test_udata_is_the_step_inputs(S):
    """S5 on the recorded run: get_udata's rows are the PID inputs of the states before each step (u[k] = pid(x[k-1]) for k >= 1)."""
    x, u, vt = S["long/x"], S["long/u"], float(S["long/vt"])
    d = -0.6 * (x[:-1, 5] - 0.0) - 0.9 * x[:-1, 3]
    a = 1.5 * (vt - x[:-1, 0])
    assert np.array_equal(u[1:, 0], d) and np.array_equal(u[1:, 1], a)


def test_sysid_desc_layout_matches_header(lib):
    from crx import abi

    d = abi.SysidDesc()
    lib.crx_sysid_desc_default(ctypes.byref(d))
    assert bytes(d) == bytes(abi.sysid_desc())
    assert ctypes.sizeof(d) == 32 and d.lamb == 1e-9 and d.first_row == 1 and d.chunk_rows == 8192


def test_workspace_bytes(lib):
    from crx import abi

    fn = lib.crx_sysid_workspace_bytes
    fn.restype = ctypes.c_size_t
    d = abi.sysid_desc()
    # 20000 rows -> 19998 pairs -> 3 tiles of 8192 per log
    assert fn(ctypes.byref(d), 3, 2, ctypes.c_int64(20000)) == (3 * 3 * 96 + 2 * 48) * 8 + 512
    assert fn(ctypes.byref(d), 3, 3, ctypes.c_int64(2)) == (3 * 1 * 96 + 3 * 48) * 8 + 512


def test_sysid_fit_refuses_without_gpu(lib, S):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible; the loud-failure path is exercised in the CPU container")
    import crx

    with pytest.raises(crx.CrxUnavailable):
        crx.sysid_fit(S["long/x"], S["long/u"])


def test_sysid_fit_rejects_bad_arguments(lib):
    from crx import abi

    b = abi.Binding(lib, "crx_")
    x, u = np.zeros((10, 6)), np.zeros((10, 2))
    with pytest.raises(RuntimeError, match="chunk_rows"):
        b.sysid_fit(abi.sysid_desc(chunk_rows=100), x, u)
    with pytest.raises(RuntimeError, match="lamb"):
        b.sysid_fit(abi.sysid_desc(lamb=-1.0), x, u)
    with pytest.raises(RuntimeError, match="decreases"):
        b.sysid_fit(abi.sysid_desc(), x, u, offsets=np.array([0, 6, 4, 10]))
    with pytest.raises(RuntimeError, match="group_offset"):
        b.sysid_fit(abi.sysid_desc(), x, u, offsets=np.array([0, 5, 10]), group_offsets=np.array([0, 1]))
    d = abi.sysid_desc()
    assert lib.crx_sysid_fit(None, 1, *([None] * 10)) == -1
    assert lib.crx_sysid_fit(ctypes.byref(d), 2, None, None, 1, *([None] * 7)) == -1   # NULL groups need n_groups == n_logs
    assert b"n_groups" in lib.crx_last_error()
