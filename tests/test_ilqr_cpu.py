"""iLQR / LQR without a GPU: the numpy model against the reference's own answers (tests/golden/ilqr.npz, recorded by
tests/golden/tools/make_ilqr.py), the C ABI of crx_ilqr_solve, and the host-side LQR mirror against the reference."""
import ctypes
import os
import pickle

import numpy as np
import pytest

import conftest
import ilqr_model

Q_DEF = np.diag([10.0, 0.0, 0.0, 4.0, 0.0, 40.0])
R_DEF = np.diag([0.1, 0.1])


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(conftest.GOLDEN, "ilqr.npz"))


@pytest.fixture(scope="module")
def LQ():
    return np.load(os.path.join(conftest.GOLDEN, "closed_loop_lqr.npz"))


@pytest.fixture(scope="module")
def lib():
    import crx

    if not os.path.exists(crx.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return crx.lib()


def _case(G, i, AB, record=None):
    A, B = AB
    N = int(G["N"][i])
    return ilqr_model.solve(A, B, Q_DEF, R_DEF, G["x0"][i][None], G["xt"][i][None], G["obs_s"][i][None, None, :N + 1],
                            G["obs_ey"][i][None, None, :N + 1], [[G["lap_off"][i]]], [1], N, max_iter=int(G["max_iter"][i]),
                            l_sum=float(G["l_sum"][i]), w_sum=float(G["w_sum"][i]), record=record)


def test_fixture_covers_every_stop(G):
    stops = G["stop"]
    for s in (ilqr_model.CONVERGED, ilqr_model.MAX_ITER, ilqr_model.STALLED):
        assert (stops == s).sum() >= 5, s
    assert G["two_cars"].any() and (G["lap_off"] != 0).any() and set(G["N"]) == {10, 20, 50}


def test_model_reproduces_reference_cases(G, AB):
    full = {int(c) for c, _ in G["full/case"]}
    for i in range(len(G["u0"])):
        r = _case(G, i, AB, record=0 if i in full else None)
        u0 = G["u0"][i]
        assert np.abs(r["U"][0, 0] - u0).max() <= 1e-12 * max(1.0, np.abs(u0).max()), i
        assert r["iters"][0] == G["iters"][i], i
        assert r["status"][0] == G["stop"][i], i
        if i in full:
            rows = np.flatnonzero(G["full/case"][:, 0] == i)
            assert len(r["iterates"]) == len(rows), i
            N = int(G["N"][i])
            for (U, X), j in zip(r["iterates"], rows):
                np.testing.assert_allclose(U, G["full/U"][j][:N], rtol=1e-12, atol=1e-12)
                np.testing.assert_allclose(X, G["full/X"][j][:N + 1], rtol=1e-12, atol=1e-12)


def test_lap_offset_truncates_toward_zero():
    L = 10.0
    assert ilqr_model.lap_offset(25.0, 9.0, L) == 20.0
    assert ilqr_model.lap_offset(5.0, -3.0, L) == 0.0      # int(-0.3) == 0
    assert ilqr_model.lap_offset(11.0, 9.5, L) == 10.0


def test_ilqr_desc_layout_matches_header(lib, AB):
    from crx import abi

    A = np.arange(36, dtype=float)
    B = np.arange(12, dtype=float) + 100
    d = abi.IlqrDesc()
    lib.crx_ilqr_desc_default(ctypes.byref(d), 50, A.ctypes.data_as(ctypes.c_void_p), B.ctypes.data_as(ctypes.c_void_p))
    assert bytes(d) == bytes(abi.ilqr_desc(50, A, B))
    assert d.N == 50 and d.max_iter == 150 and d.lamb_max == 1000.0 and d.R[3] == 0.1 and d.Q[35] == 40.0


def _args(N=10, V=1, Bn=2):
    return (np.zeros((Bn, 6)), np.zeros((Bn, 6)), np.zeros((Bn, V, N + 1)), np.zeros((Bn, V, N + 1)), np.zeros((Bn, V)),
            np.ones(Bn, dtype=np.int32))


def test_ilqr_solve_refuses_without_gpu(lib, AB):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible; the loud-failure path is exercised in the CPU container")
    import crx
    from crx import abi

    b = abi.Binding(lib, "crx_")
    d = abi.ilqr_desc(10, *AB)
    with pytest.raises(RuntimeError, match="crx_init"):
        b.ilqr_solve(d, *_args())
    from control import control
    from utils import base

    with pytest.raises((crx.CrxUnavailable, RuntimeError)):
        control.ilqr(np.zeros(6), np.array([0.8, 0, 0, 0, 0, 0.0]), base.iLQRRacingParam(),
                     {"ego": type("V", (), {"param": base.CarParam()})()}, "ego", 19.2, 0.0, 0.1, None, None)


def test_ilqr_solve_rejects_bad_arguments(lib, AB):
    from crx import abi

    b = abi.Binding(lib, "crx_")
    with pytest.raises(RuntimeError, match="N=65"):
        b.ilqr_solve(abi.ilqr_desc(65, *AB), *_args(N=65))
    with pytest.raises(RuntimeError, match="N=0"):
        b.ilqr_solve(abi.ilqr_desc(0, *AB), *_args(N=0))
    with pytest.raises(RuntimeError, match="n_obs_max=7"):
        b.ilqr_solve(abi.ilqr_desc(10, *AB, n_obs_max=7), *_args(V=7))
    with pytest.raises(RuntimeError, match=r"n_obs\[1\]=2"):
        b.ilqr_solve(abi.ilqr_desc(10, *AB), *_args()[:5], np.array([1, 2], dtype=np.int32))
    d = abi.ilqr_desc(10, *AB)
    x0, xt, os_, oe, lo, n = _args()
    out = [np.zeros((2, 11, 6)), np.zeros((2, 10, 2)), np.zeros(2), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for hole in range(len(out) + 6):
        ins = [p(a) for a in (x0, xt, os_, oe, lo, n)] + [p(a) for a in out]
        ins[hole] = None
        assert lib.crx_ilqr_solve(ctypes.byref(d), 2, *ins) == -1, hole   # CRX_ERR_ARG, before any device check
        assert b"NULL" in lib.crx_last_error()
    assert lib.crx_ilqr_solve(None, 2, *([None] * 11)) == -1


def test_lqr_single_calls_match_reference(LQ, AB):
    from control import control
    from utils import base

    A, B = AB
    for i in range(len(LQ["calls_u"])):
        par = base.LQRTrackingParam(matrix_A=A, matrix_B=B, matrix_Q=LQ["calls_Q"][i], matrix_R=LQ["calls_R"][i],
                                    vt=float(LQ["calls_xt"][i][0]), max_iter=int(LQ["calls_max_iter"][i]))
        u = control.lqr(LQ["calls_x"][i], LQ["calls_xt"][i].reshape(6, 1), par)
        np.testing.assert_allclose(u, LQ["calls_u"][i], rtol=1e-12, atol=1e-12)


def test_lqr_gain_uses_previous_iterate_on_break(AB):
    """Quirk L1: the iterate that passes the stopping test is discarded."""
    from control import control

    A, B = AB
    K1 = control._lqr_gain(A, B, Q_DEF, R_DEF, 1)
    # one iteration without a break: P <- the first Riccati step; with max_iter = 0 the gain is built from Q itself
    K0 = control._lqr_gain(A, B, Q_DEF, R_DEF, 0)
    import scipy.linalg as la

    assert np.array_equal(K0, la.inv(B.T @ Q_DEF @ B + R_DEF) @ B.T @ Q_DEF @ A)
    assert not np.array_equal(K0, K1)
    # the converged gain equals the gain from the previous iterate, which differs from the one the last step produced
    Kc = control._lqr_gain(A, B, Q_DEF, R_DEF, 50)
    P = Q_DEF
    while True:
        PB = P @ B
        nxt = A.T @ P @ A - A.T @ PB @ la.inv(R_DEF + B.T @ PB) @ B.T @ P @ A + Q_DEF
        if np.abs(nxt - P).max() < 0.01:
            break
        P = nxt
    assert np.array_equal(Kc, la.inv(B.T @ P @ B + R_DEF) @ B.T @ P @ A)
    assert not np.array_equal(Kc, la.inv(B.T @ nxt @ B + R_DEF) @ B.T @ nxt @ A)


def test_lqr_closed_loop_matches_reference(LQ):
    """control_test.py --ctrl-policy lqr --track-layout l_shape (zero noise), all 900 steps; the plant is host-side."""
    import scenarios
    from racing import offboard
    from utils import base

    race = scenarios.Race(scenarios.make_track("l_shape", 0.8), 0.1)
    race.policy(offboard.LQRTracking(base.LQRTrackingParam(vt=0.8), race.ego.system_param))
    race.run(float(LQ["steps"]) * 0.1)
    xc = np.array(race.ego.xcurv_log)
    assert xc.shape == LQ["ego_xcurv"].shape
    np.testing.assert_allclose(xc, LQ["ego_xcurv"], rtol=0, atol=1e-8)
    np.testing.assert_allclose(np.array(race.ego.xglob_log), LQ["ego_xglob"], rtol=0, atol=1e-8)


def test_controller_objects_pickle():
    from racing import offboard
    from utils import base

    for ctrl in (offboard.LQRTracking(base.LQRTrackingParam(vt=0.8), base.SystemParam()),
                 offboard.iLQRRacing(base.iLQRRacingParam(vt=0.8), base.SystemParam())):
        back = pickle.loads(pickle.dumps(ctrl, protocol=pickle.HIGHEST_PROTOCOL))
        assert type(back) is type(ctrl) and back.vt == 0.8
    p = base.iLQRRacingParam()
    assert (p.num_horizon, p.max_iter) == (50, 150) and base.LQRTrackingParam().max_iter == 50
    np.testing.assert_array_equal(p.matrix_Q, Q_DEF)
    np.testing.assert_array_equal(p.matrix_R, R_DEF)
