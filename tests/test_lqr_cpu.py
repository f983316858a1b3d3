"""Batched LQR design and per-problem iLQR models without a GPU: the numpy model (tests/lqr_model.py) against the reference's own
answers (tests/golden/closed_loop_lqr.npz) and the host mirror, its float64 noise floor against extended precision, and the C ABI
of crx_lqr_design / crx_lqr_step_dev / crx_ilqr_solve_models."""
import ctypes
import os

import numpy as np
import pytest

import conftest
import lqr_model

Q_DEF = np.diag([10.0, 0.0, 0.0, 4.0, 0.0, 40.0])
R_DEF = np.diag([0.1, 0.1])
CRX_ERR_ARG = -1
NEW_SYMBOLS = ("crx_lqr_desc_default", "crx_lqr_design", "crx_lqr_design_dev", "crx_lqr_step_dev", "crx_ilqr_solve_models",
               "crx_ilqr_solve_models_dev")


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


def test_model_reproduces_reference_calls(LQ, AB):
    A, B = AB
    for i in range(len(LQ["calls_u"])):
        m = lqr_model.design(A, B, LQ["calls_Q"][i], LQ["calls_R"][i], int(LQ["calls_max_iter"][i]))
        assert m["status"][0] in (lqr_model.CONVERGED, lqr_model.MAX_ITER), i
        u = lqr_model.step(m["K"], LQ["calls_x"][i][None], LQ["calls_xt"][i][None])[0]
        np.testing.assert_allclose(u, LQ["calls_u"][i], rtol=1e-12, atol=1e-12, err_msg=str(i))


def test_model_is_the_mirror_bit_for_bit(LQ, AB):
    from control import control

    A, B = AB
    for i in range(len(LQ["calls_u"])):
        Q, R, it = LQ["calls_Q"][i], LQ["calls_R"][i], int(LQ["calls_max_iter"][i])
        assert np.array_equal(lqr_model.design(A, B, Q, R, it)["K"][0], control._lqr_gain(A, B, Q, R, it)), i
    # L1: max_iter = 0 is the gain of P = Q
    m = lqr_model.design(A, B, Q_DEF, R_DEF, 0)
    assert m["iters"][0] == 0 and np.array_equal(m["P"][0], Q_DEF) and np.array_equal(m["K"][0], control._lqr_gain(A, B, Q_DEF, R_DEF, 0))


def test_model_noise_floor_against_extended_precision(AB):
    """Generator G, 1000 models: float64 and numpy.longdouble take the same stop decisions, far from any tie, and agree to 1e-13."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.fail("numpy.longdouble is no wider than float64 on this platform")
    A, B, _ = lqr_model.draw_models(np.random.default_rng(1), *AB, 1000)
    m = lqr_model.design(A, B, Q_DEF, R_DEF)
    x = lqr_model.design(A, B, Q_DEF, R_DEF, dtype=np.longdouble)
    assert np.array_equal(m["iters"], x["iters"]) and np.array_equal(m["status"], x["status"])
    assert set(m["status"]) == {lqr_model.CONVERGED, lqr_model.MAX_ITER}
    worst = float(np.abs(m["K"] - x["K"]).max() / np.abs(m["K"]).max())
    print("noise floor: max|dK| / max|K| = %.3g, smallest margin %.3g" % (worst, m["margin"].min()))
    assert worst <= 1e-13
    assert m["margin"].min() >= 1e-6
    # the kernel's plain 2x2 inverse in place of LAPACK's: the same decisions, the same floor
    p = lqr_model.design(A, B, Q_DEF, R_DEF, inverse="plain")
    assert np.array_equal(p["iters"], m["iters"]) and np.abs(p["K"] - m["K"]).max() <= 1e-13 * np.abs(m["K"]).max()


def test_model_status_table(AB):
    A0, B0 = AB
    A, B = np.repeat(A0[None], 4, axis=0), np.repeat(B0[None], 4, axis=0)
    A[1, 2, 3] = np.nan
    B[2, 0, 1] = np.inf
    m = lqr_model.design(A, B, Q_DEF, R_DEF)
    assert list(m["status"]) == [lqr_model.MAX_ITER, lqr_model.SINGULAR, lqr_model.SINGULAR, lqr_model.MAX_ITER]
    assert list(m["iters"]) == [50, 0, 0, 50] and np.isnan(m["K"][1:3]).all() and np.isfinite(m["K"][[0, 3]]).all()
    z = lqr_model.design(A0, np.zeros((6, 2)), Q_DEF, np.zeros((2, 2)))
    assert z["status"][0] == lqr_model.SINGULAR and np.isnan(z["K"]).all() and np.isnan(z["P"]).all()


def test_lqr_desc_layout_and_defaults(lib):
    from crx import abi

    d = abi.LqrDesc()
    lib.crx_lqr_desc_default(ctypes.byref(d))
    assert ctypes.sizeof(d) == 8 + 8 * (36 + 4 + 1)
    assert bytes(d) == bytes(abi.lqr_desc())
    assert d.max_iter == 50 and d.eps == 0.01 and d.Q[0] == 10.0 and d.Q[21] == 4.0 and d.Q[35] == 40.0 and d.R[0] == 0.1 and d.R[3] == 0.1
    assert sum(d.Q) == 54.0 and d.R[1] == 0.0 and d.R[2] == 0.0
    c = abi.lqr_desc(Q=[1, 2, 3, 4, 5, 6], R=np.array([[1.0, 2.0], [3.0, 4.0]]), max_iter=7, eps=0.5)
    assert c.Q[7] == 2.0 and c.Q[1] == 0.0 and list(c.R) == [1.0, 2.0, 3.0, 4.0] and c.max_iter == 7 and c.eps == 0.5


def test_new_symbols_exported_and_declared(lib):
    src = open(os.path.join(conftest.ROOT, "include", "crx.h")).read()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n + "(" in src, n
    assert lib.crx_version() == 400


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _holes(args, optional=()):
    """The pointer arguments with every required one NULL in turn."""
    for hole in range(len(args)):
        if hole in optional:
            continue
        a = [_p(x) for x in args]
        a[hole] = None
        yield hole, a


def test_new_entry_points_reject_null_arguments(lib, AB):
    from crx import abi

    Bn = 2
    A, B = np.zeros((Bn, 6, 6)), np.zeros((Bn, 6, 2))
    K, P = np.zeros((Bn, 2, 6)), np.zeros((Bn, 6, 6))
    it, st = np.zeros(Bn, dtype=np.int32), np.zeros(Bn, dtype=np.int32)
    d = abi.lqr_desc()

    def bad(rc):
        assert rc == CRX_ERR_ARG and lib.crx_last_error(), rc

    # crx_lqr_design: P (3) may be NULL
    for hole, a in _holes((A, B, K, P, it, st), optional=(3,)):
        bad(lib.crx_lqr_design(ctypes.byref(d), Bn, *a))
        assert b"NULL" in lib.crx_last_error(), hole
        bad(lib.crx_lqr_design_dev(ctypes.byref(d), Bn, None, *a, None))
        assert b"NULL" in lib.crx_last_error(), hole
    bad(lib.crx_lqr_design(None, Bn, _p(A), _p(B), _p(K), _p(P), _p(it), _p(st)))
    bad(lib.crx_lqr_design_dev(None, Bn, None, _p(A), _p(B), _p(K), _p(P), _p(it), _p(st), None))
    bad(lib.crx_lqr_design(ctypes.byref(d), -1, _p(A), _p(B), _p(K), _p(P), _p(it), _p(st)))
    assert b"batch" in lib.crx_last_error()
    bad(lib.crx_lqr_design(ctypes.byref(abi.lqr_desc(max_iter=-1)), Bn, _p(A), _p(B), _p(K), _p(P), _p(it), _p(st)))
    assert b"max_iter" in lib.crx_last_error()
    # crx_lqr_step_dev
    x, xt, u = np.zeros((Bn, 6)), np.zeros((Bn, 6)), np.zeros((Bn, 2))
    for hole, a in _holes((K, x, xt, u)):
        bad(lib.crx_lqr_step_dev(Bn, *a, None))
        assert b"NULL" in lib.crx_last_error(), hole
    bad(lib.crx_lqr_step_dev(-1, _p(K), _p(x), _p(xt), _p(u), None))
    # crx_ilqr_solve_models / _dev: arguments (x0, model_A, model_B, xt, obs_s, obs_ey, lap_off, n_obs, X, U, cost, status, iters)
    N = 10
    di = abi.ilqr_desc(N, *AB)
    args = (np.zeros((Bn, 6)), A, B, np.zeros((Bn, 6)), np.zeros((Bn, 1, N + 1)), np.zeros((Bn, 1, N + 1)), np.zeros((Bn, 1)),
            np.ones(Bn, dtype=np.int32), np.zeros((Bn, N + 1, 6)), np.zeros((Bn, N, 2)), np.zeros(Bn), st, it)
    for hole, a in _holes(args):
        bad(lib.crx_ilqr_solve_models(ctypes.byref(di), Bn, *a))
        assert b"NULL" in lib.crx_last_error(), hole
        bad(lib.crx_ilqr_solve_models_dev(ctypes.byref(di), Bn, None, *a, None))
        assert b"NULL" in lib.crx_last_error(), hole
    bad(lib.crx_ilqr_solve_models(None, Bn, *[_p(x) for x in args]))
    bad(lib.crx_ilqr_solve_models(ctypes.byref(di), -1, *[_p(x) for x in args]))
    bad(lib.crx_ilqr_solve_models(ctypes.byref(abi.ilqr_desc(N, *AB, max_iter=-1)), Bn, *[_p(x) for x in args]))


def test_bindings_reject_wrong_model_shapes(lib, AB):
    from crx import abi

    b = abi.Binding(lib, "crx_")
    Bn, N = 2, 10
    args = (np.zeros((Bn, 6)), np.zeros((Bn, 6)), np.zeros((Bn, 1, N + 1)), np.zeros((Bn, 1, N + 1)), np.zeros((Bn, 1)),
            np.ones(Bn, dtype=np.int32))
    d = abi.ilqr_desc(N, *AB)
    for models in ((np.zeros((3, 6, 6)), np.zeros((3, 6, 2))), (np.zeros((Bn, 6, 6)), np.zeros((Bn, 2, 6))), (np.zeros((6, 6)), np.zeros((6, 2))),
                   (np.zeros((Bn, 36)), np.zeros((Bn, 12)))):
        with pytest.raises(ValueError, match="expected shape"):
            b.ilqr_solve(d, *args, models=models)
    with pytest.raises(ValueError, match="expected shape"):
        b.lqr_design(abi.lqr_desc(), np.zeros((Bn, 6, 6)), np.zeros((3, 6, 2)))
    with pytest.raises(ValueError, match="expected shape"):
        b.lqr_design(abi.lqr_desc(), np.zeros((Bn, 6, 5)), np.zeros((Bn, 6, 2)))


def test_new_entries_refuse_without_gpu(lib, AB):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible; the loud-failure path is exercised in the CPU container")
    from crx import abi

    assert lib.crx_init(0) == -2  # CRX_ERR_NO_DEVICE
    b = abi.Binding(lib, "crx_")
    with pytest.raises(RuntimeError, match="crx_init"):
        b.lqr_design(abi.lqr_desc(), *AB)
    Bn, N = 2, 10
    args = (np.zeros((Bn, 6)), np.zeros((Bn, 6)), np.zeros((Bn, 1, N + 1)), np.zeros((Bn, 1, N + 1)), np.zeros((Bn, 1)),
            np.ones(Bn, dtype=np.int32))
    with pytest.raises(RuntimeError, match="crx_init"):
        b.ilqr_solve(abi.ilqr_desc(N, *AB), *args, models=(np.repeat(AB[0][None], Bn, axis=0), np.repeat(AB[1][None], Bn, axis=0)))
    K, x, u = np.zeros((1, 2, 6)), np.zeros((1, 6)), np.zeros((1, 2))
    assert lib.crx_lqr_step_dev(1, _p(K), _p(x), _p(x), _p(u), None) == -4  # CRX_ERR_NOT_INIT: nothing was launched
    assert b"crx_init" in lib.crx_last_error()
