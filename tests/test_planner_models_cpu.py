"""One LTI model per planner region QP, without a GPU: the C ABI of crx_planner_models_reach_dev / crx_planner_solve_models* /
crx_planner_plan_models* is exported and declared, mixed NULL model pointers are refused before the device is looked at, the Python
wrappers refuse wrong model shapes and dtypes before they touch the library, without a device the new entries fail the way their
shared-model twins do, and the reach table -- restated here in numpy, operation by operation -- is the one the reachability screen of
the shipped model is built on (the oracle applies that screen: the QPs the table proves infeasible are the ones it answers in 0
iterations)."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import conftest

NEW_SYMBOLS = ("crx_planner_models_reach_dev", "crx_planner_solve_models", "crx_planner_solve_models_dev", "crx_planner_plan_models",
               "crx_planner_plan_models_dev")
CRX_MAX_N = 24
CRX_ERR_ARG, CRX_ERR_NOT_INIT = -1, -4


def planner_reach_numpy(A, B, delta_max, a_max, N):
    """reach_bound(A, B, delta_max, a_max, 5, N - 1, gain, rows) of csrc/crx_api.hip, operation by operation in float64, in the layout
    of crx_planner_models_reach_dev: [CRX_MAX_N][7] = (rows[j] (6), gain[j]), zero for j >= N."""
    tab = np.zeros((CRX_MAX_N, 7))
    w = np.zeros(6)
    w[5] = 1.0
    acc = 0.0
    tab[0, :6] = w
    for j in range(1, N):
        v0 = v1 = 0.0
        for i in range(6):
            v0 = v0 + w[i] * B[i, 0]
            v1 = v1 + w[i] * B[i, 1]
        acc = acc + (abs(v0) * delta_max + abs(v1) * a_max)
        wn = np.zeros(6)
        for a in range(6):
            for i in range(6):
                wn[a] = wn[a] + w[i] * A[i, a]
        w = wn
        tab[j, :6] = w
        tab[j, 6] = acc
    return tab


def screened(tab, N, x0, ey_lb, ey_ub):
    """The reachability screen of the solver kernel (csrc/crx_kernels.hip) on one problem's table: True = proved infeasible."""
    fr = tab[:N, :6] @ x0
    g = tab[:N, 6]
    return bool(((ey_lb > fr + g + 1e-6) | (ey_ub < fr - g - 1e-6)).any())


@pytest.fixture(scope="module")
def lib():
    import crx

    if not os.path.exists(crx.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return crx.lib()


class _NoLibrary:
    """Stands in for the CDLL and exports nothing: a wrapper that reaches for an entry point dies with AttributeError, not ValueError."""


def _args(Bn, N):
    return np.zeros((Bn, 6)), np.zeros((Bn, N + 1)), np.zeros((Bn, N + 1)), np.zeros((Bn, N)), np.zeros(Bn)


def _plan_args(S, V, N):
    return _args(S * (V + 1), N) + (np.zeros(S, np.int32), np.zeros((S, V, N + 1)), np.zeros((S, V, N + 1)), np.zeros(S, np.int32))


def _outs(Bn, N):
    return [np.zeros((Bn, N + 1, 6)), np.zeros((Bn, N, 2)), np.zeros(Bn), np.zeros(Bn, np.int32), np.zeros(Bn), np.zeros(Bn, np.int32)]


_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731


def test_new_symbols_exported_and_declared(lib):
    src = open(os.path.join(conftest.ROOT, "include", "crx.h")).read()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n + "(" in src, n
    assert "#define CRX_PLANNER_MODEL_REACH_DOUBLES(batch) ((size_t)(batch) * CRX_MAX_N * 7)" in src
    assert "#define CRX_MAX_N %d " % CRX_MAX_N in src
    assert lib.crx_version() == 400
    from crx import abi, montecarlo, torch_api

    assert torch_api.PLANNER_REACH_ROWS == CRX_MAX_N and hasattr(torch_api, "PlannerModels")
    for f in (abi.Binding.planner_solve, abi.Binding.planner_plan, torch_api.planner_solve_dev, torch_api.planner_plan_dev,
              montecarlo.GameLaps.__init__, montecarlo.game_laps):
        assert "models" in inspect.signature(f).parameters, f


def test_mixed_null_model_pointers_are_refused_before_the_device(lib, AB):
    """All model pointers or none.  A check on pointers alone, made before the device is asked for: CRX_ERR_ARG with or without a GPU;
    the full and the empty set pass it (and then meet whatever the shared launch meets)."""
    from crx import abi

    Bn, N, V = 8, 10, 1
    S = Bn // (V + 1)
    d, sd = abi.planner_desc(N, *AB), abi.select_desc(N, V, 19.2)
    x0, bs, be, lb, ub = _args(Bn, N)
    mA, mB = np.repeat(AB[0][None], Bn, axis=0), np.repeat(AB[1][None], Bn, axis=0)
    reach = np.zeros((Bn, CRX_MAX_N, 7))
    out = _outs(Bn, N)
    sel = (np.zeros(S, np.int32), np.zeros((S, V, N + 1)), np.zeros((S, V, N + 1)), np.zeros(S, np.int32))
    sout = [np.zeros(S, np.int32), np.zeros((S, V + 1)), np.zeros((S, N + 1, 6))]

    def solve_dev(a, b, r):
        return lib.crx_planner_solve_models_dev(ctypes.byref(d), Bn, None, _p(x0), a, b, r, _p(bs), _p(be), _p(lb), _p(ub),
                                                *[_p(o) for o in out], None)

    def plan_dev(a, b, r):
        return lib.crx_planner_plan_models_dev(ctypes.byref(d), ctypes.byref(sd), S, None, _p(x0), a, b, r, _p(bs), _p(be), _p(lb), _p(ub),
                                               *[_p(s) for s in sel], *[_p(o) for o in out], *[_p(o) for o in sout], None)

    def solve_host(a, b):
        return lib.crx_planner_solve_models(ctypes.byref(d), Bn, _p(x0), a, b, _p(bs), _p(be), _p(lb), _p(ub), *[_p(o) for o in out])

    def plan_host(a, b):
        return lib.crx_planner_plan_models(ctypes.byref(d), ctypes.byref(sd), S, _p(x0), a, b, _p(bs), _p(be), _p(lb), _p(ub),
                                           *[_p(s) for s in sel], *[_p(o) for o in out], *[_p(o) for o in sout])

    A_, B_, R_ = _p(mA), _p(mB), _p(reach)
    for f in (solve_dev, plan_dev):
        for mix in ((A_, None, None), (None, B_, None), (None, None, R_), (A_, B_, None), (A_, None, R_), (None, B_, R_)):
            assert f(*mix) == CRX_ERR_ARG, (f.__name__, mix)
            assert b"model_A, model_B and model_reach go together" in lib.crx_last_error()
    for f in (solve_host, plan_host):
        for mix in ((A_, None), (None, B_)):
            assert f(*mix) == CRX_ERR_ARG, (f.__name__, mix)
            assert b"model_A and model_B go together" in lib.crx_last_error()
    import torch

    if not torch.cuda.is_available():   # the complete sets pass the pointer check and stop where the shared entries stop
        assert lib.crx_init(0) == -2
        assert solve_host(A_, B_) == solve_host(None, None) == CRX_ERR_NOT_INIT
        assert plan_host(A_, B_) == plan_host(None, None) == CRX_ERR_NOT_INIT
        assert b"crx_init" in lib.crx_last_error()


def test_numpy_wrapper_rejects_wrong_models_before_the_library(AB):
    from crx import abi

    b = abi.Binding(_NoLibrary(), "crx_")
    N, V, S = 10, 1, 2
    Bn = S * (V + 1)
    d, sd = abi.planner_desc(N, *AB), abi.select_desc(N, V, 19.2)

    def solve(models):
        return b.planner_solve(d, *_args(Bn, N), models=models)

    def plan(models):   # one model per SCENARIO
        return b.planner_plan(d, sd, *_plan_args(S, V, N), models=models)

    for f, n in ((solve, Bn), (plan, S)):
        ok_A, ok_B = np.zeros((n, 6, 6)), np.zeros((n, 6, 2))
        for models in ((np.zeros((n + 1, 6, 6)), np.zeros((n + 1, 6, 2))), (ok_A, np.zeros((n, 2, 6))), (np.zeros((6, 6)), np.zeros((6, 2))),
                       (np.zeros((n, 36)), np.zeros((n, 12))), (ok_A, np.zeros((n + 1, 6, 2)))):
            with pytest.raises(ValueError, match="expected shape"):
                f(models)
        for models in ((ok_A.astype(np.float32), ok_B), (ok_A, ok_B.astype(np.float32)), (ok_A.astype(np.int64), ok_B.astype(np.int64))):
            with pytest.raises(ValueError, match="float64"):
                f(models)
        for models in ((ok_A,), (ok_A, ok_B, ok_B), 3.0):
            with pytest.raises(ValueError, match="pair"):
                f(models)
        with pytest.raises(AttributeError):   # good models reach for the library: there is no other path
            f((ok_A, ok_B))


def test_torch_wrappers_reject_wrong_models_before_the_library(AB, monkeypatch):
    import torch

    from crx import abi, torch_api

    monkeypatch.setattr(torch_api, "_call", lambda name, *a: pytest.fail("the wrapper called %s before checking its arguments" % name))
    d = abi.planner_desc(10, *AB)
    n = 2
    A, B = torch.zeros((n, 6, 6), dtype=torch.float64), torch.zeros((n, 6, 2), dtype=torch.float64)
    # host tensors, wrong dtype, wrong shape, not tensors at all
    for a, b in ((A, B), (A.float(), B.float()), (A[:, :5], B), (A, B[:1]), (A.numpy(), B.numpy()), (A[0], B[0])):
        with pytest.raises(ValueError):
            torch_api.PlannerModels(d, a, b, regions=3)
    # anything but a PlannerModels, and one built for another batch / horizon / input box
    with pytest.raises(ValueError, match="PlannerModels"):
        torch_api._planner_models((A, B), d, n)
    m = torch_api.PlannerModels.__new__(torch_api.PlannerModels)
    m.batch, m.N, m.delta_max, m.a_max = 8, 10, d.delta_max, d.a_max
    assert torch_api._planner_models(m, d, 8) is m
    with pytest.raises(ValueError, match="built for batch"):
        torch_api._planner_models(m, d, 6)
    with pytest.raises(ValueError, match="built for batch"):
        torch_api._planner_models(m, abi.planner_desc(12, *AB), 8)


def test_new_entries_refuse_without_gpu(lib, AB):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible; the loud-failure path is exercised in the CPU container")
    from crx import abi

    assert lib.crx_init(0) == -2  # CRX_ERR_NO_DEVICE
    b = abi.Binding(lib, "crx_")
    N, V, S = 10, 1, 2
    Bn = S * (V + 1)
    d, sd = abi.planner_desc(N, *AB), abi.select_desc(N, V, 19.2)
    per = lambda n: (np.repeat(AB[0][None], n, axis=0), np.repeat(AB[1][None], n, axis=0))   # noqa: E731
    for run in (lambda m: b.planner_solve(d, *_args(Bn, N), models=m and per(Bn)),
                lambda m: b.planner_plan(d, sd, *_plan_args(S, V, N), models=m and per(S))):
        with pytest.raises(RuntimeError, match="crx_init") as shared:
            run(None)
        with pytest.raises(RuntimeError, match="crx_init") as own:
            run(True)
        assert "rc=-4" in str(shared.value) and "rc=-4" in str(own.value)   # CRX_ERR_NOT_INIT from both: an error, not a fall-back
    mA, mB = per(Bn)
    reach = np.zeros((Bn, CRX_MAX_N, 7))
    assert lib.crx_planner_models_reach_dev(ctypes.byref(d), Bn, _p(mA), _p(mB), _p(reach), None) == CRX_ERR_NOT_INIT
    assert b"crx_init" in lib.crx_last_error() and not reach.any()
    x0, bs, be, lb, ub = _args(Bn, N)
    out = _outs(Bn, N)
    rc_models = lib.crx_planner_solve_models_dev(ctypes.byref(d), Bn, None, _p(x0), _p(mA), _p(mB), _p(reach), _p(bs), _p(be), _p(lb), _p(ub),
                                                 *[_p(o) for o in out], None)
    rc_shared = lib.crx_planner_solve_dev(ctypes.byref(d), Bn, _p(x0), _p(bs), _p(be), _p(lb), _p(ub), *[_p(o) for o in out], None)
    assert rc_models == rc_shared == CRX_ERR_NOT_INIT   # nothing was launched


@pytest.mark.parametrize("N", [7, 10, 12, 20, 24])
def test_reach_table_of_the_shipped_model(AB, N):
    """The restated table against what it stands for: rows[j] = e_ey' A^j (the free response of ey_j), gain[j] = sum_{m<j} |e_ey' A^m B|
    (delta_max, a_max)' (how far the boxed inputs move it), from matrix powers; zero for j >= N."""
    from crx import abi

    A, B = AB
    d = abi.planner_desc(N, A, B)
    tab = planner_reach_numpy(A, B, d.delta_max, d.a_max, N)
    assert tab.shape == (CRX_MAX_N, 7) and not tab[N:].any()
    np.testing.assert_array_equal(tab[0], [0, 0, 0, 0, 0, 1, 0])
    gain = 0.0
    for j in range(N):
        P = np.linalg.matrix_power(A, j)
        np.testing.assert_allclose(tab[j, :6], P[5], rtol=0, atol=1e-13 * max(1.0, np.abs(P[5]).max()))
        np.testing.assert_allclose(tab[j, 6], gain, rtol=1e-13, atol=0)
        gain += abs(P[5] @ B[:, 0]) * d.delta_max + abs(P[5] @ B[:, 1]) * d.a_max
    assert (np.diff(tab[:N, 6]) > 0).all()


@pytest.mark.parametrize("N,seed,V", [(12, 21, 3), (7, 23, 2)])
def test_table_screens_what_the_oracle_screens(orc, AB, N, seed, V):
    """The oracle applies the kernel's screen to the descriptor's model: the region QPs of a draw that the restated table proves
    infeasible are exactly those it reports infeasible without iterating."""
    from crx import abi, synth

    p = synth.cfg3_planner(16, N=N, seed=seed, V=V)
    d = abi.planner_desc(N, *AB)
    ro = orc.planner_solve(d, p["x0"], p["bez_s"], p["bez_ey"], p["ey_lb"], p["ey_ub"])
    tab = planner_reach_numpy(AB[0], AB[1], d.delta_max, d.a_max, N)
    mine = np.array([screened(tab, N, p["x0"][b], p["ey_lb"][b], p["ey_ub"][b]) for b in range(len(p["x0"]))])
    theirs = (ro["status"] == abi.CRX_INFEASIBLE) & (ro["iters"] == 0)
    assert mine.any() and not mine.all()
    np.testing.assert_array_equal(mine, theirs)
