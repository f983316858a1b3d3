"""One LTI model per problem for the MPC-CBF / tracking NLP, without a GPU: the C ABI of crx_cbf_models_reach_dev /
crx_cbf_solve_models / crx_cbf_solve_models_dev is exported and declared, the Python wrappers refuse wrong model shapes and dtypes
before they touch the library, and without a device the new entries fail the way their shared-model twins do."""
import ctypes
import os

import numpy as np
import pytest

import conftest

NEW_SYMBOLS = ("crx_cbf_models_reach_dev", "crx_cbf_solve_models", "crx_cbf_solve_models_dev")


@pytest.fixture(scope="module")
def lib():
    import crx

    if not os.path.exists(crx.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return crx.lib()


class _NoLibrary:
    """Stands in for the CDLL and exports nothing: a wrapper that reaches for an entry point dies with AttributeError, not ValueError."""


def _args(Bn, N, V=1):
    return (np.zeros((Bn, 6)), np.zeros((Bn, 6)), np.zeros((Bn, V, N + 1)), np.zeros((Bn, V, N + 1)), np.zeros((Bn, V)),
            np.ones(Bn, dtype=np.int32))


def test_new_symbols_exported_and_declared(lib):
    src = open(os.path.join(conftest.ROOT, "include", "crx.h")).read()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n + "(" in src, n
    assert "#define CRX_CBF_MODEL_REACH_DOUBLES(batch)" in src
    assert lib.crx_version() == 400
    from crx import montecarlo, torch_api

    assert torch_api.CBF_REACH_ROW == 25 and "#define CRX_MAX_N 24 " in src   # a row of the reach table is CRX_MAX_N + 1 doubles
    assert hasattr(torch_api, "CbfModels")
    import inspect

    for f in (torch_api.cbf_solve_dev, montecarlo.MpccbfRaces.__init__, montecarlo.mpccbf_races):
        assert "models" in inspect.signature(f).parameters, f


def test_numpy_wrapper_rejects_wrong_models_before_the_library(AB):
    from crx import abi

    b = abi.Binding(_NoLibrary(), "crx_")
    Bn, N = 2, 10
    d = abi.cbf_desc(N, 1, *AB)
    ok_A, ok_B = np.zeros((Bn, 6, 6)), np.zeros((Bn, 6, 2))
    for models in ((np.zeros((3, 6, 6)), np.zeros((3, 6, 2))), (ok_A, np.zeros((Bn, 2, 6))), (np.zeros((6, 6)), np.zeros((6, 2))),
                   (np.zeros((Bn, 36)), np.zeros((Bn, 12))), (ok_A, np.zeros((Bn + 1, 6, 2)))):
        with pytest.raises(ValueError, match="expected shape"):
            b.cbf_solve(d, *_args(Bn, N), models=models)
    for models in ((ok_A.astype(np.float32), ok_B), (ok_A, ok_B.astype(np.float32)), (ok_A.astype(np.int64), ok_B.astype(np.int64))):
        with pytest.raises(ValueError, match="float64"):
            b.cbf_solve(d, *_args(Bn, N), models=models)
    for models in ((ok_A,), (ok_A, ok_B, ok_B), 3.0):
        with pytest.raises(ValueError, match="pair"):
            b.cbf_solve(d, *_args(Bn, N), models=models)


def test_torch_wrappers_reject_wrong_models_before_the_library(AB, monkeypatch):
    import torch

    from crx import abi, montecarlo, torch_api

    monkeypatch.setattr(torch_api, "_call", lambda name, *a: pytest.fail("the wrapper called %s before checking its arguments" % name))
    d = abi.cbf_desc(10, 1, *AB)
    Bn = 2
    A, B = torch.zeros((Bn, 6, 6), dtype=torch.float64), torch.zeros((Bn, 6, 2), dtype=torch.float64)
    # host tensors, wrong dtype, wrong shape, not tensors at all
    for a, b in ((A, B), (A.float(), B.float()), (A[:, :5], B), (A, B[:1]), (A.numpy(), B.numpy()), (A[0], B[0])):
        with pytest.raises(ValueError):
            torch_api.CbfModels(d, a, b)
    # the closed loop: model shapes are checked against the number of races
    with pytest.raises(ValueError, match="models"):
        montecarlo._models(np.zeros((3, 6, 6)), np.zeros((3, 6, 2)), Bn, "cpu")
    with pytest.raises(ValueError, match="models"):
        montecarlo._models(np.zeros((Bn, 6, 6)), np.zeros((Bn, 2, 6)), Bn, "cpu")


def test_new_entries_refuse_without_gpu(lib, AB):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible; the loud-failure path is exercised in the CPU container")
    from crx import abi

    assert lib.crx_init(0) == -2  # CRX_ERR_NO_DEVICE
    b = abi.Binding(lib, "crx_")
    Bn, N = 2, 10
    d = abi.cbf_desc(N, 1, *AB)
    models = (np.repeat(AB[0][None], Bn, axis=0), np.repeat(AB[1][None], Bn, axis=0))
    with pytest.raises(RuntimeError, match="crx_init") as shared:
        b.cbf_solve(d, *_args(Bn, N))
    with pytest.raises(RuntimeError, match="crx_init") as own:
        b.cbf_solve(d, *_args(Bn, N), models=models)
    assert "rc=-4" in str(shared.value) and "rc=-4" in str(own.value)   # CRX_ERR_NOT_INIT from both
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    reach = np.zeros((Bn, 2, 25))
    assert lib.crx_cbf_models_reach_dev(ctypes.byref(d), Bn, p(models[0]), p(models[1]), p(reach), None) == -4
    assert b"crx_init" in lib.crx_last_error()
    x0, xt, os_, oe, lo, no = _args(Bn, N)
    out = [np.zeros((Bn, N + 1, 6)), np.zeros((Bn, N, 2)), np.zeros((Bn, 1, N + 1)), np.zeros(Bn), np.zeros(Bn, np.int32), np.zeros(Bn),
           np.zeros(Bn, np.int32)]
    rc_models = lib.crx_cbf_solve_models_dev(ctypes.byref(d), Bn, None, None, p(x0), p(models[0]), p(models[1]), p(reach), p(xt), p(os_), p(oe),
                                             p(lo), p(no), None, *[p(o) for o in out], None)
    rc_shared = lib.crx_cbf_solve_ordered_dev(ctypes.byref(d), Bn, None, None, p(x0), p(xt), p(os_), p(oe), p(lo), p(no), None,
                                              *[p(o) for o in out], None)
    assert rc_models == rc_shared == -4   # nothing was launched
