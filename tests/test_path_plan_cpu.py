"""CPU-only checks of the path-planner entry points (crx_path_prep, crx_path_plan: include/crx.h P1-P8): exported symbols, the
descriptor's layout, argument refusals without a device -- and the probe that lets tests/test_gpu_path_plan.py demand equal flags and
equal side-row patterns on EVERY scenario of its draws a-d: with the mirror's path_qp_inputs and the oracle's path_solve as the
yardstick, no scenario has two region costs closer than 1e-4 relative and no s sample closer than 1e-5 to a front / rear range edge."""
import ctypes

import numpy as np
import pytest

import path_plan_cases as cases

SYMBOLS = ("crx_pathprep_desc_default", "crx_path_prep", "crx_path_prep_dev", "crx_path_plan", "crx_path_plan_dev")


@pytest.fixture(scope="module")
def lib():
    import crx

    return crx.lib()


def test_symbols_exported(lib):
    for n in SYMBOLS:
        assert hasattr(lib, n), n
    assert lib.crx_version() == 400


def test_desc_default_matches_mirror(lib):
    from crx import abi

    d = abi.PathPrepDesc()
    lib.crx_pathprep_desc_default(ctypes.byref(d), 10, 3, 5, 300, ctypes.c_double(1.0), ctypes.c_double(19.25))
    assert bytes(d) == bytes(abi.pathprep_desc(10, 3, 5, 300, 1.0, 19.25))
    assert (d.safety_factor, d.prediction_factor, d.lookahead, d.next_lap_range) == (4.5, 0.5, 4.0, 20.0)
    assert (d.veh_length, d.veh_width, d.a_max_plan) == (0.4, 0.2, 1.5)


def _plan_args(S, N, V, VA, T):
    f, i = (lambda *sh: np.zeros(sh)), (lambda *sh: np.zeros(sh, dtype=np.int32))
    R = V + 1
    ins = [i(S), f(S, 6), f(S, 6), i(S), i(S, V), f(S, VA, 6), f(S), f(S, V, N + 1), f(T), f(T), f(T)]
    outs = [f(S * R, N + 1), f(S * R), i(S * R), f(S * R), i(S * R), i(S), f(S, N + 1, 6), i(S)]
    return ins, outs


def test_argument_refusals_need_no_device(lib):
    """N > CRX_MAX_N, V > CRX_MAX_VEH and NULL arrays are CRX_ERR_ARG (-1) before the library's state is looked at: they answer the
    same with and without an initialised device.  Well-formed arguments without one: CRX_ERR_NOT_INIT, never a computation."""
    import torch

    from crx import abi

    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    for fn in (lib.crx_path_plan, lib.crx_path_prep):
        fn.restype = ctypes.c_int

    def plan(d, qd, ins, outs, drop=None):
        a = [p(x) for x in ins + outs]
        if drop is not None:
            a[drop] = None
        return lib.crx_path_plan(ctypes.byref(d), ctypes.byref(qd), ctypes.c_int(ins[1].shape[0]), *a)

    S, N, V, VA, T = 2, 10, 3, 3, 50
    ins, outs = _plan_args(S, N, V, VA, T)
    good, qd = abi.pathprep_desc(N, V, VA, T, 1.0, 19.25), abi.path_desc(N, 0.98)
    assert plan(abi.pathprep_desc(abi.CRX_MAX_N + 1, V, VA, T, 1.0, 19.25), qd, ins, outs) == -1
    assert b"N=" in lib.crx_last_error()
    assert plan(abi.pathprep_desc(N, abi.CRX_MAX_VEH + 1, VA, T, 1.0, 19.25), qd, ins, outs) == -1
    assert b"n_veh_max" in lib.crx_last_error()
    assert plan(good, abi.path_desc(N + 1, 0.98), ins, outs) == -1                      # the two descriptors disagree
    for drop in range(1, len(ins) + len(outs)):                                          # (argument 0, active, may be NULL)
        assert plan(good, qd, ins, outs, drop=drop) == -1, drop
        assert b"NULL" in lib.crx_last_error()
    pins = ins[1:10]
    pouts = [np.zeros((S * (V + 1), N + 1)) for _ in range(4)] + [np.zeros(S * (V + 1)), np.zeros(S * (V + 1)), np.zeros(S)]
    for drop in range(len(pins) + len(pouts)):
        a = [p(x) for x in pins + pouts]
        a[drop] = None
        assert lib.crx_path_prep(ctypes.byref(good), ctypes.c_int(S), *a) == -1, drop
    assert lib.crx_path_prep(ctypes.byref(abi.pathprep_desc(N, V, VA, 1, 1.0, 19.25)), ctypes.c_int(S), *[p(x) for x in pins + pouts]) == -1
    if not torch.cuda.is_available():
        assert plan(good, qd, ins, outs) == -4                                          # CRX_ERR_NOT_INIT
        assert lib.crx_path_prep(ctypes.byref(good), ctypes.c_int(S), *[p(x) for x in pins + pouts]) == -4


@pytest.mark.parametrize("name", cases.PROBED)
def test_draws_are_unambiguous(orc, name):
    """The probe behind the GPU tests' "every scenario, no exclusions".  Figures of the draws as committed, in draw order a-d: smallest
    relative gap (c2 - c1) / max(1, |c1|) between the two smallest converged region costs 5.8e-2, 2.9e-4, 4.5e-4, 4.8e-3; smallest
    distance of an s sample to a range edge 2.5e-4, 2.5e-4, 6.2e-4, 2.0e-3; draw a: 886 of 1024 regions infeasible, 121 scenarios with every
    region infeasible; draw b: winners per region 83 / 41 / 18 / 114.  (The optimal-trajectory table of l_shape reaches past the lap
    length, so neither P2 nor P8 can raise on these draws.)"""
    d, sc, m = cases.draw(name), cases.scene(name), cases.mirror_prep(name)
    S, R, N1 = d["S"], d["V"] + 1, d["N"] + 1
    assert (sc["n_veh"] == d["V"]).all() and not m["raised"].any()
    r = orc.path_solve(cases.descs(d)[2], *(m[k].reshape(S * R, -1).squeeze() for k in ("opt", "bez", "lb", "ub", "e0", "eN")))
    cost = np.where(r["status"] == 0, r["cost"], np.inf).reshape(S, R)
    two = np.sort(cost, axis=1)[:, :2]
    both = np.isfinite(two).all(axis=1)
    gap = (two[both, 1] - two[both, 0]) / np.maximum(1.0, np.abs(two[both, 0]))
    print("draw %s: %d scenarios with two converged regions, smallest relative cost gap %.3g, smallest edge distance %.3g, "
          "%d of %d regions infeasible, %d scenarios with every region infeasible"
          % (name, both.sum(), gap.min(), m["edge"].min(), (r["status"] != 0).sum(), S * R, np.isinf(cost).all(axis=1).sum()))
    assert both.sum() >= 1
    assert gap.min() >= 1e-4
    assert m["edge"].min() >= 1e-5
    flag, target, raised = cases.host_select(d, sc, m["span"], r["E"].reshape(S, R, N1), cost)
    assert not raised.any()                                                            # no scenario takes the P8 raise
    if name == "a":                                                                    # the all-inf and fall-back path is in the draw
        assert np.isinf(cost).all(axis=1).sum() >= 32
    if name == "b":
        assert (np.bincount(flag, minlength=R) > 0).all()                              # every region wins somewhere
