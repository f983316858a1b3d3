"""Mixed fields without a GPU: the numpy model of crx_mixed_prep / crx_mixed_commit_dev (tests/mixed_model.py) on hand-made races; that
the draws of tests/test_gpu_mixed.py settle and hold the cases they are there for; the defaults of crx_mixed_desc_default and the argument
refusals of the three entries; the launch sequence of montecarlo.MixedRaces.step."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import conftest
import field_model as fm
import mixed_model as mm
import test_field_cpu as tfc

CRX_ERR_ARG, CRX_ERR_NOT_INIT = -1, -4


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def _hand_race():
    """One race of four on l_shape: car 0 a lap ahead in s, cars 1 and 2 near it, car 3 NaN."""
    track = tfc._track("l_shape")
    tab, L = track.point_and_tangent, track.lap_length
    x = np.zeros((1, 4, 6))
    x[0, :, 0] = [1.2, 0.8, 0.6, 0.5]
    x[0, :, 4] = [L + 5.0, 5.6, 4.1, 9.0]
    x[0, :, 5] = [0.1, -0.1, 0.2, 0.0]
    x[0, 3] = np.nan
    return tab, L, x


def test_model_prep_on_hand_made_races():
    tab, L, x = _hand_race()
    N, Ni = 10, 12
    f = fm.prep(tab, L, x, N)
    assert f["n_obs"][0].tolist() == [2, 2, 1, 0]                             # by hand: car 2 (margin 1.2) has car 1 at 5.68 outside
    for ego_policy in range(mm.N_POLICY):
        pol = np.array([[ego_policy, mm.MPCCBF, mm.ILQR, mm.ILQR]])
        for mode in (0, 1):
            m = mm.prep(tab, L, x, pol, N, Ni, mode)
            assert m["pred_s"].shape == (1, 4, Ni + 1) and np.array_equal(m["pred_s"][..., :N + 1], f["pred_s"], equal_nan=True)
            assert np.array_equal(m["clear"], f["clear"]) and m["m_nlp"][0].tolist() == [int(ego_policy in (mm.MPC_LTI, mm.MPCCBF)), 1, 0, 0]
            assert m["m_ilqr"][0].tolist() == [int(ego_policy == mm.ILQR), 0, 1, 1]
            # the NLP family: field_model's arrays for the MPCCBF cars, nothing for the others
            for c in range(4):
                if pol[0, c] == mm.MPCCBF:
                    assert all(np.array_equal(m[k][0, c], f[k][0, c]) for k in ("obs_s", "obs_ey", "lap_off", "n_obs"))
                else:
                    assert m["n_obs"][0, c] == 0 and not m["obs_s"][0, c].any() and not m["lap_off"][0, c].any()
            # the iLQR family: car 2 sees cars 0 and 1 (mode 1; the NaN car is kept by nobody) or its last other car, the NaN car: nobody
            assert m["il_n_obs"][0, 2] == (2 if mode else 0) and m["il_n_obs"][0, 3] == 0 and m["il_n_obs"][0, 1] == 0
            if mode:
                assert np.array_equal(m["il_obs_s"][0, 2, 0], m["pred_s"][0, 0, :Ni + 1]) and np.array_equal(m["il_obs_ey"][0, 2, 1], m["pred_ey"][0, 1, :Ni + 1])
                assert m["il_lap_off"][0, 2].tolist() == [0.0, 0.0, 0.0] and not m["il_obs_s"][0, 2, 2].any()   # column 0 of a roll-out is wrapped into one lap (F3)
            if ego_policy == mm.ILQR:                            # car 0 carries a lap: offsets L against cars that do not
                assert m["il_n_obs"][0, 0] == (2 if mode else 0)
                if mode:
                    assert m["il_lap_off"][0, 0].tolist() == [L, L, 0.0] and np.array_equal(m["il_obs_s"][0, 0, 1], m["pred_s"][0, 2, :Ni + 1])
            assert not np.isnan(m["il_obs_s"]).any() and not np.isnan(m["obs_s"]).any()
    # mode 0 with a finite last car: exactly that car; no iLQR arrays with N_ilqr = 0; one car per race
    x2 = x.copy()
    x2[0, 3] = [0.5, 0, 0, 0, 9.0, 0.0]
    m = mm.prep(tab, L, x2, np.array([[mm.ILQR] * 4]), N, 50)
    assert m["pred_s"].shape[-1] == 51 and m["il_n_obs"][0].tolist() == [1, 1, 1, 1]
    assert np.array_equal(m["il_obs_s"][0, 0, 0], m["pred_s"][0, 3]) and np.array_equal(m["il_obs_s"][0, 3, 0], m["pred_s"][0, 2])
    assert "il_obs_s" not in mm.prep(tab, L, x2, np.array([[mm.ILQR] * 4]), N, 0)
    one = mm.prep(tab, L, x2[:, :1], np.array([[mm.ILQR]]), N, 12, 1)
    assert one["il_obs_s"].shape == (1, 1, 0, 13) and one["il_n_obs"].tolist() == [[0]] and np.isinf(one["clear"]).all()


def test_model_commit():
    rng = np.random.default_rng(2)
    pol = np.array([mm.NONE, mm.PID, mm.LQR, mm.MPC_LTI, mm.MPCCBF, mm.ILQR, 6, -1], dtype=np.int32)
    Bn = len(pol)
    x, vt, eyt = rng.standard_normal((Bn, 6)), rng.uniform(0.5, 1.0, Bn), rng.uniform(-0.2, 0.2, Bn)
    K, xt = rng.standard_normal((Bn, 2, 6)), rng.standard_normal((Bn, 6))
    Un, Ui = rng.standard_normal((Bn, 10, 2)), rng.standard_normal((Bn, 20, 2))
    sn, si = np.full(Bn, 1, dtype=np.int32), np.full(Bn, 5, dtype=np.int32)
    u, st = mm.commit(pol, x, pid=(vt, eyt), lqr=(K, xt), nlp=(Un, sn), ilqr=(Ui, si))
    assert st.tolist() == [4, 0, 0, 1, 1, 5, 4, 4] and not u[[0, 6, 7]].any()
    assert u[1].tolist() == [-0.6 * (x[1, 5] - eyt[1]) - 0.9 * x[1, 3], 1.5 * (vt[1] - x[1, 0])]
    np.testing.assert_allclose(u[2], -K[2] @ (x[2] - xt[2]), rtol=0, atol=1e-14)
    assert np.array_equal(u[3:5], Un[3:5, 0]) and np.array_equal(u[5], Ui[5, 0])
    u2, st2 = mm.commit(pol, x, pid=(vt, eyt), nlp=(Un, sn))
    assert st2.tolist() == [4, 0, 4, 1, 1, 4, 4, 4] and not u2[[2, 5]].any() and np.array_equal(u2[[1, 3, 4]], u[[1, 3, 4]])


@pytest.mark.parametrize("C", [1, 2, 4, 7])
def test_the_gpu_tests_draws_settle(C):
    """tests/test_gpu_mixed.draw asserts on the CPU model, before any launch, what its cases are there for; here every draw the GPU tests use."""
    import test_gpu_mixed as tg

    for name in tg.TRACKS:
        for n_ilqr in tg.N_ILQR:
            tab, L, x, dims, pol = tg.draw(name, C, tg.N_PREP, n_ilqr, 100 * C + n_ilqr)
            assert x.shape == (tg.R_PREP, C, 6) and pol.shape == (tg.R_PREP, C) and pol.dtype == np.int32
    if C == 4:
        assert tg.draw("l_shape", 4, tg.N_PREP, 12, 77, R=150)[2].shape == (150, 4, 6)


# ---- the C ABI without a device ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import crx

    return crx.lib()


def test_symbols_constants_and_default_descriptor(lib):
    from crx import abi

    src = open(os.path.join(conftest.ROOT, "include", "crx.h")).read()
    for n in ("crx_mixed_desc_default", "crx_mixed_prep", "crx_mixed_prep_dev", "crx_mixed_commit_dev"):
        assert hasattr(lib, n) and n + "(" in src, n
    for code, name in enumerate(("NONE", "PID", "LQR", "MPC_LTI", "MPCCBF", "ILQR")):
        assert "#define CRX_POLICY_%s %d" % (name, code) in src and getattr(abi, "POLICY_" + name) == code == getattr(mm, name)
        assert abi.POLICY_NAMES[code] == name.lower()
    d = abi.MixedDesc()
    lib.crx_mixed_desc_default(ctypes.byref(d), 12, 50, 4, 9, ctypes.c_double(19.25))
    assert bytes(d) == bytes(abi.mixed_desc(12, 50, 4, 9, 19.25))
    assert (d.N, d.N_ilqr, d.n_cars, d.n_seg, d.degree, d.ilqr_obstacles) == (12, 50, 4, 9, 6, 0)
    assert (d.lap_length, d.dt, d.safety_time, d.l_sum, d.w_sum) == (19.25, 0.1, 2.0, 0.4, 0.2)
    assert lib.crx_version() == 400
    assert abi.policy_codes([["pid", "MPCCBF"], ["none", "ilqr"]]).tolist() == [[1, 4], [0, 5]] and abi.policy_codes([[3, 2]]).dtype == np.int32
    for bad in ([["lmpc"]], [[6]], [[-1]], [[1.0]]):
        with pytest.raises(ValueError):
            abi.policy_codes(bad)


def test_mixed_prep_refuses_bad_arguments_without_a_device(lib):
    import torch

    from crx import abi

    lib.crx_mixed_prep.restype = ctypes.c_int
    lib.crx_mixed_prep_dev.restype = ctypes.c_int
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    R, C, N, Ni, S = 3, 4, 10, 20, 9
    f = lambda *sh: np.ones(sh)   # noqa: E731
    i = lambda *sh: np.ones(sh, dtype=np.int32)   # noqa: E731
    names = ("track", "xcurv", "policy", "car_dims", "pred_s", "pred_ey", "obs_s", "obs_ey", "lap_off", "n_obs", "obs_dims", "m_nlp", "il_obs_s",
             "il_obs_ey", "il_lap_off", "il_n_obs", "m_ilqr", "clear")

    def arrays(C=C, Ni=Ni):
        V, NP = C - 1, max(N, Ni)
        return dict(track=f(S, 6), xcurv=f(R, C, 6), policy=i(R, C), car_dims=f(R, C, 2), pred_s=f(R, C, NP + 1), pred_ey=f(R, C, NP + 1),
                    obs_s=f(R, C, V, N + 1), obs_ey=f(R, C, V, N + 1), lap_off=f(R, C, V), n_obs=i(R, C), obs_dims=f(R, C, V, 2), m_nlp=i(R, C),
                    il_obs_s=f(R, C, V, Ni + 1), il_obs_ey=f(R, C, V, Ni + 1), il_lap_off=f(R, C, V), il_n_obs=i(R, C), m_ilqr=i(R, C), clear=f(R, C))

    def call(d, a, n_races=R, dev=False):
        ptrs = [p(a[k]) for k in names]
        if dev:
            return lib.crx_mixed_prep_dev(ctypes.byref(d) if d is not None else None, ctypes.c_int(n_races), *ptrs, None)
        return lib.crx_mixed_prep(ctypes.byref(d) if d is not None else None, ctypes.c_int(n_races), *ptrs)

    def refused(d, a, what, **kw):
        for dev in (False, True):
            assert call(d, a, dev=dev, **kw) == CRX_ERR_ARG, (what, dev)
            assert lib.crx_last_error(), what

    good = lambda **kw: abi.mixed_desc(N, Ni, C, S, 19.25, **kw)   # noqa: E731
    refused(None, arrays(), "desc")
    for bad_N in (0, -1, abi.CRX_MAX_N + 1):
        refused(abi.mixed_desc(bad_N, Ni, C, S, 19.25), arrays(), "N")
        assert b"N=" in lib.crx_last_error()
    for bad_Ni in (-1, abi.CRX_ILQR_MAX_N + 1):                             # 65
        refused(abi.mixed_desc(N, bad_Ni, C, S, 19.25), arrays(), "N_ilqr")
        assert b"N_ilqr" in lib.crx_last_error()
    for bad_C in (0, abi.CRX_MAX_OBS + 2):                                  # 0 and 8
        refused(abi.mixed_desc(N, Ni, bad_C, S, 19.25), arrays(), "n_cars")
        assert b"n_cars" in lib.crx_last_error()
    for bad_S in (0, 65):
        refused(abi.mixed_desc(N, Ni, C, bad_S, 19.25), arrays(), "n_seg")
        assert b"n_seg" in lib.crx_last_error()
    for bad_mode in (2, -1):
        refused(good(ilqr_obstacles=bad_mode), arrays(), "ilqr_obstacles")
        assert b"ilqr_obstacles" in lib.crx_last_error()
    for bad in (0.0, -1.0, np.inf, np.nan):
        refused(abi.mixed_desc(N, Ni, C, S, bad), arrays(), "lap_length")
        for key in ("dt", "l_sum", "w_sum"):
            refused(good(**{key: bad}), arrays(), key)
    for bad in (0, 3, 10):
        refused(good(degree=bad), arrays(), "degree")
    refused(good(), arrays(), "n_races", n_races=-1)
    assert b"n_races" in lib.crx_last_error()
    for hole in ("track", "xcurv", "policy", "pred_s", "pred_ey", "obs_s", "obs_ey", "lap_off", "n_obs", "m_nlp", "il_obs_s", "il_obs_ey", "il_lap_off",
                 "il_n_obs", "m_ilqr"):
        refused(good(), dict(arrays(), **{hole: None}), hole)
        assert b"NULL" in lib.crx_last_error()
    for hole in ("car_dims", "obs_dims"):                                   # both or neither
        refused(good(), dict(arrays(), **{hole: None}), hole)
        assert b"go together" in lib.crx_last_error()
    for bad in (0.0, -0.4, np.inf, np.nan):                                 # the host entry reads the rows
        a = arrays()
        a["car_dims"][1, 2, 1] = bad
        assert call(good(), a) == CRX_ERR_ARG and b"car_dims" in lib.crx_last_error()
    for bad in (-1, 6, 1 << 20):                                            # ... and the policy codes
        a = arrays()
        a["policy"][2, 1] = bad
        assert call(good(), a) == CRX_ERR_ARG and b"policy" in lib.crx_last_error()
    # what may be NULL: clear; car_dims with obs_dims; the iLQR family with N_ilqr = 0; with one car the [V] arrays.  Well-formed calls get
    # as far as the library's state, as crx_field_prep's do: without a device CRX_ERR_NOT_INIT, never a computation
    if not torch.cuda.is_available():
        il = dict(il_obs_s=None, il_obs_ey=None, il_lap_off=None, il_n_obs=None, m_ilqr=None)
        one = arrays(C=1)
        for d, a in ((good(), arrays()), (good(), dict(arrays(), clear=None)), (good(), dict(arrays(), car_dims=None, obs_dims=None)),
                     (good(ilqr_obstacles=1), arrays()), (abi.mixed_desc(N, 0, C, S, 19.25), dict(arrays(Ni=0), **il)),
                     (abi.mixed_desc(N, Ni, 1, S, 19.25), dict(one, obs_s=None, obs_ey=None, lap_off=None, obs_dims=None, il_obs_s=None, il_obs_ey=None, il_lap_off=None)),
                     (abi.mixed_desc(1, 1, C, 1, 19.25), arrays()),
                     (abi.mixed_desc(abi.CRX_MAX_N, abi.CRX_ILQR_MAX_N, abi.CRX_MAX_OBS + 1, 64, 19.25), arrays(C=abi.CRX_MAX_OBS + 1, Ni=abi.CRX_ILQR_MAX_N))):
            for dev in (False, True):
                assert call(d, a, dev=dev) == CRX_ERR_NOT_INIT, (d.N, d.N_ilqr, d.n_cars, dev)
        fd, a = abi.field_desc(N, C, S, 19.25), arrays()                     # the answer crx_field_prep gives a well-formed call
        lib.crx_field_prep.restype = ctypes.c_int
        field_names = ("track", "xcurv", "car_dims", "pred_s", "pred_ey", "obs_s", "obs_ey", "lap_off", "n_obs", "obs_dims", "clear")
        assert lib.crx_field_prep(ctypes.byref(fd), ctypes.c_int(R), *[p(a[k]) for k in field_names]) == CRX_ERR_NOT_INIT


def test_mixed_commit_refuses_bad_arguments_without_a_device(lib):
    import torch

    lib.crx_mixed_commit_dev.restype = ctypes.c_int
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    Bn, N, Ni = 5, 10, 20
    f = lambda *sh: np.ones(sh)   # noqa: E731
    i = lambda *sh: np.ones(sh, dtype=np.int32)   # noqa: E731

    def arrays():
        return dict(policy=i(Bn), x=f(Bn, 6), vt=f(Bn), eyt=f(Bn), K=f(Bn, 2, 6), xt=f(Bn, 6), U_nlp=f(Bn, N, 2), nlp_status=i(Bn), U_ilqr=f(Bn, Ni, 2),
                    ilqr_status=i(Bn), u=f(Bn, 2), ctrl_status=i(Bn))

    def call(a, batch=Bn, ns=2 * N, ils=2 * Ni):
        return lib.crx_mixed_commit_dev(ctypes.c_int(batch), p(a["policy"]), p(a["x"]), p(a["vt"]), p(a["eyt"]), p(a["K"]), p(a["xt"]), p(a["U_nlp"]),
                                        ctypes.c_int(ns), p(a["nlp_status"]), p(a["U_ilqr"]), ctypes.c_int(ils), p(a["ilqr_status"]), p(a["u"]),
                                        p(a["ctrl_status"]), None)

    assert call(arrays(), batch=-1) == CRX_ERR_ARG and b"batch" in lib.crx_last_error()
    for hole in ("policy", "x", "u", "ctrl_status"):
        assert call(dict(arrays(), **{hole: None})) == CRX_ERR_ARG and b"NULL" in lib.crx_last_error(), hole
    for half in ("vt", "eyt", "K", "xt", "U_nlp", "nlp_status", "U_ilqr", "ilqr_status"):   # a family comes whole
        assert call(dict(arrays(), **{half: None})) == CRX_ERR_ARG and b"go together" in lib.crx_last_error(), half
    assert call(arrays(), ns=1) == CRX_ERR_ARG and call(arrays(), ils=0) == CRX_ERR_ARG and b"stride" in lib.crx_last_error()
    if not torch.cuda.is_available():
        none = dict(vt=None, eyt=None, K=None, xt=None, U_nlp=None, nlp_status=None, U_ilqr=None, ilqr_status=None)
        for a, kw in ((arrays(), {}), (dict(arrays(), **none), dict(ns=0, ils=0)), (dict(arrays(), U_ilqr=None, ilqr_status=None), dict(ils=0))):
            assert call(a, **kw) == CRX_ERR_NOT_INIT


# ---- the loop's launch sequence ----------------------------------------------------------------------------------------------------------
class Recorder:
    """Stands in for crx.torch_api (the technique of tests/test_montecarlo_sequence_cpu.py): workspace classes and constants are the real
    ones; every `*_dev` wrapper and longest_first is recorded as (name, arguments by parameter name) and returns what its caller goes on with."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        import torch

        from crx import torch_api

        real = getattr(torch_api, name)
        if name == "CbfModels":
            return lambda desc, A, B: ("CbfModels", desc, A, B)
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
            return args.get("ws")

        return record

    def take(self):
        """The calls recorded since the last take(): (names, {name: arguments})."""
        calls, self.calls = self.calls, []
        return [n for n, _ in calls], dict(calls)


def test_mixed_races_step_is_five_launches(AB, monkeypatch):
    import torch

    from crx import abi, montecarlo

    rec = Recorder()
    monkeypatch.setattr(montecarlo, "torch_api", rec)
    R, C, N, Ni = 2, 4, 10, 20
    z = np.zeros((R, C, 6))
    vt = np.array([[1.0, 0.9, 0.8, 0.6]] * R)
    pol = [["mpccbf", "ilqr", "pid", "lqr"], ["mpc_lti", "none", "mpccbf", "ilqr"]]
    dims = np.full((R, C, 2), 0.3)
    r = montecarlo.MixedRaces(np.zeros((5, 6)), 20.0, 1.0, AB[0], AB[1], z, z, pol, vt=vt, eyt=0.1, N=N, ilqr_N=Ni, ilqr_max_iter=30, ilqr_obstacles=1,
                              device="cpu", car_dims=dims)
    names, args = rec.take()
    assert names == ["lqr_design_dev"]                                     # the LQR cars' gains, once, under their mask
    assert args["lqr_design_dev"]["active"].tolist() == [0, 0, 0, 1, 0, 0, 0, 0] and tuple(args["lqr_design_dev"]["A"].shape) == (R * C, 6, 6)
    assert r.batch == R * C and r.policy.dtype == torch.int32 and r.policy.tolist() == [4, 5, 1, 2, 3, 0, 4, 5]
    assert r.xt[:, 0].tolist() == [1.0, 0.9, 0.8, 0.6] * R and r.xt[:, 5].tolist() == [0.1] * (R * C) and r.vt.tolist() == r.xt[:, 0].tolist()
    assert (r.mdesc.N, r.mdesc.N_ilqr, r.mdesc.n_cars, r.mdesc.n_seg, r.mdesc.ilqr_obstacles) == (N, Ni, C, 5, 1)
    assert (r.desc.N, r.desc.n_obs_max, r.desc.margin) == (N, C - 1, 0.2) and (r.idesc.N, r.idesc.n_obs_max, r.idesc.max_iter) == (Ni, C - 1, 30)
    assert tuple(r.mws.pred_s.shape) == (R, C, Ni + 1) and tuple(r.mws.il_obs_s.shape) == (R * C, C - 1, Ni + 1) and r.mws.obs_dims is not None
    before = (r.xg, r.xc, r.xg_next, r.xc_next)
    r.mws.clear[:] = torch.arange(R * C, dtype=torch.float64)
    r.step()
    names, args = rec.take()
    assert names == ["mixed_prep_dev", "cbf_solve_dev", "ilqr_solve_dev", "mixed_commit_dev", "plant_step_wrap_dev"]
    prep, nlp, il, commit, plant = (args[n] for n in names)
    m = r.mws
    assert prep["desc"] is r.mdesc and prep["track"] is r.tab and prep["xcurv"] is before[1] and prep["policy"] is r.policy and prep["ws"] is m
    assert prep["car_dims"] is r.car_dims
    assert nlp["desc"] is r.desc and nlp["x0"] is before[1] and nlp["xt"] is r.xt and nlp["obs_s"] is m.obs_s and nlp["obs_ey"] is m.obs_ey
    assert nlp["lap_off"] is m.lap_off and nlp["n_obs"] is m.n_obs and nlp["obs_dims"] is m.obs_dims and nlp["active"] is m.m_nlp
    assert nlp["ws"] is r.ws and nlp["order"] is None and nlp["models"] is None
    assert il["desc"] is r.idesc and il["x0"] is before[1] and il["xt"] is r.xt and il["obs_s"] is m.il_obs_s and il["obs_ey"] is m.il_obs_ey
    assert il["lap_off"] is m.il_lap_off and il["n_obs"] is m.il_n_obs and il["active"] is m.m_ilqr and il["ws"] is r.iws and il["models"] is None
    assert commit["policy"] is r.policy and commit["x"] is before[1] and commit["u"] is r.u and commit["ctrl_status"] is r.status
    assert commit["pid"][0] is r.vt and commit["pid"][1] is r.eyt and commit["lqr"][0] is r.K and commit["lqr"][1] is r.xt
    assert commit["nlp"][0] is r.ws.U and commit["nlp"][1] is r.ws.status and commit["ilqr"][0] is r.iws.U and commit["ilqr"][1] is r.iws.status
    assert plant["u"] is r.u and plant["u_stride"] == 2 and plant["xcurv"] is before[1] and plant["xcurv_next"] is before[3]
    assert plant["desc"] is r.plant and plant["track"] is r.tab and plant["laps"] is r.laps
    assert r.xc is before[3] and r.xc_next is before[1] and r.xg is before[2]
    assert r.min_clear.tolist() == list(range(R * C))                      # the running minimum took this step's clear
    inp = r.stats_inputs()                                                 # the field form: RaceStats attaches unchanged
    assert inp["n_cars"] == C and inp["car_dims"] is r.car_dims and inp["xcurv"] is r.xc and (inp["l_sum"], inp["w_sum"]) == (0.4, 0.2)
    # longest_first goes ahead of the NLP launch, under its mask
    r.dispatch = "longest_first"
    r.step()
    names, args = rec.take()
    assert names == ["mixed_prep_dev", "longest_first", "cbf_solve_dev", "ilqr_solve_dev", "mixed_commit_dev", "plant_step_wrap_dev"]
    assert args["longest_first"]["iters"] is r.ws.iters and args["longest_first"]["active"] is m.m_nlp and args["cbf_solve_dev"]["order"] is not None
    # a mix without iLQR cars issues no ilqr_solve_dev and asks the prep for no iLQR arrays; its family reaches the commit as None
    q = montecarlo.MixedRaces(np.zeros((5, 6)), 20.0, 1.0, AB[0], AB[1], z, z, [["mpccbf", "pid", "mpc_lti", "none"]] * R, N=N, device="cpu",
                              models=(np.tile(AB[0], (R * C, 1, 1)), np.tile(AB[1], (R * C, 1, 1))))
    assert rec.take()[0] == [] and q.iws is None and q.idesc is None and q.K is None and q.mdesc.N_ilqr == 0 and q.mws.il_obs_s is None
    assert q.models[0] == "CbfModels" and q.models[1] is q.desc and tuple(q.models[2].shape) == (R * C, 6, 6)
    q.step()
    names, args = rec.take()
    assert names == ["mixed_prep_dev", "cbf_solve_dev", "mixed_commit_dev", "plant_step_wrap_dev"]
    assert args["mixed_commit_dev"]["ilqr"] is None and args["mixed_commit_dev"]["lqr"] is None and args["mixed_commit_dev"]["nlp"][0] is q.ws.U
    assert args["cbf_solve_dev"]["models"] is q.models and args["cbf_solve_dev"]["obs_dims"] is None
    # ... and one of PID and LQR cars alone issues no solver launch at all
    p = montecarlo.MixedRaces(np.zeros((5, 6)), 20.0, 1.0, AB[0], AB[1], z, z, [["pid", "lqr", "pid", "none"]] * R, device="cpu")
    assert rec.take()[0] == ["lqr_design_dev"] and p.ws is None and p.iws is None
    p.step()
    names, args = rec.take()
    assert names == ["mixed_prep_dev", "mixed_commit_dev", "plant_step_wrap_dev"] and args["mixed_commit_dev"]["nlp"] is None
    out = montecarlo.mixed_races(np.zeros((5, 6)), 20.0, 1.0, AB[0], AB[1], z, z, pol, 4, device="cpu", log_every=2, ilqr_N=Ni)
    assert list(out) == ["xcurv", "u", "status", "laps", "min_clear"]
    assert out["xcurv"].shape == (3, R * C, 6) and out["u"].shape == (2, R * C, 2) and out["status"].shape == (2, R * C)
    with pytest.raises(ValueError):
        montecarlo.MixedRaces(np.zeros((5, 6)), 20.0, 1.0, AB[0], AB[1], z, z, [["pid"] * 8] * R, device="cpu")
    with pytest.raises(ValueError):
        montecarlo.MixedRaces(np.zeros((5, 6)), 20.0, 1.0, AB[0], AB[1], z, z, [["pid", "lmpc", "pid", "pid"]] * R, device="cpu")
    assert abi.POLICY_NAMES == ("none", "pid", "lqr", "mpc_lti", "mpccbf", "ilqr")
