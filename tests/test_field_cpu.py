"""Field races without a GPU: the numpy model of crx_field_prep (tests/field_model.py) against what the reference's own driven model
predicted (tests/golden/field_pred.npz, recorded by tests/golden/tools/make_field_pred.py) and against the existing host route
(hostprep.cbf_window + hostprep.pack_obstacles) on the mirror's predictions; the argument refusals of crx_field_prep and the defaults of
crx_field_desc_default; the launch sequence of montecarlo.FieldRaces.step."""
import ctypes
import os

import numpy as np
import pytest

import conftest
import field_model as fm

CRX_ERR_ARG, CRX_ERR_NOT_INIT = -1, -4
TRACKS = ("l_shape", "m_shape")


def _track(name, width=0.8):
    from utils import racing_env

    return racing_env.ClosedTrack(np.genfromtxt(os.path.join(conftest.ROOT, "data/track_layout/%s.csv" % name), delimiter=","), track_width=width)


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(conftest.GOLDEN, "field_pred.npz"), allow_pickle=False)


def _groups(z):
    for name in (str(t) for t in z["tracks"]):
        for N in (12, 24):
            yield name, N, "%s_N%d" % (name, N)


def _mirror_car(track):
    from racing import offboard
    from utils import base

    car = offboard.DynamicBicycleModel(name="car", param=base.CarParam(), system_param=base.SystemParam())
    car.set_track(track)
    car.set_timestep(0.1)
    return car


def _mirror_predict(car, x, n):
    car.set_state_curvilinear(np.array(x, dtype=float))
    car.set_state_global(np.zeros(6))
    return car.get_trajectory_nsteps(n)[0]


def test_fixture_holds_the_stated_draw(fixture):
    assert [str(t) for t in fixture["tracks"]] == list(TRACKS)
    crossing = 0
    for name, N, g in _groups(fixture):
        x, ps = fixture[g + "/xcurv"], fixture[g + "/pred_s"]
        assert x.shape == ((64 if N == 12 else 16), 6) and ps.shape == (x.shape[0], N + 1) and fixture[g + "/pred_ey"].shape == ps.shape
        assert x[:, 0].min() >= 0.3 and x[:, 0].max() <= 2.0
        for col in (1, 2, 3, 5):
            assert (x[:, col] > 0).any() and (x[:, col] < 0).any() and (x[:, col] != 0).all(), (g, col)
        crossing += int((np.diff(np.concatenate([x[:, 4:5], ps], axis=1), axis=1) < 0).any(axis=1).sum())
    assert crossing >= 8
    assert os.path.getsize(os.path.join(conftest.GOLDEN, "field_pred.npz")) < 100 * 1024


def test_model_and_mirror_predictions_match_the_reference(fixture):
    """rtol = 0, atol = 1e-12: the bound the project grants this sin / cos Euler arithmetic in test_plant_step."""
    for name, N, g in _groups(fixture):
        track = _track(name)
        x = fixture[g + "/xcurv"]
        ps, pe, edge, cond = fm.predict(track.point_and_tangent, track.lap_length, x, N + 1)
        assert edge.min() >= 1e-9 and cond.min() >= 0.4, g               # the tool redrew anything closer to a joint or to the frame's singularity
        np.testing.assert_allclose(ps, fixture[g + "/pred_s"], rtol=0, atol=1e-12, err_msg=g)
        np.testing.assert_allclose(pe, fixture[g + "/pred_ey"], rtol=0, atol=1e-12, err_msg=g)
        car = _mirror_car(track)
        for i in range(x.shape[0]):
            xc = _mirror_predict(car, x[i], N + 1)
            np.testing.assert_allclose(xc[4], fixture[g + "/pred_s"][i], rtol=0, atol=1e-12, err_msg=g)
            np.testing.assert_allclose(xc[5], fixture[g + "/pred_ey"][i], rtol=0, atol=1e-12, err_msg=g)
            np.testing.assert_allclose(xc[3], fixture[g + "/pred_epsi"][i], rtol=0, atol=1e-12, err_msg=g)
            assert np.array_equal(xc[0:3], np.repeat(x[i, 0:3, None], N + 1, axis=1))


def draw_races(rng, L, R, C, spread=6.0):
    """R races of C cars bunched within `spread` metres of a point drawn over the lap (so that windows fill, and some bunches straddle the
    line), each car a full state with vy, wz, epsi, ey of both signs."""
    x = np.zeros((R, C, 6))
    x[..., 0] = rng.uniform(0.3, 2.0, (R, C))
    x[..., 1] = rng.uniform(-0.2, 0.2, (R, C))
    x[..., 2] = rng.uniform(-0.6, 0.6, (R, C))
    x[..., 3] = rng.uniform(-0.3, 0.3, (R, C))
    x[..., 4] = (rng.uniform(0.0, L, (R, 1)) + rng.uniform(0.0, spread, (R, C))) % L
    x[..., 5] = rng.uniform(-0.6, 0.6, (R, C))
    return x


def test_model_window_packing_dims_match_the_host_route():
    """200 drawn races at C = 4: the model's second half on the MIRROR's predictions against hostprep.cbf_window + pack_obstacles, one NLP at
    a time as control.mpccbf calls them: integer outputs equal, doubles bit-equal."""
    from crx import hostprep

    R, C, N = 200, 4, 10
    V = C - 1
    track = _track("l_shape")
    L = track.lap_length
    rng = np.random.default_rng(31)
    x = draw_races(rng, L, R, C)
    x[:50, :, 4] += L * rng.integers(0, 3, (50, C))           # cars that carry whole laps in s: non-zero lap offsets
    dims = np.stack([rng.uniform(0.3, 0.5, (R, C)), rng.uniform(0.15, 0.25, (R, C))], axis=-1)
    car = _mirror_car(track)
    pred = np.array([[_mirror_predict(car, x[r, c], N + 1) for c in range(C)] for r in range(R)])   # [R, C, 6, N+1]
    ps, pe = pred[:, :, 4], pred[:, :, 5]
    m = fm.obstacles(ps, pe, x, L, car_dims=dims)
    assert m["n_obs"].dtype == np.int32 and set(np.unique(m["n_obs"])) == set(range(C))   # every count 0 .. V occurs
    assert (m["lap_off"] != 0).any()
    oth = fm.others(C)
    for e in range(C):
        keep, off = hostprep.cbf_window(x[:, e], ps[:, oth[e], 0], L)
        pair = np.stack([dims[:, e, None, 0] / 2 + dims[:, oth[e], 0] / 2, dims[:, e, None, 1] / 2 + dims[:, oth[e], 1] / 2], axis=-1)
        hs, he, ho, hn, hd = hostprep.pack_obstacles(keep, ps[:, oth[e]], pe[:, oth[e]], off, V, ego_s=x[:, e, 4], dims=pair)
        assert np.array_equal(m["n_obs"][:, e], hn)
        assert np.array_equal(m["obs_s"][:, e], hs) and np.array_equal(m["obs_ey"][:, e], he) and np.array_equal(m["lap_off"][:, e], ho)
        live = np.arange(V) < hn[:, None]
        assert np.array_equal(m["obs_dims"][:, e][live], hd[live])                         # the host route pads with ones,
        assert (m["obs_dims"][:, e][~live] == 0.0).all()                                   # crx_field_prep with zeros


def test_model_clear_is_the_host_expression():
    """`clear` of the model against the expression of tests/test_gpu_closed_loop.py:167-170, pair by pair."""
    rng = np.random.default_rng(32)
    L = 19.25
    x = draw_races(rng, L, 20, 3)
    c = fm.clear(x, L)
    for r in range(20):
        for e in range(3):
            vals = []
            for o in range(3):
                if o != e:
                    ds = (x[r, e, 4] - x[r, o, 4] + 0.5 * L) % L - 0.5 * L
                    vals.append((ds / 0.4) ** 6 + ((x[r, e, 5] - x[r, o, 5]) / 0.2) ** 6)
            np.testing.assert_allclose(c[r, e], min(vals), rtol=1e-12, atol=0)   # (numpy's scalar and array powers differ in the last bit)
    assert np.isinf(fm.clear(x[:, :1], L)).all()
    x[0, 1] = np.nan                                         # a NaN car: its own value is +inf, nobody else's changes through it
    c2 = fm.clear(x, L)
    assert np.isinf(c2[0, 1]) and np.isfinite(c2[0, [0, 2]]).all() and np.array_equal(c2[1:], c[1:])


# ---- the C ABI without a device ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import crx

    return crx.lib()


def test_symbols_and_default_descriptor(lib):
    from crx import abi

    src = open(os.path.join(conftest.ROOT, "include", "crx.h")).read()
    for n in ("crx_field_desc_default", "crx_field_prep", "crx_field_prep_dev"):
        assert hasattr(lib, n) and n + "(" in src, n
    d = abi.FieldDesc()
    lib.crx_field_desc_default(ctypes.byref(d), 12, 4, 9, ctypes.c_double(19.25))
    assert bytes(d) == bytes(abi.field_desc(12, 4, 9, 19.25))
    assert (d.N, d.n_cars, d.n_seg, d.degree) == (12, 4, 9, 6)
    assert (d.lap_length, d.dt, d.safety_time, d.l_sum, d.w_sum) == (19.25, 0.1, 2.0, 0.4, 0.2)
    assert lib.crx_version() == 400


def test_field_prep_refuses_bad_arguments_without_a_device(lib):
    import torch

    from crx import abi

    lib.crx_field_prep.restype = ctypes.c_int
    lib.crx_field_prep_dev.restype = ctypes.c_int
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    R, C, N, S = 3, 4, 10, 9
    V = C - 1
    f = lambda *sh: np.ones(sh)   # noqa: E731
    names = ("track", "xcurv", "car_dims", "pred_s", "pred_ey", "obs_s", "obs_ey", "lap_off", "n_obs", "obs_dims", "clear")

    def arrays(C=C):
        V = C - 1
        return dict(track=f(S, 6), xcurv=f(R, C, 6), car_dims=f(R, C, 2), pred_s=f(R, C, N + 1), pred_ey=f(R, C, N + 1), obs_s=f(R, C, V, N + 1),
                    obs_ey=f(R, C, V, N + 1), lap_off=f(R, C, V), n_obs=np.zeros((R, C), dtype=np.int32), obs_dims=f(R, C, V, 2), clear=f(R, C))

    def call(d, a, n_races=R, dev=False):
        ptrs = [p(a[k]) for k in names]
        if dev:
            return lib.crx_field_prep_dev(ctypes.byref(d) if d is not None else None, ctypes.c_int(n_races), *ptrs, None)
        return lib.crx_field_prep(ctypes.byref(d) if d is not None else None, ctypes.c_int(n_races), *ptrs)

    def refused(d, a, what, **kw):
        for dev in (False, True):
            assert call(d, a, dev=dev, **kw) == CRX_ERR_ARG, (what, dev)
            assert lib.crx_last_error(), what

    good = lambda **kw: abi.field_desc(N, C, S, 19.25, **kw)   # noqa: E731
    refused(None, arrays(), "desc")
    for bad_N in (0, -1, abi.CRX_MAX_N + 1):
        refused(abi.field_desc(bad_N, C, S, 19.25), arrays(), "N")
        assert b"N=" in lib.crx_last_error()
    for bad_C in (0, abi.CRX_MAX_OBS + 2):
        refused(abi.field_desc(N, bad_C, S, 19.25), arrays(), "n_cars")
        assert b"n_cars" in lib.crx_last_error()
    for bad_S in (0, 65):
        refused(abi.field_desc(N, C, bad_S, 19.25), arrays(), "n_seg")
        assert b"n_seg" in lib.crx_last_error()
    for bad in (0.0, -1.0, np.inf, np.nan):
        refused(abi.field_desc(N, C, S, bad), arrays(), "lap_length")
        for key in ("dt", "l_sum", "w_sum"):
            refused(good(**{key: bad}), arrays(), key)
    for bad in (0, 3, 10):                                                  # the exponent of `clear`: 2, 4, 6 or 8, as crx_cbf_desc's
        refused(good(degree=bad), arrays(), "degree")
    refused(good(), arrays(), "n_races", n_races=-1)
    assert b"n_races" in lib.crx_last_error()
    for hole in ("track", "xcurv", "pred_s", "pred_ey", "obs_s", "obs_ey", "lap_off", "n_obs"):
        refused(good(), dict(arrays(), **{hole: None}), hole)
        assert b"NULL" in lib.crx_last_error()
    for hole in ("car_dims", "obs_dims"):                                   # both or neither
        refused(good(), dict(arrays(), **{hole: None}), hole)
        assert b"go together" in lib.crx_last_error()
    for bad in (0.0, -0.4, np.inf, np.nan):                                 # the host entry reads the rows
        a = arrays()
        a["car_dims"][1, 2, 1] = bad
        assert call(good(), a) == CRX_ERR_ARG and b"car_dims" in lib.crx_last_error()
    # what may be NULL: clear; car_dims with obs_dims; with one car the obs_* / lap_off arrays.  Well-formed calls get as far as the library's
    # state: without a device CRX_ERR_NOT_INIT, never a computation
    if not torch.cuda.is_available():
        one = arrays(C=1)
        for d, a in ((good(), arrays()), (good(), dict(arrays(), clear=None)), (good(), dict(arrays(), car_dims=None, obs_dims=None)),
                     (abi.field_desc(N, 1, S, 19.25), dict(one, obs_s=None, obs_ey=None, lap_off=None, obs_dims=None)),
                     (abi.field_desc(1, C, 1, 19.25), arrays()), (abi.field_desc(abi.CRX_MAX_N, abi.CRX_MAX_OBS + 1, 64, 19.25), arrays(C=abi.CRX_MAX_OBS + 1))):
            for dev in (False, True):
                assert call(d, a, dev=dev) == CRX_ERR_NOT_INIT, (d.N, d.n_cars, dev)


# ---- the loop's launch sequence (the stand-in of tests/test_montecarlo_sequence_cpu.py) ---------------------------------------------------
def test_field_races_step_is_three_launches(AB, monkeypatch):
    import torch

    from crx import montecarlo
    from test_montecarlo_sequence_cpu import Recorder

    rec = Recorder()
    monkeypatch.setattr(montecarlo, "torch_api", rec)
    R, C, N = 2, 3, 10
    z = np.zeros((R, C, 6))
    vt = np.array([[1.0, 0.8, 0.6]] * R)
    r = montecarlo.FieldRaces(np.zeros((5, 6)), 20.0, 1.0, AB[0], AB[1], z, z, C, vt=vt, N=N, device="cpu", car_dims=np.full((R, C, 2), 0.3))
    assert rec.take()[0] == []
    assert r.batch == R * C and tuple(r.xt.shape) == (R * C, 6) and r.xt[:, 0].tolist() == [1.0, 0.8, 0.6] * R
    assert (r.desc.N, r.desc.n_obs_max, r.desc.margin) == (N, C - 1, 0.2) and (r.fdesc.n_cars, r.fdesc.n_seg) == (C, 5)
    before = (r.xg, r.xc, r.xg_next, r.xc_next)
    r.fws.clear[:] = torch.arange(R * C, dtype=torch.float64)
    r.step()
    names, args = rec.take()
    assert names == ["field_prep_dev", "cbf_solve_dev", "plant_step_wrap_dev"]
    prep, solve, plant = (args[n] for n in names)
    assert prep["desc"] is r.fdesc and prep["track"] is r.tab and prep["xcurv"] is before[1] and prep["ws"] is r.fws and prep["car_dims"] is r.car_dims
    assert solve["x0"] is before[1] and solve["obs_s"] is r.fws.obs_s and solve["obs_ey"] is r.fws.obs_ey and solve["lap_off"] is r.fws.lap_off
    assert solve["n_obs"] is r.fws.n_obs and solve["obs_dims"] is r.fws.obs_dims and solve["order"] is None and solve["models"] is None
    assert plant["u"] is r.ws.U and plant["u_stride"] == 2 * N and plant["xcurv"] is before[1] and plant["xcurv_next"] is before[3]
    assert r.xc is before[3] and r.xc_next is before[1]
    assert r.min_clear.tolist() == list(range(R * C))                      # the running minimum took this step's clear
    out = montecarlo.field_races(np.zeros((5, 6)), 20.0, 1.0, AB[0], AB[1], z, z, C, 4, device="cpu", log_every=2)
    assert list(out) == ["xcurv", "u", "status", "iters", "n_obs", "laps", "min_clear"]
    assert out["xcurv"].shape == (3, R * C, 6) and out["u"].shape == (2, R * C, 2) and out["n_obs"].shape == (2, R * C)
    assert out["laps"].shape == (R * C,) and out["min_clear"].shape == (R * C,)
