"""Field races and mixed fields on one track per race, without a GPU: the launch sequence of FieldRaces / MixedRaces / RaceStats built with
tracks= / race_track= (the stand-in of tests/test_montecarlo_sequence_cpu.py), what they refuse, the host entries' argument checks, and -- on
the numpy models alone -- that the inputs of the GPU suite (tests/field_tracks_cases.py) would expose a kernel that folded every race by
track 0's lap length."""
import ctypes as C

import numpy as np
import pytest
import torch

import field_tracks_cases as cases
import plant_tracks_ref as ref
from test_montecarlo_sequence_cpu import Recorder

WIDTH = 1.0
CRX_ERR_ARG = -1


@pytest.fixture(scope="module")
def TS():
    return ref.track_set()


@pytest.fixture(scope="module")
def lib():
    import crx

    return crx.lib()


@pytest.fixture
def rec(monkeypatch):
    from crx import montecarlo

    r = Recorder()
    monkeypatch.setattr(montecarlo, "torch_api", r)
    return r


def _field(AB, TS, race_track, R=4, Cn=3, **kw):
    from crx import montecarlo

    z = np.zeros((R, Cn, 6))
    return montecarlo.FieldRaces(None, None, WIDTH, AB[0], AB[1], z, z, Cn, device="cpu", tracks=TS, race_track=race_track, **kw)


def _mixed(AB, TS, race_track, pol, **kw):
    from crx import montecarlo

    z = np.zeros(np.shape(pol) + (6,))
    return montecarlo.MixedRaces(None, None, WIDTH, AB[0], AB[1], z, z, pol, device="cpu", ilqr_N=20, tracks=TS, race_track=race_track, **kw)


def _check_set(loop, TS, race_track, Cn):
    ts = loop.tracks
    assert ts.host is TS and ts.race_track.dtype == torch.int32 and ts.race_track.tolist() == list(race_track)
    assert ts.track_id.dtype == torch.int32 and ts.track_id.tolist() == np.repeat(race_track, Cn).tolist()
    assert np.array_equal(ts.car_lap.numpy(), TS.lap_length[np.repeat(race_track, Cn)]) and loop.lap_length is ts.car_lap and loop.tab is ts.tracks
    # the descriptors carry track 0's geometry, only to be valid ones
    assert (loop.fd.n_seg, loop.fd.lap_length) == (int(TS.n_seg[0]), float(TS.lap_length[0]))
    assert (loop.plant.n_seg, loop.plant.lap_length) == (int(TS.n_seg[0]), float(TS.lap_length[0]))


@pytest.mark.parametrize("ids", [[3, 1, 0, 2], torch.tensor([0, 0, 3, 3], dtype=torch.int64)])
def test_field_races_on_a_track_set(rec, AB, TS, ids):
    race_track = [int(i) for i in ids]
    r = _field(AB, TS, ids)
    assert rec.take()[0] == []
    _check_set(r, TS, race_track, 3)
    before = (r.xg, r.xc, r.xg_next, r.xc_next)
    r.step()
    names, args = rec.take()
    assert names == ["field_prep_tracks_dev", "cbf_solve_dev", "plant_step_tracks_wrap_dev"]
    prep, solve, plant = (args[n] for n in names)
    assert prep["desc"] is r.fdesc and prep["track_set"] is r.tracks and prep["xcurv"] is before[1] and prep["ws"] is r.fws and prep["car_dims"] is None
    assert solve["x0"] is before[1] and solve["obs_s"] is r.fws.obs_s and solve["n_obs"] is r.fws.n_obs
    assert plant["tracks"] is r.tracks and plant["tracks"].track_id.tolist() == np.repeat(race_track, 3).tolist()
    assert plant["u"] is r.ws.U and plant["xcurv"] is before[1] and plant["xcurv_next"] is before[3] and plant["laps"] is r.laps
    assert r.xc is before[3] and r.xc_next is before[1]


def test_mixed_races_on_a_track_set(rec, AB, TS):
    pol = [["mpccbf", "ilqr", "pid"], ["lqr", "mpc_lti", "mpccbf"]]
    r = _mixed(AB, TS, [2, 1], pol)
    assert rec.take()[0] == ["lqr_design_dev"]
    _check_set(r, TS, [2, 1], 3)
    before = (r.xg, r.xc, r.xg_next, r.xc_next)
    r.step()
    names, args = rec.take()
    assert names == ["mixed_prep_tracks_dev", "cbf_solve_dev", "ilqr_solve_dev", "mixed_commit_dev", "plant_step_tracks_wrap_dev"]
    prep, plant = args["mixed_prep_tracks_dev"], args["plant_step_tracks_wrap_dev"]
    assert prep["desc"] is r.mdesc and prep["track_set"] is r.tracks and prep["xcurv"] is before[1] and prep["policy"] is r.policy and prep["ws"] is r.mws
    assert plant["tracks"] is r.tracks and plant["tracks"].track_id.tolist() == [2, 2, 2, 1, 1, 1] and plant["u"] is r.u and plant["u_stride"] == 2
    assert r.xc is before[3]


def test_without_the_new_arguments_the_sequences_are_the_parents(rec, AB):
    from crx import montecarlo

    tab, z = np.zeros((5, 6)), np.zeros((2, 3, 6))
    f = montecarlo.FieldRaces(tab, 20.0, WIDTH, AB[0], AB[1], z, z, 3, device="cpu")
    m = montecarlo.MixedRaces(tab, 20.0, WIDTH, AB[0], AB[1], z, z, [["mpccbf", "ilqr", "pid"], ["lqr", "mpc_lti", "mpccbf"]], device="cpu")
    rec.take()
    assert f.tracks is None and m.tracks is None and f.lap_length == 20.0 and (f.fd.n_seg, f.fd.lap_length) == (5, 20.0)
    f.step()
    names, args = rec.take()
    assert names == ["field_prep_dev", "cbf_solve_dev", "plant_step_wrap_dev"] and args["field_prep_dev"]["track"] is f.tab
    m.step()
    assert rec.take()[0] == ["mixed_prep_dev", "cbf_solve_dev", "ilqr_solve_dev", "mixed_commit_dev", "plant_step_wrap_dev"]
    st = montecarlo.RaceStats(f)
    st.step()
    assert rec.take()[0] == ["race_stats_reset_dev", "field_prep_dev", "cbf_solve_dev", "plant_step_wrap_dev", "race_stats_dev"] and st.car_lap is None


def test_race_stats_samples_a_track_set_loop_with_the_cars_laps(rec, AB, TS):
    from crx import montecarlo

    dims = np.full((4, 3, 2), 0.3)
    r = _field(AB, TS, [3, 1, 0, 2], car_dims=dims)
    rec.take()
    st = montecarlo.RaceStats(r)
    names, args = rec.take()
    assert names == ["race_stats_reset_dev"] and args["race_stats_reset_dev"]["laps"] is r.laps
    assert (st.desc.n_opp_max, st.desc.n_cars, st.desc.lap_length, st.desc.track_width) == (2, 3, float(TS.lap_length[0]), WIDTH)
    st.update()
    st.step()
    names, args = rec.take()
    assert names == ["race_stats_laps_dev", "field_prep_tracks_dev", "cbf_solve_dev", "plant_step_tracks_wrap_dev", "race_stats_laps_dev"]
    call = args["race_stats_laps_dev"]
    assert call["lap_length"] is r.tracks.car_lap and call["desc"] is st.desc and call["ws"] is st.ws and call["sample"] == 1
    assert call["xcurv"] is r.xc and call["laps"] is r.laps and call["car_dims"] is r.car_dims and call["xt"] is r.xt and call["car_s0"] is None
    m = _mixed(AB, TS, [2, 1], [["mpccbf", "ilqr", "pid"], ["lqr", "mpc_lti", "mpccbf"]])
    rec.take()
    sm = montecarlo.RaceStats(m)
    sm.step()
    names, args = rec.take()
    assert names[0] == "race_stats_reset_dev" and names[-2:] == ["plant_step_tracks_wrap_dev", "race_stats_laps_dev"]
    assert args["race_stats_laps_dev"]["lap_length"] is m.tracks.car_lap


def test_refusals_name_the_argument(rec, AB, TS):
    from crx import montecarlo

    tab, z = np.zeros((5, 6)), np.zeros((4, 3, 6))
    with pytest.raises(ValueError, match=r"race_track: expected shape \(4,\)"):
        _field(AB, TS, [0, 1, 2])
    with pytest.raises(ValueError, match="race_track: expected an integer"):
        _field(AB, TS, np.array([0.0, 1.0, 2.0, 3.0]))
    with pytest.raises(ValueError, match="race_track: expected an integer"):
        _field(AB, TS, np.zeros((4, 1), dtype=np.int32))
    for bad in ([0, 1, 2, 4], [0, -1, 2, 3]):
        with pytest.raises(ValueError, match=r"race_track: values outside \[0, 4\)"):
            _field(AB, TS, bad)
    for cls, last in ((montecarlo.FieldRaces, 3), (montecarlo.MixedRaces, [["pid"] * 3] * 4)):
        name = cls.__name__
        with pytest.raises(ValueError, match="%s: tracks= and race_track= go together" % name):      # race_track without tracks
            cls(tab, 20.0, WIDTH, AB[0], AB[1], z, z, last, device="cpu", race_track=[0, 1, 2, 3])
        with pytest.raises(ValueError, match="%s: tracks= and race_track= go together" % name):      # tracks without race_track
            cls(None, None, WIDTH, AB[0], AB[1], z, z, last, device="cpu", tracks=TS)
        with pytest.raises(ValueError, match="with tracks= the loop has no track_table"):
            cls(tab, 20.0, WIDTH, AB[0], AB[1], z, z, last, device="cpu", tracks=TS, race_track=[0, 1, 2, 3])
        with pytest.raises(ValueError, match="%s runs on one track" % name):                          # the per-car keyword stays refused
            cls(None, None, WIDTH, AB[0], AB[1], z, z, last, device="cpu", tracks=TS, track_id=np.zeros(12, dtype=np.int32))
        with pytest.raises(ValueError, match="%s runs on one track" % name):
            cls(None, None, WIDTH, AB[0], AB[1], z, z, last, device="cpu", tracks=TS, track_id=np.zeros(12, dtype=np.int32), race_track=[0, 1, 2, 3])
    assert rec.take()[0] == []                                                                         # ... before anything was launched
    # RaceStats keeps refusing the per-car loops on a set
    cars = np.full((3, 2), 3.0), np.full((3, 2), 0.2), np.zeros((3, 2))
    per_car = montecarlo.MpccbfRaces(None, None, WIDTH, AB[0], AB[1], np.zeros((3, 6)), np.zeros((3, 6)), *cars, device="cpu", tracks=TS,
                                     track_id=[0, 1, 2])
    with pytest.raises(ValueError, match="RaceStats takes one lap length"):
        montecarlo.RaceStats(per_car)
    # the wrapper itself
    from crx import abi, torch_api

    ws = torch_api.RaceStatsWorkspace(abi.stats_desc(2, 3, 20.0, WIDTH), 12, "cpu")
    with pytest.raises(ValueError, match="lap_length"):
        torch_api.race_stats_laps_dev(abi.stats_desc(2, 3, 20.0, WIDTH), 0, 0.0, torch.zeros(12, 6), torch.zeros(12, dtype=torch.int32), ws)


def test_run_to_the_end_functions_pass_the_set_through(rec, AB, TS):
    from crx import montecarlo

    z = np.zeros((4, 3, 6))
    out = montecarlo.field_races(None, None, WIDTH, AB[0], AB[1], z, z, 3, 2, device="cpu", tracks=TS, race_track=[0, 1, 2, 3])
    assert rec.take()[0] == ["field_prep_tracks_dev", "cbf_solve_dev", "plant_step_tracks_wrap_dev"] * 2 and out["xcurv"].shape == (3, 12, 6)
    out = montecarlo.mixed_races(None, None, WIDTH, AB[0], AB[1], z, z, [["mpccbf", "pid", "pid"]] * 4, 2, device="cpu", tracks=TS,
                                 race_track=[0, 1, 2, 3])
    assert rec.take()[0] == ["mixed_prep_tracks_dev", "cbf_solve_dev", "mixed_commit_dev", "plant_step_tracks_wrap_dev"] * 2
    assert out["u"].shape == (2, 12, 2)


# ---- the host entries' argument checks: no device is needed to be refused ---------------------------------------------------------------------
def _host_call(lib, entry, TS, race_track, n_seg=None, lap=None, n_tracks=None, seg_stride=None, R=2, Cn=2, N=4):
    from crx import abi

    mixed = entry == "crx_mixed_prep_tracks"
    d = abi.mixed_desc(N, 0, Cn, 5, 20.0) if mixed else abi.field_desc(N, Cn, 5, 20.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    tab = np.ascontiguousarray(TS.tracks)
    n_seg = np.ascontiguousarray(TS.n_seg if n_seg is None else n_seg, dtype=np.int32)
    lap = np.ascontiguousarray(TS.lap_length if lap is None else lap, dtype=np.float64)
    rt = np.ascontiguousarray(race_track, dtype=np.int32)
    x = np.zeros((R * Cn, 6))
    f = lambda *s: np.zeros(s)   # noqa: E731
    i = lambda *s: np.zeros(s, dtype=np.int32)   # noqa: E731
    V, N1 = Cn - 1, N + 1
    keep = [tab, n_seg, lap, rt, x, i(R * Cn), f(R * Cn, N1), f(R * Cn, N1), f(R * Cn, V, N1), f(R * Cn, V, N1), f(R * Cn, V), i(R * Cn), i(R * Cn)]
    head = [C.byref(d), C.c_int(R), C.c_int(TS.n_tracks if n_tracks is None else n_tracks), C.c_int(TS.seg_stride if seg_stride is None else seg_stride),
            p(tab), p(n_seg), p(lap), p(rt), p(x)]
    out = [p(a) for a in keep[6:12]]
    fn = getattr(lib, entry)
    fn.restype = C.c_int
    if mixed:
        rc = fn(*head, p(keep[5]), None, *out, None, p(keep[12]), None, None, None, None, None, None)
    else:
        rc = fn(*head, None, *out, None, None)
    lib.crx_last_error.restype = C.c_char_p
    return rc, (lib.crx_last_error() or b"").decode()


@pytest.mark.parametrize("entry", ["crx_field_prep_tracks", "crx_mixed_prep_tracks"])
def test_host_entries_refuse_a_bad_set_naming_the_offender(lib, TS, entry):
    from crx import abi

    for name in ("crx_field_prep_tracks", "crx_field_prep_tracks_dev", "crx_mixed_prep_tracks", "crx_mixed_prep_tracks_dev", "crx_race_stats_laps_dev"):
        assert hasattr(lib, name), name
    bad_seg, bad_lap = TS.n_seg.copy(), TS.lap_length.copy()
    bad_seg[2], bad_lap[3] = TS.seg_stride + 1, np.inf
    zero_seg, neg_lap = TS.n_seg.copy(), TS.lap_length.copy()
    zero_seg[1], neg_lap[0] = 0, -1.0
    for kw, msg in ((dict(race_track=[0, 4]), "race_track of race 1: 4 outside [0,4)"),
                    (dict(race_track=[-1, 0]), "race_track of race 0: -1 outside [0,4)"),
                    (dict(race_track=[0, 1], n_seg=bad_seg), "n_seg of track 2: %d outside [1,%d]" % (TS.seg_stride + 1, TS.seg_stride)),
                    (dict(race_track=[0, 1], n_seg=zero_seg), "n_seg of track 1: 0 outside [1,%d]" % TS.seg_stride),
                    (dict(race_track=[0, 1], lap=bad_lap), "lap_length of track 3 must be positive and finite"),
                    (dict(race_track=[0, 1], lap=neg_lap), "lap_length of track 0 must be positive and finite"),
                    (dict(race_track=[0, 1], n_tracks=abi.CRX_MAX_TRACKS + 1), "n_tracks=%d outside [1,%d]" % (abi.CRX_MAX_TRACKS + 1, abi.CRX_MAX_TRACKS)),
                    (dict(race_track=[0, 1], seg_stride=65), "seg_stride=65 outside [1,64]")):
        rc, err = _host_call(lib, entry, TS, **kw)
        assert rc == CRX_ERR_ARG and msg in err, (kw, rc, err)


# ---- the GPU suite's inputs, on the models alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [3, 7])
def test_the_cases_tell_a_races_own_lap_from_track_0s(Cn):
    """Test a of tests/test_gpu_field_tracks.py asserts on its inputs that a kernel using track 0's lap for every race could not pass; here the
    models say what would change: at least one n_obs or lap_off, and the rows that wrap."""
    N = 10
    ts, rt, x, dims = cases.field_case(Cn, N)
    assert np.array_equal(rt, np.arange(len(rt)) % 4) and len(rt) > 256 // Cn and len(rt) % (256 // Cn) >= 2
    own = cases.field_model(ts, rt, x, N, dims)
    wrong = cases.field_model(ts, rt, x, N, dims, laps=np.full(4, ts.lap_length[0]))
    on0 = rt == 0
    for k in ("pred_s", "obs_s", "lap_off", "n_obs", "clear"):
        assert np.array_equal(own[k][on0], wrong[k][on0], equal_nan=True), k
    differs = (own["n_obs"] != wrong["n_obs"]) | (own["lap_off"] != wrong["lap_off"]).any(axis=-1)
    assert differs[~on0].any()
    print("C = %d: egos whose n_obs or lap_off changes under track 0's lap: %d of %d" % (Cn, int(differs.sum()), differs.size))
    long_track = (rt == 1) | (rt == 3)                                   # m_shape, ellipse: longer than l_shape
    with np.errstate(invalid="ignore"):
        assert (x[long_track][..., 4] > ts.lap_length[0]).any()
    L_r = ts.lap_length[rt]
    jumps = np.diff(own["obs_s"], axis=-1) < -0.5 * L_r[:, None, None, None]
    assert jumps[rt != 0].any()                                          # a kept row that wraps at its own L
