"""One track per car, the parts that need no GPU: (1) the oracle reproduces the reference's own get_curvature + vehicle_dynamics on all four
layouts, across every segment joint (tests/golden/plant_tracks.npz, tests/golden/tools/make_plant_tracks.py), which makes "the oracle at
batch 1 on table track_id[b]" the per-car reference of tests/test_gpu_plant_tracks.py; (2) abi.track_set and synth.fleet_tracks; (3) PidLaps,
LqrLaps and MpccbfRaces hand a track set to the plant launch (and MpccbfRaces launches the per-race prep), launch what they launched before
without one, and every other loop and RaceStats refuse one by name; (4) the inputs of the GPU suite's wrap test."""
import os

import numpy as np
import pytest
import torch

import conftest
import plant_params_ref as pref
import plant_tracks_ref as ref
from test_montecarlo_sequence_cpu import BN, LAP, N_LMPC, TAB, WIDTH, Recorder, _cars, _lmpc_inputs, _plant_pairs

from crx import abi, montecarlo, synth


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(conftest.GOLDEN, "plant_tracks.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def TS():
    return ref.track_set()


class TracksRecorder(Recorder):
    """The stand-in of test_montecarlo_sequence_cpu; plant_step_tracks_dev returns states, as its plant_step_dev does."""

    def __getattr__(self, name):
        record = super().__getattr__(name)
        if name != "plant_step_tracks_dev":
            return record

        def record_and_return(*a, **kw):
            record(*a, **kw)
            args = self.calls[-1][1]
            return args["xglob"].clone(), args["xcurv"].clone()

        return record_and_return


@pytest.fixture
def rec(monkeypatch):
    r = TracksRecorder()
    monkeypatch.setattr(montecarlo, "torch_api", r)
    return r


# ---- 1. the oracle on every layout ----------------------------------------------------------------------------------------------------
def test_fixture_covers_every_joint_of_every_track(G, TS):
    assert tuple(str(n) for n in G["names"]) == ref.NAMES
    assert [G["t%d/table" % t].shape[0] for t in range(4)] == [7, 11, 11, 9]
    np.testing.assert_allclose(G["lap_length"], [19.2296, 49.8402, 19.1313, 25.4248], rtol=0, atol=5e-5)
    for t in range(4):
        tab = G["t%d/table" % t]
        n_seg = tab.shape[0]
        # the mirror builds the table the reference builds
        assert np.array_equal(TS.table(t), tab) and TS.lap_length[t] == G["lap_length"][t] and TS.n_seg[t] == n_seg
        ends = tab[:, 3] + tab[:, 4]
        assert abs(ends[-1] - G["lap_length"][t]) < 1e-9
        j = G["t%d/joint/joint" % t]
        assert np.array_equal(np.sort(j), np.arange(n_seg))                                    # every joint, the finish line included
        s0, s1 = G["t%d/joint/xcurv" % t][:, 4], G["t%d/joint/xcurv_next" % t][:, 4]
        np.testing.assert_allclose(ends[j] - s0, 0.03, rtol=0, atol=1e-12)
        assert (s1 > ends[j] + 0.02).all()                                                      # ... and the step crosses it
        vx = G["t%d/joint/xcurv" % t][:, 0]
        assert (vx >= 0.75).all() and (vx <= 0.85).all()
        seg = G["t%d/sub/seg" % t]
        assert (np.bincount(seg, minlength=n_seg) == 3).all()                                   # three states inside every segment
        s = G["t%d/sub/xcurv" % t][:, 4]
        assert (s > tab[seg, 3]).all() and (s < ends[seg]).all()
        assert np.array_equal(G["t%d/sub/curv" % t], tab[seg, 5])
        for P in (G["t%d/joint/params" % t], G["t%d/sub/params" % t]):                         # even rows the default car, odd rows another
            assert (P[0::2] == abi.plant_params(1)[0]).all() and (P[1::2] != abi.plant_params(1)[0]).all()


@pytest.mark.parametrize("t", range(4))
def test_oracle_control_steps_across_the_joints(orc, G, TS, t):
    """One control step (100 sub-steps) across every joint of layout t, odd rows on non-default parameters: the bound
    tests/test_plant_params_cpu.py holds a control step to."""
    k = "t%d/joint/" % t
    d = abi.plant_desc(int(TS.n_seg[t]), float(TS.lap_length[t]))
    assert d.n_sub == 100
    og, oc = pref.oracle_cars(orc, d, TS.table(t), G[k + "xglob"], G[k + "xcurv"], G[k + "u"], G[k + "params"])
    print("oracle, %s: %d control steps across the joints, worst deviation %.3g" % (
        ref.NAMES[t], og.shape[0], max(np.abs(og - G[k + "xglob_next"]).max(), np.abs(oc - G[k + "xcurv_next"]).max())))
    np.testing.assert_allclose(oc, G[k + "xcurv_next"], rtol=0, atol=1e-13)
    np.testing.assert_allclose(og, G[k + "xglob_next"], rtol=0, atol=1e-13)
    # the helper of the GPU tests says the same, through the padded set
    ids = np.full(og.shape[0], t, dtype=np.int32)
    hg, hc = ref.oracle_tracks(orc, TS, ids, G[k + "xglob"], G[k + "xcurv"], G[k + "u"], G[k + "params"])
    assert np.array_equal(hg, og) and np.array_equal(hc, oc)


@pytest.mark.parametrize("t", range(4))
def test_oracle_single_sub_steps(orc, G, TS, t):
    """Single Euler steps inside every segment of layout t, the curvature looked up by the oracle on the layout's table: the bound of
    tests/test_plant_params_cpu.py for a single sub-step."""
    k = "t%d/sub/" % t
    d = abi.plant_desc(int(TS.n_seg[t]), float(TS.lap_length[t]), timestep=0.001)
    assert d.n_sub == 1
    og, oc = pref.oracle_cars(orc, d, TS.table(t), G[k + "xglob"], G[k + "xcurv"], G[k + "u"], G[k + "params"])
    np.testing.assert_allclose(oc, G[k + "xcurv_next"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(og, G[k + "xglob_next"], rtol=0, atol=1e-15)


# ---- 2. abi.track_set, synth.fleet_tracks ----------------------------------------------------------------------------------------------
def test_track_set_packs_and_pads(TS):
    trs = ref.layouts()
    assert TS.n_tracks == 4 and TS.seg_stride == 11 and TS.tracks.shape == (4, 11, 6) and TS.tracks.dtype == np.float64
    assert TS.n_seg.dtype == np.int32 and list(TS.n_seg) == [7, 11, 11, 9] and TS.lap_length.dtype == np.float64
    for t, tr in enumerate(trs):
        assert np.array_equal(TS.tracks[t, :TS.n_seg[t]], tr.point_and_tangent) and (TS.tracks[t, TS.n_seg[t]:] == 0.0).all()
        assert TS.lap_length[t] == tr.lap_length
    wide = ref.track_set(seg_stride=64)
    assert wide.tracks.shape == (4, 64, 6) and np.array_equal(wide.tracks[:, :11], TS.tracks) and (wide.tracks[:, 11:] == 0.0).all()
    one = abi.track_set([trs[1].point_and_tangent], [trs[1].lap_length])
    assert one.n_tracks == 1 and one.seg_stride == 11


def test_track_set_refuses():
    tab = np.ones((5, 6))
    with pytest.raises(ValueError, match="9 tracks"):
        abi.track_set([tab] * 9, [1.0] * 9)
    with pytest.raises(ValueError, match="0 tracks"):
        abi.track_set([], [])
    with pytest.raises(ValueError, match="seg_stride 65"):
        abi.track_set([np.ones((65, 6))], [1.0])
    with pytest.raises(ValueError, match="track 1 has 5 rows"):
        abi.track_set([tab[:3], tab], [1.0, 1.0], seg_stride=4)
    for bad in (0.0, -19.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="lap length of track 1"):
            abi.track_set([tab, tab], [1.0, bad])
    with pytest.raises(ValueError, match="track 0 is ragged"):
        abi.track_set([[[0.0] * 6, [0.0] * 5]], [1.0])
    with pytest.raises(ValueError, match="track 1 has shape"):
        abi.track_set([tab, np.ones((5, 7))], [1.0, 1.0])
    with pytest.raises(ValueError, match="lap lengths"):
        abi.track_set([tab, tab], [1.0])
    assert abi.track_set([tab] * 8, [1.0] * 8).n_tracks == abi.CRX_MAX_TRACKS == 8
    assert abi.track_set([np.ones((64, 6))], [1.0]).seg_stride == abi.CRX_PLANT_MAX_SEG == 64


def test_fleet_tracks():
    for batch, n in ((4, 4), (5, 4), (300, 4), (64, 8)):
        ids = synth.fleet_tracks(batch, n, 3)
        assert ids.dtype == np.int32 and ids.shape == (batch,) and set(ids.tolist()) == set(range(n))
        assert np.array_equal(ids, synth.fleet_tracks(batch, n, 3))
    assert not np.array_equal(synth.fleet_tracks(300, 4, 3), synth.fleet_tracks(300, 4, 4))
    with pytest.raises(ValueError):
        synth.fleet_tracks(3, 4, 0)


# ---- 3. the loops ------------------------------------------------------------------------------------------------------------------------
def _ids():
    return np.array([2, 0, 3], dtype=np.int32)[:BN]


def _build(kind, AB, no_table=False, **kw):
    z = np.zeros((BN, 6))
    tab, lap = (None, None) if no_table else (TAB, LAP)
    if kind == "mpccbf":
        return montecarlo.MpccbfRaces(tab, lap, WIDTH, AB[0], AB[1], z, z, *_cars(2), device="cpu", **kw)
    if kind == "pid":
        return montecarlo.PidLaps(tab, lap, z, z, 4, device="cpu", **kw)
    assert kind == "lqr"
    return montecarlo.LqrLaps(tab, lap, z, z, AB[0], AB[1], device="cpu", **kw)


TODAY = {"mpccbf": ["cbf_prep_dev", "cbf_solve_dev", "plant_step_wrap_dev"], "pid": ["plant_step_wrap_dev", "pid_log_dev"],
         "lqr": ["lqr_step_dev", "plant_step_wrap_dev"]}
BUILT = {"mpccbf": [], "pid": ["pid_log_dev"], "lqr": ["lqr_design_dev"]}


@pytest.mark.parametrize("kind", ["mpccbf", "pid", "lqr"])
@pytest.mark.parametrize("as_tensor", [False, True])
def test_loops_hand_the_track_set_to_the_plant(rec, AB, TS, kind, as_tensor):
    plain = _build(kind, AB)
    assert rec.take()[0] == BUILT[kind] and plain.tracks is None and plain.lap_length == LAP
    plain.step()
    names_plain, args_plain = rec.take()
    assert names_plain == TODAY[kind]                                                           # without tracks=: today's sequence
    assert args_plain["plant_step_wrap_dev"]["track"] is plain.tab
    ids = _ids()
    P = synth.fleet_plant_params(BN, 0.3, 1)
    loop = _build(kind, AB, no_table=True, **dict(tracks=TS, track_id=torch.as_tensor(ids) if as_tensor else ids, plant_params=P))
    assert rec.take()[0] == BUILT[kind]
    ts = loop.tracks
    assert ts.n_tracks == 4 and ts.seg_stride == 11 and np.array_equal(ts.tracks.numpy(), TS.tracks) and np.array_equal(ts.n_seg.numpy(), TS.n_seg)
    assert ts.track_id.dtype == torch.int32 and np.array_equal(ts.track_id.numpy(), ids)
    assert torch.is_tensor(loop.lap_length) and np.array_equal(loop.lap_length.numpy(), TS.lap_length[ids])
    for _ in range(2):
        before = _plant_pairs(loop)
        loop.step()
        names, args = rec.take()
        plant = args["plant_step_tracks_wrap_dev"]
        assert names == [{"plant_step_wrap_dev": "plant_step_tracks_wrap_dev", "cbf_prep_dev": "cbf_prep_laps_dev"}.get(n, n) for n in TODAY[kind]]
        assert plant["tracks"] is ts and plant["params"] is loop.plant_params and plant["laps"] is loop.laps and plant["desc"] is loop.plant
        assert plant["xglob"] is before[0] and plant["xcurv"] is before[1] and plant["xglob_next"] is before[2] and plant["xcurv_next"] is before[3]
        assert loop.xg is before[2] and loop.xc is before[3] and loop.xg_next is before[0] and loop.xc_next is before[1]
        if kind == "mpccbf":
            assert args["cbf_prep_laps_dev"]["lap_length"] is loop.lap_length and args["cbf_prep_laps_dev"]["xcurv"] is before[1]
            assert plant["u"] is loop.ws.U and plant["u_stride"] == 2 * loop.N and args["cbf_solve_dev"]["x0"] is loop.xc_next
    if kind == "mpccbf":
        loop.step_glue()
        names, args = rec.take()
        assert names == ["cbf_solve_dev", "plant_step_tracks_dev"] and args["plant_step_tracks_dev"]["tracks"] is ts
        assert args["plant_step_tracks_dev"]["params"] is loop.plant_params
        assert tuple(args["cbf_solve_dev"]["lap_off"].shape) == (BN, 2)
        plain.step_glue()
        assert rec.take()[0] == ["cbf_solve_dev", "plant_step_dev"]


def test_run_functions_take_a_track_set(rec, AB, TS):
    z, ids = np.zeros((BN, 6)), _ids()
    montecarlo.mpccbf_races(None, None, WIDTH, AB[0], AB[1], z, z, *_cars(2), 2, device="cpu", tracks=TS, track_id=ids)
    montecarlo.lqr_laps(None, None, z, z, 2, AB[0], AB[1], device="cpu", tracks=TS, track_id=ids)
    montecarlo.pid_laps(None, None, z, z, 2, device="cpu", tracks=TS, track_id=ids)
    seen = [a["tracks"] for n, a in rec.calls if n == "plant_step_tracks_wrap_dev"]
    names = [n for n, _ in rec.calls]
    assert len(seen) == 6 and all(np.array_equal(s.track_id.numpy(), ids) for s in seen)
    assert "plant_step_wrap_dev" not in names and "cbf_prep_dev" not in names and names.count("cbf_prep_laps_dev") == 2


def test_track_set_arguments_are_checked(rec, AB, TS):
    ids = _ids()
    with pytest.raises(ValueError, match="go together"):
        _build("pid", AB, no_table=True, track_id=ids)
    with pytest.raises(ValueError, match="go together"):
        montecarlo.PidLaps(None, None, np.zeros((BN, 6)), np.zeros((BN, 6)), 4, device="cpu", tracks=TS)
    with pytest.raises(ValueError, match="pass None"):
        montecarlo.PidLaps(TAB, LAP, np.zeros((BN, 6)), np.zeros((BN, 6)), 4, device="cpu", tracks=TS, track_id=ids)
    with pytest.raises(ValueError, match="track_id"):
        _build("lqr", AB, no_table=True, **dict(tracks=TS, track_id=np.arange(BN + 1, dtype=np.int32) % 4))
    for bad in (-1, 4):
        with pytest.raises(ValueError, match=r"outside \[0, 4\)"):
            _build("lqr", AB, no_table=True, **dict(tracks=TS, track_id=np.array([0, bad, 1], dtype=np.int32)))
    with pytest.raises(ValueError, match="integer"):
        _build("lqr", AB, no_table=True, **dict(tracks=TS, track_id=np.zeros(BN)))


def test_other_loops_refuse_a_track_set(rec, AB, TS):
    """None of them may silently drive every car on track 0."""
    z, ids = np.zeros((BN, 6)), _ids()
    kw = dict(tracks=TS, track_id=ids, device="cpu")
    builders = {
        "IlqrRaces": lambda: montecarlo.IlqrRaces(TAB, LAP, AB[0], AB[1], z, z, np.full(BN, 3.0), np.full(BN, 0.2), np.zeros(BN), N=12, **kw),
        "LmpcLaps": lambda: montecarlo.LmpcLaps(TAB, LAP, WIDTH, *_lmpc_inputs(), N=N_LMPC, **kw),
        "GameLaps": lambda: montecarlo.GameLaps(TAB, LAP, WIDTH, AB[0], AB[1], np.zeros((7, 6)), *_lmpc_inputs(), *_cars(3), N=N_LMPC, **kw),
        "FieldGames": lambda: montecarlo.FieldGames(TAB, LAP, WIDTH, AB[0], AB[1], np.zeros((7, 6)), 1, *_lmpc_inputs(), N=N_LMPC, **kw),
        "SeedLaps": lambda: montecarlo.SeedLaps(TAB, LAP, WIDTH, AB[0], AB[1], z, z, **kw),
        "FieldRaces": lambda: montecarlo.FieldRaces(TAB, LAP, WIDTH, AB[0], AB[1], z, z, 1, **kw),
        "MixedRaces": lambda: montecarlo.MixedRaces(TAB, LAP, WIDTH, AB[0], AB[1], z, z, [["mpccbf"]] * BN, **kw),
    }
    for name, build in builders.items():
        with pytest.raises(ValueError, match="%s runs on one track" % name):
            build()
    assert rec.take()[0] == []                                                                 # ... before anything was launched
    loop = _build("lqr", AB, no_table=True, **dict(tracks=TS, track_id=ids))
    with pytest.raises(ValueError, match="RaceStats takes one lap length"):
        montecarlo.RaceStats(loop)


# ---- 4. the inputs of the GPU suite's wrap test -------------------------------------------------------------------------------------------
def test_noisy_case_has_no_car_on_its_line(orc, TS):
    """plant_tracks_ref.noisy_case at B = 300, track_id = b % 4: the oracle alone puts at most 3 cars within 1e-9 of THEIR OWN lap length
    (where the GPU's last-place differences could flip the wrap), and the wrap acts for at least 20 cars on each track."""
    B = 300
    ids = ref.interleaved(B)
    xc, xg, U, z, near = ref.noisy_case(TS, ids)
    P = synth.fleet_plant_params(B, 0.3, ref.NOISY_SEED)
    L = TS.lap_length[ids]
    _, oc = ref.oracle_tracks(orc, TS, ids, xg, xc, np.ascontiguousarray(U[:, 0, :]), P, z)
    assert (np.abs(oc[:, 4] - L) <= 1e-9).sum() <= 3
    _, crossed = ref.wrap(oc, L)
    per_track = [int(crossed[ids == t].sum()) for t in range(4)]
    print("cars crossing their own line, per track:", per_track)
    assert near.sum() == 100 and all(n >= 20 for n in per_track) and not crossed[~near].any()
    # on the wrong lap length the bookkeeping would differ: the tracks' lines are not each other's
    assert (ref.wrap(oc, np.full(B, TS.lap_length[0]))[1] != crossed).sum() >= 50
    clipped = np.abs(z * np.array([0.01, 0.01, 0.005])) > np.array([0.05, 0.1, 0.05])
    assert clipped[:, 0].any() and clipped[:, 1].any() and clipped[:, 2].any() and (~clipped).all(axis=1).sum() >= 100
