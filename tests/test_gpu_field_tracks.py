"""Field races and mixed fields on one track per race, on the GPU: crx_field_prep_tracks_dev, crx_mixed_prep_tracks_dev and
crx_race_stats_laps_dev against the numpy models called per track with the track's own table and lap length (tests/field_tracks_cases.py) and,
bit for bit, against the one-track entries on each track's races; FieldRaces / MixedRaces / RaceStats on a track set against four one-track
loops.  The four layouts of plant_tracks_ref.track_set(), race_track = r % 4 unless said otherwise."""
import numpy as np
import pytest

import field_tracks_cases as cases
import mixed_model as mm
import plant_tracks_ref as ref
import race_stats_model as rsm
import test_gpu_field as tf
import test_gpu_mixed as tm
import test_gpu_race_stats as trs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import crx

    return crx.init(0)


def _dev():
    import torch

    return torch.device("cuda", 0)


def _t(a, dtype=None):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64 if dtype is None else dtype, device=_dev())


def _set(ts, race_track, C, raw_ids=None):
    """A RaceTrackSetDev; raw_ids: ids written over race_track on the device afterwards (ids the host-side check would refuse)."""
    import torch

    from crx import torch_api

    s = torch_api.RaceTrackSetDev(ts, race_track, C, _dev())
    if raw_ids is not None:
        s.race_track.copy_(torch.as_tensor(np.ascontiguousarray(raw_ids), dtype=torch.int32))
    return s


def _run_field(desc, ts, race_track, x, dims=None, clear=True, raw_ids=None):
    """One crx_field_prep_tracks_dev launch; returns host arrays shaped as the model's (test_gpu_field._run)."""
    import torch

    from crx import torch_api

    R, C = x.shape[:2]
    V, N1 = C - 1, desc.N + 1
    ws = torch_api.FieldWorkspace(desc, R, _dev(), dims=dims is not None, clear=clear)
    torch_api.field_prep_tracks_dev(desc, _set(ts, race_track, C, raw_ids), _t(x.reshape(R * C, 6)), ws, car_dims=None if dims is None else _t(dims))
    torch.cuda.synchronize()
    out = dict(pred_s=ws.pred_s, pred_ey=ws.pred_ey, obs_s=ws.obs_s.reshape(R, C, V, N1), obs_ey=ws.obs_ey.reshape(R, C, V, N1),
               lap_off=ws.lap_off.reshape(R, C, V), n_obs=ws.n_obs.reshape(R, C))
    if dims is not None:
        out["obs_dims"] = ws.obs_dims.reshape(R, C, V, 2)
    if clear:
        out["clear"] = ws.clear.reshape(R, C)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _run_mixed(desc, ts, race_track, x, pol, dims=None, raw_ids=None):
    """One crx_mixed_prep_tracks_dev launch; host arrays shaped as the model's (test_gpu_mixed._run)."""
    import torch

    from crx import torch_api

    R, C = x.shape[:2]
    V, N1, NI1 = C - 1, desc.N + 1, desc.N_ilqr + 1
    ws = torch_api.MixedWorkspace(desc, R, _dev(), dims=dims is not None)
    torch_api.mixed_prep_tracks_dev(desc, _set(ts, race_track, C, raw_ids), _t(x.reshape(R * C, 6)), _t(pol.reshape(-1), torch.int32), ws,
                                    car_dims=None if dims is None else _t(dims))
    torch.cuda.synchronize()
    out = dict(pred_s=ws.pred_s, pred_ey=ws.pred_ey, obs_s=ws.obs_s.reshape(R, C, V, N1), obs_ey=ws.obs_ey.reshape(R, C, V, N1),
               lap_off=ws.lap_off.reshape(R, C, V), n_obs=ws.n_obs.reshape(R, C), m_nlp=ws.m_nlp.reshape(R, C), clear=ws.clear.reshape(R, C))
    if dims is not None:
        out["obs_dims"] = ws.obs_dims.reshape(R, C, V, 2)
    if desc.N_ilqr > 0:
        out.update(il_obs_s=ws.il_obs_s.reshape(R, C, V, NI1), il_obs_ey=ws.il_obs_ey.reshape(R, C, V, NI1),
                   il_lap_off=ws.il_lap_off.reshape(R, C, V), il_n_obs=ws.il_n_obs.reshape(R, C), m_ilqr=ws.m_ilqr.reshape(R, C))
    return {k: v.cpu().numpy() for k, v in out.items()}


def _fdesc(ts, N, C):
    """The descriptor of a set launch: track 0's geometry, which the entry does not use."""
    from crx import abi

    return abi.field_desc(N, C, int(ts.n_seg[0]), float(ts.lap_length[0]))


def _mdesc(ts, N_ilqr, C, mode, t=0):
    from crx import abi

    return abi.mixed_desc(cases.N_MIXED, N_ilqr, C, int(ts.n_seg[t]), float(ts.lap_length[t]), ilqr_obstacles=mode)


# ---- a. model parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", sorted(cases.SHAPES))
def test_field_prep_tracks_matches_the_model_per_track(gpu, C):
    for N in cases.HORIZONS:
        ts, rt, x, dims = cases.field_case(C, N)
        R = len(rt)
        assert R > 256 // C and len(set(rt[(R // (256 // C)) * (256 // C):])) >= 2          # a full block and a partial one that mixes tracks
        m_plain, m_dims = cases.field_model(ts, rt, x, N), cases.field_model(ts, rt, x, N, dims)
        # a kernel that used track 0's lap could not pass: egos beyond l_shape's lap, kept rows that wrap at their own L
        L_r = ts.lap_length[rt]
        with np.errstate(invalid="ignore"):
            assert (x[(rt == 1) | (rt == 3)][..., 4] > ts.lap_length[0]).any()
        if C > 1:
            assert (np.diff(m_dims["obs_s"], axis=-1) < -0.5 * L_r[:, None, None, None])[rt != 0].any()
        else:
            assert (np.diff(m_dims["pred_s"], axis=-1) < -0.5 * L_r[:, None, None])[rt != 0].any()
        desc = _fdesc(ts, N, C)
        for use_dims in (False, True):
            for clear in (False, True):
                tag = (C, N, use_dims, clear)
                m = m_dims if use_dims else m_plain
                g = _run_field(desc, ts, rt, x, dims if use_dims else None, clear)
                assert g["n_obs"].dtype == np.int32 and np.array_equal(g["n_obs"], m["n_obs"]), tag
                for k in ("pred_s", "pred_ey", "obs_s", "obs_ey", "lap_off"):
                    np.testing.assert_allclose(g[k], m[k], rtol=0, atol=1e-12, equal_nan=True, err_msg=str(tag + (k,)))
                if use_dims:
                    assert np.array_equal(g["obs_dims"], m["obs_dims"]), tag
                if clear:
                    np.testing.assert_allclose(g["clear"], m["clear"], rtol=1e-12, atol=0, err_msg=str(tag))
                # the NaN car of each layout (race 3 of its draw) poisons only its own predictions
                nan_row = np.isnan(g["pred_s"]).any(axis=-1)
                assert nan_row.sum() == 4 and not np.isnan(g["obs_s"]).any() and not np.isnan(g["obs_ey"]).any(), tag


# ---- b. bit identity with the one-track entries ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", sorted(cases.SHAPES))
def test_field_rows_of_a_track_are_the_one_track_launchs_bits(gpu, C):
    from crx import abi

    N = 10
    ts, rt, x, dims = cases.field_case(C, N)
    full = _run_field(_fdesc(ts, N, C), ts, rt, x, dims)
    plain = _run_field(_fdesc(ts, N, C), ts, rt, x, None)
    for t in range(ts.n_tracks):
        on = rt == t
        d1 = abi.field_desc(N, C, int(ts.n_seg[t]), float(ts.lap_length[t]))
        for got, dm in ((full, dims[on]), (plain, None)):
            one = tf._run(d1, ts.table(t), x[on], dm)
            assert sorted(one) == sorted(got)
            for k in one:
                assert tf._same_bits(got[k][on], one[k]), (t, k)
        # a set of one track, whatever the descriptor's geometry says, is the shared launch
        ts1 = abi.track_set([ts.table(t)], [ts.lap_length[t]])
        alone = _run_field(_fdesc(ts, N, C), ts1, np.zeros(int(on.sum()), dtype=np.int32), x[on], dims[on])
        for k in alone:
            assert tf._same_bits(alone[k], full[k][on]), (t, k)


@pytest.mark.parametrize("n_ilqr", [6, 20])
def test_mixed_rows_of_a_track_are_the_one_track_launchs_bits(gpu, n_ilqr):
    from crx import abi

    C = 3
    ts, rt, x, dims, pol = cases.mixed_case(C, n_ilqr)
    assert n_ilqr < cases.N_MIXED or n_ilqr > cases.N_MIXED
    for mode in (0, 1):
        full = _run_mixed(_mdesc(ts, n_ilqr, C, mode), ts, rt, x, pol, dims)
        for t in range(ts.n_tracks):
            on = rt == t
            one = tm._run(_mdesc(ts, n_ilqr, C, mode, t), ts.table(t), x[on], pol[on], dims[on])
            assert sorted(one) == sorted(full)
            for k in one:
                assert tf._same_bits(full[k][on], one[k]), (mode, t, k)
            if mode == 1:
                ts1 = abi.track_set([ts.table(t)], [ts.lap_length[t]])
                alone = _run_mixed(_mdesc(ts, n_ilqr, C, mode), ts1, np.zeros(int(on.sum()), dtype=np.int32), x[on], pol[on], dims[on])
                for k in alone:
                    assert tf._same_bits(alone[k], one[k]), (t, k)
        il = pol == mm.ILQR
        assert (full["il_lap_off"][il & (rt != 0)[:, None]] != 0).any()         # an iLQR lap offset computed with a lap that is not track 0's


# ---- c. position independence ------------------------------------------------------------------------------------------------------------------
def test_a_race_keeps_its_bits_wherever_it_stands(gpu):
    C, N = 3, 10
    ts, rt, x, dims = cases.field_case(C, N)
    desc = _fdesc(ts, N, C)
    full = _run_field(desc, ts, rt, x, dims)
    perm = np.random.default_rng(5).permutation(len(rt))
    shuffled = _run_field(desc, ts, rt[perm], x[perm], dims[perm])
    for k in full:
        assert tf._same_bits(shuffled[k], full[k][perm]), k
    by_track = np.argsort(rt, kind="stable")
    srt = _run_field(desc, ts, rt[by_track], x[by_track], dims[by_track])
    for k in full:
        assert tf._same_bits(srt[k], full[k][by_track]), k
    n_ilqr = 20
    ts, rt, x, dims, pol = cases.mixed_case(C, n_ilqr)
    mdesc = _mdesc(ts, n_ilqr, C, 1)
    mfull = _run_mixed(mdesc, ts, rt, x, pol, dims)
    mshuf = _run_mixed(mdesc, ts, rt[perm], x[perm], pol[perm], dims[perm])
    for k in mfull:
        assert tf._same_bits(mshuf[k], mfull[k][perm]), k


# ---- d. padding is never read; an id out of range never becomes an address ----------------------------------------------------------------------
def _poisoned(ts, seg_stride=None):
    """The set with every row past n_seg[t] filled with NaN and 1e300 (seg_stride: a wider packing, so that every track has padding)."""
    from crx import abi

    p = abi.track_set([ts.table(t) for t in range(ts.n_tracks)], ts.lap_length, seg_stride=seg_stride)
    for t in range(p.n_tracks):
        p.tracks[t, p.n_seg[t]:, 0::2] = np.nan
        p.tracks[t, p.n_seg[t]:, 1::2] = 1e300
    assert np.isnan(p.tracks).any() and all(np.isfinite(p.table(t)).all() for t in range(p.n_tracks))
    return p


def test_padding_rows_are_never_read(gpu):
    C, N, n_ilqr = 3, 10, 20
    ts, rt, x, dims = cases.field_case(C, N)
    clean = _run_field(_fdesc(ts, N, C), ts, rt, x, dims)
    for stride in (None, ts.seg_stride + 5):
        got = _run_field(_fdesc(ts, N, C), _poisoned(ts, stride), rt, x, dims)
        for k in clean:
            assert tf._same_bits(got[k], clean[k]), (stride, k)
    ts, rt, x, dims, pol = cases.mixed_case(C, n_ilqr)
    mclean = _run_mixed(_mdesc(ts, n_ilqr, C, 1), ts, rt, x, pol, dims)
    mgot = _run_mixed(_mdesc(ts, n_ilqr, C, 1), _poisoned(ts, ts.seg_stride + 5), rt, x, pol, dims)
    for k in mclean:
        assert tf._same_bits(mgot[k], mclean[k]), k


def test_a_race_without_a_track_is_harmless(gpu):
    """Device entry only: race 9 has id -1, race 80 id n_tracks.  The kernels compare the id before any use of it (race_track_of, crx_prep.hip),
    so those races read no table: NaN predictions, nobody kept, clear NaN, no solver mask -- and every other race keeps its bits."""
    C, N, n_ilqr = 3, 10, 20
    ts, rt, x, dims = cases.field_case(C, N)
    bad = np.zeros(len(rt), dtype=bool)
    bad[[9, 80]] = True
    raw = rt.copy()
    raw[9], raw[80] = -1, ts.n_tracks
    clean = _run_field(_fdesc(ts, N, C), ts, rt, x, dims)
    got = _run_field(_fdesc(ts, N, C), ts, rt, x, dims, raw_ids=raw)
    for k in clean:
        assert tf._same_bits(got[k][~bad], clean[k][~bad]), k
    assert np.isnan(got["pred_s"][bad]).all() and np.isnan(got["pred_ey"][bad]).all() and np.isnan(got["clear"][bad]).all()
    for k in ("obs_s", "obs_ey", "lap_off", "n_obs", "obs_dims"):
        assert not got[k][bad].any(), k
    ts, rt, x, dims, pol = cases.mixed_case(C, n_ilqr)
    pol = pol.copy()                                                     # solver policies in the two races: their masks must still come out 0
    pol[9], pol[80] = (mm.MPCCBF, mm.ILQR, mm.MPC_LTI), (mm.ILQR, mm.MPCCBF, mm.PID)
    for mode in (0, 1):
        mclean = _run_mixed(_mdesc(ts, n_ilqr, C, mode), ts, rt, x, pol, dims)
        mgot = _run_mixed(_mdesc(ts, n_ilqr, C, mode), ts, rt, x, pol, dims, raw_ids=raw)
        for k in mclean:
            assert tf._same_bits(mgot[k][~bad], mclean[k][~bad]), (mode, k)
        assert np.isnan(mgot["pred_s"][bad]).all() and np.isnan(mgot["pred_ey"][bad]).all() and np.isnan(mgot["clear"][bad]).all()
        for k in ("obs_s", "obs_ey", "lap_off", "n_obs", "obs_dims", "m_nlp", "m_ilqr", "il_n_obs", "il_obs_s", "il_obs_ey", "il_lap_off"):
            assert not mgot[k][bad].any(), (mode, k)


# ---- e. mixed model parity ---------------------------------------------------------------------------------------------------------------------
def test_mixed_prep_tracks_matches_the_model_per_track(gpu):
    C, n_ilqr = 3, 20
    ts, rt, x, dims, pol = cases.mixed_case(C, n_ilqr)
    assert len(rt) == 87
    for mode in (0, 1):
        for use_dims in (False, True):
            d = dims if use_dims else None
            m = cases.mixed_model(ts, rt, x, pol, n_ilqr, mode, d)
            g = _run_mixed(_mdesc(ts, n_ilqr, C, mode), ts, rt, x, pol, d)
            assert sorted(g) == sorted(k for k in m if k not in ("edge", "cond", "gap"))
            tm._check_prep(g, m, ("tracks", mode, use_dims), use_dims, n_ilqr)


# ---- f. race statistics ------------------------------------------------------------------------------------------------------------------------
def _assert_rows(ws, states, members):
    """Every field of the device state, at the cars members[t], is the model state states[t] run on those cars alone: as bits."""
    got = {name: v.cpu().numpy() for name, v in ws.fields().items()}
    for t, idx in enumerate(members):
        for name in trs.INT_FIELDS + trs.F64_FIELDS:
            a, b = got[name][..., idx], states[t][name]
            assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=name in trs.F64_FIELDS), (t, name)
    return got


def _summaries_add_up(total, parts):
    for k, v in total.items():
        vals = [p[k] for p in parts]
        if k in ("lap1_min", "lap2_min"):
            live = [q for q in vals if q >= 0]
            want = min(live) if live else -1
        elif k == "min_clear":
            want = min(vals)
        elif k in ("lap1_max", "lap2_max", "ey_max"):
            want = max(vals)
        elif k == "laps_hist":
            want = [sum(h) for h in zip(*vals)]
        else:
            want = sum(vals)
        assert (list(v) if k == "laps_hist" else v) == want, (k, v, vals)


def _stats_field_case(ts, rt, C, T, seed):
    """test_gpu_race_stats._field_case with every race walking along ITS track: cars bunched within 3 m, some of them starting just short of
    their own line, so that they cross it and pass each other near it."""
    rng = np.random.default_rng(seed)
    R = len(rt)
    L = ts.lap_length[rt][:, None]
    start = np.where(np.arange(R)[:, None] % 2 == 0, L - rng.uniform(0.5, 2.5, (R, 1)), rng.uniform(0.0, 1.0, (R, 1)) * L)
    s = (start + rng.uniform(0.0, 3.0, (R, C)))[None] + np.cumsum(rng.uniform(0.0, 0.8, (T, R, C)), axis=0)
    x = rng.uniform(-1.0, 1.0, (T, R, C, 6))
    x[..., 4], x[..., 5] = np.fmod(s, L[None]), rng.uniform(-0.4, 0.4, (T, R, C))
    x[3:7, R - 1, C - 1] = np.nan
    dims = np.stack([rng.uniform(0.3, 0.6, (R, C)), rng.uniform(0.15, 0.3, (R, C))], axis=-1)
    dims[0, 0, 1] = -0.2
    return x.reshape(T, R * C, 6), np.floor(s / L[None]).astype(np.int32).reshape(T, R * C), dims


def test_race_stats_laps_field_mode(gpu):
    import torch

    from crx import abi, torch_api

    R, C, T = 40, 3, 12
    ts, rt = ref.track_set(), cases.ids(R)
    x, laps, dims = _stats_field_case(ts, rt, C, T, 40)
    car_track = np.repeat(rt, C)
    members = [np.nonzero(car_track == t)[0] for t in range(ts.n_tracks)]
    states = []
    for t, idx in enumerate(members):
        st = rsm.reset(len(idx), C - 1, laps[0][idx])
        for k in range(T):
            rsm.sample(st, k, x[k][idx], laps[k][idx], ts.lap_length[t], 1.0, n_cars=C, car_dims=dims[rt == t])
        states.append(st)
    assert sum(int(st["passes"].sum()) for st in states) > 0 and sum(int((st["n_laps"] > 0).sum()) for st in states) > 10
    assert all((st["n_laps"] > 0).any() for st in states)                                        # cars cross the line of every track
    desc = abi.stats_desc(C - 1, C, float(ts.lap_length[0]), 1.0)
    ws = torch_api.RaceStatsWorkspace(desc, R * C, _dev())
    xd, ld, dd, lap = _t(x), _t(laps, torch.int32), _t(dims), _t(ts.lap_length[car_track])
    torch_api.race_stats_reset_dev(desc, ld[0], ws)
    for k in range(T):
        torch_api.race_stats_laps_dev(desc, k, 0.0, xd[k], ld[k], ws, car_dims=dd, lap_length=lap)
    torch.cuda.synchronize()
    _assert_rows(ws, states, members)
    total = abi.stats_summary_record(*(a[0].cpu().numpy() for a in torch_api.race_stats_summary_dev(desc, ws)))
    # ... and against crx_race_stats_dev on each track's races alone
    parts = []
    for t, idx in enumerate(members):
        d1 = abi.stats_desc(C - 1, C, float(ts.lap_length[t]), 1.0)
        w1 = torch_api.RaceStatsWorkspace(d1, len(idx), _dev())
        ix = torch.as_tensor(idx, device=_dev())
        torch_api.race_stats_reset_dev(d1, ld[0][ix].contiguous(), w1)
        for k in range(T):
            torch_api.race_stats_dev(d1, k, 0.0, xd[k][ix].contiguous(), ld[k][ix].contiguous(), w1, car_dims=_t(dims[rt == t]))
        torch.cuda.synchronize()
        for name, v in w1.fields().items():
            assert np.array_equal(v.cpu().numpy(), getattr(ws, name)[..., ix].cpu().numpy(), equal_nan=True), (t, name)
        parts.append(abi.stats_summary_record(*(a[0].cpu().numpy() for a in torch_api.race_stats_summary_dev(d1, w1))))
    _summaries_add_up(total, parts)
    # a car whose lap length is not positive and finite is a non-finite row: the model with that car's state NaN says the same
    lap_bad = ts.lap_length[car_track].copy()
    lap_bad[[4, 50, 77]] = [0.0, np.nan, -3.0]
    wb = torch_api.RaceStatsWorkspace(desc, R * C, _dev())
    torch_api.race_stats_reset_dev(desc, ld[0], wb)
    for k in range(T):
        torch_api.race_stats_laps_dev(desc, k, 0.0, xd[k], ld[k], wb, car_dims=dd, lap_length=_t(lap_bad))
    torch.cuda.synchronize()
    nf = wb.nonfinite_step.cpu().numpy()
    assert (nf[[4, 50, 77]] == 0).all() and (wb.n_samples.cpu().numpy()[[4, 50, 77]] == 0).all()
    others = np.ones(R * C, dtype=bool)
    others[[3, 4, 5, 48, 49, 50, 75, 76, 77]] = False                                            # their races see them as before: by their states
    for name in ("n_samples", "nonfinite_step", "n_laps", "passes", "min_clear"):
        assert np.array_equal(getattr(wb, name).cpu().numpy()[others], getattr(ws, name).cpu().numpy()[others], equal_nan=True), name


def test_race_stats_laps_scripted_mode(gpu):
    import torch

    from crx import abi, torch_api

    Bn, V, T = 100, 2, 12
    ts = ref.track_set()
    car_track = ref.interleaved(Bn)
    Lc = ts.lap_length[car_track]
    rng = np.random.default_rng(100)
    # egos start just short of their own line; scripted cars a little ahead of them, slower: crossings and passes near the line
    s = (Lc - rng.uniform(0.2, 1.5, Bn))[None] + np.cumsum(rng.uniform(0.2, 0.6, (T, Bn)), axis=0)
    x = rng.uniform(-1.0, 1.0, (T, Bn, 6))
    x[..., 4], x[..., 5] = np.fmod(s, Lc[None]), rng.uniform(-0.4, 0.4, (T, Bn))
    x[5:7, 10] = np.nan
    laps = np.floor(s / Lc[None]).astype(np.int32)
    s0 = s[0][:, None] + rng.uniform(0.3, 2.0, (Bn, V))
    v, ey = rng.uniform(0.0, 1.5, (Bn, V)), rng.uniform(-0.4, 0.4, (Bn, V))
    xt = rng.uniform(0.0, 1.0, (Bn, 6))
    times = trs._times(T)
    members = [np.nonzero(car_track == t)[0] for t in range(ts.n_tracks)]
    states = []
    for t, idx in enumerate(members):
        st = rsm.reset(len(idx), V, laps[0][idx])
        for k in range(T):
            rsm.sample(st, k, x[k][idx], laps[k][idx], ts.lap_length[t], 1.0, t=times[k], car_s0=s0[idx], car_v=v[idx], car_ey=ey[idx], xt=xt[idx])
        states.append(st)
    assert all((st["n_laps"] > 0).any() and st["passes"].sum() > 0 for st in states)
    desc = abi.stats_desc(V, 0, float(ts.lap_length[0]), 1.0)
    ws = torch_api.RaceStatsWorkspace(desc, Bn, _dev())
    xd, ld, lap = _t(x), _t(laps, torch.int32), _t(Lc)
    kw = dict(car_s0=_t(s0), car_v=_t(v), car_ey=_t(ey), xt=_t(xt))
    torch_api.race_stats_reset_dev(desc, ld[0], ws)
    for k in range(T):
        torch_api.race_stats_laps_dev(desc, k, times[k], xd[k], ld[k], ws, lap_length=lap, **kw)
    torch.cuda.synchronize()
    _assert_rows(ws, states, members)
    total = abi.stats_summary_record(*(a[0].cpu().numpy() for a in torch_api.race_stats_summary_dev(desc, ws)))
    parts = []
    for t, idx in enumerate(members):
        d1 = abi.stats_desc(V, 0, float(ts.lap_length[t]), 1.0)
        w1 = torch_api.RaceStatsWorkspace(d1, len(idx), _dev())
        ix = torch.as_tensor(idx, device=_dev())
        kw1 = {k: a[ix].contiguous() for k, a in kw.items()}
        torch_api.race_stats_reset_dev(d1, ld[0][ix].contiguous(), w1)
        for k in range(T):
            torch_api.race_stats_dev(d1, k, times[k], xd[k][ix].contiguous(), ld[k][ix].contiguous(), w1, **kw1)
        torch.cuda.synchronize()
        for name, val in w1.fields().items():
            assert np.array_equal(val.cpu().numpy(), getattr(ws, name)[..., ix].cpu().numpy(), equal_nan=True), (t, name)
        parts.append(abi.stats_summary_record(*(a[0].cpu().numpy() for a in torch_api.race_stats_summary_dev(d1, w1))))
        assert parts[-1] == rsm.summary(states[t])[0]
    _summaries_add_up(total, parts)


# ---- g. closed loops ---------------------------------------------------------------------------------------------------------------------------
def _starts(trs_, rt, C, seed):
    """Every race's cars 1.2 m apart on its own track, some races starting just short of their line; the global states that go with them."""
    rng = np.random.default_rng(seed)
    R = len(rt)
    x0 = np.zeros((R, C, 6))
    x0[..., 0] = 0.4
    L = np.array([trs_[t].lap_length for t in rt])
    x0[..., 4] = (np.where(np.arange(R) % 2 == 0, L - 1.5, rng.uniform(0.0, 1.0, R) * L)[:, None] + 1.2 * np.arange(C)[None, :]) % L[:, None]
    x0[..., 5] = rng.choice([-0.3, -0.1, 0.1, 0.3], (R, C))
    g0 = np.stack([tf._globals(trs_[t], x0[r]) for r, t in enumerate(rt)])
    vt = np.sort(rng.uniform(0.6, 1.1, (R, C)), axis=1)[:, ::-1].copy()
    return x0, g0, vt


def test_field_races_on_a_set_are_four_one_track_loops(gpu, AB):
    from crx import montecarlo

    R, C, N, steps = 8, 3, 10, 20
    trs_, ts, rt = ref.layouts(1.0), ref.track_set(), cases.ids(8)
    x0, g0, vt = _starts(trs_, rt, C, 8)
    kw = dict(N=N)
    r = montecarlo.field_races(None, None, 1.0, AB[0], AB[1], x0, g0, C, steps, vt=vt, tracks=ts, race_track=rt, **kw)
    assert np.isfinite(r["xcurv"]).all() and r["laps"].sum() > 0 and (r["n_obs"] > 0).any()
    for t in range(ts.n_tracks):
        on = rt == t
        cars = np.repeat(on, C)
        one = montecarlo.field_races(ts.table(t), float(ts.lap_length[t]), 1.0, AB[0], AB[1], x0[on], g0[on], C, steps, vt=vt[on], **kw)
        for k in ("xcurv", "u", "status", "n_obs"):
            assert tm._bits(r[k][:, cars], one[k]), (t, k)
        for k in ("laps", "min_clear"):
            assert tm._bits(r[k][cars], one[k]), (t, k)


def test_mixed_races_and_their_statistics_on_a_set_are_four_one_track_loops(gpu, AB):
    from crx import montecarlo

    R, C, N, steps = 8, 3, 10, 20
    trs_, ts, rt = ref.layouts(1.0), ref.track_set(), cases.ids(8)
    x0, g0, vt = _starts(trs_, rt, C, 9)
    pol = np.array([["mpccbf", "ilqr", "pid"], ["lqr", "mpc_lti", "mpccbf"]] * 4)[np.random.default_rng(2).permutation(R)]
    kw = dict(N=N, ilqr_N=20, ilqr_max_iter=20)

    def run(loop):
        st = montecarlo.RaceStats(loop)
        st.update()
        xs = [loop.xc.clone()]
        for _ in range(steps):
            st.step()
            xs.append(loop.xc.clone())
        return np.stack([a.cpu().numpy() for a in xs]), loop.u.cpu().numpy(), loop.status.cpu().numpy(), st.per_car(), st.summary()

    m = montecarlo.MixedRaces(None, None, 1.0, AB[0], AB[1], x0, g0, pol, vt=vt, tracks=ts, race_track=rt, **kw)
    xs, u, status, per, total = run(m)
    assert np.isfinite(xs).all() and m.laps.sum() > 0
    parts = []
    for t in range(ts.n_tracks):
        on = rt == t
        cars = np.repeat(on, C)
        q = montecarlo.MixedRaces(ts.table(t), float(ts.lap_length[t]), 1.0, AB[0], AB[1], x0[on], g0[on], pol[on], vt=vt[on], **kw)
        xs1, u1, status1, per1, rec1 = run(q)
        assert tm._bits(xs[:, cars], xs1) and tm._bits(u[cars], u1) and np.array_equal(status[cars], status1), t
        assert tm._bits(m.min_clear.cpu().numpy()[cars], q.min_clear.cpu().numpy()) and np.array_equal(m.laps.cpu().numpy()[cars], q.laps.cpu().numpy())
        assert sorted(per1) == sorted(per)
        for name in per1:
            assert np.array_equal(per[name][..., cars], per1[name], equal_nan=True), (t, name)
        parts.append(rec1)
    _summaries_add_up(total, parts)


# ---- h. host entries ---------------------------------------------------------------------------------------------------------------------------
def test_host_entries_give_the_device_bits_and_refuse_bad_sets(gpu):
    import crx
    from crx import abi

    C, N, n_ilqr = 3, 10, 20
    ts, rt, x, dims = cases.field_case(C, N)
    dev = _run_field(_fdesc(ts, N, C), ts, rt, x, dims)
    host = crx.field_prep_tracks(_fdesc(ts, N, C), ts, rt, x, dims)
    assert sorted(host) == sorted(dev)
    for k in dev:
        assert tf._same_bits(np.asarray(host[k]), dev[k]), k
    ts, rt, x, dims, pol = cases.mixed_case(C, n_ilqr)
    mdev = _run_mixed(_mdesc(ts, n_ilqr, C, 1), ts, rt, x, pol, dims)
    mhost = crx.mixed_prep_tracks(_mdesc(ts, n_ilqr, C, 1), ts, rt, x, pol, dims)
    assert sorted(mhost) == sorted(mdev)
    for k in mdev:
        assert tf._same_bits(np.asarray(mhost[k]), mdev[k]), k
    # refusals, the offender named
    bad_id = rt.copy()
    bad_id[17] = ts.n_tracks
    seg0 = abi.TrackSet(ts.tracks, ts.n_seg.copy(), ts.lap_length)
    seg0.n_seg[2] = 0
    lap0 = abi.TrackSet(ts.tracks, ts.n_seg, ts.lap_length.copy())
    lap0.lap_length[1] = np.nan
    for call in (lambda s, i: crx.field_prep_tracks(_fdesc(ts, N, C), s, i, x, dims), lambda s, i: crx.mixed_prep_tracks(_mdesc(ts, n_ilqr, C, 1), s, i, x, pol, dims)):
        for s, i, msg in ((ts, bad_id, "race_track of race 17: 4 outside"), (seg0, rt, "n_seg of track 2: 0 outside"),
                          (lap0, rt, "lap_length of track 1 must be positive and finite")):
            with pytest.raises(RuntimeError, match=msg):
                call(s, i)
