"""Race statistics on the GPU (include/crx.h "Race statistics"): the per-car state after hand-made state sequences, the batch summary,
and montecarlo.RaceStats in a loop, against the numpy model (tests/race_stats_model.py).  The kernel is compiled with contraction
off and the model rounds every operation on its own, so integers AND floating-point fields are compared bit for bit."""
import os

import numpy as np
import pytest

import conftest
import race_stats_model as rsm

pytestmark = pytest.mark.gpu

L, WIDTH, L_SUM, W_SUM = 20.0, 1.0, 0.5, 0.2      # a half-length sum that is exact in binary: ds == l_sum can be hit exactly
T_CRAFT, V_CRAFT = 24, 3
INT_FIELDS = rsm.INT_FIELDS + ("lap_step",)
F64_FIELDS = ("min_clear", "ey_max", "sum_ey2", "sum_dv2", "ds_prev")


@pytest.fixture(scope="module")
def gpu():
    import crx

    return crx.init(0)


def _times(T):
    """the scripted cars' clock at each sample, advanced by += 0.1 like the loops'"""
    t, out = 0.0, []
    for _ in range(T):
        out.append(t)
        t += 0.1
    return out


def crafted():
    """Five cars x 24 samples against three scripted cars each (ego rows [T,5,6], laps [T,5], car_s0 / car_v / car_ey [5,3], n_opp [5]):
      0  closes on a standing car 0.125 m per sample: ds = -l_sum exactly at sample 20 (h == 1: no contact), contact from sample 21 on
      1  |ey| == track_width at samples 8, 9 (on the track), one ulp beyond at sample 10 (off), back inside afterwards; cars 1 and 2 sit
         ON the ego, but n_opp = 1 keeps them out
      2  would pass a standing car at sample 10, but its row is NaN at samples 10 and 11: no pass is counted across the gap
      3  passes a standing car (sample 8), is passed by a faster one, and a third car half a lap away drifts across the fold: no pass
      4  ten line crossings (samples 2, 4, .., 20) while standing still; car 0 crosses the line towards it and then passes it"""
    T, n = T_CRAFT, 5
    k = np.arange(T, dtype=float)
    x = np.zeros((T, n, 6))
    x[:, :, 0] = 0.5 + 0.01 * k[:, None]                      # vx: only sum_dv2 reads it
    laps = np.zeros((T, n), dtype=np.int32)
    s0, v, ey = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    n_opp = np.full(n, 3, dtype=np.int32)
    # car 0
    x[:, 0, 4] = 5.0 + 0.125 * k
    s0[0], ey[0] = (8.0, 14.0, 16.0), (0.0, 0.6, -0.6)
    # car 1
    x[:, 1, 4], x[:, 1, 5] = 3.0, 0.5
    x[8:10, 1, 5], x[10, 1, 5], x[11:, 1, 5] = WIDTH, -np.nextafter(WIDTH, 2.0), 0.3
    s0[1], ey[1] = (12.0, 3.0, 3.0), (0.0, 0.5, 0.3)
    n_opp[1] = 1
    # car 2
    x[:, 2, 4] = 4.0 + 0.2 * k
    x[10:12, 2, :] = np.nan
    s0[2], ey[2] = (6.0, 15.0, 17.0), (0.8, 0.0, 0.0)
    # car 3
    x[:, 3, 4] = 4.0 + 0.25 * k
    s0[3], v[3], ey[3] = (6.0, 2.1, 15.9), (0.0, 5.0, 0.0), (0.8, -0.8, 0.0)
    # car 4
    x[:, 4, 4] = 1.0
    laps[:, 4] = np.minimum(np.arange(T) // 2, 10)
    s0[4], v[4], ey[4] = (19.0, 8.0, 13.0), (2.5, 0.0, 0.0), (0.7, 0.9, 0.9)
    return x, laps, s0, v, ey, n_opp


def _check_crafted(st, idx):
    """What the crafted cars were built to show, read from a state (model or device) at their indices."""
    c0, c1, c2, c3, c4 = idx
    assert st["contact_step"][c0] == 21 and st["contact_samples"][c0] == 3 and st["min_clear"][c0] < 1.0
    assert st["off_step"][c1] == 10 and st["off_samples"][c1] == 1 and st["ey_max"][c1] == np.nextafter(WIDTH, 2.0)
    assert st["contact_step"][c1] == -1 and np.isnan(st["ds_prev"][1:, c1]).all() and np.isfinite(st["ds_prev"][0, c1])
    assert st["nonfinite_step"][c2] == 10 and st["n_samples"][c2] == T_CRAFT - 2 and st["passes"][c2] == 0 and st["passed"][c2] == 0
    assert st["ds_prev"][0, c2] > 0                                    # it IS in front of the standing car at the end
    assert st["passes"][c3] == 1 and st["passed"][c3] == 1
    assert st["n_laps"][c4] == 10 and np.array_equal(st["lap_step"][:, c4], 2 * np.arange(1, 9)) and st["laps_prev"][c4] == 10
    assert st["passes"][c4] == 0 and st["passed"][c4] == 1
    for c in (c1, c2, c3, c4):
        assert st["contact_step"][c] == -1, c
    for c in (c0, c2, c3, c4):
        assert st["off_step"][c] == -1, c


def test_crafted_h_equal_one_is_not_contact():
    """The model on car 0 alone, stopped at sample 20: the running minimum is exactly 1 and no contact has been counted."""
    x, laps, s0, v, ey, n_opp = crafted()
    st = rsm.reset(5, 3, laps[0])
    for k, t in enumerate(_times(21)):
        rsm.sample(st, k, x[k], laps[k], L, WIDTH, t=t, car_s0=s0, car_v=v, car_ey=ey, n_opp=n_opp, l_sum=L_SUM, w_sum=W_SUM)
    assert st["min_clear"][0] == 1.0 and st["contact_step"][0] == -1


def _random_cars(rng, T, n, V):
    """n cars x T samples: s walks over several laps, |ey| up to 1.2, opponents anywhere, a few NaN rows and NaN opponents."""
    s_total = rng.uniform(0.0, L, n) + np.cumsum(rng.uniform(0.0, 5.0, (T, n)), axis=0)
    x = rng.uniform(-1.0, 1.0, (T, n, 6))
    x[:, :, 4], x[:, :, 5] = np.fmod(s_total, L), rng.uniform(-1.2, 1.2, (T, n))
    x[rng.uniform(size=(T, n)) < 0.02] = np.nan
    x[rng.uniform(size=(T, n)) < 0.01, 1] = np.inf
    laps = np.floor(s_total / L).astype(np.int32)
    s0, v, ey = rng.uniform(0.0, 3 * L, (n, V)), rng.uniform(0.0, 3.0, (n, V)), rng.uniform(-1.0, 1.0, (n, V))
    v[rng.uniform(size=(n, V)) < 0.03] = np.nan
    ey[rng.uniform(size=(n, V)) < 0.03] = np.inf
    return x, laps, s0, v, ey, rng.integers(-1, V + 2, n).astype(np.int32)


def _scripted_case(n, where):
    """(inputs, model state) of n cars: random ones with the crafted five at the indices `where`; computed once per n."""
    if n not in _CASES:
        rng = np.random.default_rng(1000 + n)
        x, laps, s0, v, ey, n_opp = _random_cars(rng, T_CRAFT, n, V_CRAFT)
        for i, (src, dst) in enumerate(zip(crafted(), (x, laps, s0, v, ey, n_opp))):
            if i < 2:                                                # x, laps: sample-major
                dst[:, where] = src
            else:
                dst[where] = src
        xt = rng.uniform(0.0, 1.0, (n, 6))
        flag = rng.integers(-1, 3, (T_CRAFT, n)).astype(np.int32)
        flag[rng.uniform(size=flag.shape) < 0.5] = 0
        st = rsm.reset(n, V_CRAFT, laps[0])
        for k, t in enumerate(_times(T_CRAFT)):
            rsm.sample(st, k, x[k], laps[k], L, WIDTH, t=t, car_s0=s0, car_v=v, car_ey=ey, n_opp=n_opp, xt=xt, flag=flag[k], l_sum=L_SUM,
                       w_sum=W_SUM)
        _check_crafted(st, where)
        _CASES[n] = (dict(x=x, laps=laps, s0=s0, v=v, ey=ey, n_opp=n_opp, xt=xt, flag=flag), st)
    return _CASES[n]


_CASES = {}


def _dev(a, dtype=None):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=torch.device("cuda", 0))


def _run_scripted(desc, c):
    """reset + one race_stats_dev per sample on the device; returns the workspace."""
    import torch

    from crx import torch_api

    n = c["x"].shape[1]
    ws = torch_api.RaceStatsWorkspace(desc, n, torch.device("cuda", 0))
    ws.stat_i.fill_(77); ws.stat_d.fill_(-3.0)                       # the reset writes every field
    s0, v, ey, n_opp, xt = _dev(c["s0"]), _dev(c["v"]), _dev(c["ey"]), _dev(c["n_opp"]), _dev(c["xt"])
    x, laps, flag = _dev(c["x"]), _dev(c["laps"]), _dev(c["flag"])
    torch_api.race_stats_reset_dev(desc, laps[0], ws)
    for k, t in enumerate(_times(x.shape[0])):
        torch_api.race_stats_dev(desc, k, t, x[k], laps[k], ws, car_s0=s0, car_v=v, car_ey=ey, n_opp=n_opp, xt=xt, flag=flag[k])
    torch.cuda.synchronize()
    return ws


def _assert_state(ws, st, tag=""):
    got = {name: v.cpu().numpy() for name, v in ws.fields().items()}
    assert sorted(got) == sorted(INT_FIELDS + F64_FIELDS)
    for name in INT_FIELDS:
        assert got[name].dtype == np.int32 and np.array_equal(got[name], st[name]), (tag, name, np.nonzero(got[name] != st[name]))
    for name in F64_FIELDS:
        same = (got[name] == st[name]) | (np.isnan(got[name]) & np.isnan(st[name]))
        assert got[name].dtype == np.float64 and same.all(), (tag, name, np.nonzero(~same), got[name][~same], st[name][~same])
    return got


@pytest.mark.parametrize("n,where", [(5, [0, 1, 2, 3, 4]), (257, [0, 255, 256, 128, 64])])
def test_scripted_mode_matches_model(gpu, n, where):
    from crx import abi

    c, st = _scripted_case(n, where)
    desc = abi.stats_desc(V_CRAFT, 0, L, WIDTH, l_sum=L_SUM, w_sum=W_SUM)
    got = _assert_state(_run_scripted(desc, c), st, n)
    _check_crafted(got, where)
    if n > 5:
        assert (st["nonfinite_step"] >= 0).sum() > 10 and (st["passes"] > 0).sum() > 10 and (st["contact_step"] >= 0).sum() > 3


def test_summary_matches_model(gpu):
    import torch

    from crx import abi, torch_api

    n = 257
    c, st = _scripted_case(n, [0, 255, 256, 128, 64])
    desc = abi.stats_desc(V_CRAFT, 0, L, WIDTH, l_sum=L_SUM, w_sum=W_SUM)
    ws = _run_scripted(desc, c)
    group = np.where(np.arange(n) % 7 < 4, 0, np.where(np.arange(n) % 7 < 6, 1, 2)).astype(np.int32)   # 148, 73 and 36 cars
    group[5] = 2
    for grp, G in ((None, 1), (group, 3)):
        sum_i, sum_d = torch_api.race_stats_summary_dev(desc, ws, None if grp is None else _dev(grp), G)
        torch.cuda.synchronize()
        assert sum_i.dtype == torch.int64 and tuple(sum_i.shape) == (G, abi.STATS_SUM_NI) and tuple(sum_d.shape) == (G, abi.STATS_SUM_ND)
        want = rsm.summary(st, grp, G)
        for g in range(G):
            got = abi.stats_summary_record(sum_i[g].cpu().numpy(), sum_d[g].cpu().numpy())
            assert got == want[g], (g, got, want[g])
        assert sum(w["cars"] for w in want) == n and all(w["lap2_count"] > 0 and w["nonfinite"] > 0 for w in want)
    # the host-pointer entry on the same state: the same record
    hi, hd = gpu.race_stats_summary(desc, ws.stat_i.cpu().numpy(), ws.stat_d.cpu().numpy(), group, 3)
    assert np.array_equal(hi, sum_i.cpu().numpy()) and np.array_equal(hd, sum_d.cpu().numpy())


def test_host_entries_give_the_device_bits(gpu):
    from crx import abi

    c, st = _scripted_case(5, [0, 1, 2, 3, 4])
    desc = abi.stats_desc(V_CRAFT, 0, L, WIDTH, l_sum=L_SUM, w_sum=W_SUM)
    si, sd = gpu.race_stats_reset(desc, c["laps"][0])
    for k, t in enumerate(_times(T_CRAFT)):
        gpu.race_stats(desc, k, t, c["x"][k], c["laps"][k], si, sd, car_s0=c["s0"], car_v=c["v"], car_ey=c["ey"], n_opp=c["n_opp"], xt=c["xt"],
                       flag=c["flag"][k])
    assert np.array_equal(si[abi.STATS_I["passes"]], st["passes"]) and np.array_equal(si[abi.STATS_I["lap_step"]:abi.STATS_I["lap_step"] + 8], st["lap_step"])
    assert np.array_equal(sd[abi.STATS_D["min_clear"]], st["min_clear"]) and np.array_equal(sd[abi.STATS_D["sum_dv2"]], st["sum_dv2"])


def _field_case(R, C, T, seed):
    """R races of C cars bunched within a few metres, drifting at different speeds: contacts, passes both ways; one car NaN for a while, one
    non-positive width."""
    rng = np.random.default_rng(seed)
    s = (rng.uniform(0.0, L, (R, 1)) + rng.uniform(0.0, 3.0, (R, C)))[None] + np.cumsum(rng.uniform(0.0, 0.8, (T, R, C)), axis=0)
    x = rng.uniform(-1.0, 1.0, (T, R, C, 6))
    x[..., 4], x[..., 5] = np.fmod(s, L), rng.uniform(-0.4, 0.4, (T, R, C))
    if C > 1:
        x[3:7, R - 1, C - 1] = np.nan
    dims = np.stack([rng.uniform(0.3, 0.6, (R, C)), rng.uniform(0.15, 0.3, (R, C))], axis=-1)
    dims[0, 0, 1] = -0.2
    return x.reshape(T, R * C, 6), np.floor(s / L).astype(np.int32).reshape(T, R * C), dims


@pytest.mark.parametrize("R,C", [(2, 3), (1, 1)])
@pytest.mark.parametrize("use_dims", [False, True])
def test_field_mode_matches_model(gpu, R, C, use_dims):
    import torch

    from crx import abi, torch_api

    T = 16
    x, laps, dims = _field_case(R, C, T, 10 * R + C)
    desc = abi.stats_desc(C - 1, C, L, WIDTH)
    st = rsm.reset(R * C, C - 1, laps[0])
    for k in range(T):
        rsm.sample(st, k, x[k], laps[k], L, WIDTH, n_cars=C, car_dims=dims if use_dims else None)
    ws = torch_api.RaceStatsWorkspace(desc, R * C, torch.device("cuda", 0))
    xd, ld, dd = _dev(x), _dev(laps), _dev(dims)
    torch_api.race_stats_reset_dev(desc, ld[0], ws)
    for k in range(T):
        torch_api.race_stats_dev(desc, k, 0.0, xd[k], ld[k], ws, car_dims=dd if use_dims else None)
    torch.cuda.synchronize()
    _assert_state(ws, st, (R, C, use_dims))
    if C == 1:
        assert np.isinf(st["min_clear"]).all() and (st["contact_step"] == -1).all()
    else:
        assert np.isfinite(st["min_clear"]).all()                        # the NaN car lowered nobody's clear (and left it finite)
        assert st["nonfinite_step"][R * C - 1] == 3 and (st["nonfinite_step"][:-1] == -1).all()
        assert (st["contact_step"] >= 0).any() and st["passes"].sum() > 0 and st["passes"].sum() == st["passed"].sum()
        if use_dims:   # the non-positive width took the descriptor's value: the model with that value written out gives the same state
            fixed = dims.copy()
            fixed[0, 0, 1] = 0.2
            st2 = rsm.reset(R * C, C - 1, laps[0])
            for k in range(T):
                rsm.sample(st2, k, x[k], laps[k], L, WIDTH, n_cars=C, car_dims=fixed)
            assert np.array_equal(st2["min_clear"], st["min_clear"])


def _track(width=1.0):
    from utils import racing_env

    return racing_env.ClosedTrack(np.genfromtxt(os.path.join(conftest.ROOT, "data/track_layout/l_shape.csv"), delimiter=","), track_width=width)


def test_replay_of_field_races(gpu, AB):
    """FieldRaces keeps min_clear from crx_field_prep's `clear` (contraction on); the states its 12 steps started from, replayed through
    race_stats_dev (contraction off), give the same minimum to 1e-14 relative."""
    import torch

    from crx import abi, montecarlo, torch_api
    from test_gpu_field import _globals

    track = _track(1.0)
    tab, Lt = track.point_and_tangent, track.lap_length
    R, C, N, steps = 2, 3, 10, 12
    vt = np.array([[1.0, 0.8, 0.6], [1.2, 0.5, 0.9]])
    x0 = np.zeros((R, C, 6))
    x0[..., 0], x0[..., 4], x0[..., 5] = 0.5 * vt, 1.0 + 0.7 * np.arange(C)[None, :], [0.15, -0.15, 0.15]
    g0 = _globals(track, x0.reshape(-1, 6))
    r = montecarlo.field_races(tab, Lt, track.width, AB[0], AB[1], x0, g0, C, steps, vt=vt, N=N)
    assert np.isfinite(r["min_clear"]).all()
    desc = abi.stats_desc(C - 1, C, Lt, track.width)
    ws = torch_api.RaceStatsWorkspace(desc, R * C, torch.device("cuda", 0))
    laps = torch.zeros(R * C, dtype=torch.int32, device=ws.stat_i.device)
    torch_api.race_stats_reset_dev(desc, laps, ws)
    xs = _dev(r["xcurv"])
    for k in range(steps):
        torch_api.race_stats_dev(desc, k, 0.0, xs[k], laps, ws)
    torch.cuda.synchronize()
    np.testing.assert_allclose(ws.min_clear.cpu().numpy(), r["min_clear"], rtol=1e-14, atol=0)


def test_race_stats_in_the_game_loop(gpu, AB, golden_racing_game):
    """GameLaps, 4 races x 30 steps on the golden safe set against synth.multi_tests_traffic, stepped through RaceStats: per_car() equals
    the model applied to the logged states, lap counters, branch masks and the scripted cars' clock."""
    import torch

    import helpers
    import scenarios
    from crx import montecarlo, synth

    A, B = AB
    g = golden_racing_game
    track = _track(1.0)
    opt = scenarios.table("optimal_traj", "xcurv_l_shape")
    d, ss, us, qf, time_ss, lin_points, lin_input = helpers.lmpc_lap_setup(g, track)
    Bn, steps, V = 4, 30, 3
    s0, v, ey = synth.multi_tests_traffic(Bn, V, seed=1)
    x0 = np.tile(g["lmpc/x"][0], (Bn, 1)); xg0 = np.tile(g["lap1/xglob"][-1], (Bn, 1))
    tile = lambda a: np.tile(a[None], (Bn,) + (1,) * a.ndim)   # noqa: E731
    game = montecarlo.GameLaps(track.point_and_tangent, track.lap_length, track.width, A, B, opt, tile(ss), tile(us), tile(qf), tile(time_ss),
                               np.full(Bn, 2, dtype=np.int32), x0, xg0, tile(lin_points), tile(lin_input), s0, v, ey)
    stats = montecarlo.RaceStats(game)
    log = []
    snap = lambda: log.append((game.lm.xc.clone(), game.lm.laps.clone(), game.m_ot.clone(), game.t))   # noqa: E731
    stats.update(); snap()
    for _ in range(steps):
        stats.step(); snap()
    torch.cuda.synchronize()
    assert stats.n_updates == steps + 1
    st = rsm.reset(Bn, V, np.zeros(Bn, dtype=np.int32))
    for k, (xc, laps, m_ot, t) in enumerate(log):
        rsm.sample(st, k, xc.cpu().numpy(), laps.cpu().numpy(), track.lap_length, track.width, t=t, car_s0=s0, car_v=v, car_ey=ey,
                   flag=m_ot.cpu().numpy())
    got = stats.per_car()
    assert sorted(got) == sorted(INT_FIELDS + F64_FIELDS)
    for name in INT_FIELDS + F64_FIELDS:
        assert np.array_equal(got[name], st[name], equal_nan=name in F64_FIELDS), (name, got[name], st[name])
    assert (got["n_samples"] == steps + 1).all() and np.isfinite(got["min_clear"]).all() and (got["sum_dv2"] == 0).all()
    rec = stats.summary()
    assert rec == rsm.summary(st)[0] and rec["cars"] == Bn and rec["n_samples"] == Bn * (steps + 1)
