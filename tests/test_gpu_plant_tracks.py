"""One track per car on the GPU (crx_plant_tracks_kernel / crx_plant_tracks_cars_kernel behind crx_plant_step_tracks_dev /
crx_plant_step_tracks_plain_dev / crx_plant_step_tracks, crx_cbfprep_laps_kernel behind crx_cbf_prep_laps_dev, and the tracks= / track_id=
arguments of PidLaps, LqrLaps and MpccbfRaces).  The reference for car b is the oracle at batch 1 on table track_id[b] with that track's
n_seg and lap_length in the descriptor (tests/plant_tracks_ref.py; tests/test_plant_tracks_cpu.py holds the oracle to the reference on all
four layouts).  The track set is the four layouts, track_id = b % 4 (every wavefront holds all four); batches 1, 67 (a full wave and a
partial one) and 300 (across the 256-thread block boundary)."""
import ctypes as C

import numpy as np
import pytest

import plant_params_ref as pref
import plant_tracks_ref as ref

pytestmark = pytest.mark.gpu

PLANT_TOL = 1e-12     # tests/test_gpu_parity.py test_plant_step
X_TOL = 1e-11         # tests/test_gpu_sysid.py: the PID closed loop against the host loop
W_TOL = 1e-8          # tests/test_gpu_sysid.py: the fit against the numpy mirror, relative
B_BIG = 300
CRX_ERR_ARG = -1      # include/crx.h
WIDTH = 1.0


@pytest.fixture(scope="module")
def gpu():
    import crx

    return crx.init(0)


@pytest.fixture(scope="module")
def S():
    """The track set of the four layouts, a valid plant descriptor and the tensor helpers."""
    import torch

    from crx import abi

    dev = torch.device("cuda", 0)

    class Ctx:
        ts = ref.track_set()

        @staticmethod
        def t(a, dt=torch.float64):
            return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)

        @staticmethod
        def desc(t):
            return abi.plant_desc(int(Ctx.ts.n_seg[t]), float(Ctx.ts.lap_length[t]))

    Ctx.dev = dev
    Ctx.d = Ctx.desc(0)
    return Ctx


def _set_dev(S, ts, ids):
    """TrackSetDev of host set ts with the ids as they are given: the wrapper's range check is stepped around for the bad-id cases."""
    from crx import torch_api

    ids = np.asarray(ids, dtype=np.int32)
    sd = torch_api.TrackSetDev(ts, np.clip(ids, 0, ts.n_tracks - 1), S.dev)
    sd.track_id = S.t(ids, sd.track_id.dtype)
    return sd


def _tracks_wrap(S, ts, ids, xg, xc, u, u_stride, z, P, laps0=None, d=None):
    """plant_step_tracks_wrap_dev on host arrays -> (xglob_next, xcurv_next, laps) as host arrays."""
    import torch

    from crx import torch_api

    n = xg.shape[0]
    og, oc = torch.empty((n, 6), dtype=torch.float64, device=S.dev), torch.empty((n, 6), dtype=torch.float64, device=S.dev)
    laps = S.t(np.zeros(n) if laps0 is None else laps0, torch.int32)
    torch_api.plant_step_tracks_wrap_dev(S.d if d is None else d, _set_dev(S, ts, ids), S.t(xg), S.t(xc), S.t(u), u_stride, og, oc, laps,
                                         noise_z=None if z is None else S.t(z), params=None if P is None else S.t(P))
    torch.cuda.synchronize()
    return og.cpu().numpy(), oc.cpu().numpy(), laps.cpu().numpy()


def _tracks_plain(S, ts, ids, xg, xc, u, P):
    import torch

    from crx import torch_api

    og, oc = torch_api.plant_step_tracks_dev(S.d, _set_dev(S, ts, ids), S.t(xg), S.t(xc), S.t(u), params=None if P is None else S.t(P))
    torch.cuda.synchronize()
    return og.cpu().numpy(), oc.cpu().numpy()


def _single_wrap(S, t, xg, xc, u, u_stride, z, P, laps0):
    """The shipped one-table launch (crx_plant_step_params_dev; crx_plant_step_noise_dev without params) on table t alone."""
    import torch

    from crx import torch_api

    n = xg.shape[0]
    og, oc = torch.empty((n, 6), dtype=torch.float64, device=S.dev), torch.empty((n, 6), dtype=torch.float64, device=S.dev)
    laps = S.t(laps0, torch.int32)
    torch_api.plant_step_wrap_dev(S.desc(t), S.t(S.ts.table(t)), S.t(xg), S.t(xc), S.t(u), u_stride, og, oc, laps, noise_z=None if z is None else S.t(z),
                                  params=None if P is None else S.t(P))
    torch.cuda.synchronize()
    return og.cpu().numpy(), oc.cpu().numpy(), laps.cpu().numpy()


@pytest.mark.parametrize("with_params", [False, True])
def test_a_parity_one_step(gpu, orc, S, with_params):
    """No wrap, no noise, B = 300 (two blocks), every car against the oracle on its own track (and its own parameter row)."""
    from crx import synth

    ids = ref.interleaved(B_BIG)
    rng = np.random.default_rng(11)
    xc, xg, u = ref.draw_states(rng, S.ts, ids)
    P = synth.fleet_plant_params(B_BIG, 0.3, 11) if with_params else None
    og, oc = ref.oracle_tracks(orc, S.ts, ids, xg, xc, u, P)
    gg, gc = _tracks_plain(S, S.ts, ids, xg, xc, u, P)
    print("test a (params %s): B = %d, worst |xcurv - oracle| %.3g, |xglob - oracle| %.3g (bound %g)" % (
        with_params, B_BIG, np.abs(gc - oc).max(), np.abs(gg - og).max(), PLANT_TOL))
    np.testing.assert_allclose(gc, oc, rtol=0, atol=PLANT_TOL)       # every car: none is left out
    np.testing.assert_allclose(gg, og, rtol=0, atol=PLANT_TOL)
    # the tracks matter: the same cars on track 0 alone end elsewhere
    zg, zc = _tracks_plain(S, S.ts, np.zeros(B_BIG, dtype=np.int32), xg, xc, u, P)
    moved = np.abs(zc - gc).max(axis=1)
    assert moved.max() > 1e-6 and (moved[ids != 0] > 1e-6).sum() >= 50 and np.array_equal(zc[ids == 0], gc[ids == 0])
    # the smaller batches say the same
    for n in (1, 67):
        sg, sc = _tracks_plain(S, S.ts, ids[:n], xg[:n], xc[:n], u[:n], None if P is None else P[:n])
        assert np.array_equal(sg, gg[:n]) and np.array_equal(sc, gc[:n])


def test_b_noise_wrap_strided_inputs(gpu, orc, S):
    import torch

    import crx
    from crx import synth, torch_api

    ids = ref.interleaved(B_BIG)
    L = S.ts.lap_length[ids]
    xc, xg, U, z, near = ref.noisy_case(S.ts, ids)
    P = synth.fleet_plant_params(B_BIG, 0.3, ref.NOISY_SEED)
    og, oc = ref.oracle_tracks(orc, S.ts, ids, xg, xc, np.ascontiguousarray(U[:, 0, :]), P, z)
    on_line = np.abs(oc[:, 4] - L) <= 1e-9          # a last-place difference could flip the wrap there
    assert on_line.sum() <= 3
    hc, crossed = ref.wrap(oc, L)
    laps0 = np.arange(B_BIG) % 5
    gg, gc, laps = _tracks_wrap(S, S.ts, ids, xg, xc, U, 24, z, P, laps0=laps0)
    keep = ~on_line
    print("test b: B = %d, %d cars crossed, %d left out, worst |xcurv - oracle| %.3g, |xglob - oracle| %.3g (bound %g)" % (
        B_BIG, crossed.sum(), on_line.sum(), np.abs(gc - hc)[keep].max(), np.abs(gg - og)[keep].max(), PLANT_TOL))
    np.testing.assert_allclose(gc[keep], hc[keep], rtol=0, atol=PLANT_TOL)
    np.testing.assert_allclose(gg[keep], og[keep], rtol=0, atol=PLANT_TOL)
    assert np.array_equal(laps[keep], (laps0 + crossed)[keep])
    assert all(crossed[ids == t].sum() >= 20 for t in range(4)) and (crossed == 0).sum() >= 200
    # laps is optional (the C entry itself)
    og2, oc2 = torch.empty((B_BIG, 6), dtype=torch.float64, device=S.dev), torch.empty((B_BIG, 6), dtype=torch.float64, device=S.dev)
    fn = crx.lib().crx_plant_step_tracks_dev
    fn.restype = C.c_int
    sd = _set_dev(S, S.ts, ids)
    tt = [S.t(xg), S.t(xc), S.t(U), S.t(z), S.t(P)]
    p = lambda a: C.c_void_p(a.data_ptr())   # noqa: E731
    rc = fn(C.byref(S.d), C.c_int(B_BIG), C.c_int(sd.n_tracks), C.c_int(sd.seg_stride), p(sd.tracks), p(sd.n_seg), p(sd.lap_length), p(sd.track_id),
            p(tt[0]), p(tt[1]), p(tt[2]), C.c_int(24), p(tt[3]), p(tt[4]), p(og2), p(oc2), C.c_void_p(0), torch_api._stream())
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(oc2.cpu().numpy(), gc) and np.array_equal(og2.cpu().numpy(), gg)


@pytest.mark.parametrize("with_params", [False, True])
def test_c_bit_identity_with_the_single_track_launches(gpu, S, with_params):
    """The rows of the mixed launch with track_id == t are the bits of the shipped one-table launch on table t alone over those cars, noise
    and wrap included; a set of ONE track is the shipped launch over all cars."""
    from crx import abi, synth

    ids = ref.interleaved(B_BIG)
    xc, xg, U, z, _ = ref.noisy_case(S.ts, ids)
    P = synth.fleet_plant_params(B_BIG, 0.3, 13) if with_params else None
    laps0 = np.arange(B_BIG) % 3
    mg, mc, ml = _tracks_wrap(S, S.ts, ids, xg, xc, U, 24, z, P, laps0=laps0)
    assert np.isfinite(mc).all() and (ml > laps0).sum() >= 80
    for t in range(4):
        i = ids == t
        sg, sc, sl = _single_wrap(S, t, xg[i], xc[i], U[i], 24, z[i], None if P is None else P[i], laps0[i])
        assert np.array_equal(mc[i], sc) and np.array_equal(mg[i], sg) and np.array_equal(ml[i], sl), t
        # n_tracks = 1: a set that holds table t only, every car on it
        one = abi.track_set([S.ts.table(t)], [S.ts.lap_length[t]])
        xs = xc.copy()
        xs[:, 4] = np.where(i, xs[:, 4], np.minimum(xs[:, 4], S.ts.lap_length[t] - 1.0))      # the others' lines are not this track's
        og, oc, ol = _tracks_wrap(S, one, np.zeros(B_BIG, dtype=np.int32), xg, xs, U, 24, z, P, laps0=laps0, d=S.desc(t))
        sg, sc, sl = _single_wrap(S, t, xg, xs, U, 24, z, P, laps0)
        assert np.array_equal(oc, sc) and np.array_equal(og, sg) and np.array_equal(ol, sl), t


def test_d_position_independence(gpu, S):
    """One car -- state, input, noise, parameter row, track -- alone, as car 66 of 67 and as car 299 of 300: the same bits, whatever tracks
    the others are on.  A neighbour with track_id -1 and one with track_id n_tracks go non-finite alone."""
    from crx import synth

    ids = ref.interleaved(B_BIG)
    xc, xg, U, z, _ = ref.noisy_case(S.ts, ids, seed=5)
    P = synth.fleet_plant_params(B_BIG, 0.3, 5)
    u = np.ascontiguousarray(U[:, 0, :])
    for j in (3, 6, 9, 0):                             # near their lines, one car per track (3 % 4 = 3, 6 % 4 = 2, 9 % 4 = 1, 0)
        one = (xg[j:j + 1], xc[j:j + 1], u[j:j + 1], z[j:j + 1], P[j:j + 1], ids[j:j + 1])
        ag, ac, al = _tracks_wrap(S, S.ts, one[5], one[0], one[1], one[2], 2, one[3], one[4])
        for n in (67, B_BIG):
            arrs = [a[:n].copy() for a in (xg, xc, u, z, P, ids)]
            for a, o in zip(arrs, one):
                a[n - 1] = o[0]
            g, c, l = _tracks_wrap(S, S.ts, arrs[5], arrs[0], arrs[1], arrs[2], 2, arrs[3], arrs[4])
            assert np.array_equal(g[n - 1], ag[0]) and np.array_equal(c[n - 1], ac[0]) and l[n - 1] == al[0], (j, n)
            # other tracks around it, two bad ids among them: car n - 1 does not move, only the bad cars go non-finite, their counters stay
            arrs[5][: n - 1] = (arrs[5][: n - 1] + 1 + np.arange(n - 1) % 3) % 4
            arrs[5][0], arrs[5][n // 2] = -1, S.ts.n_tracks
            laps0 = np.full(n, 7)
            g2, c2, l2 = _tracks_wrap(S, S.ts, arrs[5], arrs[0], arrs[1], arrs[2], 2, arrs[3], arrs[4], laps0=laps0)
            assert np.array_equal(g2[n - 1], ag[0]) and np.array_equal(c2[n - 1], ac[0]) and l2[n - 1] == al[0] + 7, (j, n)
            bad = np.zeros(n, dtype=bool)
            bad[[0, n // 2]] = True
            assert np.isnan(c2[bad]).all() and np.isnan(g2[bad]).all() and (l2[bad] == 7).all()
            assert np.isfinite(c2[~bad]).all() and np.isfinite(g2[~bad]).all()
            # every other car keeps the bits it has without the bad neighbours
            arrs[5][0], arrs[5][n // 2] = 0, 0
            g3, c3, l3 = _tracks_wrap(S, S.ts, arrs[5], arrs[0], arrs[1], arrs[2], 2, arrs[3], arrs[4], laps0=laps0)
            assert np.array_equal(c3[~bad], c2[~bad]) and np.array_equal(g3[~bad], g2[~bad]) and np.array_equal(l3[~bad], l2[~bad])


def test_e_padding_is_never_read(gpu, S):
    from crx import abi, synth

    ids = ref.interleaved(B_BIG)
    xc, xg, U, z, _ = ref.noisy_case(S.ts, ids, seed=6)
    P = synth.fleet_plant_params(B_BIG, 0.3, 6)
    base = _tracks_wrap(S, S.ts, ids, xg, xc, U, 24, z, P)
    assert np.isfinite(base[1]).all()
    wide = ref.track_set(seg_stride=64)
    pad = np.zeros(wide.tracks.shape[:2], dtype=bool)
    for t in range(4):
        pad[t, wide.n_seg[t]:] = True
    for ts in (S.ts, wide):
        p = pad[:, :ts.seg_stride]
        for fill in (np.full(6, np.nan), np.array([0.0, 0.0, 0.0, -1e9, 3e9, 0.7])):      # NaN rows; rows that would match every s
            tr = ts.tracks.copy()
            tr[p] = fill
            got = _tracks_wrap(S, abi.TrackSet(tr, ts.n_seg, ts.lap_length), ids, xg, xc, U, 24, z, P)
            for x, y in zip(got, base):
                assert np.array_equal(x, y)
    # ... and the rows that are not padding are read: the match-all row in place of track 1's first one moves its cars
    tr = S.ts.tracks.copy()
    tr[1, 0] = [0.0, 0.0, 0.0, -1e9, 3e9, 0.7]
    got = _tracks_wrap(S, abi.TrackSet(tr, S.ts.n_seg, S.ts.lap_length), ids, xg, xc, U, 24, z, P)
    assert not np.array_equal(got[1][ids == 1], base[1][ids == 1]) and np.array_equal(got[1][ids != 1], base[1][ids != 1])


def test_f_host_pointer_entry(gpu, S):
    import crx
    from crx import abi, synth

    n = 67
    ids = ref.interleaved(n)
    rng = np.random.default_rng(12)
    xc, xg, u = ref.draw_states(rng, S.ts, ids)
    P = synth.fleet_plant_params(n, 0.3, 12)
    for params in (P, None):
        h = crx.plant_step_tracks(S.d, S.ts, ids, xg, xc, u, params=params)
        dg, dc = _tracks_plain(S, S.ts, ids, xg, xc, u, params)
        assert np.array_equal(h["xglob"], dg) and np.array_equal(h["xcurv"], dc) and np.isfinite(dc).all()

    def refused(match, ts=S.ts, track_id=ids, params=P):
        with pytest.raises(RuntimeError, match=match) as e:
            crx.plant_step_tracks(S.d, ts, track_id, xg, xc, u, params=params)
        assert "rc=%d " % CRX_ERR_ARG in str(e.value)

    for car, val in ((5, -1), (66, 4), (0, 99)):
        bad = ids.copy()
        bad[car] = val
        refused(r"track_id of car %d\b" % car, track_id=bad)
    bad = ids.copy()
    bad[[9, 30]] = 4
    refused(r"track_id of car 9\b", track_id=bad)                                           # the first offending car
    for t, val in ((0, 0), (3, 12), (2, -1)):
        ns = S.ts.n_seg.copy()
        ns[t] = val
        refused(r"n_seg of track %d\b" % t, ts=abi.TrackSet(S.ts.tracks, ns, S.ts.lap_length))
    ns = S.ts.n_seg.copy()
    ns[[1, 2]] = 0
    refused(r"n_seg of track 1\b", ts=abi.TrackSet(S.ts.tracks, ns, S.ts.lap_length))   # the first offending track
    for t, val in ((0, 0.0), (1, -49.8), (2, np.inf), (3, np.nan)):
        ll = S.ts.lap_length.copy()
        ll[t] = val
        refused(r"lap_length of track %d\b" % t, ts=abi.TrackSet(S.ts.tracks, S.ts.n_seg, ll))
    for car, col, val in ((5, 0, 0.0), (66, 3, -0.024), (40, 7, np.nan)):
        bp = P.copy()
        bp[car, col] = val
        refused(r"params of car %d\b" % car, params=bp)
    with pytest.raises(ValueError):
        crx.plant_step_tracks(S.d, S.ts, ids[:-1], xg, xc, u)
    # the _dev entries check what they can: the set's dimensions
    import torch

    from crx import torch_api

    sd = _set_dev(S, S.ts, ids)
    for nt, stride in ((0, 11), (9, 11), (4, 0), (4, 65)):
        sd.n_tracks, sd.seg_stride = nt, stride
        with pytest.raises(RuntimeError, match="rc=%d " % CRX_ERR_ARG):
            torch_api._call("crx_plant_step_tracks_plain_dev", C.byref(S.d), C.c_int(n), C.c_int(nt), C.c_int(stride), torch_api._ptr(sd.tracks),
                            torch_api._ptr(sd.n_seg), torch_api._ptr(sd.lap_length), torch_api._ptr(sd.track_id), torch_api._ptr(S.t(xg)),
                            torch_api._ptr(S.t(xc)), torch_api._ptr(S.t(u)), None, torch_api._ptr(torch.empty((n, 6), dtype=torch.float64, device=S.dev)),
                            torch_api._ptr(torch.empty((n, 6), dtype=torch.float64, device=S.dev)), torch_api._stream())
    d0 = pref.desc_with(S.d, pref.desc_row(S.d))
    d0.m = 0.0                                                                              # the descriptor must still be a valid one
    with pytest.raises(RuntimeError, match="rc=-"):
        crx.plant_step_tracks(d0, S.ts, ids, xg, xc, u, params=P)


def test_g_cbf_prep_with_per_race_lap_lengths(gpu, S):
    """For every track, the races on it get the bits cbf_prep_dev computes with that track's scalar lap length: races just before and just
    after their own line, on lap 0 and lap 2, scripted cars beside them and a lap ahead."""
    import torch

    from crx import torch_api

    Bn, V, N, t_now, dt = 256, 3, 10, 1.3, 0.1
    ids = ref.interleaved(Bn)
    L = S.ts.lap_length[ids]
    rng = np.random.default_rng(17)
    xc = np.zeros((Bn, 6))
    xc[:, 0] = rng.uniform(0.4, 1.2, Bn)
    side = np.where(np.arange(Bn) // 4 % 2 == 0, -1.0, 1.0)                         # before / after the line
    lap = np.arange(Bn) // 8 % 3
    xc[:, 4] = lap * L + L + side * rng.uniform(0.0, 0.3, Bn)
    xc[:, 5] = rng.uniform(-0.3, 0.3, Bn)
    v = rng.uniform(0.1, 0.5, (Bn, V))
    gap = np.stack([rng.uniform(-1.0, 1.5, Bn), rng.uniform(-0.2, 0.8, Bn) + L, rng.uniform(2.0, 9.0, Bn)], axis=1)   # beside, a lap ahead, far
    s0 = xc[:, 4:5] + gap - v * t_now
    ey = rng.uniform(-0.4, 0.4, (Bn, V))

    def outs(n):
        return (torch.empty((n, V, N + 1), dtype=torch.float64, device=S.dev), torch.empty((n, V, N + 1), dtype=torch.float64, device=S.dev),
                torch.empty((n, V), dtype=torch.float64, device=S.dev), torch.empty((n,), dtype=torch.int32, device=S.dev))

    mixed = outs(Bn)
    torch_api.cbf_prep_laps_dev(N, S.t(L), t_now, dt, S.t(xc), S.t(s0), S.t(v), S.t(ey), *mixed)
    torch.cuda.synchronize()
    kept = mixed[3].cpu().numpy()
    assert (kept < V).any() and (kept >= 2).any() and (mixed[2].cpu().numpy() != 0.0).any()      # windows that filter, lap offsets that act
    for t in range(4):
        i = ids == t
        single = outs(int(i.sum()))
        torch_api.cbf_prep_dev(N, float(S.ts.lap_length[t]), t_now, dt, S.t(xc[i]), S.t(s0[i]), S.t(v[i]), S.t(ey[i]), *single)
        torch.cuda.synchronize()
        sel = S.t(i, torch.bool)
        for m, s in zip(mixed, single):
            assert torch.equal(m[sel], s), t
    # another track's lap length gives other arrays: the races are told apart
    wrong = outs(Bn)
    torch_api.cbf_prep_dev(N, float(S.ts.lap_length[0]), t_now, dt, S.t(xc), S.t(s0), S.t(v), S.t(ey), *wrong)
    torch.cuda.synchronize()
    assert not torch.equal(wrong[2], mixed[2])


def test_h_the_chain_on_different_tracks(gpu, orc, S):
    """PidLaps on 8 cars, two per track, 300 steps with given noise, every car starting 18 m before its own line: against control.pid + the
    oracle's noisy plant on the car's track + the per-track wrap on the host; identify() against the numpy mirror on the host log; the two
    l_shape cars retrace a single-track PidLaps of the same two cars."""
    import contextlib
    import io

    import torch

    from crx import montecarlo
    from system import system_identification

    Bn, steps, vt = 8, 300, 0.8
    ids = ref.interleaved(Bn)
    L = S.ts.lap_length[ids]
    z = np.random.default_rng(31).normal(size=(steps, Bn, 3))
    x0 = np.tile(np.array([0.3, 0, 0, 0, 0, 0.0]), (Bn, 1))
    x0[:, 0] += 0.01 * np.arange(Bn)
    x0[:, 4] = L - 18.0
    with contextlib.redirect_stdout(io.StringIO()):      # control.pid prints its solver time
        xh, uh = ref.pid_oracle_loop(orc, S.ts, ids, x0, z, vt)
    r = montecarlo.pid_laps(None, None, x0, x0, steps, vt=vt, noise_z=z, tracks=S.ts, track_id=ids)
    fit = r.identify(1e-9)
    torch.cuda.synchronize()
    xl, ul = r.x_log.cpu().numpy(), r.u_log.cpu().numpy()
    dx, du = np.abs(xl - xh).max(), np.abs(ul - uh).max()
    assert (np.diff(xh[:, :, 4], axis=1) < -1.0).any(axis=1).all() and (r.laps.cpu().numpy() == 1).all()      # every car crossed its own line
    assert (fit.status.cpu().numpy() == 0).all()
    A, Bm = fit.A.cpu().numpy(), fit.B.cpu().numpy()
    dW = 0.0
    for b in range(Bn):
        Ah, Bh, _ = system_identification.linear_regression(xh[b], uh[b], 1e-9)
        W = np.vstack([Ah.T, Bh.T])
        dW = max(dW, np.abs(np.vstack([A[b].T, Bm[b].T]) - W).max() / np.abs(W).max())
    print("test h: max|dx| %.3e max|du| %.3e (bound %g), max|dW|/max|W| %.3e (bound %g)" % (dx, du, X_TOL, dW, W_TOL))
    assert dx <= X_TOL and du <= X_TOL
    assert dW <= W_TOL
    i = ids == 0
    plain = montecarlo.pid_laps(S.ts.table(0), float(S.ts.lap_length[0]), x0[i], x0[i], steps, vt=vt, noise_z=z[:, i])
    torch.cuda.synchronize()
    assert np.array_equal(plain.x_log.cpu().numpy(), xl[i]) and np.array_equal(plain.u_log.cpu().numpy(), ul[i])


def _loops(kind, AB, S, ids, n=2, single=None):
    """`n` identically built loops of one kind, race b on track ids[b] -- or, with single = t, on table t alone (the shipped launches)."""
    from crx import montecarlo

    Bn = len(ids)
    rng = np.random.default_rng(7)
    x0 = np.zeros((Bn, 6))
    x0[:, 0] = rng.uniform(0.6, 0.9, Bn)
    x0[:, 4] = S.ts.lap_length[ids] - rng.uniform(0.2, 0.7, Bn)                  # close enough to cross their own lines inside 20 steps
    x0[:, 5] = rng.uniform(-0.1, 0.1, Bn)
    s0, v, ey = x0[:, 4:5] + np.tile([1.2, 3.0], (Bn, 1)), np.full((Bn, 2), 0.3), np.tile([0.2, -0.2], (Bn, 1))
    if single is None:
        tab, lap, kw, i = None, None, dict(tracks=S.ts, track_id=ids), slice(None)
    else:
        tab, lap, kw, i = S.ts.table(single), float(S.ts.lap_length[single]), {}, ids == single
    if kind == "lqr":
        return [montecarlo.LqrLaps(tab, lap, x0[i], x0[i], AB[0], AB[1], vt=0.8, **kw) for _ in range(n)]
    return [montecarlo.MpccbfRaces(tab, lap, WIDTH, AB[0], AB[1], x0[i], x0[i], s0[i], v[i], ey[i], vt=0.8, N=10, **kw) for _ in range(n)]


@pytest.mark.parametrize("kind", ["lqr", "mpccbf"])
def test_i_closed_loops_take_it(gpu, AB, S, kind):
    """One step of the loop on a track set = its own solver launch on the state before the step, then plant_step_tracks_wrap_dev by hand:
    the same bits (the scheme of test_gpu_plant_params.test_h)."""
    import torch

    from crx import torch_api

    ids = ref.interleaved(8)
    a, b = _loops(kind, AB, S, ids)
    assert torch.equal(a.xc, b.xc) and torch.equal(a.lap_length, S.t(S.ts.lap_length[ids]))
    a.step()
    if kind == "lqr":
        torch_api.lqr_step_dev(b.K, b.xc, b.xt, b.u)
        u, stride = b.u, 2
    else:
        torch_api.cbf_prep_laps_dev(b.N, b.lap_length, b.t, b.timestep, b.xc, b.s0, b.v, b.ey, b.obs_s, b.obs_e, b.lap_off, b.n_obs)
        torch_api.cbf_solve_dev(b.desc, b.xc, b.xt, b.obs_s, b.obs_e, b.lap_off, b.n_obs, ws=b.ws)
        u, stride = b.ws.U, 2 * b.N
    og, oc, laps = torch.empty_like(b.xg), torch.empty_like(b.xc), b.laps.clone()
    torch_api.plant_step_tracks_wrap_dev(b.plant, b.tracks, b.xg, b.xc, u, stride, og, oc, laps, noise_z=None, params=None)
    torch.cuda.synchronize()
    assert torch.isfinite(a.xc).all() and (a.xc[:, 4] != b.xc[:, 4]).all()                  # the cars moved
    assert torch.equal(a.xc, oc) and torch.equal(a.xg, og) and torch.equal(a.laps, laps)


def test_i_mpccbf_races_against_single_track_loops(gpu, AB, S):
    """20 steps of 8 races over the four tracks = four single-track loops over the same races: equal xc, u and status, step by step."""
    import torch

    ids = ref.interleaved(8)
    mixed = _loops("mpccbf", AB, S, ids, n=1)[0]
    singles = [_loops("mpccbf", AB, S, ids, n=1, single=t)[0] for t in range(4)]
    for k in range(20):
        mixed.step()
        for t, s in enumerate(singles):
            s.step()
            sel = S.t(ids == t, torch.bool)
            assert torch.equal(mixed.xc[sel], s.xc) and torch.equal(mixed.u[sel], s.u) and torch.equal(mixed.ws.status[sel], s.ws.status), (k, t)
            assert torch.equal(mixed.xg[sel], s.xg) and torch.equal(mixed.laps[sel], s.laps)
    torch.cuda.synchronize()
    assert torch.isfinite(mixed.xc).all() and (mixed.laps.cpu().numpy() == 1).sum() >= 4 and (mixed.ws.status.cpu().numpy() == 0).sum() >= 4
    # the glue restatement of the step takes the set too and lands where the launches do (the bound test_gpu_closed_loop.py holds glue=True to)
    a, b = _loops("mpccbf", AB, S, ids)
    a.step()
    b.step_glue()
    torch.cuda.synchronize()
    assert torch.equal(a.laps, b.laps) and (a.xc - b.xc).abs().max().item() <= 1e-9
