"""One BicycleDynamicsParam set per car on the GPU (crx_plant_cars_kernel behind crx_plant_step_params_dev / crx_plant_step_params and the
plant_params argument of every closed loop of crx.montecarlo).  The reference for car b is the oracle at batch 1 with the descriptor's ten
fields set to row b (tests/plant_params_ref.py; tests/test_plant_params_cpu.py holds the oracle to the reference's vehicle_dynamics on
non-default parameters).  Batches 1, 67 (a full wave and a partial one) and 300 (across the 256-thread block boundary), track l_shape."""
import numpy as np
import pytest

import helpers
import plant_params_ref as ref

pytestmark = pytest.mark.gpu

PLANT_TOL = 1e-12     # tests/test_gpu_parity.py test_plant_step, the same state draw
X_TOL = 1e-11         # tests/test_gpu_sysid.py: the PID closed loop against the host loop
W_TOL = 1e-8          # tests/test_gpu_sysid.py test_f_many_cars_with_device_noise: the fit against the numpy mirror, relative
B_BIG = 300
CRX_ERR_ARG = -1      # include/crx.h


@pytest.fixture(scope="module")
def gpu():
    import crx

    return crx.init(0)


@pytest.fixture(scope="module")
def T():
    """Track table, lap length, plant descriptor and the tensor helpers."""
    import torch

    tr = ref.track()
    dev = torch.device("cuda", 0)

    class Ctx:
        tab, L = tr.point_and_tangent, tr.lap_length
        track = tr

        @staticmethod
        def t(a, dt=torch.float64):
            return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)

    from crx import abi

    Ctx.d = abi.plant_desc(Ctx.tab.shape[0], Ctx.L)
    Ctx.dev = dev
    return Ctx


def _wrap_dev(T, d, xg, xc, u, u_stride, z, P, laps0=None):
    """plant_step_wrap_dev on host arrays -> (xglob_next, xcurv_next, laps) as host arrays.  u: the array the plant reads at u_stride."""
    import torch

    from crx import torch_api

    n = xg.shape[0]
    og, oc = torch.empty((n, 6), dtype=torch.float64, device=T.dev), torch.empty((n, 6), dtype=torch.float64, device=T.dev)
    laps = T.t(np.zeros(n) if laps0 is None else laps0, torch.int32)
    torch_api.plant_step_wrap_dev(d, T.t(T.tab), T.t(xg), T.t(xc), T.t(u), u_stride, og, oc, laps, noise_z=None if z is None else T.t(z),
                                  params=None if P is None else T.t(P))
    torch.cuda.synchronize()
    return og.cpu().numpy(), oc.cpu().numpy(), laps.cpu().numpy()


def _plain_dev(T, d, xg, xc, u, P):
    import torch

    from crx import torch_api

    og, oc = torch_api.plant_step_dev(d, T.t(T.tab), T.t(xg), T.t(xc), T.t(u), params=None if P is None else T.t(P))
    torch.cuda.synchronize()
    return og.cpu().numpy(), oc.cpu().numpy()


def test_a_parity_one_step(gpu, orc, T):
    """No wrap, no noise, B = 300 (two blocks), every car against the oracle on its own parameter row."""
    from crx import synth

    rng = np.random.default_rng(11)
    xc, xg, u = ref.draw_states(rng, B_BIG, T.L)
    P = synth.fleet_plant_params(B_BIG, 0.3, 11)
    og, oc = ref.oracle_cars(orc, T.d, T.tab, xg, xc, u, P)
    gg, gc = _plain_dev(T, T.d, xg, xc, u, P)
    print("test a: B = %d, worst |xcurv - oracle| %.3g, |xglob - oracle| %.3g (bound %g)" % (B_BIG, np.abs(gc - oc).max(), np.abs(gg - og).max(), PLANT_TOL))
    np.testing.assert_allclose(gc, oc, rtol=0, atol=PLANT_TOL)
    np.testing.assert_allclose(gg, og, rtol=0, atol=PLANT_TOL)
    # the parameters matter: the same cars on the descriptor's set move elsewhere
    _, dc = _plain_dev(T, T.d, xg, xc, u, None)
    assert np.abs(dc - gc).max() > 1e-3
    # crx_plant_step_params_dev itself (lap wrap applied): the same cars, the wrap added on the host
    wg, wc, laps = _wrap_dev(T, T.d, xg, xc, u, 2, None, P)
    hc, crossed = ref.wrap(gc, T.L)
    assert np.array_equal(wc, hc) and np.array_equal(wg, gg) and np.array_equal(laps, crossed)


def test_b_noise_wrap_strided_inputs(gpu, orc, T):
    from crx import synth

    xc, xg, U, z, near = ref.noisy_case(B_BIG, T.L)
    P = synth.fleet_plant_params(B_BIG, 0.3, ref.NOISY_SEED)
    og, oc = ref.oracle_cars(orc, T.d, T.tab, xg, xc, np.ascontiguousarray(U[:, 0, :]), P, z)
    on_line = np.abs(oc[:, 4] - T.L) <= 1e-9          # a last-place difference could flip the wrap there
    assert on_line.sum() <= 3
    hc, crossed = ref.wrap(oc, T.L)
    laps0 = np.arange(B_BIG) % 5
    gg, gc, laps = _wrap_dev(T, T.d, xg, xc, U, 24, z, P, laps0=laps0)
    keep = ~on_line
    print("test b: B = %d, %d cars crossed, %d left out, worst |xcurv - oracle| %.3g, |xglob - oracle| %.3g (bound %g)" % (
        B_BIG, crossed.sum(), on_line.sum(), np.abs(gc - hc)[keep].max(), np.abs(gg - og)[keep].max(), PLANT_TOL))
    np.testing.assert_allclose(gc[keep], hc[keep], rtol=0, atol=PLANT_TOL)
    np.testing.assert_allclose(gg[keep], og[keep], rtol=0, atol=PLANT_TOL)
    assert np.array_equal(laps[keep], (laps0 + crossed)[keep])
    assert crossed.sum() >= 20 and (crossed == 0).sum() >= 200
    # laps is optional (the C entry itself: the torch wrapper always passes a counter)
    import ctypes as C

    import torch

    import crx
    from crx import torch_api

    og2, oc2 = torch.empty((B_BIG, 6), dtype=torch.float64, device=T.dev), torch.empty((B_BIG, 6), dtype=torch.float64, device=T.dev)
    fn = crx.lib().crx_plant_step_params_dev
    fn.restype = C.c_int
    tt = [T.t(T.tab), T.t(xg), T.t(xc), T.t(U), T.t(z), T.t(P)]
    p = lambda a: C.c_void_p(a.data_ptr())   # noqa: E731
    rc = fn(C.byref(T.d), C.c_int(B_BIG), p(tt[0]), p(tt[1]), p(tt[2]), p(tt[3]), C.c_int(24), p(tt[4]), p(tt[5]), p(og2), p(oc2), C.c_void_p(0),
            torch_api._stream())
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(oc2.cpu().numpy(), gc) and np.array_equal(og2.cpu().numpy(), gg)


def test_c_bit_identity_with_the_shared_launch(gpu, T):
    """Every row = the descriptor's ten values: the per-car kernel computes the bits of the shared one, noise and wrap included."""
    xc, xg, U, z, _ = ref.noisy_case(B_BIG, T.L)
    P = np.tile(ref.desc_row(T.d), (B_BIG, 1))
    laps0 = np.arange(B_BIG) % 3
    sg, sc, sl = _wrap_dev(T, T.d, xg, xc, U, 24, z, None, laps0=laps0)
    cg, cc, cl = _wrap_dev(T, T.d, xg, xc, U, 24, z, P, laps0=laps0)
    assert np.array_equal(cc, sc) and np.array_equal(cg, sg) and np.array_equal(cl, sl)
    assert (sl > laps0).sum() >= 20


def test_d_position_independence(gpu, T):
    """One car -- state, input, noise, parameter row -- alone, as car 66 of 67 and as car 299 of 300: the same bits, whatever the others hold."""
    from crx import synth

    xc, xg, U, z, _ = ref.noisy_case(B_BIG, T.L, seed=5)
    P = synth.fleet_plant_params(B_BIG, 0.3, 5)
    u = np.ascontiguousarray(U[:, 0, :])
    j = 3                                            # near the line: its wrap acts or not, alike in every position
    one = (xg[j:j + 1], xc[j:j + 1], u[j:j + 1], z[j:j + 1], P[j:j + 1])
    ag, ac, al = _wrap_dev(T, T.d, one[0], one[1], one[2], 2, one[3], one[4])
    for n in (67, B_BIG):
        arrs = [a[:n].copy() for a in (xg, xc, u, z, P)]
        for a, o in zip(arrs, one):
            a[n - 1] = o[0]
        g, c, l = _wrap_dev(T, T.d, arrs[0], arrs[1], arrs[2], 2, arrs[3], arrs[4])
        assert np.array_equal(g[n - 1], ag[0]) and np.array_equal(c[n - 1], ac[0]) and l[n - 1] == al[0], n
        # other neighbours, a bad one among them: car n - 1 does not move, and only the bad car goes non-finite
        arrs[4][: n - 1] = P[1:n][::-1]
        arrs[4][0, 0] = 0.0                                     # m = 0 in car 0 (the device entry cannot read the rows)
        g2, c2, l2 = _wrap_dev(T, T.d, arrs[0], arrs[1], arrs[2], 2, arrs[3], arrs[4])
        assert np.array_equal(g2[n - 1], ag[0]) and np.array_equal(c2[n - 1], ac[0]) and l2[n - 1] == al[0], n
        assert not np.isfinite(c2[0]).all() and np.isfinite(c2[1:]).all() and np.isfinite(g2[1:]).all()


def test_e_descriptor_values_are_ignored(gpu, T):
    from crx import synth

    xc, xg, U, z, _ = ref.noisy_case(B_BIG, T.L, seed=6)
    P = synth.fleet_plant_params(B_BIG, 0.3, 6)
    d2 = ref.desc_with(T.d, ref.desc_row(T.d))
    d2.m, d2.Iz, d2.Df = 123.0, 7.0, 0.1
    a = _wrap_dev(T, T.d, xg, xc, U, 24, z, P)
    b = _wrap_dev(T, d2, xg, xc, U, 24, z, P)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    # ... and are what moves the cars without params
    c = _wrap_dev(T, d2, xg, xc, U, 24, z, None)
    assert np.abs(c[1] - a[1]).max() > 1e-3
    # the descriptor must still be a valid one
    d2.m = 0.0
    with pytest.raises(RuntimeError, match="rc=-"):
        _wrap_dev(T, d2, xg, xc, U, 24, z, P)


def test_f_host_pointer_entry(gpu, T):
    import crx
    from crx import synth

    n = 67
    rng = np.random.default_rng(12)
    xc, xg, u = ref.draw_states(rng, n, T.L)
    P = synth.fleet_plant_params(n, 0.3, 12)
    h = crx.plant_step(T.d, T.tab, xg, xc, u, params=P)
    dg, dc = _plain_dev(T, T.d, xg, xc, u, P)
    assert np.array_equal(h["xglob"], dg) and np.array_equal(h["xcurv"], dc)
    # against crx_plant_step_params_dev where its lap wrap does not act
    wg, wc, _ = _wrap_dev(T, T.d, xg, xc, u, 2, None, P)
    same_lap = dc[:, 4] <= T.L
    assert same_lap.sum() >= 20 and np.array_equal(wc[same_lap], h["xcurv"][same_lap]) and np.array_equal(wg, h["xglob"])
    # params = None: crx_plant_step as it is
    h0, hn = crx.plant_step(T.d, T.tab, xg, xc, u), crx.plant_step(T.d, T.tab, xg, xc, u, params=None)
    sg, sc = _plain_dev(T, T.d, xg, xc, u, None)
    assert np.array_equal(h0["xcurv"], hn["xcurv"]) and np.array_equal(h0["xglob"], hn["xglob"])
    assert np.array_equal(h0["xcurv"], sc) and np.array_equal(h0["xglob"], sg)
    # rows the host entry refuses, naming the car
    for car, col, val in ((5, 0, 0.0), (66, 3, -0.024), (40, 7, np.nan), (0, 5, np.inf)):
        bad = P.copy()
        bad[car, col] = val
        with pytest.raises(RuntimeError, match=r"rc=-\d+ .*car %d\b" % car) as e:
            crx.plant_step(T.d, T.tab, xg, xc, u, params=bad)
        assert "rc=%d " % CRX_ERR_ARG in str(e.value)
    bad = P.copy()
    bad[[9, 30], 0] = -1.0
    with pytest.raises(RuntimeError, match=r"car 9\b"):      # the first offending car
        crx.plant_step(T.d, T.tab, xg, xc, u, params=bad)
    with pytest.raises(ValueError):
        crx.plant_step(T.d, T.tab, xg, xc, u, params=P[:-1])


def test_g_the_chain_on_different_cars(gpu, orc, T):
    """PidLaps on four different cars (one of them the default) against control.pid + the oracle's noisy plant + the wrap on the host, car
    by car; identify() against the numpy mirror on the host log; the default car retraces the run without plant_params; the identified
    models differ."""
    import contextlib
    import io

    import torch

    from crx import abi, montecarlo
    from system import system_identification

    Bn, steps, vt = 4, 300, 0.8
    P = abi.plant_params(Bn) * ref.CHAIN_FACTORS
    z = np.random.default_rng(31).normal(size=(steps, Bn, 3))
    x0 = np.tile(np.array([0.3, 0, 0, 0, 0, 0.0]), (Bn, 1))
    with contextlib.redirect_stdout(io.StringIO()):      # control.pid prints its solver time
        xh, uh = ref.pid_oracle_loop(orc, T.tab, T.L, x0, P, z, vt)
    r = montecarlo.pid_laps(T.tab, T.L, x0, x0, steps, vt=vt, noise_z=z, plant_params=P)
    fit = r.identify(1e-9)
    torch.cuda.synchronize()
    xl, ul = r.x_log.cpu().numpy(), r.u_log.cpu().numpy()
    dx, du = np.abs(xl - xh).max(), np.abs(ul - uh).max()
    assert (np.diff(xh[:, :, 4], axis=1) < -1.0).any(axis=1).all() and (r.laps.cpu().numpy() >= 1).all()      # every car crossed the line
    assert (fit.status.cpu().numpy() == 0).all()
    A, Bm = fit.A.cpu().numpy(), fit.B.cpu().numpy()
    dW = 0.0
    for b in range(Bn):
        Ah, Bh, _ = system_identification.linear_regression(xh[b], uh[b], 1e-9)
        W = np.vstack([Ah.T, Bh.T])
        dW = max(dW, np.abs(np.vstack([A[b].T, Bm[b].T]) - W).max() / np.abs(W).max())
    dA = min(np.abs(A[b] - A[0]).max() for b in range(1, Bn))
    print("test g: max|dx| %.3e max|du| %.3e (bound %g), max|dW|/max|W| %.3e (bound %g), min max|A_b - A_0| %.3g" % (dx, du, X_TOL, dW, W_TOL, dA))
    assert dx <= X_TOL and du <= X_TOL
    assert dW <= W_TOL
    assert dA > 1e-3
    plain = montecarlo.pid_laps(T.tab, T.L, x0[:1], x0[:1], steps, vt=vt, noise_z=z[:, :1])
    torch.cuda.synchronize()
    assert np.array_equal(plain.x_log.cpu().numpy()[0], xl[0]) and np.array_equal(plain.u_log.cpu().numpy()[0], ul[0])


def _loops(kind, AB, g, T, P, Bn):
    """Two identically built loops of one kind on B different cars: (the one that steps, the one whose solver launch is replayed)."""
    from crx import montecarlo

    rng = np.random.default_rng(7)
    x0 = np.zeros((Bn, 6))
    x0[:, 0] = rng.uniform(0.6, 0.9, Bn)
    x0[:, 5] = rng.uniform(-0.1, 0.1, Bn)
    if kind == "lqr":
        return [montecarlo.LqrLaps(T.tab, T.L, x0, x0, AB[0], AB[1], vt=0.8, plant_params=P) for _ in range(2)]
    if kind == "mpccbf":
        s0, v, ey = np.tile([1.2, 3.0], (Bn, 1)), np.full((Bn, 2), 0.3), np.tile([0.2, -0.2], (Bn, 1))
        return [montecarlo.MpccbfRaces(T.tab, T.L, T.track.width, AB[0], AB[1], x0, x0, s0, v, ey, vt=0.8, N=10, plant_params=P) for _ in range(2)]
    if kind == "ilqr":
        return [montecarlo.IlqrRaces(T.tab, T.L, AB[0], AB[1], x0, x0, np.full(Bn, 1.5), np.full(Bn, 0.3), np.full(Bn, 0.2), vt=0.8, N=20,
                                     max_iter=30, plant_params=P) for _ in range(2)]
    assert kind == "lmpc"
    d, ss, us, qf, time_ss, lin_points, lin_input = helpers.lmpc_lap_setup(g, T.track)
    xl = np.tile(g["lmpc/x"][0], (Bn, 1))
    xg = np.tile(g["lap1/xglob"][-1], (Bn, 1))
    tile = lambda a: np.tile(a[None], (Bn,) + (1,) * a.ndim)   # noqa: E731
    return [montecarlo.LmpcLaps(T.tab, T.L, T.track.width, tile(ss), tile(us), tile(qf), tile(time_ss), np.full(Bn, 2, dtype=np.int32), xl, xg,
                                tile(lin_points), tile(lin_input), plant_params=P) for _ in range(2)]


def _replay_solver(kind, b):
    """The loop's own solver launch on its current state -> (u, u_stride) as its step hands them to the plant."""
    from crx import torch_api

    if kind == "lqr":
        torch_api.lqr_step_dev(b.K, b.xc, b.xt, b.u)
        return b.u, 2
    if kind == "mpccbf":
        torch_api.cbf_prep_dev(b.N, b.lap_length, b.t, b.timestep, b.xc, b.s0, b.v, b.ey, b.obs_s, b.obs_e, b.lap_off, b.n_obs)
        torch_api.cbf_solve_dev(b.desc, b.xc, b.xt, b.obs_s, b.obs_e, b.lap_off, b.n_obs, ws=b.ws)
        return b.ws.U, 2 * b.N
    if kind == "ilqr":
        obs_s, obs_e, lap_off = b.predictions()
        torch_api.ilqr_solve_dev(b.desc, b.xc, b.xt, obs_s, obs_e, lap_off, b.n_obs, ws=b.ws)
        return b.ws.U, 2 * b.N
    b._plan(b.lin_points, b.lin_input, False)
    return b.ws.U[:, 0, :].contiguous(), 2


@pytest.mark.parametrize("kind", ["lqr", "mpccbf", "ilqr", "lmpc"])
def test_h_closed_loops_take_it(gpu, AB, golden_racing_game, T, kind):
    """One step of the loop on five different cars = its solver launch on the state before the step, then plant_step_wrap_dev with the
    loop's parameter rows applied by hand: the same bits."""
    import torch

    from crx import synth, torch_api

    Bn = 5
    P = synth.fleet_plant_params(Bn, 0.3, 8)
    a, b = _loops(kind, AB, golden_racing_game, T, P, Bn)
    assert torch.equal(a.xc, b.xc) and torch.equal(a.plant_params, T.t(P))
    a.step()
    u, stride = _replay_solver(kind, b)
    outs = []
    for params in (b.plant_params, None):
        og, oc, laps = torch.empty_like(b.xg), torch.empty_like(b.xc), b.laps.clone()
        torch_api.plant_step_wrap_dev(b.plant, b.tab, b.xg, b.xc, u, stride, og, oc, laps, noise_z=None, params=params)
        outs.append((og, oc, laps))
    torch.cuda.synchronize()
    og, oc, laps = outs[0]
    assert torch.isfinite(a.xc).all() and (a.xc[:, 4] != b.xc[:, 4]).all()                  # the cars moved
    assert torch.equal(a.xc, oc) and torch.equal(a.xg, og) and torch.equal(a.laps, laps)
    assert not torch.equal(a.xc, outs[1][1])                                                # ... and not as the default car does
