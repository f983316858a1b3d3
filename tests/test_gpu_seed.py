"""Seed laps on the GPU (crx_seed_commit_dev, crx_seed_log_dev, crx.montecarlo.SeedLaps; include/crx.h "Seed laps", S1-S6): every car's own
PID lap and MPC-LTI lap become its own safe set.  The kernels are held to tests/seed_model.py bit for bit; the loop to the reference's own
recording of the two laps (tests/golden/racing_game.npz) at the bounds the project already holds its device PID loop and its MPC-LTI lap
to; cars that finish at different steps to the same cars seeded alone, bit for bit."""
import numpy as np
import pytest

import plant_params_ref as ref
import seed_model

pytestmark = pytest.mark.gpu

LAP0_TOL = 1e-11      # tests/test_gpu_sysid.py X_TOL: the device PID loop against the host loop
LAP1_TOL = 1e-5       # tests/test_gpu_closed_loop.py:146-150: the MPC-LTI lap against the reference's recording
# The first learning-MPC steps from the SEEDED safe set against the reference's recording (test_d).  Not derivable: the seeded lap 1 is
# itself only 1e-5 from the recording and feeds regressions whose normal equations reach condition 3e11 (include/crx.h, learning-MPC prep).
# Measured once on an MI355X: see LMPC_DEV_MEASURED; the bound is ten times that (the run is deterministic, the
# margin is for compiler and driver updates).
LMPC_DEV_MEASURED = 3.26e-6   # max |u - lmpc/U| over the ten steps; max |x - lmpc/x| = 4.41e-7
LMPC_DEV_TOL = 3.26e-5


@pytest.fixture(scope="module")
def gpu():
    import crx

    return crx.init(0)


@pytest.fixture(scope="module")
def track():
    return ref.track()


def _t(a, dtype=None):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=torch.device("cuda", 0))


# ---- the kernels against the model ---------------------------------------------------------------------------------------------------------
def _crafted(Bn, P, N, L):
    """Cars in every phase, crossing and not; car 1: one free log row and no crossing (-> phase 3, flag 2); car 2: a solver status that is
    not converged (flag 1); car 3: frozen, 1e-3 before the line, with a plant output that crossed (S4 puts laps back); the last car of
    B = 257 sits behind the block boundary."""
    rng = np.random.default_rng(Bn)
    c = dict(phase=rng.integers(0, 4, Bn).astype(np.int32), seed_status=rng.integers(0, 4, Bn).astype(np.int32),
             vt=rng.uniform(0.5, 0.9, Bn), eyt=rng.uniform(-0.1, 0.1, Bn), x=rng.normal(size=(Bn, 6)), U_mpc=rng.normal(size=(Bn, N, 2)),
             mpc_status=rng.choice([0, 0, 1, 4, 5], Bn).astype(np.int32), u=rng.normal(size=(Bn, 2)),
             xglob_prev=rng.normal(size=(Bn, 6)), xcurv=rng.normal(size=(Bn, 6)), xglob=rng.normal(size=(Bn, 6)),
             laps_prev=rng.integers(0, 3, Bn).astype(np.int32), n_log=rng.integers(1, P - 1, Bn).astype(np.int32),
             crossed=rng.integers(0, 2, Bn).astype(np.int32), m_mpc=rng.integers(0, 2, Bn).astype(np.int32),
             log_x=rng.normal(size=(Bn, P, 6)), log_u=rng.normal(size=(Bn, P, 2)))
    c["x"][:, 4] = rng.uniform(0.0, L, Bn)
    c["xcurv"][:, 4] = rng.uniform(0.0, L, Bn)
    c["laps"] = (c["laps_prev"] + rng.integers(0, 2, Bn)).astype(np.int32)
    c["phase"][:5] = [0, 1, 1, 2, 3]
    c["laps"][0] = c["laps_prev"][0] + 1                                 # car 0 finishes its PID lap
    c["n_log"][1], c["laps"][1] = P - 1, c["laps_prev"][1]               # car 1 runs out of log rows
    c["mpc_status"][2], c["seed_status"][2], c["laps"][2] = 1, 0, c["laps_prev"][2] + 1   # car 2: CRX_MAX_ITER, and it finishes its MPC-LTI lap
    c["x"][3, 4], c["xcurv"][3, 4], c["laps"][3] = L - 1e-3, 0.07, c["laps_prev"][3] + 1   # car 3: frozen next to the line
    if Bn > 5:
        c["phase"][-1], c["laps"][-1] = 1, c["laps_prev"][-1] + 1
    return c


@pytest.mark.parametrize("Bn", [5, 257])
def test_a_kernels_against_the_model(gpu, Bn):
    import torch
    from crx import torch_api

    P, N, L = 7, 10, 19.25
    c = _crafted(Bn, P, N, L)
    m = {k: v.copy() for k, v in c.items()}
    seed_model.commit(m["phase"], m["vt"], m["eyt"], m["x"], m["U_mpc"], m["mpc_status"], m["seed_status"], m["u"])
    seed_model.log(L, m["x"], m["xglob_prev"], m["xcurv"], m["xglob"], m["u"], m["laps"], m["laps_prev"], m["log_x"], m["log_u"], m["n_log"],
                   m["crossed"], m["phase"], m["seed_status"], m["m_mpc"])
    assert m["phase"][1] == 3 and m["seed_status"][1] & 2 and m["seed_status"][2] == 1 and m["phase"][2] == 2 and m["phase"][0] == 1
    assert m["laps"][3] == c["laps_prev"][3] and m["crossed"][3] == 0 and np.array_equal(m["xcurv"][3], c["x"][3])
    d = {k: _t(v) for k, v in c.items()}
    torch_api.seed_commit_dev(N, d["phase"], d["vt"], d["eyt"], d["x"], d["U_mpc"], d["mpc_status"], d["seed_status"], d["u"])
    torch_api.seed_log_dev(L, d["x"], d["xglob_prev"], d["xcurv"], d["xglob"], d["u"], d["laps"], d["laps_prev"], d["log_x"], d["log_u"],
                           d["n_log"], d["crossed"], d["phase"], d["seed_status"], d["m_mpc"])
    torch.cuda.synchronize()
    for k in c:
        np.testing.assert_array_equal(d[k].cpu().numpy(), m[k], err_msg=k)
    with pytest.raises(ValueError):
        torch_api.seed_log_dev(L, d["x"], d["xglob_prev"], d["x"], d["xglob"], d["u"], d["laps"], d["laps_prev"], d["log_x"], d["log_u"],
                               d["n_log"], d["crossed"], d["phase"], d["seed_status"], d["m_mpc"])


# ---- the reference's scenario --------------------------------------------------------------------------------------------------------------
def _host(r):
    import torch

    torch.cuda.synchronize()
    names = ("ss", "us", "qf", "time_ss", "it", "xc", "xg", "laps", "phase", "seed_status", "m_mpc", "n_log", "traj_status")
    return {k: getattr(r, k).cpu().numpy() for k in names}


@pytest.fixture(scope="module")
def seeded(gpu, track, AB):
    """B = 4 copies of auto_racing_game_test's ego from the zero state, vt = 0.7, zero noise, the shipped model; run to the hand-over."""
    from crx import montecarlo

    z = np.zeros((4, 6))
    r = montecarlo.SeedLaps(track.point_and_tangent, track.lap_length, track.width, AB[0], AB[1], z, z, vt=0.7)
    r.run(700)
    return r, _host(r)


def test_b_the_reference_scenario(seeded, golden_racing_game):
    g = golden_racing_game
    r, h = seeded
    assert r.k == 576                                                     # the first read of the count after step 554
    assert (h["phase"] == 2).all() and (h["seed_status"] == 0).all() and (h["it"] == 2).all() and (h["m_mpc"] == 0).all()
    for k, v in h.items():
        np.testing.assert_array_equal(v[1:], v[:1].repeat(3, axis=0), err_msg=k)   # four copies, the same bits
    np.testing.assert_array_equal(h["time_ss"][:, :2], np.tile([294, 260], (4, 1)))
    ref_ss, ref_u, ref_q = g["ss/ss0"].transpose(2, 0, 1), g["ss/u0"].transpose(2, 0, 1), g["ss/Qfun0"].T
    ss, us, qf = h["ss"][0], h["us"][0], h["qf"][0]
    for lap, tol in ((0, LAP0_TOL), (1, LAP1_TOL)):
        print("lap %d: max |ss - ss0| = %.3g, max |u - u0| = %.3g (bound %g)" % (lap, np.abs(ss[lap] - ref_ss[lap]).max(),
                                                                                 np.abs(us[lap] - ref_u[lap]).max(), tol))
    np.testing.assert_allclose(ss[0], ref_ss[0], rtol=0, atol=LAP0_TOL)
    np.testing.assert_allclose(us[0], ref_u[0], rtol=0, atol=LAP0_TOL)
    np.testing.assert_allclose(ss[1], ref_ss[1], rtol=0, atol=LAP1_TOL)
    np.testing.assert_allclose(us[1], ref_u[1], rtol=0, atol=LAP1_TOL)
    np.testing.assert_array_equal(ss[2:], ref_ss[2:]); np.testing.assert_array_equal(us[2:], ref_u[2:])   # untouched: 10000
    np.testing.assert_array_equal(qf, ref_q)                              # step counts: exact
    inp = r.lmpc_inputs()
    np.testing.assert_allclose(inp["lin_points"][0].cpu().numpy(), ref_ss[0][1:14], rtol=0, atol=LAP0_TOL)
    np.testing.assert_allclose(inp["lin_input"][0].cpu().numpy(), ref_u[0][1:13], rtol=0, atol=LAP0_TOL)
    np.testing.assert_allclose(h["xc"][0], g["lmpc/x"][0], rtol=0, atol=LAP1_TOL)
    np.testing.assert_allclose(h["xg"][0], g["lap1/xglob"][-1], rtol=0, atol=LAP1_TOL)


# ---- cars that finish at different times ---------------------------------------------------------------------------------------------------
def test_c_cars_finish_at_different_times(gpu, track, AB):
    import torch
    from crx import montecarlo

    vt = np.linspace(0.5, 0.9, 6)
    z = np.zeros((6, 6))
    tab, L, W = track.point_and_tangent, track.lap_length, track.width
    r = montecarlo.SeedLaps(tab, L, W, AB[0], AB[1], z, z, vt=vt)
    log = []
    while r.k < 1000 and (r.k % 32 or r.k == 0 or r.n_driving()):
        r.step()
        log.append((r.phase.clone(), r.xc.clone(), r.xg.clone(), r.laps.clone()))
    h = _host(r)
    assert (h["phase"] == 2).all() and (h["seed_status"] == 0).all(), (h["phase"], h["seed_status"])
    total = h["time_ss"][:, :2].sum(axis=1)
    print("steps to the hand-over per car:", total, "laps:", h["time_ss"][:, :2].tolist())
    assert len(set(total.tolist())) == 6 and (np.diff(total) < 0).all()  # a faster target, a shorter pair of laps
    # from the step a car reaches phase 2 its states and lap counter never change again
    ph, xc, xg, laps = (torch.stack([row[i] for row in log]).cpu().numpy() for i in range(4))
    for b in range(6):
        k2 = int(np.argmax(ph[:, b] == 2))
        assert ph[k2, b] == 2 and k2 + 1 == total[b] and (ph[k2:, b] == 2).all()
        assert b < 5 or len(ph) - k2 >= 100                               # the fastest car stood for a long while
        for a in (xc, xg, laps):
            np.testing.assert_array_equal(a[k2:, b], a[k2:k2 + 1, b].repeat(len(a) - k2, axis=0))
    # every car equals, bit for bit, the same car seeded alone
    for b in range(6):
        one = montecarlo.SeedLaps(tab, L, W, AB[0], AB[1], z[:1], z[:1], vt=vt[b]).run(1000)
        h1 = _host(one)
        for k in ("ss", "us", "qf", "time_ss", "it", "xc", "xg", "laps", "phase", "seed_status"):
            np.testing.assert_array_equal(h1[k][0], h[k][b], err_msg="car %d %s" % (b, k))


# ---- into the learning MPC, on the device --------------------------------------------------------------------------------------------------
def test_d_into_the_learning_mpc(seeded, track, golden_racing_game):
    import torch
    from crx import montecarlo

    g = golden_racing_game
    r, _ = seeded
    lm = montecarlo.LmpcLaps(track.point_and_tangent, track.lap_length, track.width, **r.lmpc_inputs())
    assert lm.ss.is_cuda and lm.ss.data_ptr() != r.ss.data_ptr()
    n = int(g["lmpc_first_uncertified"])
    assert n == 10
    xs, us, st, ps = [lm.xc.clone()], [], [], []
    for _ in range(n):
        lm.step()
        xs.append(lm.xc.clone()); us.append(lm.u_old.clone()); st.append(lm.ws.status.clone()); ps.append(lm.pws.status.clone())
    torch.cuda.synchronize()
    xs, us, st, ps = (torch.stack(a).cpu().numpy() for a in (xs, us, st, ps))
    # the reference certified these steps: exact conditions
    assert (st == 0).all() and (ps == 0).all(), (st, ps)
    np.testing.assert_array_equal(xs[:, 1:], xs[:, :1].repeat(3, axis=1))
    dev_x, dev_u = float(np.abs(xs[:, 0] - g["lmpc/x"][:n + 1]).max()), float(np.abs(us[:, 0] - g["lmpc/U"][:n, 0]).max())
    print("learning-MPC steps 0..%d from the seeded safe set: max |x - lmpc/x| = %.3g, max |u - lmpc/U| = %.3g (measured %s, bound %s)" % (
        n, dev_x, dev_u, LMPC_DEV_MEASURED, LMPC_DEV_TOL))
    assert LMPC_DEV_TOL is not None and max(dev_x, dev_u) <= LMPC_DEV_TOL


# ---- a fleet ------------------------------------------------------------------------------------------------------------------------------
def test_e_a_fleet(gpu, track, AB):
    import scenarios
    import torch
    from crx import montecarlo, synth

    Bn = 8
    tab, L, W = track.point_and_tangent, track.lap_length, track.width
    P = synth.fleet_plant_params(Bn, 0.1, 7)
    z = np.zeros((Bn, 6))
    fit = montecarlo.pid_laps(tab, L, z, z, 600, vt=0.7, noise_seed=3, plant_params=P).identify()
    assert (fit.status.cpu().numpy() == 0).all()
    r = montecarlo.SeedLaps(tab, L, W, None, None, z, z, vt=0.7, models=(fit.A, fit.B), plant_params=P).run(1100)
    h = _host(r)
    print("fleet: phase", h["phase"], "seed_status", h["seed_status"], "time_ss", h["time_ss"][:, :2].tolist())
    assert (h["phase"] == 2).all(), (h["phase"], h["seed_status"])
    assert np.isfinite(h["xc"]).all() and np.isfinite(h["xg"]).all() and (h["it"] == 2).all()
    assert len({tuple(t) for t in h["time_ss"][:, :2].tolist()}) > 1      # different cars, different laps
    cars = scenarios.RACING_GAME["cars"]
    s0, v, ey = (np.tile([c[i] for c in cars], (Bn, 1)) for i in (1, 2, 3))
    game = montecarlo.GameLaps(tab, L, W, AB[0], AB[1], scenarios.table("optimal_traj", "xcurv_l_shape"), **r.lmpc_inputs(), car_s0=s0,
                               car_v=v, car_ey=ey, plant_params=P)
    for _ in range(30):
        game.step()
    torch.cuda.synchronize()
    assert torch.isfinite(game.lm.xc).all() and torch.isfinite(game.lm.xg).all() and torch.isfinite(game.u).all()
