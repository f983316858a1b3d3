"""crx_ilqr_solve on the GPU (GPU box only): against the reference's own answers (tests/golden/ilqr.npz), against the numpy model
(tests/ilqr_model.py) on recorded and fuzzed problems, batch independence, the reference's ilqr_test closed loop through the mirror
(tests/golden/closed_loop_ilqr.npz) and the device-resident races (crx.montecarlo.ilqr_races).

Comparison rule against the model: iters and status equal, U, X and cost within 1e-9 (relative to max(1, |value|)).  A problem
may differ only where the model reports a deciding margin (accept, convergence or lambda test) below 1e-10 -- a near tie whose
outcome the last bits of a cost sum decide; such problems are listed and budgeted at one per 200."""
import numpy as np
import pytest

import conftest
import ilqr_model

pytestmark = pytest.mark.gpu

Q_DEF = np.diag([10.0, 0.0, 0.0, 4.0, 0.0, 40.0])
R_DEF = np.diag([0.1, 0.1])
TIE = 1e-10


def _close(a, b, tol=1e-9):
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))))


def _agree(g, m, j):
    return (g["iters"][j] == m["iters"][j] and g["status"][j] == m["status"][j] and _close(g["U"][j], m["U"][j])
            and _close(g["X"][j], m["X"][j]) and _close(g["cost"][j], m["cost"][j]))


def _check_vs_model(g, m, label):
    bad = [j for j in range(len(m["iters"])) if not _agree(g, m, j)]
    ties = [j for j in bad if m["min_margin"][j] < TIE]
    real = [j for j in bad if m["min_margin"][j] >= TIE]
    assert not real, "%s: %d problems differ from the model with margins >= %g: %s" % (
        label, len(real), TIE, [(j, int(g["iters"][j]), int(m["iters"][j]), float(m["min_margin"][j])) for j in real[:8]])
    return ties


@pytest.fixture(scope="module")
def gpu():
    import crx

    return crx.init(0)


@pytest.fixture(scope="module")
def G():
    return np.load(conftest.GOLDEN + "/ilqr.npz")


def test_reference_cases(gpu, G, AB):
    from crx import abi

    A, B = AB
    ties = []
    for i in range(len(G["u0"])):
        N = int(G["N"][i])
        d = abi.ilqr_desc(N, A, B, max_iter=int(G["max_iter"][i]), l_sum=float(G["l_sum"][i]), w_sum=float(G["w_sum"][i]))
        args = (G["x0"][i][None], G["xt"][i][None], G["obs_s"][i][None, None, :N + 1], G["obs_ey"][i][None, None, :N + 1],
                np.array([[G["lap_off"][i]]]), np.ones(1, dtype=np.int32))
        g = gpu.ilqr_solve(d, *args)
        m = ilqr_model.solve(A, B, Q_DEF, R_DEF, *args, N, max_iter=int(G["max_iter"][i]), l_sum=float(G["l_sum"][i]),
                             w_sum=float(G["w_sum"][i]))
        if not _agree(g, m, 0):
            assert m["min_margin"][0] < TIE, (i, int(g["iters"][0]), int(m["iters"][0]), float(m["min_margin"][0]))
            ties.append(i)
            continue
        assert np.abs(g["U"][0, 0] - G["u0"][i]).max() <= 1e-9, i
        assert g["iters"][0] == G["iters"][i] and g["status"][0] == G["stop"][i], i
    assert len(ties) <= 1, ties


def _fuzz_batch(rng, Bn, N, A, B):
    """Bn problems of horizon N around the reference's scenario with 0..6 obstacles (the multi-obstacle sum included)."""
    x0 = np.column_stack([rng.uniform(0, 1.2, Bn), rng.uniform(-0.05, 0.05, Bn), rng.uniform(-0.3, 0.3, Bn),
                          rng.uniform(-0.2, 0.2, Bn), rng.uniform(0, 40, Bn), rng.uniform(-0.4, 0.4, Bn)])
    xt = np.zeros((Bn, 6))
    xt[:, 0] = rng.choice([0.6, 0.8, 1.0], Bn)
    xt[:, 5] = np.where(rng.random(Bn) < 0.3, rng.uniform(-0.2, 0.2, Bn), 0.0)
    V = 6
    k = np.arange(N + 1)
    s0 = x0[:, 4:5] + rng.uniform(-3, 3, (Bn, V))
    vo = rng.uniform(0, 1, (Bn, V))
    obs_s = s0[:, :, None] + (vo[:, :, None] * 0.1) * k
    obs_ey = np.repeat(rng.uniform(-0.4, 0.4, (Bn, V))[:, :, None], N + 1, axis=2)
    L = 19.22957795362994
    lap_off = ilqr_model.lap_offset(x0[:, 4:5], obs_s[:, :, 0], L)
    n_obs = rng.integers(0, V + 1, Bn).astype(np.int32)
    return x0, xt, obs_s, obs_ey, lap_off, n_obs


def test_fuzz_against_model(gpu, AB):
    from crx import abi

    rng = np.random.default_rng(2024)
    A0, B0 = AB
    A1 = A0 * (1 + 0.02 * rng.standard_normal(A0.shape)) * (A0 != 0)
    B1 = B0 * (1 + 0.05 * rng.standard_normal(B0.shape))
    ties, total = [], 0
    for N in range(1, 65):
        A, B = (A0, B0) if N % 2 else (A1, B1)
        args = _fuzz_batch(rng, 64, N, A, B)
        d = abi.ilqr_desc(N, A, B, n_obs_max=6)
        g = gpu.ilqr_solve(d, *args)
        m = ilqr_model.solve(A, B, Q_DEF, R_DEF, *args, N)
        ties += [(N, j) for j in _check_vs_model(g, m, "N=%d" % N)]
        total += 64
        assert (m["status"] != ilqr_model.MAX_ITER).any()
    assert total == 4096
    assert len(ties) <= total // 200, ties


def test_batch_independence_and_mask(gpu, AB):
    import torch

    from crx import abi, torch_api

    A, B = AB
    N = 50
    rng = np.random.default_rng(7)
    args = _fuzz_batch(rng, 4096, N, A, B)
    d = abi.ilqr_desc(N, A, B, n_obs_max=6)
    dev = torch.device("cuda", 0)
    t = [torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in args]
    full = torch_api.ilqr_solve_dev(d, *t)
    torch.cuda.synchronize()
    F = {k: getattr(full, k).cpu().numpy() for k in ("X", "U", "cost", "status", "iters")}
    for j in (0, 1, 2047, 4095):
        one = gpu.ilqr_solve(d, *(a[j:j + 1] for a in args))
        for k in F:
            assert np.array_equal(one[k][0], F[k][j]), (j, k)
    active = torch.as_tensor((np.arange(4096) % 3 == 0).astype(np.int32), device=dev)
    ws = torch_api.IlqrWorkspace(d, 4096, dev)
    for k in ("X", "U", "cost"):
        getattr(ws, k).fill_(-7.0)
    ws.iters.fill_(-3)
    torch_api.ilqr_solve_dev(d, *t, ws=ws, active=active)
    torch.cuda.synchronize()
    on = active.cpu().numpy().astype(bool)
    M = {k: getattr(ws, k).cpu().numpy() for k in ("X", "U", "cost", "status", "iters")}
    assert (M["status"][~on] == abi.CRX_SKIPPED).all()
    for k in ("X", "U", "cost"):
        assert (M[k][~on] == -7.0).all(), k
        assert np.array_equal(M[k][on], F[k][on]), k
    assert (M["iters"][~on] == -3).all() and np.array_equal(M["iters"][on], F["iters"][on])
    assert np.array_equal(M["status"][on], F["status"][on])


def _ilqr_race(car=(4.0, 0.2, 0.1), steps=500, record=None):
    """car_racing/tests/ilqr_test.py --track-layout l_shape --simulation through the mirror (zero noise)."""
    import scenarios
    from racing import offboard
    from utils import base

    race = scenarios.Race(scenarios.make_track("l_shape", 1.0), 0.1)
    race.policy(offboard.iLQRRacing(base.iLQRRacingParam(vt=0.8), race.ego.system_param))
    race.scripted_car("car1", *car)
    race.run(steps * 0.1)
    return race


def test_closed_loop_matches_reference(gpu, AB, monkeypatch):
    import crx

    ref = np.load(conftest.GOLDEN + "/closed_loop_ilqr.npz")
    calls = []
    solve = crx.ilqr_solve

    def rec(desc, *a):
        r = solve(desc, *a)
        calls.append((desc.l_sum, desc.w_sum, desc.N, desc.max_iter) + tuple(np.array(x) for x in a) + (int(r["iters"][0]),))
        return r

    monkeypatch.setattr(crx, "ilqr_solve", rec)
    race = _ilqr_race(steps=int(ref["steps"]))
    e = np.array(race.ego.xcurv_log)
    it = np.array([c[-1] for c in calls])
    assert e.shape == ref["ego_xcurv"].shape and len(it) == len(ref["iters"])
    diff = np.flatnonzero((it != ref["iters"]) | (np.abs(e - ref["ego_xcurv"]).max(axis=1) > 1e-6))
    if len(diff) == 0:
        np.testing.assert_allclose(np.array(race.cars[0].xcurv_log), ref["car1_xcurv"], atol=1e-12)
        return
    # a decision flipped: it must be a near tie of the model at the first differing step; story level after it
    k = int(diff[0])
    A, B = AB
    l_sum, w_sum, N, max_iter = calls[k][:4]
    m = ilqr_model.solve(A, B, Q_DEF, R_DEF, *calls[k][4:10], N, max_iter=max_iter, l_sum=l_sum, w_sum=w_sum)
    assert m["min_margin"][0] < TIE, ("step %d differs without a near tie" % k, float(m["min_margin"][0]))
    np.testing.assert_allclose(e[:k], ref["ego_xcurv"][:k], atol=1e-6)
    _story(race, ref)


def _progress(xcurv, L):
    s = xcurv[:, 4]
    return s[-1] + L * np.sum(np.diff(s) < -0.5 * L)


def _story(race, ref):
    L = float(ref["lap_length"])
    e, r = np.array(race.ego.xcurv_log), ref["ego_xcurv"]
    assert abs(_progress(e, L) - _progress(r, L)) <= 0.05
    car = ref["car1_xcurv"]

    def closest(x):
        ds = np.abs(((x[:, 4] - car[:, 4]) + L / 2) % L - L / 2)
        return np.min(np.hypot(ds, x[:, 5] - car[:, 5]))

    assert abs(closest(e) - closest(r)) <= 0.05


def test_races_match_single_race_mirror(gpu, AB):
    from crx import montecarlo
    import scenarios

    A, B = AB
    track = scenarios.make_track("l_shape", 1.0)
    ref = np.load(conftest.GOLDEN + "/closed_loop_ilqr.npz")
    Bn = 64
    rng = np.random.default_rng(3)
    s0, v, ey = rng.uniform(2.0, 8.0, Bn), rng.uniform(0.1, 0.5, Bn), rng.uniform(-0.3, 0.3, Bn)
    s0[0], v[0], ey[0] = 4.0, 0.2, 0.1                          # race 0 = the reference's ilqr_test scenario
    steps = int(ref["steps"])
    r = montecarlo.ilqr_races(track.point_and_tangent, track.lap_length, A, B, np.zeros((Bn, 6)), np.zeros((Bn, 6)), s0, v, ey,
                              steps, vt=0.8)
    # race 0 against the reference's own closed loop
    np.testing.assert_array_equal(r["iters"][:, 0], ref["iters"])
    np.testing.assert_allclose(r["xcurv"][1:, 0], ref["ego_xcurv"], atol=1e-6)
    # races 0..3 against the single-race mirror loop for 100 steps
    for j in range(4):
        race = _ilqr_race(car=(s0[j], v[j], ey[j]), steps=100)
        np.testing.assert_allclose(r["xcurv"][1:101, j], np.array(race.ego.xcurv_log), atol=1e-6, err_msg="race %d" % j)
    assert np.isfinite(r["xcurv"]).all()
