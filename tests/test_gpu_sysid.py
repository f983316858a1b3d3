"""crx_sysid_fit on the GPU (GPU box only): against the reference's own identification (tests/golden/sysid.npz), against the
numpy mirror (system.system_identification.linear_regression) on fuzzed logs and groups, bit identity across batches, the
singular case, the device-resident PID experiment (crx.montecarlo.pid_laps) and the device entry point against the host one."""
import os

import numpy as np
import pytest

import conftest

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
# closed loop of pid_laps against the reference's recorded run (measured on the MI355X: DESIGN.md section 10)
X_TOL = 1e-11
W_TOL = 1e-9


@pytest.fixture(scope="module")
def gpu():
    import crx

    return crx.init(0)


@pytest.fixture(scope="module")
def S():
    return np.load(os.path.join(conftest.GOLDEN, "sysid.npz"))


def _W(A, B):
    """W [8,6] from A [6,6], B [6,2] (S4: A = W'[:, 0:6], B = W'[:, 6:8])."""
    return np.vstack([np.asarray(A).T, np.asarray(B).T])


def _pairs(x, u):
    X = np.hstack((x[1:-1], u[1:-1]))
    return X, x[2:]


def _numpy_fit(X, Y, lamb):
    G = X.T @ X + lamb * np.eye(8)
    b = X.T @ Y
    return np.linalg.inv(G) @ b, G, b


def _fit_ratios(Wg, X, Y, lamb):
    """(max|W_gpu - W_numpy| / (K eps cond(G) max|W|), ||G W_gpu - b|| / (max(1e-12, K eps cond(G)) ||G|| ||W_gpu||), numpy's err):
    ratios <= 1 pass.  K = 128 covers the rounding of the Gram sums themselves (up to 20000 rows) that eps cond(G) leaves out: numpy
    against numpy with the Gram re-summed in 32-row chunks reaches 32 eps cond(G) max|W| on these logs, the GPU 34 (DESIGN.md
    section 10).  The residual keeps 1e-12 where G is well conditioned; an explicit inverse is not backward stable, and numpy's own W
    of a 5-row log at lamb = 1e-9 leaves 9e6 times that residual, so the bound grows with eps cond(G) there."""
    Wn, G, b = _numpy_fit(X, Y, lamb)
    c = np.linalg.cond(G)
    dW = np.abs(Wg - Wn).max() / (128 * EPS * c * np.abs(Wn).max())
    res = np.linalg.norm(G @ Wg - b) / (max(1e-12, 128 * EPS * c) * np.linalg.norm(G) * np.linalg.norm(Wg))
    E = X @ Wn - Y
    # err moves with W: |X (W_gpu - W_numpy)| <= max row 1-norm of X * max|W_gpu - W_numpy|
    err_tol = 1e-9 + np.abs(X).sum(1).max() * np.abs(Wg - Wn).max()
    return dW, res, np.vstack([E.max(0), E.min(0)]), err_tol


def _check_fit(Wg, X, Y, lamb, label):
    dW, res, err, err_tol = _fit_ratios(Wg, X, Y, lamb)
    assert dW <= 1.0 and res <= 1.0, (label, dW, res)
    return err, err_tol


def _logs(rng, lengths):
    """Random logs: states a slow random walk with a lap-like sawtooth in s, inputs a bounded random signal."""
    xs, us = [], []
    for T in lengths:
        x = np.cumsum(rng.normal(0, 0.05, (T, 6)), axis=0) + rng.normal(0, 1, 6)
        x[:, 4] = np.mod(np.arange(T) * 0.05 + rng.uniform(0, 20), 20.0)
        xs.append(x)
        us.append(rng.uniform(-1, 1, (T, 2)))
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return np.concatenate(xs), np.concatenate(us), off


def test_a_reference_log(gpu, S):
    import crx

    r = crx.sysid_fit(S["long/x"], S["long/u"], lamb=float(S["long/lamb"]))
    assert r["status"][0] == 0 and r["n_pairs"][0] == 4998
    Wr = _W(S["long/A"], S["long/B"])
    assert np.abs(_W(r["A"][0], r["B"][0]) - Wr).max() <= 1e-9 * np.abs(Wr).max()
    assert np.abs(r["err"][0] - S["long/err"]).max() <= 1e-10


@pytest.mark.parametrize("lamb", [1e-9, 1e-3, 1.0])
def test_b_fuzzed_logs_against_numpy(gpu, lamb):
    import crx

    rng = np.random.default_rng(5)
    lengths = rng.integers(2, 600, 2048)
    lengths[0], lengths[1] = 2, 3
    lengths[[7, 300, 1200, 2047]] = [20000, 8195, 4098, 12001]   # many tiles; tile edges
    x, u, off = _logs(rng, lengths)
    r = crx.sysid_fit(x, u, offsets=off, lamb=lamb)
    empty = lengths == 2   # T = 2: no pair, CRX_SKIPPED
    assert empty[0] and not empty[1]
    assert np.isnan(r["A"][empty]).all() and np.isnan(r["B"][empty]).all() and np.isnan(r["err"][empty]).all()
    bad = np.nonzero((r["status"] != np.where(empty, 4, 0)) | (r["n_pairs"] != lengths - 2))[0]
    assert bad.size == 0, [(int(l), int(lengths[l]), int(r["status"][l]), int(r["n_pairs"][l])) for l in bad[:10]]
    worst = [0.0, 0.0, 0.0]
    for l in np.nonzero(~empty)[0]:
        X, Y = _pairs(x[off[l]:off[l + 1]], u[off[l]:off[l + 1]])
        dW, res, err, err_tol = _fit_ratios(_W(r["A"][l], r["B"][l]), X, Y, lamb)
        dE = np.abs(r["err"][l] - err).max() / (err_tol * max(1.0, np.abs(err).max()))
        worst = [max(worst[0], dW), max(worst[1], res), max(worst[2], dE)]
    print("fuzz lamb %g: worst ratios dW %.3g residual %.3g err %.3g" % (lamb, *worst))
    assert max(worst) <= 1.0, worst


def test_c_groups(gpu):
    import crx

    rng = np.random.default_rng(6)
    lengths = rng.integers(2, 3000, 70)
    x, u, off = _logs(rng, lengths)
    go = np.array([0, 64, 65, 65, 70], dtype=np.int32)   # a 64-log group, a one-log group, an empty group, five logs
    r = crx.sysid_fit(x, u, offsets=off, group_offsets=go)
    assert list(r["status"]) == [0, 0, 4, 0]
    for g in (0, 3):
        parts = [_pairs(x[off[l]:off[l + 1]], u[off[l]:off[l + 1]]) for l in range(go[g], go[g + 1])]
        X, Y = np.vstack([p[0] for p in parts]), np.vstack([p[1] for p in parts])
        assert r["n_pairs"][g] == X.shape[0]
        err, err_tol = _check_fit(_W(r["A"][g], r["B"][g]), X, Y, 1e-9, g)
        assert np.abs(r["err"][g] - err).max() <= err_tol * max(1.0, np.abs(err).max())
    lone = crx.sysid_fit(x, u, offsets=off)
    for k in ("A", "B", "err", "n_pairs"):
        assert np.array_equal(r[k][1], lone[k][64]), k


def test_d_bit_identity(gpu, S):
    import crx

    x, u = S["long/x"], S["long/u"]
    alone = crx.sysid_fit(x, u)
    rng = np.random.default_rng(8)
    Bn = 4096
    xb = np.tile(x, (Bn, 1)) + np.repeat(rng.normal(0, 1e-3, (Bn, 1, 6)), len(x), axis=1).reshape(-1, 6)
    ub = np.tile(u, (Bn, 1))
    j = 1234
    xb[j * len(x):(j + 1) * len(x)] = x
    batch = crx.sysid_fit(xb.reshape(Bn, len(x), 6), ub)
    assert (batch["status"] == 0).all()
    pad = 777   # another offset: rows before the log belong to a first log
    xs = np.vstack([rng.normal(0, 1, (pad, 6)), x])
    us = np.vstack([rng.normal(0, 1, (pad, 2)), u])
    shifted = crx.sysid_fit(xs, us, offsets=np.array([0, pad, pad + len(x)]))
    for k in ("A", "B", "err"):
        assert np.array_equal(alone[k][0], batch[k][j]), k
        assert np.array_equal(alone[k][0], shifted[k][1]), k


def test_e_singular(gpu):
    import crx

    rng = np.random.default_rng(9)
    x, u, off = _logs(rng, [500, 500, 500])
    u[off[1]:off[2]] = 0.0
    r = crx.sysid_fit(x, u, offsets=off, lamb=0.0)
    assert list(r["status"]) == [0, 6, 0]
    assert np.isnan(r["A"][1]).all() and np.isnan(r["B"][1]).all() and np.isnan(r["err"][1]).all()
    ref = crx.sysid_fit(x, u, offsets=off[[0, 1]], lamb=0.0)
    assert np.array_equal(r["A"][0], ref["A"][0]) and np.array_equal(r["err"][0], ref["err"][0])
    sub = crx.sysid_fit(x[off[2]:], u[off[2]:], lamb=0.0)
    assert np.array_equal(r["A"][2], sub["A"][0]) and np.array_equal(r["err"][2], sub["err"][0])


def _track(S):
    from utils import racing_env

    return racing_env.ClosedTrack(S["track_spec"], track_width=1.0)


@pytest.mark.parametrize("name", ["long", "short"])
def test_f_pid_laps_against_reference(gpu, S, name):
    import torch

    from crx import montecarlo

    tr = _track(S)
    T, Bn = int(S[name + "/steps"]), 4
    x0 = np.tile(S[name + "/x0"], (Bn, 1))
    z = np.repeat(S[name + "/z"][:, None, :], Bn, axis=1)
    r = montecarlo.pid_laps(tr.point_and_tangent, tr.lap_length, x0, x0, T, vt=float(S[name + "/vt"]), noise_z=z)
    xl, ul = r.x_log.cpu().numpy(), r.u_log.cpu().numpy()
    for b in range(1, Bn):   # copies of the scenario: the same bits
        assert np.array_equal(xl[b], xl[0]) and np.array_equal(ul[b], ul[0])
    dx = np.abs(xl[0] - S[name + "/x"]).max()
    du = np.abs(ul[0] - S[name + "/u"]).max()
    ws = r.identify(float(S[name + "/lamb"]))
    torch.cuda.synchronize()
    assert (ws.status.cpu().numpy() == 0).all()
    Wr = _W(S[name + "/A"], S[name + "/B"])
    dW = np.abs(_W(ws.A[0].cpu().numpy(), ws.B[0].cpu().numpy()) - Wr).max() / np.abs(Wr).max()
    print("pid_laps %s: max|dx| %.3e max|du| %.3e max|dW|/max|W| %.3e" % (name, dx, du, dW))
    assert dx <= X_TOL and du <= X_TOL and dW <= W_TOL


def test_f_many_cars_with_device_noise(gpu, S):
    import torch

    from crx import montecarlo

    tr = _track(S)
    Bn, T = 4096, 5000
    rng = np.random.default_rng(10)
    vt = rng.uniform(0.4, 1.0, Bn)
    x0 = np.tile(S["long/x0"], (Bn, 1))
    r = montecarlo.pid_laps(tr.point_and_tangent, tr.lap_length, x0, x0, T, vt=vt, noise_seed=3)
    ws = r.identify(1e-9)
    torch.cuda.synchronize()
    ey = r.x_log[:, :, 5].abs().max().item()
    assert ey < 0.5, ey   # on the track (half width 0.5)
    assert (ws.status.cpu().numpy() == 0).all()
    assert (ws.n_pairs.cpu().numpy() == T - 2).all()
    assert (r.laps.cpu().numpy() >= 1).all()
    # a sample of the fits against the numpy mirror on the same logs
    from system import system_identification

    xl, ul = r.x_log.cpu().numpy(), r.u_log.cpu().numpy()
    for b in rng.choice(Bn, 8, replace=False):
        A, B, err = system_identification.linear_regression(xl[b], ul[b], 1e-9)
        W = _W(A, B)
        assert np.abs(_W(ws.A[b].cpu().numpy(), ws.B[b].cpu().numpy()) - W).max() <= 1e-8 * np.abs(W).max(), b


def test_g_device_matches_host(gpu):
    import torch

    import crx
    from crx import abi, torch_api

    rng = np.random.default_rng(11)
    lengths = rng.integers(2, 9000, 300)
    x, u, off = _logs(rng, lengths)
    go = np.array([0, 1, 50, 50, 299, 300], dtype=np.int32)
    h = crx.sysid_fit(x, u, offsets=off, group_offsets=go)
    hu = crx.sysid_fit(x, u, offsets=off)
    dev = torch.device("cuda", 0)
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)  # noqa: E731
    d = abi.sysid_desc()
    ws = torch_api.sysid_fit_dev(d, t(x), t(u), t(off, torch.int64), t(go, torch.int32))
    wu = torch_api.sysid_fit_dev(d, t(x), t(u), t(off, torch.int64), max_log_rows=20000)
    torch.cuda.synchronize()
    for k in ("A", "B", "err", "n_pairs", "status"):
        assert np.array_equal(getattr(ws, k).cpu().numpy(), h[k], equal_nan=k not in ("n_pairs", "status")), k
        assert np.array_equal(getattr(wu, k).cpu().numpy(), hu[k], equal_nan=k not in ("n_pairs", "status")), k
