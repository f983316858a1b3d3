"""crx_lqr_design / crx_lqr_step_dev and the per-problem models of crx_ilqr_solve on the GPU (GPU box only): against the reference's
recorded control.lqr calls and closed loop (tests/golden/closed_loop_lqr.npz), against the numpy models (tests/lqr_model.py,
tests/ilqr_model.py), the status table, batch independence, and the device-resident chain PID laps -> identify -> LQR design -> laps.

Comparison rule against lqr_model: iters and status equal, max|dK| <= 1e-11 max|K| per car (P alike).  Two correct float64 and
extended-precision implementations differ by about 1e-15 on the generator used here (tests/test_lqr_cpu.py); the kernel differs from
numpy in FMA contraction and in the 2x2 inverse only.  A car whose stop decision came within 1e-8 (relative) of a tie in the model
may be left out, at most one car in a hundred."""
import ctypes

import numpy as np
import pytest

import conftest
import ilqr_model
import lqr_model

pytestmark = pytest.mark.gpu

Q_DEF = np.diag([10.0, 0.0, 0.0, 4.0, 0.0, 40.0])
R_DEF = np.diag([0.1, 0.1])
REL = 1e-11
TIE_LQR = 1e-8
TIE = 1e-10        # iLQR: the rule of tests/test_gpu_ilqr.py


@pytest.fixture(scope="module")
def gpu():
    import crx

    return crx.init(0)


@pytest.fixture(scope="module")
def LQ():
    return np.load(conftest.GOLDEN + "/closed_loop_lqr.npz")


@pytest.fixture(scope="module")
def fuzz(AB):
    """Generator G: 71 models as batches of 1, 3 and 67, with the model's answers for max_iter 0, 1, 2, 50 (computed once)."""
    A, B, s = lqr_model.draw_models(np.random.default_rng(11), *AB, 71)
    return dict(A=A, B=B, s=s, parts=((0, 1), (1, 4), (4, 71)),
                model={it: lqr_model.design(A, B, Q_DEF, R_DEF, it) for it in (0, 1, 2, 50)})


def _rel(g, m):
    """Per car: max|g - m| / max|m| over the car's matrix."""
    return np.abs(g - m).max(axis=(1, 2)) / np.abs(m).max(axis=(1, 2))


def _check_vs_model(g, m, label, with_P=True):
    """The comparison rule of the module docstring; returns (cars left out, worst relative deviation of the others)."""
    out = [j for j in range(len(m["iters"])) if m["margin"][j] < TIE_LQR]
    keep = np.array([j for j in range(len(m["iters"])) if j not in out], dtype=int)
    assert np.array_equal(g["iters"][keep], m["iters"][keep]), (label, g["iters"][keep], m["iters"][keep])
    assert np.array_equal(g["status"][keep], m["status"][keep]), (label, g["status"][keep], m["status"][keep])
    worst = float(_rel(g["K"][keep], m["K"][keep]).max())
    if with_P:
        worst = max(worst, float(_rel(g["P"][keep], m["P"][keep]).max()))
    assert worst <= REL, (label, worst)
    return out, worst


def test_1_reference_calls(gpu, LQ, AB):
    import torch

    from crx import abi, torch_api

    A, B = AB
    dev = torch.device("cuda", 0)
    worst = 0.0
    for i in range(len(LQ["calls_u"])):
        Q, R, it = LQ["calls_Q"][i], LQ["calls_R"][i], int(LQ["calls_max_iter"][i])
        m = lqr_model.design(A, B, Q, R, it)
        g = gpu.lqr_design(abi.lqr_desc(Q=Q, R=R, max_iter=it), A, B)
        assert g["iters"][0] == m["iters"][0], i
        assert g["status"][0] == m["status"][0] and g["status"][0] in (abi.CRX_CONVERGED, abi.CRX_MAX_ITER), i
        u = torch.zeros((1, 2), dtype=torch.float64, device=dev)
        torch_api.lqr_step_dev(torch.as_tensor(g["K"], device=dev), torch.as_tensor(LQ["calls_x"][i][None], device=dev),
                               torch.as_tensor(LQ["calls_xt"][i][None], device=dev), u)
        u, ur = u.cpu().numpy()[0], LQ["calls_u"][i]
        dev_i = float((np.abs(u - ur) / np.maximum(1.0, np.abs(ur))).max())
        worst = max(worst, dev_i)
        assert dev_i <= 1e-10, (i, u, ur)
    print("test 1: worst |u - calls_u| / max(1, |u|) = %.3g (bound 1e-10)" % worst)


def test_2_fuzz_against_model(gpu, fuzz):
    from crx import abi

    left, total, worst = [], 0, 0.0
    for it in (0, 1, 2, 50):
        m = fuzz["model"][it]
        d = abi.lqr_desc(max_iter=it)
        for lo, hi in fuzz["parts"]:
            mm = {k: v[lo:hi] for k, v in m.items()}
            g = gpu.lqr_design(d, fuzz["A"][lo:hi], fuzz["B"][lo:hi])
            out, w = _check_vs_model(g, mm, "max_iter=%d batch=%d" % (it, hi - lo))
            left += [(it, lo + j) for j in out]
            worst = max(worst, w)
            total += hi - lo
            # P = NULL and P given: the same K bits
            g0 = gpu.lqr_design(d, fuzz["A"][lo:hi], fuzz["B"][lo:hi], want_P=False)
            assert "P" not in g0 and np.array_equal(g0["K"], g["K"]) and np.array_equal(g0["iters"], g["iters"])
    assert total == 284
    assert len(left) <= total // 100, left
    m50 = fuzz["model"][50]
    assert {lqr_model.CONVERGED, lqr_model.MAX_ITER} == set(m50["status"])     # both ends of the loop are in the draw
    print("test 2: worst max|dK| / max|K|, max|dP| / max|P| = %.3g (bound %g), %d of %d cars left out, smallest margin %.3g" % (
        worst, REL, len(left), total, min(fuzz["model"][it]["margin"].min() for it in (1, 2, 50))))


def test_3_transposed_shortcut_is_not_what_runs(gpu, fuzz):
    """L2: (B'PA)' in place of A'(PB) lands on other iterates; the kernel sides with the model."""
    from crx import abi

    j = np.flatnonzero(fuzz["s"] == 5e-2)
    A, B = fuzz["A"][j], fuzz["B"][j]
    m = {k: v[j] for k, v in fuzz["model"][50].items()}
    v = lqr_model.design(A, B, Q_DEF, R_DEF, 50, transposed_shortcut=True)
    differs = (v["iters"] != m["iters"]) | (_rel(v["K"], m["K"]) > REL)
    assert differs.any(), "the draw has no car on which the shortcut shows"
    g = gpu.lqr_design(abi.lqr_desc(), A, B)
    far = differs & (m["margin"] >= TIE_LQR)
    assert far.any()
    assert np.array_equal(g["iters"][far], m["iters"][far]) and (_rel(g["K"][far], m["K"][far]) <= REL).all()
    print("test 3: the shortcut differs on %d of %d cars" % (differs.sum(), len(j)))


def test_4_status_table(gpu, AB):
    import torch

    from crx import abi, torch_api

    A0, B0 = AB
    A, B = np.repeat(A0[None], 5, axis=0), np.repeat(B0[None], 5, axis=0)
    A[1, 2, 3] = np.nan
    B[2, 0, 1] = np.inf
    A[3, 5, 5] = -np.inf
    g = gpu.lqr_design(abi.lqr_desc(), A, B)
    m = lqr_model.design(A, B, Q_DEF, R_DEF)
    assert list(g["status"]) == [abi.CRX_MAX_ITER, abi.CRX_SINGULAR, abi.CRX_SINGULAR, abi.CRX_SINGULAR, abi.CRX_MAX_ITER]
    assert np.array_equal(g["status"], m["status"]) and np.array_equal(g["iters"], m["iters"])
    assert np.isnan(g["K"][1:4]).all() and np.isnan(g["P"][1:4]).all()
    assert np.array_equal(g["K"][0], g["K"][4]) and np.isfinite(g["K"][0]).all() and np.isfinite(g["P"][0]).all()
    # all-zero B with R = 0: a zero determinant in the first step
    z = gpu.lqr_design(abi.lqr_desc(R=np.zeros((2, 2))), A0, np.zeros((6, 2)))
    assert z["status"][0] == abi.CRX_SINGULAR and np.isnan(z["K"]).all() and np.isnan(z["P"]).all() and z["iters"][0] == 1
    z0 = gpu.lqr_design(abi.lqr_desc(R=np.zeros((2, 2)), max_iter=0), A0, np.zeros((6, 2)))
    assert z0["status"][0] == abi.CRX_SINGULAR and np.isnan(z0["K"]).all() and z0["iters"][0] == 0
    # L1: max_iter = 0 is the gain of P = Q
    k0 = gpu.lqr_design(abi.lqr_desc(max_iter=0), A0, B0)
    m0 = lqr_model.design(A0, B0, Q_DEF, R_DEF, 0)
    assert k0["iters"][0] == 0 and k0["status"][0] == abi.CRX_MAX_ITER and np.array_equal(k0["P"][0], Q_DEF)
    assert (_rel(k0["K"], m0["K"]) <= REL).all()
    # a masked car: CRX_SKIPPED, outputs untouched
    dev = torch.device("cuda", 0)
    ws = torch_api.LqrWorkspace(5, dev)
    ws.K.fill_(-7.0)
    ws.P.fill_(-7.0)
    ws.iters.fill_(-7)
    ws.status.fill_(-7)
    active = torch.tensor([1, 1, 0, 1, 0], dtype=torch.int32, device=dev)
    torch_api.lqr_design_dev(abi.lqr_desc(), torch.as_tensor(A, device=dev), torch.as_tensor(B, device=dev), ws=ws, active=active)
    torch.cuda.synchronize()
    st, K, P, it = ws.status.cpu().numpy(), ws.K.cpu().numpy(), ws.P.cpu().numpy(), ws.iters.cpu().numpy()
    assert list(st) == [abi.CRX_MAX_ITER, abi.CRX_SINGULAR, abi.CRX_SKIPPED, abi.CRX_SINGULAR, abi.CRX_SKIPPED]
    assert (K[[2, 4]] == -7.0).all() and (P[[2, 4]] == -7.0).all() and (it[[2, 4]] == -7).all()
    assert np.array_equal(K[0], g["K"][0]) and np.array_equal(P[0], g["P"][0]) and it[0] == g["iters"][0]


def test_5_bit_identity(gpu, fuzz, AB):
    import torch

    from crx import abi, torch_api

    d = abi.lqr_desc()
    A, B = fuzz["A"][4:71], fuzz["B"][4:71]          # the batch of 67
    full = gpu.lqr_design(d, A, B)
    big_A, big_B, _ = lqr_model.draw_models(np.random.default_rng(12), *AB, 4096)
    for j in (5, 40):
        one = gpu.lqr_design(d, A[j], B[j])
        for pos in (0, 33, 66):
            Ap, Bp = A.copy(), B.copy()
            Ap[pos], Bp[pos] = A[j], B[j]
            at = gpu.lqr_design(d, Ap, Bp)
            for k in ("K", "P", "iters"):
                assert np.array_equal(at[k][pos], one[k][0]), (j, pos, k)
        for k in ("K", "P", "iters", "status"):
            assert np.array_equal(full[k][j], one[k][0]), (j, k)
        big_A[2047 + j], big_B[2047 + j] = A[j], B[j]
    big = gpu.lqr_design(d, big_A, big_B)
    for j in (5, 40):
        for k in ("K", "P", "iters", "status"):
            assert np.array_equal(big[k][2047 + j], full[k][j]), (j, k)
    # the host entry against the device entry
    dev = torch.device("cuda", 0)
    ws = torch_api.lqr_design_dev(d, torch.as_tensor(big_A, device=dev), torch.as_tensor(big_B, device=dev))
    torch.cuda.synchronize()
    for k in ("K", "P", "iters", "status"):
        assert np.array_equal(getattr(ws, k).cpu().numpy(), big[k]), k


def test_6_closed_loop(gpu, LQ, AB):
    import scenarios
    from crx import montecarlo

    track = scenarios.make_track("l_shape", 0.8)
    steps = 200
    r = montecarlo.lqr_laps(track.point_and_tangent, track.lap_length, np.zeros((2, 6)), np.zeros((2, 6)), steps, *AB, vt=0.8)
    assert (r["design_status"] == 1).all() and (r["design_iters"] == 50).all()     # the shipped model: CRX_MAX_ITER after 50 steps
    dev_x = float(np.abs(r["xcurv"][1:steps + 1, 0] - LQ["ego_xcurv"][:steps]).max())
    print("test 6: max|xcurv - ego_xcurv| over %d steps = %.3g (bound 1e-6)" % (steps, dev_x))
    assert dev_x <= 1e-6
    assert np.array_equal(r["xcurv"][:, 1], r["xcurv"][:, 0]) and np.array_equal(r["u"][:, 1], r["u"][:, 0])


def test_7_pipeline(gpu):
    import scenarios
    import torch

    from crx import abi, montecarlo, torch_api

    track = scenarios.make_track("l_shape", 0.8)
    Bn = 8
    vt = np.linspace(0.5, 0.9, Bn)
    x0 = np.zeros((Bn, 6))
    fit = montecarlo.pid_laps(track.point_and_tangent, track.lap_length, x0, x0, 300, vt=vt, noise_seed=5).identify()
    d = abi.lqr_desc()
    ws = torch_api.lqr_design_dev(d, fit.A, fit.B)
    torch.cuda.synchronize()
    fs, st = fit.status.cpu().numpy(), ws.status.cpu().numpy()
    assert (fs == 0).sum() >= Bn - 1 and fs[3] == 0, fs
    assert np.isin(st[fs == 0], (abi.CRX_CONVERGED, abi.CRX_MAX_ITER)).all(), st
    A, B = fit.A.cpu().numpy(), fit.B.cpu().numpy()
    good = np.flatnonzero(fs == 0)
    g = {k: getattr(ws, k).cpu().numpy() for k in ("K", "P", "iters", "status")}
    m = lqr_model.design(A[good], B[good], Q_DEF, R_DEF)
    out, worst = _check_vs_model({k: v[good] for k, v in g.items()}, m, "identified models")
    assert not out, out
    print("test 7: identified models, worst deviation from the model %.3g, design status %s" % (worst, st))
    laps = montecarlo.LqrLaps(track.point_and_tangent, track.lap_length, x0, x0, fit.A, fit.B, vt=0.8, noise_seed=6)
    assert np.array_equal(laps.K.cpu().numpy(), g["K"])
    for _ in range(50):
        laps.step()
    torch.cuda.synchronize()
    xc = laps.xc.cpu().numpy()
    assert np.isfinite(xc[good]).all() and np.isfinite(laps.u.cpu().numpy()[good]).all()
    assert (xc[good, 4] > 0.5).all(), xc[:, 4]     # the cars moved
    # a failed fit's NaN model: that car is CRX_SINGULAR, the others keep their bits
    A2 = fit.A.clone()
    A2[3] = float("nan")
    ws2 = torch_api.lqr_design_dev(d, A2, fit.B)
    torch.cuda.synchronize()
    assert ws2.status[3].item() == abi.CRX_SINGULAR and torch.isnan(ws2.K[3]).all() and torch.isnan(ws2.P[3]).all()
    others = [j for j in range(Bn) if j != 3]
    for k in ("K", "P", "iters", "status"):
        a, b = getattr(ws2, k).cpu().numpy()[others], g[k][others]
        assert np.array_equal(a, b, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b), k


def _ilqr_fuzz_batch(rng, Bn, N):
    """The recipe of tests/test_gpu_ilqr.py's fuzz generator: Bn problems of horizon N around the reference's scenario with 0..6
    obstacles."""
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


def _close(a, b, tol=1e-9):
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))))


def _dev9(a, b):
    return float((np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(1.0, np.abs(b))).max())


KEYS = ("X", "U", "cost", "status", "iters")


def test_8_ilqr_per_problem_models(gpu, AB):
    import torch

    from crx import abi, torch_api

    rng = np.random.default_rng(2025)
    mA, mB, _ = lqr_model.draw_models(rng, *AB, 5, scales=(2e-2,))
    Bn = 67
    which = np.arange(Bn) % 5
    A_b, B_b = mA[which], mB[which]
    ties, total, worst = [], 0, 0.0
    dev = torch.device("cuda", 0)
    for N in (1, 2, 50, 64):
        args = _ilqr_fuzz_batch(rng, Bn, N)
        d0 = abi.ilqr_desc(N, *AB, n_obs_max=6)
        mixed = gpu.ilqr_solve(d0, *args, models=(A_b, B_b))                                       # (b)
        for i in range(5):
            idx = np.flatnonzero(which == i)
            sub = tuple(a[idx] for a in args)
            per = gpu.ilqr_solve(d0, *sub, models=(A_b[idx], B_b[idx]))                           # (a)
            shared = gpu.ilqr_solve(abi.ilqr_desc(N, mA[i], mB[i], n_obs_max=6), *sub)
            for k in KEYS:
                assert np.array_equal(per[k], shared[k]), (N, i, k)
                assert np.array_equal(mixed[k][idx], per[k]), (N, i, k)
            m = ilqr_model.solve(mA[i], mB[i], Q_DEF, R_DEF, *sub, N)                              # (c)
            for jj, j in enumerate(idx):
                ok = (per["iters"][jj] == m["iters"][jj] and per["status"][jj] == m["status"][jj] and _close(per["U"][jj], m["U"][jj])
                      and _close(per["X"][jj], m["X"][jj]) and _close(per["cost"][jj], m["cost"][jj]))
                if not ok:
                    assert m["min_margin"][jj] < TIE, (N, i, int(j), int(per["iters"][jj]), int(m["iters"][jj]), float(m["min_margin"][jj]))
                    ties.append((N, int(j)))
                else:
                    worst = max(worst, _dev9(per["U"][jj], m["U"][jj]), _dev9(per["X"][jj], m["X"][jj]), _dev9(per["cost"][jj], m["cost"][jj]))
            total += len(idx)
        # (d) both model pointers NULL: the shared launch
        t = [torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in args]
        ref = torch_api.ilqr_solve_dev(d0, *t)
        ws = torch_api.IlqrWorkspace(d0, Bn, dev)
        torch_api._call("crx_ilqr_solve_models_dev", ctypes.byref(d0), ctypes.c_int(Bn), None, torch_api._ptr(t[0]), None, None,
                        *[torch_api._ptr(x) for x in t[1:]], *[torch_api._ptr(getattr(ws, k)) for k in KEYS], torch_api._stream())
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(getattr(ws, k), getattr(ref, k)), (N, k)
        # the device entry with models against the host entry
        wm = torch_api.ilqr_solve_dev(d0, *t, models=(torch.as_tensor(A_b, device=dev), torch.as_tensor(B_b, device=dev)))
        torch.cuda.synchronize()
        for k in KEYS:
            assert np.array_equal(getattr(wm, k).cpu().numpy(), mixed[k]), (N, k)
    assert total == 4 * Bn
    assert len(ties) <= total // 200, ties
    print("test 8c: worst deviation from ilqr_model %.3g (bound 1e-9), %d near ties of %d" % (worst, len(ties), total))


def test_8e_races_on_the_default_model(gpu, AB):
    import scenarios
    from crx import montecarlo

    A, B = AB
    track = scenarios.make_track("l_shape", 1.0)
    Bn = 8
    rng = np.random.default_rng(3)
    s0, v, ey = rng.uniform(2.0, 8.0, Bn), rng.uniform(0.1, 0.5, Bn), rng.uniform(-0.3, 0.3, Bn)
    a = (track.point_and_tangent, track.lap_length, A, B, np.zeros((Bn, 6)), np.zeros((Bn, 6)), s0, v, ey, 20)
    r0 = montecarlo.ilqr_races(*a, vt=0.8)
    r1 = montecarlo.ilqr_races(*a, vt=0.8, models=(np.repeat(A[None], Bn, axis=0), np.repeat(B[None], Bn, axis=0)))
    for k in ("xcurv", "u", "status", "iters", "laps"):
        assert np.array_equal(r0[k], r1[k]), k
    assert np.isfinite(r1["xcurv"]).all() and (r1["iters"] > 0).all()
