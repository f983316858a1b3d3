"""Record the reference's own iLQR / LQR answers (control.ilqr, control.lqr: plain numpy, no solver
wheel involved) into tests/golden/ilqr.npz, closed_loop_ilqr.npz and closed_loop_lqr.npz.

Run in the build container only (the reference does not exist on the GPU box):

    python tests/golden/tools/make_ilqr.py

The reference is imported through ref_harness.install() and is not modified.  Its iterations are
observed by swapping the module attribute control.ilqr_helper.get_cost_derivation for a counting
wrapper that also keeps each iterate (uvar, xvar) it is handed; "Convergence achieved" is read from
stdout.  From the iterate sequence the accept / reject decisions, hence lambda, are reconstructed:
an iterate whose inputs differ from its predecessor's was accepted.  That decides the stop kind of
a solve that neither converged nor ran short of max_iter.
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.normpath(os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import ref_harness  # noqa: E402

M = ref_harness.install()
import sympy as sp  # noqa: E402

base, offboard, racing_env, control = M["base"], M["offboard"], M["racing_env"], M["control"]
helper = control.ilqr_helper

CONVERGED, MAX_ITER, STALLED = 0, 1, 5  # crx_status codes
ITERATES = []
_orig = helper.get_cost_derivation


def _counting(ctrl_U, dX, Q, R, N, xvar, *rest):
    ITERATES.append((np.array(ctrl_U, dtype=float), np.array(xvar, dtype=float)))
    return _orig(ctrl_U, dX, Q, R, N, xvar, *rest)


helper.get_cost_derivation = _counting


class _Car:
    """Just what control.ilqr reads of a vehicle: param.length / width and the n-step prediction."""

    def __init__(self, length, width, traj=None):
        self.param = base.CarParam(length=length, width=width)
        self.traj = traj

    def get_trajectory_nsteps(self, time, timestep, n):
        assert self.traj.shape == (6, n)
        return self.traj, None


def _param(N, max_iter, vt):
    return base.iLQRRacingParam(vt=vt, num_horizon=N, max_iter=max_iter)


def stop_kind(iters, u_ret, converged, max_iter):
    """Reconstruct lambda from the recorded iterates (accept <=> the next iterate's inputs changed)."""
    if converged:
        return CONVERGED
    lamb = 1.0
    for j in range(iters):
        nxt = ITERATES[j + 1][0] if j + 1 < iters else None
        acc = (not np.array_equal(nxt, ITERATES[j][0])) if nxt is not None else (not np.array_equal(u_ret, ITERATES[j][0][:, 0]))
        lamb = lamb / 10 if acc else lamb * 10
    if iters < max_iter or lamb > 1000:
        return STALLED
    return MAX_ITER


def ilqr_call(x0, xt, N, max_iter, lap_length, ego_dims, car1_dims, obs, extra=None):
    """One control.ilqr call.  obs (6, N+1) is the prediction of the LAST non-ego vehicle (quirk I1); `extra`
    (length, width, traj) puts a car2 after car1 so that car1 supplies only the dimensions."""
    vehicles = {"ego": _Car(*ego_dims)}
    if extra is None:
        vehicles["car1"] = _Car(car1_dims[0], car1_dims[1], obs)
    else:
        vehicles["car1"] = _Car(car1_dims[0], car1_dims[1], extra)
        vehicles["car2"] = _Car(0.7, 0.35, obs)
    del ITERATES[:]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        u = control.ilqr(np.array(x0, float), np.array(xt, float), _param(N, max_iter, xt[0]), vehicles, "ego",
                         lap_length, 0.0, 0.1, None, None)
    conv = "Convergence achieved" in buf.getvalue()
    iters = len(ITERATES)
    return np.array(u, float), iters, stop_kind(iters, u, conv, max_iter)


def gen_single(n_cases=200, n_full=24, seed=7):
    rng = np.random.default_rng(seed)
    L = racing_env.ClosedTrack(np.genfromtxt("data/track_layout/l_shape.csv", delimiter=","), track_width=1.0).lap_length
    Nmax = 50
    rec = {k: [] for k in ("x0", "xt", "N", "max_iter", "lap_length", "obs_s", "obs_ey", "lap_off", "l_sum", "w_sum", "u0",
                           "iters", "stop", "kind", "two_cars")}
    full_U, full_X, full_case = [], [], []
    counts = {CONVERGED: 0, MAX_ITER: 0, STALLED: 0}
    tries = 0
    while len(rec["u0"]) < n_cases:
        tries += 1
        i = len(rec["u0"])
        N = int(rng.choice([10, 20, 50], p=[0.25, 0.25, 0.5]))
        vt = float(rng.choice([0.6, 0.8, 1.0]))
        eyt = 0.0 if rng.random() < 0.7 else float(rng.uniform(-0.2, 0.2))
        kind = int(rng.integers(0, 4))  # 0 ahead, 1 alongside, 2 behind, 3 across the lap line
        x0 = np.array([rng.uniform(0, 1.2), rng.uniform(-0.05, 0.05), rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2),
                       rng.uniform(0.0, 2 * L), rng.uniform(-0.4, 0.4)])
        ds0 = {0: rng.uniform(0.3, 3.0), 1: rng.uniform(-0.3, 0.3), 2: rng.uniform(-3.0, -0.3), 3: rng.uniform(-1.5, 1.5)}[kind]
        if kind == 3:
            x0[4] = float(rng.choice([L, 2 * L])) + rng.uniform(-1.0, 1.0)
            if rng.random() < 0.15:
                x0[4] = rng.uniform(0.0, 1.0)
        so = x0[4] + ds0
        vo = rng.uniform(0.0, 1.0)
        eyo = rng.uniform(-0.4, 0.4)
        k = np.arange(N + 1)
        obs = np.zeros((6, N + 1))
        obs[0], obs[4], obs[5] = vo, so + vo * 0.1 * k, eyo + rng.uniform(-0.02, 0.02) * k * (rng.random() < 0.3)
        ego_dims, car1_dims = (0.4, 0.2), (0.4, 0.2)
        if rng.random() < 0.25:
            ego_dims = (rng.uniform(0.3, 0.6), rng.uniform(0.15, 0.3))
            car1_dims = (rng.uniform(0.3, 0.6), rng.uniform(0.15, 0.3))
        two = rng.random() < 0.1
        extra = None
        if two:
            extra = np.zeros((6, N + 1))
            extra[4], extra[5] = x0[4] + 5.0, 0.3
        # the rarer stops: a few solves with a short iteration budget, and obstacle-overlap starts for the lambda blow-up
        want = min(counts, key=counts.get) if min(counts.values()) < 6 else None
        max_iter = 150
        if want == MAX_ITER:
            max_iter = int(rng.integers(1, 4))
        elif want == STALLED:
            obs[4] = x0[4] + rng.uniform(-0.1, 0.1) + vo * 0.1 * k
            obs[5] = x0[5] + rng.uniform(-0.05, 0.05)
        xt = np.array([vt, 0, 0, 0, 0, eyt], float)
        u0, iters, stop = ilqr_call(x0, xt, N, max_iter, L, ego_dims, car1_dims, obs, extra)
        if want is not None and stop != want and tries < 5000:
            continue
        if want is None and counts[stop] > 0.8 * n_cases:
            continue
        counts[stop] += 1
        cyc_e, cyc_o = int(x0[4] / L), int(obs[4, 0] / L)
        pad = lambda a: np.concatenate([a, np.full(Nmax + 1 - (N + 1), np.nan)])  # noqa: E731
        for key, val in (("x0", x0), ("xt", xt), ("N", N), ("max_iter", max_iter), ("lap_length", L), ("obs_s", pad(obs[4])),
                         ("obs_ey", pad(obs[5])), ("lap_off", (cyc_e - cyc_o) * L),
                         ("l_sum", ego_dims[0] / 2 + car1_dims[0] / 2), ("w_sum", ego_dims[1] / 2 + car1_dims[1] / 2),
                         ("u0", u0), ("iters", iters), ("stop", stop), ("kind", kind), ("two_cars", two)):
            rec[key].append(val)
        if len(set(c for c, _ in full_case)) < n_full and (i % 8 == 0 or stop != CONVERGED) and iters <= 40:
            for j, (U, X) in enumerate(ITERATES):
                full_U.append(np.pad(U.T, ((0, Nmax - N), (0, 0)), constant_values=np.nan))
                full_X.append(np.pad(X.T, ((0, Nmax - N), (0, 0)), constant_values=np.nan))
                full_case.append((i, j))
    out = {k: np.array(v) for k, v in rec.items()}
    out["full/case"] = np.array(full_case, dtype=np.int32)
    out["full/U"] = np.array(full_U)
    out["full/X"] = np.array(full_X)
    np.savez_compressed(os.path.join(OUT, "ilqr.npz"), **out)
    print("ilqr.npz: %d cases, stops %s, iterates %d of %d cases, %d bytes" % (
        len(out["u0"]), counts, len(full_case), len(set(c for c, _ in full_case)), os.path.getsize(os.path.join(OUT, "ilqr.npz"))))


def gen_closed_loop_ilqr(steps=500):
    """car_racing/tests/ilqr_test.py --track-layout l_shape --simulation (zero noise)."""
    track = racing_env.ClosedTrack(np.genfromtxt("data/track_layout/l_shape.csv", delimiter=","), track_width=1.0)
    ego = offboard.DynamicBicycleModel(name="ego", param=base.CarParam(edgecolor="black"), system_param=base.SystemParam())
    ego.set_zero_noise()
    ego.set_state_curvilinear(np.zeros((6,))); ego.set_state_global(np.zeros((6,))); ego.start_logging()
    ego.set_ctrl_policy(offboard.iLQRRacing(base.iLQRRacingParam(vt=0.8), ego.system_param))
    ego.ctrl_policy.set_timestep(0.1); ego.set_track(track); ego.ctrl_policy.set_track(track)
    t = sp.symbols("t")
    car1 = offboard.NoDynamicsModel(name="car1", param=base.CarParam(edgecolor="orange"))
    car1.set_track(track)
    car1.set_state_curvilinear_func(t, 0.2 * t + 4.0, 0.1 + 0.0 * t)
    car1.start_logging()
    sim = offboard.CarRacingSim(); sim.set_timestep(0.1); sim.set_track(track)
    sim.add_vehicle(ego); ego.ctrl_policy.set_racing_sim(sim); sim.add_vehicle(car1)
    iters, us = [], []
    orig = control.ilqr

    def rec(*a, **k):
        n0 = len(ITERATES)
        u = orig(*a, **k)
        iters.append(len(ITERATES) - n0)
        us.append(np.array(u, float))
        return u

    control.ilqr = rec
    del ITERATES[:]
    with contextlib.redirect_stdout(io.StringIO()):
        sim.sim(sim_time=steps * 0.1)
    control.ilqr = orig
    np.savez_compressed(os.path.join(OUT, "closed_loop_ilqr.npz"), steps=len(us), ego_xcurv=np.array(ego.xcurv_log),
                        ego_xglob=np.array(ego.xglob_log), ego_u=np.array(us), iters=np.array(iters, dtype=np.int32),
                        car1_xcurv=np.array(car1.xcurv_log), lap_length=track.lap_length)
    print("closed_loop_ilqr.npz: %d steps, iters %d..%d, final ego s %.3f" % (len(us), min(iters), max(iters), ego.xcurv[4]))


def gen_closed_loop_lqr(steps=900, n_calls=50, seed=11):
    """car_racing/tests/control_test.py --ctrl-policy lqr --track-layout l_shape --simulation (zero noise), and single
    control.lqr calls on drawn states and parameters."""
    track = racing_env.ClosedTrack(np.genfromtxt("data/track_layout/l_shape.csv", delimiter=","), track_width=0.8)
    ego = offboard.DynamicBicycleModel(name="ego", param=base.CarParam(edgecolor="black"), system_param=base.SystemParam())
    ego.set_zero_noise()
    ego.set_state_curvilinear(np.zeros((6,))); ego.set_state_global(np.zeros((6,))); ego.start_logging()
    ego.set_ctrl_policy(offboard.LQRTracking(base.LQRTrackingParam(vt=0.8), ego.system_param))
    ego.ctrl_policy.set_timestep(0.1); ego.ctrl_policy.set_track(track); ego.set_track(track)
    sim = offboard.CarRacingSim(); sim.set_timestep(0.1); sim.set_track(track)
    sim.add_vehicle(ego); ego.ctrl_policy.set_racing_sim(sim)
    with contextlib.redirect_stdout(io.StringIO()):
        sim.sim(sim_time=steps * 0.1)
    rng = np.random.default_rng(seed)
    xs, xts, qs, rs, its, us = [], [], [], [], [], []
    for i in range(n_calls):
        x = np.array([rng.uniform(0, 1.2), rng.uniform(-0.1, 0.1), rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3),
                      rng.uniform(0, 40), rng.uniform(-0.4, 0.4)])
        xt = np.array([rng.choice([0.6, 0.8, 1.0]), 0, 0, 0, 0, rng.uniform(-0.2, 0.2) if i % 3 else 0.0]).reshape(6, 1)
        Q = np.diag([10.0, 0.0, 0.0, 4.0, 0.0, 40.0]) if i % 2 == 0 else np.diag(rng.uniform(0, 50, 6))
        R = np.diag([0.1, 0.1]) if i % 2 == 0 else np.diag(rng.uniform(0.05, 1.0, 2))
        it = int(rng.choice([1, 2, 5, 50]))
        par = base.LQRTrackingParam(matrix_Q=Q, matrix_R=R, vt=float(xt[0, 0]), max_iter=it)
        with contextlib.redirect_stdout(io.StringIO()):
            u = control.lqr(x, xt, par)
        xs.append(x); xts.append(xt[:, 0]); qs.append(Q); rs.append(R); its.append(it); us.append(np.array(u, float))
    np.savez_compressed(os.path.join(OUT, "closed_loop_lqr.npz"), steps=steps, ego_xcurv=np.array(ego.xcurv_log),
                        ego_xglob=np.array(ego.xglob_log), calls_x=np.array(xs), calls_xt=np.array(xts),
                        calls_Q=np.array(qs), calls_R=np.array(rs), calls_max_iter=np.array(its), calls_u=np.array(us))
    print("closed_loop_lqr.npz: %d steps, final ego s %.3f; %d single calls" % (steps, ego.xcurv[4], n_calls))


if __name__ == "__main__":
    which = sys.argv[1:] or ["single", "ilqr_loop", "lqr"]
    if "single" in which:
        gen_single()
    if "lqr" in which:
        gen_closed_loop_lqr()
    if "ilqr_loop" in which:
        gen_closed_loop_ilqr()
