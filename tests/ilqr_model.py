"""Batch-vectorised numpy model of the iLQR that crx_ilqr_solve implements (include/crx.h, quirks I1..I6), the checker of the
GPU tests where the reference does not exist.

Written from the algorithm's description: roll out from u = 0; stage derivatives of stages 0..N-1 with the exponential
repelling term; terminal value = stage N-1's derivatives; backward pass with Quu^-1 = V diag(1 / (max(l, 0) + lamb)) V';
full-step forward pass with feedback; accept iff the barrier-free cost decreased (lamb /= factor, stop when the relative decrease
is below eps), else lamb *= factor (stop when lamb > lamb_max); at most max_iter backward passes.

Every decision also yields the relative margin that decided it, so a test can tell a genuine mismatch from a near tie whose
outcome rounding may flip: accept |cost_new - cost| / |cost|, convergence |rel - eps| / eps, lambda |lamb - lamb_max| / lamb_max.
"""
import numpy as np

CONVERGED, MAX_ITER, STALLED = 0, 1, 5


def solve(A, B, Q, R, x0, xt, obs_s, obs_ey, lap_off, n_obs, N, max_iter=150, eps=0.01, lamb_init=1.0, lamb_factor=10.0,
          lamb_max=1000.0, margin=0.15, q1=2.5, q2=2.5, l_sum=0.4, w_sum=0.2, record=None):
    """x0, xt (Bn,6); obs_s, obs_ey (Bn,V,>=N+1); lap_off (Bn,V); n_obs (Bn,).  record: index of a problem whose iterates
    (U (N,2), X (N+1,6)) at every derivative evaluation are returned in out["iterates"]."""
    A, B, Q, R = (np.asarray(m, dtype=float) for m in (A, B, Q, R))
    x0 = np.atleast_2d(np.asarray(x0, dtype=float))
    xt = np.atleast_2d(np.asarray(xt, dtype=float))
    Bn = x0.shape[0]
    obs_s = np.asarray(obs_s, dtype=float).reshape(Bn, -1, np.shape(obs_s)[-1])[:, :, :N + 1]
    obs_ey = np.asarray(obs_ey, dtype=float).reshape(Bn, -1, np.shape(obs_ey)[-1])[:, :, :N + 1]
    lap_off = np.asarray(lap_off, dtype=float).reshape(Bn, -1)
    n_obs = np.asarray(n_obs).reshape(Bn)
    V = obs_s.shape[1]
    slot = np.arange(V)[None, :] < n_obs[:, None]                     # (Bn, V) obstacles that count
    p4, p5 = 1.0 / (l_sum * l_sum), 1.0 / (w_sum * w_sum)
    Q2, R2 = 2 * Q, 2 * R

    def rollout(x_first, x_ref, u_ref, k_ff, K_fb):
        """forward pass; with k_ff = None the plain rollout of u_ref"""
        X = np.zeros((Bn, N + 1, 6))
        U = np.zeros((Bn, N, 2))
        X[:, 0] = x_first
        for i in range(N):
            if k_ff is None:
                U[:, i] = u_ref[:, i]
            else:
                U[:, i] = (u_ref[:, i] + k_ff[:, i]) + np.einsum("bac,bc->ba", K_fb[:, i], X[:, i] - x_ref[:, i])
            X[:, i + 1] = X[:, i] @ A.T + U[:, i] @ B.T
        return X, U

    def cost_of(X, U):
        d = X - xt[:, None, :]
        ls = np.einsum("bki,ij,bkj->bk", d, Q, d)
        lu = np.einsum("bki,ij,bkj->bk", U, R, U)
        c = np.zeros(Bn)
        for k in range(N):
            c = (c + ls[:, k]) + lu[:, k]
        return c + ls[:, N]

    X, U = rollout(x0, None, np.zeros((Bn, N, 2)), None, None)
    cost = cost_of(X, U)
    lamb = np.full(Bn, float(lamb_init))
    live = np.ones(Bn, dtype=bool)
    status = np.full(Bn, MAX_ITER, dtype=np.int32)
    iters = np.zeros(Bn, dtype=np.int32)
    margins = np.full((Bn, max(max_iter, 1), 3), np.nan)              # per iteration: accept, convergence, lambda
    iterates = []
    for it in range(max_iter):
        if not live.any():
            break
        iters[live] += 1
        if record is not None and live[record]:
            iterates.append((U[record].copy(), X[record].copy()))
        # stage derivatives 0..N-1 (I2); barrier (I5) summed over the counted obstacles (I1)
        dX = X[:, :N] - xt[:, None, :]
        lx = np.einsum("ij,bkj->bki", Q2, dX)
        ds = (X[:, None, :N, 4] - obs_s[:, :, :N]) - lap_off[:, :, None]     # (Bn, V, N)
        de = X[:, None, :N, 5] - obs_ey[:, :, :N]
        h = (1.0 + margin) - ((ds * p4) * ds + (de * p5) * de)
        hd4, hd5 = (-2.0 * p4) * ds, (-2.0 * p5) * de
        e = np.exp(q2 * h) * slot[:, :, None]
        gb, hb = (q1 * q2) * e, (q1 * (q2 * q2)) * e
        lxx = np.broadcast_to(Q2, (Bn, N, 6, 6)).copy()
        for v in range(V):
            lx[:, :, 4] += gb[:, v] * hd4[:, v]
            lx[:, :, 5] += gb[:, v] * hd5[:, v]
            lxx[:, :, 4, 4] += hb[:, v] * (hd4[:, v] * hd4[:, v])
            lxx[:, :, 4, 5] += hb[:, v] * (hd4[:, v] * hd5[:, v])
            lxx[:, :, 5, 4] += hb[:, v] * (hd4[:, v] * hd5[:, v])
            lxx[:, :, 5, 5] += hb[:, v] * (hd5[:, v] * hd5[:, v])
        lu = np.einsum("ij,bkj->bki", R2, U)
        # backward pass (I4)
        Vx, Vxx = lx[:, N - 1].copy(), lxx[:, N - 1].copy()
        kf = np.zeros((Bn, N, 2))
        Kf = np.zeros((Bn, N, 2, 6))
        for i in range(N - 1, -1, -1):
            Qx = lx[:, i] + Vx @ A
            Qu = lu[:, i] + Vx @ B
            Qxx = lxx[:, i] + A.T @ Vxx @ A
            Quu = R2 + B.T @ Vxx @ B
            Qux = B.T @ Vxx @ A
            w, Vec = np.linalg.eig(Quu)
            w = np.maximum(w.real, 0.0) + lamb[:, None]
            Vec = Vec.real
            Qinv = np.einsum("bij,bj,bkj->bik", Vec, 1.0 / w, Vec)
            kf[:, i] = -np.einsum("bij,bj->bi", Qinv, Qu)
            Kf[:, i] = -Qinv @ Qux
            KtQ = np.swapaxes(Kf[:, i], 1, 2) @ Quu
            Vx = Qx - np.einsum("bij,bj->bi", KtQ, kf[:, i])
            Vxx = Qxx - KtQ @ Kf[:, i]
        Xn, Un = rollout(x0, X, U, kf, Kf)
        cost_new = cost_of(Xn, Un)
        acc = live & (cost_new < cost)
        rej = live & ~acc
        margins[live, it, 0] = np.abs(cost_new - cost)[live] / np.abs(cost[live])
        rel = np.abs((cost_new - cost) / cost)
        X[acc], U[acc] = Xn[acc], Un[acc]
        lamb[acc] = lamb[acc] / lamb_factor
        margins[acc, it, 1] = np.abs(rel[acc] - eps) / eps
        conv = acc & (rel < eps)
        cost[acc] = cost_new[acc]
        lamb[rej] = lamb[rej] * lamb_factor
        margins[rej, it, 2] = np.abs(lamb[rej] - lamb_max) / lamb_max
        stall = rej & (lamb > lamb_max)
        status[conv], status[stall] = CONVERGED, STALLED
        live &= ~(conv | stall)
    out = dict(X=X, U=U, cost=cost, status=status, iters=iters, margins=margins,
               min_margin=np.nanmin(np.where(np.isnan(margins), np.inf, margins).reshape(Bn, -1), axis=1))
    if record is not None:
        out["iterates"] = iterates
    return out


def lap_offset(s_ego, s_obs0, lap_length):
    """(int(s_ego / L) - int(s_obs,0 / L)) L with int() truncating toward zero (quirk I5)."""
    return (np.trunc(np.asarray(s_ego) / lap_length) - np.trunc(np.asarray(s_obs0) / lap_length)) * lap_length
