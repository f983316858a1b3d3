"""NumPy restatement of crx_mixed_prep and crx_mixed_commit_dev (include/crx.h, "Mixed fields"), written from their specification on top of
the models the project already has: field_model.predict / obstacles / clear (the roll-out, the window test and packing of the MPC-CBF cars,
`clear`), ilqr_model.lap_offset (quirk I5) and the PID law of seed_model.commit.  Nothing of the product is imported."""
import numpy as np

import field_model as fm
import ilqr_model
import seed_model

NONE, PID, LQR, MPC_LTI, MPCCBF, ILQR = range(6)
N_POLICY = 6
CRX_CONVERGED, CRX_SKIPPED = 0, 4


def state_finite(xcurv):
    """[...]: every component of the state is finite (what "a car whose state is non-finite" means)."""
    return np.isfinite(np.asarray(xcurv, dtype=float)).all(axis=-1)


def ilqr_slots(policy, finite, e, r, ilqr_obstacles):
    """The cars in the iLQR slots of ego e of race r, in order: none unless the ego is a finite ILQR car; else the finite other cars in car
    order (mode 1), or the last other car in car order alone, if it is finite (mode 0, quirk I1)."""
    C = policy.shape[1]
    if policy[r, e] != ILQR or not finite[r, e] or C < 2:
        return []
    oth = [o for o in range(C) if o != e]
    if not ilqr_obstacles:
        oth = oth[-1:]
    return [o for o in oth if finite[r, o]]


def prep(track, L, xcurv, policy, N, N_ilqr, ilqr_obstacles=0, dt=0.1, safety_time=2.0, degree=6, car_dims=None, l_sum=0.4, w_sum=0.2):
    """All of crx_mixed_prep for xcurv [R, C, 6], policy [R, C]: pred_s, pred_ey [R,C,NP+1]; obs_s, obs_ey [R,C,V,N+1], lap_off [R,C,V], n_obs,
    m_nlp [R,C], (obs_dims [R,C,V,2]); with N_ilqr > 0 il_obs_s, il_obs_ey [R,C,V,N_ilqr+1], il_lap_off [R,C,V], il_n_obs, m_ilqr [R,C]; clear
    [R,C] -- plus `edge`, `cond`, `gap` [R,C] of field_model.prep, what a draw is filtered by (gap: of every ego, whatever its policy)."""
    x, pol = np.asarray(xcurv, dtype=float), np.asarray(policy)
    R, C = pol.shape
    V, NP = C - 1, max(N, N_ilqr)
    ps, pe, edge, cond = fm.predict(track, L, x, NP + 1, dt)
    f = fm.obstacles(ps[..., :N + 1], pe[..., :N + 1], x, L, safety_time, car_dims, l_sum, w_sum)
    cbf = pol == MPCCBF
    out = dict(pred_s=ps, pred_ey=pe, edge=edge, cond=cond, gap=f["gap"], clear=fm.clear(x, L, degree, car_dims, l_sum, w_sum))
    out["obs_s"] = np.where(cbf[..., None, None], f["obs_s"], 0.0)
    out["obs_ey"] = np.where(cbf[..., None, None], f["obs_ey"], 0.0)
    out["lap_off"] = np.where(cbf[..., None], f["lap_off"], 0.0)
    out["n_obs"] = np.where(cbf, f["n_obs"], 0).astype(np.int32)
    out["m_nlp"] = (cbf | (pol == MPC_LTI)).astype(np.int32)
    if car_dims is not None:
        out["obs_dims"] = np.where(cbf[..., None, None], f["obs_dims"], 0.0)
    if N_ilqr > 0:
        NI1 = N_ilqr + 1
        fin = state_finite(x)
        il_s, il_e, il_off = np.zeros((R, C, V, NI1)), np.zeros((R, C, V, NI1)), np.zeros((R, C, V))
        il_n = np.zeros((R, C), dtype=np.int32)
        for r in range(R):
            for e in range(C):
                for v, o in enumerate(ilqr_slots(pol, fin, e, r, ilqr_obstacles)):
                    il_s[r, e, v], il_e[r, e, v] = ps[r, o, :NI1], pe[r, o, :NI1]
                    il_off[r, e, v] = ilqr_model.lap_offset(x[r, e, 4], ps[r, o, 0], L)
                    il_n[r, e] += 1
        out.update(il_obs_s=il_s, il_obs_ey=il_e, il_lap_off=il_off, il_n_obs=il_n, m_ilqr=(pol == ILQR).astype(np.int32))
    return out


def lqr_law(K, x, xt):
    """u = -K (x - xt) with the sum in the kernel's order: from 0.0, c = 0 .. 5, every product and every sum rounded on its own."""
    d = x - xt
    v = np.zeros(K.shape[:-1])
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(6):
            v = v + K[..., c] * d[..., None, c]
    return -v


def commit(policy, x, pid=None, lqr=None, nlp=None, ilqr=None):
    """crx_mixed_commit_dev: (u [B,2], ctrl_status [B] int32).  policy [B]; x [B,6]; the families as pairs or None: pid = (vt, eyt) [B] each,
    lqr = (K [B,2,6], xt [B,6]), nlp = (U [B,N,2], status [B]), ilqr = (U [B,Ni,2], status [B])."""
    pol = np.asarray(policy)
    Bn = pol.shape[0]
    u, st = np.zeros((Bn, 2)), np.full(Bn, CRX_SKIPPED, dtype=np.int32)
    if pid is not None:
        up = np.zeros((Bn, 2))
        with np.errstate(invalid="ignore", over="ignore"):
            seed_model.commit(np.zeros(Bn, dtype=np.int32), pid[0], pid[1], x, None, None, None, up)
        m = pol == PID
        u[m], st[m] = up[m], CRX_CONVERGED
    if lqr is not None:
        m = pol == LQR
        u[m], st[m] = lqr_law(lqr[0], x, lqr[1])[m], CRX_CONVERGED
    for fam, codes in ((nlp, (MPC_LTI, MPCCBF)), (ilqr, (ILQR,))):
        if fam is not None:
            m = np.isin(pol, codes)
            u[m], st[m] = fam[0][m, 0], fam[1][m]
    return u, st
