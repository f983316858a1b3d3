"""NumPy model of crx_seed_commit_dev and crx_seed_log_dev, written from rules S1-S6 of include/crx.h ("Seed laps"), one car at a time.
Every array is the caller's and is updated in place, as the device entries do; float64 operations are NumPy's, each rounded on its own, so
the kernels are held to these bits."""
import numpy as np

CRX_CONVERGED = 0
MPC_FAILED, LOG_FULL = 1, 2


def commit(phase, vt, eyt, x, U_mpc, mpc_status, seed_status, u):
    """After the solver launch, before the plant.  phase, mpc_status, seed_status [B] int32; vt, eyt [B]; x [B,6]; U_mpc [B,N,2]; u [B,2]."""
    for b in range(len(phase)):
        if phase[b] == 0:                                   # S1: control.pid
            u[b, 0] = np.float64(-0.6) * (x[b, 5] - eyt[b]) - np.float64(0.9) * x[b, 3]
            u[b, 1] = np.float64(1.5) * (vt[b] - x[b, 0])
        elif phase[b] == 1:                                 # S2: u_0 of the MPC-LTI plan; a failed solve is flagged
            u[b] = U_mpc[b, 0]
            if mpc_status[b] != CRX_CONVERGED:
                seed_status[b] |= MPC_FAILED
        else:                                               # S3
            u[b] = 0.0


def log(lap_length, xcurv_prev, xglob_prev, xcurv, xglob, u, laps, laps_prev, log_x, log_u, n_log, crossed, phase, seed_status, m_mpc):
    """After the plant, before add_trajectory.  States [B,6]; u [B,2]; log_x [B,P,6]; log_u [B,P,2]; the rest [B] int32."""
    P = log_x.shape[1]
    for b in range(len(phase)):
        if phase[b] >= 2:                                   # S4: frozen
            xcurv[b] = xcurv_prev[b]
            xglob[b] = xglob_prev[b]
            laps[b] = laps_prev[b]
            crossed[b] = 0
            continue
        cr = 1 if laps[b] > laps_prev[b] else 0             # S5: the assignments of crx_game_log_dev
        laps_prev[b] = laps[b]
        crossed[b] = cr
        n = int(n_log[b])
        row = xcurv[b].copy()
        row[4] = xcurv[b, 4] + np.float64(lap_length) * np.float64(cr)
        log_x[b, min(n, P - 1)] = row
        log_u[b, min(max(n - 1, 0), P - 1)] = u[b]
        n_log[b] = n + 1
        if cr:                                              # S6
            phase[b] += 1
        elif n_log[b] == P:
            phase[b] = 3
            seed_status[b] |= LOG_FULL
        m_mpc[b] = 1 if phase[b] == 1 else 0


class State:
    """The per-car arrays of a seed loop of B cars with P log rows, as crx.montecarlo.SeedLaps starts them."""

    def __init__(self, xcurv0, P):
        B = len(xcurv0)
        i32 = lambda v=0: np.full(B, v, dtype=np.int32)   # noqa: E731
        self.phase, self.seed_status, self.m_mpc = i32(), i32(), i32()
        self.laps, self.laps_prev, self.crossed, self.n_log = i32(), i32(), i32(), i32(1)
        self.log_x, self.log_u = np.zeros((B, P, 6)), np.zeros((B, P, 2))
        self.log_x[:, 0] = xcurv0
        self.u = np.zeros((B, 2))
