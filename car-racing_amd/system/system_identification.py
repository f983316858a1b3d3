"""LTI system identification of the simulator's car (reference system/system_identification.py:4-43): a ridge regression of
x_{k+1} on (x_k, u_k) over one logged run.  Host numpy, like control.lqr: one regression of a few thousand rows is not a hot
path.  The batched device version (many logs, groups of logs) is crx.sysid_fit / crx.torch_api.sysid_fit_dev; include/crx.h
states the semantics both keep as S1..S5."""
import numpy as np


def linear_regression(x, u, lamb):
    """x [T,6] states, u [T,2] inputs, lamb ridge coefficient.  Returns A [6,6], B [6,2] and error [2,6] = column-wise max and
    min of the fit's residuals.
    S1: the pairs are (x_k, u_k) -> x_{k+1} for k = 1 .. T-2 (row 0 does not enter).  S2: s is regressed as logged, lap wraps
    included.  S3: W = inv(X'X + lamb I) (X'Y), the inverse formed explicitly, as the reference does."""
    T = x.shape[0]
    Y = x[2:T, :]
    X = np.hstack((x[1:T - 1, :], u[1:T - 1, :]))
    gram = np.dot(X.T, X) + lamb * np.eye(X.shape[1])
    W = np.dot(np.linalg.inv(gram), np.dot(X.T, Y))
    A = W.T[:, 0:6]
    B = W.T[:, 6:8]
    residual = np.dot(X, W) - Y
    error = np.vstack((np.max(residual, axis=0), np.min(residual, axis=0)))
    return A, B, error


def get_udata(ego):
    """The inputs of a finished run in step order (S5): each completed lap's `inputs`, then the running lap's `lap_inputs`, the
    number of rows of each taken from its recorded times; round(time / timestep) rows in all."""
    dt = ego.timestep
    u = np.zeros((round(ego.time / dt), 2))
    row = 0
    for lap in range(ego.laps):
        n = round((ego.times[lap][-1] - ego.times[lap][0]) / dt)
        for j in range(n):
            u[row, :] = ego.inputs[lap][j][:]
            row += 1
    n = round((ego.lap_times[-1] - ego.lap_times[0]) / dt)
    for j in range(n):
        u[row, :] = ego.lap_inputs[j][:]
        row += 1
    return u
