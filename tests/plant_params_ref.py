"""The per-car reference of the plant tests (tests/test_plant_params_cpu.py, tests/test_gpu_plant_params.py): the oracle takes the ten
BicycleDynamicsParam values from the descriptor, so the reference for car b is the oracle called at batch 1 with the descriptor's ten
fields set to row b of the parameter array.  tests/test_plant_params_cpu.py holds the oracle to the reference's own vehicle_dynamics on
non-default parameters (tests/golden/plant_params.npz).  No GPU, no library: numpy, the oracle and the host mirror."""
import ctypes as C
import os

import numpy as np

import conftest

NAMES = ("m", "lf", "lr", "Iz", "Df", "Cf", "Bf", "Dr", "Cr", "Br")   # BicycleDynamicsParam.get_params()


def track(width=1.0):
    from utils import racing_env

    spec = np.genfromtxt(os.path.join(conftest.ROOT, "data/track_layout/l_shape.csv"), delimiter=",")
    return racing_env.ClosedTrack(spec, track_width=width)


def desc_with(d, row):
    """A copy of plant descriptor d with its ten parameter fields set to `row`."""
    c = type(d).from_buffer_copy(d)
    for n, v in zip(NAMES, row):
        setattr(c, n, float(v))
    return c


def desc_row(d):
    return np.array([getattr(d, n) for n in NAMES])


def oracle_cars(orc, d, tab, xg, xc, u, P, z=None):
    """(xglob_next, xcurv_next) [B,6] of one control step, car b on row P[b]: B oracle calls at batch 1 (crx_oracle_plant_step_noise with
    z [B,3], the plain crx_oracle_plant_step without).  No lap wrap: wrap() below."""
    Bn = xg.shape[0]
    og, oc = np.zeros((Bn, 6)), np.zeros((Bn, 6))
    tab = np.ascontiguousarray(tab, dtype=np.float64)
    fn = orc.lib.crx_oracle_plant_step_noise
    fn.restype = C.c_int
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    for b in range(Bn):
        db = desc_with(d, P[b])
        if z is None:
            r = orc.plant_step(db, tab, xg[b:b + 1], xc[b:b + 1], u[b:b + 1])
            og[b], oc[b] = r["xglob"][0], r["xcurv"][0]
        else:
            a = [np.ascontiguousarray(v[b:b + 1], dtype=np.float64) for v in (xg, xc, u, z)]
            g1, c1 = np.zeros((1, 6)), np.zeros((1, 6))
            assert fn(C.byref(db), C.c_int(1), p(tab), *[p(v) for v in a], p(g1), p(c1)) == 0
            og[b], oc[b] = g1[0], c1[0]
    return og, oc


def wrap(xc, lap_length):
    """ModelBase.update_memory (base.py:795-819) on the host: s > lap_length -> s -= lap_length, one lap more.  Returns (xc, crossed)."""
    xc = xc.copy()
    crossed = xc[:, 4] > lap_length
    xc[crossed, 4] -= lap_length
    return xc, crossed.astype(np.int32)


def draw_states(rng, B, lap_length):
    """(xc, xg, u) as tests/test_gpu_parity.py test_plant_step draws them."""
    xc = np.stack([rng.uniform(0.3, 2.0, B), rng.normal(0, 0.05, B), rng.normal(0, 0.3, B), rng.uniform(-0.2, 0.2, B),
                   rng.uniform(-1.0, 2.2 * lap_length, B), rng.uniform(-0.8, 0.8, B)], axis=1)
    xg = np.stack([xc[:, 0], xc[:, 1], xc[:, 2], rng.uniform(-3, 3, B), rng.uniform(-5, 5, B), rng.uniform(-5, 5, B)], axis=1)
    u = np.stack([rng.uniform(-0.5, 0.5, B), rng.uniform(-1, 1, B)], axis=1)
    return xc, xg, u


NOISY_SEED = 21


def noisy_case(B, lap_length, seed=NOISY_SEED):
    """Inputs of the noise / wrap / stride test: states as draw_states, but a third of the cars within one control step of the lap
    length (s = L - U(0, 2) * 0.1 vx: about half of those cross) and the rest inside the lap; u inside a [B,12,2] array of which the
    plant reads row 0 (u_stride 24); z scaled by 1, 6 and 20 so that the three clips act."""
    rng = np.random.default_rng(seed)
    xc, xg, u = draw_states(rng, B, lap_length)
    xc[:, 4] = rng.uniform(0.0, lap_length - 1.0, B)
    near = np.arange(B) % 3 == 0
    xc[near, 4] = lap_length - rng.uniform(0.0, 2.0, int(near.sum())) * 0.1 * xc[near, 0]
    U = rng.normal(size=(B, 12, 2))
    U[:, 0, :] = u
    z = rng.normal(size=(B, 3)) * rng.choice([1.0, 6.0, 20.0], size=(B, 1))
    return xc, xg, U, z, near


# the four cars of the chain test: the default car and three others (m, lf, lr, Iz, Df, Cf, Bf, Dr, Cr, Br as multiples of the defaults)
CHAIN_FACTORS = np.array([
    [1.0] * 10,
    [1.3, 1.2, 0.8, 1.3, 0.75, 1.1, 0.9, 0.8, 0.9, 1.1],
    [0.7, 0.8, 1.2, 0.75, 1.25, 0.9, 1.2, 1.2, 1.1, 0.8],
    [1.15, 0.9, 1.3, 1.2, 0.8, 1.25, 0.8, 1.3, 0.8, 1.25],
])


def pid_oracle_loop(orc, tab, lap_length, x0, P, z, vt, timestep=0.1):
    """PidLaps on the host: control.pid, the oracle's noisy plant per car (oracle_cars), the lap wrap.  x0 [B,6], P [B,10], z [T,B,3].
    Returns (x_log [B,T,6], u_log [B,T,2]) as crx_pid_log_dev keeps them: x_log[:, k] the state after step k (s wrapped), u_log[:, k] the
    input applied in that step."""
    from control import control
    from crx import abi

    T, Bn = z.shape[0], x0.shape[0]
    d = abi.plant_desc(tab.shape[0], lap_length, timestep=timestep)
    xc, xg = x0.copy(), x0.copy()
    xl, ul = np.zeros((Bn, T, 6)), np.zeros((Bn, T, 2))
    for k in range(T):
        u = np.stack([control.pid(xc[b], np.array([vt, 0, 0, 0, 0, 0.0])) for b in range(Bn)])
        xg, xc = oracle_cars(orc, d, tab, xg, xc, u, P, z[k])
        xc, _ = wrap(xc, lap_length)
        xl[:, k], ul[:, k] = xc, u
    return xl, ul
