"""The per-car reference of the track-set tests (tests/test_plant_tracks_cpu.py, tests/test_gpu_plant_tracks.py): the reference for car b is
the oracle called at batch 1 on table track_id[b], with that track's n_seg and lap_length in the descriptor and -- with `params` given --
the descriptor's ten fields set to row b (plant_params_ref.oracle_cars).  tests/test_plant_tracks_cpu.py holds the oracle to the reference's
own get_curvature + vehicle_dynamics on all four layouts (tests/golden/plant_tracks.npz).  No GPU, no library: numpy, the oracle and the
host mirror."""
import os

import numpy as np

import conftest
import plant_params_ref as pref

NAMES = ("l_shape", "m_shape", "goggle", "ellipse")


def layouts(width=1.0):
    """The four layouts as the host mirror's ClosedTrack objects, in the order of NAMES."""
    from utils import racing_env

    return [racing_env.ClosedTrack(np.genfromtxt(os.path.join(conftest.ROOT, "data/track_layout/%s.csv" % n), delimiter=","), track_width=width)
            for n in NAMES]


def track_set(seg_stride=None):
    from crx import abi

    trs = layouts()
    return abi.track_set([t.point_and_tangent for t in trs], [t.lap_length for t in trs], seg_stride=seg_stride)


def oracle_tracks(orc, ts, track_id, xg, xc, u, P=None, z=None, timestep=0.1):
    """(xglob_next, xcurv_next) [B,6] of one control step, car b on track track_id[b] of the TrackSet ts (and on row P[b]): the oracle at
    batch 1, track by track.  No lap wrap: wrap() below."""
    from crx import abi

    Bn = xg.shape[0]
    og, oc = np.zeros((Bn, 6)), np.zeros((Bn, 6))
    for t in range(ts.n_tracks):
        idx = np.nonzero(np.asarray(track_id) == t)[0]
        if not len(idx):
            continue
        d = abi.plant_desc(int(ts.n_seg[t]), float(ts.lap_length[t]), timestep=timestep)
        rows = np.tile(pref.desc_row(d), (len(idx), 1)) if P is None else P[idx]
        g, c = pref.oracle_cars(orc, d, ts.table(t), xg[idx], xc[idx], u[idx], rows, None if z is None else z[idx])
        og[idx], oc[idx] = g, c
    return og, oc


def wrap(xc, car_lap):
    """ModelBase.update_memory (base.py:795-819) on the host with every car's own lap length [B].  Returns (xc, crossed)."""
    xc = xc.copy()
    crossed = xc[:, 4] > car_lap
    xc[crossed, 4] -= car_lap[crossed]
    return xc, crossed.astype(np.int32)


def interleaved(B, n_tracks=4):
    """track_id = b % n_tracks: every wavefront holds every track."""
    return (np.arange(B) % n_tracks).astype(np.int32)


def draw_states(rng, ts, track_id):
    """plant_params_ref.draw_states with every car's s drawn over 2.2 laps of its own track."""
    L = ts.lap_length[track_id]
    B = len(track_id)
    xc, xg, u = pref.draw_states(rng, B, 1.0)
    xc[:, 4] = rng.uniform(-1.0, 2.2 * L)
    return xc, xg, u


NOISY_SEED = 41


def noisy_case(ts, track_id, seed=NOISY_SEED):
    """Inputs of the noise / wrap / stride test: states as draw_states, but the cars b % 3 == 0 -- a third of every track's cars with
    track_id = b % 4 -- within one control step of THEIR OWN line (s = L_b - U(0, 1) * 0.1 vx: most of them cross) and the rest
    inside their lap; u inside a [B,12,2] array of which the plant reads row 0 (u_stride 24); z scaled by 1, 6 and 20 so that the three
    clips act."""
    rng = np.random.default_rng(seed)
    B = len(track_id)
    L = ts.lap_length[track_id]
    xc, xg, u = pref.draw_states(rng, B, 1.0)
    xc[:, 4] = rng.uniform(0.0, L - 1.0)
    near = np.arange(B) % 3 == 0
    xc[near, 4] = L[near] - rng.uniform(0.0, 1.0, int(near.sum())) * 0.1 * xc[near, 0]
    U = rng.normal(size=(B, 12, 2))
    U[:, 0, :] = u
    z = rng.normal(size=(B, 3)) * rng.choice([1.0, 6.0, 20.0], size=(B, 1))
    return xc, xg, U, z, near


def pid_oracle_loop(orc, ts, track_id, x0, z, vt, P=None, timestep=0.1):
    """PidLaps on a track set on the host: control.pid, the oracle's noisy plant on the car's own track, the per-track wrap.  x0 [B,6],
    z [T,B,3].  Returns (x_log [B,T,6], u_log [B,T,2]) as crx_pid_log_dev keeps them."""
    from control import control

    T, Bn = z.shape[0], x0.shape[0]
    L = ts.lap_length[track_id]
    xc, xg = x0.copy(), x0.copy()
    xl, ul = np.zeros((Bn, T, 6)), np.zeros((Bn, T, 2))
    for k in range(T):
        u = np.stack([control.pid(xc[b], np.array([vt, 0, 0, 0, 0, 0.0])) for b in range(Bn)])
        xg, xc = oracle_tracks(orc, ts, track_id, xg, xc, u, P, z[k], timestep=timestep)
        xc, _ = wrap(xc, L)
        xl[:, k], ul[:, k] = xc, u
    return xl, ul
