"""Record the reference's own zero-input prediction of a driven car into tests/golden/field_pred.npz.

Run in the build container only (the reference does not exist on the GPU box):

    python tests/golden/tools/make_field_pred.py

racing/offboard.py:51-94 (DynamicBicycleModel.get_estimation / get_trajectory_nsteps(n)) is what control.mpccbf asks a driven opponent for
on its realtime_flag == True branch (control.py:512-514).  This tool imports the reference's racing.offboard the way make_golden.py does
(ref_harness: the shim directory on sys.path), sets one DynamicBicycleModel on a track and a drawn state, and stores what
get_trajectory_nsteps(N + 1) returns.  Per group `<track>_N<N>` (l_shape and m_shape; 64 states at N = 12, 16 at N = 24):

    <group>/xcurv       [n, 6]         the drawn state: vx 0.3 .. 2.0, vy, wz, epsi, ey non-zero of both signs, s over the lap
    <group>/pred_s      [n, N+1]       row 4 of the returned xcurv_nsteps
    <group>/pred_ey     [n, N+1]       row 5
    <group>/pred_epsi   [n, N+1]       row 3; rows 0 .. 2 are the state's vx, vy, wz in every column (asserted here), so these three rows
                                       and xcurv are the full xcurv rows
    tracks                             the track names

Each group's first states are placed, not drawn, in s: a quarter of them so that the prediction crosses the finish line inside the horizon
(the wrap of offboard.py:90-91), a quarter so that it crosses the first straight / curve joint; the tool asserts at least 8 of each per
N = 12 group (2 per N = 24 group).  A state is redrawn when some visited s -- the state's own and every predicted one -- lies within 1e-9
of a segment end or of the lap length (the reference raises at a joint, racing_env.py:244); so is a state whose roll-out comes
near the singularity of the curvilinear frame (|1 - curv ey| < 0.4: see record()).  Both counts are printed (0 for a joint and 4, 1, 2, 1
for the singularity with the seed below, in group order).  Data only: inputs, outputs and names.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.normpath(os.path.join(HERE, ".."))
ROOT = os.path.normpath(os.path.join(HERE, "..", "..", ".."))
sys.path.insert(0, HERE)
import ref_harness  # noqa: E402

TRACKS = ("l_shape", "m_shape")
GROUPS = ((12, 64), (24, 16))   # (N, states per track)


def draw_state(rng, L, s=None):
    sign = lambda: rng.choice([-1.0, 1.0])   # noqa: E731
    return np.array([rng.uniform(0.3, 2.0), sign() * rng.uniform(0.02, 0.3), sign() * rng.uniform(0.05, 0.8), sign() * rng.uniform(0.02, 0.4),
                     rng.uniform(0.0, L) if s is None else s, sign() * rng.uniform(0.05, 0.6)])


def edge_distance(track, s):
    """Smallest distance of the s values (each inside one lap) to a segment end; the ends include 0 and the lap length."""
    ends = np.concatenate([track.point_and_tangent[:, 3], [track.lap_length]])
    return np.abs(np.asarray(s, dtype=float)[:, None] - ends[None, :]).min()


def segment_of(track, s):
    tab = track.point_and_tangent
    return int(np.nonzero((s >= tab[:, 3]) & (s <= tab[:, 3] + tab[:, 4]))[0][0])


def record(M, name, N, n, rng):
    base, offboard, racing_env = M["base"], M["offboard"], M["racing_env"]
    track = racing_env.ClosedTrack(np.genfromtxt(os.path.join(ROOT, "data/track_layout/%s.csv" % name), delimiter=","), 0.8)
    L, tab = track.lap_length, track.point_and_tangent
    joint = next(tab[i + 1, 3] for i in range(len(tab) - 1) if tab[i, 5] != tab[i + 1, 5])   # the first straight / curve joint
    car = offboard.DynamicBicycleModel(name="car", param=base.CarParam(), system_param=base.SystemParam())
    car.set_track(track)
    car.set_timestep(0.1)
    xs, preds, redrawn, off_track, line, curve = [], [], 0, 0, 0, 0
    while len(xs) < n:
        k = len(xs)
        # placed: a car one to N/2 steps in front of the line / of the joint at its own speed; the rest drawn over the lap
        x = draw_state(rng, L)
        if k < n // 2:
            x[4] = (L if k < n // 4 else joint) - x[0] * 0.1 * rng.uniform(1.0, N / 2)
        car.set_state_curvilinear(x.copy())
        car.set_state_global(np.zeros(6))
        xc, _ = car.get_trajectory_nsteps(N + 1)
        visited = np.concatenate([[x[4]], xc[4]])
        visited = np.where(visited < 0, visited + L, visited)          # (a car sliding backwards across the line: the lookup's `while s < 0`)
        # |1 - curv ey| along the roll-out: the curvilinear frame is singular at ey = 1 / curv, and a roll-out that comes near it amplifies every
        # rounding error by 1 / (1 - curv ey)^2 -- no two float64 implementations agree to 1e-12 there.  A car on a track of half-width 0.8 stays
        # above 1 - 0.7 * 0.8 = 0.44 on these layouts; a drawn state whose zero-input roll-out drops below 0.4 is redrawn as well
        cond = min(abs(1 - track.get_curvature(s) * ey) for s, ey in zip(visited, np.concatenate([[x[5]], xc[5]])))
        if edge_distance(track, visited) < 1e-9 or cond < 0.4:
            redrawn += edge_distance(track, visited) < 1e-9
            off_track += cond < 0.4
            continue
        line += int((np.diff(visited) < 0).any())
        segs = [segment_of(track, s) for s in visited]
        curve += int(any(tab[a, 5] != tab[b, 5] for a, b in zip(segs[:-1], segs[1:])))
        xs.append(x)
        preds.append(np.array(xc))
    assert line >= n // 8 and curve >= n // 8, (name, N, line, curve)
    print("%s N=%d: %d states, %d cross the finish line, %d a straight/curve joint, %d redrawn for a joint, %d for the frame's singularity" % (
        name, N, n, line, curve, redrawn, off_track))
    g = "%s_N%d" % (name, N)
    P = np.array(preds)
    X = np.array(xs)
    assert np.array_equal(P[:, 0:3], np.repeat(X[:, 0:3, None], N + 1, axis=2))
    return {g + "/xcurv": X, g + "/pred_s": P[:, 4], g + "/pred_ey": P[:, 5], g + "/pred_epsi": P[:, 3]}


if __name__ == "__main__":
    M = ref_harness.install()
    rng = np.random.default_rng(20261)
    out = {"tracks": np.array(TRACKS)}
    for N, n in GROUPS:
        for name in TRACKS:
            out.update(record(M, name, N, n, rng))
    path = os.path.join(OUT, "field_pred.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))
