"""Record the reference's curvature lookup and plant on ALL FOUR track layouts into tests/golden/plant_tracks.npz.

Run in the build container only (the reference does not exist on the GPU box):

    python tests/golden/tools/make_plant_tracks.py

The oracle's curvature lookup was pinned against the reference on l_shape alone; the plant's track-set entries
(crx_plant_step_tracks*) look every car's curvature up on its own track, so the recording covers every segment joint of every layout.
This tool loads system/vehicle_dynamics.py and utils/racing_env.py BY PATH (numpy only -- no solver wheel, no stand-in), as
make_plant_params.py does, and runs racing_env.get_curvature + vehicle_dynamics the way DynamicBicycleModel.forward_dynamics does
(base.py:909-928).  Stored, for layout t = 0 .. 3 (names: l_shape, m_shape, goggle, ellipse):

    names [4], lap_length [4]
    t{t}/table [n_seg,6]                the reference's point_and_tangent
    t{t}/joint/joint [J]                which joint each row crosses: joint j = the end of segment j (the last one is the finish line)
    t{t}/joint/params [J,10], xglob, xcurv, u, xglob_next, xcurv_next
                                        J = n_seg full control steps (100 sub-steps of 0.001 s), each starting 0.03 m before its joint at
                                        vx 0.75 .. 0.85, so the step carries the car across the joint (asserted); no lap wrap (s runs past
                                        the lap length on the last joint, as in the reference before update_memory).  Odd rows drive a
                                        non-default parameter set (0.7 .. 1.3 times the defaults, as make_plant_params.py draws them)
    t{t}/sub/seg [M]                    the segment each single sub-step starts in, M = 3 n_seg: three states inside every segment, at
                                        0.05, 0.5 and 0.95 of its length (a state EXACTLY on a joint matches two rows, and the reference's
                                        int(np.where(...)) then raises, racing_env.py:236-245: nothing to record there)
    t{t}/sub/params, xglob, xcurv, u, curv, xglob_next, xcurv_next      those single Euler steps of 0.001 s
"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.normpath(os.path.join(HERE, ".."))
ROOT = os.path.normpath(os.path.join(HERE, "..", "..", ".."))
REF_ROOT = os.environ.get("CRX_REFERENCE_ROOT", "/root/reference")
NAMES = ("l_shape", "m_shape", "goggle", "ellipse")


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF_ROOT, "car_racing", rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


vd = _load("ref_vehicle_dynamics", "system/vehicle_dynamics.py")
racing_env = _load("ref_racing_env", "utils/racing_env.py")

DEFAULTS = np.array([1.98, 0.125, 0.125, 0.024, 0.8 * 1.98 * 9.81 / 2.0, 1.25, 1.0, 0.8 * 1.98 * 9.81 / 2.0, 1.25, 1.0])   # base.py:686-697


class Params:
    def __init__(self, row):
        self.row = [float(v) for v in row]

    def get_params(self):
        return tuple(self.row)


def draw_params(rng, n):
    p = np.tile(DEFAULTS, (n, 1))
    p[1::2] *= rng.uniform(0.7, 1.3, (len(p[1::2]), 10))
    return p


def draw_states(rng, s):
    n = len(s)
    xc = np.stack([rng.uniform(0.75, 0.85, n), rng.normal(0, 0.02, n), rng.normal(0, 0.1, n), rng.uniform(-0.1, 0.1, n), np.asarray(s, dtype=float),
                   rng.uniform(-0.3, 0.3, n)], axis=1)
    xg = np.stack([xc[:, 0], xc[:, 1], xc[:, 2], rng.uniform(-3, 3, n), rng.uniform(-5, 5, n), rng.uniform(-5, 5, n)], axis=1)
    u = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.5, 0.5, n)], axis=1)
    return xg, xc, u


def control_step(track, par, xglob, xcurv, u, timestep=0.1):
    delta_t, i = 0.001, 0
    while (i + 1) * delta_t <= timestep:                                                  # base.py:909-928
        curv = track.get_curvature(xcurv[4])
        xglob, xcurv = vd.vehicle_dynamics(par, curv, xglob, xcurv, delta_t, u)
        i = i + 1
    return xglob, xcurv


def record(rng, t, name):
    spec = np.genfromtxt(os.path.join(ROOT, "data/track_layout/%s.csv" % name), delimiter=",")
    track = racing_env.ClosedTrack(spec, 1.0)
    tab = np.array(track.point_and_tangent, dtype=np.float64)
    n_seg = tab.shape[0]
    ends = tab[:, 3] + tab[:, 4]
    out = {"t%d/table" % t: tab}
    # one control step across every joint
    P = draw_params(rng, n_seg)
    xg, xc, u = draw_states(rng, ends - 0.03)
    res = [control_step(track, Params(P[j]), xg[j], xc[j], u[j]) for j in range(n_seg)]
    gn, cn = np.array([r[0] for r in res]), np.array([r[1] for r in res])
    assert (xc[:, 4] < ends).all() and (cn[:, 4] > ends + 0.02).all(), "a step did not cross its joint"
    out.update({"t%d/joint/joint" % t: np.arange(n_seg, dtype=np.int32), "t%d/joint/params" % t: P, "t%d/joint/xglob" % t: xg,
                "t%d/joint/xcurv" % t: xc, "t%d/joint/u" % t: u, "t%d/joint/xglob_next" % t: gn, "t%d/joint/xcurv_next" % t: cn})
    # single sub-steps: three states inside every segment
    seg = np.repeat(np.arange(n_seg), 3)
    s = tab[seg, 3] + tab[seg, 4] * np.tile([0.05, 0.5, 0.95], n_seg)
    P = draw_params(rng, len(s))
    xg, xc, u = draw_states(rng, s)
    curv = np.array([track.get_curvature(v) for v in s])
    res = [vd.vehicle_dynamics(Params(P[i]), curv[i], xg[i], xc[i], 0.001, u[i]) for i in range(len(s))]
    out.update({"t%d/sub/seg" % t: seg.astype(np.int32), "t%d/sub/params" % t: P, "t%d/sub/xglob" % t: xg, "t%d/sub/xcurv" % t: xc,
                "t%d/sub/u" % t: u, "t%d/sub/curv" % t: curv, "t%d/sub/xglob_next" % t: np.array([r[0] for r in res]),
                "t%d/sub/xcurv_next" % t: np.array([r[1] for r in res])})
    return out, float(track.lap_length)


if __name__ == "__main__":
    rng = np.random.default_rng(20251)
    out, laps = {}, []
    for t, name in enumerate(NAMES):
        o, L = record(rng, t, name)
        out.update(o)
        laps.append(L)
    out["names"] = np.array(NAMES)
    out["lap_length"] = np.array(laps)
    path = os.path.join(OUT, "plant_tracks.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))
