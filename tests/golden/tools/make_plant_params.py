"""Record the reference's plant on NON-default vehicle parameters into tests/golden/plant_params.npz.

Run in the build container only (the reference does not exist on the GPU box):

    python tests/golden/tools/make_plant_params.py

system/vehicle_dynamics.vehicle_dynamics(dynamics_param, ...) takes the parameter set as its first argument (:6); the reference's
simulator always hands it a fresh CarParam() (utils/base.py:906), so nothing of the reference ever runs it on another car.  This
tool does: it loads system/vehicle_dynamics.py and utils/racing_env.py BY PATH (numpy only -- no solver wheel, no stand-in) and
passes a small object with get_params().  Stored:

    step/params [40,10]      one set per step, every entry 0.7 .. 1.3 times its BicycleDynamicsParam default (base.py:686-697), with
                             lf != lr, Df != Dr, Cf != Cr, Bf != Br in every set (independent draws; asserted) -- so the
                             "lf on the rear axle" line (:26) shows
    step/xglob, xcurv, u, curv, xglob_next, xcurv_next      40 single Euler steps of 0.001 s, drawn as make_golden.gen_harness draws them
    pid/params [10]          one such set
    pid/xcurv_log, pid/xglob_log [30,6]     the PID closed loop on l_shape (vt = 0.8, track width 0.8, from rest), zero noise: the
                             sub-step loop of DynamicBicycleModel.forward_dynamics (base.py:897-928) around vehicle_dynamics with THAT set,
                             the PID law of control.pid (control/control.py:20-21; two lines, restated here because control.py imports
                             casadi), no lap crossing in 30 steps
"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.normpath(os.path.join(HERE, ".."))
ROOT = os.path.normpath(os.path.join(HERE, "..", "..", ".."))
REF_ROOT = os.environ.get("CRX_REFERENCE_ROOT", "/root/reference")


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


def draw(rng, n):
    p = DEFAULTS * rng.uniform(0.7, 1.3, (n, 10))
    for a, b in ((1, 2), (4, 7), (5, 8), (6, 9)):   # lf / lr, Df / Dr, Cf / Cr, Bf / Br
        assert (np.abs(p[:, a] - p[:, b]) > 1e-3 * DEFAULTS[a]).all()
    return p


def single_steps(rng):
    n = 40
    P = draw(rng, n)
    xg = rng.normal(size=(n, 6)); xc = rng.normal(size=(n, 6)) * 0.3
    xc[:, 0] = rng.uniform(0.3, 1.5, n); xg[:, 0:3] = xc[:, 0:3]
    u = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-1, 1, n)], axis=1)
    curv = rng.uniform(-0.7, 0.7, n)
    res = [vd.vehicle_dynamics(Params(P[i]), curv[i], xg[i], xc[i], 0.001, u[i]) for i in range(n)]
    return {"step/params": P, "step/xglob": xg, "step/xcurv": xc, "step/u": u, "step/curv": curv,
            "step/xglob_next": np.array([r[0] for r in res]), "step/xcurv_next": np.array([r[1] for r in res])}


def pid_loop(rng, steps=30, timestep=0.1, vt=0.8):
    spec = np.genfromtxt(os.path.join(ROOT, "data/track_layout/l_shape.csv"), delimiter=",")
    track = racing_env.ClosedTrack(spec, 0.8)
    par = Params(draw(rng, 1)[0])
    xglob, xcurv = np.zeros(6), np.zeros(6)
    logc, logg = [], []
    for _ in range(steps):
        u = np.array([-0.6 * (xcurv[5] - 0.0) - 0.9 * xcurv[3], 1.5 * (vt - xcurv[0])])   # control.py:20-21
        delta_t, i = 0.001, 0
        while (i + 1) * delta_t <= timestep:                                                  # base.py:909-928
            curv = track.get_curvature(xcurv[4])
            xglob, xcurv = vd.vehicle_dynamics(par, curv, xglob, xcurv, delta_t, u)
            i = i + 1
        assert xcurv[4] < track.lap_length
        logc.append(xcurv.copy()); logg.append(xglob.copy())
    return {"pid/params": np.array(par.row), "pid/xcurv_log": np.array(logc), "pid/xglob_log": np.array(logg)}


if __name__ == "__main__":
    rng = np.random.default_rng(20250)
    out = single_steps(rng)
    out.update(pid_loop(rng))
    path = os.path.join(OUT, "plant_params.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))
