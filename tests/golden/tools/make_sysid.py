"""Record the reference's system identification experiment (car_racing/tests/system_identification_test.py: one car under
PIDTracking on the ellipse track, 500 s at dt = 0.1 s, then system_identification.get_udata / linear_regression) into
tests/golden/sysid.npz, plus a second, shorter run at another target speed.

Run in the build container only (the reference does not exist on the GPU box):

    python tests/golden/tools/make_sysid.py

The reference is imported through ref_harness.install() and is not modified; the experiment's CSV outputs are not written.
np.random is seeded before each run and np.random.randn is wrapped so that every draw the plant's process noise takes is kept in
call order (three per control step: vx, vy, wz).  Stored per run (prefix "long/" or "short/"): x = xcurv_log [T,6], u =
get_udata(ego) [T,2], z = the draws [T,3], A, B, err = linear_regression(x, u, lamb), and the scenario (track_spec, vt, x0,
steps, seed, lamb, dt).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.normpath(os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import ref_harness  # noqa: E402

M = ref_harness.install()
base, offboard, racing_env = M["base"], M["offboard"], M["racing_env"]
from system import system_identification  # noqa: E402  (the reference's)

TRACK_SPEC = np.array([[3, 0], [np.pi / 2 * 1.5, -1.5], [2, 0], [np.pi / 2 * 1.5, -1.5], [6, 0], [np.pi / 2 * 1.5, -1.5],
                       [2.0, 0], [np.pi / 2 * 1.5, -1.5]])
DRAWS = []
_randn = np.random.randn


def _recording_randn(*shape):
    v = _randn(*shape)
    DRAWS.append(np.array(v, dtype=float).reshape(-1))
    return v


np.random.randn = _recording_randn


def run(vt, sim_time, seed, lamb=1e-9, dt=0.1, x0=(0.3, 0, 0, 0, 0, 0)):
    track = racing_env.ClosedTrack(TRACK_SPEC, track_width=1.0)
    ego = offboard.DynamicBicycleModel(name="ego", param=base.CarParam(edgecolor="black"))
    ego.set_state_curvilinear(np.array(x0, dtype=float))
    ego.set_state_global(np.array(x0, dtype=float))
    ego.set_ctrl_policy(offboard.PIDTracking(vt=vt))
    ego.ctrl_policy.set_timestep(dt)
    ego.set_track(track)
    sim = offboard.CarRacingSim()
    sim.set_timestep(dt)
    sim.set_track(track)
    sim.add_vehicle(ego)
    ego.ctrl_policy.set_racing_sim(sim)
    del DRAWS[:]
    np.random.seed(seed)
    sim.sim(sim_time=sim_time)
    x = np.stack(sim.vehicles["ego"].xcurv_log, axis=0)
    u = system_identification.get_udata(sim.vehicles["ego"])
    A, B, err = system_identification.linear_regression(x, u, lamb)
    z = np.concatenate(DRAWS)
    assert z.shape[0] == 3 * x.shape[0], (z.shape, x.shape)
    print("vt %.2f: %d rows, %d laps, lap length %.4f, |A| %.3f" % (vt, x.shape[0], ego.laps, track.lap_length, np.abs(A).max()))
    return dict(x=x, u=u, z=z.reshape(-1, 3), A=A, B=B, err=err, vt=vt, steps=x.shape[0], seed=seed, lamb=lamb, dt=dt,
                x0=np.array(x0, dtype=float), laps=ego.laps, lap_length=track.lap_length)


if __name__ == "__main__":
    out = dict(track_spec=TRACK_SPEC)
    for name, r in (("long", run(0.5, 500.0, seed=2022)), ("short", run(0.8, 60.0, seed=7))):
        for k, v in r.items():
            out[name + "/" + k] = np.asarray(v)
    path = os.path.join(OUT, "sysid.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))
