"""Field races: R races of C cars that all drive themselves under MPC-CBF; prints ONE JSON line.

    python tools/field_bench.py [--R 1024] [--C 4] [--steps 300] [--seed 1] [--windows 10] [--N 10]

One GPU pass on the track l_shape, two loops of the same solver batch B = R C, obstacle slots V = C - 1 and horizon N:
  field      montecarlo.FieldRaces: the cars of a race start 1.5 m apart on drawn lanes, every car with its own target speed U(0.5, 1.0),
             plant noise on (seed).
  scripted   montecarlo.MpccbfRaces as it stands: B independent egos from the same states, each with V scripted cars 1.5 m apart ahead
             of it at 0.2 .. 0.4 m/s -- the loop every release so far shipped, as the yardstick for the prep launch and the step.
Reported:
  outcome    of `field` over --steps control steps from the start: share of converged solves, laps, mean obstacle count per NLP, and from
             crx.montecarlo.RaceStats (sampled on the states the steps start from): cars with contact at some step (clear < 1), cars
             that left the track, cars with a non-finite state, overtakes made, the smallest clear.
  step_ms    per loop, the free-running step() by device events (crx_timer_*): --windows windows of --steps / --windows steps each,
             alternating between the loops after one warm-up window each; median of the window means, with min, max and spread
             (max - min) / median.
  split_ms   per loop, prep / solve / plant: each launch of a step between its own pair of events, a device synchronise after every
             step (so the three do not add up to step_ms: nothing overlaps here), mean over --steps / --windows steps.
Both loops keep running from where the outcome pass left them: the timed steps see cars that have met, not the start grid.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for p in (ROOT, os.path.join(ROOT, "car-racing_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _track():
    from utils import racing_env

    spec = np.genfromtxt(os.path.join(ROOT, "data/track_layout/l_shape.csv"), delimiter=",")
    return racing_env.ClosedTrack(spec, track_width=1.0)


def _launches(r):
    """(prep, solve, plant): the three launches of r.step(), one callable each, for a FieldRaces or an MpccbfRaces."""
    from crx import montecarlo, torch_api

    if isinstance(r, montecarlo.FieldRaces):
        f = r.fws
        return (lambda: torch_api.field_prep_dev(r.fdesc, r.tab, r.xc, f, car_dims=r.car_dims),
                lambda: torch_api.cbf_solve_dev(r.desc, r.xc, r.xt, f.obs_s, f.obs_ey, f.lap_off, f.n_obs, ws=r.ws, models=r.models, obs_dims=f.obs_dims),
                lambda: r._advance(r.ws.U, 2 * r.N))

    def plant():
        r._advance(r.ws.U, 2 * r.N)
        r.t += r.timestep

    return (lambda: torch_api.cbf_prep_dev(r.N, r.lap_length, r.t, r.timestep, r.xc, r.s0, r.v, r.ey, r.obs_s, r.obs_e, r.lap_off, r.n_obs),
            lambda: torch_api.cbf_solve_dev(r.desc, r.xc, r.xt, r.obs_s, r.obs_e, r.lap_off, r.n_obs, ws=r.ws, models=r.models), plant)


def _window(r, timer, steps):
    import torch

    timer.begin()
    for _ in range(steps):
        r.step()
    timer.end()
    torch.cuda.synchronize()
    return timer.ms() / steps


def _split(r, steps):
    import torch

    from crx import torch_api

    timers = [torch_api.Timer() for _ in range(3)]
    acc = np.zeros(3)
    for _ in range(steps):
        for t, launch in zip(timers, _launches(r)):
            t.begin()
            launch()
            t.end()
        torch.cuda.synchronize()
        acc += [t.ms() for t in timers]
    return dict(zip(("prep", "solve", "plant"), (round(float(v), 5) for v in acc / steps)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--R", type=int, default=1024)
    ap.add_argument("--C", type=int, default=4)
    ap.add_argument("--N", type=int, default=10)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--windows", type=int, default=10)
    a = ap.parse_args()
    import torch

    import crx
    from crx import montecarlo, synth, torch_api

    crx.init(0)
    track = _track()
    tab, L = track.point_and_tangent, track.lap_length
    A, B = synth.load_AB()
    R, C, V = a.R, a.C, a.C - 1
    rng = np.random.default_rng(a.seed)
    x0 = np.zeros((R, C, 6))
    x0[..., 0] = 0.3
    x0[..., 4] = (rng.uniform(0.0, L, (R, 1)) + 1.5 * np.arange(C)[None, :]) % L
    x0[..., 5] = rng.choice([-0.3, -0.1, 0.1, 0.3], (R, C))
    vt = rng.uniform(0.5, 1.0, (R, C))
    field = montecarlo.FieldRaces(tab, L, track.width, A, B, x0, x0, C, vt=vt, N=a.N, noise_seed=a.seed)
    # the outcome figures come from crx.montecarlo.RaceStats, one launch per step, sampled on the states each step STARTS from (the
    # states FieldRaces.min_clear covers)
    stats = montecarlo.RaceStats(field)
    conv = n_obs = 0
    for _ in range(a.steps):
        stats.update()
        field.step()
        conv += (field.ws.status == 0).sum()
        n_obs += field.fws.n_obs.sum()
    rec = stats.summary()
    out = dict(R=R, C=C, N=a.N, steps=a.steps, seed=a.seed,
               outcome=dict(converged=round(float(conv) / (a.steps * R * C), 5), contacts=rec["contact"], off_track=rec["off"],
                            non_finite=rec["nonfinite"], overtakes=rec["passes"], min_clear=rec["min_clear"], cars=R * C,
                            laps_min=int(field.laps.min()), laps_max=int(field.laps.max()), mean_n_obs=round(float(n_obs) / (a.steps * R * C), 4)))
    loops = dict(field=field)
    if V >= 1:
        flat = x0.reshape(R * C, 6)
        s0 = flat[:, 4:5] + 1.5 * (1 + np.arange(V))[None, :]
        loops["scripted"] = montecarlo.MpccbfRaces(tab, L, track.width, A, B, flat, flat, s0, rng.uniform(0.2, 0.4, (R * C, V)),
                                                   rng.choice([-0.3, -0.1, 0.1, 0.3], (R * C, V)), vt=0.8, N=a.N, noise_seed=a.seed)
        for _ in range(a.steps):
            loops["scripted"].step()
    timer, per = torch_api.Timer(), max(a.steps // a.windows, 1)
    ms = {k: [] for k in loops}
    for k, r in loops.items():
        _window(r, timer, per)
    for _ in range(a.windows):
        for k, r in loops.items():
            ms[k].append(_window(r, timer, per))
    out["step_ms"] = {k: dict(ms=round(float(np.median(v)), 5), min=round(min(v), 5), max=round(max(v), 5),
                              spread=round((max(v) - min(v)) / float(np.median(v)), 4)) for k, v in ms.items()}
    out["split_ms"] = {k: _split(r, per) for k, r in loops.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
