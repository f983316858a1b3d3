"""Seed laps on the device: every car's own PID lap and MPC-LTI lap into its own safe set; prints ONE JSON line.

    python tools/seed_bench.py [--B 4096] [--seed 1] [--split-steps 20] [--fleet 0.1,0.3] [--lmpc-steps 300]

One GPU pass on the track l_shape:
  seed       montecarlo.SeedLaps of B nominal cars from standstill on the shipped model, target speeds U(0.6, 0.8) per car so that the cars
             hand over at different steps, zero noise.  steps_to_last_handover = the largest time_ss[0] + time_ss[1]; steps_run = what run()
             took (it reads the count of driving cars every 32 steps); total_ms = the whole run() by device events, host reads included.
  split_ms   the five launches of a step (solve, commit, plant, log, addtraj), each between its own pair of events with a device synchronise
             after every step (so they do not add up to a free-running step: nothing overlaps here), mean over --split-steps steps: once from
             step 50 on (every car in its PID lap: the solver launch is masked out for all of them) and once from the step at which the
             median car is half-way through its MPC-LTI lap (in_mpc = share of the cars the solver launch is solving for).
  fleet      per spread of --fleet: synth.fleet_plant_params(B, spread, seed) drives the FIRST learning-MPC lap of every car (LmpcLaps,
             plant_params = the fleet, --lmpc-steps steps, zero noise) from
               own_identified   its own seeded safe set, the MPC-LTI lap on the model identified from its own PID laps (pid_laps, vt
                                U(0.5, 0.9), device noise, 600 steps -> identify(1e-9): the chain PidLaps -> identify -> SeedLaps -> LmpcLaps)
               own_shipped      its own seeded safe set, the MPC-LTI lap on the one shipped model
               nominal          the recorded safe set of the nominal car (tests/golden/racing_game.npz), tiled: what every loop did so far
             and reports per arm: cars seeded (phase 2) and seed_status counts; over the steps of each car's first lap the share of converged
             QPs and the count of singular stage regressions (prep_status != 0); lap time percentiles in steps over the cars that finished
             the lap; cars that finished; cars off the track and non-finite (crx.montecarlo.RaceStats).
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

NAMES = ("solve", "commit", "plant", "log", "addtraj")


def _track():
    from utils import racing_env

    spec = np.genfromtxt(os.path.join(ROOT, "data/track_layout/l_shape.csv"), delimiter=",")
    return racing_env.ClosedTrack(spec, track_width=1.0)


def _launches(r):
    """The five launches of SeedLaps.step(), one callable each."""
    from crx import torch_api

    prev = {}

    def plant():
        prev["c"], prev["g"] = r.xc, r.xg
        r._advance(r.u, 2)

    def traj():
        torch_api.lmpc_addtraj_dev(r.pdesc, r.crossed, r.log_x, r.log_u, r.n_log, r.ss, r.us, r.qf, r.time_ss, r.it, r.step_no, r.xc, r.traj_status)
        r.k += 1

    return (lambda: torch_api.cbf_solve_dev(r.desc, r.xc, r.xt, r.obs_s, r.obs_e, r.lap_off, r.n_obs, ws=r.ws, active=r.m_mpc, models=r.models),
            lambda: torch_api.seed_commit_dev(r.N, r.phase, r.vt, r.eyt, r.xc, r.ws.U, r.ws.status, r.seed_status, r.u), plant,
            lambda: torch_api.seed_log_dev(r.lap_length, prev["c"], prev["g"], r.xc, r.xg, r.u, r.laps, r.laps_prev, r.log_x, r.log_u, r.n_log,
                                           r.crossed, r.phase, r.seed_status, r.m_mpc), traj)


def _split(r, steps):
    import torch

    from crx import torch_api

    timers = [torch_api.Timer() for _ in NAMES]
    acc = np.zeros(len(NAMES))
    in_mpc = float((r.phase == 1).double().mean())
    for _ in range(steps):
        for t, launch in zip(timers, _launches(r)):
            t.begin()
            launch()
            t.end()
        torch.cuda.synchronize()
        acc += [t.ms() for t in timers]
    return dict(zip(NAMES, (round(float(v), 5) for v in acc / steps)), in_mpc=round(in_mpc, 4), from_step=r.k - steps)


def _first_lmpc_lap(lm, steps, ok=None):
    """`steps` control steps of a LmpcLaps under a RaceStats; the solver figures count the steps a car starts in its first lap.  ok [B] bool:
    the cars that count (a car that was not seeded has no safe set of its own; it is stepped and left out of every figure)."""
    import torch

    from crx import montecarlo

    if ok is None:
        ok = torch.ones(lm.batch, dtype=torch.bool, device=lm.device)
    stats = montecarlo.RaceStats(lm, group=ok.to(torch.int32), n_groups=2)
    stats.update()
    z = lambda: torch.zeros((), dtype=torch.int64, device=lm.device)   # noqa: E731
    n, conv, sing = z(), z(), z()
    for _ in range(steps):
        first = (lm.laps == 0) & ok
        stats.step()
        n += first.sum()
        conv += (first & (lm.ws.status == 0)).sum()
        sing += (first & (lm.pws.status != 0)).sum()
    rec, per = stats.summary()[1], stats.per_car()
    lap = per["lap_step"][0][ok.cpu().numpy()]
    done = lap[lap >= 0]
    pct = [int(v) for v in np.percentile(done, [5, 50, 95])] if len(done) else None
    return dict(qp_converged=round(float(conv) / max(int(n), 1), 5), prep_singular=int(sing), qps=int(n), finished=int(len(done)),
                lap_steps_p5_p50_p95=pct, off_track=rec["off"], non_finite=rec["nonfinite"], cars=rec["cars"])


def _seed_report(r):
    ph, st = r.phase.cpu().numpy(), r.seed_status.cpu().numpy()
    return dict(seeded=int((ph == 2).sum()), failed=int((ph == 3).sum()), still_driving=int((ph < 2).sum()),
                mpc_failed_flag=int(((st & 1) != 0).sum()), log_full_flag=int(((st & 2) != 0).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--split-steps", type=int, default=20)
    ap.add_argument("--fleet", default="0.1,0.3")
    ap.add_argument("--lmpc-steps", type=int, default=300)
    a = ap.parse_args()
    import torch

    import crx
    from crx import montecarlo, synth, torch_api

    crx.init(0)
    track = _track()
    tab, L, W = track.point_and_tangent, track.lap_length, track.width
    A, B = synth.load_AB()
    Bn = a.B
    rng = np.random.default_rng(a.seed)
    z = np.zeros((Bn, 6))
    vt = rng.uniform(0.6, 0.8, Bn)
    out = dict(B=Bn, seed=a.seed)
    # ---- the seed run, timed as a whole
    montecarlo.SeedLaps(tab, L, W, A, B, z, z, vt=vt).run(64)          # warm-up: the kernels are loaded
    torch.cuda.synchronize()
    r = montecarlo.SeedLaps(tab, L, W, A, B, z, z, vt=vt)
    timer = torch_api.Timer()
    timer.begin()
    r.run(1200)
    timer.end()
    torch.cuda.synchronize()
    t = r.time_ss[:, :2].cpu().numpy().astype(np.int64)
    total = t.sum(axis=1)
    out["seed"] = dict(_seed_report(r), steps_run=r.k, steps_to_last_handover=int(total.max()), steps_to_first_handover=int(total.min()),
                       total_ms=round(timer.ms(), 2), ms_per_step=round(timer.ms() / r.k, 5),
                       lap0_steps_min_max=[int(t[:, 0].min()), int(t[:, 0].max())], lap1_steps_min_max=[int(t[:, 1].min()), int(t[:, 1].max())])
    # ---- the per-launch split, in the PID phase and in the MPC-LTI phase
    r2 = montecarlo.SeedLaps(tab, L, W, A, B, z, z, vt=vt)
    for _ in range(50):
        r2.step()
    out["split_ms"] = dict(pid=_split(r2, a.split_steps))
    mid = int(np.median(t[:, 0] + t[:, 1] // 2))
    while r2.k < mid:
        r2.step()
    out["split_ms"]["mpc"] = _split(r2, a.split_steps)
    del r, r2
    # ---- a fleet: the first learning-MPC lap from the car's own safe set, and from the nominal car's
    g = np.load(os.path.join(ROOT, "tests", "golden", "racing_game.npz"))
    ss = np.ascontiguousarray(g["ss/ss0"].transpose(2, 0, 1)); us = np.ascontiguousarray(g["ss/u0"].transpose(2, 0, 1))
    qf, tss = np.ascontiguousarray(g["ss/Qfun0"].T), g["ss/time_ss"].astype(np.int32)
    tile = lambda v: torch.as_tensor(np.ascontiguousarray(v), device=torch.device("cuda", 0))[None].expand(Bn, *np.shape(v))   # noqa: E731
    nominal = dict(ss_xcurv=tile(ss), u_ss=tile(us), qfun=tile(qf), time_ss=tile(tss), it=torch.full((Bn,), 2, dtype=torch.int32, device="cuda"),
                   xcurv0=tile(g["lmpc/x"][0]), xglob0=tile(g["lap1/xglob"][-1]), lin_points=tile(ss[0, 1:14]), lin_input=tile(us[0, 1:13]))
    out["fleet"] = {}
    for spread in [float(s) for s in a.fleet.split(",") if s]:
        P = synth.fleet_plant_params(Bn, spread, a.seed)
        fit = montecarlo.pid_laps(tab, L, z, z, 600, vt=rng.uniform(0.5, 0.9, Bn), noise_seed=a.seed, plant_params=P).identify(1e-9)
        arms = {"failed_fits": int((fit.status != 0).sum())}
        for name, models in (("own_identified", (fit.A, fit.B)), ("own_shipped", None)):
            s = montecarlo.SeedLaps(tab, L, W, A, B, z, z, vt=0.7, models=models, plant_params=P).run(1200)
            ts = s.time_ss[:, :2].cpu().numpy()
            ok_dev = s.phase == 2
            ok = ok_dev.cpu().numpy()
            arms[name] = dict(seed=dict(_seed_report(s), lap0_steps_p50=int(np.median(ts[ok, 0])) if ok.any() else None,
                                        lap1_steps_p50=int(np.median(ts[ok, 1])) if ok.any() else None))
            arms[name].update(_first_lmpc_lap(montecarlo.LmpcLaps(tab, L, W, **s.lmpc_inputs(), plant_params=P), a.lmpc_steps, ok_dev))
            del s
        arms["nominal"] = _first_lmpc_lap(montecarlo.LmpcLaps(tab, L, W, **nominal, plant_params=P), a.lmpc_steps)
        out["fleet"]["%g" % spread] = arms
    print(json.dumps(out))


if __name__ == "__main__":
    main()
