"""Times of the batched LQR design (crx_lqr_design_dev), of the LQR closed loop (crx.montecarlo.LqrLaps) and of the iLQR races with
per-car models beside the shared model; prints ONE JSON line.

    python tools/lqr_bench.py [--batches 1,256,4096,16384] [--reps 50] [--cars 4096] [--lap-steps 200] [--race-steps 30] [--rounds 3]

  design/<B>:  device-event ms per design launch of B perturbed models (median and minimum of --reps), designs/s, p50 / p100 of
               iters, the status counts
  laps/<B>:    closed-loop control steps of B cars under LqrLaps (one lqr-step + one plant launch per step): ms per step by a host
               clock around the loop and a device synchronise, and the lqr-step launch alone by device events
  ilqr/<B>:    ms per control step of IlqrRaces with one model for all cars (`shared`) and with per-car copies of that model
               (`per_car`), measured in alternation (--rounds windows of --race-steps steps each, after a warm-up window) in this
               process; `ratio` = per_car / shared of the medians.  Copies of one model, so that both arms solve the same problems
               with the same iteration counts and the ratio isolates the model loads.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for p in (ROOT, os.path.join(ROOT, "car-racing_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,256,4096,16384")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--cars", type=int, default=4096)
    ap.add_argument("--lap-steps", type=int, default=200)
    ap.add_argument("--race-steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import torch

    import crx
    from crx import abi, montecarlo, torch_api
    from utils import racing_env

    from lqr_model import draw_models   # tests/: A0 (1 + s z), B0 (1 + s z), s dealt round-robin from `scales`

    crx.init(0)
    A0 = np.genfromtxt(os.path.join(ROOT, "data/sys/LTI/matrix_A.csv"), delimiter=",")
    B0 = np.genfromtxt(os.path.join(ROOT, "data/sys/LTI/matrix_B.csv"), delimiter=",")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    d = abi.lqr_desc()
    out = {"workload": "lqr", "max_iter": d.max_iter, "eps": d.eps}
    timer = torch_api.Timer()
    for Bn in [int(b) for b in a.batches.split(",")]:
        A, B = (torch.as_tensor(x, device=dev) for x in draw_models(rng, A0, B0, Bn)[:2])
        ws = torch_api.LqrWorkspace(Bn, dev)
        torch_api.lqr_design_dev(d, A, B, ws=ws)   # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            timer.begin()
            torch_api.lqr_design_dev(d, A, B, ws=ws)
            timer.end()
            ms.append(timer.ms())
        it, st = ws.iters.cpu().numpy(), ws.status.cpu().numpy()
        med = float(np.median(ms))
        out["design/%d" % Bn] = dict(ms=round(med, 4), ms_min=round(float(np.min(ms)), 4), designs_per_s=round(Bn / med * 1e3, 1),
                                     iters_p50=float(np.median(it)), iters_p100=int(it.max()),
                                     converged=int((st == abi.CRX_CONVERGED).sum()), max_iter=int((st == abi.CRX_MAX_ITER).sum()),
                                     singular=int((st == abi.CRX_SINGULAR).sum()))
    track = racing_env.ClosedTrack(np.genfromtxt(os.path.join(ROOT, "data/track_layout/l_shape.csv"), delimiter=","), track_width=1.0)
    Bn = a.cars
    zeros = np.zeros((Bn, 6))
    if a.lap_steps:
        mA, mB, _ = draw_models(rng, A0, B0, Bn, scales=(1e-3, 1e-2))
        r = montecarlo.LqrLaps(track.point_and_tangent, track.lap_length, zeros, zeros, mA, mB, vt=0.8, device=dev, noise_seed=1)
        for _ in range(10):
            r.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.lap_steps):
            r.step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ms = []
        for _ in range(a.reps):
            timer.begin()
            torch_api.lqr_step_dev(r.K, r.xc, r.xt, r.u)
            timer.end()
            ms.append(timer.ms())
        out["laps/%d" % Bn] = dict(steps=a.lap_steps, ms_per_step=round(dt / a.lap_steps * 1e3, 4),
                                   car_steps_per_s=round(Bn * a.lap_steps / dt, 1), lqr_step_kernel_ms=round(float(np.median(ms)), 4),
                                   finite=bool(torch.isfinite(r.xc).all().item()))
    if a.race_steps:
        cars = (rng.uniform(2, 8, Bn), rng.uniform(0.1, 0.5, Bn), rng.uniform(-0.3, 0.3, Bn))
        models = (np.repeat(A0[None], Bn, axis=0), np.repeat(B0[None], Bn, axis=0))

        def races(m):
            return montecarlo.IlqrRaces(track.point_and_tangent, track.lap_length, A0, B0, zeros, zeros, *cars, device=dev, models=m)

        arms = {"shared": races(None), "per_car": races(models)}
        ms = {k: [] for k in arms}
        for rnd in range(a.rounds + 1):   # the first window of each arm is its warm-up
            for k, r in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.race_steps):
                    r.step()
                torch.cuda.synchronize()
                if rnd:
                    ms[k].append((time.perf_counter() - t0) / a.race_steps * 1e3)
        same = bool(torch.equal(arms["shared"].xc, arms["per_car"].xc))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        out["ilqr/%d" % Bn] = dict(steps=a.race_steps, rounds=a.rounds, shared_ms_per_step=round(med["shared"], 4),
                                   per_car_ms_per_step=round(med["per_car"], 4), ratio=round(med["per_car"] / med["shared"], 4),
                                   shared_windows=[round(v, 4) for v in ms["shared"]], per_car_windows=[round(v, 4) for v in ms["per_car"]],
                                   same_states=same)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
