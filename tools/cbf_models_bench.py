"""What one LTI model per problem costs the MPC-CBF / tracking NLP launches: crx_cbf_solve_dev beside crx_cbf_solve_models_dev fed copies
of the shipped model -- the same problems, the same iterates bit for bit, so the ratio isolates the set-up that differs; prints ONE JSON line.

    python tools/cbf_models_bench.py [--reps 20] [--rounds 5] [--races 4096] [--race-steps 30] [--reach-batch 4096]

  cfg2/256, cfg4/16384:  device-event ms per launch, `shared` and `models` arms in alternating windows of --reps launches in this process
                         (--rounds windows each after a warm-up window); per arm the window medians, their median and their spread
                         (max - min) / median; `ratio` = models / shared of the medians; `same` = the outputs are the same bits
  races/<B>:             ms per control step of MpccbfRaces with and without models= (host clock around a window of --race-steps steps and a
                         device synchronise), alternating windows as above
  reach/<B>:             the crx_cbf_models_reach_dev launch alone (device events, median of --reps)
A models arm slower than the shared arm's own window-to-window spread is to be explained from tools/asm_census.py of the two instantiations.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for p in (ROOT, os.path.join(ROOT, "car-racing_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _arms_stats(ms):
    out = {}
    for k, v in ms.items():
        med = float(np.median(v))
        out[k] = dict(ms=round(med, 4), windows=[round(x, 4) for x in v], spread=round((max(v) - min(v)) / med, 4))
    out["ratio"] = round(out["models"]["ms"] / out["shared"]["ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--races", type=int, default=4096)
    ap.add_argument("--race-steps", type=int, default=30)
    ap.add_argument("--reach-batch", type=int, default=4096)
    a = ap.parse_args()
    import torch

    import crx
    from crx import abi, montecarlo, synth, torch_api
    from utils import racing_env

    crx.init(0)
    A0 = np.genfromtxt(os.path.join(ROOT, "data/sys/LTI/matrix_A.csv"), delimiter=",")
    B0 = np.genfromtxt(os.path.join(ROOT, "data/sys/LTI/matrix_B.csv"), delimiter=",")
    dev = torch.device("cuda", 0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    copies = lambda n: (t(np.repeat(A0[None], n, axis=0)), t(np.repeat(B0[None], n, axis=0)))   # noqa: E731
    timer = torch_api.Timer()
    out = {"workload": "cbf_models", "reps": a.reps, "rounds": a.rounds}

    def launch_ms(fn):
        w = []
        for _ in range(a.reps):
            timer.begin()
            fn()
            timer.end()
            w.append(timer.ms())
        return float(np.median(w))

    for name, p, kw in (("cfg2/256", synth.cfg2_mpccbf(256), {}),
                        ("cfg4/16384", synth.cfg4_tracking_cbf(16384), dict(Q=(10.0, 0, 0, 5.0, 0, 50.0), per_stage_target=True))):
        n = len(p["x0"])
        d = abi.cbf_desc(p["N"], p["obs_s"].shape[1], A0, B0, alpha=p["alpha"], margin=p["margin"], **kw)
        args = [t(p[k]) for k in ("x0", "xt", "obs_s", "obs_ey", "lap_off")] + [t(p["n_obs"].astype(np.int32))]
        m = torch_api.CbfModels(d, *copies(n))
        ws = {"shared": torch_api.CbfWorkspace(d, n, dev), "models": torch_api.CbfWorkspace(d, n, dev)}
        arms = {"shared": lambda: torch_api.cbf_solve_dev(d, *args, ws=ws["shared"]),
                "models": lambda: torch_api.cbf_solve_dev(d, *args, ws=ws["models"], models=m)}
        ms = {k: [] for k in arms}
        for rnd in range(a.rounds + 1):   # the first window of each arm is its warm-up
            for k, fn in arms.items():
                v = launch_ms(fn)
                if rnd:
                    ms[k].append(v)
        torch.cuda.synchronize()
        r = _arms_stats(ms)
        r["same"] = all(torch.equal(getattr(ws["shared"], k), getattr(ws["models"], k)) for k in ("X", "U", "sigma", "cost", "status", "kkt", "iters"))
        r["converged"] = int((ws["shared"].status == 0).sum().item())
        out[name] = r
    if a.races:
        n = a.races
        track = racing_env.ClosedTrack(np.genfromtxt(os.path.join(ROOT, "data/track_layout/l_shape.csv"), delimiter=","), track_width=1.0)
        rng = np.random.default_rng(5)
        z = np.zeros((n, 6))
        # ONE scripted car per race: the shape with a tuned models instantiation (<1,12,6,10>).  With two cars the shared arm runs the tuned
        # <2,12,6,10> and the models arm the general <2,12,6,0>: measured 1.279 against 1.575 ms per step, the general kernels' price
        cars = (rng.uniform(3.0, 17.0, (n, 1)), rng.uniform(0.1, 0.4, (n, 1)), rng.choice([-0.5, -0.3, -0.1, 0.1, 0.3, 0.5], (n, 1)))

        def races(models):
            return montecarlo.MpccbfRaces(track.point_and_tangent, track.lap_length, track.width, A0, B0, z, z, *cars, vt=0.8, N=10, device=dev,
                                          models=models)

        arms = {"shared": races(None), "models": races(copies(n))}
        ms = {k: [] for k in arms}
        for rnd in range(a.rounds + 1):
            for k, r in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.race_steps):
                    r.step()
                torch.cuda.synchronize()
                if rnd:
                    ms[k].append((time.perf_counter() - t0) / a.race_steps * 1e3)
        r = _arms_stats(ms)
        r["same"] = all(torch.equal(getattr(arms["shared"], k), getattr(arms["models"], k)) for k in ("xc", "u")) and bool(
            torch.equal(arms["shared"].ws.status, arms["models"].ws.status))
        r["steps"] = a.race_steps
        out["races/%d" % n] = r
    if a.reach_batch:
        n = a.reach_batch
        d = abi.cbf_desc(12, 1, A0, B0)
        mA, mB = copies(n)
        reach = torch.empty((n, 2, torch_api.CBF_REACH_ROW), dtype=torch.float64, device=dev)
        import ctypes as C

        fn = lambda: torch_api._call("crx_cbf_models_reach_dev", C.byref(d), C.c_int(n), torch_api._ptr(mA), torch_api._ptr(mB),   # noqa: E731
                                     torch_api._ptr(reach), torch_api._stream())
        fn()
        out["reach/%d" % n] = dict(ms=round(launch_ms(fn), 5))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
