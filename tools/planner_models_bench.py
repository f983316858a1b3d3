"""What one LTI model per region QP costs the planner step: crx_planner_plan_dev beside crx_planner_plan_models_dev fed copies of the
shipped model -- the same QPs, the same iterates bit for bit, so the ratio isolates what differs: the per-problem global loads of the model
and of the reach table where the shared kernel reads kernel arguments; prints ONE JSON line.

    python tools/planner_models_bench.py [--reps 20] [--rounds 5] [--scen 4096] [--N 12]

  plan/<S>:   cfg3_planner(S, N) through planner_plan_dev (S * (V + 1) region QPs + the selection): device-event ms per launch, `shared` and
              `models` arms in alternating windows of --reps launches in this process (--rounds windows each after a warm-up window); per arm
              the window medians, their median and their spread (max - min) / median; `ratio` = models / shared of the medians; `same` = the
              outputs are the same bits
  reach/<B>:  the crx_planner_models_reach_dev launch alone at the same batch B = S * (V + 1) (device events, median of --reps)
A models arm slower than the shared arm's own window-to-window spread is to be explained.
"""
import argparse
import ctypes as C
import json
import os
import sys

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
    ap.add_argument("--scen", type=int, default=4096)
    ap.add_argument("--N", type=int, default=12)
    a = ap.parse_args()
    import torch

    import crx
    from crx import abi, synth, torch_api

    crx.init(0)
    A0, B0 = synth.load_AB()
    dev = torch.device("cuda", 0)
    t = lambda x, dt=None: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)   # noqa: E731
    timer = torch_api.Timer()
    out = {"workload": "planner_models", "reps": a.reps, "rounds": a.rounds, "N": a.N}

    def launch_ms(fn):
        w = []
        for _ in range(a.reps):
            timer.begin()
            fn()
            timer.end()
            w.append(timer.ms())
        return float(np.median(w))

    S = a.scen
    p = synth.cfg3_planner(S, N=a.N)
    V = p["V"]
    R = V + 1
    d, sd = abi.planner_desc(a.N, A0, B0), abi.select_desc(a.N, V, p["lap_length"])
    args = [t(p[k]) for k in ("x0", "bez_s", "bez_ey", "ey_lb", "ey_ub")] + [t(p["n_veh"], np.int32), t(p["obs_s"]), t(p["obs_ey"]),
                                                                           t(p["old_flag"], np.int32)]
    m = torch_api.PlannerModels(d, t(np.repeat(A0[None], S, axis=0)), t(np.repeat(B0[None], S, axis=0)), regions=R)
    ws = {k: (torch_api.PlannerWorkspace(d, S * R, dev), torch_api.SelectWorkspace(sd, S, dev)) for k in ("shared", "models")}
    arms = {"shared": lambda: torch_api.planner_plan_dev(d, sd, *args, *ws["shared"]),
            "models": lambda: torch_api.planner_plan_dev(d, sd, *args, *ws["models"], models=m)}
    ms = {k: [] for k in arms}
    for rnd in range(a.rounds + 1):   # the first window of each arm is its warm-up
        for k, fn in arms.items():
            v = launch_ms(fn)
            if rnd:
                ms[k].append(v)
    torch.cuda.synchronize()
    r = _arms_stats(ms)
    r["same"] = all(torch.equal(getattr(ws["shared"][0], k), getattr(ws["models"][0], k)) for k in ("X", "U", "cost", "status", "kkt", "iters")) and all(
        torch.equal(getattr(ws["shared"][1], k), getattr(ws["models"][1], k)) for k in ("flag", "sel_cost", "best_X"))
    r["converged"] = int((ws["shared"][0].status == 0).sum().item())
    r["qps"] = S * R
    out["plan/%d" % S] = r
    fn = lambda: torch_api._call("crx_planner_models_reach_dev", C.byref(d), C.c_int(S * R), torch_api._ptr(m.A), torch_api._ptr(m.B),   # noqa: E731
                                 torch_api._ptr(m.reach), torch_api._stream())
    fn()
    out["reach/%d" % (S * R)] = dict(ms=round(launch_ms(fn), 5))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
