"""What the overtake path planner costs on the device; prints ONE JSON line.

    python tools/path_plan_bench.py [--reps 20] [--rounds 5] [--scen 4096] [--N 10] [--races 4096] [--slice 256]

  plan/<S>:   the fused step crx_path_plan_dev (prep -> region QPs under the per-QP mask -> selection + target) on cfg3_raw(S, N) behind the
              scene kernel -- three cars per scenario, their offsets x 2.2 on a track of width 2.5 so that the middle regions are feasible.
              Device-event ms per launch in alternating windows of --reps launches with a second arm, `prep+solve` (crx_path_prep_dev +
              crx_path_solve_dev: every QP, no selection), --rounds windows per arm after a warm-up window each; per arm the window medians,
              their median and their spread (max - min) / median; `scen_per_s` from the fused median.
              `host_loop`: the only way to run this step without the new entry points -- per scenario the mirror's path_qp_inputs,
              crx.path_solve on its regions, arg-min and target in numpy -- timed with the HOST clock on the FIRST --slice scenarios only (it is
              a slice: the loop is linear in the scenario count), as ms per scenario and scenarios per second; `same_flags` = the loop and the
              fused step choose the same region on every scenario of the slice.
  game/<B>:   GameLaps step time, planner="path" beside planner="traj" (for information: another planner, another overtake branch), B
              races against two scripted cars, the same alternating windows; a window = --reps steps, host clock around a synchronised window.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for p in (ROOT, os.path.join(ROOT, "car-racing_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _stats(ms):
    out = {}
    for k, v in ms.items():
        med = float(np.median(v))
        out[k] = dict(ms=round(med, 4), windows=[round(x, 4) for x in v], spread=round((max(v) - min(v)) / med, 4))
    return out


def _host_step(i, x, veh, sc, opt, N, tw, L, qd):
    """One scenario on the host: planning/overtake_path_planner.get_local_path's arithmetic on plain arrays."""
    import crx
    from crx import hostprep
    from planning import overtake_path_planner as opp
    from planning import planner_helper as ph

    mk = lambda s: types.SimpleNamespace(xcurv=s, param=types.SimpleNamespace(length=0.4, width=0.2))   # noqa: E731
    nv = int(sc["n_veh"][i])
    order = [int(v) for v in sc["order"][i, :nv]]
    info = ph.get_agent_info({"ego": mk(x[i]), **{v: mk(veh[i, v]) for v in order}}, order, types.SimpleNamespace(lap_length=L))
    rows = np.array([[veh[i, v, 4], sc["obs_ey"][i, k].max(), sc["obs_ey"][i, k].min()] for k, v in enumerate(order)])
    cps = ph.bezier_control_points(nv, rows, info.max_delta_v, 0.5, tw, L, 0.2, opt, x[i])
    qp = opp.path_qp_inputs(x[i, 4], x[i, 5], rows, info, cps, ph.bezier_polylines(cps, N), opt[:, 4], opt[:, 5], N, tw, L, 4.5, 0.5, 0.4, 0.2)
    r = crx.path_solve(qd, *qp)
    costs = [float(c) for c in r["cost"]]
    flag = costs.index(min(costs))
    span = info.max_s + 4.5 * 0.4 + 0.5 * info.max_delta_v - x[i, 4]
    target = np.zeros((N + 1, 6))
    target[:, 4] = x[i, 4] + span * np.arange(N + 1) / N
    target[:, 5] = r["E"][flag]
    s_end = target[-1, 4]
    s_q = max(s_end - L, opt[0, 4]) if s_end >= L else max(s_end, opt[0, 4])
    vx_t = hostprep.interp_clipped(opt[:, 4], opt[:, 0], s_q)
    a = np.clip((vx_t - x[i, 0]) / (2 * (s_end - x[i, 4]) / (vx_t + x[i, 0])), -1.5, 1.5)
    target[0] = x[i]
    with np.errstate(invalid="ignore"):
        target[:N, 0] = (x[i, 0] ** 2 + 2 * a * (target[:N, 4] - x[i, 4])) ** 0.5
    return flag, target


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scen", type=int, default=4096)
    ap.add_argument("--N", type=int, default=10)
    ap.add_argument("--races", type=int, default=4096)
    ap.add_argument("--slice", type=int, default=256)
    a = ap.parse_args()
    import torch

    import crx
    from crx import abi, montecarlo, synth, torch_api

    crx.init(0)
    dev = torch.device("cuda", 0)
    t = lambda x, dt=None: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)   # noqa: E731
    timer = torch_api.Timer()
    out = {"workload": "path_plan", "reps": a.reps, "rounds": a.rounds, "N": a.N}

    def launch_ms(fn):
        w = []
        for _ in range(a.reps):
            timer.begin()
            fn()
            timer.end()
            w.append(timer.ms())
        return float(np.median(w))

    # ---- arm 1: the fused step
    S, N, tw = a.scen, a.N, 2.5
    w = synth.cfg3_raw(S, N=N, track_width=tw)
    V, L, opt = w["V"], float(w["lap_length"]), w["opt"]
    cars = w["cars"].copy()
    cars[:, :, 2] *= 2.2
    veh = np.zeros((S, V, 6))
    veh[:, :, 0], veh[:, :, 4], veh[:, :, 5] = cars[:, :, 1], np.where(cars[:, :, 0] > L, cars[:, :, 0] - L, cars[:, :, 0]), cars[:, :, 2]
    pred_s = cars[:, :, 0, None] + 0.1 * np.arange(N + 1)[None, None, :] * cars[:, :, 1, None]
    pred_ey = np.repeat(cars[:, :, 2, None], N + 1, axis=2)
    x = t(w["x"])
    sw = torch_api.planner_scene_dev(abi.scene_desc(N, V, V, L), x, t(np.full(S, V), np.int32), t(veh), t(pred_s), t(pred_ey))
    pd, qd = abi.pathprep_desc(N, V, V, opt.shape[0], tw, L), abi.path_desc(N, 0.98)
    ins = [x, x, sw.n_veh, sw.order, t(veh), sw.max_dv, sw.obs_ey, t(opt[:, 4]), t(opt[:, 5])]
    opt_vx = t(opt[:, 0])
    ws = {k: torch_api.PathPlanWorkspace(pd, S, dev) for k in ("fused", "prep+solve")}
    arms = {"fused": lambda: torch_api.path_plan_dev(pd, qd, *ins, opt_vx, ws=ws["fused"]),
            "prep+solve": lambda: torch_api.path_solve_dev(qd, torch_api.path_prep_dev(pd, *ins, ws=ws["prep+solve"]))}
    ms = {k: [] for k in arms}
    for rnd in range(a.rounds + 1):   # the first window of each arm is its warm-up
        for k, fn in arms.items():
            v = launch_ms(fn)
            if rnd:
                ms[k].append(v)
    torch.cuda.synchronize()
    r = _stats(ms)
    r["scen_per_s"] = round(S / (r["fused"]["ms"] * 1e-3))
    r["qps"] = S * (V + 1)
    r["converged"] = int((ws["fused"].status == 0).sum().item())
    r["same_E"] = bool(torch.equal(ws["fused"].E, ws["prep+solve"].E))
    n = min(a.slice, S)
    sc = {k: getattr(sw, k).cpu().numpy() for k in ("n_veh", "order", "obs_ey")}
    _host_step(0, w["x"], veh, sc, opt, N, tw, L, qd)   # (warm-up: imports, staging buffers)
    t0 = time.perf_counter()
    host = [_host_step(i, w["x"], veh, sc, opt, N, tw, L, qd) for i in range(n)]
    dt = time.perf_counter() - t0
    flags = ws["fused"].flag.cpu().numpy()
    r["host_loop"] = dict(slice=n, ms_per_scen=round(dt / n * 1e3, 4), scen_per_s=round(n / dt, 1),
                          same_flags=bool(all(host[i][0] == flags[i] for i in range(n))),
                          target_max_dev=float(max(np.nanmax(np.abs(host[i][1] - ws["fused"].target[i].cpu().numpy())) for i in range(n))))
    r["speedup_vs_host_loop"] = round(r["scen_per_s"] / r["host_loop"]["scen_per_s"], 1)
    out["plan/%d" % S] = r

    # ---- arm 2: GameLaps step time
    from utils import racing_env

    A, B = synth.load_AB()
    g = np.load(os.path.join(ROOT, "tests", "golden", "racing_game.npz"))
    track = racing_env.ClosedTrack(np.genfromtxt(os.path.join(ROOT, "data/track_layout/l_shape.csv"), delimiter=","), track_width=1.0)
    Bn, Nl = a.races, 12
    ss = np.ascontiguousarray(g["ss/ss0"].transpose(2, 0, 1)); us = np.ascontiguousarray(g["ss/u0"].transpose(2, 0, 1))
    qf = np.ascontiguousarray(g["ss/Qfun0"].T); time_ss = g["ss/time_ss"].astype(np.int32)
    x0 = np.tile(g["lmpc/x"][0], (Bn, 1)); xg0 = np.tile(g["lap1/xglob"][-1], (Bn, 1))
    s0, v, ey = synth.multi_tests_traffic(Bn, 2, seed=70)
    tl = lambda arr: np.tile(arr[None], (Bn,) + (1,) * arr.ndim)   # noqa: E731
    games = {k: montecarlo.GameLaps(track.point_and_tangent, track.lap_length, track.width, A, B, opt, tl(ss), tl(us), tl(qf), tl(time_ss),
                                    np.full(Bn, 2, dtype=np.int32), x0, xg0, tl(ss[0, 1:Nl + 2]), tl(us[0, 1:Nl + 1]), s0, v, ey, device=dev, planner=k)
             for k in ("traj", "path")}
    gms = {k: [] for k in games}
    share = {k: [] for k in games}
    for rnd in range(a.rounds + 1):
        for k, gm in games.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ot = torch.zeros((), dtype=torch.int64, device=dev)
            for _ in range(a.reps):
                gm.step()
                ot += gm.overtake.sum()          # (stays on the device: no sync inside the window)
            torch.cuda.synchronize()
            if rnd:
                gms[k].append((time.perf_counter() - t0) / a.reps * 1e3)
                share[k].append(float(ot.item()) / (a.reps * Bn))
    gr = _stats(gms)
    for k in games:
        gr[k]["overtake_share"] = round(float(np.mean(share[k])), 3)
        gr[k]["finite"] = bool(torch.isfinite(games[k].lm.xc).all().item())
    gr["ratio_path_over_traj"] = round(gr["path"]["ms"] / gr["traj"]["ms"], 4)
    out["game/%d" % Bn] = gr
    print(json.dumps(out))


if __name__ == "__main__":
    main()
