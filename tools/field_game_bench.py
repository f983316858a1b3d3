"""Field games: R races of C cars that all play the racing game; prints ONE JSON line.

    python tools/field_game_bench.py [--R 256] [--C 4] [--steps 200] [--seed 1] [--windows 10] [--nominal] [--spread 0.1] [--planner traj]

One GPU pass on the track l_shape, one process per row (R, C, planner).  The safe sets of the B = R C cars:
  default    the chain PidLaps -> identify -> SeedLaps for a fleet (synth.fleet_plant_params(B, --spread, seed)): every car its own plant, its
             own identified model, its own two seed laps.  A car that did not seed (phase != 2) takes the nominal safe set; `unseeded` counts them.
  --nominal  the recorded safe set of the nominal car (tests/golden/racing_game.npz), tiled; the shipped model and plant for every car.
montecarlo.grid_start then puts car c of a race at the first step of its last safe-set lap that lies 1.5 c m beyond a step drawn per race.
Two loops of the same batch B, the same grid states and the same planner, as section 14 compares its two arms:
  field      montecarlo.FieldGames: the C cars of a race see each other (crx_field_traffic_dev).
  scripted   montecarlo.GameLaps as it stands: B independent cars from the same states, each with V = C - 1 scripted cars 1.5 m apart ahead
             of it at 0.2 .. 0.4 m/s (crx_game_traffic_dev) -- the yardstick for the traffic launch and the step.  (C = 1: the field arm only.)
Reported:
  outcome    of `field` over --steps control steps from the grid, plant noise on (seed): share of car-steps in the overtake branch, share of
             converged learning-MPC QPs / tracking NLPs among the car-steps that ran them, and crx.montecarlo.RaceStats' summary (contacts,
             overtakes made and suffered, cars off the track, non-finite, samples under the branch flag, laps).
  step_ms    per loop, the free-running step() by device events (crx_timer_*): --windows windows of --steps / --windows steps each,
             alternating between the loops after one warm-up window each; median of the window means, with min, max and spread.
  split_ms   per loop, every launch of a step between its own pair of events with the branches on one stream and a device synchronise
             after every step (so they do not add up to step_ms: nothing overlaps here), mean over --steps / --windows steps.
Both loops keep running from where the outcome pass left them.
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

GRID_FIELDS = ("step_no", "n_log", "log_x", "log_u", "u_old", "u_prev")


def _track():
    from utils import racing_env

    spec = np.genfromtxt(os.path.join(ROOT, "data/track_layout/l_shape.csv"), delimiter=",")
    return racing_env.ClosedTrack(spec, track_width=1.0)


def _nominal(Bn):
    import torch

    g = np.load(os.path.join(ROOT, "tests", "golden", "racing_game.npz"))
    ss = np.ascontiguousarray(g["ss/ss0"].transpose(2, 0, 1)); us = np.ascontiguousarray(g["ss/u0"].transpose(2, 0, 1))
    qf, tss = np.ascontiguousarray(g["ss/Qfun0"].T), g["ss/time_ss"].astype(np.int32)
    tile = lambda v: torch.as_tensor(np.ascontiguousarray(v), device=torch.device("cuda", 0))[None].expand(Bn, *np.shape(v)).contiguous()   # noqa: E731
    return dict(ss_xcurv=tile(ss), u_ss=tile(us), qfun=tile(qf), time_ss=tile(tss), it=torch.full((Bn,), 2, dtype=torch.int32, device="cuda"),
                xcurv0=tile(g["lmpc/x"][0]), xglob0=tile(g["lap1/xglob"][-1]), lin_points=tile(ss[0, 1:14]), lin_input=tile(us[0, 1:13]))


def _grid_k(inp, R, C, rng, gap=1.5, N=12):
    """k [R C]: per race a drawn step k0 of car 0's lap; car c at the first step of ITS last lap whose s lies gap * c beyond its own s at k0
    (the last admissible step if the lap ends before)."""
    import torch

    Bn = R * C
    ar = torch.arange(Bn, device=inp["ss_xcurv"].device)
    j = inp["it"].long() - 1
    s = inp["ss_xcurv"][ar, j][:, :, 4]                                         # [B, P]
    kmax = inp["time_ss"].long()[ar, j] - N - 1
    k0 = torch.as_tensor(np.repeat(rng.integers(0, 100, R), C), device=s.device)
    k0 = torch.minimum(k0, kmax)
    target = s[ar, k0] + gap * torch.as_tensor(np.tile(np.arange(C), R), dtype=torch.float64, device=s.device)
    row = torch.arange(s.shape[1], device=s.device)[None, :]
    ok = (s >= target[:, None]) & (row <= kmax[:, None]) & (row >= k0[:, None])
    return torch.where(ok.any(dim=1), ok.to(torch.int32).argmax(dim=1), kmax).cpu().numpy()


class _Timed:
    """Stands in for crx.torch_api inside crx.montecarlo: every `*_dev` wrapper runs between its own pair of device events."""

    def __init__(self, real):
        self.real, self.timers, self.order = real, {}, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not name.endswith("_dev"):
            return fn

        def timed(*a, **kw):
            if name not in self.timers:
                self.timers[name] = self.real.Timer()
                self.order.append(name)
            t = self.timers[name]
            t.begin()
            out = fn(*a, **kw)
            t.end()
            return out

        return timed


def _split(r, steps):
    import torch

    from crx import montecarlo, torch_api

    overlap, r.overlap = r.overlap, False
    proxy = _Timed(torch_api)
    montecarlo.torch_api = proxy
    acc = {}
    try:
        for _ in range(steps):
            r.step()
            torch.cuda.synchronize()
            for name in proxy.order:
                acc[name] = acc.get(name, 0.0) + proxy.timers[name].ms()
    finally:
        montecarlo.torch_api, r.overlap = torch_api, overlap
    return {name[:-4]: round(acc[name] / steps, 5) for name in proxy.order}


def _window(r, timer, steps):
    import torch

    timer.begin()
    for _ in range(steps):
        r.step()
    timer.end()
    torch.cuda.synchronize()
    return timer.ms() / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--R", type=int, default=256)
    ap.add_argument("--C", type=int, default=4)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--nominal", action="store_true")
    ap.add_argument("--spread", type=float, default=0.1)
    ap.add_argument("--planner", default="traj", choices=("traj", "path"))
    a = ap.parse_args()
    import torch

    import crx
    from crx import montecarlo, synth, torch_api

    crx.init(0)
    track = _track()
    tab, L, W = track.point_and_tangent, track.lap_length, track.width
    A, B = synth.load_AB()
    opt = np.genfromtxt(os.path.join(ROOT, "data/optimal_traj/xcurv_l_shape.csv"), delimiter=",")
    R, C, V = a.R, a.C, a.C - 1
    Bn = R * C
    rng = np.random.default_rng(a.seed)
    out = dict(R=R, C=C, steps=a.steps, seed=a.seed, planner=a.planner, safe_sets="nominal" if a.nominal else "fleet %g" % a.spread)
    models = P = None
    inp = _nominal(Bn)
    if not a.nominal:
        z = np.zeros((Bn, 6))
        P = synth.fleet_plant_params(Bn, a.spread, a.seed)
        fit = montecarlo.pid_laps(tab, L, z, z, 600, vt=rng.uniform(0.5, 0.9, Bn), noise_seed=a.seed, plant_params=P).identify(1e-9)
        models = (fit.A, fit.B)
        s = montecarlo.SeedLaps(tab, L, W, A, B, z, z, vt=0.7, models=models, plant_params=P).run(1200)
        ok = s.phase == 2
        own = s.lmpc_inputs()
        pick = lambda mine, nom: torch.where(ok.reshape((Bn,) + (1,) * (mine.dim() - 1)), mine, nom)   # noqa: E731
        inp = {name: pick(own[name].contiguous(), inp[name]) for name in inp}
        out["unseeded"], out["failed_fits"] = int((~ok).sum()), int((fit.status != 0).sum())
        del s
    k = _grid_k(inp, R, C, rng)
    grid = montecarlo.grid_start(inp, k, track)
    x0 = grid["xcurv0"].cpu().numpy().reshape(R, C, 6)
    gaps = np.diff(x0[..., 4], axis=1) % L if C > 1 else np.zeros((R, 0))
    out["grid"] = dict(k_min=int(k.min()), k_max=int(k.max()), gap_m_p5_p50_p95=[round(float(v), 3) for v in np.percentile(gaps, [5, 50, 95])] if C > 1 else None)
    field = montecarlo.FieldGames(tab, L, W, A, B, opt, C, **grid, models=models, plant_params=P, planner=a.planner, noise_seed=a.seed)
    stats = montecarlo.RaceStats(field)
    stats.update()
    zero = lambda: torch.zeros((), dtype=torch.int64, device=field.lm.device)   # noqa: E731
    n_ot, qp_ok, nlp_ok = zero(), zero(), zero()
    for _ in range(a.steps):
        stats.step()
        n_ot += field.m_ot.sum()
        qp_ok += ((field.lm.ws.status == 0) & (field.m_lm != 0)).sum()
        nlp_ok += ((field.tws.status == 0) & (field.m_ot != 0)).sum()
    rec = stats.summary()
    n_ot, total = int(n_ot), a.steps * Bn
    out["outcome"] = dict(overtake_share=round(n_ot / total, 5), qp_converged=round(int(qp_ok) / max(total - n_ot, 1), 5),
                          nlp_converged=round(int(nlp_ok) / max(n_ot, 1), 5) if n_ot else None, scene_overflow=int(field.overflow_seen.sum()),
                          laps_min=int(field.lm.laps.min()), laps_max=int(field.lm.laps.max()), race_stats=rec)
    loops = dict(field=field)
    if V >= 1:
        flat = grid["xcurv0"].cpu().numpy()
        s0 = flat[:, 4:5] + 1.5 * (1 + np.arange(V))[None, :]
        inputs = [grid[n] for n in ("ss_xcurv", "u_ss", "qfun", "time_ss", "it", "xcurv0", "xglob0", "lin_points", "lin_input")]
        scripted = montecarlo.GameLaps(tab, L, W, A, B, opt, *inputs, s0, rng.uniform(0.2, 0.4, (Bn, V)), rng.choice([-0.3, -0.1, 0.1, 0.3], (Bn, V)),
                                       models=models, plant_params=P, planner=a.planner, noise_seed=a.seed)
        for name in GRID_FIELDS:       # the same bookkeeping as the field's cars: k steps into the lap
            getattr(scripted.lm, name).copy_(grid[name].to(scripted.lm.device))
        for _ in range(a.steps):
            scripted.step()
        loops["scripted"] = scripted
    timer, per = torch_api.Timer(), max(a.steps // a.windows, 1)
    ms = {name: [] for name in loops}
    for name, r in loops.items():
        _window(r, timer, per)
    for _ in range(a.windows):
        for name, r in loops.items():
            ms[name].append(_window(r, timer, per))
    out["step_ms"] = {name: dict(ms=round(float(np.median(v)), 5), min=round(min(v), 5), max=round(max(v), 5),
                                 spread=round((max(v) - min(v)) / float(np.median(v)), 4)) for name, v in ms.items()}
    out["split_ms"] = {name: _split(r, per) for name, r in loops.items()}
    print(json.dumps(out, default=lambda o: o.item() if hasattr(o, "item") else o.tolist()))


if __name__ == "__main__":
    main()
