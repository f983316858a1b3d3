"""A fleet of DIFFERENT cars, each controlled on the model identified from its own laps; prints ONE JSON line.

    python tools/fleet_bench.py [--B 4096] [--steps 600] [--spread 0.1] [--seed 1] [--reps 20] [--windows 50]

One parameterised GPU pass, on the track l_shape:
  fleet       P = synth.fleet_plant_params(B, spread, seed): every car's ten BicycleDynamicsParam values its default times 1 + spread U(-1, 1).
  identify    pid_laps(plant_params=P) for --steps control steps (vt U(0.5, 0.9) per car, device noise), then identify(1e-9): one (A, B) per
              car, from its own laps.  `fit_failed` = fits that are not CRX_CONVERGED.
  lqr         lqr_design + LqrLaps for --steps control steps at vt = 0.8, in two arms ON THE SAME FLEET and the same noise seed: `per_car` on the
              identified models, `shipped` on the one model of data/sys/LTI for every car.  Per arm, over the LAST HALF of the run and the
              cars that stayed finite and on the track: p50 / p95 over the cars of the RMS ey and of the RMS vx - vt; `off_track` = cars whose
              |ey| passed the track's half width at any step, `non_finite` = cars with a non-finite state at any step, `design_failed` =
              designs that are not CRX_CONVERGED / CRX_MAX_ITER.
  plant_ms    the plant launch ALONE (crx_plant_step_noise_dev: noise, lap wrap) by device events, `shared` (one parameter set, the kernel
              every loop ran before) against `per_car` (crx_plant_step_params_dev), alternating windows of --reps launches in this one
              process, --windows windows per arm after one warm-up window each: ms per launch as the median of the window means, with the
              windows' min, max and spread (max - min) / median.
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


def _lqr_arm(track, x0, A, B, P, steps, vt, noise_seed):
    from crx import abi, montecarlo

    r = montecarlo.LqrLaps(track.point_and_tangent, track.lap_length, x0, x0, A, B, vt=vt, noise_seed=noise_seed, plant_params=P)
    # two crx.montecarlo.RaceStats on the one loop, sampled after every step: `whole` over the run (off track, non-finite), `tail` reset
    # where the last half begins (the sums behind the RMS figures; LqrLaps' xt carries vt)
    half = steps // 2
    whole, tail = montecarlo.RaceStats(r, track_width=track.width, first_sample=1), None
    for k in range(steps):
        whole.step()
        if k == steps - half:
            tail = montecarlo.RaceStats(r, track_width=track.width)
        if tail is not None:
            tail.update()
    w, t = whole.per_car(), tail.per_car()
    finite = w["nonfinite_step"] < 0
    off = finite & (w["off_step"] >= 0)
    ok = finite & ~off
    rms_ey, rms_dv = np.sqrt(t["sum_ey2"] / half)[ok], np.sqrt(t["sum_dv2"] / half)[ok]
    st = r.design.status.cpu().numpy()
    pct = lambda v, q: round(float(np.percentile(v, q)), 5) if v.size else None   # noqa: E731
    return dict(rms_ey_p50=pct(rms_ey, 50), rms_ey_p95=pct(rms_ey, 95), rms_dv_p50=pct(rms_dv, 50), rms_dv_p95=pct(rms_dv, 95),
                off_track=int(off.sum()), non_finite=int((~finite).sum()), laps_p50=float(np.median(r.laps.cpu().numpy())),
                design_failed=int((~np.isin(st, (abi.CRX_CONVERGED, abi.CRX_MAX_ITER))).sum()))


def _plant_ms(track, x0, P, reps, windows):
    import torch

    from crx import abi, torch_api

    dev = torch.device("cuda", 0)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)   # noqa: E731
    Bn = x0.shape[0]
    tab, d = t(track.point_and_tangent), abi.plant_desc(track.point_and_tangent.shape[0], track.lap_length)
    xg, xc, Pd = t(x0), t(x0), t(P)
    u = t(np.tile([0.05, 0.3], (Bn, 1)))
    z = torch.randn((Bn, 3), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    og, oc = torch.empty_like(xg), torch.empty_like(xc)
    laps = torch.zeros(Bn, dtype=torch.int32, device=dev)
    arms = dict(shared=None, per_car=Pd)

    def window(params):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            torch_api.plant_step_wrap_dev(d, tab, xg, xc, u, 2, og, oc, laps, noise_z=z, params=params)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    for params in arms.values():
        window(params)
    ms = {k: [] for k in arms}
    for _ in range(windows):
        for k, params in arms.items():
            ms[k].append(window(params))
    out = {}
    for k, v in ms.items():
        med = float(np.median(v))
        out[k] = dict(ms=round(med, 5), min=round(min(v), 5), max=round(max(v), 5), spread=round((max(v) - min(v)) / med, 4))
    out["per_car_over_shared"] = round(out["per_car"]["ms"] / out["shared"]["ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--spread", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=50)
    a = ap.parse_args()
    import torch

    import crx
    from crx import abi, montecarlo, synth

    crx.init(0)
    track = _track()
    P = synth.fleet_plant_params(a.B, a.spread, a.seed)
    rng = np.random.default_rng(a.seed)
    x0 = np.zeros((a.B, 6))
    x0[:, 0] = 0.3
    pid = montecarlo.pid_laps(track.point_and_tangent, track.lap_length, x0, x0, a.steps, vt=rng.uniform(0.5, 0.9, a.B), noise_seed=a.seed,
                              plant_params=P)
    fit = pid.identify(1e-9)
    torch.cuda.synchronize()
    fit_failed = int((fit.status != abi.CRX_CONVERGED).sum().item())
    A0, B0 = synth.load_AB()
    x0[:, 0] = 0.8
    arms = dict(per_car=_lqr_arm(track, x0, fit.A, fit.B, P, a.steps, 0.8, a.seed + 1),
                shipped=_lqr_arm(track, x0, A0, B0, P, a.steps, 0.8, a.seed + 1))
    out = dict(B=a.B, steps=a.steps, spread=a.spread, seed=a.seed, fit_failed=fit_failed, lqr=arms,
               plant_ms=dict(reps=a.reps, windows=a.windows, **_plant_ms(track, x0, P, a.reps, a.windows)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
