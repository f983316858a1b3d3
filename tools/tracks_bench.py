"""One track per car: what the per-lane table reads of crx_plant_tracks_kernel cost; prints ONE JSON line.

    python tools/tracks_bench.py [--B 4096,65536] [--races 4096] [--reps 20] [--windows 30] [--seed 1]

One parameterised GPU pass.  The track set is the four layouts of data/track_layout (7, 11, 11, 9 rows).
  plant_ms    the plant launch ALONE (noise, lap wrap) by device events at every batch of --B, five arms on the same inputs, inputs and draws,
              alternating windows of --reps launches in this one process, --windows windows per arm after one warm-up window each: ms per
              launch as the median of the window means, with the windows' min, max and spread (max - min) / median.
                shared        crx_plant_step_noise_dev on l_shape: the kernel every loop ran before (table reads are LDS broadcasts)
                equal         crx_plant_step_tracks_dev, every track_id 0: per-lane reads that all hit one row
                sorted        ids b * 4 // B: every wavefront but three on one track
                interleaved   ids b % 4: every wavefront holds all four tracks
                shared_long   the control: the `shared` kernel on m_shape alone (11 rows), what the longest scans of the mix cost without
                              any per-lane read
              and every other arm over `shared`.  Every car starts inside its own lap, at the same fraction of the lap in every arm, so the
              scans stop at all rows.
  races_ms    one MpccbfRaces step (prep, solver, plant) of --races races, `single` on l_shape against `tracks` on the four layouts (ids
              b % 4), the same ego states relative to the line and the same scripted cars: ms per step over --reps steps from a common
              snapshot, median of --windows windows, alternating.
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

NAMES = ("l_shape", "m_shape", "goggle", "ellipse")


def _layouts():
    from utils import racing_env

    return [racing_env.ClosedTrack(np.genfromtxt(os.path.join(ROOT, "data/track_layout/%s.csv" % n), delimiter=","), track_width=1.0) for n in NAMES]


def _summary(ms, base):
    out = {}
    for k, v in ms.items():
        med = float(np.median(v))
        out[k] = dict(ms=round(med, 5), min=round(min(v), 5), max=round(max(v), 5), spread=round((max(v) - min(v)) / med, 4))
    for k in ms:
        if k != base:
            out["%s_over_%s" % (k, base)] = round(out[k]["ms"] / out[base]["ms"], 4)
    return out


def _plant_ms(ts, Bn, reps, windows, seed):
    import torch

    from crx import abi, torch_api

    dev = torch.device("cuda", 0)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)   # noqa: E731
    rng = np.random.default_rng(seed)
    frac = rng.uniform(0.02, 0.95, Bn)                          # where in its lap a car is: the same fraction in every arm
    ids = dict(equal=np.zeros(Bn, dtype=np.int32), sorted=(np.arange(Bn) * ts.n_tracks // Bn).astype(np.int32),
               interleaved=(np.arange(Bn) % ts.n_tracks).astype(np.int32))
    d = abi.plant_desc(int(ts.n_seg[0]), float(ts.lap_length[0]))
    long_t = int(np.argmax(ts.n_seg))
    u = t(np.tile([0.05, 0.3], (Bn, 1)))
    z = torch.randn((Bn, 3), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))
    laps = torch.zeros(Bn, dtype=torch.int32, device=dev)

    def states(track_id):
        x = np.zeros((Bn, 6))
        x[:, 0] = 0.8
        x[:, 4] = frac * ts.lap_length[track_id]
        return t(x)

    one = lambda k: (abi.plant_desc(int(ts.n_seg[k]), float(ts.lap_length[k])), t(ts.table(k)))   # noqa: E731
    arms = {"shared": (one(0), states(ids["equal"]))}
    for k, v in ids.items():
        arms[k] = (torch_api.TrackSetDev(ts, v, dev), states(v))
    arms["shared_long"] = (one(long_t), states(np.full(Bn, long_t)))
    og, oc = torch.empty((Bn, 6), dtype=torch.float64, device=dev), torch.empty((Bn, 6), dtype=torch.float64, device=dev)

    def window(arm):
        sd, x = arm
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            if isinstance(sd, tuple):
                torch_api.plant_step_wrap_dev(sd[0], sd[1], x, x, u, 2, og, oc, laps, noise_z=z)
            else:
                torch_api.plant_step_tracks_wrap_dev(d, sd, x, x, u, 2, og, oc, laps, noise_z=z)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    for arm in arms.values():
        window(arm)
    ms = {k: [] for k in arms}
    for _ in range(windows):
        for k, arm in arms.items():
            ms[k].append(window(arm))
    return _summary(ms, "shared")


def _races_ms(ts, Bn, reps, windows, seed):
    import torch

    from crx import montecarlo, synth

    A, B = synth.load_AB()
    rng = np.random.default_rng(seed)
    ids = (np.arange(Bn) % ts.n_tracks).astype(np.int32)
    x0 = np.zeros((Bn, 6))
    x0[:, 0] = rng.uniform(0.6, 0.9, Bn)
    back = rng.uniform(0.5, 6.0, Bn)                            # metres before the line, the same in both arms
    x0[:, 5] = rng.uniform(-0.1, 0.1, Bn)
    gap, v, ey = np.tile([1.2, 3.0], (Bn, 1)), np.full((Bn, 2), 0.3), np.tile([0.2, -0.2], (Bn, 1))

    def build(tracks):
        x = x0.copy()
        x[:, 4] = (ts.lap_length[ids] if tracks else ts.lap_length[0]) - back
        kw = dict(tracks=ts, track_id=ids) if tracks else {}
        tab, lap = (None, None) if tracks else (ts.table(0), float(ts.lap_length[0]))
        return montecarlo.MpccbfRaces(tab, lap, 1.0, A, B, x, x, x[:, 4:5] + gap, v, ey, vt=0.8, N=10, **kw)

    arms = {"single": build(False), "tracks": build(True)}
    snaps = {}
    for k, r in arms.items():
        for _ in range(3):
            r.step()
        torch.cuda.synchronize()
        snaps[k] = montecarlo.Snapshot(r)

    def window(k):
        r = arms[k]
        snaps[k].restore()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            r.step()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    for k in arms:
        window(k)
    ms = {k: [] for k in arms}
    for _ in range(windows):
        for k in arms:
            ms[k].append(window(k))
    return _summary(ms, "single")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", default="4096,65536")
    ap.add_argument("--races", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=30)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    import crx
    from crx import abi

    crx.init(0)
    trs = _layouts()
    ts = abi.track_set([t.point_and_tangent for t in trs], [t.lap_length for t in trs])
    out = dict(tracks=list(NAMES), n_seg=[int(n) for n in ts.n_seg], reps=a.reps, windows=a.windows, seed=a.seed,
               plant_ms={str(Bn): _plant_ms(ts, Bn, a.reps, a.windows, a.seed) for Bn in (int(v) for v in a.B.split(","))})
    if a.races > 0:
        out["races_ms"] = dict(races=a.races, **_races_ms(ts, a.races, a.reps, max(a.windows // 3, 3), a.seed))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
