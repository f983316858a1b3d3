"""One track per race: what staging a whole track set and the per-lane table reads cost crx_field_prep_tracks_kernel
and one FieldRaces step; prints ONE JSON line.

    python tools/field_tracks_bench.py [--shapes 4096x3,585x7] [--races 1024x3] [--reps 20] [--windows 30] [--seed 1]

One parameterised GPU pass.  The track set is the four layouts of data/track_layout (7, 11, 11, 9 rows).  Five arms on the same cars -- every
race at the same fraction of ITS lap in every arm, its cars 0.9 m apart -- alternating windows of --reps launches in this one process, --windows
windows per arm after one warm-up window each: ms per launch as the median of the window means, with the windows' min, max and spread
(max - min) / median, and every other arm over `shared`.
    shared        crx_field_prep_dev on l_shape: the parent's entry (7 rows staged per block, table reads are LDS broadcasts)
    equal         crx_field_prep_tracks_dev, every race_track 0: 44 rows staged per block, per-lane reads that all hit one row
    sorted        ids r * 4 // R: every block but three on one track
    interleaved   ids r % 4: every block, and every wavefront, holds all four tracks
    shared_long   the control: the `shared` kernel on m_shape alone (11 rows), what the longest scans of the mix cost without a set
  prep_ms   the prep launch ALONE by device events at every R x C of --shapes, N = 10, with car_dims and clear
  step_ms   one FieldRaces step (prep, solver, plant) at --races, the same arms: --reps steps from a common snapshot, a third of the windows
`equal_over_shared` is the cost of the per-lane form against the parent's entry on the same cars; `interleaved_over_shared_long` what the mix
itself costs."""
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
ARMS = ("shared", "equal", "sorted", "interleaved", "shared_long")


def _layouts():
    from utils import racing_env

    return [racing_env.ClosedTrack(np.genfromtxt(os.path.join(ROOT, "data/track_layout/%s.csv" % n), delimiter=","), track_width=1.0) for n in NAMES]


def _summary(ms):
    out = {}
    for k, v in ms.items():
        med = float(np.median(v))
        out[k] = dict(ms=round(med, 5), min=round(min(v), 5), max=round(max(v), 5), spread=round((max(v) - min(v)) / med, 4))
    for k in ms:
        if k != "shared":
            out["%s_over_shared" % k] = round(out[k]["ms"] / out["shared"]["ms"], 4)
    out["interleaved_over_shared_long"] = round(out["interleaved"]["ms"] / out["shared_long"]["ms"], 4)
    return out


def _arm_ids(ts, R):
    """arm -> (race_track [R] of the set arms, or the one track of a shared arm)"""
    return dict(shared=0, equal=np.zeros(R, dtype=np.int32), sorted=(np.arange(R) * ts.n_tracks // R).astype(np.int32),
                interleaved=(np.arange(R) % ts.n_tracks).astype(np.int32), shared_long=int(np.argmax(ts.n_seg)))


def _states(ts, ids, frac, Cn, vx):
    R = len(frac)
    L = ts.lap_length[ids] if isinstance(ids, np.ndarray) else np.full(R, ts.lap_length[ids])
    x = np.zeros((R, Cn, 6))
    x[..., 0] = vx
    x[..., 4] = (frac * L)[:, None] + 0.9 * np.arange(Cn)[None, :]
    x[..., 5] = np.where(np.arange(Cn) % 2 == 0, 0.15, -0.15)[None, :]
    return x


def _windows(arms, window, windows):
    for k in arms:
        window(k)
    ms = {k: [] for k in arms}
    for _ in range(windows):
        for k in arms:
            ms[k].append(window(k))
    return _summary(ms)


def _prep_ms(ts, R, Cn, reps, windows, seed):
    import torch

    from crx import abi, torch_api

    dev = torch.device("cuda", 0)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)   # noqa: E731
    rng = np.random.default_rng(seed)
    frac = rng.uniform(0.02, 0.9, R)
    dims = t(np.stack([rng.uniform(0.3, 0.5, (R, Cn)), rng.uniform(0.15, 0.25, (R, Cn))], axis=-1))
    N = 10
    arms = {}
    for k, ids in _arm_ids(ts, R).items():
        x = t(_states(ts, ids, frac, Cn, 0.8).reshape(R * Cn, 6))
        if isinstance(ids, np.ndarray):
            desc = abi.field_desc(N, Cn, int(ts.n_seg[0]), float(ts.lap_length[0]))
            arms[k] = (desc, torch_api.RaceTrackSetDev(ts, ids, Cn, dev), x, torch_api.FieldWorkspace(desc, R, dev, dims=True))
        else:
            desc = abi.field_desc(N, Cn, int(ts.n_seg[ids]), float(ts.lap_length[ids]))
            arms[k] = (desc, t(ts.table(ids)), x, torch_api.FieldWorkspace(desc, R, dev, dims=True))

    def window(k):
        desc, tr, x, ws = arms[k]
        prep = torch_api.field_prep_dev if torch.is_tensor(tr) else torch_api.field_prep_tracks_dev
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            prep(desc, tr, x, ws, car_dims=dims)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    out = _windows(arms, window, windows)
    out["kept_per_ego"] = {k: round(float(arms[k][3].n_obs.double().mean()), 3) for k in arms}
    return out


def _step_ms(ts, R, Cn, reps, windows, seed):
    import torch

    from crx import montecarlo, synth

    A, B = synth.load_AB()
    rng = np.random.default_rng(seed)
    frac = rng.uniform(0.02, 0.9, R)
    vt = np.sort(rng.uniform(0.6, 1.0, (R, Cn)), axis=1)[:, ::-1].copy()
    arms, snaps = {}, {}
    for k, ids in _arm_ids(ts, R).items():
        x = _states(ts, ids, frac, Cn, 0.5)
        if isinstance(ids, np.ndarray):
            arms[k] = montecarlo.FieldRaces(None, None, 1.0, A, B, x, x, Cn, vt=vt, N=10, tracks=ts, race_track=ids)
        else:
            arms[k] = montecarlo.FieldRaces(ts.table(ids), float(ts.lap_length[ids]), 1.0, A, B, x, x, Cn, vt=vt, N=10)
        for _ in range(3):
            arms[k].step()
        torch.cuda.synchronize()
        snaps[k] = montecarlo.Snapshot(arms[k])

    def window(k):
        snaps[k].restore()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            arms[k].step()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    return _windows(arms, window, windows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x3,585x7")
    ap.add_argument("--races", default="1024x3")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=30)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    import crx
    from crx import abi

    crx.init(0)
    trs = _layouts()
    ts = abi.track_set([t.point_and_tangent for t in trs], [t.lap_length for t in trs])
    shape = lambda s: tuple(int(v) for v in s.split("x"))   # noqa: E731
    out = dict(tracks=list(NAMES), n_seg=[int(n) for n in ts.n_seg], reps=a.reps, windows=a.windows, seed=a.seed,
               prep_ms={s: _prep_ms(ts, *shape(s), a.reps, a.windows, a.seed) for s in a.shapes.split(",")})
    if a.races:
        out["step_ms"] = dict(shape=a.races, **_step_ms(ts, *shape(a.races), a.reps, max(a.windows // 3, 3), a.seed))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
