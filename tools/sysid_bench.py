"""Throughput of crx_sysid_fit_dev (batched LTI system identification, include/crx.h S1..S5) on device-resident logs; prints
ONE JSON line.

    python tools/sysid_bench.py [--rows 5000] [--batch 4096] [--reps 20] [--chunks 8192] [--pid-steps 0]

  one/<rows>:          one log of --rows rows, one fit
  batch/<B>x<rows>:    B logs of --rows rows, one fit per log
  group/<B>x<rows>:    the same B logs pooled into one group, one fit
For each: device-event ms per call (median of --reps), fits/s, and the effective HBM rate 2 passes x rows x 64 B / time (the
Gram and the residual pass each stream every row's 48 B of x and 16 B of u once).  --chunks runs the cases at several
chunk_rows.  --pid-steps K > 0 also times K steps of crx.montecarlo.PidLaps over the batch (plant + PID log per step).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chunks", default="8192")
    ap.add_argument("--pid-steps", type=int, default=0)
    a = ap.parse_args()

    import torch

    import crx
    from crx import abi, torch_api

    crx.init(0)
    dev = torch.device("cuda", 0)
    T, Bn = a.rows, a.batch
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    x = torch.randn((Bn * T, 6), generator=gen, dtype=torch.float64, device=dev)
    u = torch.randn((Bn * T, 2), generator=gen, dtype=torch.float64, device=dev)
    off = torch.arange(Bn + 1, dtype=torch.int64, device=dev) * T
    one_grp = torch.tensor([0, Bn], dtype=torch.int32, device=dev)
    cases = [("one/%d" % T, x[:T], u[:T], off[:2], None, 1),
             ("batch/%dx%d" % (Bn, T), x, u, off, None, Bn),
             ("group/%dx%d" % (Bn, T), x, u, off, one_grp, Bn)]
    out = dict(tool="sysid_bench", rows=T, batch=Bn, reps=a.reps)
    for chunk in [int(c) for c in a.chunks.split(",")]:
        d = abi.sysid_desc(1e-9, chunk_rows=chunk)
        for name, xx, uu, oo, go, n_logs in cases:
            ws = torch_api.sysid_fit_dev(d, xx, uu, oo, go, max_log_rows=T)
            for _ in range(3):
                torch_api.sysid_fit_dev(d, xx, uu, oo, go, max_log_rows=T, ws=ws)
            ms = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                torch_api.sysid_fit_dev(d, xx, uu, oo, go, max_log_rows=T, ws=ws)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            assert (ws.status == 0).all().item()
            med = float(np.median(ms))
            n_fits = ws.status.shape[0]
            key = name if len(a.chunks.split(",")) == 1 else "%s/chunk%d" % (name, chunk)
            out[key] = dict(ms=round(med, 4), fits_per_s=round(n_fits / med * 1e3, 1),
                            gb_per_s=round(2 * n_logs * T * 64 / (med * 1e-3) / 1e9, 1))
    if a.pid_steps > 0:
        from crx import montecarlo
        from utils import racing_env

        spec = np.array([[3, 0], [np.pi / 2 * 1.5, -1.5], [2, 0], [np.pi / 2 * 1.5, -1.5], [6, 0], [np.pi / 2 * 1.5, -1.5],
                         [2.0, 0], [np.pi / 2 * 1.5, -1.5]])
        tr = racing_env.ClosedTrack(spec, track_width=1.0)
        x0 = np.tile([0.3, 0, 0, 0, 0, 0.0], (Bn, 1))
        r = montecarlo.PidLaps(tr.point_and_tangent, tr.lap_length, x0, x0, a.pid_steps, vt=np.linspace(0.4, 1.0, Bn), noise_seed=1)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r.run()
        e1.record()
        e1.synchronize()
        out["pid_laps/%dx%d" % (Bn, a.pid_steps)] = dict(ms=round(e0.elapsed_time(e1), 2),
                                                          ms_per_step=round(e0.elapsed_time(e1) / a.pid_steps, 4))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
