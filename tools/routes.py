"""Which kernel does a launch reach?  Batch 1 of every combination the units' selectors distinguish (csrc/crx_kernels_*.hip: Unit::select_inst),
for comparing two builds of the library (CRX_LIB=...) whose kernels are the same bits and whose launchers were rewritten.

    [CRX_LIB=..] rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/routes.py launch
    python tools/routes.py names DIR > A.txt      the library's kernel names of the trace in launch order, one per line: `diff` two of them
    [CRX_LIB=..] python tools/routes.py queries   crx_debug_resident_per_cu and crx_debug_lds_bytes over the same (N, slots) grid

The grid: planner region QP N = 3..24 with both qp_method; CBF NLP N = 3..24 with 0..6 obstacle slots, exponent 6 and 4; both again with one LTI
model per problem (copies of the shipped model); the two-wave route (N = 10, 12, one slot) under crx_debug_speculation(1).  A combination the
library refuses is printed as such (stdout belongs to the comparison as well).
"""
import csv
import glob
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "car-racing_amd")]
NS, SLOTS, DEGREES = range(3, 25), range(0, 7), (6, 4)


def launch():
    import numpy as np
    import crx
    from crx import abi, synth

    gpu = crx.init()
    A, B = synth.load_AB()
    L = crx.lib()

    def attempt(what, fn):
        try:
            st = fn()["status"]
            print("%-44s status %d" % (what, int(st[0])))
        except RuntimeError as e:
            print("%-44s refused: %s" % (what, str(e)[:100]))

    for models in (None, (A[None], B[None])):
        tag = "models " if models is not None else ""
        for N in NS:
            p = synth.cfg3_planner(1, N=N)
            for qm in (0, 1):
                d = abi.planner_desc(N, A, B)
                d.opts.qp_method = qm
                args = tuple(p[k][:1] for k in ("x0", "bez_s", "bez_ey", "ey_lb", "ey_ub"))
                attempt("%splanner N=%d qp_method=%d" % (tag, N, qm), lambda: gpu.planner_solve(d, *args, models=models))
        for N in NS:
            for V in SLOTS:
                if V == 0:
                    p = synth.cfg2_mpccbf(1, N=N, n_obs=1, safe_start=False)
                    args = (p["x0"], p["xt"], np.zeros((1, 0, N + 1)), np.zeros((1, 0, N + 1)), np.zeros((1, 0)), np.zeros(1, np.int32))
                else:
                    p = synth.cfg2_mpccbf(1, N=N, n_obs=V, safe_start=False)
                    args = (p["x0"], p["xt"], p["obs_s"], p["obs_ey"], p["lap_off"], p["n_obs"].astype(np.int32))
                for deg in DEGREES:
                    d = abi.cbf_desc(N, V, A, B, degree=deg)
                    attempt("%scbf N=%d slots=%d degree=%d" % (tag, N, V, deg), lambda: gpu.cbf_solve(d, *args, models=models))
    L.crx_debug_speculation(1)
    for N in (10, 12):
        p = synth.cfg2_mpccbf(1, N=N, n_obs=1, safe_start=False)
        d = abi.cbf_desc(N, 1, A, B)
        attempt("two-wave cbf N=%d slots=1 degree=6" % N,
                lambda: gpu.cbf_solve(d, p["x0"], p["xt"], p["obs_s"], p["obs_ey"], p["lap_off"], p["n_obs"].astype(np.int32)))
    L.crx_debug_speculation(0)


def queries():
    import ctypes as C
    import crx

    crx.init()
    L = crx.lib()
    L.crx_debug_lds_bytes.restype = C.c_long
    for N in NS:
        for V in SLOTS:
            print("N=%d slots=%d resident/CU %d  LDS %d B" % (N, V, L.crx_debug_resident_per_cu(0, N, V), L.crx_debug_lds_bytes(0, N, V)))


def names(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        if not r["Kernel_Name"].startswith("__amd_"):   # (the runtime's own copy kernels around the host-pointer calls)
            print(r["Kernel_Name"])


if __name__ == "__main__":
    {"launch": launch, "queries": queries, "names": lambda: names(sys.argv[2])}[sys.argv[1]]()
