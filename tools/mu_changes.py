"""In how many iterations of the headline batch does the barrier parameter change?  (Round 24: an assembly that is skipped while mu stands still pays
only in those that keep it.)
python tools/mu_changes.py [index ...]
  the whole batch: the CPU oracle's iteration trace, one problem at a time (the same algorithm: the iteration counts are the kernel's; no GPU)
  the named problems (default: none) once more from the kernel's own trace rows (needs a GPU and a -DCRX_PHASE_CLOCKS build: CRX_LIB=tools/ab/libcrx_trace.so)
An iteration "changes mu" when the mu it solves with differs from the previous iteration's; the first iteration of a solve and the one behind a
restart / restoration (mu reset) are counted apart: they assemble everything anyway."""
import os, sys, ctypes as C
ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, ROOT + "/car-racing_amd", ROOT + "/tests"]
import numpy as np
from crx import abi, synth
import oracle
import bit_pins as U   # the oracle's trace and its line formats

KEYS = ("x0", "xt", "obs_s", "obs_ey", "lap_off", "n_obs")
A, B = synth.load_AB()
p = synth.cfg2_mpccbf(256, safe_start=False); d = abi.cbf_desc(12, 1, A, B, alpha=0.8, margin=0.2)
orc = oracle.load()


def count(mus, reset):
    """mus[k]: mu iteration k solved with; reset[k]: iteration k is a first one (start, behind a restart / restoration) -> (kept, changed, first)"""
    kept = changed = first = 0
    for k, mu in enumerate(mus):
        if k == 0 or reset[k]: first += 1
        elif mu == mus[k - 1]: kept += 1
        else: changed += 1
    return kept, changed, first


tot = np.zeros(3, dtype=int); per = []
for b in range(256):
    out, lines = U.oracle_trace(orc, d, [np.ascontiguousarray(p[k][b:b + 1]) for k in KEYS])
    found, again = [], []
    for ln in lines:
        m = U.IT.match(ln)
        if m: found.append(float(m.group(3))); again.append(False); continue
        if U.AGAIN.search(ln) and again: again[-1] = True
    # the mu iteration k solved with is the one iteration k + 1 finds (printed with two digits; a cut is a factor of 5 at least above the floor);
    # behind a restart / restoration, and for the last iteration, the trace does not show it: those iterations are left out
    mus = [found[k + 1] for k in range(len(found) - 1) if not again[k]]
    reset = [k > 0 and again[k - 1] for k in range(len(found) - 1) if not again[k]]
    c = count(mus, reset); tot += c; per.append((int(out["iters"][0]), b, c))
print("headline batch (256 problems), CPU oracle: %d iterations keep mu, %d change it, %d are first ones (start / behind a restart): changed / (kept + changed) = %.1f %%"
      % (tot[0], tot[1], tot[2], 100.0 * tot[1] / (tot[0] + tot[1])))
for it, b, c in sorted(per, reverse=True)[:4]:
    print("  #%d, %d iterations: kept %d, changed %d, first %d: %.1f %%" % (b, it, c[0], c[1], c[2], 100.0 * c[1] / max(1, c[0] + c[1])))
if len(sys.argv) > 1:
    import crx
    gpu = crx.init(); L = crx.lib()
    for idx in map(int, sys.argv[1:]):
        L.crx_trace_enable(0, 64)
        rr = gpu.cbf_solve(d, *[p[k][idx:idx + 1] for k in KEYS])
        buf = np.zeros((64, 16)); L.crx_trace_read(buf.ctypes.data_as(C.c_void_p), 64)
        L.crx_trace_enable(0, 0)
        n = min(int(rr["iters"][0]), 64)
        mus = buf[:n, 3].tolist()
        # (a restart / restoration resets mu to mu_init: an iteration whose mu is ABOVE the previous one's is behind one)
        c = count(mus, [k > 0 and mus[k] > mus[k - 1] for k in range(n)])
        print("  #%d on the GPU (trace rows), %d iterations: kept %d, changed %d, first %d: %.1f %%   mu: %s" % (idx, n, c[0], c[1], c[2], 100.0 * c[1] / max(1, c[0] + c[1]), " ".join("%.1e" % m for m in mus)))
