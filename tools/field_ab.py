"""A/B of two builds of the field family's prep kernels (crx_field_prep_kernel, crx_field_traffic_kernel, crx_mixed_prep_kernel in
csrc/crx_prep.hip), bit for bit: every output array of field_prep_dev, field_traffic_dev and mixed_prep_dev on the draws of
tests/test_gpu_field.py and tests/test_gpu_mixed.py at the shapes their tests use -- R = 37 (a partial block for every C in 1, 2, 4, 7) and
R = 150 (several blocks), both tracks, N in 10, 24, N_ilqr in 0, 12, 50 with both ilqr_obstacles modes, with and without car_dims, with
`clear` on and off.  Usage: [CRX_LIB=...] python tools/field_ab.py TAG;  python tools/field_ab.py --compare A B   (dumps under tools/ab/)"""
import os
import sys

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, ROOT + "/car-racing_amd", ROOT + "/tests"]
OUT = ROOT + "/tools/ab/field_ab_%s.npz"
if sys.argv[1] == "--compare":
    a, b = np.load(OUT % sys.argv[2]), np.load(OUT % sys.argv[3])
    bad = [k for k in sorted(set(a.files) | set(b.files)) if k not in a.files or k not in b.files or a[k].tobytes() != b[k].tobytes()]
    print("compared %d arrays of %s and %d of %s: %s" % (len(a.files), sys.argv[2], len(b.files), sys.argv[3],
                                                          "IDENTICAL" if not bad else "DIFFERENT in %s" % bad))
    sys.exit(1 if bad else 0)
import crx   # noqa: E402
from crx import abi   # noqa: E402
import test_gpu_field as tf   # noqa: E402
import test_gpu_field_game as tg   # noqa: E402
import test_gpu_mixed as tm   # noqa: E402

crx.init(0)
out = {}


def keep(tag, r):
    for k, v in r.items():
        out["/".join(str(t) for t in tag) + "/" + k] = v


for name in tm.TRACKS:
    for C in tm.CARS:
        for R in (tf.R_PREP, 150):
            for N in (10, 24) if R == tf.R_PREP else (10,):
                tab, L, x, dims, _ = tf.draw(name, C, N, 100 * C + N, R=R)
                fdesc = abi.field_desc(N, C, tab.shape[0], L)
                keep(("traffic", name, C, R, N), tg._run(fdesc, tab, x))
                for d in (None, dims):
                    for clear in (False, True):
                        keep(("field", name, C, R, N, d is not None, clear), tf._run(fdesc, tab, x, d, clear))
            for n_ilqr in tm.N_ILQR:
                tab, L, x, dims, pol = tm.draw(name, C, tm.N_PREP, n_ilqr, 100 * C + n_ilqr, R=R)
                for mode in (0, 1):
                    mdesc = abi.mixed_desc(tm.N_PREP, n_ilqr, C, tab.shape[0], L, ilqr_obstacles=mode)
                    for d in (None, dims):
                        for clear in (False, True):
                            keep(("mixed", name, C, R, n_ilqr, mode, d is not None, clear), tm._run(mdesc, tab, x, pol, d, clear))
os.makedirs(os.path.dirname(OUT), exist_ok=True)
np.savez(OUT % sys.argv[1], **out)
print("%s: %d output arrays of %d launches dumped (%s)" % (sys.argv[1], len(out), len({k.rsplit("/", 1)[0] for k in out}), crx.lib()._name))
