"""Record tests/golden/lmpc_bits.npz: every output of crx_lmpc_solve for the cases of tests/test_gpu_lmpc_bits.py, as bit patterns.

Run on an MI355X with the library whose bits are to be pinned -- the commit BEFORE a change to crx_lmpc.hip, never the changed one:

    python tests/golden/tools/make_lmpc_bits.py [OUT.npz]        (default: tests/golden/lmpc_bits.npz)

The cases, their inputs and the encoding (byte planes, XOR against fix12) are the test's own: CASES, solve(), SUBSET, xor_base(), and
planes() of tests/bit_pins.py.  The file is read back through the test's recorded_bits() and compared with what was solved before it counts as
written.
"""
import os
import sys

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "car-racing_amd"), os.path.join(ROOT, "tests")]

import bit_pins as P   # noqa: E402
import test_gpu_lmpc_bits as T   # noqa: E402


def main(out):
    import crx

    gpu = crx.init()
    res = {case: {k: P.bits(np.asarray(v)) for k, v in T.solve(gpu, case).items()} for case in T.CASES}
    arrays = {}
    for case, r in res.items():
        assert sorted(r) == list(T.OUTPUTS), sorted(r)
        for k, b in r.items():
            if b.dtype == np.uint64:
                base = T.xor_base(case, k, lambda c, kk: res[c][kk])
                b = P.planes(b if base is None else b ^ base)
            arrays[case + "/" + k] = b
        print(case, "status counts", np.bincount(r["status"], minlength=6).tolist(), "longest", int(r["iters"].max()), "total", int(r["iters"].sum()))
    np.savez_compressed(out, **arrays)
    z = np.load(out, allow_pickle=False)
    for case, r in res.items():
        for k, b in r.items():
            back = T.recorded_bits(z, case, k)
            assert back.dtype == b.dtype and np.array_equal(back, b), (case, k)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "lmpc_bits.npz"))
