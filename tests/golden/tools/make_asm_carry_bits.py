"""Choose and record tests/golden/asm_carry_bits.npz: problems that enter the Newton assembly of the one-obstacle interior-point loop in every way
it can be entered, and every output of crx_cbf_solve for them, as the library whose bits are to be pinned computes it.

    python tests/golden/tools/make_asm_carry_bits.py --select-only          the choice and its proof, on the CPU oracle alone (no GPU)
    python tests/golden/tools/make_asm_carry_bits.py [OUT.npz]               the same, then the recording: on an MI355X, with the library of the
                                                                             commit BEFORE a change to the kernels (CRX_LIB=...), never the changed one

The choice (deterministic; the paths, the trace reader and the encoding are the test's own: tests/test_gpu_asm_carry_bits.py PATHS, paths_of()), made
as make_uniform_ctrl_bits.py makes its own: synth.cfg2_mpccbf(64, N, seed, safe_start=False) is drawn for the seeds of SEEDS in that order, every
problem is solved ALONE by the CPU oracle with its iteration trace on, and the draws are scanned until every path of PATHS has been seen at the
horizon.  Per path the first PER_PATH problems that show it are taken; the batch is filled to 64 with the remaining problems of the first draw, in
index order.  The proof is asserted here from the oracle's trace of the CHOSEN batch, per horizon, and the path its trace cannot show (UNVERIFIED)
is printed by name with its proxy count.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", "..", ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "car-racing_amd"), os.path.join(ROOT, "tests"), HERE]

import bit_pins as P   # noqa: E402
import test_gpu_asm_carry_bits as T   # noqa: E402
from make_uniform_ctrl_bits import SEEDS, write_npz   # noqa: E402

PER_PATH = 3
MIN_DRAWS = 6   # restarts, jam re-runs and absent obstacles are one or two per draw: the scan goes on for this many draws, or until every path has PER_PATH problems


def choose(orc, AB, N):
    """-> (src [n, 2] int32 = (seed, index) per chosen problem, the arguments of crx_cbf_solve for them, the descriptor)"""
    seen = {p: [] for p in T.PATHS}
    draws, d = {}, None
    for seed in SEEDS:
        p = draws[seed] = P.draw(N, seed)
        d = d or P.descriptor(N, AB, p)
        _, per = T.batch_paths(orc, d, [np.asarray(p[k]) for k in P.INPUTS])
        for i, n in enumerate(per):
            for path in T.PATHS:
                if n[path] and len(seen[path]) < PER_PATH:
                    seen[path].append((seed, i))
        print("N = %d: seed %d scanned, problems per path so far: %s" % (N, seed, {k: len(v) for k, v in seen.items()}))
        if all(seen.values()) and (len(draws) >= MIN_DRAWS or all(len(v) >= PER_PATH for v in seen.values())):
            break
    missing = [k for k, v in seen.items() if not v]
    assert not missing, (N, "no problem of the scanned draws takes", missing)
    rank = {s: r for r, s in enumerate(SEEDS)}
    chosen = sorted(set(sum(seen.values(), [])), key=lambda si: (rank[si[0]], si[1]))
    for i in range(P.DRAW):   # the rest of the first draw
        if len(chosen) >= P.BATCH:
            break
        if (SEEDS[0], i) not in chosen:
            chosen.append((SEEDS[0], i))
    chosen.sort(key=lambda si: (rank[si[0]], si[1]))
    assert len(chosen) <= P.BATCH
    src = np.array(chosen, dtype=np.int32)
    args = [np.ascontiguousarray(np.stack([np.asarray(draws[s][k])[i] for s, i in chosen])) for k in P.INPUTS]
    return src, args, d


def prove(orc, d, N, args):
    ro, per = T.batch_paths(orc, d, args)
    n = T.totals(per)
    print("N = %d, %d problems, by the oracle: %s" % (N, len(args[0]), {k: n[k] for k in T.PATHS}))
    for what in T.PATHS:
        assert n[what] >= 1, (N, what, n)
    for k, why in T.UNVERIFIED.items():
        print("N = %d, UNVERIFIED %s: %s -- proxy count %d" % (N, k, why, n[k]))
    print("N = %d, oracle status counts %s, longest %d, total %d iterations" % (N, np.bincount(ro["status"], minlength=6).tolist(), int(ro["iters"].max()), int(ro["iters"].sum())))
    return ro


def main(argv):
    import oracle

    select_only = "--select-only" in argv
    out = ([a for a in argv if not a.startswith("--")] or [os.path.join(ROOT, "tests", "golden", "asm_carry_bits.npz")])[0]
    orc = oracle.load()
    AB = (np.genfromtxt(os.path.join(ROOT, "data/sys/LTI/matrix_A.csv"), delimiter=","), np.genfromtxt(os.path.join(ROOT, "data/sys/LTI/matrix_B.csv"), delimiter=","))
    arrays, todo = {}, []
    for N in P.HORIZONS:
        src, args, d = choose(orc, AB, N)
        ro = prove(orc, d, N, args)
        arrays["N%d/src" % N] = src
        for k, a in zip(P.INPUTS, args):
            arrays["N%d/in/%s" % (N, k)] = a
        todo.append((N, d, args, ro))
    if select_only:
        return
    import crx

    gpu = crx.init()
    print("recording with", crx.LIB_PATH)
    for N, d, args, ro in todo:
        rg = gpu.cbf_solve(d, *args)
        assert sorted(rg) == sorted(P.OUTPUTS), sorted(rg)
        again = gpu.cbf_solve(d, *args)
        for k in P.OUTPUTS:
            assert np.array_equal(P.bits(rg[k]), P.bits(again[k])), (N, k, "two launches of the same library disagree")
            arrays["N%d/%s" % (N, k)] = rg[k]
        assert np.array_equal(rg["status"], ro["status"]) and np.array_equal(rg["iters"], ro["iters"]), (N, "the GPU and the oracle took different paths")
        print("N = %d recorded: status counts %s, longest %d" % (N, np.bincount(rg["status"], minlength=6).tolist(), int(rg["iters"].max())))
    write_npz(out, arrays)
    z = np.load(out, allow_pickle=False)
    for k, a in arrays.items():
        assert z[k].dtype == a.dtype and np.array_equal(P.bits(z[k]), P.bits(a)), k
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
