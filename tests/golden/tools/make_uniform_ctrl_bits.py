"""Choose and record tests/golden/uniform_ctrl_bits.npz: problems on which every decision of the one-obstacle interior-point loop falls both ways,
and every output of crx_cbf_solve for them, as the library whose bits are to be pinned computes it.

    python tests/golden/tools/make_uniform_ctrl_bits.py --select-only          the choice and its proof, on the CPU oracle alone (no GPU)
    python tests/golden/tools/make_uniform_ctrl_bits.py [OUT.npz]               the same, then the recording: on an MI355X, with the library of the
                                                                                commit BEFORE a change to the kernels (CRX_LIB=...), never the changed one

The choice (deterministic; the paths, the trace reader and the encoding are the test's own: tests/test_gpu_uniform_ctrl_bits.py PATHS, paths_of()):
synth.cfg2_mpccbf(64, N, seed, safe_start=False) is drawn for the seeds of SEEDS in that order, every problem is solved ALONE by the CPU oracle with
its iteration trace on, and the draws are scanned until every path of PATHS has been seen at the horizon.  Per path the first PER_PATH problems that
show it are taken; the batch is filled to 64 with the remaining problems of the first draw, in index order.  The proof is asserted here from the
oracle's trace of the CHOSEN batch, per horizon -- a condition on the inputs, which the oracle alone has to meet -- and the two paths its trace cannot
show (UNVERIFIED) are printed by name with their proxy counts.

The file is written with fixed zip timestamps and no compression: the same library on the same inputs gives the same bytes.
"""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "car-racing_amd"), os.path.join(ROOT, "tests")]

import bit_pins as P   # noqa: E402
import test_gpu_uniform_ctrl_bits as T   # noqa: E402

SEEDS = (67,) + tuple(s for s in range(64) if s != 67)   # 67: the draw of tests/test_gpu_obs1_carry_bits.py (restart, restoration, jam exits at both horizons)
PER_PATH = 3


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
        if all(seen.values()):
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


def write_npz(path, arrays):
    """np.savez with nothing that changes from run to run: entries in the order given, stored, timestamps of 1980-01-01"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def main(argv):
    import oracle

    select_only = "--select-only" in argv
    out = ([a for a in argv if not a.startswith("--")] or [os.path.join(ROOT, "tests", "golden", "uniform_ctrl_bits.npz")])[0]
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
