"""What the bit-pin tests (tests/test_gpu_*_bits.py) and the tools that record their fixtures (tests/golden/tools/make_*_bits.py) share: how bit
patterns are compared with a recording, how the CPU oracle's iteration trace is captured and read, and how a recorded batch of crx_cbf_solve goes
through the entries of the library.  A plain module, imported by name.  Seeds, case tables, the paths a fixture must hold and the reading of a trace
for them stay in the test module they belong to.
"""
import os
import re
import sys
import tempfile

import numpy as np

# crx_cbf_solve: the arguments behind the descriptor, and every output
INPUTS = ("x0", "xt", "obs_s", "obs_ey", "lap_off", "n_obs")
OUTPUTS = ("X", "U", "sigma", "cost", "status", "kkt", "iters")
JAM_COUNT, JAM_ALPHA = 5, 1e-3   # crx_kernels.hip / crx_oracle.c

# the oracle's iteration trace (crx_oracle_set_verbose(1); oracle/crx_oracle.c has the formats).  Groups:
#   IT     the line an iteration begins with: 1 it, 2 e_p, 3 mu, 4 dw_last, 5 nf -- as the iteration FINDS them
#   STEP   what the iteration did: 1 a_p, 2 alpha, 3 acc, 4 ftype, 5 dw
#   AGAIN  a restart from the crash point or a restoration behind it: 1 which, 2 acc, 3 jam
IT = re.compile(r"^it +(\d+) f \S+ ed \S+ ep (\S+) ec \S+ mu (\S+) dw (\S+) nf (\d+)")
STEP = re.compile(r"a_p (\S+) a_d \S+ alpha (\S+) acc (\d) ftype (\d) theta \S+ Dphi \S+ curv \S+ dw (\S+)")
AGAIN = re.compile(r"(RESTART|RESTORE).*\(acc (\d) jam (\d+)\)")


def bits(a):
    """float64 as its 64-bit patterns, anything else as it is"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def planes(b):
    """uint64 [*S] -> uint8 [8, *S] (byte i of every value together, so that signs and exponents compress): how plain_bits.npz, feedback_layout_bits.npz
    and lmpc_bits.npz hold a float64 output"""
    return np.ascontiguousarray(np.moveaxis(np.ascontiguousarray(b)[..., None].view(np.uint8), -1, 0))


def unplanes(a):
    """uint8 [8, *S] -> uint64 [*S]"""
    return np.ascontiguousarray(np.moveaxis(a, 0, -1)).view(np.uint64)[..., 0]


def oracle_stderr(orc, run):
    """-> (run(), what the oracle wrote to stderr meanwhile) with its iteration trace on.  One thread: the lines of a problem stay together."""
    import oracle

    threads = oracle.threads()
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            oracle.set_threads(1)
            orc.lib.crx_oracle_set_verbose(1)
            out = run()
        finally:
            orc.lib.crx_oracle_set_verbose(0)
            oracle.set_threads(threads)
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        return out, tmp.read().decode()


def nonzero_dw(text):
    """iterations of a trace with delta_w != 0"""
    return sum(1 for m in re.findall(r"curv \S+ dw (\S+)", text) if float(m) != 0.0)


def recorded_args(recorded, N):
    return [np.ascontiguousarray(recorded["N%d/in/%s" % (N, k)]) for k in INPUTS]


def assert_recorded(N, route, got, recorded):
    """every output of `got` against "N<N>/<output>" of the recording: the problems that differ per output, printed, and none may"""
    assert sorted(got) == sorted(OUTPUTS)
    report = []
    for k in OUTPUTS:
        want = recorded["N%d/%s" % (N, k)]
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, (route, k)
        diff = np.nonzero((bits(got[k]) != bits(want)).reshape(len(want), -1).any(axis=1))[0]
        print("N = %d, %s, %s: %d problems differ from the recording%s" % (N, route, k, diff.size, "" if diff.size == 0 else ", first %d" % diff[0]))
        if diff.size:
            report.append((k, int(diff.size), int(diff[0])))
    assert not report, (N, route, report)


def assert_same_bits(what, k, got, want):
    """one output against its recorded bit patterns (both as bits() gives them), entry by entry"""
    assert got.dtype == want.dtype and got.shape == want.shape, k
    diff = np.nonzero(got != want)
    assert diff[0].size == 0, (what, k, "differs from the recording in %d entries, first at problem %d" % (diff[0].size, diff[0][0]))


def shipped_models(AB, n):
    """per-problem models that are n copies of the shipped model"""
    return (np.repeat(AB[0][None], n, axis=0), np.repeat(AB[1][None], n, axis=0))


def solve(gpu, d, args, AB, models, perm):
    """the batch through one entry; perm: problem i of the launch is problem perm[i] of the batch, the outputs are put back in batch order"""
    a = args if perm is None else [np.ascontiguousarray(x[perm]) for x in args]
    kw = dict(models=shipped_models(AB, len(args[0]))) if models else {}
    got = gpu.cbf_solve(d, *a, **kw)
    if perm is not None:
        inv = np.argsort(perm)
        got = {k: np.ascontiguousarray(v[inv]) for k, v in got.items()}
    return got


def solve_two_wave_idle(gpu, d, args):
    """the batch through the two-wave unit with its second wave idle (crx_debug_speculation(2)): the one-wave schedule"""
    import crx

    L = crx.lib()
    try:
        L.crx_debug_speculation(2)
        return gpu.cbf_solve(d, *args)
    finally:
        L.crx_debug_speculation(0)


# ---- fixtures of CHOSEN problems (uniform_ctrl_bits.npz, asm_carry_bits.npz): single problems of synth.cfg2_mpccbf(64, N, seed, safe_start=False) draws,
# "N<N>/src" = (seed, index) of each, chosen and proved by the oracle's trace of every problem solved alone
HORIZONS = (12, 10)
DRAW = 64    # problems per synth draw
BATCH = 64   # problems per horizon in the fixture, at most


def draw(N, seed):
    from crx import synth

    return synth.cfg2_mpccbf(DRAW, N=N, seed=int(seed), safe_start=False)


def descriptor(N, AB, p):
    from crx import abi

    return abi.cbf_desc(N, 1, AB[0], AB[1], alpha=p["alpha"], margin=p["margin"])


def oracle_trace(orc, d, args):
    """-> (outputs of the oracle, the lines of its iteration trace)"""
    out, text = oracle_stderr(orc, lambda: orc.cbf_solve(d, *args))
    return out, text.splitlines()


def batch_paths(orc, d, args, paths_of):
    """-> (oracle outputs per problem, stacked; list of paths_of(lines, b) per problem b): the problems solved ONE AT A TIME, so that a trace is one
    problem's"""
    outs, per = [], []
    for b in range(len(args[0])):
        out, lines = oracle_trace(orc, d, [np.ascontiguousarray(a[b:b + 1]) for a in args])
        outs.append(out)
        per.append(paths_of(lines, b))
    return {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}, per
