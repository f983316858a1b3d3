"""The tuned one-obstacle NLP kernels with their line-search decisions taken as scalar branches (round 22, CRX_UNIFORM_CTRL), bit for bit against
a recording of the PARENT commit's library.

crx_solve_kernel<1,12,6,12> and <1,12,6,10> pass the conditions of the backtracking loop -- the trial loop's alpha >= alpha_min, theta_max / NaN,
the filter verdict, the switching condition, Armijo, sufficient decrease -- through wave_uniform (crx_wave.h): where a value lives changes, no
floating-point operation does, so no output bit may move.  A wrong branch would: a decision read from the first lane that the other lanes did not
share, or a scalar loop leaving a trial early, changes the accepted step length and with it every later iterate.

The problems are CHOSEN so that every decision of the interior-point loop that round 22 looked at falls both ways at least once (PATHS below; the
round rewrote the line search only, the list is the whole loop's so that a later round that moves another decision has its cases here).  They are
single problems of synth.cfg2_mpccbf(64, N, seed, safe_start=False) draws, at most 64 per horizon: "N12/src" lists (seed, index) of each.
tests/golden/tools/make_uniform_ctrl_bits.py searches the draws on the CPU ORACLE, which runs the same algorithm, and proves the choice from the
oracle's iteration trace (crx_oracle_set_verbose(1)); test_fixture_holds_every_path repeats that proof, without a GPU, on every run.  Two paths the
oracle's trace cannot show are listed in UNVERIFIED, not assumed: the trace does not say WHY a trial was refused (filter entry, theta_max or plain
insufficient decrease), and the oracle factorises densely, so a sigma_0 pivot that fails behind a clean sweep has no counterpart in it.  For each a
proxy count is printed (backtracked trials under a non-empty filter; corrected iterations).

tests/golden/uniform_ctrl_bits.npz: the six inputs ("N12/in/x0", ..) and the seven outputs ("N12/X", ..) of crx_cbf_solve for both horizons, recorded
on an MI355X with libcrx.so built from the parent of the commit that added this test (the shared-model launch, problems in index order).  The GPU
tests run the recorded inputs through the shared-model and the per-problem-model entries, in index order and permuted, and compare status,
iterations, KKT error and every trajectory array bit for bit.
"""
import os
import re
import sys
import tempfile

import numpy as np
import pytest

import conftest

HORIZONS = (12, 10)
DRAW = 64    # problems per synth draw
BATCH = 64   # problems per horizon in the fixture, at most
INPUTS = ("x0", "xt", "obs_s", "obs_ey", "lap_off", "n_obs")
OUTPUTS = ("X", "U", "sigma", "cost", "status", "kkt", "iters")
JAM_COUNT, JAM_ALPHA = 5, 1e-3   # crx_kernels.hip / crx_oracle.c
# what the oracle's trace proves of one problem
PATHS = ("backtracked",        # a step accepted behind at least one refused trial (ls >= 1)
         "armijo",             # accepted by the Armijo test under the switching condition (ftype = 1)
         "append",             # accepted by sufficient decrease, and the filter grew by the entry
         "ls_failed",          # no acceptable step: restoration or restart entered with acc = 0
         "jam_rerun",          # a jam exit that finds nothing to restore and re-runs the iteration
         "two_mu",             # the barrier parameter reduced twice (or more) in one iteration
         "dw0_doomed",         # a corrected iteration whose dw = 0 attempt failed, cold schedule (dw_last = 0)
         "dw3_doomed",         # a corrected iteration whose dw_last / 3 attempt failed as well (warm schedule, grown at least once)
         "restart")            # a restart from the crash point
UNVERIFIED = {"filter_reject": "a trial refused by a filter entry (proxy: trials refused while the filter is not empty)",
              "sigma0_pivot": "a sigma_0 pivot that fails behind a clean sweep (proxy: corrected iterations; the oracle factorises densely)"}

_IT = re.compile(r"^it +(\d+) f \S+ ed \S+ ep (\S+) ec \S+ mu (\S+) dw (\S+) nf (\d+)")
_STEP = re.compile(r"a_p (\S+) a_d \S+ alpha (\S+) acc (\d) ftype (\d) theta \S+ Dphi \S+ curv \S+ dw (\S+)")
_AGAIN = re.compile(r"(RESTART|RESTORE).*\(acc (\d) jam (\d+)\)")


def draw(N, seed):
    from crx import synth

    return synth.cfg2_mpccbf(DRAW, N=N, seed=int(seed), safe_start=False)


def descriptor(N, AB, p):
    from crx import abi

    return abi.cbf_desc(N, 1, AB[0], AB[1], alpha=p["alpha"], margin=p["margin"])


def oracle_trace(orc, d, args):
    """-> (outputs of the oracle, the lines of its iteration trace).  One thread: the lines of a problem stay together."""
    import oracle

    threads = oracle.threads()
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            oracle.set_threads(1)
            orc.lib.crx_oracle_set_verbose(1)
            out = orc.cbf_solve(d, *args)
        finally:
            orc.lib.crx_oracle_set_verbose(0)
            oracle.set_threads(threads)
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        return out, tmp.read().decode().splitlines()


def paths_of(lines, opts):
    """-> {path or proxy: count} of ONE problem's trace.  The `it` line of iteration k prints mu, dw_last and the filter size as the iteration
    finds them (before its barrier update); the step line prints what the iteration did."""
    n = dict.fromkeys(PATHS + tuple(UNVERIFIED), 0)

    def one_mu(mu):   # crx_ipm.h, ipm_next_mu
        return max(opts.tol / 10.0, min(opts.kappa_mu * mu, mu ** opts.theta_mu))

    its = []   # per iteration: [ep, mu, dw_last, nf, step or None]
    for ln in lines:
        m = _IT.match(ln)
        if m:
            its.append([float(m.group(2)), float(m.group(3)), float(m.group(4)), int(m.group(5)), None, None])
            continue
        m = _STEP.search(ln)
        if m and its:
            its[-1][4] = (float(m.group(1)), float(m.group(2)), int(m.group(3)), int(m.group(4)), float(m.group(5)))
            continue
        m = _AGAIN.search(ln)
        if m and its:
            its[-1][5] = (m.group(1), int(m.group(2)))
    run = 0
    for k, (ep, mu, dwl, nf, step, again) in enumerate(its):
        nxt = its[k + 1] if k + 1 < len(its) else None
        # (mu is printed with two digits: a second reduction is a factor of 2.5 at the very least below the first -- at the floor tol / 10)
        if nxt is not None and again is None and nxt[1] < 0.7 * one_mu(mu) and one_mu(mu) > opts.tol / 10.0 * 1.01:
            n["two_mu"] += 1
        if step is None:
            continue
        a_p, al, acc, ftype, dw = step
        refused = al < 0.75 * a_p          # (the trial lengths halve; a_p is printed with four digits)
        n["backtracked"] += bool(acc and refused)
        n["armijo"] += bool(acc and ftype == 1)
        if acc and ftype == 0 and nxt is not None and again is None:
            reduced = nxt[1] != mu
            n["append"] += (nxt[3] == 1) if reduced else (nxt[3] == nf + 1)
        n["filter_reject"] += bool(refused and nf > 0)
        n["dw0_doomed"] += bool(dw != 0.0 and dwl == 0.0)
        n["dw3_doomed"] += bool(dwl != 0.0 and dw > 2.0 * dwl / 3.0)
        n["sigma0_pivot"] += dw != 0.0
        run = run + 1 if (acc and al < JAM_ALPHA and ep > opts.tol) else 0
        jammed = bool(acc and run >= JAM_COUNT)
        if again is not None:
            n["restart"] += again[0] == "RESTART"
            n["ls_failed"] += again[1] == 0
            run = 0
        elif jammed and nxt is not None:
            n["jam_rerun"] += 1            # followed by neither RESTART nor RESTORE: nothing to restore, the iteration runs again
    return n


def batch_paths(orc, d, args):
    """-> (oracle outputs per problem, stacked; list of paths_of() per problem): the problems solved ONE AT A TIME, so that a trace is one problem's"""
    outs, per = [], []
    for b in range(len(args[0])):
        out, lines = oracle_trace(orc, d, [np.ascontiguousarray(a[b:b + 1]) for a in args])
        outs.append(out)
        per.append(paths_of(lines, d.opts))
    return {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}, per


def totals(per):
    return {k: int(sum(p[k] for p in per)) for k in PATHS + tuple(UNVERIFIED)}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(conftest.GOLDEN, "uniform_ctrl_bits.npz"), allow_pickle=False)


def recorded_args(recorded, N):
    return [np.ascontiguousarray(recorded["N%d/in/%s" % (N, k)]) for k in INPUTS]


@pytest.mark.parametrize("N", HORIZONS)
def test_fixture_holds_every_path(N, AB, orc, recorded):
    """No GPU: the recorded inputs are the problems "src" names, and the oracle -- alone -- takes every path of PATHS on them."""
    src = recorded["N%d/src" % N]
    args = recorded_args(recorded, N)
    assert 1 <= len(src) <= BATCH and all(len(a) == len(src) for a in args)
    draws = {int(s): draw(N, s) for s in sorted(set(src[:, 0].tolist()))}
    for k, a in zip(INPUTS, args):
        want = np.stack([np.asarray(draws[int(s)][k])[int(i)] for s, i in src])
        assert a.dtype == want.dtype and np.array_equal(bits(a), bits(want)), (N, k, "the recorded inputs are not the draws' problems")
    d = descriptor(N, AB, draws[int(src[0, 0])])
    ro, per = batch_paths(orc, d, args)
    n = totals(per)
    print("N = %d, %d problems, by the oracle: %s" % (N, len(src), n))
    print("N = %d, NOT verifiable from the oracle's trace: %s" % (N, "; ".join("%s = %s" % kv for kv in UNVERIFIED.items())))
    for what in PATHS:
        assert n[what] >= 1, (N, what, n)
    # the recording's statuses and iteration counts are the oracle's (the GPU and the oracle run the same algorithm)
    assert np.array_equal(recorded["N%d/status" % N], ro["status"]), (N, np.nonzero(recorded["N%d/status" % N] != ro["status"])[0])
    assert np.array_equal(recorded["N%d/iters" % N], ro["iters"]), (N, np.nonzero(recorded["N%d/iters" % N] != ro["iters"])[0])


def _assert_recorded(N, route, got, recorded):
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


@pytest.fixture(scope="module", params=HORIZONS)
def batch(request, AB, recorded):
    import crx

    N = request.param
    args = recorded_args(recorded, N)
    d = descriptor(N, AB, draw(N, recorded["N%d/src" % N][0, 0]))
    return N, crx.init(), d, args


def _solve(gpu, d, args, AB, models, perm):
    """the batch through one entry; perm: problem i of the launch is problem perm[i] of the batch, the outputs are put back in batch order"""
    n = len(args[0])
    a = args if perm is None else [np.ascontiguousarray(x[perm]) for x in args]
    kw = dict(models=(np.repeat(AB[0][None], n, axis=0), np.repeat(AB[1][None], n, axis=0))) if models else {}
    got = gpu.cbf_solve(d, *a, **kw)
    if perm is not None:
        inv = np.argsort(perm)
        got = {k: np.ascontiguousarray(v[inv]) for k, v in got.items()}
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["index order", "permuted"])
@pytest.mark.parametrize("models", [False, True], ids=["shared model", "per-problem models"])
def test_bits_are_the_parents(batch, AB, recorded, models, order):
    N, gpu, d, args = batch
    perm = None if order == "index order" else np.random.default_rng(22).permutation(len(args[0]))
    got = _solve(gpu, d, args, AB, models, perm)
    _assert_recorded(N, "%s, %s" % ("per-problem models" if models else "shared model", order), got, recorded)
