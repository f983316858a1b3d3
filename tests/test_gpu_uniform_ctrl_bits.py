"""The tuned one-obstacle NLP kernels with their line-search decisions taken as scalar branches (round 22), bit for bit against a recording of the
PARENT commit's library.  The round's A/B switch, CRX_UNIFORM_CTRL, is retired: the scalar branches are part of the lone-wave form of
crx_kernels.hip, and this test is the standing pin of that code.

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

import numpy as np
import pytest

import bit_pins
import conftest
from bit_pins import AGAIN, BATCH, HORIZONS, INPUTS, IT, JAM_ALPHA, JAM_COUNT, STEP, bits, descriptor, draw, recorded_args

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


def paths_of(lines, opts):
    """-> {path or proxy: count} of ONE problem's trace.  The `it` line of iteration k prints mu, dw_last and the filter size as the iteration
    finds them (before its barrier update); the step line prints what the iteration did."""
    n = dict.fromkeys(PATHS + tuple(UNVERIFIED), 0)

    def one_mu(mu):   # crx_ipm.h, ipm_next_mu
        return max(opts.tol / 10.0, min(opts.kappa_mu * mu, mu ** opts.theta_mu))

    its = []   # per iteration: [ep, mu, dw_last, nf, step or None]
    for ln in lines:
        m = IT.match(ln)
        if m:
            its.append([float(m.group(2)), float(m.group(3)), float(m.group(4)), int(m.group(5)), None, None])
            continue
        m = STEP.search(ln)
        if m and its:
            its[-1][4] = (float(m.group(1)), float(m.group(2)), int(m.group(3)), int(m.group(4)), float(m.group(5)))
            continue
        m = AGAIN.search(ln)
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
    return bit_pins.batch_paths(orc, d, args, lambda lines, b: paths_of(lines, d.opts))


def totals(per):
    return {k: int(sum(p[k] for p in per)) for k in PATHS + tuple(UNVERIFIED)}


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(conftest.GOLDEN, "uniform_ctrl_bits.npz"), allow_pickle=False)


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


@pytest.fixture(scope="module", params=HORIZONS)
def batch(request, AB, recorded):
    import crx

    N = request.param
    args = recorded_args(recorded, N)
    d = descriptor(N, AB, draw(N, recorded["N%d/src" % N][0, 0]))
    return N, crx.init(), d, args


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["index order", "permuted"])
@pytest.mark.parametrize("models", [False, True], ids=["shared model", "per-problem models"])
def test_bits_are_the_parents(batch, AB, recorded, models, order):
    N, gpu, d, args = batch
    perm = None if order == "index order" else np.random.default_rng(22).permutation(len(args[0]))
    got = bit_pins.solve(gpu, d, args, AB, models, perm)
    bit_pins.assert_recorded(N, "%s, %s" % ("per-problem models" if models else "shared model", order), got, recorded)
