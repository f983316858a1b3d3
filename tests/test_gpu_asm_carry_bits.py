"""The tuned one-obstacle NLP kernels with the Newton assembly's schedule changed (round 24), bit for bit against a recording of the PARENT commit's
library.  The round's A/B switch, CRX_ASM_CARRY, is retired: the schedule is part of the lone-wave form of crx_kernels.hip, and this test is the
standing pin of that code.

crx_solve_kernel<1,12,6,12> and <1,12,6,10> (obstacle unit and per-problem-model unit) rearrange assemble_newton: what the assembly of an
iteration computes must stay the same expression on the same operands whatever ran in front of it -- an accepted step that kept the barrier
parameter, one that cut it, a start, a restart, a restoration, a jam re-run, a convexified sweep that zeroed kS / kE behind it -- and whatever the
rows are: a problem whose obstacle is absent runs the one-slot kernel with every CBF row off, and the assembly still visits those rows.

The problems are CHOSEN so that each of those ways into the assembly occurs at least once per horizon (PATHS below).  They are single problems of
synth.cfg2_mpccbf(64, N, seed, safe_start=False) draws, at most 64 per horizon: "N12/src" lists (seed, index) of each.
tests/golden/tools/make_asm_carry_bits.py searches the draws on the CPU ORACLE, which runs the same algorithm, and proves the choice from the
oracle's iteration trace (crx_oracle_set_verbose(1)) and from the inputs; test_fixture_holds_every_path repeats that proof, without a GPU, on every
run.  Three paths are listed in UNVERIFIED, not assumed.  One the oracle's trace cannot show: it prints dw = 0 for an iteration whose matrix was
convexified, so a convexified run of two or more iterations is not visible in it; its proxy is a run of at least two iterations behind a RESTART --
the crash path, the only one on which the kernel convexifies, and on which the exact matrix fails for iterations in a row (crx_oracle.c, the
sticky convexification).  Two no problem of the draws takes: none of the 4160 problems per horizon that the tool's 65 seeds draw cuts mu in its
first iteration, and none prints RESTORE (a closed-form restoration that is not a restart; in the kernel a restart IS the restoration block, run
over all rows, and leaves it by the same `continue`).  Both are counted all the same, so a later fixture that holds one says so.

tests/golden/asm_carry_bits.npz: the six inputs ("N12/in/x0", ..) and the seven outputs ("N12/X", ..) of crx_cbf_solve for both horizons, recorded on
an MI355X with libcrx.so built from the parent of the commit that added this test (the shared-model launch, problems in index order).  The GPU tests
run the recorded inputs through the shared-model and the per-problem-model entries, in index order and permuted, and compare status, iterations,
KKT error and every trajectory array bit for bit.
"""
import os

import numpy as np
import pytest

import bit_pins
import conftest
import test_gpu_uniform_ctrl_bits as U   # its reader of the trace for two_mu / jam_rerun
from bit_pins import AGAIN, BATCH, HORIZONS, INPUTS, IT, STEP, bits, descriptor, draw, recorded_args

# what the oracle's trace (and n_obs) proves of one problem
PATHS = ("mu_kept",            # an iteration that keeps mu right after an accepted step
         "mu_cut",             # an iteration that cuts mu right after an accepted step
         "two_mu",             # mu cut twice (or more) in one iteration
         "after_restart",      # an iteration that runs right after a restart from the crash point (the kernel's restoration block, all rows)
         "jam_rerun",          # a jam exit that finds nothing to restore and re-runs the iteration
         "n_obs_0")            # a problem without an obstacle in the one-slot kernel: every CBF row is off
# not assumed: what the trace cannot show, and what no problem of the 65 draws the tool can scan (4160 problems per horizon) does -- counted all the
# same, so that a fixture that happens to hold one says so
UNVERIFIED = {"convex_run": "a convexified run of at least two iterations (proxy: runs of >= 2 iterations behind a RESTART; the trace prints dw = 0 for them)",
              "mu_cut_first": "mu cut in the first iteration of a solve (no scanned draw: the start's dual infeasibility is above kappa_eps mu_init)",
              "after_restore": "an iteration right after a closed-form restoration that is not a restart (no scanned draw prints RESTORE; the kernel "
                               "re-enters its loop at the same point after a restart, a restoration and a jam re-run)"}


def paths_of(lines, opts, n_obs):
    """-> {path or proxy: count} of ONE problem's trace.  The `it` line of iteration k prints mu as the iteration FINDS it (before its barrier
    update): the mu iteration k solved with is the one iteration k + 1 prints, unless a restart or a restoration (which reset mu) lies between."""
    n = dict.fromkeys(PATHS + tuple(UNVERIFIED), 0)
    u = U.paths_of(lines, opts)
    n["two_mu"], n["jam_rerun"] = u["two_mu"], u["jam_rerun"]
    n["n_obs_0"] = int(n_obs == 0)
    its = []   # per iteration: [mu found, accepted, RESTART / RESTORE behind it or None]
    for ln in lines:
        m = IT.match(ln)
        if m:
            its.append([float(m.group(3)), False, None])
            continue
        m = STEP.search(ln)
        if m and its:
            its[-1][1] = int(m.group(3)) == 1
            continue
        m = AGAIN.search(ln)
        if m and its:
            its[-1][2] = m.group(1)

    def mu_used(k):   # None where the trace does not show it
        return its[k + 1][0] if k + 1 < len(its) and its[k][2] is None else None

    behind_restart = 0
    for k, (mu, acc, again) in enumerate(its):
        used = mu_used(k)
        if k == 0 and used is not None and used < mu:
            n["mu_cut_first"] += 1
        if k >= 1 and its[k - 1][1] and its[k - 1][2] is None and used is not None:   # right after an accepted step: mu found = mu of that step
            n["mu_kept"] += used == mu
            n["mu_cut"] += used < mu
        if k >= 1 and its[k - 1][2] is not None:
            n["after_restart"] += its[k - 1][2] == "RESTART"
            n["after_restore"] += its[k - 1][2] == "RESTORE"
        if k >= 1 and its[k - 1][2] == "RESTART":
            behind_restart = 1
        elif behind_restart and its[k - 1][2] is None:
            behind_restart += 1
            n["convex_run"] += behind_restart == 2
        else:
            behind_restart = 0
    return n


def batch_paths(orc, d, args):
    n_obs = np.asarray(args[INPUTS.index("n_obs")])
    return bit_pins.batch_paths(orc, d, args, lambda lines, b: paths_of(lines, d.opts, int(n_obs[b])))


def totals(per):
    return {k: int(sum(p[k] for p in per)) for k in PATHS + tuple(UNVERIFIED)}


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(conftest.GOLDEN, "asm_carry_bits.npz"), allow_pickle=False)


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
    perm = None if order == "index order" else np.random.default_rng(24).permutation(len(args[0]))
    got = bit_pins.solve(gpu, d, args, AB, models, perm)
    bit_pins.assert_recorded(N, "%s, %s" % ("per-problem models" if models else "shared model", order), got, recorded)
