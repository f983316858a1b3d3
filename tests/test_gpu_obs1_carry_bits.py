"""The tuned one-obstacle NLP kernels after the carry-forward of round 21, bit for bit against a recording of the PARENT commit's library.

Round 21 stops crx_solve_kernel<1,12,6,12> and <1,12,6,10> forming two things twice: first_order at the end of the accept step takes the four
normalised CBF distances of a lane's row from the accepted line-search trial, and the accept pass takes the multiplier step dnu of every row from
the row-step pass, through the first rows of Kk.  (The round's A/B switches, CRX_DIST_CARRY and CRX_DNU_CARRY, are retired: both carries are part
of the lone-wave form of crx_kernels.hip, and this test is the standing pin of that code.)  Both carry a number that the second place formed from the same operands with
the same roundings, so no output bit may move.  This test pins that, on a batch in which the carried values could be the WRONG ones:

  * a step accepted after backtracking -- the carried distances must be the last trial's, not the first's;
  * a restart from the crash point -- the first_order behind it has no accepted trial and must evaluate afresh;
  * a closed-form restoration and a solve that ends restored (status 3, CRX_RESTORED);
  * a jam exit (ls_failed == 2: an accepted step thrown away behind the row steps, which have stored their dnu by then), among them one that finds
    nothing to restore and re-runs the iteration from its top -- the re-run's adjoint sweep reads hg as the abandoned iteration left it, which is
    why dnu is not parked there;
  * an iteration with a non-zero delta_w (inertia correction: the backward sweep that overwrites Kk runs more than once);
  * a problem with n_obs = 0 in the one-slot instantiation (the `here == false` arm of first_order).

The batch: synth.cfg2_mpccbf(64, N, seed=67, safe_start=False), N = 12 and N = 10.  Seeds 0 .. 402 were searched on the CPU oracle for a batch
that holds ALL of the above at BOTH horizons, counted from the oracle's iteration trace (crx_oracle_set_verbose(1), one thread): 67 is the only
one (most draws have no absent obstacle, no restart or no jam).  The presences are asserted below from that trace, every run, so the test cannot
pass on a draw that exercises nothing; statuses and iteration counts of the GPU are compared with the oracle's, problem by problem.

tests/golden/obs1_carry_bits.npz holds the six inputs ("N12/in/x0", ..) and the seven outputs ("N12/X", ..) of crx_cbf_solve for both horizons:
recorded on an MI355X with libcrx.so built from the parent of the commit that added this test (the shared-model launch; the per-problem-model
route and the two-wave kernel with its second wave idle gave the same bits there).  Inputs and outputs only.

The same inputs then go through the per-problem-model unit (which carries, too) and the two-wave unit with its second wave idle (which keeps
the evaluations: its register file has no room for the carried values); both must give the recording's bits.
"""
import os

import numpy as np
import pytest

import bit_pins
import conftest
from bit_pins import AGAIN, INPUTS, IT, JAM_ALPHA, JAM_COUNT, OUTPUTS, STEP, bits

pytestmark = pytest.mark.gpu

SEED = 67
BATCH = 64


def _oracle_trace(orc, d, args):
    """-> (outputs of the oracle, counts over the batch read from its iteration trace)"""
    out, text = bit_pins.oracle_stderr(orc, lambda: orc.cbf_solve(d, *args))
    lines = text.splitlines()
    n = dict(backtracked=0, restart=0, restore=0, jam_exit=0, jam_rerun=0, inertia=0)
    run, ep, pending = 0, 0.0, False
    for ln in lines:
        m = IT.match(ln)
        if m:   # the next iteration begins: a jam that was followed by neither RESTART nor RESTORE had nothing to restore
            n["jam_rerun"] += pending
            pending = False
            if int(m.group(1)) == 0:
                run = 0
            ep = float(m.group(2))
            continue
        m = STEP.search(ln)
        if m:
            a_p, al, acc, dw = float(m.group(1)), float(m.group(2)), int(m.group(3)), float(m.group(5))
            n["backtracked"] += bool(acc and al < 0.75 * a_p)     # (the trial lengths halve; a_p is printed with four digits)
            n["inertia"] += dw != 0.0
            run = run + 1 if (acc and al < JAM_ALPHA and ep > d.opts.tol) else 0
            pending = bool(acc and run >= JAM_COUNT)
            continue
        m = AGAIN.search(ln)
        if m:
            pending, run = False, 0
            n["restart" if m.group(1) == "RESTART" else "restore"] += 1
            n["jam_exit"] += int(m.group(2)) == 1               # thrown away although the line search had accepted it
    return out, n


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(conftest.GOLDEN, "obs1_carry_bits.npz"), allow_pickle=False)


@pytest.fixture(scope="module", params=[12, 10])
def batch(request, AB, recorded):
    """-> (N, gpu, descriptor, arguments): the recorded inputs, which are the draw the docstring names."""
    import crx
    from crx import abi, synth

    N = request.param
    p = synth.cfg2_mpccbf(BATCH, N=N, seed=SEED, safe_start=False)
    args = bit_pins.recorded_args(recorded, N)
    for k, a in zip(INPUTS, args):
        assert a.dtype == np.asarray(p[k]).dtype and np.array_equal(bits(a), bits(p[k])), (N, k, "the recorded inputs are not the draw of seed %d" % SEED)
    d = abi.cbf_desc(N, 1, AB[0], AB[1], alpha=p["alpha"], margin=p["margin"])
    return N, crx.init(), d, args


def _assert_recorded(N, route, got, recorded):
    assert all(len(recorded["N%d/%s" % (N, k)]) == BATCH for k in OUTPUTS), (N, "the recording is not of %d problems" % BATCH)
    bit_pins.assert_recorded(N, route, got, recorded)


def test_shared_model_route_and_what_the_batch_holds(batch, orc, recorded):
    N, gpu, d, args = batch
    ro, n = _oracle_trace(orc, d, args)
    n["restored"] = int((ro["status"] == 3).sum())
    n["no_obstacle"] = int((args[INPUTS.index("n_obs")] == 0).sum())
    print("N = %d, by the oracle: %s" % (N, n))
    for what in ("backtracked", "restart", "restored", "jam_exit", "jam_rerun", "inertia", "no_obstacle"):
        assert n[what] >= 1, (N, what, n)
    rg = gpu.cbf_solve(d, *args)
    _assert_recorded(N, "shared model", rg, recorded)
    assert np.array_equal(rg["status"], ro["status"]), (N, np.nonzero(rg["status"] != ro["status"])[0])
    assert np.array_equal(rg["iters"], ro["iters"]), (N, np.nonzero(rg["iters"] != ro["iters"])[0])


def test_per_problem_models_route(batch, AB, recorded):
    N, gpu, d, args = batch
    _assert_recorded(N, "per-problem models", gpu.cbf_solve(d, *args, models=bit_pins.shipped_models(AB, BATCH)), recorded)


def test_two_wave_route_second_wave_idle(batch, recorded):
    N, gpu, d, args = batch
    _assert_recorded(N, "two-wave unit, second wave idle", bit_pins.solve_two_wave_idle(gpu, d, args), recorded)
