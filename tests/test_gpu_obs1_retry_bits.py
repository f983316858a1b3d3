"""The inertia-correction retries and the accept step of crx_solve_kernel<1,12,6,12> and <1,12,6,10>, bit for bit against a recording.

The accept step takes the CBF row values of the accepted line-search trial instead of evaluating them again (crx_kernels.hip, the loads-first
form), and work on the retry loop of the inertia correction (one set-up of the backward sweep per Newton system: HISTORY.md, round 9) goes through
the same paths.  Neither may change one bit of any output.  (The A/B switches of the two, CRX_CBF_CARRY and CRX_RETRY_SHARED, are retired; this
test is the standing pin of that code.)  tests/golden/obs1_retry_bits.npz holds every output of crx_cbf_solve for the batch
below (X, U, sigma, cost, status, kkt, iters; N = 12 and N = 10), recorded on an MI355X with the library of the commit BEFORE the change (the
parent of the commit that added this test).  The recording is compared with == on the bit patterns, and status and iteration counts are
compared with the oracle's, problem by problem, without exceptions.

The batch: synth.cfg2_mpccbf(32, N, seed=127, safe_start=False) -- one obstacle, no scenario filter.  Seeds were searched upwards from 0 with the
oracle for the first batch in which BOTH horizons hold every path such work touches, and hold them densely; 127 is the first:

                                                                                  N = 12   N = 10
    Newton systems that climb the cold schedule (dw_last = 0: 1e-4, 1e-2, ..)
        to delta_w >= 1   (0, 1e-4 and 1e-2 failed)                                    5        5
        to delta_w >= 100 (1 failed as well)                                           4        4
    Newton systems on the warm schedule (dw_last / 3, x 8)                            27       14
    convexified retries on the crash path (the exact matrix failed first)              3        7
    iterations that start convexified (the sticky rule: no retry)                      6       19
    restarts from the crash point                                                      1        1
    iterations whose accepted alpha is below the first trial's (backtracking)         77       76

(counted from crx_oracle_set_verbose(1): the delta_w and dw_last of every iteration, its a_p and accepted alpha, and the "RESTART" lines; the
convexified retries with a build of oracle/crx_oracle.c that prints a line where it takes that retry -- the shipped oracle reports it as
delta_w = 0).  The longest solve takes 51 (N = 12) and 37 (N = 10) iterations; one problem of N = 12 ends at the iteration limit and one of
N = 10 restored, the other 31 converge.
"""
import os

import numpy as np
import pytest

import conftest
from bit_pins import INPUTS, OUTPUTS, assert_same_bits, bits

pytestmark = pytest.mark.gpu

SEED = 127
BATCH = 32


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(conftest.GOLDEN, "obs1_retry_bits.npz"), allow_pickle=False)


@pytest.mark.parametrize("N", [12, 10])
def test_obs1_retry_outputs_bit_for_bit(orc, AB, recorded, N):
    import crx
    from crx import abi, synth

    gpu = crx.init()
    A, B = AB
    p = synth.cfg2_mpccbf(BATCH, N=N, seed=SEED, safe_start=False)
    d = abi.cbf_desc(N, 1, A, B, alpha=p["alpha"], margin=p["margin"])
    args = [p[k] for k in INPUTS]
    rg, ro = gpu.cbf_solve(d, *args), orc.cbf_solve(d, *args)
    assert sorted(rg) == sorted(OUTPUTS)
    # the batch is the one the docstring describes
    assert (ro["status"] == 0).sum() == 31 and int(ro["iters"].max()) == {12: 51, 10: 37}[N]
    for k in OUTPUTS:
        want = recorded["N%d/%s" % (N, k)]
        assert rg[k].dtype == want.dtype and rg[k].shape == want.shape, k
        assert_same_bits(N, k, bits(rg[k]), bits(want))
    assert np.array_equal(rg["status"], ro["status"]), (N, np.nonzero(rg["status"] != ro["status"])[0])
    assert np.array_equal(rg["iters"], ro["iters"]), (N, np.nonzero(rg["iters"] != ro["iters"])[0])
