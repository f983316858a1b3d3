"""The one-obstacle NLP kernels crx_solve_kernel<1,12,6,12> and <1,12,6,10>, bit for bit against a recording.

Work on these kernels that only moves instructions (which pass loads when, what lives in which register file) must not change one
bit of any output.  tests/golden/obs1_bits.npz holds every output of crx_cbf_solve for the batch below (X, U, sigma, cost, status,
kkt, iters; N = 12 and N = 10), recorded on an MI355X with the library of the commit BEFORE the row passes were reordered (the
parent of the commit that added this test).  The recording is compared with == on the bit patterns, and status and iteration
counts are compared with the oracle's, problem by problem, without exceptions.  (The A/B switch of that reordering, CRX_LOADS_FIRST, is
retired: the reordered passes are the loads-first form of crx_kernels.hip, and this test is the standing pin of that code.)

The batch: synth.cfg2_mpccbf(64, N, seed=161, safe_start=False) -- one obstacle, no scenario filter.  Seeds were searched upwards from 0 for a batch in
which, by the oracle, BOTH horizons hold every path the kernel has beside the healthy iteration: 67 is the first (its longest solve
takes 81 iterations), 161 the second and the one used:

                                                           N = 12   N = 10
    restarts from the crash point                               1        1
    iterations with a non-zero delta_w                         22       16
    convexified retries (crash path)                           32       28
    problems that end restored (status 3, CRX_RESTORED)         1        1

(counted from crx_oracle_set_verbose(1): the "RESTART" lines and the delta_w of every iteration; the convexified retries with a build
of oracle/crx_oracle.c that prints a line where it takes that retry -- the shipped oracle reports it as delta_w = 0).  The longest
solve takes 34 (N = 12) and 33 (N = 10) iterations.
"""
import os

import numpy as np
import pytest

import conftest
from bit_pins import INPUTS, OUTPUTS, assert_same_bits, bits

pytestmark = pytest.mark.gpu

SEED = 161


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(conftest.GOLDEN, "obs1_bits.npz"), allow_pickle=False)


@pytest.mark.parametrize("N", [12, 10])
def test_obs1_outputs_bit_for_bit(orc, AB, recorded, N):
    import crx
    from crx import abi, synth

    gpu = crx.init()
    A, B = AB
    p = synth.cfg2_mpccbf(64, N=N, seed=SEED, safe_start=False)
    d = abi.cbf_desc(N, 1, A, B, alpha=p["alpha"], margin=p["margin"])
    args = [p[k] for k in INPUTS]
    rg, ro = gpu.cbf_solve(d, *args), orc.cbf_solve(d, *args)
    assert sorted(rg) == sorted(OUTPUTS)
    # the batch is the one the docstring describes: a restored verdict among converged ones
    assert (ro["status"] == 3).sum() == 1 and (ro["status"] == 0).sum() == 63
    for k in OUTPUTS:
        want = recorded["N%d/%s" % (N, k)]
        assert rg[k].dtype == want.dtype and rg[k].shape == want.shape, k
        assert_same_bits(N, k, bits(rg[k]), bits(want))
    assert np.array_equal(rg["status"], ro["status"]), (N, np.nonzero(rg["status"] != ro["status"])[0])
    assert np.array_equal(rg["iters"], ro["iters"]), (N, np.nonzero(rg["iters"] != ro["iters"])[0])
