"""The Riccati feedback gains moved in LDS (one block per stage at a fixed offset, Lay::KS; HISTORY.md, round 20): bit for bit against a recording.

Moving the gains changes where numbers are stored and nothing that is computed, in EVERY instantiation of the solver source.  The recordings of
tests/test_gpu_obs1_bits.py, test_gpu_obs1_retry_bits.py, test_gpu_obs1_routes_bits.py and test_gpu_plain_bits.py pin <1,12,6,{12,10}>, the planner
kernels, <3,20,6,20> and the general one-obstacle kernel at N = 11.  tests/golden/feedback_layout_bits.npz holds every output of the solve for five
more batches of 16 problems, one per layout class and kernel form that no recording pinned, recorded on an MI355X with the library of the commit
BEFORE the move (the parent of the commit that added this test), and compared with == on the bit patterns, without exceptions:

    obs2n10     synth.cfg2_mpccbf(16, N=10, n_obs=2, safe_start=False): crx_solve_kernel<2,12,6,10>, where H lies over dZ and the gains follow (P | p | T);
                NX = 8 is even: K rows on their own stride, then kff (a lane of the update pass keeps NU store bases)
    obs3n12     the same at N = 12 with three obstacles: <3,12,6,12>, the one class whose H does not fit dZ (the gains follow H); NX = 9: records
    obs1n20     N = 20, one obstacle: the tuned class-24 kernel <1,24,6,20> (twenty unrolled stages, (P | p) in registers); NX = 7: records
    gen5n7      N = 7, five obstacles: the generic six-slot kernel of the general unit (NX = 12), whose update phase takes TWO passes over the
                lanes (the second pass holds the feedback columns and 25 lanes that own no entry of the map)
    gen1n3      N = 3, one obstacle: the general unit at the smallest horizon the descriptor check accepts -- three blocks in all, where a
                store that leaves its block lands in another array at once

Every lane of the update pass stores the feedback column it carries (lanes that own no entry of the lane map carry column 0, same bits as the column's
own lane); a lane that stored anything else, or anywhere else, would show here as a changed iterate.  The seeds were chosen with the oracle so that
every batch holds converged solves and iterations with a non-zero delta_w (inertia retries: a sweep that breaks off and is repeated); the test asserts
both again, the first from the recording, the second from the oracle's trace, so that a batch stays the one described.

The fixture holds a float64 output of shape S as its 64-bit patterns cut into byte planes, uint8 [8, *S], and an integer output as it is (the
format of plain_bits.npz).
"""
import os

import numpy as np
import pytest

import bit_pins
import conftest
from bit_pins import INPUTS, assert_same_bits, bits

pytestmark = pytest.mark.gpu

# case -> (horizon, obstacle slots, seed of the draw)
CASES = {
    "obs2n10": (10, 2, 1),
    "obs3n12": (12, 3, 1),
    "obs1n20": (20, 1, 1),
    "gen5n7": (7, 5, 1),
    "gen1n3": (3, 1, 161),   # (three draws in 3000 have an iteration with delta_w != 0 at this horizon: 104, 161, 931)
}
BATCH = 16


def solve(binding, AB, case, seed=None):
    """Every output of `case` from `binding` (the GPU library's or the oracle's)."""
    from crx import abi, synth

    A, B = AB
    N, n_obs, s = CASES[case]
    p = synth.cfg2_mpccbf(BATCH, N=N, seed=s if seed is None else seed, n_obs=n_obs, safe_start=False)
    d = abi.cbf_desc(N, n_obs, A, B, alpha=p["alpha"], margin=p["margin"])
    return binding.cbf_solve(d, *[p[k] for k in INPUTS])


def oracle_nonzero_dw(orc, AB, case, seed=None):
    """(the oracle's outputs for `case`, the number of its iterations with delta_w != 0), the latter from its per-iteration trace (stderr)."""
    r, text = bit_pins.oracle_stderr(orc, lambda: solve(orc, AB, case, seed))
    return r, bit_pins.nonzero_dw(text)


def planes(a):
    """The fixture's form of output `a` (module docstring)."""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float64:
        return a
    return bit_pins.planes(a.view(np.uint64))


def recorded_bits(z, case, k):
    a = z[case + "/" + k]
    if a.dtype != np.uint8:
        return a
    return bit_pins.unplanes(a)


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(conftest.GOLDEN, "feedback_layout_bits.npz"), allow_pickle=False)


@pytest.mark.parametrize("case", sorted(CASES))
def test_outputs_bit_for_bit(orc, AB, recorded, case):
    import crx

    gpu = crx.init()
    rg = solve(gpu, AB, case)
    # the batch is the one the docstring describes
    status = recorded_bits(recorded, case, "status")
    ro, nonzero_dw = oracle_nonzero_dw(orc, AB, case)
    print(case, "recorded: converged", int((status == 0).sum()), "of", status.size, "longest", int(recorded_bits(recorded, case, "iters").max()),
          "| oracle: converged", int((ro["status"] == 0).sum()), "iterations with delta_w != 0", nonzero_dw)
    assert status.size == BATCH and (status == 0).sum() >= 1
    assert nonzero_dw >= 1
    names = sorted(k[len(case) + 1:] for k in recorded.files if k.startswith(case + "/"))
    assert sorted(rg) == names
    for k in names:
        assert_same_bits(case, k, bits(np.asarray(rg[k])), recorded_bits(recorded, case, k))
