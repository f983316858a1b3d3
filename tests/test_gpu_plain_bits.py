"""The plain forms of the interior-point passes of crx_solve_kernel, bit for bit against a recording.

tests/test_gpu_obs1_bits.py and test_gpu_obs1_retry_bits.py pin crx_solve_kernel<1,12,6,{12,10}> only: the instantiations that run the
"loads first" form of the two-pass phases.  Every other instantiation runs the plain form of the same phases, and the planner
instantiations run the predictor-corrector arm and the certificate exit besides.  Work that restates those passes (one statement of a
pass's operands and arithmetic for both forms: HISTORY.md, round 13) must not change one bit of any output there either.
tests/golden/plain_bits.npz holds every output of the solve for the batches below, recorded on an MI355X with the library of the commit
BEFORE that work (the parent of the commit that added this test).  The recording is compared with == on the bit patterns, without
exceptions.

The batches are small and still reach the side paths; each was checked with the oracle (status counts, iteration counts and, from
crx_oracle_set_verbose(1), the "RESTART" lines and the delta_w of every iteration), and the test asserts those facts again so that a
batch stays the one described:

    plan12/q0, plan12/q1    synth.cfg3_planner(32, 12, seed=3), qp_method 0 and 1: 128 region QPs, 81 converge and 47 are proved infeasible
    plan10/q0, plan10/q1    the same at N = 10 (81 and 47 again): the certificate exit, the predictor-corrector arm (qp_method 0) and the
                            plain line-search arm (qp_method 1) of the planner instantiations
    cfg4                    synth.cfg4_tracking_cbf(32, N=20, seed=26, safe_start=False), the descriptor of tools/cbf_ab.py: the tuned
                            three-obstacle kernel <3,20,6,20>.  31 converge, 1 ends restored, the longest solve takes 98 iterations, one
                            restart from the crash point, iterations with a non-zero delta_w
    gen11                   synth.cfg2_mpccbf(32, N=11, seed=47, safe_start=False): N = 11 has no tuned instantiation, so the general
                            unit (run-time horizon) serves it.  All 32 converge, the longest solve takes 58 iterations, one restart,
                            iterations with a non-zero delta_w

How the fixture holds the bit patterns (to stay under 256 KB; nothing is lost): an integer output as it is; a float64 output of shape S as
its 64-bit patterns cut into byte planes, uint8 [8, *S] (byte i of every value together, so that signs and exponents compress); and for the
q1 planner cases the planes are of pattern(q1) XOR pattern(q0) -- the same QPs solved by the other method, equal in their leading bits.
recorded_bits() undoes both.

The planner cases also require the kernel's status to be the oracle's, QP by QP.  cfg4 and gen11 do not: long solves through the crash path
are where kernel and oracle may part by an iteration, and the recording is what pins the kernel there.
"""
import os

import numpy as np
import pytest

import bit_pins
import conftest
from bit_pins import INPUTS, assert_same_bits, bits

pytestmark = pytest.mark.gpu

CASES = ("plan12/q0", "plan12/q1", "plan10/q0", "plan10/q1", "cfg4", "gen11")


def solve(binding, AB, case):
    """Every output of `case` from `binding` (the GPU library's or the oracle's)."""
    from crx import abi, synth

    A, B = AB
    if case.startswith("plan"):
        N, qm = int(case[4:6]), int(case[-1])
        p = synth.cfg3_planner(32, N, seed=3)
        d = abi.planner_desc(N, A, B)
        d.opts.qp_method = qm
        return binding.planner_solve(d, *[p[k] for k in ("x0", "bez_s", "bez_ey", "ey_lb", "ey_ub")])
    if case == "cfg4":
        p = synth.cfg4_tracking_cbf(32, N=20, seed=26, safe_start=False)
        d = abi.cbf_desc(20, 3, A, B, alpha=0.6, margin=0.15, Q=(10.0, 0, 0, 5.0, 0, 50.0), per_stage_target=True)
    else:
        p = synth.cfg2_mpccbf(32, N=11, seed=47, safe_start=False)
        d = abi.cbf_desc(11, 1, A, B, alpha=p["alpha"], margin=p["margin"])
    return binding.cbf_solve(d, *[p[k] for k in INPUTS])


def oracle_verbose(orc, AB, case):
    """The oracle's outputs for `case` with what its per-iteration trace (stderr) says: (outputs, restarts, iterations with delta_w != 0)."""
    r, text = bit_pins.oracle_stderr(orc, lambda: solve(orc, AB, case))
    return r, text.count("RESTART"), bit_pins.nonzero_dw(text)


def recorded_bits(z, case, k):
    """The recorded bit patterns of output `k` of `case` (the encoding: module docstring)."""
    a = z[case + "/" + k]
    if a.dtype != np.uint8:
        return a
    b = bit_pins.unplanes(a)
    return b ^ recorded_bits(z, case.replace("q1", "q0"), k) if case.endswith("q1") else b


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(conftest.GOLDEN, "plain_bits.npz"), allow_pickle=False)


@pytest.mark.parametrize("case", CASES)
def test_plain_outputs_bit_for_bit(orc, AB, recorded, case):
    import crx

    gpu = crx.init()
    rg = solve(gpu, AB, case)
    # the batch is the one the docstring describes
    if case.startswith("plan"):
        ro = solve(orc, AB, case)
        assert ro["status"].size == 128 and (ro["status"] == 0).sum() == 81 and (ro["status"] == 2).sum() == 47
    else:
        ro, restarts, nonzero_dw = oracle_verbose(orc, AB, case)
        print(case, "oracle: restarts", restarts, "iterations with delta_w != 0", nonzero_dw, "longest", int(ro["iters"].max()))
        assert restarts >= 1 and nonzero_dw >= 1
        if case == "cfg4":
            assert (ro["status"] == 0).sum() == 31 and (ro["status"] == 3).sum() == 1 and int(ro["iters"].max()) == 98
        else:
            assert (ro["status"] == 0).all() and ro["status"].size == 32 and int(ro["iters"].max()) == 58
    names = sorted(k[len(case) + 1:] for k in recorded.files if k.startswith(case + "/"))
    assert sorted(rg) == names
    for k in names:
        assert_same_bits(case, k, bits(np.asarray(rg[k])), recorded_bits(recorded, case, k))
    if case.startswith("plan"):
        assert np.array_equal(rg["status"], ro["status"]), (case, np.nonzero(rg["status"] != ro["status"])[0])
