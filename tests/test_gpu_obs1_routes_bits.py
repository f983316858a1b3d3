"""The three routes to the tuned one-obstacle NLP kernels give the same bits on the retry-dense batch of tests/test_gpu_obs1_retry_bits.py.

crx_solve_kernel<1,12,6,12> and <1,12,6,10> are compiled three times: in the obstacle unit (one LTI model per launch: the route the recording of
obs1_retry_bits.npz covers), in the per-problem-model unit (crx_kernels_models_obs.hip) and in the two-wave unit (crx_kernels_spec.hip, opt-in
through the diagnostics switch crx_debug_speculation; mode 2 leaves its second wave idle, which is the one-wave schedule).  A change to
crx_wave.h or to the retry loop of the inertia correction lands in all three, and only the first is pinned by a recording.  Here the batch
synth.cfg2_mpccbf(32, N, seed=127, safe_start=False) is solved through each, with per-problem models that are copies of the shipped model, and
every output of the three is compared with == on the bit patterns.

MEASURED on the MI355X with the library of the parent of the commit that added this test: the per-problem-model route equals the shared-model
launch in every bit at both horizons; the two-wave unit with its second wave idle did NOT -- statuses and iteration counts equal for all 32
problems, but 778 / 285 / 20 / 11 / 21 entries of X / U / sigma / cost / kkt differed at N = 12 (856 / 319 / 19 / 12 / 28 at N = 10), by at most
1e-11 in X and 5e-8 in cost; with the iteration limit at 1 already ~170 entries of X by one ulp.  Cause (crx_kernels.hip, where the kernel forms its
lane index): the two-wave kernel's `threadIdx.x & 63` told the compiler that lane < 64, the one-wave kernel's `threadIdx.x` tells it only that the
lane is not negative.  With lane < 64 the first pass of the coordinate loops lies provably below stage N, sel(k < N, nuv * jv2, 0.0) of
first_order folds to the bare product there, and the product is fused into the subtraction: one rounding for the one-wave kernel's two.  The
two-wave kernel now hands the compiler an opaque lane index that is known to be non-negative and nothing else; all three routes give the same bits.
"""
import numpy as np
import pytest

import bit_pins
from bit_pins import INPUTS, OUTPUTS, bits

pytestmark = pytest.mark.gpu

SEED = 127
BATCH = 32


@pytest.fixture(scope="module", params=[12, 10])
def routes(request, AB):
    """-> (N, gpu, descriptor, arguments, outputs of the shared-model launch): solved once per horizon."""
    import crx
    from crx import abi, synth

    N = request.param
    gpu = crx.init()
    A, B = AB
    p = synth.cfg2_mpccbf(BATCH, N=N, seed=SEED, safe_start=False)
    d = abi.cbf_desc(N, 1, A, B, alpha=p["alpha"], margin=p["margin"])
    args = [p[k] for k in INPUTS]
    shared = gpu.cbf_solve(d, *args)
    assert sorted(shared) == sorted(OUTPUTS)
    assert int(shared["iters"].max()) == {12: 51, 10: 37}[N]   # the batch of the recording
    return N, gpu, d, args, shared


def _assert_same(N, route, got, shared):
    report = []
    for k in OUTPUTS:
        assert got[k].dtype == shared[k].dtype and got[k].shape == shared[k].shape, (route, k)
        diff = np.nonzero(bits(got[k]) != bits(shared[k]))[0]
        worst = float(np.abs(got[k].astype(np.float64) - shared[k].astype(np.float64)).max()) if diff.size else 0.0
        print("N = %d, %s, %s: %d entries differ%s" % (N, route, k, diff.size, "" if diff.size == 0 else ", first at problem %d, largest |difference| %.3e" % (diff[0], worst)))
        if diff.size:
            report.append((k, int(diff.size), int(diff[0])))
    assert not report, (N, route, report)


def test_per_problem_models_route(routes, AB):
    N, gpu, d, args, shared = routes
    _assert_same(N, "per-problem models", gpu.cbf_solve(d, *args, models=bit_pins.shipped_models(AB, BATCH)), shared)


def test_two_wave_route_second_wave_idle(routes):
    N, gpu, d, args, shared = routes
    _assert_same(N, "two-wave unit, second wave idle", bit_pins.solve_two_wave_idle(gpu, d, args), shared)
