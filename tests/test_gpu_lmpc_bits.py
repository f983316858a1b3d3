"""Every output of crx_lmpc_kernel, all six shipped instantiations, bit for bit against a recording.

tests/test_gpu_plain_bits.py does this for crx_solve_kernel; the learning-MPC kernel had only tools/lmpc_ab.py, run by hand on two
libraries.  Work that restates the kernel's passes (one statement of the row map, of the trial slack, of the model roll-out: HISTORY.md,
round 15) or changes how it is scheduled must not change one bit of X, U, lam, cost, status, kkt or iters.  tests/golden/lmpc_bits.npz holds
those outputs for the batches below, recorded on an MI355X (tests/golden/tools/make_lmpc_bits.py) with the library of the commit BEFORE that
work (the parent of the commit that added this test).  The recording is compared with == on the bit patterns, without exceptions.

The inputs are the 47 learning-MPC QPs recorded from the reference's LMPC lap (helpers.lmpc_inputs, tests/golden/racing_game.npz), built into
each case the way test_fuzz_descriptors builds them: stage models idx = minimum(arange(N), 11) (the last one repeated past N = 12), ss / qfun
zero-padded from 44 to n_ss_max columns, n_ss = 44 for every QP, ey_max from lmpc/lap_width.  Each case selects one instantiation
<NMAX, DENSE, MSS, NFIX>.

With all 47 QPs the recording is about 270 KB, over the 256 KB a fixture of this kind may take (the low mantissa bytes of X, U and lam do not
compress), so the cases solve a FIXED SUBSET: the 41 QPs with indices 0..29 and 36..46.  The six left out, 30..35, converge in every case in
10..17 iterations, as their neighbours 26..29 and 36..39 do, which stay; every QP that ends with status 1, 2 or 5 in any case and every long
solve stays.  The oracle's status counts [0..5] and longest / total iteration counts of the subset were measured on the CPU and are asserted on
the oracle by every run, so that a batch stays the one described (in brackets: the same for all 47):

    case             N   n_ss_max  Q                   instantiation       oracle status counts                  longest / total
    fix12            12  44        0                   <12,false,44,12>    32,0,9,0,0,0    [38,0,9,0,0,0]        26 / 647    [26 / 726]
    fix12_noscreen   12  44        0, reach_screen=0   the same; the Farkas certificate where the screen skipped
                                                                           32,0,9,0,0,0    [38,0,9,0,0,0]        26 / 672    [26 / 751]
    n9                9  44        0                   <12,false,44,0>     25,0,16,0,0,0   [31,0,16,0,0,0]       29 / 648    [29 / 731]
    ss60             12  60        0                   <12,false,60,0>     32,0,9,0,0,0    [38,0,9,0,0,0]        26 / 647    [26 / 726]
    n16              16  44        0                   <16,false,60,0>     31,2,7,0,0,1    [37,2,7,0,0,1]        72 / 704    [72 / 788]
    q12              12  44        (1,0,0,.5,0,4)      <12,true,60,0>      29,5,7,0,0,0    [35,5,7,0,0,0]        231 / 1106  [231 / 1193]
    q14              14  44        (1,0,0,.5,0,4)      <16,true,60,0>      25,11,5,0,0,0   [31,11,5,0,0,0]       400 / 1768  [400 / 1860]
    noise            12  44        0                   the 8 QPs of tests/golden/lmpc_noise_floor.npz: no status 0, every solve ended by the
                                                       stagnation rule (<= 80 iterations), as test_lmpc_noise_floor_qps has it

Together: both attempts, the reach screen and the Farkas certificate, the divergence heuristic (status 5), max_iter, the stagnation rule, the
dense and the band Hu, both layout capacities, both horizon classes, the static-LDS instantiation.  295 QPs.

fix12, fix12_noscreen, n9 and ss60 also require the kernel's status to be the oracle's, QP by QP (as test_golden_lmpc does).  n16, q12, q14
and noise do not: long solves may part from the oracle by an iteration, and there the recording is what pins the kernel.

How the fixture holds the bit patterns (the encoding of plain_bits.npz; nothing is lost): an integer output as it is; a float64 output of
shape S as its 64-bit patterns cut into byte planes, uint8 [8, *S].  fix12_noscreen and ss60 solve fix12's QPs again, so for them the planes
are of pattern(case) XOR pattern(fix12), fix12's lam [41, 44] continued with zero patterns to ss60's [41, 60].  recorded_bits() undoes both.
"""
import os

import numpy as np
import pytest

import bit_pins
import conftest
import helpers
from bit_pins import assert_same_bits, bits

pytestmark = pytest.mark.gpu

Q_TRACK = (1.0, 0.0, 0.0, 0.5, 0.0, 4.0)
#        case: (N, n_ss_max, Q, reach_screen, oracle status counts, oracle longest solve, oracle iterations in total)
TABLE = {
    "fix12": (12, 44, None, 1, (32, 0, 9, 0, 0, 0), 26, 647),
    "fix12_noscreen": (12, 44, None, 0, (32, 0, 9, 0, 0, 0), 26, 672),
    "n9": (9, 44, None, 1, (25, 0, 16, 0, 0, 0), 29, 648),
    "ss60": (12, 60, None, 1, (32, 0, 9, 0, 0, 0), 26, 647),
    "n16": (16, 44, None, 1, (31, 2, 7, 0, 0, 1), 72, 704),
    "q12": (12, 44, Q_TRACK, 1, (29, 5, 7, 0, 0, 0), 231, 1106),
    "q14": (14, 44, Q_TRACK, 1, (25, 11, 5, 0, 0, 0), 400, 1768),
}
SUBSET = np.r_[0:30, 36:47]   # of the 47 recorded QPs (module docstring)
CASES = tuple(TABLE) + ("noise",)
SAME_STATUS_AS_ORACLE = ("fix12", "fix12_noscreen", "n9", "ss60")
XOR_BASE = {"fix12_noscreen": "fix12", "ss60": "fix12"}
OUTPUTS = ("U", "X", "cost", "iters", "kkt", "lam", "status")


def solve(binding, case):
    """Every output of `case` from `binding` (the GPU library's or the oracle's)."""
    from crx import abi

    if case == "noise":
        z = np.load(os.path.join(conftest.GOLDEN, "lmpc_noise_floor.npz"), allow_pickle=False)
        return binding.lmpc_solve(abi.lmpc_desc(12, 44), *[z[k] for k in ("x0", "u_old", "A", "B", "C", "ss", "qfun", "n_ss")])
    N, M, Q, screen = TABLE[case][:4]
    g = np.load(os.path.join(conftest.GOLDEN, "racing_game.npz"), allow_pickle=False)
    _, (x, u_old, A, B, C, ss44, qf44) = helpers.lmpc_inputs(g, SUBSET)
    n, M0 = ss44.shape[0], ss44.shape[2]
    ey_max = float(g["lmpc/lap_width"][0])
    d = abi.lmpc_desc(N=N, n_ss_max=M, ey_max=ey_max) if Q is None else abi.lmpc_desc(N=N, n_ss_max=M, ey_max=ey_max, Q=Q)
    d.opts.reach_screen = screen
    idx = np.minimum(np.arange(N), A.shape[1] - 1)
    ss, qf = np.zeros((n, 6, M)), np.zeros((n, M))
    ss[:, :, :M0], qf[:, :M0] = ss44, qf44
    return binding.lmpc_solve(d, x, u_old, A[:, idx], B[:, idx], C[:, idx], ss, qf, np.full(n, M0, np.int32))


def xor_base(case, k, of):
    """The pattern XORed into the planes of float64 output `k` of `case`: that of XOR_BASE[case] (of(case, k) -> its uint64 pattern), continued with
    zeros along the last axis to this case's width; None for a case that has no base."""
    if case not in XOR_BASE:
        return None
    b = of(XOR_BASE[case], k)
    width = (of(case, k).shape[-1] if b.ndim else 0) - (b.shape[-1] if b.ndim else 0)
    return np.pad(b, [(0, 0)] * (b.ndim - 1) + [(0, width)]) if width else b


def recorded_bits(z, case, k):
    """The recorded bit patterns of output `k` of `case` (the encoding: module docstring)."""
    a = z[case + "/" + k]
    if a.dtype != np.uint8:
        return a
    b = bit_pins.unplanes(a)
    base = xor_base(case, k, lambda c, kk: b if c == case else recorded_bits(z, c, kk))
    return b if base is None else b ^ base


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(conftest.GOLDEN, "lmpc_bits.npz"), allow_pickle=False)


@pytest.mark.parametrize("case", CASES)
def test_lmpc_outputs_bit_for_bit(orc, recorded, case):
    import crx

    gpu = crx.init()
    rg, ro = solve(gpu, case), solve(orc, case)
    # the batch is the one the docstring describes
    counts, longest, total = np.bincount(ro["status"], minlength=6).tolist(), int(ro["iters"].max()), int(ro["iters"].sum())
    print(case, "oracle: status counts", counts, "longest", longest, "total", total)
    if case == "noise":
        assert ro["status"].size == 8 and counts[0] == 0 and longest <= 80
    else:
        assert ro["status"].size == SUBSET.size == 41 and (tuple(counts), longest, total) == TABLE[case][4:]
    assert sorted(rg) == list(OUTPUTS) == sorted(k[len(case) + 1:] for k in recorded.files if k.startswith(case + "/"))
    for k in OUTPUTS:
        assert_same_bits(case, k, bits(np.asarray(rg[k])), recorded_bits(recorded, case, k))
    if case in SAME_STATUS_AS_ORACLE:
        assert np.array_equal(rg["status"], ro["status"]), (case, np.nonzero(rg["status"] != ro["status"])[0])
