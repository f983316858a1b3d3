"""Register, scratch and LDS budget of the tuned one-obstacle NLP kernels, read from the library that SHIPS (no GPU, no recompilation).

crx_solve_kernel<1,12,6,12> (the headline of bench.py) and <1,12,6,10> run one wave per problem at two waves per SIMD; what they may use is
DESIGN.md 5.1: at most 248 VGPRs (at 253 the register allocator of this toolchain crashes on the two-wave instantiation of the same source, so
the budget keeps the next change away from that wall), no scratch, 20 432 B of LDS (eight problems per CU), and no more SGPRs spilled into VGPR
lanes than profiles/r08_census.txt records for the instantiation.  tools/kernel_resources.py reads the figures from the metadata notes of the
code objects embedded in libcrx.so.

As shipped by the commit that added this test: <1,12,6,12> 248 VGPRs (its parent: 251), 134 SGPR spills (250), scratch 0, LDS 20 432 B;
<1,12,6,10> 236 VGPRs (240), 161 SGPR spills (266), scratch 0, LDS 20 432 B.  Of the 248, two carry spilled SGPRs in their lanes (the parent
needed three: crash_search indexed the descriptor's A and B with constants, which parks both matrices in SGPRs at once; it now reads them back from
LDS); the other 246 are the peak of the unrolled Riccati sweep.  Compiled alone (tools/kernel_resources.py one 1 12 6 12) the kernel takes two
registers fewer than in its translation unit: the budget is about what ships.
"""
import os
import re
import sys

import pytest

import conftest

sys.path.insert(0, os.path.join(conftest.ROOT, "tools"))


@pytest.fixture(scope="module")
def shipped():
    import kernel_resources as kr

    if not os.path.exists(kr.READELF):
        pytest.skip("ROCm binutils (%s) not installed: the shipped code objects cannot be read here" % kr.READELF)
    return kr.shipped(os.path.join(conftest.PKG, "crx", "libcrx.so"))


def _recorded_spills(nfix):
    txt = open(os.path.join(conftest.ROOT, "profiles", "r08_census.txt")).read()
    m = re.search(r"crx_solve_kernel<1,12,6,%d>\s+production build:.*?\.sgpr_spill_count: (\d+)" % nfix, txt)
    assert m, "profiles/r08_census.txt has no production line for <1,12,6,%d>" % nfix
    return int(m.group(1))


@pytest.mark.parametrize("nfix", [12, 10])
def test_obs1_kernel_budget(shipped, nfix):
    name = "_Z16crx_solve_kernelILi1ELi12ELi6ELi%dELi0ELi0EEv11crx_kparams" % nfix
    assert name in shipped, sorted(shipped)[:5]
    r = shipped[name]
    print(name, r)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
    assert r["lds"] == 20432, r
    assert r["sgpr_spill"] <= _recorded_spills(nfix), (r, _recorded_spills(nfix))
    assert r["vgpr"] <= 248, r
