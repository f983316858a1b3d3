"""Instruction count of the unrolled Riccati sweep of crx_solve_kernel<1,12,6,12> (the headline of bench.py), from the sources (no GPU).

A lone solver wave pays one issue slot per instruction whatever its class, so the static census of tools/asm_census.py IS the cost
model of an iteration.  Round 20 took the integer address arithmetic of the feedback stores out of every stage of the sweep (one record per stage
and input at a compile-time offset: Lay::KR); profiles/r20_census.txt records the census of that commit in its section "==== new".  This test
runs the census again and asserts that neither the iteration (first to last clock read) nor the `factor + update` phase of any stage has more
instructions than recorded: address arithmetic that creeps back into the stages shows here, before anybody has to measure it.

Compiles the instantiation twice (production and phase-clock build): about a minute.  Skips where hipcc is not installed.
"""
import os
import re
import subprocess
import sys

import pytest

import conftest

TOOLS = os.path.join(conftest.ROOT, "tools")


def figures(text):
    """(instructions of the iteration, largest `factor + update` of a stage) of the first census of <1,12,6,12> in `text`."""
    m = re.search(r"^crx_solve_kernel<1,12,6,12>.*?^iteration, first to last clock read\s+(\d+)", text, re.S | re.M)
    assert m, "no census of <1,12,6,12>"
    stages = [int(v) for v in re.findall(r"^ric N-\d+: factor \+ update\s+(\d+)", m.group(0), re.M)]
    assert len(stages) == 12, stages
    return int(m.group(1)), max(stages)


def test_sweep_census_not_above_the_record():
    sys.path.insert(0, TOOLS)
    import recipe

    hipcc = recipe.recipe()[0]
    if not hipcc or not os.path.exists(hipcc):
        pytest.skip("hipcc (%s) not installed: the instantiation cannot be compiled here" % hipcc)
    txt = open(os.path.join(conftest.ROOT, "profiles", "r20_census.txt")).read()
    assert txt.count("\n==== new\n") == 1
    rec_iter, rec_stage = figures(txt.split("\n==== new\n", 1)[1])
    out = subprocess.run([sys.executable, os.path.join(TOOLS, "asm_census.py"), "1", "12", "6", "12"], capture_output=True, text=True, check=True).stdout
    now_iter, now_stage = figures(out)
    print("iteration %d (recorded %d), largest factor + update of a stage %d (recorded %d)" % (now_iter, rec_iter, now_stage, rec_stage))
    assert rec_stage <= 65, rec_stage   # (what the round set itself: HISTORY.md, round 20)
    assert now_iter <= rec_iter and now_stage <= rec_stage
