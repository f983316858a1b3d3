"""The wave reductions of csrc/crx_wave.h compile without two compiler artefacts (no GPU: the probe is compiled to gfx950 assembly and read).

A lone wave pays per instruction issued, and every interior-point iteration runs eight row reductions, so what the compiler adds to a butterfly
step is paid 32 times per iteration:

  * a DPP move whose `old` operand is tied to its source (`update_dpp(x, x, ..)`) has destination = source, and since the source is still live --
    it is the other operand of the OP -- the compiler copies it first: two v_mov_b32 per step.  Seen here as `v_mov_b32_dpp vN, vN`.
  * fmax / fmin of operands that came through integer DPP moves, v_permlane*_swap or v_readlane get a canonicalising `v_max_f64 x, x, x` each.

The probe holds one kernel per reduction primitive (the scans are not reductions: `v = dpp_zfill(v)` may well keep its register).
"""
import os
import re
import shutil
import subprocess

import pytest

import conftest

CSRC = os.path.join(conftest.PKG, "csrc")
PROBE = r"""
#include "crx_wave.h"
#define K(name, body) extern "C" __global__ void __launch_bounds__(WAVE) name(const double* in, double* out) { \
    const int lane = threadIdx.x; double a = in[lane], b = in[64 + lane], c = in[128 + lane], d = in[192 + lane]; (void)b; (void)c; (void)d; body }
K(probe_wave_sum, out[lane] = wave_sum(a);)
K(probe_wave_prod, out[lane] = wave_prod(a);)
K(probe_wave_max, out[lane] = wave_max(a);)
K(probe_wave_min, out[lane] = wave_min(a);)
K(probe_wave_sum2, wave_sum2(a, b); out[lane] = a; out[64 + lane] = b;)
K(probe_wave_max2, wave_max2(a, b); out[lane] = a; out[64 + lane] = b;)
K(probe_wave_sum4, wave_sum4(a, b, c, d); out[lane] = a; out[64 + lane] = b; out[128 + lane] = c; out[192 + lane] = d;)
K(probe_wave_max4, wave_max4(a, b, c, d); out[lane] = a; out[64 + lane] = b; out[128 + lane] = c; out[192 + lane] = d;)
K(probe_row_max, ROW_REDUCE(a, op_max) out[lane] = a;)
K(probe_row_min, ROW_REDUCE(a, op_min) out[lane] = a;)
K(probe_logacc_total, LogAcc l; l.mul(a); l.mul(b); out[lane] = l.wave_total();)
K(probe_logacc_total_with, LogAcc l; l.mul(a); out[lane] = l.wave_total_with(b); out[64 + lane] = b;)
"""
KERNELS = re.findall(r"K\((probe_\w+),", PROBE)


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    """{kernel: [instruction lines]} of the probe, compiled as the library's units are (-O3, gfx950)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc is not installed: the probe cannot be compiled here")
    tmp = tmp_path_factory.mktemp("wave_asm")
    src, out = tmp / "probe.hip", tmp / "probe.s"
    src.write_text(PROBE)
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I", CSRC, str(src), "-o", str(out)],
                   check=True, capture_output=True, text=True)
    kernels, cur = {}, None
    for line in out.read_text().splitlines():
        m = re.match(r"(probe_\w+):", line)
        if m:
            cur = kernels.setdefault(m.group(1), [])
        elif cur is not None and re.match(r"\s+[sv]_\w+|\s+(global|ds|flat)_\w+", line):
            cur.append(line.split(";")[0].strip())
            if cur[-1].startswith("s_endpgm"):
                cur = None
    assert sorted(kernels) == sorted(KERNELS), sorted(kernels)
    return kernels


def test_no_canonicalising_self_max(asm):
    """No v_max_f64 / v_min_f64 with three identical operands: the max / min reductions are the bare instruction (op_max / op_min)."""
    bad, seen = [], 0
    for k, lines in asm.items():
        for ins in lines:
            m = re.match(r"v_(?:max|min)_f64(?:_e64)?\s+(\S+),\s*(\S+),\s*(\S+)$", ins)
            if m:
                seen += 1
                if m.group(1) == m.group(2) == m.group(3):
                    bad.append((k, ins))
    assert seen >= 4 * 7, seen   # the probe did compile max / min reductions: seven row reductions of four steps at the least
    assert not bad, bad


def test_no_dpp_move_onto_its_source(asm):
    """No v_mov_b32_dpp with destination = source: dpp_f64 has no tied `old` operand."""
    bad, seen = [], 0
    for k, lines in asm.items():
        for ins in lines:
            m = re.match(r"v_mov_b32_dpp\s+(\w+),\s*(\w+)\s", ins)
            if m:
                seen += 1
                if m.group(1) == m.group(2):
                    bad.append((k, ins))
    assert seen >= 8 * len(KERNELS), seen   # four steps of two moves in every kernel
    assert not bad, bad
