"""The build recipe of libcrx is ONE table (car-racing_amd/csrc/Makefile), and an A/B library built from it is whole.  No GPU.

Every object of the library appears once in the Makefile with its source and its unit flags; `make recipe` prints the table and tools/recipe.py
reads it.  Part one: the table names real files, no *.hip stands outside it, the tools that recompile a unit take source and flags from it and keep
no copy of the scheduler / MachineLICM flags.  Part two: `make variant` (tools/build_variant.sh) compiles one unit differently and links it with
the in-tree objects of EVERY other unit -- the library loads, exports what the in-tree library exports, holds the same kernels, and the in-tree
objects are not touched.  (A variant script with an object list of its own once linked 8 of 16 objects: undefined symbols at load time, unnoticed.)
"""
import glob
import os
import re
import shutil
import subprocess
import sys

import pytest

import conftest

TOOLS = os.path.join(conftest.ROOT, "tools")
CSRC = os.path.join(conftest.PKG, "csrc")
sys.path.insert(0, TOOLS)


@pytest.fixture(scope="module")
def table():
    if shutil.which("make") is None:
        pytest.skip("make is not installed: the recipe cannot be printed")
    import recipe

    hipcc, tab = recipe.recipe()
    assert hipcc and len(tab) >= 16, (hipcc, sorted(tab))
    return hipcc, tab


def test_recipe_sources_exist_and_cover_csrc(table):
    _, tab = table
    sources = {src for src, _ in tab.values()}
    for src in sources:
        assert os.path.isfile(os.path.join(CSRC, src)), src
    # every *.hip of csrc is compiled by the recipe, or is crx_kernels.hip, which the solver units include: no other *.hip is included by anything
    # (kernel text with two instantiations lives in a header: crx_plant_step.h, crx_path_qp.h)
    included = set()
    for f in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")):
        included |= set(re.findall(r'^\s*#\s*include\s+"([^"]+\.hip)"', open(f).read(), re.M))
    assert included == {"crx_kernels.hip"}, sorted(included)
    stray = sorted(os.path.basename(f) for f in glob.glob(os.path.join(CSRC, "*.hip")) if os.path.basename(f) not in sources | included)
    assert not stray, stray
    # the link line: twenty objects, each from a source of its own
    linked = [o for o in tab if "_one_" not in o]
    assert len(linked) == 20 and len({tab[o][0] for o in linked}) == 20, linked


def test_kernel_resources_compiles_what_the_recipe_states(table):
    import kernel_resources as kr

    hipcc, tab = table
    for name, obj in kr.UNITS.items():
        assert obj in tab, (name, obj)
        src, flags = tab[obj]
        assert kr.unit_command(name, ["-DX=1"]) == [hipcc] + flags + ["-DX=1", os.path.join(CSRC, src)], name
    # `one`: crx_kernels_one.hip, built as the unit that ships the instantiation is built
    for nobs, probe, unit in (("1", "crx_kernels_one_obs.o", "crx_kernels_obs.o"), ("0", "crx_kernels_one_plan.o", "crx_kernels.o")):
        src, flags = tab[probe]
        assert src == "crx_kernels_one.hip" and flags == tab[unit][1], (probe, flags, tab[unit][1])
        assert kr.unit_command("one", [nobs, "12", "6", "12"]) == [hipcc] + flags + ["-DCRX_PROBE_ONE=%s,12,6,12" % nobs, os.path.join(CSRC, src)]


def test_tools_keep_no_copy_of_the_unit_flags():
    hits = []
    for f in sorted(glob.glob(os.path.join(TOOLS, "*.py")) + glob.glob(os.path.join(TOOLS, "*.sh"))):
        txt = open(f).read()
        hits += [(os.path.basename(f), w) for w in ("amdgpu-sched-strategy", "disable-machine-licm") if w in txt]
    assert not hits, hits


def test_kernel_diff_tells_moved_from_differs():
    """A kernel at another place of its code object differs in the descriptor's entry offset (bytes 16..23) and in nothing else: `moved`."""
    import kernel_diff as kd

    text, meta = b"\x01\x02\x03\x04", [".name: k", ".vgpr_count: 7"]
    desc = bytes(range(64))
    moved = desc[:16] + (0x1234).to_bytes(8, "little") + desc[24:]
    assert kd.verdict_of((text, desc, meta), (text, desc, list(meta))) == "same"
    assert kd.verdict_of((text, desc, meta), (text, moved, meta)) == "moved"
    assert kd.verdict_of((text, desc, meta), (text, moved[:48] + b"\xff" + moved[49:], meta)) == "differs (kd)"      # a resource word as well
    assert kd.verdict_of((text, desc, meta), (text + b"\x00", moved, meta)) == "differs (text, kd)"
    assert kd.verdict_of((text, desc, meta), (text, moved, meta[:1])) == "differs (kd, meta)"
    assert kd.verdict_of((text, desc, None), (text, desc, None)) == "differs (meta)"                                # no metadata entry: not comparable


def test_kernel_diff_tells_renamed_from_differs():
    """Other .text bytes under the same mnemonic at every position, with descriptor (but for the entry offset) and metadata equal: `renamed`."""
    import kernel_diff as kd

    meta, desc = [".name: k", ".vgpr_count: 7"], bytes(range(64))
    moved = desc[:16] + (0x1234).to_bytes(8, "little") + desc[24:]
    mn = ["s_load_dword", "v_mov_b32_e32", "v_fma_f64", "s_endpgm"]
    old = (b"\x01\x02\x03\x04", desc, meta, mn)
    assert kd.verdict_of(old, (b"\x01\x02\x03\x05", desc, meta, list(mn))) == "renamed"
    assert kd.verdict_of(old, (b"\x01\x02\x03\x05", moved, meta, list(mn))) == "renamed"
    assert kd.verdict_of(old, (b"\x01\x02\x03\x05", desc, meta, [mn[0], mn[2], mn[1], mn[3]])) == "differs (text)"       # the same instructions in another order
    assert kd.verdict_of(old, (b"\x01\x02\x03\x05", desc, meta, mn + ["s_nop"])) == "differs (text)"
    assert kd.verdict_of(old, (b"\x01\x02\x03\x05", desc, meta[:1], list(mn))) == "differs (text, meta)"                  # a resource changed
    assert kd.verdict_of(old, (b"\x01\x02\x03\x05", desc[:48] + b"\xff" + desc[49:], meta, list(mn))) == "differs (text, kd)"
    assert kd.verdict_of(old[:3], (b"\x01\x02\x03\x05", desc, meta)) == "differs (text)"                                 # not disassembled: no claim
    # the disassembly is read per function symbol, mnemonics only
    txt = "\nDisassembly of section .text:\n\n0000000000001700 <k>:\n\ts_load_dword s3, s[0:1], 0x4      // 000000001700: C00200C0\n\ts_endpgm\n\n0000000000001800 <f>:\n\tv_mov_b32_e32 v0, v1\n"
    assert kd.mnemonics_of(txt) == {"k": ["s_load_dword", "s_endpgm"], "f": ["v_mov_b32_e32"]}


def _dynsyms(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if l.split() and "__hip_cuid_" not in l)


def test_variant_library_is_whole(table):
    import kernel_diff as kd

    hipcc, tab = table
    objs = [os.path.join(CSRC, o) for o in tab if "_one_" not in o]
    lib = os.path.join(conftest.PKG, "crx", "libcrx.so")
    if not (os.path.exists(hipcc) and all(os.path.exists(o) for o in objs) and os.path.exists(lib)):
        pytest.skip("hipcc or the in-tree objects are absent: no variant can be linked here")
    if not (os.path.exists(kd.OBJDUMP) and os.path.exists(kd.READELF) and shutil.which("nm")):
        pytest.skip("binutils missing: the variant's kernels and symbols cannot be read here")
    watched = objs + [os.path.join(CSRC, ".flags")]
    before = {f: os.stat(f).st_mtime_ns for f in watched}
    name = "recipe_test_%d" % os.getpid()
    vlib = os.path.join(TOOLS, "ab", "libcrx_%s.so" % name)
    try:
        # the cheapest unit, with a macro nothing reads
        r = subprocess.run(["bash", os.path.join(TOOLS, "build_variant.sh"), name, "-DCRX_A_MACRO_NOTHING_READS=1", "crx_lqr.hip"], capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0 and os.path.exists(vlib), r.stdout[-2000:] + r.stderr[-2000:]
        assert os.path.exists(os.path.join(TOOLS, "ab", name, "crx_lqr.o"))
        # an absent unit is an undefined symbol here (a fresh process: this one may hold the in-tree library already)
        ld = subprocess.run([sys.executable, "-c", "import ctypes, sys; ctypes.CDLL(sys.argv[1])", vlib], capture_output=True, text=True, timeout=120)
        assert ld.returncode == 0, ld.stderr[-2000:]
        assert _dynsyms(vlib) == _dynsyms(lib)
        old, new = kd.kernels(lib), kd.kernels(vlib)
        assert sorted(old) == sorted(new) and len(new) >= 100, sorted(set(old) ^ set(new))
        verdicts = {n: kd.verdict_of(old[n], new[n]) for n in old}
        assert all(v in ("same", "moved") for v in verdicts.values()), {n: v for n, v in verdicts.items() if v not in ("same", "moved")}
        assert {f: os.stat(f).st_mtime_ns for f in watched} == before
    finally:
        shutil.rmtree(os.path.join(TOOLS, "ab", name), ignore_errors=True)
        if os.path.exists(vlib):
            os.remove(vlib)
