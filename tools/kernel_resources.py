"""Registers, scratch and occupancy of the solver kernels, from the compiler's own remarks (no GPU needed):
    python tools/kernel_resources.py [obs|plan|gen|spec|lmpc|models_plan|models_obs|models_gen|prep|plant|game|order|path|pathplan] [flags]   (recompiles the unit as `make recipe` states it, with
                                                       -Rpass-analysis=kernel-resource-usage)
    python tools/kernel_resources.py one NOBS NMAX DEG NFIX [flags]     ONE instantiation compiled alone (csrc/crx_kernels_one.hip)
    python tools/kernel_resources.py lib [FILE.so]     what SHIPS: the kernel metadata of every code object embedded in the library (default: the in-tree
                                                       libcrx.so), no recompilation -- shipped() below, which tests/test_kernel_budget_cpu.py asserts on"""
import os, re, subprocess, sys, tempfile
ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
S = os.path.join(ROOT, "car-racing_amd", "csrc")
READELF = os.environ.get("LLVM_READELF", "/opt/rocm/lib/llvm/bin/llvm-readelf")
def demangle(n):   # crx_solve_kernel<NOBS, NMAX, DEG, NFIX, ..>: _Z16crx_solve_kernelILi1ELi12ELi6ELi12ELi0ELi0EEv11crx_kparams
    m = re.match(r"_Z\d+([a-z_]+)I((?:Li\d+E|Lb[01]E)+)E", n)
    return "%s<%s>" % (m.group(1), ",".join(re.findall(r"L[ib](\d+)E", m.group(2)))) if m else n
def shipped(lib=None):
    """{mangled kernel name: {vgpr, agpr, sgpr, sgpr_spill, vgpr_spill, scratch (B/lane), lds (B)}} of every kernel embedded in the library, from the
    metadata notes of its code objects (extracted as tools/exec_prologue_check.py extracts them)."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import exec_prologue_check as epc
    lib = lib or os.path.join(ROOT, "car-racing_amd", "crx", "libcrx.so")
    keys = {"vgpr_count": "vgpr", "agpr_count": "agpr", "sgpr_count": "sgpr", "sgpr_spill_count": "sgpr_spill", "vgpr_spill_count": "vgpr_spill",
            "private_segment_fixed_size": "scratch", "group_segment_fixed_size": "lds"}
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in epc.code_objects(lib, tmp):
            notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True, check=True).stdout
            for blk in re.split(r"\n\s+- \.", notes):   # one list entry of amdhsa.kernels per kernel
                name = re.search(r"\.name:\s+(\S+)", blk)
                if not name or ".vgpr_count" not in blk:
                    continue
                out[name.group(1)] = {v: int(m.group(1)) for k, v in keys.items() if (m := re.search(r"\." + k + r":\s+(\d+)", blk))}
    return out
which = sys.argv[1] if len(sys.argv) > 1 else "obs"
if __name__ != "__main__":
    which = None
elif which == "lib":
    for n, r in sorted(shipped(sys.argv[2] if len(sys.argv) > 2 else None).items(), key=lambda kv: demangle(kv[0])):
        print("%-52s vgpr %3d agpr %3d sgpr spills %3d scratch %4d B/lane  LDS %6d B" % (demangle(n) + (" [models]" if "models" in n else ""), r["vgpr"], r.get("agpr", 0),
              r["sgpr_spill"], r["scratch"], r["lds"]))
    sys.exit(0)
# unit name -> its object in the Makefile's recipe (tools/recipe.py: source and flags are read from `make recipe`, none is kept here)
UNITS = {"plan": "crx_kernels.o", "obs": "crx_kernels_obs.o", "gen": "crx_kernels_gen.o", "spec": "crx_kernels_spec.o", "models_plan": "crx_kernels_models_plan.o",
         "models_obs": "crx_kernels_models_obs.o", "models_gen": "crx_kernels_models_gen.o", "lmpc": "crx_lmpc.o", "prep": "crx_prep.o",
         "plant": "crx_plant.o", "game": "crx_game.o", "order": "crx_order.o", "path": "crx_path.o", "pathplan": "crx_pathplan.o"}
def unit_command(which, args):
    """-> the compile command of a unit name (UNITS, or `one NOBS NMAX DEG NFIX`: crx_kernels_one.hip as the unit that ships the instantiation is built)"""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import recipe
    if which == "one":
        return recipe.command("crx_kernels_one_obs.o" if args[0] != "0" else "crx_kernels_one_plan.o", ["-DCRX_PROBE_ONE=" + ",".join(args[:4])] + args[4:])
    return recipe.command(UNITS[which], args)
def recompile():
    cmd = unit_command(which, sys.argv[2:])
    cmd = cmd[:-1] + ["-Rpass-analysis=kernel-resource-usage", "-c", cmd[-1], "-o", "/dev/null"]
    t = subprocess.run(cmd, capture_output=True, text=True).stderr
    for b in re.split(r"remark: [^\n]*Function Name: ", t)[1:]:
        g = lambda k: (re.search(k + r": (\d+)", b) or [0, "?"])[1]
        print("%-44s vgpr %3s agpr %3s sgpr %3s scratch %4s B/lane  waves/SIMD %s" % (demangle(b.split("\n")[0].split(" [")[0]), g("VGPRs"), g("AGPRs"), g("SGPRs"),
              g(r"ScratchSize \[bytes/lane\]"), g(r"Occupancy \[waves/SIMD\]")))
if __name__ == "__main__":
    recompile()
