"""The build recipe of libcrx as the Makefile states it: `make recipe` prints, per object, the source and the exact compile flags.  Every tool
that recompiles a unit reads them here, so that none keeps a copy.
    python tools/recipe.py            prints the table"""
import os
import subprocess

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CSRC = os.path.join(ROOT, "car-racing_amd", "csrc")


def recipe(*make_args):
    """-> (hipcc, {object: (source, [flags])}), sources relative to car-racing_amd/csrc; make_args e.g. "EXTRA=-DCRX_PHASE_CLOCKS" """
    out = subprocess.run(["make", "-s", "--no-print-directory", "-C", CSRC, "recipe"] + list(make_args), capture_output=True, text=True, check=True).stdout
    hipcc, table = None, {}
    for line in out.splitlines():
        w = line.split()
        if w and w[0] == "HIPCC":
            hipcc = w[1]
        elif len(w) >= 2 and w[0].endswith(".o"):
            table[w[0]] = (w[1], w[2:])
    return hipcc, table


def command(obj, extra=(), *make_args):
    """-> the hipcc command line that compiles `obj` as the library's build does, without -c / -o: [hipcc, flags.., extra.., source path]"""
    hipcc, table = recipe(*make_args)
    src, flags = table[obj]
    return [hipcc] + flags + list(extra) + [os.path.join(CSRC, src)]


if __name__ == "__main__":
    hipcc, table = recipe()
    print("HIPCC", hipcc)
    for obj, (src, flags) in table.items():
        print("%-28s %-30s %s" % (obj, src, " ".join(flags)))
