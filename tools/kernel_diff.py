"""Are the GPU kernels of two builds the same bits?  Needs no GPU.

    python tools/kernel_diff.py [--allow-renamed] OLD NEW          (two libcrx.so, or two .o of the same translation unit)

Every gfx950 code object embedded in the two files is extracted (exec_prologue_check.code_objects) and read as an ELF file.  One line per kernel
(a function symbol NAME with a kernel descriptor NAME.kd):
    same      identical .text bytes, identical 64-byte kernel descriptor, identical metadata entry (VGPR / AGPR / SGPR counts, LDS and
              scratch sizes, arguments) -- whatever its position inside the code object or the order of the code objects
    moved     as `same`, but for the descriptor's entry-offset field (bytes 16..23: the distance from the descriptor to the entry point) -- the
              kernel sits elsewhere in its code object, or in another one.  Not a difference
    renamed   the .text bytes differ, but the disassembly has the same number of instructions with the same mnemonic at every position (operands
              are not compared: other register names, the other side of a move pair), and descriptor (but for the entry offset, as in `moved`)
              and metadata entry are equal: what restating a pass in the source leaves behind when registers, scratch, LDS and the instruction
              stream stay what they were.  Bits on the GPU can still change; the bit-for-bit tests decide that
    differs   names which of text / kd / meta differ
    missing   in one of the two files only
Exit status 0 when every kernel is `same` or `moved` (with --allow-renamed: or `renamed`), 1 otherwise, 2 when the ROCm binutils are absent.
"""
import os
import shutil
import struct
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from exec_prologue_check import OBJDUMP, code_objects, demangle  # noqa: E402

READELF = os.path.join(os.path.dirname(OBJDUMP), "llvm-readelf")


def elf_kernels(path):
    """-> {kernel symbol: (text bytes, descriptor bytes)} of one ELF64 little-endian code object"""
    d = open(path, "rb").read()
    shoff, = struct.unpack_from("<Q", d, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", d, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", d, shoff + i * shentsize) for i in range(shnum)]   # name, type, flags, addr, offset, size, link, info, ..

    def body(shndx, value, size):
        _, typ, _, addr, off, _, _, _, _, _ = sec[shndx]
        return b"" if typ == 8 else d[off + value - addr: off + value - addr + size]   # (8 = SHT_NOBITS)

    syms = {}
    for (_, typ, _, _, off, size, link, _, _, entsize) in sec:
        if typ != 2:   # SHT_SYMTAB
            continue
        stroff = sec[link][4]
        for o in range(off, off + size, entsize):
            name, info, _, shndx, value, ssize = struct.unpack_from("<IBBHQQ", d, o)
            if 0 < shndx < shnum:
                syms[d[stroff + name: d.index(b"\0", stroff + name)].decode()] = (info & 15, shndx, value, ssize)
    return {n: (body(*syms[n][1:]), body(*syms[n + ".kd"][1:])) for n in syms if syms[n][0] == 2 and n + ".kd" in syms}   # (2 = STT_FUNC)


def metadata(path):
    """-> {kernel symbol: the lines of its entry in the amdhsa.kernels note, sorted}"""
    txt = subprocess.run([READELF, "--notes", path], capture_output=True, text=True, check=True).stdout
    out, cur, inside = {}, None, False
    for l in txt.split("\n"):
        if l.startswith("amdhsa.kernels:"):
            inside = True
        elif inside and l[:1] not in (" ", ""):
            inside = False
        elif inside and l.startswith("  - "):
            cur = []
            l = "    " + l[4:]
        if inside and cur is not None and l.startswith("    "):
            cur.append(l.strip())
            if l.strip().startswith(".symbol:"):
                out[l.split(":", 1)[1].strip().strip("'\"")[:-3]] = cur   # ('NAME.kd')
    return {k: sorted(v) for k, v in out.items()}


def mnemonics(path):
    """-> {function symbol: the mnemonics of its instructions, in order} of one code object"""
    return mnemonics_of(subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", path], capture_output=True, text=True, check=True).stdout)


def mnemonics_of(txt):
    """The same, on `llvm-objdump -d --no-show-raw-insn` text."""
    out, cur = {}, None
    for l in txt.split("\n"):
        if l.endswith(">:") and " <" in l:
            cur = out.setdefault(l[l.index(" <") + 2:-2], [])
        elif cur is not None and l[:1] in ("\t", " ") and l.strip():
            cur.append(l.split()[0])
    return out


def verdict_of(old, new):
    """(text, kd, meta[, mnemonics]) of one kernel in the two builds -> `same`, `moved`, `renamed` or `differs (..)`"""
    what = [w for w, a, b in zip(("text", "kd", "meta"), old, new) if a != b or a is None]
    kd_moved = len(old[1]) == len(new[1]) == 64 and old[1][:16] + old[1][24:] == new[1][:16] + new[1][24:]   # KERNEL_CODE_ENTRY_BYTE_OFFSET alone
    if what == ["kd"] and kd_moved:
        return "moved"
    if what in (["text"], ["text", "kd"]) and kd_moved and len(old) > 3 and old[3] and old[3] == new[3]:
        return "renamed"
    return "differs (%s)" % ", ".join(what) if what else "same"


def kernels(path, asm=False):
    tmp = tempfile.mkdtemp(prefix="crx_kd_")
    try:
        res = {}
        for co in code_objects(path, tmp):
            meta = metadata(co)
            mn = mnemonics(co) if asm else {}
            for n, (text, kd) in elf_kernels(co).items():
                res[n] = (text, kd, meta.get(n), mn.get(n))
        return res
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main(argv):
    allow = "--allow-renamed" in argv
    argv = [a for a in argv if a != "--allow-renamed"]
    if len(argv) != 2:
        print(__doc__)
        return 2
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        print("kernel_diff: %s / llvm-readelf not found -- nothing compared" % OBJDUMP)
        return 2
    old, new = kernels(argv[0]), kernels(argv[1])
    if any(n in new and old[n][0] != new[n][0] and old[n][2] == new[n][2] for n in old):   # a candidate for `renamed`: disassemble as well
        old, new = kernels(argv[0], asm=True), kernels(argv[1], asm=True)
    bad = 0
    for n in sorted(set(old) | set(new)):
        if n not in old or n not in new:
            verdict = "missing in " + (argv[0] if n not in old else argv[1])
        else:
            verdict = verdict_of(old[n], new[n])
        bad += verdict not in (("same", "moved", "renamed") if allow else ("same", "moved"))
        print("%-8s %s  [%d B]" % (verdict, demangle(n), len((new.get(n) or old[n])[0])))
    print("kernel_diff: %d kernel(s), %d not the same" % (len(set(old) | set(new)), bad))
    return 1 if bad or not old else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
